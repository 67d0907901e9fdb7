"""
Fleet goal chains through waypoints (lqrrt_amd.connect_vias, k_connect_via_search_multi / k_connect_via_commit_multi) on the CPU:
further rows of the rule's reference (tests/connect_via_reference.py) pinned to winners worked out on committed fixtures, the host
side of the public function, and what the compiler says about the two kernels whose grids span several engines.  The device side is
compared bit for bit in tests/test_connect_vias_gpu.py and tests/test_fleet_connect_via_gpu.py.
"""
import functools
import os
import re
import shutil
import sys

import numpy as np
import pytest

import lqrrt_amd
import connect_reference as cr
import connect_via_reference as cvr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Fixtures cut at or below their first goal node, the waypoints the fixture plan's nodes from that node on: fixture -> (first goal
# node, number of waypoints).
BEYOND = {"double_integrator_600": (5, 15), "boat_novice_lqr_400": (144, 6)}

# fixture, nodes kept, with the waypoints (True) or without (False: Q = 0), goal tries, winner (cost, v, j) or None, the winner's
# edge lengths (None: not pinned).  The table is the reference's: a reference that drifts fails here.
NEW_ROWS = [("double_integrator_600", 1, True, 1, (41, 0, 13), [20, 20]),
            # connect_goal's own candidate (j = Q = 15) reaches the goal at cost 41 too: the tie goes to the smaller j
            ("double_integrator_600", 1, True, 8, (41, 0, 13), None),
            ("double_integrator_600", 1, False, 1, None, None),
            ("double_integrator_600", 5, False, 1, (81, 3, 0), None),
            ("double_integrator_600", 5, True, 1, (41, 0, 13), None),
            ("boat_novice_lqr_400", 144, True, 1, (529, 142, 6), None),
            ("boat_novice_lqr_400", 144, True, 8, (461, 16, 0), [20] * 14)]


@functools.lru_cache(maxsize=None)
def case(name):
    return cr.case(name)


@functools.lru_cache(maxsize=None)
def beyond(name):
    """The waypoints of a BEYOND fixture (read-only)."""
    s, g = case(name)
    first, count = BEYOND[name]
    assert cr.first_goal_node(s, g) == first
    ids, way = cvr.plan_states(g, first)
    assert len(ids) == count and ids[-1] == int(g["node_seq"][-1])
    way.setflags(write=False)
    return way


def row_way(name, with_way):
    s, _ = case(name)
    return beyond(name) if with_way else np.zeros((0, s.nstates))


@functools.lru_cache(maxsize=None)
def ref_win(name, size, with_way, tries, incumbent=cvr.NO_INCUMBENT, nodes=None):
    """The reference's winner (cost, v, j, edges) or None; computed once per case and left unchanged."""
    s, g = case(name)
    return cvr.from_fixture(s, g, size).search_via(row_way(name, with_way), goal_tries=tries, incumbent=incumbent,
                                                   nodes=None if nodes is None else list(nodes))


@pytest.mark.parametrize("name,size,with_way,tries,winner,lens", NEW_ROWS)
def test_reference_is_pinned_to_the_new_rows(name, size, with_way, tries, winner, lens):
    win = ref_win(name, size, with_way, tries)
    found = None if win is None else [len(e[0]) for e in win[3]]
    print(name, size, len(row_way(name, with_way)), tries, None if win is None else win[:3], found)
    assert (None if win is None else win[:3]) == winner
    if lens is not None:
        assert found == lens


def test_the_tie_with_connect_goals_own_candidate_goes_to_the_smaller_j():
    s, g = case("double_integrator_600")
    r = cvr.from_fixture(s, g, 1)
    way = beyond("double_integrator_600")
    own = r.chain_via(0, len(way), way, 8)
    assert own is not None and own[0] == 41                        # j = Q = 15: connect_goal's candidate, at the winner's cost
    assert ref_win("double_integrator_600", 1, True, 8)[:3] == (41, 0, 13)


def test_car_chains_that_miss_the_goal():
    s, g, r, way = cvr.row_inputs("car_500", 217, [217])
    for v, j in ((213, 1), (0, 0), (216, 0)):
        assert r.chain_via(v, j, way, 1) is None, (v, j)
    assert r.chain_via(213, 0, way, 1)[0] == 1050


def _native_planner():
    car = lqrrt_amd.systems.Car(0)
    cons = lqrrt_amd.Constraints(car.nstates, car.ncontrols, car.goal_buffer, car.is_feasible)
    return lqrrt_amd.Planner(car.dynamics, car.lqr, cons, error_tol=car.error_tol, erf=car.erf, goal0=car.goal, printing=False,
                             **car.plan_kwargs)


def _callback_planner():
    cons = lqrrt_amd.Constraints(2, 1, [0.1, 0.1], lambda x, u: True)
    return lqrrt_amd.Planner(lambda x, u, dt: x + dt * np.array([x[1], u[0]]), lambda x, u: (np.eye(2), np.array([[1.0, 1.0]])), cons,
                             horizon=1, dt=0.1, goal0=[1.0, 0.0], printing=False)


def test_connect_vias_of_nobody():
    assert lqrrt_amd.connect_vias([], []) == []
    import lqrrt
    assert lqrrt.connect_vias is lqrrt_amd.connect_vias
    assert "connect_vias" in lqrrt_amd.__all__ and "connect_vias" in lqrrt.__all__


def test_connect_vias_without_plans_changes_nothing():
    a, b = _native_planner(), _native_planner()
    way = np.zeros((2, a.nstates))
    assert lqrrt_amd.connect_vias([a, b], [way, None]) == [False, False]       # no tree on the device: no native call, no engine
    assert lqrrt_amd.connect_vias([a], [[]], goal_tries=2, nodes=[[0]], finish_on_goal=True) == [False]
    assert lqrrt_amd.connect_vias([a, b], [None, way], nodes=[None, [0, 1]]) == [False, False]
    for p in (a, b):
        assert p.tree is None and not hasattr(p, "node_seq") and not p.plan_reached_goal
        assert getattr(p, "_engine", None) is None


def test_connect_vias_refuses_before_touching_anybody():
    a, b = _native_planner(), _native_planner()
    way = np.zeros((2, a.nstates))
    with pytest.raises(ValueError, match="twice"):
        lqrrt_amd.connect_vias([a, b, a], [way] * 3)
    cb = _callback_planner()
    assert cb.callback_mode
    with pytest.raises(ValueError, match="Python"):
        lqrrt_amd.connect_vias([a, cb], [way, None])
    with pytest.raises(ValueError, match="Planner"):
        lqrrt_amd.connect_vias([a, object()], [way, None])
    with pytest.raises(ValueError, match="goal_tries"):
        lqrrt_amd.connect_vias([a, b], [way, way], goal_tries=0)
    with pytest.raises(ValueError, match="per planner"):
        lqrrt_amd.connect_vias([a, b], [way, way], nodes=[None])
    with pytest.raises(ValueError, match="per planner"):
        lqrrt_amd.connect_vias([a, b], [way])                       # a waypoints sequence of the wrong length
    with pytest.raises(ValueError, match="per planner"):
        lqrrt_amd.connect_vias([], [way])
    with pytest.raises(ValueError, match="shape"):
        lqrrt_amd.connect_vias([a, b], [way, np.zeros((2, a.nstates + 1))])
    with pytest.raises(ValueError, match="shape"):
        lqrrt_amd.connect_vias([a, b], [np.zeros(a.nstates), way])  # one state, not a table
    with pytest.raises(ValueError, match="shape"):
        lqrrt_amd.connect_vias([a, b], [way, np.zeros((1, 2, a.nstates))])
    for p in (a, b):
        assert p.tree is None and not hasattr(p, "node_seq")
        assert getattr(p, "_engine", None) is None


def test_connect_vias_shares_the_connection_steps_and_calls_the_batched_pair():
    src = open(os.path.join(ROOT, "lqrrt_amd", "planner.py")).read()
    fleet = src[src.index("def connect_vias("):src.index("def connect_goals(")]
    assert "Engine.connect_via_search_multi(" in fleet and "Engine.connect_via_commit_multi(" in fleet
    assert ".connect_via_search(" not in fleet and ".connect_via_commit(" not in fleet
    for name in ("_connect_begin(", "_connect_incumbent(", "_connect_accept("):
        assert name in fleet, name
    eng = open(os.path.join(ROOT, "lqrrt_amd", "engine.py")).read()
    for method in ("connect_via_search_multi", "connect_via_commit_multi"):
        body = eng[eng.index("    def %s(" % method):]
        body = body[:body.index("\n    def ", 10)]
        assert "_connect_multi_args(" in body and "_waypoints" in body, method
    assert callable(lqrrt_amd.engine.Engine.connect_via_search_multi) and callable(lqrrt_amd.engine.Engine.connect_via_commit_multi)


def test_fleet_via_stays_plain_launches_that_wrap_the_solo_bodies():
    for f in ("connect_via_multi.hpp", "engine_connect_via_multi.hpp", "engine_connect_via.hpp", "engine_connect.hpp", "engine_refine.hpp"):
        text = open(os.path.join(ROOT, "lqrrt_amd", "csrc", f)).read()
        for word in ("hipLaunchCooperativeKernel", "hipModuleLaunchCooperativeKernel", "cooperative_groups", "grid.sync", "this_grid"):
            assert word not in text, (f, word)
    src = open(os.path.join(ROOT, "lqrrt_amd", "csrc", "connect_via_multi.hpp")).read()
    assert "connect_via_search_body<S>(" in src and "connect_via_commit_body<S>(" in src
    assert "refine_edge<S>(" not in src and "S::step(" not in src
    assert "multi_engine_of" in src and "struct ConnectViaDesc" in src and src.count("launch_constant(") >= 4
    assert src.count("__launch_bounds__(64)") == 2
    kernels = open(os.path.join(ROOT, "lqrrt_amd", "csrc", "kernels.hpp")).read()
    assert kernels.index('#include "connect_via.hpp"') < kernels.index('#include "connect_via_multi.hpp"')
    engine = open(os.path.join(ROOT, "lqrrt_amd", "csrc", "engine.hip")).read()
    assert engine.index('#include "engine_connect_via.hpp"') < engine.index('#include "engine_connect_via_multi.hpp"')
    host = open(os.path.join(ROOT, "lqrrt_amd", "csrc", "engine_connect_via_multi.hpp")).read()
    # the shared checks, depth functions and the two runners rather than copies: connect_via_winner_check stands for range_ok and
    # connect_depth_of; the runners (engine_refine.hpp) for the chunks, the scratch, refine_multi_protos for multi_sync_proto,
    # multi_grid for retain_grid, the keys' read-back and multi_commit_adopt for refine_adopt; a failed call drains the stream
    # (StreamDrain: one in each runner, armed before the runner's only upload)
    for name in ("connect_multi_check(", "connect_via_check(", "connect_depths(", "connect_via_winner_check(", "connect_via_candidates_check(",
                 "connect_via_deepest_check(", "incumbent_check(", "multi_id_list(", "multi_search_run(", "multi_commit_run(",
                 "connect_via_fill_args(", "connect_via_decode("):
        assert name in host, name
    refine = open(os.path.join(ROOT, "lqrrt_amd", "csrc", "engine_refine.hpp")).read()
    search = refine[refine.index("static int multi_search_run("):refine.index("static int multi_commit_run(")]
    commit = refine[refine.index("static int multi_commit_run("):refine.index("static int refine_multi_check(")]
    for name in ("multi_chunks(", "refine_multi_scratch(", "refine_multi_protos(", "multi_grid(", "keys_of("):
        assert name in search, name
    for name in ("multi_chunks(", "multi_commit_head(", "refine_multi_scratch(", "refine_multi_protos(", "multi_commit_adopt("):
        assert name in commit, name
    for f in ("engine_connect_via_multi.hpp", "engine_reach_multi.hpp", "engine_connect.hpp"):
        text = open(os.path.join(ROOT, "lqrrt_amd", "csrc", f)).read()
        multi = text[text.index("static int connect_multi_check("):] if f == "engine_connect.hpp" else text   # (its solo calls guard their own images)
        assert "StreamDrain drain(st)" not in multi and "drain.arm();" not in multi, f
    for run in (search, commit):                                    # the search and the commit
        assert run.count("StreamDrain drain(st)") == 1 and run.count("drain.arm();") == 1
        assert run.count("hipMemcpyHostToDevice") == 1
        assert run.index("StreamDrain drain(st)") < run.index("drain.arm();") < run.index("hipMemcpyAsync(")
    assert "dalloc(" not in host and "hipMalloc" not in host       # no buffer of its own
    for copied in ("range_ok(", "connect_depth_of(", "multi_sync_proto(", "retain_grid(", "refine_adopt(", "0x7fffffff", "0xffffffff", "g_err"):
        assert copied not in host, copied
    shared = {"engine_connect_via.hpp": ("range_ok(", "connect_winner_check("), "engine_connect.hpp": ("connect_depth_of(", "range_ok("),
              "engine_refine.hpp": ("multi_sync_proto(", "retain_grid(", "refine_adopt(", "struct StreamDrain", "g_err = keep;")}
    for f, names in shared.items():
        text = open(os.path.join(ROOT, "lqrrt_amd", "csrc", f)).read()
        for name in names:
            assert name in text, (f, name)


def test_abi_declares_the_two_calls_and_keeps_its_version():
    hdr = open(os.path.join(ROOT, "include", "lqrrt_hip.h")).read()
    assert "int lqrrt_connect_via_search_multi(" in hdr and "int lqrrt_connect_via_commit_multi(" in hdr
    from lqrrt_amd import _native as nat
    assert "lqrrt_connect_via_search_multi" in nat.SIGNATURES and "lqrrt_connect_via_commit_multi" in nat.SIGNATURES
    assert nat.lib().lqrrt_abi_version() == 1
    assert nat.lib().lqrrt_connect_via_search_multi is not None and nat.lib().lqrrt_connect_via_commit_multi is not None


def test_multi_via_kernels_keep_their_solo_twins_frame_and_occupancy():
    """For every model S, UserSystem included and none excepted: k_connect_via_search_multi<S> exists, its private segment is no
    larger than that of k_connect_via_search<S> and its occupancy no lower; the same for k_connect_via_commit_multi<S> against
    k_connect_via_commit<S>."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    assert shutil.which(kr.HIPCC) or os.path.exists(kr.HIPCC), "hipcc is what builds the package: it cannot be missing here"
    user = os.path.join(ROOT, "examples", "user_system", "unicycle.hpp")
    rows = kr.parse(kr.remarks(["-DLQRRT_USER_SYSTEM=\"%s\"" % user]))

    def by_model(kernel):
        out = {}
        for r in rows:
            m = re.match(r"void lq::%s<lq::(.+?) ?>\(" % kernel, r["name"])
            if m:
                out[m.group(1)] = r
        return out
    for stage in ("search", "commit"):
        solo, multi = by_model("k_connect_via_%s" % stage), by_model("k_connect_via_%s_multi" % stage)
        assert len(solo) >= 10 and "UserSystem" in solo, sorted(solo)
        assert sorted(multi) == sorted(solo)
        for model in solo:
            print("%-7s %-18s solo %4d B occ %d vgpr %3d agpr %3d   multi %4d B occ %d vgpr %3d agpr %3d" % (
                stage, model, solo[model]["scratch"], solo[model]["occupancy"], solo[model]["vgpr"], solo[model]["agpr"],
                multi[model]["scratch"], multi[model]["occupancy"], multi[model]["vgpr"], multi[model]["agpr"]))
        worse = {m: (solo[m]["scratch"], multi[m]["scratch"], solo[m]["occupancy"], multi[m]["occupancy"]) for m in solo
                 if multi[m]["scratch"] > solo[m]["scratch"] or multi[m]["occupancy"] < solo[m]["occupancy"]}
        assert not worse, (stage, worse)
