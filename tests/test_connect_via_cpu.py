"""
Goal chains through waypoints (Planner.connect_via) on the CPU: the reference of the rule (tests/connect_via_reference.py, composed
from connect_reference.Connector and so from the C oracle's one steer) pinned to winners worked out on committed fixtures, the host
side of the public methods, and what the compiler says about the two kernels.  The device is compared with the same reference bit
for bit in tests/test_connect_via_gpu.py.
"""
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

ROWS, row_inputs = cvr.ROWS, cvr.row_inputs


@pytest.mark.parametrize("name,size,way_ids,tries,connect,winner,lens", ROWS)
def test_reference_is_pinned_to_worked_rows(name, size, way_ids, tries, connect, winner, lens):
    s, g, r, way = row_inputs(name, size, way_ids)
    got = r.search(goal_tries=tries)
    assert (None if got is None else (got[0], got[1])) == connect
    win = r.search_via(way, goal_tries=tries)
    found = [len(e[0]) for e in win[3]]
    print(name, size, len(way), tries, win[:3], found)
    assert win[:3] == winner
    if isinstance(lens, int):
        assert len(found) == lens and 1 in found and 16 in found and sum(1 for v in found if v < 20) == 2
    else:
        assert found == lens
    if connect is not None:
        assert winner[0] <= connect[0]
    size0 = r.size
    plan, ids = r.commit_via(win)
    assert ids == list(range(size0, size0 + len(found))) and plan == r.climb(winner[1]) + ids
    assert r.cost(plan) == winner[0] and r.in_goal(r.states[plan[-1]])


def test_reference_without_waypoints_is_the_goal_connection():
    s, g = cr.case("car_2000")
    r = cvr.from_fixture(s, g, 217)
    a, b = r.search(), r.search_via(np.zeros((0, s.nstates)))
    assert (a[0], a[1], 0) == b[:3] == (951, 211, 0)
    assert all(np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1]) and np.array_equal(p[2], q[2]) for p, q in zip(a[2], b[3]))
    assert r.search_via([], incumbent=951) is None and r.search_via([], incumbent=952)[:3] == (951, 211, 0)


def test_reference_winner_is_independent_of_the_order():
    s, g, r, way = row_inputs("car_500", 217, [217])
    ids = np.random.RandomState(5).permutation(217).tolist()
    wins = [r.search_via(way, goal_tries=1, nodes=k)[:3] for k in (ids, sorted(ids), ids[::-1])]
    assert wins == [(1050, 213, 0)] * 3


def _native_planner():
    car = lqrrt_amd.systems.Car(0)
    cons = lqrrt_amd.Constraints(car.nstates, car.ncontrols, car.goal_buffer, car.is_feasible)
    return lqrrt_amd.Planner(car.dynamics, car.lqr, cons, error_tol=car.error_tol, erf=car.erf, goal0=car.goal, printing=False,
                             **car.plan_kwargs)


def test_connect_via_without_a_plan_changes_nothing():
    p = _native_planner()
    way = np.zeros((2, p.nstates))
    assert p.connect_via(way) is False
    assert p.connect_via([], goal_tries=2, nodes=[0], finish_on_goal=True) is False
    assert p.tree is None and not hasattr(p, "node_seq") and not p.plan_reached_goal
    assert p.plan_waypoints().shape == (0, p.nstates)
    with pytest.raises(ValueError):
        p.connect_via(way, goal_tries=0)
    with pytest.raises(ValueError):
        p.connect_via(np.zeros((2, p.nstates + 1)))
    with pytest.raises(ValueError):
        p.connect_via(np.zeros(p.nstates))


def test_connect_via_refuses_callback_mode():
    cons = lqrrt_amd.Constraints(2, 1, [0.1, 0.1], lambda x, u: True)
    p = lqrrt_amd.Planner(lambda x, u, dt: x + dt * np.array([x[1], u[0]]), lambda x, u: (np.eye(2), np.array([[1.0, 1.0]])), cons,
                          horizon=1, dt=0.1, goal0=[1.0, 0.0], printing=False)
    assert p.callback_mode
    with pytest.raises(NotImplementedError, match="Python"):
        p.connect_via(np.zeros((1, 2)))


def test_connect_via_shares_the_connection_steps():
    src = open(os.path.join(ROOT, "lqrrt_amd", "planner.py")).read()
    body = src[src.index("    def connect_via(self"):src.index("    def plan_waypoints(self")]
    for name in ("_connect_begin(", "_connect_incumbent(", "_connect_accept("):
        assert name in body, name
    assert "_drop_host_tail" not in body and "_adopt_plan" not in body


def test_abi_declares_the_two_calls_and_keeps_its_version():
    hdr = open(os.path.join(ROOT, "include", "lqrrt_hip.h")).read()
    assert "int lqrrt_connect_via_search(" in hdr and "int lqrrt_connect_via_commit(" in hdr
    from lqrrt_amd import _native as nat
    assert nat.lib().lqrrt_abi_version() == 1
    assert nat.lib().lqrrt_connect_via_search is not None and nat.lib().lqrrt_connect_via_commit is not None


def test_via_kernels_keep_the_refinements_frame():
    """For every model S, none excepted: k_connect_via_search<S> has a private segment no larger and an occupancy no lower than
    k_refine_search<S> -- its nearest relative, whose targets also vary -- and k_connect_via_commit<S> no more than k_refine_commit<S>."""
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
        refine, via = by_model("k_refine_%s" % stage), by_model("k_connect_via_%s" % stage)
        assert len(refine) >= 10 and "UserSystem" in refine, sorted(refine)
        assert sorted(via) == sorted(refine)
        for model in refine:
            print("%-7s %-18s refine %4d B occ %d vgpr %3d agpr %3d   via %4d B occ %d vgpr %3d agpr %3d" % (
                stage, model, refine[model]["scratch"], refine[model]["occupancy"], refine[model]["vgpr"], refine[model]["agpr"],
                via[model]["scratch"], via[model]["occupancy"], via[model]["vgpr"], via[model]["agpr"]))
        worse = {m: (refine[m]["scratch"], via[m]["scratch"], refine[m]["occupancy"], via[m]["occupancy"]) for m in refine
                 if via[m]["scratch"] > refine[m]["scratch"] or via[m]["occupancy"] < refine[m]["occupancy"]}
        assert not worse, (stage, worse)


def test_via_stays_plain_launches_built_from_the_refinements_pieces():
    for f in ("connect_via.hpp", "engine_connect_via.hpp"):
        text = open(os.path.join(ROOT, "lqrrt_amd", "csrc", f)).read()
        for word in ("hipLaunchCooperativeKernel", "hipModuleLaunchCooperativeKernel", "cooperative_groups", "grid.sync", "this_grid"):
            assert word not in text, (f, word)
    src = open(os.path.join(ROOT, "lqrrt_amd", "csrc", "connect_via.hpp")).read()
    for name in ("refine_start<S>(", "refine_edge<S>(", "refine_in_goal<S>(", "refine_best(", "stage_geo(", "GainLds<S>", "launch_constant(",
                 "refine_write_node<S>(", "connect_via_search_body"):
        assert name in src, name
    assert src.count("__launch_bounds__(64)") == 2 and "S::step(" not in src
