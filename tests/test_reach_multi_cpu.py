"""
Several trees asked about many goals per call (lqrrt_amd.fleet_goal_costs / lqrrt_amd.retargets, k_reach_search_multi /
k_reach_commit_multi) on the CPU: a table of multi-engine calls pinned with the C oracle and recomputed here from the reference of
the rule (tests/reach_reference.py, a connect_reference.Connector per target and tree), the host side of the two public functions,
the ABI's declarations, the shape of the new sources, and what the compiler says about the two kernels whose grids span several
engines.  The device is compared with the same table bit for bit in tests/test_reach_multi_gpu.py, the planners end to end in
tests/test_fleet_reach_gpu.py.
"""
import os
import re
import shutil
import sys

import numpy as np
import pytest

import lqrrt_amd
from lqrrt_amd import _native as nat
import connect_reference as cr
import reach_reference as rh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The pinned calls: per model ONE Engine.reach_search_multi over engines that each hold a prefix of the model's fixture tree.  An
# engine is (nodes kept, goal_tries, [(target, winner)]); a target is spelled as in reach_reference.PINNED -- ("own", scale),
# ("node", k): the state of fixture node k (k may lie beyond the prefix: it is a state, not an id), ("far",).  The first engine of
# the car's and of boat_novice's call is reach_reference.PINNED's own row.
PINNED_CALLS = {
    "car_2000": [
        (217, 8, rh.PINNED[("car_2000", 217)]),
        (150, 3, [(("own", 1.0), None)]),
        (400, 2, [(("own", 1.0), (951, 211)), (("node", 300), (1151, 215)), (("node", 350), (1951, 319))]),
        (150, 8, [(("node", 40), (351, 12)), (("node", 90), (551, 16))]),
    ],
    "boat_novice_300": [
        (107, 8, rh.PINNED[("boat_novice_300", 107)]),
        (60, 3, [(("node", 20), (81, 1))]),                         # (with eight tries it is the root: (81, 0), the next engine's row)
        (60, 8, [(("own", 1.0), None), (("node", 20), (81, 0)), (("node", 50), (401, 41)), (("node", 40), (281, 23)), (("far",), None)]),
    ],
    "double_integrator_600": [
        (1, 8, [(("own", 1.0), (41, 0)), (("node", 0), None), (("node", 3), None), (("node", 30), None), (("node", 45), (41, 0)),
                (("own", 0.25), (48, 0)), (("far",), (101, 0))]),
        (5, 2, [(("own", 0.25), (89, 3))]),
        (50, 2, [(("own", 1.0), (41, 0)), (("node", 30), (166, 9)), (("far",), None)]),
        (5, 8, [(("node", 0), (61, 1)), (("node", 3), (61, 2)), (("node", 30), None), (("own", 0.25), (48, 0))]),
    ],
}


def pinned_call(name):
    """(system, fixture, [(size, goal_tries, goals [T][n], buffers [T][n], [winner or None] * T)]) of a pinned call."""
    s, g = cr.case(name)
    out = []
    for size, tries, rows in PINNED_CALLS[name]:
        goals, bufs = rh.pinned_targets(s, g, rows)
        out.append((size, tries, goals, bufs, [w for _, w in rows]))
    return s, g, out


@pytest.mark.parametrize("name", sorted(PINNED_CALLS))
def test_reference_gives_the_pinned_calls(name):
    """Every engine's row is the reference's on that prefix with that engine's goal_tries, and the table has the shape that makes a
    wrong grid mapping show: winners and none, an engine with one target, neighbours that differ in T and in size."""
    s, g, engines = pinned_call(name)
    got = [rh.from_fixture(s, g, size).search(goals, bufs, goal_tries=tries) for size, tries, goals, bufs, _ in engines]
    print(name, got)
    assert got == [want for _, _, _, _, want in engines]
    flat = [w for row in got for w in row]
    assert 2 * sum(w is not None for w in flat) >= len(flat) and any(w is None for w in flat)
    assert any(len(want) == 1 for _, _, _, _, want in engines)
    assert any(a[0] != b[0] and len(a[4]) != len(b[4]) for a in engines for b in engines)


def _native_planner():
    car = lqrrt_amd.systems.Car(0)
    cons = lqrrt_amd.Constraints(car.nstates, car.ncontrols, car.goal_buffer, car.is_feasible)
    return car, lqrrt_amd.Planner(car.dynamics, car.lqr, cons, error_tol=car.error_tol, erf=car.erf, goal0=car.goal, printing=False,
                                  **car.plan_kwargs)


def _callback_planner():
    cons = lqrrt_amd.Constraints(2, 1, [0.1, 0.1], lambda x, u: True)
    return lqrrt_amd.Planner(lambda x, u, dt: x + dt * np.array([x[1], u[0]]), lambda x, u: (np.eye(2), np.array([[1.0, 1.0]])), cons,
                             horizon=1, dt=0.1, goal0=[1.0, 0.0], printing=False)


def test_both_names_are_exported():
    import lqrrt
    for name in ("fleet_goal_costs", "retargets"):
        assert name in lqrrt_amd.__all__ and name in lqrrt.__all__
        assert getattr(lqrrt, name) is getattr(lqrrt_amd, name)
    assert lqrrt_amd.retargets([], []) == []


def test_without_plans_nothing_happens():
    (car, a), (_, b) = _native_planner(), _native_planner()
    goal = np.array(car.goal, dtype=np.float64)
    goals = np.array([goal, goal + 1.0, goal + 2.0])
    for kw in (dict(), dict(goal_buffers=car.goal_buffer, goal_tries=2, nodes=[[0], None])):
        steps, nodes = lqrrt_amd.fleet_goal_costs([a, b], goals, **kw)
        for m in (steps, nodes):
            assert m.shape == (2, 3) and m.dtype == np.int64 and np.all(m == -1)
    assert lqrrt_amd.retargets([a, b], [goal + 1.0, None]) == [False, False]
    assert lqrrt_amd.retargets([a, b], [goal, goal + 1.0], goal_tries=2, nodes=[[0], None], finish_on_goal=True) == [False, False]
    for p in (a, b):                                                # no tree on the device: no native call, no engine
        assert p.tree is None and not hasattr(p, "node_seq") and not p.plan_reached_goal
        assert getattr(p, "_engine", None) is None and np.array_equal(p.goal, goal)


def test_refusals_before_touching_anybody():
    (car, a), (_, b) = _native_planner(), _native_planner()
    n = car.nstates
    goal = np.array(car.goal, dtype=np.float64)
    cb = _callback_planner()
    assert cb.callback_mode
    neg = -np.abs(np.asarray(car.goal_buffer, dtype=np.float64)) - 1.0
    for bad, match in ((dict(planners=[a, b, a], goals=[goal]), "twice"),
                       (dict(planners=[a, cb], goals=[goal]), "Python"),
                       (dict(planners=[a, object()], goals=[goal]), "Planner"),
                       (dict(planners=[a, b], goals=[goal], nodes=[None]), "per planner"),
                       (dict(planners=[a, b], goals=[goal], goal_tries=0), "goal_tries"),
                       (dict(planners=[a, b], goals=goal), "shape"),
                       (dict(planners=[a, b], goals=[goal[:-1]]), "states"),
                       (dict(planners=[a, b], goals=np.zeros((0, n))), "shape"),
                       (dict(planners=[a, b], goals=[goal], goal_buffers=np.ones(n + 1)), "goal_buffers"),
                       (dict(planners=[a, b], goals=[goal, goal], goal_buffers=np.ones((3, n))), "goal_buffers"),
                       (dict(planners=[a, b], goals=[goal], goal_buffers=neg), "negative")):
        with pytest.raises(ValueError, match=match):
            lqrrt_amd.fleet_goal_costs(**bad)
    for bad, match in ((dict(planners=[a, b, a], goals=[goal] * 3), "twice"),
                       (dict(planners=[a, cb], goals=[goal, [1.0, 0.0]]), "Python"),
                       (dict(planners=[a, object()], goals=[goal, goal]), "Planner"),
                       (dict(planners=[a, b], goals=[goal, goal], nodes=[None]), "per planner"),
                       (dict(planners=[a, b], goals=[goal]), "per planner"),
                       (dict(planners=[a, b], goals=[goal, goal], goal_tries=0), "goal_tries"),
                       (dict(planners=[a, b], goals=[goal, goal[:-1]]), "dimensionality"),
                       (dict(planners=[a, b], goals=[goal, [goal, goal]]), "dimensionality")):
        with pytest.raises(ValueError, match=match):
            lqrrt_amd.retargets(**bad)
    for p in (a, b):
        assert p.tree is None and not hasattr(p, "node_seq") and np.array_equal(p.goal, goal)


def test_retarget_and_retargets_share_their_steps():
    """retarget calls the instance's own reach_search / reach_commit, retargets the batched ones; both accept a winner with the same
    steps in the same order, and hand the grown goal to the goal connection."""
    src = open(os.path.join(ROOT, "lqrrt_amd", "planner.py")).read()
    solo = src[src.index("    def retarget(self"):src.index("# ------------------------------------------------------------------------------------------ setters")]
    fleet = src[src.index("def retargets("):]
    costs = src[src.index("def fleet_goal_costs("):src.index("def retargets(")]
    assert "eng.reach_search(" in solo and "eng.reach_commit(" in solo and "self.connect_goal(" in solo
    assert fleet.count("Engine.reach_search_multi(") == 1 and fleet.count("Engine.reach_commit_multi(") == 1 and "connect_goals(" in fleet
    assert ".reach_search(" not in fleet and ".reach_commit(" not in fleet and "_fleet_commit(" in fleet
    order = [fleet.index(w) for w in (".set_goal(", "._engine_resolution(", "._grown_goal =", "._connect_accept(")]
    assert order == sorted(order)
    assert costs.count("Engine.reach_search_multi(") == 1 and ".reach_search(" not in costs and "_commit" not in costs
    for part in (fleet, costs):
        assert "_fleet_check(" in part and "_fleet_begin(" in part and "_fleet_groups(" in part
    assert "_goal_costs_targets(" in costs and "_goal_costs_targets(" in src[src.index("    def goal_costs(self"):src.index("    def retarget(self")]
    eng = open(os.path.join(ROOT, "lqrrt_amd", "engine.py")).read()
    both = eng[eng.index("    def _targets_multi("):eng.index("    def push_samples(")]
    assert "._targets(" in both and "_commit_outputs(" in both and "_commit_results(" in both and "_goal_box" not in both


def test_header_declares_the_two_calls():
    text = open(os.path.join(ROOT, "include", "lqrrt_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("lqrrt_reach_search_multi", "lqrrt_reach_commit_multi"):
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in nat.SIGNATURES
        assert hasattr(nat.lib(), name)
    assert len(nat.SIGNATURES["lqrrt_reach_search_multi"][1]) == 14 and len(nat.SIGNATURES["lqrrt_reach_commit_multi"][1]) == 12
    assert nat.lib().lqrrt_abi_version() == 1
    assert callable(lqrrt_amd.engine.Engine.reach_search_multi) and callable(lqrrt_amd.engine.Engine.reach_commit_multi)


def test_reach_multi_stays_plain_launches():
    """One stream, plain launches: no cooperative launch, no grid-wide barrier, no inline assembly; the two kernels wrap the bodies
    that exist and hold no copy of the chain; the host runs on the multi path that exists and allocates nothing of its own."""
    csrc = os.path.join(ROOT, "lqrrt_amd", "csrc")
    for f in ("reach_multi.hpp", "engine_reach_multi.hpp"):
        text = open(os.path.join(csrc, f)).read()
        for word in ("hipLaunchCooperativeKernel", "hipModuleLaunchCooperativeKernel", "cooperative_groups", "grid.sync", "this_grid",
                     "asm"):
            assert word not in text, (f, word)
    src = open(os.path.join(csrc, "reach_multi.hpp")).read()
    for name in ("reach_search_body<S>(", "refine_commit_body<S>(", "multi_engine_of(", "launch_constant(", "struct ReachDesc",
                 "struct ReachCommitDesc", "k_reach_search_multi", "k_reach_commit_multi"):
        assert name in src, name
    assert "S::step(" not in src and "refine_edge<S>(" not in src and src.count("__launch_bounds__(64)") == 2
    assert "- (unsigned)gr.block0[e]" in src                        # the body's block index is relative to the engine's first workgroup
    host = open(os.path.join(csrc, "engine_reach_multi.hpp")).read()
    assert host.count("hipLaunchKernelGGL(") == 2 and "k_reach_search_multi<S>" in host and "k_reach_commit_multi<S>" in host
    for name in ("connect_depths(", "reach_target_fill(", "reach_target_check(", "multi_engines_check(", "multi_id_list(", "candidates_check(",
                 "connect_winner_check(", "multi_search_run(", "multi_commit_run("):
        assert name in host, name
    # ... the two runners of engine_refine.hpp, which hold the chunks, the scratch, the grid and the call's one synchronise
    refine = open(os.path.join(csrc, "engine_refine.hpp")).read()
    search = refine[refine.index("static int multi_search_run("):refine.index("static int multi_commit_run(")]
    commit = refine[refine.index("static int multi_commit_run("):refine.index("static int refine_multi_check(")]
    for name in ("multi_chunks(", "refine_multi_scratch(", "multi_grid(", "refine_multi_protos("):
        assert name in search, name
    for name in ("multi_chunks(", "refine_multi_scratch(", "multi_commit_head(", "refine_multi_protos(", "multi_commit_adopt("):
        assert name in commit, name
    assert "hipMalloc" not in host and "dalloc(" not in host and "hipStreamSynchronize(" not in host
    assert search.count("hipStreamSynchronize(") == 1 and commit.count("hipStreamSynchronize(") == 1          # one per call
    for run in (search, commit):
        assert run.index("HIPCHK(hipStreamSynchronize(st));") < run.index("drain.disarm();")
    kernels = open(os.path.join(csrc, "kernels.hpp")).read()
    assert kernels.index('#include "reach.hpp"') < kernels.index('#include "reach_multi.hpp"')
    engine = open(os.path.join(csrc, "engine.hip")).read()
    assert engine.index('#include "engine_reach.hpp"') < engine.index('#include "engine_reach_multi.hpp"')


def test_multi_kernels_keep_their_twins_frame_and_occupancy():
    """For every model S, UserSystem included: k_reach_search_multi<S> has a private segment no larger and an occupancy no lower than
    k_reach_search<S>, and k_reach_commit_multi<S> the same against k_refine_commit_multi<S> -- the indirection through EngineProto
    and the descriptors, and the resolution block that travels in the commit's descriptor, cost neither."""
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
    for twin, multi in (("k_reach_search", "k_reach_search_multi"), ("k_refine_commit_multi", "k_reach_commit_multi")):
        a, b = by_model(twin), by_model(multi)
        assert len(a) >= 10 and "UserSystem" in a, sorted(a)
        assert sorted(b) == sorted(a)
        for model in a:
            print("%-22s %s %4d B occ %d vgpr %3d agpr %d sgpr %3d   %s %4d B occ %d vgpr %3d agpr %d sgpr %3d" % (
                model, twin, a[model]["scratch"], a[model]["occupancy"], a[model]["vgpr"], a[model]["agpr"], a[model].get("sgpr", -1),
                multi, b[model]["scratch"], b[model]["occupancy"], b[model]["vgpr"], b[model]["agpr"], b[model].get("sgpr", -1)))
        worse = {m: (a[m]["scratch"], b[m]["scratch"], a[m]["occupancy"], b[m]["occupancy"]) for m in a
                 if b[m]["scratch"] > a[m]["scratch"] or b[m]["occupancy"] < a[m]["occupancy"]}
        assert not worse, (multi, worse)
