"""
One tree asked about many goals (Planner.goal_costs / Planner.retarget) on the CPU: the reference of the rule
(tests/reach_reference.py, a connect_reference.Connector per target) against rows pinned with the C oracle, the host side of the
two public methods, the ABI's declarations, and what the compiler says about the search kernel.  The device search is compared with
the same reference and the same rows in tests/test_reach_gpu.py.
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


@pytest.mark.parametrize("name,size", sorted(rh.PINNED))
def test_reference_gives_the_pinned_rows(name, size):
    """goal_tries = 8, the fixture's horizon, no incumbent: per target the winner (cost, node) of a Connector of its own."""
    s, g = cr.case(name)
    rows = rh.PINNED[(name, size)]
    goals, bufs = rh.pinned_targets(s, g, rows)
    got = rh.from_fixture(s, g, size).search(goals, bufs)
    print(name, size, got)
    assert got == [w for _, w in rows]
    assert sum(w is not None for w in got) >= 5
    # "own goal" and "own goal, buffer x 0.25" share the goal and differ in the box only; "far" differs in one state
    assert np.array_equal(goals[0], goals[5]) and not np.array_equal(bufs[0], bufs[5]) and goals[6][0] == goals[0][0] + 1e4
    # the first row is connect_reference's own winner on that prefix
    own = cr.from_fixture(s, g, size).search()
    assert (own[0], own[1]) == got[0]


def test_reference_targets_do_not_interact():
    """A target's winner is the same alone, first, last, and next to a copy of itself with a tighter incumbent."""
    s, g = cr.case("car_2000")
    r = rh.from_fixture(s, g, 217)
    goals, bufs = rh.pinned_targets(s, g, rh.PINNED[("car_2000", 217)])
    alone = [r.search(goals[t:t + 1], bufs[t:t + 1])[0] for t in range(len(goals))]
    assert alone == r.search(goals, bufs) == r.search(goals[::-1], bufs[::-1])[::-1]
    assert r.search(goals[[0, 0]], bufs[[0, 0]], incumbents=[951, 952]) == [None, (951, 211)]
    ids = np.random.RandomState(5).permutation(217).tolist()
    assert r.search(goals[:3], bufs[:3], nodes=ids) == alone[:3]
    assert r.search(goals[:3], bufs[:3], nodes=[211]) == [(951, 211), None, None]
    assert r.search(goals[:3], bufs[:3], nodes=[]) == [None, None, None]


def _native_planner():
    car = lqrrt_amd.systems.Car(0)
    cons = lqrrt_amd.Constraints(car.nstates, car.ncontrols, car.goal_buffer, car.is_feasible)
    return car, lqrrt_amd.Planner(car.dynamics, car.lqr, cons, error_tol=car.error_tol, erf=car.erf, goal0=car.goal, printing=False,
                                  **car.plan_kwargs)


def test_without_a_plan_nothing_happens():
    car, p = _native_planner()
    goal = np.array(car.goal, dtype=np.float64)
    assert p.goal_costs([goal, goal + 1.0]) is None
    assert p.goal_costs([goal], goal_buffers=car.goal_buffer, goal_tries=2, nodes=[0]) is None
    assert p.retarget(goal + 1.0) is False
    assert p.retarget(goal, goal_tries=2, nodes=[0], finish_on_goal=True) is False
    assert p.tree is None and not hasattr(p, "node_seq") and not p.plan_reached_goal
    assert np.array_equal(p.goal, goal)


def test_refusals():
    car, p = _native_planner()
    n = car.nstates
    goal = np.array(car.goal, dtype=np.float64)
    for bad in (dict(goals=[goal], goal_tries=0), dict(goals=goal), dict(goals=[goal[:-1]]), dict(goals=np.zeros((0, n))),
                dict(goals=[goal], goal_buffers=np.ones(n + 1)), dict(goals=[goal, goal], goal_buffers=np.ones((3, n))),
                dict(goals=[goal], goal_buffers=-np.abs(np.asarray(car.goal_buffer, dtype=np.float64)) - 1.0)):
        with pytest.raises(ValueError):
            p.goal_costs(**bad)
    with pytest.raises(ValueError):
        p.retarget(goal, goal_tries=0)
    with pytest.raises(ValueError):
        p.retarget(goal[:-1])
    with pytest.raises(ValueError):
        p.retarget([goal, goal])
    assert np.array_equal(p.goal, goal) and p.tree is None


def test_callback_mode_is_refused():
    cons = lqrrt_amd.Constraints(2, 1, [0.1, 0.1], lambda x, u: True)
    p = lqrrt_amd.Planner(lambda x, u, dt: x + dt * np.array([x[1], u[0]]), lambda x, u: (np.eye(2), np.array([[1.0, 1.0]])), cons,
                          horizon=1, dt=0.1, goal0=[1.0, 0.0], printing=False)
    assert p.callback_mode
    with pytest.raises(NotImplementedError, match="Python"):
        p.goal_costs([[1.0, 0.0]])
    with pytest.raises(NotImplementedError, match="Python"):
        p.retarget([2.0, 0.0])


def test_the_goal_box_has_one_statement():
    """Engine.set_resolution and the target tables of reach_search / reach_commit compute their boxes in one helper."""
    src = open(os.path.join(ROOT, "lqrrt_amd", "engine.py")).read()

    def body(method):
        b = src[src.index("    def %s(" % method):]
        return b[:b.index("\n    def ", 10)]
    assert "_goal_box(" in body("set_resolution") and "_goal_box(" in body("_targets")
    assert "_targets(" in body("reach_search") and "_targets(" in body("reach_commit")
    assert src.count("g[i] - b[i]") == 1 and src.count("g[i] + b[i]") == 1
    plan = open(os.path.join(ROOT, "lqrrt_amd", "planner.py")).read()
    retarget = plan[plan.index("    def retarget(self"):plan.index("# ------------------------------------------------------------------------------------------ setters")]
    order = [retarget.index(w) for w in ("self.set_goal(goal)", "self._engine_resolution(eng)", "self._grown_goal =", "self._connect_accept(")]
    assert order == sorted(order)
    assert "_engine_resolution(eng)" in plan[plan.index("    def _plan_prepare(self"):plan.index("    def _plan_start(self")]


def test_header_declares_the_two_calls():
    text = open(os.path.join(ROOT, "include", "lqrrt_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("lqrrt_reach_search", "lqrrt_reach_commit"):
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in nat.SIGNATURES
        assert hasattr(nat.lib(), name)
    assert len(nat.SIGNATURES["lqrrt_reach_search"][1]) == 13 and len(nat.SIGNATURES["lqrrt_reach_commit"][1]) == 10
    assert nat.lib().lqrrt_abi_version() == 1
    assert callable(lqrrt_amd.engine.Engine.reach_search) and callable(lqrrt_amd.engine.Engine.reach_commit)


def test_reach_stays_plain_launches():
    """One stream, plain launches: no cooperative launch, no grid-wide barrier; the chain's pieces are the refinement's, not copies."""
    for f in ("reach.hpp", "engine_reach.hpp"):
        text = open(os.path.join(ROOT, "lqrrt_amd", "csrc", f)).read()
        for word in ("hipLaunchCooperativeKernel", "hipModuleLaunchCooperativeKernel", "cooperative_groups", "grid.sync", "this_grid",
                     "asm(", "asm volatile"):
            assert word not in text, (f, word)
    src = open(os.path.join(ROOT, "lqrrt_amd", "csrc", "reach.hpp")).read()
    for name in ("refine_start<S>(", "refine_edge<S>(", "refine_in_goal<S>(", "refine_best(", "stage_geo(", "GainLds<S>", "launch_constant(",
                 "connect_key("):
        assert name in src, name
    assert src.count("__launch_bounds__(64)") == 1 and "S::step(" not in src and "reach_search_body<S>(" in src
    host = open(os.path.join(ROOT, "lqrrt_amd", "csrc", "engine_reach.hpp")).read()
    # the depth pass and the staging of table and id list are connect's, the scratch the solo search runner's
    assert "connect_depths(" in host and "ReachSearchSolo h{{std::vector<int>((size_t)e->N), nodes_host, count}" in host and "return solo_search_run(" in host
    # reach adds exactly one launch site of its own, the search; its commit is the connect commit's function, which replays with
    # k_refine_commit (the refinement's commit hooks) and adopts through the solo commit runner / refine_adopt
    assert host.count("hipLaunchKernelGGL(") == 1 and "k_reach_search<S>" in host and "hipMalloc" not in host and "dalloc(" not in host
    assert "return connect_commit_run(" in host and "k_refine_commit" not in host
    connect = open(os.path.join(ROOT, "lqrrt_amd", "csrc", "engine_connect.hpp")).read()
    shared = connect[connect.index("static int connect_commit_run("):connect.index('extern "C" int lqrrt_connect_commit(')]
    assert "return solo_commit_run(" in shared and "RefineCommitSolo{" in shared and "hipLaunchKernelGGL(" not in shared
    assert connect.count("connect_commit_run(") == 2                # its definition and lqrrt_connect_commit's call
    refine = open(os.path.join(ROOT, "lqrrt_amd", "csrc", "engine_refine.hpp")).read()
    hooks = refine[refine.index("struct RefineCommitSolo"):refine.index('extern "C" int lqrrt_refine_search(')]
    assert hooks.count("hipLaunchKernelGGL(") == 1 and "k_refine_commit<S>" in hooks and "dim3(1)" in hooks
    finish = refine[refine.index("static int solo_commit_run("):refine.index("static void refine_decode(")]
    assert "solo_scratch(" in finish and "refine_adopt(" in finish and "LQRRT_E_CAPACITY" in finish and "LQRRT_E_STATE" in finish
    kernels = open(os.path.join(ROOT, "lqrrt_amd", "csrc", "kernels.hpp")).read()
    assert kernels.index('#include "connect.hpp"') < kernels.index('#include "reach.hpp"')


def test_reach_search_keeps_the_connect_searchs_frame():
    """For every model S, UserSystem included: k_reach_search<S> exists, its private segment is no larger than that of
    k_connect_search<S> and its occupancy no lower -- it is the same chain with its goal and box read from a table."""
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
    connect, reach = by_model("k_connect_search"), by_model("k_reach_search")
    assert len(connect) >= 10 and "UserSystem" in connect, sorted(connect)
    assert sorted(reach) == sorted(connect)
    for model in connect:
        print("%-22s connect %4d B occ %d vgpr %3d sgpr %3d   reach %4d B occ %d vgpr %3d sgpr %3d" % (
            model, connect[model]["scratch"], connect[model]["occupancy"], connect[model]["vgpr"], connect[model].get("sgpr", -1),
            reach[model]["scratch"], reach[model]["occupancy"], reach[model]["vgpr"], reach[model].get("sgpr", -1)))
    worse = {m: (connect[m]["scratch"], reach[m]["scratch"], connect[m]["occupancy"], reach[m]["occupancy"]) for m in connect
             if reach[m]["scratch"] > connect[m]["scratch"] or reach[m]["occupancy"] < connect[m]["occupancy"]}
    assert not worse, worse
