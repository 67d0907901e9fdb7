"""
Tree-wide goal connection (Planner.connect_goal) on the CPU: the reference of the rule (tests/connect_reference.py, composed from
the C oracle's primitives) on committed fixtures, the host side of the public method, and what the compiler says about the search
kernel.  The device search is compared with the same reference bit for bit in tests/test_connect_gpu.py.
"""
import os
import re
import shutil
import sys

import numpy as np
import pytest

import coracle
import lqrrt_amd
import connect_reference as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# fixture trees cut off BEFORE their first goal node (no node lies in the goal box: the planner would fall back):
# name, nodes kept, winner (cost, start node), lengths of the appended edges, steps of the search's own first hit (the node cut off)
PREFIXES = [("car_2000", 217, (951, 211), [50, 50], 1101),
            ("boat_novice_300", 107, (781, 77), [20] * 8, 821),
            ("boat_novice_lqr_400", 144, (481, 73), [20] * 8, 529),     # Riccati gains
            ("boat_advanced_10k", 3308, (1707, 3305), [10], None),
            ("double_integrator_600", 5, (41, 0), [20, 20], 101)]       # box grid

# full fixture trees, the fixture plan's step count as incumbent: name, winner (cost, start node) or None
FULL = [("car_500", (951, 211)),
        ("boat_novice_lqr_400", (481, 73)),                            # off the plan (574 steps; refine_plan's first round: 450)
        ("boat_advanced_10k", (1256, 5993)),                           # node 5993 lies in the goal box itself, at 1255 steps
        ("pendulum_lqr_120", None), ("boat_advanced_200", None), ("boat_advanced_3000", None)]


def _check_chain(s, r, size0, plan):
    """Every appended edge re-simulates from its parent's end state, every row is feasible, the stored gain is lqr(x_end, u_last)[1];
    the plan is a parent chain from the root that ends in the goal box (the checks of test_reference_refines_fixture_plans)."""
    o = coracle.make(s, 16)
    for nid in range(size0, r.size):
        xs, us = r.edges[nid]
        x = r.states[r.pID[nid]]
        for k in range(len(xs)):
            x = o.dynamics(x, us[k])
            assert np.array_equal(x, xs[k]), (nid, k)
            assert o.feasible(xs[k], us[k]), (nid, k)
        assert np.array_equal(r.states[nid], xs[-1])
        assert np.array_equal(r.K[nid], o.gain(xs[-1], us[-1]))
    assert plan[0] == 0 and all(r.pID[b] == a for a, b in zip(plan, plan[1:]))
    assert r.in_goal(r.states[plan[-1]])


@pytest.mark.parametrize("name,size,winner,lens,first_hit", PREFIXES)
def test_reference_connects_goal_free_prefixes(name, size, winner, lens, first_hit):
    s, g = cr.case(name)
    assert cr.first_goal_node(s, g) == size
    r = cr.from_fixture(s, g, size)
    assert not any(r.in_goal(x) for x in r.states)
    win = r.search()
    print(name, None if win is None else (win[0], win[1], [len(e[0]) for e in win[2]]))
    assert win is not None and (win[0], win[1]) == winner
    assert [len(e[0]) for e in win[2]] == lens
    if first_hit is not None:                                       # shorter than the plan the search itself finds later
        full = cr.from_fixture(s, g)
        assert full.depths()[size] == first_hit and win[0] < first_hit
    plan, ids = r.commit_chain(win)
    assert ids == list(range(size, size + len(lens))) and plan == r.climb(win[1]) + ids
    assert r.cost(plan) == win[0] == r.depths()[plan[-1]]
    _check_chain(s, r, size, plan)


@pytest.mark.parametrize("name,winner", FULL)
def test_reference_on_full_fixture_trees(name, winner):
    s, g = cr.case(name)
    r = cr.from_fixture(s, g)
    incumbent = r.cost([int(v) for v in g["node_seq"]])
    assert incumbent == len(g["plan_x"])
    win = r.search(incumbent=incumbent)
    print(name, incumbent, None if win is None else (win[0], win[1], [len(e[0]) for e in win[2]]))
    assert (None if win is None else (win[0], win[1])) == winner
    if win is None:
        return
    assert win[0] < incumbent
    size0 = r.size
    plan, _ = r.commit_chain(win)
    _check_chain(s, r, size0, plan)


def test_reference_winner_inside_the_goal_box_needs_an_edge():
    s, g = cr.case("boat_advanced_10k")
    r = cr.from_fixture(s, g)
    assert r.in_goal(r.states[5993]) and r.depths()[5993] == 1255
    cost, edges = r.chain(5993)
    assert cost == 1256 and [len(e[0]) for e in edges] == [1]


@pytest.mark.parametrize("name", ["car_500", "boat_novice_lqr_400"])
def test_reference_agrees_with_the_refinement_on_the_plan(name):
    """Restricted to the plan's nodes but the last, the candidates are the refinement's (i, P-1) under another name."""
    s, g = cr.case(name)
    r = cr.from_fixture(s, g)
    plan = [int(v) for v in g["node_seq"]]
    P = len(plan)
    prefix = np.cumsum([1] + [r.elen[p] for p in plan[1:]])
    best = None
    for i in range(P - 1):                                          # Refiner.round's chain of candidate (i, P-1), without its pruning
        x, K, cost = r.states[plan[i]], r.K[plan[i]], int(prefix[i])
        for t in range(P - 1, P - 1 + 8):
            ln, xs, us, Ke = r._edge(x, K, r.goal)
            if ln == 0:
                continue
            cost += ln
            x, K = xs[-1], Ke.copy()
            if r.in_goal(x):
                if best is None or (cost, i) < best:
                    best = (cost, i)
                break
    win = r.search(nodes=plan[:-1])
    assert best is not None and win is not None
    assert (win[0], win[1]) == (best[0], plan[best[1]])


def test_reference_winner_is_independent_of_the_order():
    s, g = cr.case("car_2000")
    r = cr.from_fixture(s, g, 217)
    ids = np.random.RandomState(5).permutation(217).tolist()
    a, b, c = r.search(nodes=ids), r.search(nodes=sorted(ids)), r.search(nodes=ids[::-1])
    assert (a[0], a[1]) == (b[0], b[1]) == (c[0], c[1]) == (951, 211)
    assert r.search(nodes=ids, incumbent=951) is None               # the winner's own cost as incumbent: nothing shorter
    assert r.search(nodes=[v for v in ids if v != 211])[:2] != (951, 211)


def _native_planner():
    car = lqrrt_amd.systems.Car(0)
    cons = lqrrt_amd.Constraints(car.nstates, car.ncontrols, car.goal_buffer, car.is_feasible)
    return lqrrt_amd.Planner(car.dynamics, car.lqr, cons, error_tol=car.error_tol, erf=car.erf, goal0=car.goal, printing=False,
                             **car.plan_kwargs)


def test_connect_goal_without_a_plan_changes_nothing():
    p = _native_planner()
    assert p.connect_goal() is False
    assert p.connect_goal(goal_tries=2, nodes=[0], finish_on_goal=True) is False
    assert p.tree is None and not hasattr(p, "node_seq") and not p.plan_reached_goal
    with pytest.raises(ValueError):
        p.connect_goal(goal_tries=0)


def test_connect_goal_refuses_callback_mode():
    cons = lqrrt_amd.Constraints(2, 1, [0.1, 0.1], lambda x, u: True)
    p = lqrrt_amd.Planner(lambda x, u, dt: x + dt * np.array([x[1], u[0]]), lambda x, u: (np.eye(2), np.array([[1.0, 1.0]])), cons,
                          horizon=1, dt=0.1, goal0=[1.0, 0.0], printing=False)
    assert p.callback_mode
    with pytest.raises(NotImplementedError, match="Python"):
        p.connect_goal()


def test_connect_goal_shares_the_refinement_steps():
    """connect_goal goes through refine_plan's helpers (begin checks, incumbent, dropping the host tail, adoption)."""
    src = open(os.path.join(ROOT, "lqrrt_amd", "planner.py")).read()
    body = src[src.index("    def connect_goal(self"):src.index("    def _in_goal(self")]
    for name in ("_refine_begin(", "_refine_incumbent(", "_refine_accept(", "_refine_end("):
        assert name in body, name
    assert "_drop_host_tail" not in body and "_adopt_plan" not in body


def test_connect_search_keeps_the_refinement_searchs_frame():
    """For every model S: k_connect_search<S> exists, its private segment is no larger than that of k_refine_search<S> and its
    occupancy no lower -- it is the same chain with fewer targets."""
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
    refine, connect = by_model("k_refine_search"), by_model("k_connect_search")
    assert len(refine) >= 10 and "UserSystem" in refine, sorted(refine)
    assert sorted(connect) == sorted(refine)
    for model in refine:
        print("%-18s refine %4d B occ %d vgpr %3d   connect %4d B occ %d vgpr %3d" % (
            model, refine[model]["scratch"], refine[model]["occupancy"], refine[model]["vgpr"],
            connect[model]["scratch"], connect[model]["occupancy"], connect[model]["vgpr"]))
    worse = {m: (refine[m]["scratch"], connect[m]["scratch"], refine[m]["occupancy"], connect[m]["occupancy"]) for m in refine
             if connect[m]["scratch"] > refine[m]["scratch"] or connect[m]["occupancy"] < refine[m]["occupancy"]}
    assert not worse, worse


def test_connection_stays_plain_launches():
    """One stream, plain launches: no cooperative launch, no grid-wide barrier; the chain's pieces are the refinement's, not copies."""
    for f in ("connect.hpp", "engine_connect.hpp"):
        text = open(os.path.join(ROOT, "lqrrt_amd", "csrc", f)).read()
        for word in ("hipLaunchCooperativeKernel", "hipModuleLaunchCooperativeKernel", "cooperative_groups", "grid.sync", "this_grid"):
            assert word not in text, (f, word)
    src = open(os.path.join(ROOT, "lqrrt_amd", "csrc", "connect.hpp")).read()
    for name in ("refine_start<S>(", "refine_edge<S>(", "refine_in_goal<S>(", "refine_best(", "stage_geo("):
        assert name in src, name
    assert "__launch_bounds__(64)" in src and "S::step(" not in src
