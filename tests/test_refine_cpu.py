"""
Plan refinement (Planner.refine_plan) on the CPU: the reference of the rule (tests/refine_reference.py, composed from the C
oracle's primitives) on committed fixtures, and the host side of the public method.  The device search is compared with the
same reference bit for bit in tests/test_refine_gpu.py.
"""
import os

import numpy as np
import pytest

import coracle
import lqrrt_amd
import refine_reference as rr

# plan step counts T/dt before and after refinement to the fix-point (at most 8 rounds, 8 goal tries)
FIXTURES = [("car", "500", 1101, 496), ("car", "2000", 1690, 601),
            ("boat_novice", "300", 953, 678), ("boat_novice", "firstgoal", 821, 741)]


def _fixture(golden_dir, name, tag):
    path = os.path.join(golden_dir, "traj_%s_%s.npz" % (name, tag))
    if not os.path.exists(path):
        pytest.fail("fixture missing: tests/golden is committed, a lost fixture must not turn into a pass")
    return np.load(path)


@pytest.mark.parametrize("name,tag,before,after", FIXTURES)
def test_reference_refines_fixture_plans(golden_dir, name, tag, before, after):
    g = _fixture(golden_dir, name, tag)
    s = lqrrt_amd.systems.SYSTEMS[name](0)
    r, plan = rr.from_fixture(s, g)
    assert r.cost(plan) == before == len(g["plan_x"])
    size0 = r.size
    costs = [before]
    for _ in range(8):
        win = r.round(plan)
        if win is None:
            break
        assert win[0] < costs[-1]                                   # costs never increase: a round is accepted only below C
        plan, ids = r.commit(plan, win)
        assert r.cost(plan) == win[0]
        costs.append(win[0])
    assert costs[-1] == after and len(costs) >= 2
    # every new edge re-simulates from its parent's end state, every state on it is feasible
    o = coracle.make(s, 16)
    for nid in range(size0, r.size):
        xs, us = r.edges[nid]
        x = r.states[r.pID[nid]]
        for k in range(len(xs)):
            x = o.dynamics(x, us[k])
            assert np.array_equal(x, xs[k]), (nid, k)
            assert o.feasible(xs[k], us[k]), (nid, k)
        assert np.array_equal(r.states[nid], xs[-1])
        assert np.array_equal(r.K[nid], o.gain(xs[-1], us[-1]))      # tree.add_node's lqr(x_end, u_last)
    # the refined plan is a parent chain from the root that ends in the goal box
    assert plan[0] == 0 and all(r.pID[b] == a for a, b in zip(plan, plan[1:]))
    assert r.in_goal(r.states[plan[-1]])


def test_reference_respects_capacity(golden_dir):
    g = _fixture(golden_dir, "car", "500")
    s = lqrrt_amd.systems.Car(0)
    r, plan = rr.from_fixture(s, g)
    cap = r.size + 5                                                # the first winner's chain has 9 nodes
    out, log = r.refine(plan, capacity=cap)
    assert log == [] and out == plan and r.size == cap - 5


def _native_planner():
    car = lqrrt_amd.systems.Car(0)
    cons = lqrrt_amd.Constraints(car.nstates, car.ncontrols, car.goal_buffer, car.is_feasible)
    return lqrrt_amd.Planner(car.dynamics, car.lqr, cons, error_tol=car.error_tol, erf=car.erf, goal0=car.goal, printing=False,
                             **car.plan_kwargs)


def test_refine_plan_without_a_plan_changes_nothing():
    p = _native_planner()
    assert p.refine_plan() == 0
    assert p.refine_plan(max_rounds=3, goal_tries=2) == 0
    assert p.tree is None and not hasattr(p, "node_seq")
    with pytest.raises(ValueError):
        p.refine_plan(goal_tries=0)


def test_refine_plan_refuses_callback_mode():
    cons = lqrrt_amd.Constraints(2, 1, [0.1, 0.1], lambda x, u: True)
    p = lqrrt_amd.Planner(lambda x, u, dt: x + dt * np.array([x[1], u[0]]), lambda x, u: (np.eye(2), np.array([[1.0, 1.0]])), cons,
                          horizon=1, dt=0.1, goal0=[1.0, 0.0], printing=False)
    assert p.callback_mode
    with pytest.raises(NotImplementedError, match="Python"):
        p.refine_plan()
