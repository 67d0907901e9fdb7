"""
Tree retention (Engine.tree_retain / Planner.replan) on the CPU: the reference of the rule (tests/retain_reference.py, plain
NumPy) on trees grown by the C oracle, and the host side of the public methods.  The device kernels are compared with the same
reference bit for bit in tests/test_retain_gpu.py.
"""
import ctypes

import numpy as np
import pytest

import coracle
import lqrrt_amd
import retain_reference as rr

ARRAYS = ("state", "K", "pID", "elen", "xedge", "uedge")


def boat_tree():
    """boat_advanced, seed 1, grown until it exceeds 5000 nodes: 5001 nodes, 54 goal hits, best plan of 91 nodes."""
    s = lqrrt_amd.systems.BoatAdvanced(0)
    o = coracle.make(s, 6000, seed=1)
    o.extend(max_nodes=5000)
    return s, o


def plan_of(pID, end):
    plan = [int(end)]
    while pID[plan[-1]] != -1:
        plan.append(int(pID[plan[-1]]))
    return plan[::-1]


def scenario_a(s, o):
    """The world of scenario A: one more circle, 4 m beside node 45 of the best plan.  Returns (plan, obstacle table)."""
    plan = plan_of(o.parents(), o.best()[0])
    mid = o.states()[plan[45]]
    return plan, np.vstack((np.asarray(s.obs, dtype=np.float64).reshape(-1, 3), [mid[0] + 4.0, mid[1], 1.0]))


@pytest.fixture(scope="module")
def grown():
    s, o = boat_tree()
    return s, o, rr.oracle_arrays(o)


def test_identity_retain_is_a_no_op(grown):
    """Root 0 without revalidation: every array unchanged, and rule 4 reproduces what the loop itself had accumulated."""
    s, o, arr = grown
    assert o.size == 5001
    lo, hi = rr.goal_box(s)
    r = rr.retain(*arr, 0, None, lo, hi)
    for name, before in zip(ARRAYS, arr):
        np.testing.assert_array_equal(r[name], before, err_msg=name)
    np.testing.assert_array_equal(r["ignored"], o.ignored())
    np.testing.assert_array_equal(r["old_to_new"], np.arange(5001))
    st = r["stats"]
    assert (st["old_size"], st["kept"], st["outside"], st["infeasible"], st["orphaned"], st["root_feasible"]) == (5001, 5001, 0, 0, 0, 1)
    assert st["goal_hits"] == o.hits == 54
    assert (st["best_end"], st["best_steps"]) == o.best() == (4363, 1261)


def test_scenario_a_every_category(grown):
    s, o, arr = grown
    plan, obs2 = scenario_a(s, o)
    assert len(plan) == 91 and plan[-1] == 4363 and plan[45] == 970 and plan[20] == 114
    s2 = lqrrt_amd.systems.BoatAdvanced(0, obstacles=obs2)
    o2 = coracle.make(s2, 6000, seed=9)
    lo, hi = rr.goal_box(s)
    # root 0: nothing outside, the obstacle cuts 147 edges and orphans 471 nodes, the old best plan among them
    r0 = rr.retain(*arr, 0, o2.feasible, lo, hi)
    st = r0["stats"]
    assert (st["kept"], st["outside"], st["infeasible"], st["orphaned"], st["root_feasible"]) == (4383, 0, 147, 471, 1)
    assert st["goal_hits"] == 34 and r0["old_to_new"][4363] == -1
    assert st["kept"] + st["outside"] + st["infeasible"] + st["orphaned"] == st["old_size"] == 5001
    # root = node 20 of the plan
    r = rr.retain(*arr, plan[20], o2.feasible, lo, hi)
    st = r["stats"]
    assert st["old_size"] - st["outside"] == 3240                               # the subtree of node 114
    assert (st["kept"], st["infeasible"], st["orphaned"], st["goal_hits"]) == (2622, 147, 471, 28)
    assert (st["best_end"], st["best_steps"]) == (2083, 1366) and r["old_ids"][2083] == 3841
    assert int(r["ignored"].sum()) == 282
    check_invariants(arr, r, plan[20], o2.feasible)
    # the same root without revalidation keeps the whole subtree
    rn = rr.retain(*arr, plan[20], None, lo, hi)
    assert (rn["stats"]["kept"], rn["stats"]["infeasible"], rn["stats"]["orphaned"]) == (3240, 0, 0)
    # the kept tree is a tree the sequential planner can keep growing on the new map
    o2.load_tree(r["state"], r["K"], r["pID"], r["ignored"])
    o2.extend(max_nodes=st["kept"] + 399)
    assert (o2.size, o2.iterations) == (3022, 978)
    np.testing.assert_array_equal(o2.states()[:2622], r["state"])


def check_invariants(arr, r, root, feasible):
    state, K, pID, elen, xedge, uedge = arr
    st, old = r["stats"], r["old_ids"]
    M = st["kept"]
    assert st["kept"] + st["outside"] + st["infeasible"] + st["orphaned"] == st["old_size"] == len(state)
    assert old[0] == root and r["pID"][0] == -1 and r["elen"][0] == 1
    assert np.array_equal(r["xedge"][0, 0], state[root]) and not r["uedge"][0, 0].any()
    assert np.all(r["pID"][1:] < np.arange(1, M)) and np.all(r["pID"][1:] >= 0)
    assert np.all(np.diff(old) > 0)                                             # order-preserving
    np.testing.assert_array_equal(r["state"], state[old])
    np.testing.assert_array_equal(r["K"], K[old])
    np.testing.assert_array_equal(old[r["pID"][1:]], pID[old[1:]])              # the same parents, renumbered
    for k in range(1, M):
        i = old[k]
        assert r["elen"][k] == elen[i]
        np.testing.assert_array_equal(r["xedge"][k, :elen[i]], xedge[i, :elen[i]])
        np.testing.assert_array_equal(r["uedge"][k, :elen[i]], uedge[i, :elen[i]])
        if feasible is not None:
            assert all(feasible(r["xedge"][k, j], r["uedge"][k, j]) for j in range(elen[i])), k
    assert np.array_equal(np.flatnonzero(r["old_to_new"] >= 0), old)


@pytest.mark.parametrize("name", ["car", "double_integrator"])
def test_invariants_on_other_geometry_models(name):
    """Car (circles swept by a hull) and the double integrator (boxes through the CSR grid): a tree grown in one world, retained
    in another."""
    if name == "car":
        s = lqrrt_amd.systems.Car(0)
        o = coracle.make(s, 1400, seed=3)
        o.extend(max_nodes=1200)
        at = o.states()[o.size // 2]
        obs2 = np.vstack((np.asarray(s.obs, dtype=np.float64).reshape(-1, 3), [at[0], at[1], 1.5]))
        s2 = lqrrt_amd.systems.Car(0, obstacles=obs2)
    else:
        s = lqrrt_amd.systems.DoubleIntegrator(n_boxes=200, seed=2)
        o = coracle.make(s, 1000, seed=3)
        o.extend(max_nodes=800)
        at = o.states()[o.size // 2][:3]
        s2 = lqrrt_amd.systems.DoubleIntegrator(n_boxes=200, seed=2)
        s2.set_obstacles(np.vstack((s.obs, np.concatenate((at - 3.0, at + 3.0)))))
    o2 = coracle.make(s2, 16, seed=3)
    arr = rr.oracle_arrays(o)
    lo, hi = rr.goal_box(s)
    pID = arr[2]
    root = int(pID[pID[o.size // 2]]) if pID[o.size // 2] > 0 else 0
    for rt in sorted(set((0, root))):
        r = rr.retain(*arr, rt, o2.feasible, lo, hi)
        check_invariants(arr, r, rt, o2.feasible)
        assert r["stats"]["infeasible"] > 0                                      # the new obstacle sits on a node
    leaf = int(np.setdiff1d(np.arange(o.size), pID)[-1])
    r = rr.retain(*arr, leaf, o2.feasible, lo, hi)
    assert r["stats"]["kept"] == 1 and r["stats"]["outside"] == o.size - 1 and r["stats"]["goal_hits"] == 0
    assert r["pID"].tolist() == [-1] and r["elen"].tolist() == [1] and np.array_equal(r["state"][0], arr[0][leaf])
    with pytest.raises(ValueError, match="doesn't exist"):
        rr.retain(*arr, o.size, None, lo, hi)


# ---------------------------------------------------------------------------------------------- the public methods, host side

def _native_planner(**over):
    car = lqrrt_amd.systems.Car(0)
    cons = lqrrt_amd.Constraints(car.nstates, car.ncontrols, car.goal_buffer, car.is_feasible)
    kw = dict(error_tol=car.error_tol, erf=car.erf, goal0=car.goal, printing=False, **car.plan_kwargs)
    kw.update(over)
    return car, lqrrt_amd.Planner(car.dynamics, car.lqr, cons, **kw)


def test_replan_without_a_tree_raises():
    car, p = _native_planner()
    with pytest.raises(RuntimeError, match="no tree to keep"):
        p.replan(0, car.sample_space)
    assert p.tree is None and not hasattr(p, "node_seq")


def test_replan_refuses_callback_mode():
    cons = lqrrt_amd.Constraints(2, 1, [0.1, 0.1], lambda x, u: True)
    p = lqrrt_amd.Planner(lambda x, u, dt: x + dt * np.array([x[1], u[0]]), lambda x, u: (np.eye(2), np.array([[1.0, 1.0]])), cons,
                          horizon=1, dt=0.1, goal0=[1.0, 0.0], printing=False)
    assert p.callback_mode
    with pytest.raises(NotImplementedError, match="Python"):
        p.replan(0, [(0, 1), (0, 1)])


def test_plan_node_after_on_a_hand_set_plan():
    car, p = _native_planner(dt=0.1)
    with pytest.raises(RuntimeError):
        p.plan_node_after(0.0)
    S, K = np.eye(car.nstates), np.zeros((car.ncontrols, car.nstates))
    t = lqrrt_amd.Tree(np.zeros(car.nstates), (S, K))
    row = lambda v: np.full(car.nstates, float(v))
    u = np.zeros(car.ncontrols)
    t.add_node(0, row(3), (S, K), [row(1), row(2), row(3)], [u, u, u])          # reached after 3 steps
    t.add_node(0, row(9), (S, K), [row(9)], [u])                                # not on the plan
    t.add_node(1, row(5), (S, K), [row(4), row(5)], [u, u])                     # after 5 steps
    t.add_node(3, row(9), (S, K), [row(6), row(7), row(8), row(9)], [u] * 4)    # after 9 steps
    p.tree, p.node_seq = t, [0, 1, 3, 4]
    x_seq, _ = t.trajectory(p.node_seq)
    assert len(x_seq) == 10                                                     # t_seq = 0 .. 0.9
    assert p.plan_node_after(0.0) == (0, 0, 0.0)
    assert p.plan_node_after(-1.0) == (0, 0, 0.0)
    k, node, tk = p.plan_node_after(0.05)
    assert (k, node) == (1, 1) and tk == pytest.approx(0.3)
    assert p.plan_node_after(0.3)[:2] == (1, 1)
    assert p.plan_node_after(0.31)[:2] == (2, 3)
    k, node, tk = p.plan_node_after(0.6)
    assert (k, node) == (3, 4) and tk == pytest.approx(0.9)
    assert np.array_equal(x_seq[int(round(tk / 0.1))], t.state[node])           # t_k indexes the node's state on the plan
    assert p.plan_node_after(100.0)[:2] == (3, 4)                                # beyond the plan's end: its last node


def test_retain_stats_struct_matches_the_header():
    from lqrrt_amd import _native as nat
    assert ctypes.sizeof(nat.RetainStats) == 40
    assert [f[0] for f in nat.RetainStats._fields_] == list(rr.STAT_KEYS)
    assert "lqrrt_tree_retain" in nat.SIGNATURES
    assert hasattr(lqrrt_amd.engine.Engine, "tree_retain") and hasattr(lqrrt_amd.Planner, "replan")
