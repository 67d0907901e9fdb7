"""
Tree retention on the device (csrc/retain.hpp through lqrrt_tree_retain) against the reference of the rule
(tests/retain_reference.py, NumPy + the C oracle's feasibility test), BIT FOR BIT: states, gains, parents, edge lengths, every
live edge row, ignore flags, goal bookkeeping, the stats and the id map.  Then growth from the kept tree against the sequential
C oracle, the host route (Engine.tree_load) and Planner.replan end to end.
"""
import os

import numpy as np
import pytest

import retain_reference as rr
from retain_compare import check_retained

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WAVE = 256


def _hspan(s, horizon=None):
    kw = s.plan_kwargs
    horizon = kw["horizon"] if horizon is None else horizon
    if hasattr(horizon, "__len__"):
        return tuple(int(v) for v in np.divide(horizon, kw["dt"]).astype(np.int64))
    return int(horizon / kw["dt"])


def _engine(s, capacity, wave=WAVE, horizon=None, seed=1):
    """An engine set up like Planner does it: resolution, default sampler, MT19937 of RandomState(seed)."""
    from lqrrt_amd.engine import Engine
    kw = s.plan_kwargs
    eng = Engine(s, capacity=capacity, max_wave=wave)
    H = _hspan(s, horizon)
    if isinstance(H, tuple):
        eng.set_resolution(kw["dt"], kw["FPR"], H[1], np.abs(s.error_tol), s.goal, np.abs(s.goal_buffer), adaptive=True,
                           hspan_min=H[0], horizon_iters_state=1)
    else:
        eng.set_resolution(kw["dt"], kw["FPR"], H, np.abs(s.error_tol), s.goal, np.abs(s.goal_buffer))
    space = np.array(s.sample_space, dtype=np.float64)
    eng.set_sampler(np.mean(space, axis=1), np.diff(space).flatten(), np.array(s.goal_bias, dtype=np.float64), 10)
    _seed(eng, seed)
    return eng


def _seed(eng, seed):
    st = np.random.RandomState(seed).get_state()
    eng.set_mt19937(st[1], st[2])


def _oracle(s, capacity, seed, horizon=None):
    """The C oracle of the world `s` describes NOW."""
    import coracle
    return coracle.make(s, capacity, seed=seed, horizon=horizon)


def _retain_and_compare(eng, s, root, revalidate, oracle=None):
    """Reads the tree back, retains on the device and in the reference, compares everything.  Returns the reference's result."""
    arr = rr.engine_arrays(eng)
    lo, hi = rr.goal_box(s)
    o = oracle if oracle is not None else _oracle(s, 16, 1)
    ref = rr.retain(*arr, root, o.feasible if revalidate else None, lo, hi)
    stats, old_to_new = eng.tree_retain(root, revalidate=revalidate)
    print("retain root %d revalidate %s: %s" % (root, revalidate, stats))
    check_retained(eng, ref, stats, old_to_new)
    return ref


def _grow_and_compare(eng, s, ref, more=400, seed=9, sync=False, wave=WAVE, horizon=None, may_stall=False):
    """extend by `more` nodes with a fresh MT19937 stream == the C oracle given the reference's kept tree (load_tree).  Both sides
    stop after 40 * more attempts at the latest (a root that cannot move would otherwise be tried for ever)."""
    kept = ref["stats"]["kept"]
    _seed(eng, seed)
    o = _oracle(s, kept + more + 2 * wave + 8, seed, horizon=horizon)
    o.load_tree(ref["state"], ref["K"], ref["pID"], ref["ignored"])
    if sync:
        eng.set_wave_mode("synchronous")
        st = eng.extend(wave, max_attempts=40 * more, node_limit=kept + more - 1)
        o.extend_sync(wave, max_iters=40 * more, max_nodes=kept + more - 1)
    else:
        st = eng.extend(wave, max_attempts=40 * more, node_limit=kept + more - 1)
        o.extend(max_iters=40 * more, max_nodes=kept + more - 1)
    assert eng.size == o.size and (may_stall or eng.size >= kept + more)
    assert st.attempts == o.iterations
    np.testing.assert_array_equal(eng.parents(), o.parents())
    np.testing.assert_array_equal(eng.states(), o.states())
    np.testing.assert_array_equal(eng.gains(), o.gains())
    np.testing.assert_array_equal(eng.edge_lengths()[kept:], o.edge_lengths()[kept:])
    np.testing.assert_array_equal(eng.ignored(), o.ignored())
    np.testing.assert_array_equal(eng.states()[:kept], ref["state"])            # the kept part is untouched
    return o


def _plan_of(eng):
    end = eng.plan_best()[0]
    assert end >= 0
    return eng.climb(end)


def _boat_5001():
    import lqrrt_amd
    s = lqrrt_amd.systems.BoatAdvanced(0)
    eng = _engine(s, 5000 + 2 * WAVE + 8)
    eng.tree_reset(s.x0)
    eng.extend(WAVE, node_limit=5000)
    assert eng.size == 5001 and eng.plan_best() == (4363, 1261, 54)
    return s, eng


def _scenario_a(s, eng):
    """One more circle, 4 m beside node 45 of the best plan; the device sees it after sync_geometry."""
    plan = _plan_of(eng)
    assert len(plan) == 91 and plan[45] == 970 and plan[20] == 114
    mid = eng.states(plan[45], 1)[0]
    s.set_obstacles(np.vstack((np.asarray(s.obs, dtype=np.float64).reshape(-1, 3), [mid[0] + 4.0, mid[1], 1.0])))
    assert eng.sync_geometry()
    return plan


def test_identity_retain_changes_nothing():
    s, eng = _boat_5001()
    before = rr.engine_arrays(eng)
    ign = eng.ignored()
    fp = eng.footprint()
    ref = _retain_and_compare(eng, s, 0, False)
    assert ref["stats"]["kept"] == 5001 and ref["stats"]["goal_hits"] == 54
    for a, b in zip(before, rr.engine_arrays(eng)):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(eng.ignored(), ign)
    ref = _retain_and_compare(eng, s, 0, True)                                   # the same world: every edge passes again
    assert ref["stats"]["kept"] == 5001 and ref["stats"]["infeasible"] == 0 and ref["stats"]["root_feasible"] == 1
    assert eng.footprint() == fp                                                 # all scratch is transient
    _grow_and_compare(eng, s, ref)
    eng.close()


@pytest.mark.parametrize("root_index,revalidate,mode", [(0, True, "exact"), (20, True, "exact"), (20, False, "exact"),
                                                        (0, False, "exact"), (20, True, "synchronous")])
def test_scenario_a_bit_for_bit_then_growth(root_index, revalidate, mode):
    s, eng = _boat_5001()
    plan = _scenario_a(s, eng)
    ref = _retain_and_compare(eng, s, plan[root_index], revalidate)
    st = ref["stats"]
    if revalidate:
        assert (st["infeasible"], st["orphaned"]) == (147, 471)
        assert (st["kept"], st["goal_hits"]) == ((4383, 34) if root_index == 0 else (2622, 28))
    if root_index == 20 and revalidate:
        assert (st["best_end"], st["best_steps"]) == (2083, 1366) and ref["old_ids"][2083] == 3841 and int(ref["ignored"].sum()) == 282
    o = _grow_and_compare(eng, s, ref, sync=(mode == "synchronous"))
    if root_index == 20 and revalidate and mode == "exact":
        assert (o.size, o.iterations) == (3022, 978)
        # the host route: the reference's kept tree through Engine.tree_load, grown from the same stream
        b = _engine(s, 5000 + 2 * WAVE + 8, seed=9)
        xe, ue = rr.packed_edges(ref)
        b.tree_load(ref["state"], ref["K"], ref["pID"], edge_len=ref["elen"], xedge=xe, uedge=ue, ignored=ref["ignored"])
        b.extend(WAVE, max_attempts=16000, node_limit=st["kept"] + 399)
        np.testing.assert_array_equal(eng.states(), b.states())
        np.testing.assert_array_equal(eng.gains(), b.gains())
        np.testing.assert_array_equal(eng.parents(), b.parents())
        xa, ua, la = eng.edges()
        xb, ub, lb = b.edges()
        live = np.arange(xa.shape[1])[None, :] < la[:, None]
        np.testing.assert_array_equal(la, lb)
        np.testing.assert_array_equal(xa[live], xb[live])
        np.testing.assert_array_equal(ua[live], ub[live])
        np.testing.assert_array_equal(eng.ignored(), b.ignored())
        b.close()
    eng.close()


def test_leaf_root_and_bad_roots():
    s, eng = _boat_5001()
    leaf = int(np.setdiff1d(np.arange(eng.size), eng.parents())[-1])
    with pytest.raises(ValueError, match="doesn't exist"):
        eng.tree_retain(eng.size)
    with pytest.raises(ValueError, match="doesn't exist"):
        eng.tree_retain(-1)
    assert eng.size == 5001
    ref = _retain_and_compare(eng, s, leaf, True)
    assert ref["stats"]["kept"] == 1 and eng.size == 1
    # (this leaf sits where its edge was cut: as a root it cannot move, both sides spend their attempts and add nothing)
    _grow_and_compare(eng, s, ref, more=50, may_stall=True)
    # an early leaf of a smaller tree, in open water
    eng.tree_reset(s.x0)
    _seed(eng, 1)
    eng.extend(WAVE, max_attempts=20000, node_limit=600)
    leaf = int(np.setdiff1d(np.arange(eng.size), eng.parents())[0])
    ref = _retain_and_compare(eng, s, leaf, True)
    assert ref["stats"]["kept"] == 1
    _grow_and_compare(eng, s, ref, more=100, may_stall=True)
    eng.close()


def _other_world(name):
    """(system, nodes to grow, horizon, change): `change(system, engine)` alters the world between growth and retain."""
    import lqrrt_amd
    S = lqrrt_amd.systems

    def far_node(eng, dims):
        """state of the node farthest from the root: an obstacle there cuts the end of a branch, not the root's surroundings"""
        x = eng.states()
        return x[int(np.argmax(np.linalg.norm(x[:, :dims] - x[0, :dims], axis=1)))]

    def circle_on_a_node(r):
        def change(s, eng):
            at = far_node(eng, 2)
            s.set_obstacles(np.vstack((np.asarray(s.obs, dtype=np.float64).reshape(-1, 3), [at[0], at[1], r])))
        return change
    if name == "car":
        return S.Car(0), 1200, None, circle_on_a_node(1.0)
    if name == "boat_novice_lqr":
        return S.BoatNoviceLqr(0), 500, None, circle_on_a_node(2.0)
    if name == "boat_advanced_adaptive":
        return S.BoatAdvanced(0), 1500, (0.5, 2.0), circle_on_a_node(2.0)
    if name == "double_integrator":
        def boxes(s, eng):
            at = far_node(eng, 3)[:3]
            s.set_obstacles(np.vstack((s.obs, np.concatenate((at - 3.0, at + 3.0)))))
        return S.DoubleIntegrator(n_boxes=1000, seed=0), 1500, None, boxes
    if name == "ros_boat":
        g = np.load(os.path.join(GOLDEN, "ros_boat.npz"))
        s = S.RosBoat("boat")
        grid = np.array(g["grid"])
        s.set_occupancy_grid(grid, g["origin"], cpm=float(g["cpm"]), threshold=float(g["threshold"]))
        s.goal = [float(v) for v in g["goal"]]
        s.sample_space = [tuple(r) for r in g["sample_space"]]
        s.x0 = np.array(g["state"][0], dtype=np.float64)

        def occupy(s, eng):
            at = far_node(eng, 2)
            cpm = float(g["cpm"])
            ix, iy = int(cpm * (at[0] - g["origin"][0])), int(cpm * (at[1] - g["origin"][1]))
            new = grid.copy()
            k = max(int(2.0 * cpm), 1)
            new[max(iy - k, 0):iy + k + 1, max(ix - k, 0):ix + k + 1] = 100
            s.set_occupancy_grid(new, g["origin"], cpm=cpm, threshold=float(g["threshold"]))
        return s, 1200, None, occupy
    raise KeyError(name)


@pytest.mark.parametrize("name", ["car", "boat_novice_lqr", "double_integrator", "ros_boat", "boat_advanced_adaptive"])
def test_other_systems_bit_for_bit(name):
    """Circles under a hull (car), Riccati gains (boat_novice_lqr), boxes through the CSR grid (double integrator), an occupancy
    grid that changes between plan and retain (ROS boat), the adaptive horizon (edges of up to hspan[1] rows)."""
    s, nodes, horizon, change = _other_world(name)
    eng = _engine(s, nodes + 2 * WAVE + 8, horizon=horizon, seed=3)
    eng.tree_reset(s.x0)
    eng.extend(WAVE, max_attempts=60 * nodes, node_limit=nodes)
    assert eng.size > nodes // 2, eng.size
    N = eng.size
    change(s, eng)
    assert eng.sync_geometry()
    ref = _retain_and_compare(eng, s, 0, True, oracle=_oracle(s, 16, 3, horizon=horizon))
    st = ref["stats"]
    assert st["infeasible"] > 0 and st["kept"] > 1 and st["kept"] + st["outside"] + st["infeasible"] + st["orphaned"] == N
    if not isinstance(_hspan(s, horizon), tuple):
        _grow_and_compare(eng, s, ref, more=300, may_stall=True)
    else:
        # the heuristic's horizon state is the engine's own and is not touched by a retain; the oracle starts from it
        import coracle
        kw = s.plan_kwargs
        H = _hspan(s, horizon)
        state = eng.horizon_iters_state()
        kept, more = st["kept"], 300
        o = coracle.COracle(s, kept + more + 2 * WAVE + 8)
        o.configure(kw["dt"], kw["FPR"], H[1], s.error_tol, s.goal, s.goal_buffer, s.sample_space, s.goal_bias, 10)
        o.set_adaptive(H[0], H[1], state)
        o.seed(9)
        o.reset(s.x0)
        o.load_tree(ref["state"], ref["K"], ref["pID"], ref["ignored"])
        _seed(eng, 9)
        eng.extend(WAVE, max_attempts=40 * more, node_limit=kept + more - 1)
        o.extend(max_iters=40 * more, max_nodes=kept + more - 1)
        np.testing.assert_array_equal(eng.parents(), o.parents())
        np.testing.assert_array_equal(eng.states(), o.states())
        np.testing.assert_array_equal(eng.ignored(), o.ignored())
    # the grown tree again: from a node in its middle, under the same new map, then from the parent of its last node as it is
    pid = eng.parents()
    mid = eng.size // 2
    _retain_and_compare(eng, s, int(pid[pid[mid]]) if pid[mid] > 0 else mid, True, oracle=_oracle(s, 16, 3, horizon=horizon))
    if eng.size > 1:
        _retain_and_compare(eng, s, int(eng.parents()[eng.size - 1]), False)
    eng.close()


def test_retain_at_full_capacity_and_footprint():
    """A tree that fills the engine's capacity is retained (the scratch does not live in the pools), and the footprint is the
    same afterwards: every buffer of a retain is transient."""
    import lqrrt_amd
    from lqrrt_amd import _native as nat
    s = lqrrt_amd.systems.Car(0)
    eng = _engine(s, 900, wave=64, seed=2)
    eng.tree_reset(s.x0)
    eng.extend(64, node_limit=700)
    x0, K0 = np.ascontiguousarray(s.x0, dtype=np.float64), np.ascontiguousarray(eng.gains(0, 1)[0])
    while True:
        rc = nat.lib().lqrrt_tree_append(eng.h, 0, nat.ptr(x0), nat.ptr(K0), 1, None, None, eng._stream())
        if rc == nat.E_CAPACITY:
            break
        nat.check(rc)
    full = eng.size
    assert full >= 900
    fp = eng.footprint()
    ref = _retain_and_compare(eng, s, 0, True)
    assert ref["stats"]["kept"] == full
    pid = eng.parents()
    ref = _retain_and_compare(eng, s, int(pid[pid[600]]) or 1, True)
    assert 1 <= ref["stats"]["kept"] < full
    assert eng.footprint() == fp
    eng.close()


# ---------------------------------------------------------------------------------------------- Planner.replan

def _planner(s, max_nodes=5000, **over):
    import lqrrt_amd as lqrrt
    cons = lqrrt.Constraints(s.nstates, s.ncontrols, s.goal_buffer, s.is_feasible)
    kw = dict(s.plan_kwargs)
    kw.update(error_tol=s.error_tol, erf=s.erf, min_time=2, max_time=3, max_nodes=max_nodes, goal0=s.goal,
              sys_time=lambda: 0.0, printing=False, wave_size=WAVE)
    kw.update(over)
    return lqrrt.Planner(s.dynamics, s.lqr, cons, **kw)


def _check_plan(p):
    assert p.tree.climb(p.node_seq[-1]) == list(p.node_seq) and p.node_seq[0] == 0
    x_seq, u_seq = p.tree.trajectory(p.node_seq)
    assert np.array_equal(np.array(x_seq), np.array(p.x_seq)) and np.array_equal(np.array(u_seq), np.array(p.u_seq))
    assert p.T == len(p.x_seq) * p.dt and np.array_equal(p.t_seq, np.arange(len(p.x_seq)) * p.dt)
    assert p._engine.feasible_batch(np.array(p.x_seq)).all()


def test_replan_keeps_the_subtree_and_grows_it():
    """The clock stands still, so both plans end when the tree exceeds max_nodes (deterministic, as tests/test_hip_parity.py):
    the first plan is the 5001-node tree of scenario A, the replan from node 20 of its best plan keeps 2622 nodes under the new
    map and grows until the tree exceeds 5000 again -- the engine-level sequence, i.e. the C oracle given the kept tree."""
    import lqrrt_amd
    s = lqrrt_amd.systems.BoatAdvanced(0)
    p = _planner(s)
    np.random.seed(1)
    assert p.update_plan(s.x0, s.sample_space, goal_bias=s.goal_bias) is False   # ended by max_nodes
    eng = p._engine
    assert p.tree.size == 5001 and eng.plan_best() == (4363, 1261, 54)
    first_tree = p.tree                                                          # held: must stay what it was
    first_state, first_pid = first_tree.state.copy(), list(first_tree.pID)
    plan = _plan_of(eng)
    mid = eng.states(plan[45], 1)[0]
    s.set_obstacles(np.vstack((np.asarray(s.obs, dtype=np.float64).reshape(-1, 3), [mid[0] + 4.0, mid[1], 1.0])))   # replan syncs it
    arr = rr.engine_arrays(eng)
    lo, hi = rr.goal_box(s)
    o = _oracle(s, 5000 + 2 * WAVE + 8, 9)
    ref = rr.retain(*arr, plan[20], o.feasible, lo, hi)
    with pytest.raises(ValueError, match="doesn't exist"):
        p.replan(5001, s.sample_space, goal_bias=s.goal_bias)
    np.random.seed(9)
    assert p.replan(plan[20], s.sample_space, goal_bias=s.goal_bias) is False    # ended by max_nodes again
    assert p.retained == ref["stats"] and p.retained["kept"] == 2622
    assert p._engine is eng and p.tree is not first_tree and p.tree.on_device
    o.load_tree(ref["state"], ref["K"], ref["pID"], ref["ignored"])
    o.extend(max_nodes=5000)
    assert p.tree.size == eng.size == o.size == 5001
    np.testing.assert_array_equal(eng.parents(), o.parents())
    np.testing.assert_array_equal(eng.states(), o.states())
    np.testing.assert_array_equal(eng.gains(), o.gains())
    np.testing.assert_array_equal(eng.ignored(), o.ignored())
    np.testing.assert_array_equal(eng.states()[:2622], ref["state"])
    # the plan and the bookkeeping: the reference's rule over the final tree
    assert np.array_equal(p.x_seq[0], arr[0][plan[20]]) and np.array_equal(p.tree.state[0], arr[0][plan[20]])
    final = rr.retain(*rr.engine_arrays(eng), 0, None, lo, hi)["stats"]
    assert eng.plan_best() == (final["best_end"], final["best_steps"], final["goal_hits"])
    assert p.plan_reached_goal and final["goal_hits"] >= 28 and final["best_steps"] <= 1366
    _check_plan(p)
    k, node, tk = p.plan_node_after(0.5 * p.T)
    assert node == p.node_seq[k] and np.array_equal(p.x_seq[int(round(tk / p.dt))], p.tree.state[node])
    # the tree object of the first plan was detached, not overwritten
    assert not first_tree.on_device and first_tree.size == 5001
    np.testing.assert_array_equal(first_tree.state, first_state)
    assert list(first_tree.pID) == first_pid
    np.testing.assert_array_equal(np.array(first_tree.x_seq[plan[20]]), arr[4][plan[20], :arr[3][plan[20]]])
    # refine_plan works on the replanned tree
    size0, T0 = p.tree.size, p.T
    rounds = p.refine_plan(max_rounds=2)
    assert rounds >= 0 and p.tree.size >= size0 and p.T <= T0
    _check_plan(p)
    # a planner whose engine was recreated has no tree to keep
    p.set_runtime(max_nodes=4000)
    with pytest.raises(RuntimeError, match="no tree to keep"):
        p.replan(0, s.sample_space, goal_bias=s.goal_bias)
    p.set_runtime(max_nodes=5000)
    p.set_resolution(dt=2 * p.dt)
    with pytest.raises(RuntimeError, match="dt or horizon"):
        p.replan(0, s.sample_space, goal_bias=s.goal_bias)


def test_replan_revalidation_drops_the_best_plan():
    """From the old root under the new map the kept best plan is gone: the replan starts from the next best kept one and T gets
    longer.  specific_time=0 with a standing clock: the plan ends after its first native call, on a goal plan."""
    import lqrrt_amd
    s = lqrrt_amd.systems.BoatAdvanced(0)
    p = _planner(s)
    np.random.seed(1)
    p.update_plan(s.x0, s.sample_space, goal_bias=s.goal_bias)
    eng = p._engine
    end0, steps0, _ = eng.plan_best()
    assert (end0, steps0) == (4363, 1261)
    plan = _plan_of(eng)
    mid = eng.states(plan[45], 1)[0]
    s.set_obstacles(np.vstack((np.asarray(s.obs, dtype=np.float64).reshape(-1, 3), [mid[0] + 4.0, mid[1], 1.0])))
    np.random.seed(9)
    assert p.replan(0, s.sample_space, goal_bias=s.goal_bias, specific_time=0) is True
    r = p.retained
    assert (r["kept"], r["goal_hits"], r["infeasible"], r["orphaned"]) == (4383, 34, 147, 471) and r["best_steps"] == 1533
    end, steps, hits = eng.plan_best()
    assert hits >= 34 and steps <= 1533
    assert p.plan_reached_goal and p.node_seq[-1] == end and p.T == steps * p.dt
    assert p.T > steps0 * p.dt                                                   # longer than the plan the new obstacle cut
    assert p._in_goal(p.x_seq[-1])
    _check_plan(p)
    # without revalidation, from node 20 of the old best plan, that plan's tail is kept (a fresh identical first plan)
    s.set_obstacles(np.asarray(s.obs, dtype=np.float64).reshape(-1, 3)[:-1])
    q = _planner(s)
    np.random.seed(1)
    q.update_plan(s.x0, s.sample_space, goal_bias=s.goal_bias)
    ref = rr.retain(*rr.engine_arrays(q._engine), plan[20], None, *rr.goal_box(s))
    assert ref["stats"]["kept"] == 3240 and ref["old_ids"][ref["stats"]["best_end"]] == 4363
    np.random.seed(9)
    assert q.replan(plan[20], s.sample_space, goal_bias=s.goal_bias, specific_time=0, revalidate=False) is True
    assert q.retained == ref["stats"] and q.T <= ref["stats"]["best_steps"] * q.dt < 1261 * q.dt
