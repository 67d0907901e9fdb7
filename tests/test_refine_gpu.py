"""
Plan refinement on the device (csrc/refine.hpp through lqrrt_refine_search / lqrrt_refine_commit) against the reference of
the rule (tests/refine_reference.py, the C oracle's primitives), BIT FOR BIT: the winner (cost, i, j) of every round, and every
appended node's state, gain, parent, edge length and edge rows.  Then Planner.refine_plan end to end.
"""
import os

import numpy as np
import pytest

import refine_reference as rr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _case(name):
    """(system, fixture, goal-buffer factor) of a committed fixture whose final tree and plan are refined."""
    import lqrrt_amd
    S = lqrrt_amd.systems
    if name == "ros_boat":
        g = np.load(os.path.join(GOLDEN, "ros_boat.npz"))
        s = S.RosBoat("boat")
        s.set_occupancy_grid(g["grid"], g["origin"], cpm=float(g["cpm"]), threshold=float(g["threshold"]))
        s.goal = [float(v) for v in g["goal"]]
        s.sample_space = [tuple(r) for r in g["sample_space"]]
        return s, g
    g = np.load(os.path.join(GOLDEN, "traj_%s.npz" % name))
    if name.startswith("double_integrator"):
        return S.DoubleIntegrator(n_boxes=int(g["n_boxes"]), seed=int(g["box_seed"])), g
    return S.SYSTEMS[name.rsplit("_", 1)[0]](0), g


def _engine(s, g, goal_buffer, extra=64):
    from lqrrt_amd.engine import Engine
    kw = s.plan_kwargs
    N = len(g["state"])
    eng = Engine(s, capacity=N + extra, max_wave=64)
    Hpool = max(int(np.max(g["edge_len"])), rr.from_fixture(s, g)[0].H)
    eng.set_resolution(kw["dt"], kw["FPR"], Hpool, np.abs(np.asarray(s.error_tol, dtype=np.float64)), s.goal, goal_buffer)
    el = np.array(g["edge_len"], dtype=np.int32)
    el[0] = 1
    eng.tree_load(g["state"], g["K"], g["pID"], edge_len=el)
    return eng


def _compare_refinement(name, factor=1.0, max_rounds=8):
    s, g = _case(name)
    buf = factor * np.abs(np.asarray(s.goal_buffer, dtype=np.float64))
    ref, plan = rr.from_fixture(s, g, goal_buffer=buf)
    eng = _engine(s, g, buf)
    H = ref.H
    rounds = []
    for _ in range(max_rounds):
        C = ref.cost(plan)
        want = ref.round(plan)
        got = eng.refine_round(plan, H, C)
        assert got == (None if want is None else tuple(want[:3])), (name, len(rounds))
        if want is None:
            break
        ids = eng.refine_commit(plan, H, got[1], got[2])
        plan, ids_ref = ref.commit(plan, want)
        assert ids == ids_ref
        first, k = ids[0], len(ids)
        assert np.array_equal(eng.states(first, k), np.array([ref.states[v] for v in ids]))
        assert np.array_equal(eng.gains(first, k), np.array([ref.K[v] for v in ids]))
        assert eng.parents(first, k).tolist() == [ref.pID[v] for v in ids]
        assert eng.edge_lengths(first, k).tolist() == [ref.elen[v] for v in ids]
        for v in ids:
            x, u = eng.edge(v)
            assert np.array_equal(x, ref.edges[v][0]) and np.array_equal(u, ref.edges[v][1]), (name, v)
        assert eng.climb(plan[-1]) == plan
        rounds.append(want[:3])
    eng.close()
    return rounds


@pytest.mark.parametrize("name,factor,max_rounds,expect", [
    ("car_500", 1.0, 8, [(551, 2, 12), (501, 0, 1), (496, 0, 1)]),
    ("car_2000", 1.0, 8, [(601, 2, 5)]),
    ("boat_novice_300", 1.0, 8, [(679, 23, 43), (678, 29, 33)]),
    ("boat_novice_firstgoal", 1.0, 8, [(741, 23, 29)]),
    ("boat_advanced_10k", 1.0, 1, []),                              # 113 plan nodes, 6 328 candidates, none reaches the goal box
    ("boat_advanced_10k", 2.0, 2, [(501, 41, 46)]),                 # ... twice as wide a box: one winner, then none
    # Riccati gains (DareLds in the workgroup's GainLds) on every step of every chain and in the appended nodes; the searched chains
    # hold FPR-cut edges (about one edge in ten), whose end gain is evaluated again:
    ("boat_novice_lqr_400", 1.0, 8, [(450, 0, 14)]),                 # 23 appended nodes
    ("boat_novice_lqr_400", 2.0, 8, [(390, 0, 14), (387, 18, 19)]),
    ("pendulum_lqr_120", 1.0, 2, []),                               # a fallback plan (no goal hit): no chain reaches the goal box
    ("double_integrator_600", 1.0, 8, [(41, 0, 18), (38, 0, 1), (36, 0, 1), (21, 0, 1)]),
    ("ros_boat", 1.0, 8, [(481, 5, 38), (465, 0, 3), (464, 9, 15)]),
])
def test_device_rounds_match_reference(name, factor, max_rounds, expect):
    assert _compare_refinement(name, factor, max_rounds) == expect


def _fill(eng, x0, K0):
    """Appends copies of the root until the engine's tree is full; returns its size then."""
    from lqrrt_amd import _native as nat
    x0, K0 = np.ascontiguousarray(x0, dtype=np.float64), np.ascontiguousarray(K0, dtype=np.float64)
    while True:
        rc = nat.lib().lqrrt_tree_append(eng.h, 0, nat.ptr(x0), nat.ptr(K0), 1, None, None, eng._stream())
        if rc == nat.E_CAPACITY:
            return eng.size
        nat.check(rc)


def test_device_commit_capacity_stop():
    """A full tree refuses the winner's chain with LQRRT_E_CAPACITY and stays as it was."""
    from lqrrt_amd import _native as nat
    s, g = _case("car_500")
    ref, plan = rr.from_fixture(s, g)
    eng = _engine(s, g, np.abs(np.asarray(s.goal_buffer, dtype=np.float64)), extra=5)
    full = _fill(eng, g["state"][0], g["K"][0])
    want = ref.round(plan)
    assert eng.refine_round(plan, ref.H, ref.cost(plan)) == tuple(want[:3])
    with pytest.raises(nat.NativeError) as ex:
        eng.refine_commit(plan, ref.H, want[1], want[2])
    assert ex.value.code == nat.E_CAPACITY and eng.size == full
    assert eng.climb(plan[-1]) == plan and eng.refine_round(plan, ref.H, ref.cost(plan)) == tuple(want[:3])
    eng.close()


def _planner(name="car", finish=False, seed=3, **kw):
    import lqrrt_amd
    s = lqrrt_amd.systems.SYSTEMS[name](0)
    cons = lqrrt_amd.Constraints(s.nstates, s.ncontrols, s.goal_buffer, s.is_feasible)
    p = lqrrt_amd.Planner(s.dynamics, s.lqr, cons, error_tol=s.error_tol, erf=s.erf, goal0=s.goal, printing=False,
                          min_time=0.0, max_time=10, max_nodes=kw.pop("max_nodes", 3000), wave_size=256, **s.plan_kwargs)
    np.random.seed(seed)
    p.update_plan(s.x0, s.sample_space, goal_bias=s.goal_bias, finish_on_goal=finish)
    assert p.plan_reached_goal
    return s, p


def _check_plan(s, p, finish=False):
    x_seq, u_seq = p.tree.trajectory(p.node_seq)
    assert p.tree.climb(p.node_seq[-1]) == list(p.node_seq)
    assert np.array_equal(np.array(x_seq), np.array(p.x_seq)) and np.array_equal(np.array(u_seq), np.array(p.u_seq))
    assert np.array_equal(p.t_seq, np.arange(len(p.x_seq)) * p.dt)
    if not finish:                                                  # (the finish_on_goal edge is not part of T, planner.py:294-303)
        assert p.T == len(p.x_seq) * p.dt
    assert p._engine.feasible_batch(np.array(p.x_seq)).all()
    assert np.array_equal(p.get_state(len(p.x_seq) * p.dt + 1.0), p.x_seq[-1])


def _reference_of(s, p):
    """The reference's refinement of the planner's own tree and plan (without a finish_on_goal node)."""
    eng = p._engine
    ref = rr.Refiner(s, eng.states(), eng.gains(), eng.parents(), eng.edge_lengths(), p.horizon_iters)
    plan = [v for v in p.node_seq if v < eng.size]
    return ref, ref.refine(plan)


@pytest.mark.parametrize("name", ["car", "boat_novice"])
def test_refine_plan_end_to_end(name):
    accepted = 0
    for seed in range(1, 7):
        s, p = _planner(name, seed=seed)
        T0, size0 = p.T, p.tree.size
        ref, (plan_ref, log) = _reference_of(s, p)
        rounds = p.refine_plan()
        assert rounds == len(log) and p.node_seq == plan_ref, seed
        assert p.tree.size == size0 + sum(len(ids) for _, _, _, ids in log)
        assert p.T <= T0 and (p.T < T0) == (rounds > 0)
        assert p._in_goal(p.x_seq[-1])
        _check_plan(s, p)
        if rounds:
            assert np.array_equal(np.array(p.x_seq[-len(ref.edges[plan_ref[-1]][0]):]), ref.edges[plan_ref[-1]][0])
            T1 = p.T
            assert p.refine_plan() == 0 and p.T == T1               # at the fix-point (or max_rounds): nothing changes
        accepted += rounds
        if accepted >= 2:
            break
    assert accepted >= 1


def test_refine_plan_finish_on_goal():
    for seed in range(1, 9):
        s, p = _planner("car", finish=True, seed=seed)
        goal_node = p.node_seq[-1]
        if goal_node < p._engine.size:                              # the force-arrive steer produced nothing: no goal node
            continue
        assert np.array_equal(p.tree.state[goal_node], s.goal)
        core0 = 1 + sum(p._engine.edge_lengths()[v] for v in p.node_seq[1:-1])
        _, (plan_ref, log) = _reference_of(s, p)
        rounds = p.refine_plan()
        assert rounds == len(log)
        if not rounds:
            assert p.node_seq[-1] == goal_node
            continue
        plan = p.node_seq
        assert plan[:-1] == plan_ref
        assert np.array_equal(p.tree.state[plan[-1]], s.goal) and plan[-1] == p.tree.size - 1    # a new goal node, on the new end
        assert p.tree._host_nodes() == 1
        core1 = 1 + sum(p._engine.edge_lengths()[v] for v in plan[1:-1])
        assert core1 < core0 and p.T == core1 * p.dt
        _check_plan(s, p, finish=True)
        return
    pytest.fail("no finish_on_goal plan of the car with a shorter refinement in 8 seeds")


def test_refine_plan_stops_at_capacity():
    """A tree filled to its capacity cannot hold any chain: refine_plan returns 0 and the plan is untouched."""
    s, p = _planner("car", max_nodes=1500)
    eng = p._engine
    plan, T0 = list(p.node_seq), p.T
    _fill(eng, s.x0, eng.gains(0, 1)[0])
    assert p.refine_plan() == 0
    assert p.node_seq == plan and p.T == T0


def test_refine_plan_adopts_accepted_rounds_when_a_call_fails():
    """A native failure in a later round: the rounds accepted before it stay adopted (plan, tree, interpolators), then it raises."""
    from lqrrt_amd import _native as nat
    s, p = _planner("car", seed=1)
    _, (plan_ref, log) = _reference_of(s, p)
    assert len(log) >= 2
    plan0, eng = list(p.node_seq), p._engine
    calls = []
    commit = eng.refine_commit

    def failing_commit(*a, **kw):
        calls.append(1)
        if len(calls) == 2:
            raise nat.NativeError(nat.E_HIP, "injected failure")
        return commit(*a, **kw)
    eng.refine_commit = failing_commit
    try:
        with pytest.raises(nat.NativeError, match="injected"):
            p.refine_plan()
    finally:
        del eng.refine_commit
    c, i, j, ids = log[0]
    assert p.node_seq == plan0[:i + 1] + ids and p.tree.size == eng.size
    assert p.T == c * p.dt
    _check_plan(s, p)


def test_refine_search_plan_size_limit():
    """One launch holds at most 2^32 threads: a plan of 11 587 nodes (67 M candidates) is refused with LQRRT_E_ARG (ValueError)."""
    from lqrrt_amd.engine import Engine
    import lqrrt_amd
    s = lqrrt_amd.systems.Car(0)
    kw = s.plan_kwargs
    P = 11587
    eng = Engine(s, capacity=P + 8, max_wave=64)
    eng.set_resolution(kw["dt"], kw["FPR"], 50, np.abs(np.asarray(s.error_tol, dtype=np.float64)), s.goal, s.goal_buffer)
    eng.tree_load(np.tile(s.x0, (P, 1)), np.zeros((P, s.ncontrols, s.nstates)), np.arange(-1, P - 1))
    with pytest.raises(ValueError, match="exceed one launch"):
        eng.refine_round(list(range(P)), 50, 10 ** 6)
    eng.close()
