"""
Tree-wide goal connection on the device (csrc/connect.hpp through lqrrt_connect_search / lqrrt_connect_commit) against the
reference of the rule (tests/connect_reference.py, the C oracle's primitives), BIT FOR BIT: the winner (cost, node), and every
appended node's state, gain, parent, edge length and edge rows.  Then Planner.connect_goal end to end.
"""
import numpy as np
import pytest

import connect_reference as cr

pytestmark = pytest.mark.gpu


def _engine(s, g, size=None, extra=64):
    """The first `size` nodes of a fixture's tree on an engine (as tests/test_refine_gpu.py _engine loads the whole tree)."""
    from lqrrt_amd.engine import Engine
    kw = s.plan_kwargs
    N = len(g["state"]) if size is None else int(size)
    eng = Engine(s, capacity=N + extra, max_wave=64)
    el = np.array(g["edge_len"][:N], dtype=np.int32)
    el[0] = 1
    Hpool = max(int(np.max(el)), cr.horizon_of(s, g))
    eng.set_resolution(kw["dt"], kw["FPR"], Hpool, np.abs(np.asarray(s.error_tol, dtype=np.float64)), s.goal, s.goal_buffer)
    eng.tree_load(g["state"][:N], g["K"][:N], g["pID"][:N], edge_len=el)
    return eng


def _plan_cost(ref, g):
    return ref.cost([int(v) for v in g["node_seq"]])


def _compare_commit(eng, ref, win, H):
    """connect_commit against the reference's commit (the assertions of tests/test_refine_gpu.py _compare_refinement)."""
    ids = eng.connect_commit(win[1], H)
    plan, ids_ref = ref.commit_chain(win)
    assert ids == ids_ref
    first, k = ids[0], len(ids)
    assert np.array_equal(eng.states(first, k), np.array([ref.states[v] for v in ids]))
    assert np.array_equal(eng.gains(first, k), np.array([ref.K[v] for v in ids]))
    assert eng.parents(first, k).tolist() == [ref.pID[v] for v in ids]
    assert eng.edge_lengths(first, k).tolist() == [ref.elen[v] for v in ids]
    for v in ids:
        x, u = eng.edge(v)
        assert np.array_equal(x, ref.edges[v][0]) and np.array_equal(u, ref.edges[v][1]), v
    assert eng.climb(ids[-1]) == plan and eng.size == ref.size
    return plan, ids


# name, nodes loaded (None: the whole tree, the fixture plan's cost as incumbent), expected winner -- "ref": whatever the reference yields
CASES = [("car_2000", 217, (951, 211)),
         ("boat_novice_300", 107, (781, 77)),
         ("boat_novice_lqr_400", 144, (481, 73)),                   # Riccati gains
         ("boat_advanced_10k", 3308, (1707, 3305)),
         ("double_integrator_600", 5, (41, 0)),                     # box grid
         ("car_500", None, (951, 211)),
         ("boat_novice_lqr_400", None, (481, 73)),
         ("boat_advanced_10k", None, (1256, 5993)),                 # 10 001 candidates
         ("pendulum_lqr_120", None, None), ("boat_advanced_200", None, None), ("boat_advanced_3000", None, None),
         ("ros_boat", None, "ref")]                                 # occupancy grid


@pytest.mark.parametrize("name,size,expect", CASES)
def test_device_search_and_commit_match_reference(name, size, expect):
    s, g = cr.case(name)
    ref = cr.from_fixture(s, g, size)
    incumbent = cr.NO_INCUMBENT if size is not None else _plan_cost(ref, g)
    want = ref.search(incumbent=incumbent)
    eng = _engine(s, g, size)
    fp0 = eng.footprint()
    got = eng.connect_search(ref.H, incumbent)
    print(name, size, incumbent, got)
    assert got == (None if want is None else (want[0], want[1]))
    if expect != "ref":
        assert got == expect
    if want is not None:
        _compare_commit(eng, ref, want, ref.H)
        assert eng.connect_search(ref.H, want[0]) is None           # the tree with its new chain: nothing below the winner's cost
    assert eng.footprint() == fp0                                   # the depth table and the id list are scratch, not footprint
    eng.close()


def test_at_least_five_cases_have_a_winner():
    assert sum(1 for _, _, e in CASES if e not in (None, "ref")) >= 5


def test_device_search_over_an_id_list():
    s, g = cr.case("car_2000")
    ref = cr.from_fixture(s, g, 217)
    eng = _engine(s, g, 217)
    ids = np.random.RandomState(5).permutation(217)
    assert eng.connect_search(ref.H, cr.NO_INCUMBENT, nodes=ids) == (951, 211)
    assert eng.connect_search(ref.H, cr.NO_INCUMBENT, nodes=np.sort(ids)) == (951, 211)
    assert eng.connect_search(ref.H, 951, nodes=ids) is None        # the winner's own cost as incumbent: nothing shorter
    assert eng.connect_search(ref.H, 952, nodes=ids) == (951, 211)
    rest = [int(v) for v in ids if v != 211]
    want = ref.search(nodes=rest)
    assert eng.connect_search(ref.H, cr.NO_INCUMBENT, nodes=rest) == (want[0], want[1]) != (951, 211)
    assert eng.connect_search(ref.H, cr.NO_INCUMBENT, nodes=[]) is None
    with pytest.raises(ValueError):
        eng.connect_search(ref.H, cr.NO_INCUMBENT, nodes=[0, 217])
    with pytest.raises(ValueError):
        eng.connect_search(ref.H, 0)
    with pytest.raises(ValueError):
        eng.connect_search(ref.H + 10 ** 6, cr.NO_INCUMBENT)
    eng.close()


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
    """A full tree refuses the winner's chain with LQRRT_E_CAPACITY; tree and mirrors stay as they were."""
    from lqrrt_amd import _native as nat
    s, g = cr.case("car_2000")
    ref = cr.from_fixture(s, g, 217)
    eng = _engine(s, g, 217, extra=1)                               # (the winner's chain has two nodes)
    nodes = list(range(217))                                        # (the copies of the root that fill the tree are not candidates)
    full = _fill(eng, g["state"][0], g["K"][0])
    parents, lens = eng.parents(), eng.edge_lengths()
    assert eng.connect_search(ref.H, cr.NO_INCUMBENT, nodes=nodes) == (951, 211)
    with pytest.raises(nat.NativeError) as ex:
        eng.connect_commit(211, ref.H)
    assert ex.value.code == nat.E_CAPACITY and eng.size == full
    assert np.array_equal(eng.parents(), parents) and np.array_equal(eng.edge_lengths(), lens)
    assert eng.climb(211) == ref.climb(211)
    assert eng.connect_search(ref.H, cr.NO_INCUMBENT, nodes=nodes) == (951, 211)
    eng.close()


def test_device_commit_refuses_a_chain_that_misses_the_goal():
    from lqrrt_amd import _native as nat
    s, g = cr.case("car_2000")
    ref = cr.from_fixture(s, g, 217)
    assert ref.chain(0) is None                                     # eight steers from the root do not reach the goal box
    eng = _engine(s, g, 217)
    with pytest.raises(nat.NativeError) as ex:
        eng.connect_commit(0, ref.H)
    assert ex.value.code == nat.E_STATE and eng.size == 217
    assert eng.connect_search(ref.H, cr.NO_INCUMBENT) == (951, 211)
    eng.close()


def test_retain_sees_the_committed_chain_as_a_goal_hit():
    s, g = cr.case("car_2000")
    ref = cr.from_fixture(s, g, 217)
    eng = _engine(s, g, 217)
    win = ref.search()
    plan, ids = _compare_commit(eng, ref, win, ref.H)
    stats, old_to_new = eng.tree_retain(0, revalidate=False)
    assert stats["kept"] == 219 and old_to_new[:219].tolist() == list(range(219))
    assert stats["goal_hits"] >= 1 and stats["best_end"] == ids[-1] and stats["best_steps"] == win[0] == 951
    eng.close()


def _car_planner(max_nodes, finish=False, seed=1, **kw):
    import lqrrt_amd
    s = lqrrt_amd.systems.Car(0)
    cons = lqrrt_amd.Constraints(s.nstates, s.ncontrols, s.goal_buffer, s.is_feasible)
    p = lqrrt_amd.Planner(s.dynamics, s.lqr, cons, error_tol=s.error_tol, erf=s.erf, goal0=s.goal, printing=False,
                          max_nodes=max_nodes, wave_size=256, **dict(s.plan_kwargs, **kw))
    np.random.seed(seed)
    p.update_plan(s.x0, s.sample_space, goal_bias=s.goal_bias, xrand_gen=10, finish_on_goal=finish)
    return s, p


def _reference_of(s, p):
    eng = p._engine
    return cr.Connector(s, eng.states(), eng.gains(), eng.parents(), eng.edge_lengths(), p.horizon_iters)


def test_connect_goal_rescues_a_fallback_plan():
    """The fixture's recipe (seed 1, a clock that stands still, ended by the node limit) with max_nodes below the fixture's first goal
    node: the plan is the fallback.  connect_goal replaces it with the reference's winner on the tree the run grew."""
    s, p = _car_planner(215, min_time=2, max_time=3, sys_time=lambda: 0.0)
    eng = p._engine
    assert not p.plan_reached_goal and eng.size == 216 and not p._in_goal(p.x_seq[-1])
    ref = _reference_of(s, p)
    win = ref.search()
    print("fallback tree of %d nodes: reference winner %s" % (ref.size, None if win is None else win[:2]))
    assert win is not None
    plan_ref, ids_ref = ref.commit_chain(win)
    assert p.connect_goal() is True
    assert p.plan_reached_goal and p.node_seq == plan_ref and p.tree.size == eng.size == ref.size
    assert p._in_goal(p.x_seq[-1]) and p.T == win[0] * p.dt and len(p.x_seq) == win[0]
    assert p.node_seq[0] == 0 and p.tree.climb(p.node_seq[-1]) == p.node_seq
    assert all(p.tree.pID[b] == a for a, b in zip(p.node_seq, p.node_seq[1:]))
    x_seq, u_seq = p.tree.trajectory(p.node_seq)
    assert np.array_equal(np.array(x_seq), np.array(p.x_seq)) and np.array_equal(np.array(u_seq), np.array(p.u_seq))
    assert np.array_equal(p.t_seq, np.arange(len(p.x_seq)) * p.dt)
    assert np.array_equal(np.array(p.x_seq[-len(ref.edges[ids_ref[-1]][0]):]), ref.edges[ids_ref[-1]][0])
    assert np.array_equal(p.get_state(p.T), p.x_seq[-1]) and np.array_equal(p.get_state(p.T + 1.0), p.x_seq[-1])
    assert np.array_equal(eng.states(ids_ref[0], len(ids_ref)), np.array([ref.states[v] for v in ids_ref]))
    # a second call finds nothing below the plan it has just made
    seq, T = list(p.node_seq), p.T
    assert p.connect_goal() is False and p.node_seq == seq and p.T == T and p.tree.size == ref.size
    # refine_plan works on the new plan, as the refinement's reference does
    plan_refined, log = ref.refine(plan_ref)
    assert p.refine_plan() == len(log) and p.node_seq == plan_refined
    assert p.T == ref.cost(plan_refined) * p.dt and p._in_goal(p.x_seq[-1])


def test_connect_goal_finish_on_goal_request():
    """finish_on_goal=True on a fallback plan: the exact-goal steer runs from the chain's last node."""
    s, p = _car_planner(215, min_time=2, max_time=3, sys_time=lambda: 0.0)
    ref = _reference_of(s, p)
    win = ref.search()
    plan_ref, _ = ref.commit_chain(win)
    assert p.connect_goal(finish_on_goal=True) is True
    assert p.node_seq[:len(plan_ref)] == plan_ref and p.T == win[0] * p.dt
    if len(p.node_seq) > len(plan_ref):                             # (the force-arrive steer may produce nothing)
        assert p.node_seq[-1] == p.tree.size - 1 and p.tree._host_nodes() == 1
        assert np.array_equal(p.tree.state[p.node_seq[-1]], s.goal)
    assert p.connect_goal() is False


def test_connect_goal_with_a_finish_node():
    """A plan that ends in a finish_on_goal node is left unchanged, or replaced with the finish node run again: whichever the reference
    predicts for the device tree under the plan's cost without that node."""
    for seed in range(1, 9):
        s, p = _car_planner(3000, finish=True, seed=seed, min_time=0.0, max_time=10)
        assert p.plan_reached_goal
        eng = p._engine
        goal_node = p.node_seq[-1]
        if goal_node < eng.size:                                    # the force-arrive steer produced nothing: no goal node
            continue
        ref = _reference_of(s, p)
        core = p.node_seq[:-1]
        win = ref.search(incumbent=ref.cost(core))
        seq, T, size = list(p.node_seq), p.T, p.tree.size
        print("seed %d: plan of %d steps, reference winner %s" % (seed, ref.cost(core), None if win is None else win[:2]))
        if win is None:
            assert p.connect_goal() is False
            assert p.node_seq == seq and p.T == T and p.tree.size == size
        else:
            plan_ref, _ = ref.commit_chain(win)
            assert p.connect_goal() is True
            assert p.node_seq[:len(plan_ref)] == plan_ref and p.T == win[0] * p.dt < T
            if len(p.node_seq) > len(plan_ref):                     # the finish node, run again from the new end
                assert p.node_seq[-1] == p.tree.size - 1 and p.tree._host_nodes() == 1
                assert np.array_equal(p.tree.state[p.node_seq[-1]], s.goal)
            else:
                assert p.tree._host_nodes() == 0
        return
    pytest.fail("no finish_on_goal plan of the car in 8 seeds")


def test_connect_goal_stops_at_capacity():
    """A tree filled to its capacity cannot hold the chain: connect_goal returns False and the plan is untouched."""
    s, p = _car_planner(215, min_time=2, max_time=3, sys_time=lambda: 0.0)
    eng = p._engine
    seq, T = list(p.node_seq), p.T
    _fill(eng, s.x0, eng.gains(0, 1)[0])
    assert p.connect_goal(nodes=list(range(216))) is False
    assert p.node_seq == seq and p.T == T and not p.plan_reached_goal


def test_example_runs():
    """examples/connect_goal_gpu.py: the budget runs out before the first goal hit, connect_goal finds a plan, refine_plan shortens it."""
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "connect_goal_gpu.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    T = [float(v) for v in re.findall(r"T = ([0-9.]+) s", out.stdout)]
    assert "budget spent: tree of 216 nodes, reached goal: False" in out.stdout
    assert re.search(r"connect_goal in [0-9.]+ ms: True, reached goal: True", out.stdout)
    assert len(T) == 3 and T[1] == 95.1 and T[2] <= T[1]


def test_connect_goal_refusals_on_a_live_tree():
    """Hand-added nodes: refine_plan's RuntimeError.  A goal changed since the tree was grown: the engine's goal box is the old one."""
    s, p = _car_planner(215, min_time=2, max_time=3, sys_time=lambda: 0.0)
    seq = list(p.node_seq)
    p.tree.add_node(0, s.x0, None, [np.array(s.x0)], [np.zeros(s.ncontrols)])
    with pytest.raises(RuntimeError, match="add_node"):
        p.connect_goal()
    p.tree._drop_host_tail()
    goal = np.array(s.goal, dtype=np.float64)
    p.set_goal(goal + 1.0)
    with pytest.raises(RuntimeError, match="goal changed"):
        p.connect_goal()
    p.set_goal(goal)
    assert p.node_seq == seq and p.connect_goal() is True
