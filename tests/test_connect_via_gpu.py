"""
Goal chains through waypoints on the device (csrc/connect_via.hpp through lqrrt_connect_via_search / lqrrt_connect_via_commit)
against the reference of the rule (tests/connect_via_reference.py, the C oracle's primitives), BIT FOR BIT: the winner
(cost, node, j), and every appended node's state, gain, parent, edge length and edge rows, the climb and the size.  Then
Planner.connect_via end to end, and the search on a tree after Engine.tree_retain.
"""
import ctypes as C

import numpy as np
import pytest

import connect_reference as cr
import connect_via_reference as cvr

ROWS, row_inputs = cvr.ROWS, cvr.row_inputs

pytestmark = pytest.mark.gpu


def _engine(s, g, size=None, extra=64):
    """The first `size` nodes of a fixture's tree on an engine (tests/test_connect_gpu.py _engine)."""
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


def _compare_commit(eng, ref, win, way, H, tries=8):
    """connect_via_commit against the reference's commit (the assertions of tests/test_connect_gpu.py _compare_commit)."""
    ids = eng.connect_via_commit(win[1], win[2], way, H, tries)
    plan, ids_ref = ref.commit_via(win)
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


def _search_and_commit(s, g, ref, way, size, tries, expect=None):
    want = ref.search_via(way, goal_tries=tries)
    eng = _engine(s, g, size)
    fp0 = eng.footprint()
    got = eng.connect_via_search(way, ref.H, cvr.NO_INCUMBENT, tries)
    print(size, len(way), tries, got)
    assert got == (None if want is None else want[:3])
    if expect is not None:
        assert got == expect
    if want is not None:
        _compare_commit(eng, ref, want, way, ref.H, tries)
        # nothing below the winner's cost from the nodes that were searched (the appended nodes are new candidates: they may do better)
        assert eng.connect_via_search(way, ref.H, want[0], tries, nodes=np.arange(size)) is None
    assert eng.footprint() == fp0                                   # depth table, id list, waypoints and key are scratch
    eng.close()
    return want


@pytest.mark.parametrize("name,size,way_ids,tries,connect,winner,lens", ROWS)
def test_worked_rows_match_reference(name, size, way_ids, tries, connect, winner, lens):
    s, g, ref, way = row_inputs(name, size, way_ids)
    _search_and_commit(s, g, ref, way, size, tries, expect=winner)


def _beyond(name):
    """A fixture cut before its first goal node, the waypoints its plan's nodes beyond the cut."""
    s, g = cr.case(name)
    size = cr.first_goal_node(s, g)
    ids, way = cvr.plan_states(g, size)
    assert len(ids) >= 1
    return s, g, cvr.from_fixture(s, g, size), way, size


@pytest.mark.parametrize("name", ["boat_novice_lqr_400",             # the Riccati gain in GainLds under varying targets
                                  "double_integrator_600"])          # box grid, 12 states
def test_further_models_match_reference(name):
    s, g, ref, way, size = _beyond(name)
    want = _search_and_commit(s, g, ref, way, size, 8)
    assert want is not None


def test_no_waypoints_is_connect_search_bit_for_bit():
    s, g = cr.case("car_2000")
    ref = cvr.from_fixture(s, g, 217)
    a, b = _engine(s, g, 217), _engine(s, g, 217)
    none = np.zeros((0, s.nstates))
    assert a.connect_search(ref.H, cr.NO_INCUMBENT) == (951, 211)
    assert b.connect_via_search(none, ref.H, cr.NO_INCUMBENT) == (951, 211, 0)
    one = a.connect_search(ref.H, cr.NO_INCUMBENT, goal_tries=1)
    assert b.connect_via_search([], ref.H, cr.NO_INCUMBENT, goal_tries=1) == (None if one is None else one + (0,))
    ids_a, ids_b = a.connect_commit(211, ref.H), b.connect_via_commit(211, 0, none, ref.H)
    assert ids_a == ids_b == [217, 218] and a.size == b.size == 219
    assert np.array_equal(a.states(), b.states()) and np.array_equal(a.gains(), b.gains())
    assert np.array_equal(a.parents(), b.parents()) and np.array_equal(a.edge_lengths(), b.edge_lengths())
    for v in ids_a:
        assert all(np.array_equal(p, q) for p, q in zip(a.edge(v), b.edge(v)))
    assert a.climb(218) == b.climb(218)
    a.close()
    b.close()


def test_incumbent_edge_and_order_independence():
    s, g, ref, way = row_inputs("car_500", 217, [217])
    eng = _engine(s, g, 217)
    H = ref.H
    assert eng.connect_via_search(way, H, cvr.NO_INCUMBENT, 1) == (1050, 213, 0)
    assert eng.connect_via_search(way, H, 1050, 1) is None          # the winner's own cost as incumbent: nothing shorter
    assert eng.connect_via_search(way, H, 1051, 1) == (1050, 213, 0)
    ids = np.random.RandomState(5).permutation(217)
    for lst in (ids, ids[::-1], np.sort(ids)[::-1], np.concatenate((ids, ids[:40], [213, 213]))):
        assert eng.connect_via_search(way, H, cvr.NO_INCUMBENT, 1, nodes=lst) == (1050, 213, 0)
    rest = [int(v) for v in ids if v != 213]
    want = ref.search_via(way, goal_tries=1, nodes=rest)
    assert eng.connect_via_search(way, H, cvr.NO_INCUMBENT, 1, nodes=rest) == (None if want is None else want[:3]) != (1050, 213, 0)
    assert eng.connect_via_search(way, H, cvr.NO_INCUMBENT, 1, nodes=[]) is None
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


def _raw_search(eng, nodes, way, Q, tries, H, incumbent=cvr.NO_INCUMBENT):
    from lqrrt_amd import _native as nat
    ids = None if nodes is None else np.ascontiguousarray(nodes, dtype=np.int32)
    way = np.ascontiguousarray(way, dtype=np.float64)
    cost, node, j = C.c_int64(), C.c_int32(), C.c_int32()
    return nat.lib().lqrrt_connect_via_search(eng.h, None if ids is None else nat.ptr(ids), 0 if ids is None else len(ids), nat.ptr(way), Q,
                                              tries, H, incumbent, C.byref(cost), C.byref(node), C.byref(j), eng._stream())


def test_refusals_leave_tree_and_footprint_unchanged():
    from lqrrt_amd import _native as nat
    s, g, ref, way = row_inputs("car_500", 217, [217])
    H = ref.H
    eng = _engine(s, g, 217, extra=1)                               # (the winner's chain has two nodes)
    nodes = list(range(217))                                        # (the copies of the root that fill the tree are not candidates)
    full = _fill(eng, g["state"][0], g["K"][0])
    fp0, parents, lens, states = eng.footprint(), eng.parents(), eng.edge_lengths(), eng.states()

    def unchanged():
        return eng.footprint() == fp0 and eng.size == full and np.array_equal(eng.parents(), parents) \
            and np.array_equal(eng.edge_lengths(), lens) and np.array_equal(eng.states(), states)
    assert _raw_search(eng, [0, 5, 3], way, 1, 1, H) == nat.E_ARG and unchanged()           # unsorted
    assert _raw_search(eng, [0, 3, 3], way, 1, 1, H) == nat.E_ARG and unchanged()           # not STRICTLY ascending
    assert _raw_search(eng, [0, full], way, 1, 1, H) == nat.E_ARG and unchanged()           # an id outside the tree
    bad = way.copy()
    for value in (np.nan, np.inf):
        bad[0, 1] = value
        assert _raw_search(eng, None, bad, 1, 1, H) == nat.E_ARG and unchanged()
        with pytest.raises(ValueError):
            eng.connect_via_commit(213, 0, bad, H, 1)
    with pytest.raises(ValueError):
        eng.connect_via_search(np.zeros((1, s.nstates + 1)), H, cvr.NO_INCUMBENT)           # wrong width
    with pytest.raises(ValueError):
        eng.connect_via_search(way[0], H, cvr.NO_INCUMBENT)                                 # one state, not a table
    with pytest.raises(ValueError):
        eng.connect_via_commit(213, 0, np.zeros((1, s.nstates - 1)), H)
    assert _raw_search(eng, None, way, 1, 0, H) == nat.E_ARG and unchanged()                # goal_tries = 0
    assert _raw_search(eng, None, way, 1, 1, H + 10 ** 6) == nat.E_ARG and unchanged()      # a horizon beyond the pools
    assert _raw_search(eng, None, way, 1, 1, H, incumbent=0) == nat.E_ARG and unchanged()
    many = np.zeros((2 ** 26 // full + 1, s.nstates))                                       # more candidates than one launch
    assert _raw_search(eng, None, many, len(many), 1, H) == nat.E_ARG and unchanged()
    with pytest.raises(ValueError):
        eng.connect_via_commit(213, 2, way, H, 1)                                           # j beyond Q
    assert unchanged()
    # a tree with capacity one short of the winner's chain
    assert eng.connect_via_search(way, H, cvr.NO_INCUMBENT, 1, nodes=nodes) == (1050, 213, 0)
    with pytest.raises(nat.NativeError) as ex:
        eng.connect_via_commit(213, 0, way, H, 1)
    assert ex.value.code == nat.E_CAPACITY and unchanged()
    assert eng.climb(213) == ref.climb(213)
    assert eng.connect_via_search(way, H, cvr.NO_INCUMBENT, 1, nodes=nodes) == (1050, 213, 0)
    eng.close()


def test_commit_refuses_a_chain_that_misses_the_goal():
    from lqrrt_amd import _native as nat
    s, g, ref, way = row_inputs("car_500", 217, [217])
    assert ref.chain_via(0, 0, way, 1) is None
    eng = _engine(s, g, 217)
    fp0 = eng.footprint()
    with pytest.raises(nat.NativeError) as ex:
        eng.connect_via_commit(0, 0, way, ref.H, 1)
    assert ex.value.code == nat.E_STATE and eng.size == 217 and eng.footprint() == fp0
    assert eng.parents().tolist() == ref.pID and eng.climb(213) == ref.climb(213)
    assert eng.connect_via_search(way, ref.H, cvr.NO_INCUMBENT, 1) == (1050, 213, 0)
    eng.close()


def _car_planner(max_nodes, seed=1, **kw):
    import lqrrt_amd
    s = lqrrt_amd.systems.Car(0)
    cons = lqrrt_amd.Constraints(s.nstates, s.ncontrols, s.goal_buffer, s.is_feasible)
    p = lqrrt_amd.Planner(s.dynamics, s.lqr, cons, error_tol=s.error_tol, erf=s.erf, goal0=s.goal, printing=False,
                          max_nodes=max_nodes, wave_size=256, **dict(s.plan_kwargs, **kw))
    np.random.seed(seed)
    p.update_plan(s.x0, s.sample_space, goal_bias=s.goal_bias, xrand_gen=10, finish_on_goal=False)
    return s, p


def test_connect_via_rescues_a_plan_connect_goal_cannot():
    """The fixture's recipe (seed 1, a clock that stands still, ended by the node limit): a longer run's plan, then a run stopped so
    early that connect_goal finds nothing.  The longer run's plan beyond that tree as waypoints: connect_via finds the reference's plan."""
    s, long_run = _car_planner(500, min_time=2, max_time=3, sys_time=lambda: 0.0)
    assert long_run.plan_reached_goal
    s, p = _car_planner(107, min_time=2, max_time=3, sys_time=lambda: 0.0)
    eng = p._engine
    assert not p.plan_reached_goal and eng.size == 108
    assert np.array_equal(long_run._engine.states(0, 108), eng.states())    # the same tree, stopped earlier
    start = next(k for k, v in enumerate(long_run.node_seq) if v >= eng.size)
    way = long_run.plan_waypoints(start)
    assert len(way) == len(long_run.node_seq) - start >= 1
    assert np.array_equal(way, np.array([long_run.tree.state[v] for v in long_run.node_seq[start:]]))
    ref = cvr.ViaConnector(s, eng.states(), eng.gains(), eng.parents(), eng.edge_lengths(), p.horizon_iters)
    assert ref.search() is None
    win = ref.search_via(way)
    print("tree of %d nodes, %d waypoints: reference winner %s" % (ref.size, len(way), None if win is None else win[:3]))
    assert win is not None and win[:3] == (992, 63, 0)
    plan_ref, ids_ref = ref.commit_via(win)
    seq, T = list(p.node_seq), p.T
    assert p.connect_goal() is False and p.node_seq == seq and p.T == T and not p.plan_reached_goal
    assert p.connect_via(way) is True
    assert p.plan_reached_goal and p.node_seq == plan_ref and p.tree.size == eng.size == ref.size
    assert p._in_goal(p.x_seq[-1]) and p.T == win[0] * p.dt and len(p.x_seq) == win[0]
    x_ref = np.vstack([ref.edges[v][0] for v in ids_ref])
    u_ref = np.vstack([ref.edges[v][1] for v in ids_ref])
    assert np.array_equal(np.array(p.x_seq[-len(x_ref):]), x_ref) and np.array_equal(np.array(p.u_seq[-len(u_ref):]), u_ref)
    x_seq, u_seq = p.tree.trajectory(p.node_seq)
    assert np.array_equal(np.array(x_seq), np.array(p.x_seq)) and np.array_equal(np.array(u_seq), np.array(p.u_seq))
    assert np.array_equal(p.t_seq, np.arange(len(p.x_seq)) * p.dt)
    assert np.array_equal(p.get_state(p.T + 1.0), p.x_seq[-1])
    # a second call finds nothing below the plan it has just made from the nodes already searched; the appended nodes are new
    # candidates, and what they find is the reference's again
    seq, T = list(p.node_seq), p.T
    assert p.connect_via(way, nodes=range(108)) is False and p.node_seq == seq and p.T == T and p.tree.size == ref.size
    again = ref.search_via(way, incumbent=win[0])
    print("second call: reference winner %s" % (None if again is None else (again[:3],)))
    if again is None:
        assert p.connect_via(way) is False and p.node_seq == seq and p.T == T and p.tree.size == ref.size
    else:
        plan_ref, _ = ref.commit_via(again)
        assert p.connect_via(way) is True and p.node_seq == plan_ref and p.T == again[0] * p.dt < T and p.tree.size == ref.size
    # refine_plan works on the new plan, as the refinement's reference does
    plan_refined, log = ref.refine(plan_ref)
    assert p.refine_plan() == len(log) and p.node_seq == plan_refined
    assert p.T == ref.cost(plan_refined) * p.dt and p._in_goal(p.x_seq[-1])


def test_search_on_a_retained_tree_with_one_more_obstacle():
    """A grown car tree, one more circle on its best plan, a retain from the plan's third node with revalidation: the reference is
    built from the arrays read back after the retain, the waypoints are the old plan's lost states.  Bit for bit whatever is found."""
    import lqrrt_amd
    from lqrrt_amd.engine import Engine
    s = lqrrt_amd.systems.Car(0)
    kw = s.plan_kwargs
    H = int(kw["horizon"] / kw["dt"])
    eng = Engine(s, capacity=700, max_wave=64)
    eng.set_resolution(kw["dt"], kw["FPR"], H, np.abs(s.error_tol), s.goal, np.abs(s.goal_buffer))
    space = np.array(s.sample_space, dtype=np.float64)
    eng.set_sampler(np.mean(space, axis=1), np.diff(space).flatten(), np.array(s.goal_bias, dtype=np.float64), 10)
    st = np.random.RandomState(1).get_state()
    eng.set_mt19937(st[1], st[2])
    eng.tree_reset(s.x0)
    eng.extend(64, node_limit=400)
    end, steps, hits = eng.plan_best()
    assert end >= 0 and hits >= 1
    plan = eng.climb(end)
    old_states = eng.states()
    at = old_states[plan[(2 * len(plan)) // 3]]
    s.set_obstacles(np.vstack((np.asarray(s.obs, dtype=np.float64).reshape(-1, 3), [at[0], at[1], 1.5])))
    assert eng.sync_geometry()
    stats, old_to_new = eng.tree_retain(plan[2], revalidate=True)
    lost = [v for v in plan[2:] if old_to_new[v] < 0]
    assert stats["infeasible"] >= 1 and len(lost) >= 1
    way = old_states[lost]
    ref = cvr.ViaConnector(s, eng.states(), eng.gains(), eng.parents(), eng.edge_lengths(), H)
    incumbent = stats["best_steps"] if stats["goal_hits"] else cvr.NO_INCUMBENT
    want = ref.search_via(way, incumbent=incumbent)
    got = eng.connect_via_search(way, H, incumbent)
    print("retained %d of %d nodes, %d lost plan states, incumbent %d: device %s, reference %s"
          % (stats["kept"], len(old_states), len(lost), incumbent, got, None if want is None else want[:3]))
    assert got == (None if want is None else want[:3])
    # which it was: the kept tree holds no goal node (89 of 401 nodes stay, 8 plan states are lost), and the chain from kept node 86
    # through all 8 lost states reaches the goal
    assert (stats["kept"], len(old_states), len(lost), stats["goal_hits"]) == (89, 401, 8, 0) and got == (882, 86, 0)
    _compare_commit(eng, ref, want, way, H)
    eng.close()


def test_example_runs():
    """examples/connect_via_gpu.py: a tree stopped at 108 nodes, connect_goal finds nothing, connect_via finds the plan of the table's
    third row (992 steps), refine_plan shortens it."""
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "connect_via_gpu.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    T = [float(v) for v in re.findall(r"T = ([0-9.]+) s", out.stdout)]
    assert "budget spent: tree of 108 nodes, reached goal: False" in out.stdout and "connect_goal: False" in out.stdout
    assert re.search(r"connect_via over 8 waypoints in [0-9.]+ ms: True, reached goal: True", out.stdout)
    assert len(T) == 4 and T[2] == 99.2 and T[3] <= T[2]
