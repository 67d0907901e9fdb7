"""
One tree asked about many goals on the device (csrc/reach.hpp through lqrrt_reach_search / lqrrt_reach_commit) against the reference
of the rule (tests/reach_reference.py: a connect_reference.Connector per target, the C oracle's primitives), BIT FOR BIT: every
target's winner (cost, node), and every appended node's state, gain, parent, edge length and edge rows.  Then Planner.goal_costs and
Planner.retarget end to end.
"""
import numpy as np
import pytest

import connect_reference as cr
import reach_reference as rh
from test_connect_gpu import _car_planner, _compare_commit, _engine, _fill

pytestmark = pytest.mark.gpu


def _snapshot(eng):
    return eng.size, eng.parents().copy(), eng.edge_lengths().copy(), eng.footprint()


def _unchanged(eng, snap):
    return eng.size == snap[0] and np.array_equal(eng.parents(), snap[1]) and np.array_equal(eng.edge_lengths(), snap[2]) \
        and eng.footprint() == snap[3]


@pytest.mark.parametrize("name,size", sorted(rh.PINNED))
def test_all_targets_in_one_call(name, size):
    """The pinned table in ONE reach_search per tree (T = 7): a wrong target index, goal or box shows as a wrong (cost, node)."""
    s, g = cr.case(name)
    rows = rh.PINNED[(name, size)]
    goals, bufs = rh.pinned_targets(s, g, rows)
    ref = rh.from_fixture(s, g, size)
    want = ref.search(goals, bufs)
    eng = _engine(s, g, size)
    snap = _snapshot(eng)
    got = eng.reach_search(goals, bufs, ref.H)
    print(name, size, got)
    assert got == want == [w for _, w in rows]
    assert sum(w is not None for w in got) >= 5
    assert _unchanged(eng, snap)                                    # keys, targets, depth table and id list are scratch, not footprint
    eng.close()


@pytest.mark.parametrize("name,size,nodes", [("double_integrator_600", 5, [0, 1, 2, 3, 4]), ("ros_boat", None, [0, 3, 11, 47, 150])])
def test_box_grid_and_occupancy_grid_match_reference(name, size, nodes):
    """The double integrator with its box grid (5 nodes) and ros_boat on its occupancy grid: own goal + the states of tree nodes."""
    s, g = cr.case(name)
    ref = rh.from_fixture(s, g, size)
    nodes = [k for k in nodes if 0 < k < ref.size]
    goals = np.array([np.asarray(s.goal, dtype=np.float64)] + [rh.node_target(g, k) for k in nodes])
    want = ref.search(goals)
    eng = _engine(s, g, size)
    snap = _snapshot(eng)
    got = eng.reach_search(goals, s.goal_buffer, ref.H)
    print(name, got)
    assert got == want
    assert _unchanged(eng, snap)
    eng.close()


def test_one_target_and_duplicates():
    """T = 1 with the engine's own goal is connect_search; the same target twice with different incumbents has two keys."""
    s, g = cr.case("car_2000")
    ref = rh.from_fixture(s, g, 217)
    eng, twin = _engine(s, g, 217), _engine(s, g, 217)
    own = np.asarray(s.goal, dtype=np.float64)[None, :]
    for inc, want in ((951, None), (952, (951, 211)), (cr.NO_INCUMBENT, (951, 211))):
        assert twin.connect_search(ref.H, inc) == want
        assert eng.reach_search(own, s.goal_buffer, ref.H, [inc]) == [want]
    assert eng.reach_search(own, s.goal_buffer, ref.H) == [(951, 211)]
    both = np.repeat(own, 2, axis=0)
    assert eng.reach_search(both, s.goal_buffer, ref.H, [951, 952]) == [None, (951, 211)]
    assert eng.reach_search(both, s.goal_buffer, ref.H, [952, 951]) == [(951, 211), None]
    eng.close(), twin.close()


def test_grid_mapping_edges():
    s, g = cr.case("car_2000")
    ref = rh.from_fixture(s, g, 217)
    goals, bufs = rh.pinned_targets(s, g, rh.PINNED[("car_2000", 217)][:3])
    want = [w for _, w in rh.PINNED[("car_2000", 217)][:3]]
    eng = _engine(s, g, 217)
    ids = np.random.RandomState(5).permutation(217)
    assert eng.reach_search(goals, bufs, ref.H, nodes=ids) == want
    assert eng.reach_search(goals, bufs, ref.H, nodes=np.sort(ids)) == want
    assert eng.reach_search(goals, bufs, ref.H, nodes=ids[::-1].copy()) == want
    # count = 1: every workgroup index is a target index
    one = ref.search(goals, bufs, nodes=[211])
    assert one[0] == (951, 211)
    assert eng.reach_search(goals, bufs, ref.H, nodes=[211]) == one
    few = [12, 211, 16]
    assert eng.reach_search(goals, bufs, ref.H, nodes=few) == ref.search(goals, bufs, nodes=few)
    assert eng.reach_search(goals, bufs, ref.H, nodes=[]) == [None, None, None]
    eng.close()


def test_host_refusals():
    s, g = cr.case("car_2000")
    ref = rh.from_fixture(s, g, 217)
    eng = _engine(s, g, 217)
    n = s.nstates
    own = np.asarray(s.goal, dtype=np.float64)
    buf = np.abs(np.asarray(s.goal_buffer, dtype=np.float64))
    snap = _snapshot(eng)
    bad_goal = own.copy()
    bad_goal[1] = np.nan
    neg = buf.copy()
    neg[0] = -neg[0] - 1.0                                          # lo > hi in dimension 0
    for kw in (dict(goals=np.zeros((0, n)), buffers=buf),           # T = 0
               dict(goals=np.repeat(own[None, :], 1025, axis=0), buffers=buf, nodes=[0]),
               dict(goals=[own], buffers=buf, nodes=[0, 217]),      # an id beyond the tree
               dict(goals=[own], buffers=buf, nodes=[-1]),
               dict(goals=[own, own], buffers=[buf, neg]),
               dict(goals=[own, bad_goal], buffers=buf),
               dict(goals=[own], buffers=buf, incumbents=[0]),
               dict(goals=[own], buffers=buf, incumbents=[2 ** 31]),
               dict(goals=[own], buffers=buf, goal_tries=0),
               # 1024 targets x 65536 candidates x 64 threads = 2^32: refused on the host, nothing launched
               dict(goals=np.repeat(own[None, :], 1024, axis=0), buffers=buf, nodes=np.zeros(65536, dtype=np.int32))):
        with pytest.raises(ValueError):
            eng.reach_search(horizon_iters=ref.H, **kw)
        assert _unchanged(eng, snap)
    with pytest.raises(ValueError):
        eng.reach_search([own], buf, ref.H + 10 ** 6)
    for kw in (dict(goal=bad_goal, buffer=buf, node=211), dict(goal=own, buffer=neg, node=211), dict(goal=own, buffer=buf, node=217)):
        with pytest.raises(ValueError):
            eng.reach_commit(horizon_iters=ref.H, **kw)
        assert _unchanged(eng, snap)
    assert eng.reach_search([own], buf, ref.H) == [(951, 211)]
    eng.close()


class _Toward(object):
    """An engine whose connect_commit is reach_commit toward one target: what test_connect_gpu._compare_commit drives."""

    def __init__(self, eng, goal, buf):
        self._eng, self._goal, self._buf = eng, goal, buf

    def connect_commit(self, node, horizon_iters, goal_tries=8):
        return self._eng.reach_commit(self._goal, self._buf, node, horizon_iters, goal_tries)

    def __getattr__(self, name):
        return getattr(self._eng, name)


@pytest.mark.parametrize("row", [1, 4])
def test_commit_matches_reference(row):
    """reach_commit for two different targets on twins, against Connector(goal=...).commit_chain; the engine's own goal box stays."""
    s, g = cr.case("car_2000")
    rows = rh.PINNED[("car_2000", 217)]
    goals, bufs = rh.pinned_targets(s, g, rows)
    ref = rh.from_fixture(s, g, 217)
    con = ref.connector(goals[row], bufs[row])
    win = con.search()
    assert (win[0], win[1]) == rows[row][1]
    eng = _engine(s, g, 217)
    fp0 = eng.footprint()
    assert eng.connect_search(ref.H, cr.NO_INCUMBENT) == (951, 211)
    plan, ids = _compare_commit(_Toward(eng, goals[row], bufs[row]), con, win, ref.H)
    assert plan == con.climb(win[1]) + ids and con.in_goal(eng.states(ids[-1], 1)[0])
    assert eng.footprint() == fp0
    # the engine's own goal and box are what they were: the old question has its old answer on the grown tree's old nodes
    assert eng.connect_search(ref.H, cr.NO_INCUMBENT, nodes=list(range(217))) == (951, 211)
    assert eng.reach_search(goals[row:row + 1], bufs[row:row + 1], ref.H, [win[0]]) == [None]
    eng.close()


def test_commit_capacity_and_missed_target():
    from lqrrt_amd import _native as nat
    s, g = cr.case("car_2000")
    rows = rh.PINNED[("car_2000", 217)]
    goals, bufs = rh.pinned_targets(s, g, rows)
    ref = rh.from_fixture(s, g, 217)
    assert ref.connector(goals[4], bufs[4]).chain(0) is None        # eight steers from the root do not reach target "node 200"
    eng = _engine(s, g, 217)
    with pytest.raises(nat.NativeError) as ex:
        eng.reach_commit(goals[4], bufs[4], 0, ref.H)
    assert ex.value.code == nat.E_STATE and eng.size == 217
    with pytest.raises(nat.NativeError) as ex:                      # the far target: no chain ends in its box
        eng.reach_commit(goals[6], bufs[6], 211, ref.H)
    assert ex.value.code == nat.E_STATE and eng.size == 217
    assert eng.reach_search(goals[:5], bufs[:5], ref.H) == [w for _, w in rows[:5]]
    eng.close()
    eng = _engine(s, g, 217, extra=1)
    nodes = list(range(217))
    full = _fill(eng, g["state"][0], g["K"][0])
    parents, lens = eng.parents(), eng.edge_lengths()
    assert eng.reach_search(goals[4:5], bufs[4:5], ref.H, nodes=nodes) == [rows[4][1]]
    with pytest.raises(nat.NativeError) as ex:
        eng.reach_commit(goals[4], bufs[4], rows[4][1][1], ref.H)
    assert ex.value.code == nat.E_CAPACITY and eng.size == full
    assert np.array_equal(eng.parents(), parents) and np.array_equal(eng.edge_lengths(), lens)
    assert eng.reach_search(goals[4:5], bufs[4:5], ref.H, nodes=nodes) == [rows[4][1]]
    eng.close()


def _reach_of(s, p):
    eng = p._engine
    return rh.Reach(s, eng.states(), eng.gains(), eng.parents(), eng.edge_lengths(), p.horizon_iters)


def _off_plan_targets(s, p, ref, want=4):
    """States of `want` tree nodes off the plan as goals, the first of them ones for which the reference has a winner."""
    on_plan = set(p.node_seq)
    hit, miss = [], []
    for k in range(ref.size - 1, 0, -7):
        if k in on_plan:
            continue
        w = ref.search(ref.states[k][None, :])[0]
        (hit if w is not None else miss).append(k)
        if len(hit) >= want:
            break
    assert hit, "no node state of the tree is reachable by a goal chain"
    return (hit + miss)[:want]


def test_goal_costs_and_retarget_end_to_end():
    s, p = _car_planner(215, min_time=2, max_time=3, sys_time=lambda: 0.0)
    eng = p._engine
    assert not p.plan_reached_goal and eng.size == 216
    ref = _reach_of(s, p)
    picks = _off_plan_targets(s, p, ref)
    goals = np.array([ref.states[k] for k in picks])
    want = ref.wins(goals)
    seq, T, size, fp, goal0 = list(p.node_seq), p.T, p.tree.size, eng.footprint(), np.array(p.goal)
    steps, start = p.goal_costs(goals)
    print("targets: nodes %s -> steps %s from nodes %s" % (picks, steps.tolist(), start.tolist()))
    assert steps.tolist() == [-1 if w is None else w[0] for w in want]
    assert start.tolist() == [-1 if w is None else w[1] for w in want]
    assert (steps >= 0).sum() >= 1
    assert p.node_seq == seq and p.T == T and p.tree.size == eng.size == size and eng.footprint() == fp
    assert np.array_equal(p.goal, goal0) and not p.plan_reached_goal
    # one buffer per goal, and an id list, go through the same call
    bufs = np.abs(np.asarray(s.goal_buffer, dtype=np.float64))[None, :] * np.array([1.0, 0.5, 1.0, 0.25])[:len(goals), None]
    steps2, start2 = p.goal_costs(goals, bufs, goal_tries=4, nodes=list(range(0, size, 2)))
    want2 = ref.search(goals, bufs, goal_tries=4, nodes=list(range(0, size, 2)))
    assert list(zip(steps2.tolist(), start2.tolist())) == [(-1, -1) if w is None else w for w in want2]

    # retarget to a target far away: nothing changes
    far = goal0.copy()
    far[0] += 1e4
    assert ref.search(far[None, :]) == [None]
    assert p.retarget(far) is False
    assert p.node_seq == seq and p.T == T and p.tree.size == size and np.array_equal(p.goal, goal0) and not p.plan_reached_goal
    with pytest.raises(RuntimeError, match="goal changed"):         # (a moved goal is still what connect_goal refuses)
        p.set_goal(far)
        p.connect_goal()
    p.set_goal(goal0)

    # retarget to the cheapest target
    t = min((k for k in range(len(goals)) if want[k] is not None), key=lambda k: (want[k][0], k))
    con = ref.connector(goals[t])
    win = want[t]
    plan_ref, ids_ref = con.commit_chain(win)
    assert p.retarget(goals[t]) is True
    assert p.plan_reached_goal and np.array_equal(p.goal, goals[t]) and p.node_seq == plan_ref
    assert p.tree.size == eng.size == con.size and p.T == win[0] * p.dt and len(p.x_seq) == win[0]
    x_seq, u_seq = p.tree.trajectory(p.node_seq)
    assert np.array_equal(np.array(x_seq), np.array(p.x_seq)) and np.array_equal(np.array(u_seq), np.array(p.u_seq))
    assert np.array_equal(p.t_seq, np.arange(len(p.x_seq)) * p.dt)
    assert np.array_equal(np.array(p.x_seq[-len(con.edges[ids_ref[-1]][0]):]), con.edges[ids_ref[-1]][0])
    assert np.array_equal(eng.states(ids_ref[0], len(ids_ref)), np.array([con.states[v] for v in ids_ref]))
    assert p._in_goal(p.x_seq[-1]) and con.in_goal(p.x_seq[-1])
    assert np.array_equal(p.get_state(p.T + 1.0), p.x_seq[-1])
    # the new goal is the engine's: connect_goal no longer raises, and finds nothing below the plan just made or what the reference finds
    again = con.search(incumbent=win[0])
    seq2 = list(p.node_seq)
    if again is None:
        assert p.connect_goal() is False and p.node_seq == seq2
    else:
        plan_ref, _ = con.commit_chain(again)
        assert p.connect_goal() is True and p.node_seq == plan_ref
    # refine_plan works on the new plan, as the refinement's reference does with the new goal
    plan_refined, log = con.refine(plan_ref)
    assert p.refine_plan() == len(log) and p.node_seq == plan_refined
    assert p.T == con.cost(plan_refined) * p.dt and p._in_goal(p.x_seq[-1])
    # and the old goal is now one target among others
    steps3, _ = p.goal_costs([goal0, goals[t]])
    now = _reach_of(s, p).search(np.array([goal0, goals[t]]))
    assert steps3.tolist() == [-1 if w is None else w[0] for w in now]


def test_retarget_with_a_finish_node():
    """A plan that ends in a finish_on_goal node: retarget drops that node and runs the exact-goal steer again toward the NEW goal."""
    for seed in range(1, 9):
        s, p = _car_planner(3000, finish=True, seed=seed, min_time=0.0, max_time=10)
        eng = p._engine
        if not p.plan_reached_goal or p.node_seq[-1] < eng.size:    # the force-arrive steer produced nothing: no finish node
            continue
        ref = _reach_of(s, p)
        picks = _off_plan_targets(s, p, ref, want=1)
        goal = ref.states[picks[0]].copy()
        con = ref.connector(goal)
        win = con.search()
        plan_ref, _ = con.commit_chain(win)
        assert p.retarget(goal) is True
        assert np.array_equal(p.goal, goal) and p.plan_reached_goal
        assert p.node_seq[:len(plan_ref)] == plan_ref and p.T == win[0] * p.dt
        if len(p.node_seq) > len(plan_ref):                         # the finish node, run again from the new end toward the new goal
            assert p.node_seq[-1] == p.tree.size - 1 and p.tree._host_nodes() == 1
            assert np.array_equal(p.tree.state[p.node_seq[-1]], goal)
        else:
            assert p.tree._host_nodes() == 0
        return
    pytest.fail("no finish_on_goal plan of the car in 8 seeds")


def test_example_runs():
    """examples/retarget_gpu.py: a car plans to its goal, prints goal_costs of three alternative goals, retargets to the cheapest."""
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "retarget_gpu.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert re.search(r"plan to the first goal: reached goal: True", out.stdout)
    costs = [(int(k), float(v)) for k, v in re.findall(r"alternative (\d): ([0-9.]+) s", out.stdout)]
    assert len(costs) == 3
    m = re.search(r"retarget to alternative (\d) in [0-9.]+ ms: True, reached goal: True, T = ([0-9.]+) s", out.stdout)
    assert m, out.stdout
    best = min(costs, key=lambda c: (c[1], c[0]))
    assert int(m.group(1)) == best[0] and float(m.group(2)) == best[1]
