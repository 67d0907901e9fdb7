"""
The one-tree search and commit calls (refine, connect, reach, via) back to back on ONE engine: they stage their images in one
on-demand scratch per engine (csrc/engine_refine.hpp solo_scratch), so what one call leaves there -- a plan where the next lays its
waypoints, T keys where the next keeps one -- must not reach the next call's answer.  Every answer is compared, exactly, with the same
call made first on a fresh engine that holds the same tree at that point, and the searches and the appended nodes with the
references of the rules (tests/refine_reference.py, connect_reference.py, reach_reference.py, connect_via_reference.py).

The tree: the first 40 nodes of a fixture's tree, loaded by hand, with the state of a later fixture node as the goal, the two plan
nodes before it as waypoints (Q = 2), goal_tries 2, a 5-node plan from the root and T = 3 targets of which the engine's goal is the
first.  The double pendulum is the smallest model; its chains end far from where they aim, so its goal box is widened until the
searches have winners, and its chain of one node leaves the last refinement nothing to win.  The car's row has a chain of three
nodes and a last refinement with a winner, so that refine_commit runs behind the other six calls too.
"""
import ctypes as C

import numpy as np
import pytest

import connect_reference as cr
import connect_via_reference as cvr
import reach_reference as rr

pytestmark = pytest.mark.gpu

N0, TRIES = 40, 2
# fixture, the fixture node whose state is the goal, the goal buffer's scale, the 5-node plan, the fixture nodes of the two further
# targets; then what the reference finds (checked before the device is asked, so that a drifting reference or inputs that stop
# exercising the rule fail here): the first refinement, the connection, the waypoint chain and its edge lengths, the last refinement
ROWS = [("pendulum_150", 91, 100.0, [0, 1, 7, 9, 21], (50, 80), (101, 1, 2), (164, 7), (101, 1, 0), [50], None),
        ("car_500", 218, 4.0, [0, 2, 3, 4, 10], (212, 217), None, None, (201, 2, 0), [50, 50, 50], (173, 0, 1))]


def _load(s, states, K, pID, el, H, goal, buf, extra=16):
    """A tree loaded by hand on a fresh engine whose goal is `goal` -/+ `buf`."""
    from lqrrt_amd.engine import Engine
    kw = s.plan_kwargs
    el = np.array(el, dtype=np.int32)
    el[0] = 1
    eng = Engine(s, capacity=len(states) + extra, max_wave=64)
    eng.set_resolution(kw["dt"], kw["FPR"], max(int(np.max(el)), H), np.abs(np.asarray(s.error_tol, dtype=np.float64)), goal, buf)
    eng.tree_load(states, K, pID, edge_len=el)
    return eng


def _raw_no_launch(eng, H, goal, buf):
    """The three searches without a candidate, through the ABI: (return code, cost, index ...) each."""
    from lqrrt_amd import _native as nat
    lib, inc = nat.lib(), 12345
    root, none = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    cost, i, j, node = C.c_int64(-7), C.c_int32(-7), C.c_int32(-7), C.c_int32(-7)
    a = (lib.lqrrt_refine_search(eng.h, nat.ptr(root), 1, TRIES, H, inc, C.byref(cost), C.byref(i), C.byref(j), eng._stream()),
         cost.value, i.value, j.value)
    cost = C.c_int64(-7)
    b = (lib.lqrrt_connect_search(eng.h, nat.ptr(none), 0, TRIES, H, inc, C.byref(cost), C.byref(node), eng._stream()), cost.value, node.value)
    goals, lo, hi = eng._targets(np.asarray(goal, dtype=np.float64).reshape(1, -1), buf)
    incs, costs, nodes = np.array([inc], dtype=np.int64), np.full(1, -7, dtype=np.int64), np.full(1, -7, dtype=np.int32)
    c = (lib.lqrrt_reach_search(eng.h, nat.ptr(goals), nat.ptr(lo), nat.ptr(hi), 1, nat.ptr(none), 0, TRIES, H, nat.ptr(incs), nat.ptr(costs),
                                nat.ptr(nodes), eng._stream()), int(costs[0]), int(nodes[0]))
    return a, b, c, inc


@pytest.mark.parametrize("name,goal_node,scale,plan,others,refined,connected,via,lens,refined_last", ROWS)
def test_seven_calls_share_one_scratch(name, goal_node, scale, plan, others, refined, connected, via, lens, refined_last):
    s, g = cr.case(name)
    H = cr.horizon_of(s, g)
    goal = np.array(g["state"][goal_node], dtype=np.float64)
    buf = np.abs(np.asarray(s.goal_buffer, dtype=np.float64)) * scale
    above = [int(v) for v in cvr.ViaConnector(s, g["state"], g["K"], g["pID"], g["edge_len"], H).climb(goal_node) if v >= N0]
    way = np.array([g["state"][v] for v in above[:-1][-2:]], dtype=np.float64)
    goals = np.array([goal] + [g["state"][v] for v in others], dtype=np.float64)
    assert way.shape == (2, s.nstates) and goals.shape == (3, s.nstates)
    ref = cvr.ViaConnector(s, g["state"][:N0], g["K"][:N0], g["pID"][:N0], g["edge_len"][:N0], H, goal=goal, goal_buffer=buf)
    assert ref.climb(plan[-1]) == plan and len(plan) == 5

    def short(win, k):
        return None if win is None else tuple(win[:k])

    # the reference's answers on the 40-node tree
    want_refine = short(ref.round(plan, TRIES), 3)
    want_connect = short(ref.search(TRIES), 2)
    want_reach = rr.Reach(s, g["state"][:N0], g["K"][:N0], g["pID"][:N0], g["edge_len"][:N0], H).search(goals, buf, TRIES)
    win_via = ref.search_via(way, TRIES)
    one = [want_connect[1] if want_connect else 0]
    want_one = short(ref.search(TRIES, nodes=one), 2)
    print(name, want_refine, want_connect, want_reach, short(win_via, 3), one, want_one)
    assert (want_refine, want_connect, short(win_via, 3), [len(e[0]) for e in win_via[3]]) == (refined, connected, via, lens)
    assert want_reach[0] == want_connect and sum(w is not None for w in want_reach) >= 2

    eng = _load(s, g["state"][:N0], g["K"][:N0], g["pID"][:N0], g["edge_len"][:N0], H, goal, buf)
    fp0 = eng.footprint()

    def both(call, commit=False):
        """`call` on a fresh engine that holds the shared engine's tree, then on the shared engine: the two answers.  The trees are
        the same afterwards, a commit's new edges included."""
        twin = _load(s, eng.states(), eng.gains(), eng.parents(), eng.edge_lengths(), H, goal, buf)
        try:
            first = call(twin)
            got = call(eng)
            assert twin.size == eng.size and np.array_equal(twin.states(), eng.states()) and np.array_equal(twin.gains(), eng.gains())
            assert np.array_equal(twin.parents(), eng.parents()) and np.array_equal(twin.edge_lengths(), eng.edge_lengths())
            for v in (first if commit else []):
                assert all(np.array_equal(p, q) for p, q in zip(twin.edge(v), eng.edge(v))), v
            return first, got
        finally:
            twin.close()

    def appended(ids, ids_ref):
        assert ids == ids_ref
        assert np.array_equal(eng.states(ids[0], len(ids)), np.array([ref.states[v] for v in ids]))
        assert np.array_equal(eng.gains(ids[0], len(ids)), np.array([ref.K[v] for v in ids]))
        assert eng.parents(ids[0], len(ids)).tolist() == [ref.pID[v] for v in ids]
        assert eng.edge_lengths(ids[0], len(ids)).tolist() == [ref.elen[v] for v in ids]
        for v in ids:
            x, u = eng.edge(v)
            assert np.array_equal(x, ref.edges[v][0]) and np.array_equal(u, ref.edges[v][1]), v
        assert eng.size == ref.size

    cost = ref.cost(plan)
    assert both(lambda e: e.refine_round(plan, H, cost, TRIES)) == (want_refine, want_refine)
    assert both(lambda e: e.connect_search(H, cr.NO_INCUMBENT, TRIES)) == (want_connect, want_connect)
    assert both(lambda e: e.reach_search(goals, buf, H, None, TRIES)) == (want_reach, want_reach)
    assert both(lambda e: e.connect_via_search(way, H, cvr.NO_INCUMBENT, TRIES)) == (short(win_via, 3), short(win_via, 3))
    assert both(lambda e: e.refine_round(plan, H, cost, TRIES)) == (want_refine, want_refine)
    assert both(lambda e: e.connect_search(H, cr.NO_INCUMBENT, TRIES, nodes=one)) == (want_one, want_one)
    # the no-launch cases between the calls that launch: a one-node plan, an empty id list, T = 1 with an empty id list
    a, b, c, inc = _raw_no_launch(eng, H, goal, buf)
    assert a == (0, inc, -1, -1) and b == (0, inc, -1) and c == (0, inc, -1)

    first, ids = both(lambda e: e.connect_via_commit(win_via[1], win_via[2], way, H, TRIES), commit=True)
    new_plan, ids_ref = ref.commit_via(win_via)
    assert first == ids and eng.climb(ids[-1]) == new_plan
    appended(ids, ids_ref)
    win = ref.round(new_plan, TRIES)
    assert short(win, 3) == refined_last
    cost = ref.cost(new_plan)
    assert both(lambda e: e.refine_round(new_plan, H, cost, TRIES)) == (short(win, 3), short(win, 3))
    if win is not None:
        first, ids = both(lambda e: e.refine_commit(new_plan, H, win[1], win[2], TRIES), commit=True)
        last_plan, ids_ref = ref.commit(new_plan, win)
        assert first == ids and eng.climb(ids[-1]) == last_plan
        appended(ids, ids_ref)
    a, b, c, inc = _raw_no_launch(eng, H, goal, buf)
    assert a == (0, inc, -1, -1) and b == (0, inc, -1) and c == (0, inc, -1)
    assert eng.footprint() == fp0                                   # plan, keys, targets, waypoints, depth table and id list are scratch
    eng.close()
