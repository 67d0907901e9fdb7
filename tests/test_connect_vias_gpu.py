"""
Goal chains through waypoints for several trees per call on the device (csrc/connect_via_multi.hpp through
lqrrt_connect_via_search_multi / lqrrt_connect_via_commit_multi) against the reference of the rule (tests/connect_via_reference.py,
the C oracle's primitives), BIT FOR BIT, and against the one-tree calls on identically loaded twins.  Every call holds engines of one
model, loaded from fixture prefixes; every engine has its own waypoint table, id list, goal tries, incumbent and key.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import connect_reference as cr
import connect_via_reference as cvr
import test_connect_vias_cpu as cpu
from test_connect_via_gpu import _engine
from test_connect_multi_gpu import _same_tree, _tree

pytestmark = pytest.mark.gpu

NO = cvr.NO_INCUMBENT


def _rows(name):
    """Rows of connect_via_reference.ROWS as (fixture, nodes, waypoint key, tries, winner)."""
    return [(r[0], r[1], r[2] if isinstance(r[2], int) else tuple(r[2]), r[3], r[5]) for r in cvr.ROWS if r[0] == name]


def _new_rows(name):
    return [(r[0], r[1], "beyond" if r[2] else "none", r[3], r[4]) for r in cpu.NEW_ROWS if r[0] == name]


# per call: (fixture, nodes loaded, waypoints -- "none", "beyond" (test_connect_vias_cpu.BEYOND) or the plan nodes of a row of
# connect_via_reference.ROWS --, goal tries, the winner computed with the reference)
CALLS = {
    # Q per engine: 1, 1, 8, 8, 0, 0 -- neighbouring engines decode their candidates with different strides
    "car": _rows("car_500") + [("car_500", 217, "none", 1, None), ("car_500", 217, "none", 8, (951, 211, 0))],
    "boat_novice": _rows("boat_novice_300"),
    "double_integrator": _new_rows("double_integrator_600"),
    "riccati": _new_rows("boat_novice_lqr_400"),
}


@functools.lru_cache(maxsize=None)
def _way(name, size, key):
    s, g = cpu.case(name)
    if key == "none":
        way = np.zeros((0, s.nstates))
    elif key == "beyond":
        way = cpu.beyond(name)
    else:
        way = cvr.row_inputs(name, size, key if isinstance(key, int) else list(key))[3]
    way.setflags(write=False)
    return way


@functools.lru_cache(maxsize=None)
def _ref_win(name, size, key, tries, incumbent=NO, nodes=None):
    """The reference's winner (cost, v, j, edges) or None; computed once per case and left unchanged."""
    s, g = cpu.case(name)
    return cvr.from_fixture(s, g, size).search_via(_way(name, size, key), goal_tries=tries, incumbent=incumbent,
                                                   nodes=None if nodes is None else list(nodes))


def _load(name, size, extra=64):
    s, g = cpu.case(name)
    return _engine(s, g, size, extra)


def _horizon(name):
    s, g = cpu.case(name)
    return cr.horizon_of(s, g)


def _check_commit(eng, name, size, win, ids, where=None):
    """A batched commit against the reference's commit (the assertions of tests/test_connect_via_gpu.py _compare_commit)."""
    s, g = cpu.case(name)
    ref = cvr.from_fixture(s, g, size)
    plan, ids_ref = ref.commit_via(win)
    assert ids == ids_ref, where
    first, k = ids[0], len(ids)
    assert np.array_equal(eng.states(first, k), np.array([ref.states[v] for v in ids])), where
    assert np.array_equal(eng.gains(first, k), np.array([ref.K[v] for v in ids])), where
    assert eng.parents(first, k).tolist() == [ref.pID[v] for v in ids], where
    assert eng.edge_lengths(first, k).tolist() == [ref.elen[v] for v in ids], where
    for v in ids:
        x, u = eng.edge(v)
        assert np.array_equal(x, ref.edges[v][0]) and np.array_equal(u, ref.edges[v][1]), (where, v)
    assert eng.climb(ids[-1]) == plan and eng.size == ref.size, where


def _pairs(wins):
    return [None if w is None else (w[1], w[2]) for w in wins]


@pytest.mark.parametrize("call", sorted(CALLS))
def test_batched_search_and_commit_match_reference(call):
    from lqrrt_amd.engine import Engine
    rows = CALLS[call]
    wants = [_ref_win(name, size, key, tries) for name, size, key, tries, _ in rows]
    print(call, [None if w is None else w[:3] for w in wants])
    assert [None if w is None else w[:3] for w in wants] == [row[4] for row in rows]          # the table is the reference's
    if call == "car":
        assert [len(_way(name, size, key)) for name, size, key, _, _ in rows] == [1, 1, 8, 8, 0, 0]
    engines = [_load(name, size) for name, size, _, _, _ in rows]
    ways = [_way(name, size, key) for name, size, key, _, _ in rows]
    H = [_horizon(name) for name, _, _, _, _ in rows]
    tries = [row[3] for row in rows]
    sizes = [e.size for e in engines]
    fp0 = [e.footprint() for e in engines]
    got = Engine.connect_via_search_multi(engines, ways, H, [NO] * len(rows), tries)
    print(call, got)
    assert got == [row[4] for row in rows]
    new = Engine.connect_via_commit_multi(engines, _pairs(got), ways, H, tries)
    for k, ((name, size, _, _, _), w, ids) in enumerate(zip(rows, wants, new)):
        if w is None:
            assert ids == [] and engines[k].size == sizes[k], k
        else:
            _check_commit(engines[k], name, size, w, ids, k)
    # nothing below each winner's cost from the nodes that were searched (the appended nodes are new candidates: they may do better)
    again = Engine.connect_via_search_multi(engines, ways, H, [NO if w is None else w[0] for w in wants], tries,
                                            nodes=[np.arange(n) for n in sizes])
    assert again == [None] * len(rows)
    assert [e.footprint() for e in engines] == fp0                  # the images are scratch, not footprint
    for e in engines:
        e.close()


def test_every_engine_has_its_own_key():
    from lqrrt_amd.engine import Engine
    way = _way("car_500", 217, (217,))
    engines = [_load("car_500", 217) for _ in range(3)]
    H = [_horizon("car_500")] * 3
    got = Engine.connect_via_search_multi(engines, [way] * 3, H, [NO, 1050, 1051], 1)
    assert got == [(1050, 213, 0), None, (1050, 213, 0)]
    for e in engines:
        e.close()


def test_every_engine_has_its_own_waypoint_table():
    from lqrrt_amd.engine import Engine
    way = _way("car_500", 217, (217,))
    a, b = _load("car_500", 217), _load("car_500", 217)
    H = [_horizon("car_500")] * 2
    assert Engine.connect_via_search_multi([a, b], [way, []], H, [NO] * 2, 1) == [(1050, 213, 0), None]
    assert Engine.connect_via_search_multi([a, b], [None, way], H, [NO] * 2, 1) == [None, (1050, 213, 0)]
    _same_tree(a, b)
    a.close()
    b.close()


def test_id_lists_per_engine():
    from lqrrt_amd.engine import Engine
    way = _way("car_500", 217, (217,))
    perm = np.random.RandomState(5).permutation(217)
    rest = tuple(sorted(int(v) for v in perm if v != 213))
    want = _ref_win("car_500", 217, (217,), 1, NO, rest)
    assert (None if want is None else want[:3]) != (1050, 213, 0)
    engines = [_load("car_500", 217) for _ in range(6)]
    H = [_horizon("car_500")] * 6
    lists = [perm, perm[::-1], np.concatenate((perm, perm[:40], [213, 213])), [], [v for v in perm if v != 213], None]
    got = Engine.connect_via_search_multi(engines, [way] * 6, H, [NO] * 6, 1, nodes=lists)
    assert got == [(1050, 213, 0)] * 3 + [None, None if want is None else want[:3], (1050, 213, 0)]
    assert Engine.connect_via_search_multi(engines, [way] * 6, H, [NO] * 6, 1, nodes=None) == [(1050, 213, 0)] * 6
    assert Engine.connect_via_search_multi(engines[:2], [way] * 2, H[:2], [NO] * 2, 1, nodes=[[], []]) == [None, None]
    for e in engines:
        e.close()


def test_batched_calls_equal_the_solo_calls_on_twins():
    """Each engine's result is that of connect_via_search / connect_via_commit on an identically loaded twin: the whole tree agrees."""
    from lqrrt_amd.engine import Engine
    rows = CALLS["car"]
    fleet = [_load(name, size) for name, size, _, _, _ in rows]
    twins = [_load(name, size) for name, size, _, _, _ in rows]
    ways = [_way(name, size, key) for name, size, key, _, _ in rows]
    H = _horizon("car_500")
    tries = [row[3] for row in rows]
    got = Engine.connect_via_search_multi(fleet, ways, [H] * len(rows), [NO] * len(rows), tries)
    new = Engine.connect_via_commit_multi(fleet, _pairs(got), ways, [H] * len(rows), tries)
    for k, (p, q) in enumerate(zip(fleet, twins)):
        solo = q.connect_via_search(ways[k], H, NO, tries[k])
        assert got[k] == solo, k
        ids = [] if solo is None else q.connect_via_commit(solo[1], solo[2], ways[k], H, tries[k])
        assert new[k] == ids, k
        _same_tree(p, q, k)
        for v in ids:
            (x, u), (y, w) = p.edge(v), q.edge(v)
            assert np.array_equal(x, y) and np.array_equal(u, w), (k, v)
        assert not ids or p.climb(ids[-1]) == q.climb(ids[-1]), k
    for e in fleet + twins:
        e.close()


def test_more_engines_than_one_launch_holds():
    """34 engines: two launches (32 + 2).  The waypoint tables alternate, and so do the goal tries within each; every engine's result
    is its solo result."""
    from lqrrt_amd.engine import Engine
    name = "car_500"
    H = _horizon(name)
    way = _way(name, 217, (217,))
    combos = [("way", 1), ("none", 1), ("way", 8), ("none", 8)]
    table = {("way", 1): (1050, 213, 0), ("none", 1): None, ("way", 8): (951, 211, 1), ("none", 8): (951, 211, 0)}
    tables = {"way": way, "none": None}
    plan = [combos[k % 4] for k in range(34)]
    engines = [_load(name, 217, extra=16) for _ in plan]
    twins = {c: _load(name, 217, extra=16) for c in combos}
    solo = {c: twins[c].connect_via_search(() if tables[c[0]] is None else way, H, NO, c[1]) for c in combos}
    assert solo == table
    for c in combos:
        if solo[c] is not None:
            twins[c].connect_via_commit(solo[c][1], solo[c][2], () if tables[c[0]] is None else way, H, c[1])
    ways = [tables[w] for w, _ in plan]
    tries = [t for _, t in plan]
    got = Engine.connect_via_search_multi(engines, ways, [H] * 34, [NO] * 34, tries)
    assert got == [solo[c] for c in plan]
    new = Engine.connect_via_commit_multi(engines, _pairs(got), ways, [H] * 34, tries)
    for k, c in enumerate(plan):
        assert (new[k] == []) == (solo[c] is None), k
        _same_tree(engines[k], twins[c], k)
        for v in new[k]:
            (x, u), (y, w) = engines[k].edge(v), twins[c].edge(v)
            assert np.array_equal(x, y) and np.array_equal(u, w), (k, v)
    for e in engines + list(twins.values()):
        e.close()


def _append_root(eng, x0, K0):
    from lqrrt_amd import _native as nat
    x0, K0 = np.ascontiguousarray(x0, dtype=np.float64), np.ascontiguousarray(K0, dtype=np.float64)
    return nat.lib().lqrrt_tree_append(eng.h, 0, nat.ptr(x0), nat.ptr(K0), 1, None, None, eng._stream())


def test_a_tree_with_room_for_one_node_keeps_its_own_while_its_twin_commits():
    from lqrrt_amd import _native as nat
    from lqrrt_amd.engine import Engine
    s, g = cpu.case("car_500")
    way = _way("car_500", 217, (217,))
    H = [_horizon("car_500")] * 2
    win = _ref_win("car_500", 217, (217,), 1)
    assert len(win[3]) == 2                                         # the winner's chain has two nodes
    tight, twin = _load("car_500", 217, extra=1), _load("car_500", 217)
    cap = (217 + 1 + 63) // 64 * 64                                 # (an engine's capacity is a multiple of 64)
    for _ in range(cap - 1 - 217):                                  # copies of the root until one slot is left
        nat.check(_append_root(tight, g["state"][0], g["K"][0]))
    full = tight.size
    assert full == cap - 1
    before = _tree(tight)
    nodes = [list(range(217)), None]                                # (the copies of the root are not candidates)
    assert Engine.connect_via_search_multi([tight, twin], [way] * 2, H, [NO] * 2, 1, nodes=nodes) == [(1050, 213, 0)] * 2
    new = Engine.connect_via_commit_multi([tight, twin], [(213, 0)] * 2, [way] * 2, H, 1)
    assert new[0] is None and tight.size == full
    for x, y in zip(_tree(tight), before):
        assert np.array_equal(x, y)
    _check_commit(twin, "car_500", 217, win, new[1])
    assert tight.climb(213) == twin.climb(213)
    assert Engine.connect_via_search_multi([tight], [way], H[:1], [NO], 1, nodes=nodes[:1]) == [(1050, 213, 0)]
    # the room was one node exactly, and it is still there
    assert _append_root(tight, g["state"][0], g["K"][0]) >= 0 and _append_root(tight, g["state"][0], g["K"][0]) == nat.E_CAPACITY
    tight.close()
    twin.close()


def test_a_chain_that_misses_the_goal_fails_alone():
    from lqrrt_amd import _native as nat
    from lqrrt_amd.engine import Engine
    s, g, ref, way = cvr.row_inputs("car_500", 217, [217])
    assert ref.chain_via(213, 1, way, 1) is None                    # one steer at the goal from node 213 does not reach the box
    engines = [_load("car_500", 217) for _ in range(3)]
    H = [_horizon("car_500")] * 3
    with pytest.raises(nat.NativeError) as ex:
        Engine.connect_via_commit_multi(engines, [(213, 0), (213, 1), None], [way] * 3, H, 1)
    assert ex.value.code == nat.E_STATE and ex.value.failed == [1]
    assert ex.value.results[1] is None and ex.value.results[2] == [] and engines[1].size == engines[2].size == 217
    _check_commit(engines[0], "car_500", 217, _ref_win("car_500", 217, (217,), 1), ex.value.results[0])
    _same_tree(engines[1], engines[2])
    assert Engine.connect_via_search_multi(engines[1:], [way] * 2, H[1:], [NO] * 2, 1) == [(1050, 213, 0)] * 2
    for e in engines:
        e.close()


def _raw_search(handles, ways, Q, tries, H, incumbents=None, nodes=None):
    """lqrrt_connect_via_search_multi with the arguments as they are: no sorting, no shape checks.  Returns the code."""
    from lqrrt_amd import _native as nat
    n = len(handles)
    hs = (C.c_void_p * n)(*handles)
    ways = [None if w is None else np.ascontiguousarray(w, dtype=np.float64) for w in ways]
    wp = (C.c_void_p * n)(*[None if w is None else w.ctypes.data for w in ways])
    Q, tries, H = (np.ascontiguousarray(v, dtype=np.int32) for v in (Q, tries, H))
    inc = np.ascontiguousarray([NO] * n if incumbents is None else incumbents, dtype=np.int64)
    ids = counts = node_ptrs = None
    if nodes is not None:
        ids = [None if v is None else np.ascontiguousarray(v, dtype=np.int32) for v in nodes]
        counts = np.ascontiguousarray([0 if a is None else len(a) for a in ids], dtype=np.int32)
        node_ptrs = (C.c_void_p * n)(*[None if a is None else a.ctypes.data for a in ids])
    cost, node, j = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
    return nat.lib().lqrrt_connect_via_search_multi(hs, n, node_ptrs, None if counts is None else nat.ptr(counts), wp, nat.ptr(Q),
                                                    nat.ptr(tries), nat.ptr(H), nat.ptr(inc), nat.ptr(cost), nat.ptr(node), nat.ptr(j), None)


def _raw_commit(handles, cands, ways, Q, tries, H):
    from lqrrt_amd import _native as nat
    n = len(handles)
    hs = (C.c_void_p * n)(*handles)
    ways = [None if w is None else np.ascontiguousarray(w, dtype=np.float64) for w in ways]
    wp = (C.c_void_p * n)(*[None if w is None else w.ctypes.data for w in ways])
    Q, tries, H = (np.ascontiguousarray(v, dtype=np.int32) for v in (Q, tries, H))
    cn = np.ascontiguousarray([c[0] for c in cands], dtype=np.int32)
    cj = np.ascontiguousarray([c[1] for c in cands], dtype=np.int32)
    outs = [np.empty(64, dtype=np.int32) for _ in range(n)]
    out_ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in outs])
    caps = np.ascontiguousarray([64] * n, dtype=np.int32)
    counts = np.zeros(n, dtype=np.int32)
    return nat.lib().lqrrt_connect_via_commit_multi(hs, n, nat.ptr(cn), nat.ptr(cj), wp, nat.ptr(Q), nat.ptr(tries), nat.ptr(H), out_ptrs,
                                                    nat.ptr(caps), nat.ptr(counts), None)


def test_refused_with_nothing_launched():
    from lqrrt_amd import _native as nat
    from lqrrt_amd.engine import Engine, NodeTable
    cars = [_load("car_500", 217) for _ in range(3)]
    boat = _load("boat_novice_300", 107)
    table = NodeTable(3, 2, (2,), capacity=64)
    table.reset(np.zeros(3))
    H, Hb = _horizon("car_500"), _horizon("boat_novice_300")
    way = _way("car_500", 217, (217,))
    wayb = _way("boat_novice_300", 107, 16)
    n = cars[0].n
    everybody = cars + [boat]
    before = [_tree(e) for e in everybody]
    fp0 = [e.footprint() for e in everybody]
    hs = [e.h for e in cars]

    def unchanged():
        return [e.footprint() for e in everybody] == fp0 and all(
            e.size == len(old[0]) and all(np.array_equal(x, y) for x, y in zip(_tree(e), old)) for e, old in zip(everybody, before))
    # null entries
    assert _raw_search([hs[0], None, hs[2]], [way] * 3, [1] * 3, [1] * 3, [H] * 3) == nat.E_ARG
    assert _raw_commit([hs[0], None, hs[2]], [(213, 0)] * 3, [way] * 3, [1] * 3, [1] * 3, [H] * 3) == nat.E_ARG
    # an engine twice
    with pytest.raises(ValueError, match="twice"):
        Engine.connect_via_search_multi([cars[0], cars[1], cars[0]], [way] * 3, [H] * 3, [NO] * 3, 1)
    with pytest.raises(ValueError, match="twice"):
        Engine.connect_via_commit_multi([cars[0], cars[1], cars[0]], [(213, 0)] * 3, [way] * 3, [H] * 3, 1)
    # mixed model
    with pytest.raises(ValueError, match="model"):
        Engine.connect_via_search_multi([cars[0], boat], [way, wayb], [H, Hb], [NO] * 2)
    with pytest.raises(ValueError, match="model"):
        Engine.connect_via_commit_multi([cars[0], boat], [(213, 0), (55, 5)], [way, wayb], [H, Hb])
    # a generic engine
    assert _raw_search([hs[0], table.h], [way, None], [1, 0], [1, 1], [H, H]) == nat.E_STATE
    assert _raw_commit([hs[0], table.h], [(213, 0), (0, 0)], [way, None], [1, 0], [1, 1], [H, H]) == nat.E_STATE
    # Q < 0; Q > 0 with a null table
    assert _raw_search(hs, [way] * 3, [1, 1, -1], [1] * 3, [H] * 3) == nat.E_ARG
    assert _raw_search(hs, [way, way, None], [1, 1, 1], [1] * 3, [H] * 3) == nat.E_ARG
    assert _raw_commit(hs, [(213, 0)] * 3, [way] * 3, [1, 1, -1], [1] * 3, [H] * 3) == nat.E_ARG
    assert _raw_commit(hs, [(213, 0)] * 3, [way, way, None], [1, 1, 1], [1] * 3, [H] * 3) == nat.E_ARG
    assert unchanged()
    # a waypoint that is not finite
    for value in (np.nan, np.inf):
        bad = way.copy()
        bad[0, 1] = value
        with pytest.raises(ValueError, match="finite"):
            Engine.connect_via_search_multi(cars, [way, way, bad], [H] * 3, [NO] * 3, 1)
        with pytest.raises(ValueError, match="finite"):
            Engine.connect_via_commit_multi(cars, [(213, 0)] * 3, [way, bad, way], [H] * 3, 1)
    # tables of the wrong shape, or too few of them
    with pytest.raises(ValueError):
        Engine.connect_via_search_multi(cars, [way, way, np.zeros((1, n + 1))], [H] * 3, [NO] * 3)
    with pytest.raises(ValueError):
        Engine.connect_via_search_multi(cars, [way, way], [H] * 3, [NO] * 3)
    with pytest.raises(ValueError):
        Engine.connect_via_commit_multi(cars, [(213, 0)] * 3, [way, way[0], way], [H] * 3)
    # an id list that is not strictly ascending, an id outside the tree
    assert _raw_search(hs, [way] * 3, [1] * 3, [1] * 3, [H] * 3, nodes=[None, [0, 5, 3], None]) == nat.E_ARG
    assert _raw_search(hs, [way] * 3, [1] * 3, [1] * 3, [H] * 3, nodes=[None, None, [0, 3, 3]]) == nat.E_ARG
    with pytest.raises(ValueError, match="outside the tree"):
        Engine.connect_via_search_multi(cars, [way] * 3, [H] * 3, [NO] * 3, nodes=[None, None, [0, 217]])
    with pytest.raises(ValueError, match="outside the tree"):
        Engine.connect_via_commit_multi(cars, [(213, 0), (213, 0), (217, 0)], [way] * 3, [H] * 3)
    with pytest.raises(ValueError, match="first waypoint"):
        Engine.connect_via_commit_multi(cars, [(213, 0), (213, 2), (213, 0)], [way] * 3, [H] * 3)      # j beyond Q
    # incumbent out of range
    with pytest.raises(ValueError, match="incumbent"):
        Engine.connect_via_search_multi(cars, [way] * 3, [H] * 3, [NO, NO, 0])
    with pytest.raises(ValueError, match="incumbent"):
        Engine.connect_via_search_multi(cars, [way] * 3, [H] * 3, [NO, 2 ** 31, NO])
    # horizon, goal tries
    with pytest.raises(ValueError, match="horizon"):
        Engine.connect_via_search_multi(cars, [way] * 3, [H, H, H + 10 ** 6], [NO] * 3)
    with pytest.raises(ValueError, match="horizon"):
        Engine.connect_via_commit_multi(cars, [(213, 0)] * 3, [way] * 3, [H, H, H + 10 ** 6])
    with pytest.raises(ValueError, match="goal_tries"):
        Engine.connect_via_search_multi(cars, [way] * 3, [H] * 3, [NO] * 3, goal_tries=[8, 8, 0])
    # more candidates than one launch holds
    many = np.zeros((2 ** 26 // 217 + 1, n))
    with pytest.raises(ValueError, match="one launch"):
        Engine.connect_via_search_multi(cars, [way, many, way], [H] * 3, [NO] * 3, 1)
    # the 32-bit depth bound with (Q + tries) horizon
    with pytest.raises(ValueError, match="32-bit"):
        Engine.connect_via_search_multi(cars, [way] * 3, [H] * 3, [NO] * 3, goal_tries=[1, 1, 2 ** 31 // H])
    assert _raw_commit(hs, [(213, 0)] * 3, [way] * 3, [1] * 3, [1, 1, 2 ** 31 // H], [H] * 3) == nat.E_ARG
    with pytest.raises(ValueError):
        Engine.connect_via_search_multi(cars, [way] * 3, [H] * 3, [NO] * 3, nodes=[None])
    with pytest.raises(ValueError):
        Engine.connect_via_search_multi([], [], [], [])
    assert unchanged()
    crowd = [_load("double_integrator_600", 1, extra=2) for _ in range(129)]
    Hd = _horizon("double_integrator_600")
    wd = cpu.beyond("double_integrator_600")
    with pytest.raises(ValueError, match="128"):
        Engine.connect_via_search_multi(crowd, [wd] * 129, [Hd] * 129, [NO] * 129, 1)
    with pytest.raises(ValueError, match="128"):
        Engine.connect_via_commit_multi(crowd, [(0, 13)] * 129, [wd] * 129, [Hd] * 129, 1)
    assert all(e.size == 1 for e in crowd)
    assert Engine.connect_via_search_multi(crowd[:128], [wd] * 128, [Hd] * 128, [NO] * 128, 1) == [(41, 0, 13)] * 128     # 128 engines are a call
    assert unchanged()
    # after all of it the engines still answer
    assert Engine.connect_via_search_multi(cars, [way] * 3, [H] * 3, [NO] * 3, 1) == [(1050, 213, 0)] * 3
    table.close()
    for e in everybody + crowd:
        e.close()
