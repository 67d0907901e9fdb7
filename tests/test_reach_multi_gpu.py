"""
Several trees asked about many goals per call on the device (csrc/reach_multi.hpp through lqrrt_reach_search_multi /
lqrrt_reach_commit_multi) against the reference of the rule (tests/reach_reference.py: a connect_reference.Connector per target and
tree, the C oracle's primitives), BIT FOR BIT, and against the one-tree calls on identically loaded twins: every (engine, target)
winner (cost, node), and every appended node's state, gain, parent, edge length and edge rows.  Every call holds engines of one
model, loaded from fixture prefixes of at most a few hundred nodes.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import connect_reference as cr
import reach_reference as rh
from test_connect_gpu import _compare_commit, _engine, _fill
from test_reach_multi_cpu import PINNED_CALLS, pinned_call

pytestmark = pytest.mark.gpu

NO = cr.NO_INCUMBENT


@functools.lru_cache(maxsize=None)
def _case(name):
    return cr.case(name)


def _load(name, size, extra=64):
    s, g = _case(name)
    return _engine(s, g, size, extra)


def _horizon(name):
    s, g = _case(name)
    return cr.horizon_of(s, g)


def _snapshot(eng):
    return eng.size, eng.states().copy(), eng.gains().copy(), eng.parents().copy(), eng.edge_lengths().copy(), eng.footprint()


def _unchanged(eng, snap):
    return eng.size == snap[0] and eng.footprint() == snap[5] and all(
        np.array_equal(a, b) for a, b in zip((eng.states(), eng.gains(), eng.parents(), eng.edge_lengths()), snap[1:5]))


def _car_targets(rows=slice(None)):
    s, g = _case("car_2000")
    pinned = rh.PINNED[("car_2000", 217)][rows]
    goals, bufs = rh.pinned_targets(s, g, pinned)
    return goals, bufs, [w for _, w in pinned]


@pytest.mark.parametrize("name", sorted(PINNED_CALLS))
def test_a_pinned_call_in_one_launch(name):
    """The pinned table's call in ONE reach_search_multi: engines that differ in size, T and goal_tries side by side.  A wrong
    engine, target index, goal, box or count shows as a wrong (cost, node).  Every row is also the engine's own reach_search on a
    twin, and nothing of any engine changes."""
    from lqrrt_amd.engine import Engine
    s, g, rows = pinned_call(name)
    H = _horizon(name)
    want = [rh.from_fixture(s, g, size).search(goals, bufs, goal_tries=tries) for size, tries, goals, bufs, _ in rows]
    assert want == [w for _, _, _, _, w in rows]                    # the table is the reference's
    engines = [_load(name, size) for size, _, _, _, _ in rows]
    twins = [_load(name, size) for size, _, _, _, _ in rows]
    snaps = [_snapshot(e) for e in engines]
    got = Engine.reach_search_multi(engines, [r[2] for r in rows], [r[3] for r in rows], [H] * len(rows), None, [r[1] for r in rows])
    print(name, got)
    assert got == want
    assert all(_unchanged(e, snap) for e, snap in zip(engines, snaps))   # keys, descriptors, tables and id lists are scratch
    for k, (size, tries, goals, bufs, _) in enumerate(rows):
        assert twins[k].reach_search(goals, bufs, H, None, tries) == got[k], k
    for e in engines + twins:
        e.close()


def test_grid_mapping_edges():
    """count_k = 1 next to 217 candidates; an engine with an empty id list in the middle; permuted id lists; T_k = 1 everywhere."""
    from lqrrt_amd.engine import Engine
    s, g = _case("car_2000")
    ref = rh.from_fixture(s, g, 217)
    H = ref.H
    goals, bufs, want = _car_targets(slice(0, 3))
    engines = [_load("car_2000", 217) for _ in range(4)]
    snaps = [_snapshot(e) for e in engines]
    perm = np.random.RandomState(5).permutation(217)
    one = ref.search(goals, bufs, nodes=[211])
    assert one[0] == (951, 211)
    few = [12, 211, 16]
    # engine 0: one candidate per target, every workgroup index of its slice is a target index; engine 1: no launch share
    got = Engine.reach_search_multi(engines, [goals] * 4, [bufs] * 4, [H] * 4, nodes=[[211], [], None, perm])
    assert got == [one, [None] * 3, want, want]
    got = Engine.reach_search_multi(engines, [goals[:1], goals, goals[1:2], goals], [bufs[:1], bufs, bufs[1:2], bufs], [H] * 4,
                                    nodes=[perm[::-1].copy(), few, [], np.sort(perm)])
    assert got == [want[:1], ref.search(goals, bufs, nodes=few), [None], want]
    assert Engine.reach_search_multi(engines[:2], [goals, goals], [bufs, bufs], [H] * 2, nodes=[[], []]) == [[None] * 3] * 2
    # T_k = 1 for every engine: one target each, a different one
    got = Engine.reach_search_multi(engines[:3], [goals[k:k + 1] for k in range(3)], [bufs[k] for k in range(3)], [H] * 3)
    assert got == [[w] for w in want]
    assert all(_unchanged(e, snap) for e, snap in zip(engines, snaps))
    for e in engines:
        e.close()


def test_more_engines_than_one_launch_holds():
    """33 double-integrator engines of one to five nodes: two chunks (32 + 1), two scratch owners.  Every row is the solo row."""
    from lqrrt_amd.engine import Engine
    name = "double_integrator_600"
    s, g, rows = pinned_call(name)
    H = _horizon(name)
    small = [r for r in rows if r[0] <= 5]                          # the (1, 8), (5, 2) and (5, 8) engines of the pinned call
    assert sorted(len(r[4]) for r in small) == [1, 4, 7]
    plan = [small[k % 3] for k in range(33)]
    engines = [_load(name, r[0], extra=16) for r in plan]
    got = Engine.reach_search_multi(engines, [r[2] for r in plan], [r[3] for r in plan], [H] * 33, None, [r[1] for r in plan])
    assert got == [r[4] for r in plan]
    twin = _load(name, plan[32][0], extra=16)
    assert twin.reach_search(plan[32][2], plan[32][3], H, None, plan[32][1]) == got[32]
    assert all(e.size == r[0] for e, r in zip(engines, plan))
    for e in engines + [twin]:
        e.close()


def test_every_engine_and_target_has_its_own_key():
    """The same target in two engines and twice within one engine, with incumbents 951 / 952 / none, in every arrangement."""
    from lqrrt_amd.engine import Engine
    s, g = _case("car_2000")
    H = _horizon("car_2000")
    own = np.asarray(s.goal, dtype=np.float64)[None, :]
    both, three = np.repeat(own, 2, axis=0), np.repeat(own, 3, axis=0)
    engines = [_load("car_2000", 217) for _ in range(3)]
    buf = s.goal_buffer
    hit = (951, 211)
    for incs, want in (([[951, 952], None, [952]], [[None, hit], [hit, hit], [hit]]),
                       ([[952, 951], [951, 951], None], [[hit, None], [None, None], [hit]]),
                       ([None, [NO, 951], [951]], [[hit, hit], [hit, None], [None]])):
        assert Engine.reach_search_multi(engines, [both, both, own], [buf] * 3, [H] * 3, incs) == want
    assert Engine.reach_search_multi(engines, [three, own, both], [buf] * 3, [H] * 3, [[951, 952, NO], [951], [952, 951]]) \
        == [[None, hit, hit], [None], [hit, None]]
    assert Engine.reach_search_multi(engines, [own] * 3, [buf] * 3, [H] * 3) == [[hit]] * 3
    for e in engines:
        e.close()


def _raw_search(engines, goals, lo, hi, T, nodes=None, counts=None, n=None):
    """lqrrt_reach_search_multi with the arrays as given: what Engine.reach_search_multi never passes."""
    from lqrrt_amd import _native as nat
    m = len(engines)
    ptrs = lambda arrays: (C.c_void_p * max(m, 1))(*[None if a is None else a.ctypes.data for a in arrays])   # noqa: E731
    T = np.ascontiguousarray(T, dtype=np.int32)
    H = np.ascontiguousarray([e.horizon_iters for e in engines] or [1], dtype=np.int32)
    tries = np.full(max(m, 1), 8, dtype=np.int32)
    cost = [np.zeros(max(int(t), 1), dtype=np.int64) for t in T]
    node = [np.zeros(max(int(t), 1), dtype=np.int32) for t in T]
    handles = (C.c_void_p * max(m, 1))(*[e.h for e in engines])
    return nat.check(nat.lib().lqrrt_reach_search_multi(
        handles, m if n is None else n, ptrs(goals), ptrs(lo), ptrs(hi), nat.ptr(T), None if nodes is None else ptrs(nodes),
        None if counts is None else nat.ptr(np.ascontiguousarray(counts, dtype=np.int32)), nat.ptr(tries), nat.ptr(H), None,
        ptrs(cost), ptrs(node), engines[0]._stream() if engines else None))


def test_refused_with_nothing_launched():
    from lqrrt_amd.engine import Engine
    s, g = _case("car_2000")
    cars = [_load("car_2000", 217) for _ in range(3)]
    boat = _load("boat_novice_300", 107)
    sb, _ = _case("boat_novice_300")
    H, Hb = _horizon("car_2000"), _horizon("boat_novice_300")
    n = s.nstates
    own = np.asarray(s.goal, dtype=np.float64)
    buf = np.abs(np.asarray(s.goal_buffer, dtype=np.float64))
    bad_goal = own.copy()
    bad_goal[1] = np.nan
    neg = buf.copy()
    neg[0] = -neg[0] - 1.0                                          # lo > hi in dimension 0
    snaps = [_snapshot(e) for e in cars + [boat]]
    ok = dict(engines=cars, goals=[[own]] * 3, buffers=[buf] * 3, horizons=[H] * 3)
    for kw, match in ((dict(engines=[], goals=[], buffers=[], horizons=[]), "no engines"),
                      (dict(engines=[cars[0], cars[1], cars[0]]), "twice"),
                      (dict(engines=[cars[0], boat], goals=[[own], [np.asarray(sb.goal, dtype=np.float64)]],
                            buffers=[buf, sb.goal_buffer], horizons=[H, Hb]), "model"),
                      (dict(goals=[[own], np.zeros((0, n)), [own]]), "targets"),                      # T_k = 0
                      (dict(goals=[[own], [own], np.repeat(own[None, :], 1025, axis=0)], nodes=[None, None, [0]]), "targets"),
                      (dict(goals=[[own], [own, bad_goal], [own]]), "finite"),
                      (dict(goals=[[own], [own], [own, own]], buffers=[buf, buf, [buf, neg]]), "empty"),
                      (dict(incumbents=[None, [0], None]), "incumbent"),
                      (dict(incumbents=[None, None, [2 ** 31]]), "incumbent"),
                      (dict(nodes=[None, None, [0, 217]]), "outside the tree"),
                      (dict(nodes=[[-1], None, None]), "outside the tree"),
                      (dict(goal_tries=[8, 8, 0]), "goal_tries"),
                      (dict(horizons=[H, H, H + 10 ** 6]), "horizon"),
                      # 1024 targets x 65536 candidates x 64 threads = 2^32: refused on the host, nothing launched
                      (dict(goals=[[own], [own], np.repeat(own[None, :], 1024, axis=0)],
                            nodes=[None, None, np.zeros(65536, dtype=np.int32)]), "exceed one launch")):
        with pytest.raises(ValueError, match=match):
            Engine.reach_search_multi(**dict(ok, **kw))
        assert all(_unchanged(e, snap) for e, snap in zip(cars + [boat], snaps)), kw
    for kw in (dict(goals=[[own]]), dict(buffers=[buf]), dict(incumbents=[None]), dict(nodes=[None]), dict(incumbents=[[NO, NO], None, None])):
        with pytest.raises(ValueError):                             # one entry per engine, one incumbent per goal
            Engine.reach_search_multi(**dict(ok, **kw))
    # what the wrapper cannot say: no engines at all, and an id list that comes without the array of counts
    goal1, lo1, hi1 = cars[0]._targets([own], buf)
    with pytest.raises(ValueError, match="no engines"):
        _raw_search(cars[:2], [goal1] * 2, [lo1] * 2, [hi1] * 2, [1, 1], n=0)
    ids = np.arange(217, dtype=np.int32)
    with pytest.raises(ValueError, match="without its count"):
        _raw_search(cars[:2], [goal1] * 2, [lo1] * 2, [hi1] * 2, [1, 1], nodes=[None, ids], counts=None)
    with pytest.raises(ValueError, match="null"):
        _raw_search(cars[:2], [goal1, None], [lo1] * 2, [hi1] * 2, [1, 1])
    assert _raw_search(cars[:2], [goal1] * 2, [lo1] * 2, [hi1] * 2, [1, 1], nodes=[None, ids], counts=[0, 217]) == 0
    assert all(_unchanged(e, snap) for e, snap in zip(cars + [boat], snaps))
    # the commit's refusals
    okc = dict(engines=cars, goals=[own] * 3, buffers=[buf] * 3, nodes=[211] * 3, horizons=[H] * 3)
    for kw, match in ((dict(engines=[cars[0], cars[1], cars[0]]), "twice"),
                      (dict(engines=[cars[0], boat, cars[1]]), "model|shape"),
                      (dict(goals=[own, bad_goal, own]), "finite"),
                      (dict(buffers=[buf, buf, neg]), "empty"),
                      (dict(nodes=[211, 211, 217]), "outside the tree"),
                      (dict(nodes=[211, -2, 211]), "candidate"),
                      (dict(goal_tries=[8, 0, 8]), "goal_tries"),
                      (dict(horizons=[H, H, H + 10 ** 6]), "horizon")):
        with pytest.raises(ValueError, match=match):
            Engine.reach_commit_multi(**dict(okc, **kw))
        assert all(_unchanged(e, snap) for e, snap in zip(cars + [boat], snaps)), kw
    assert Engine.reach_search_multi(**ok) == [[(951, 211)]] * 3
    for e in cars + [boat]:
        e.close()


class _Batched(object):
    """An engine whose connect_commit hands out what a batched commit appended to it: what test_connect_gpu._compare_commit drives."""

    def __init__(self, eng, ids):
        self._eng, self._ids = eng, ids

    def connect_commit(self, node, horizon_iters, goal_tries=8):
        return self._ids

    def __getattr__(self, name):
        return getattr(self._eng, name)


def test_commit_three_targets_one_without_winner_one_without_room():
    """Four engines, three different targets: one engine has no winner (None), one has room for one node of its two-node chain and
    gets None with its tree unchanged, the others commit what Connector(goal=...).commit_chain appends."""
    from lqrrt_amd.engine import Engine
    s, g = _case("car_2000")
    goals, bufs, want = _car_targets()
    ref = rh.from_fixture(s, g, 217)
    H = ref.H
    rows = [1, 4, 6, 0]                                             # "node 40", "node 200", "far" (no winner), the own goal
    engines = [_load("car_2000", 217), _load("car_2000", 217), _load("car_2000", 217), _load("car_2000", 217, extra=1)]
    full = _fill(engines[3], g["state"][0], g["K"][0])
    ids217 = list(range(217))                                       # (the copies of the root that fill the tree are not candidates)
    parents, lens = engines[3].parents(), engines[3].edge_lengths()
    fp0 = [e.footprint() for e in engines]
    got = Engine.reach_search_multi(engines, [goals[r:r + 1] for r in rows], [bufs[r] for r in rows], [H] * 4,
                                    nodes=[None, None, None, ids217])
    assert got == [[want[r]] for r in rows] and got[2] == [None]
    new = Engine.reach_commit_multi(engines, [goals[r] for r in rows], [bufs[r] for r in rows],
                                    [None if w[0] is None else w[0][1] for w in got], [H] * 4)
    assert new[2] == [] and engines[2].size == 217
    assert new[3] is None and engines[3].size == full
    assert np.array_equal(engines[3].parents(), parents) and np.array_equal(engines[3].edge_lengths(), lens)
    for k in (0, 1):
        con = ref.connector(goals[rows[k]], bufs[rows[k]])
        win = con.search()
        assert (win[0], win[1]) == want[rows[k]]
        plan, ids = _compare_commit(_Batched(engines[k], new[k]), con, win, H)
        assert plan == con.climb(win[1]) + ids and con.in_goal(engines[k].states(ids[-1], 1)[0])
    assert [e.footprint() for e in engines] == fp0
    # the engines' own goal and box are what they were: the old question has its old answer on the old nodes
    assert Engine.connect_search_multi(engines, [H] * 4, [NO] * 4, nodes=[ids217] * 4) == [(951, 211)] * 4
    for e in engines:
        e.close()


def test_a_chain_that_misses_its_target_fails_alone():
    from lqrrt_amd import _native as nat
    from lqrrt_amd.engine import Engine
    s, g = _case("car_2000")
    goals, bufs, want = _car_targets()
    ref = rh.from_fixture(s, g, 217)
    H = ref.H
    assert ref.connector(goals[4], bufs[4]).chain(0) is None        # eight steers from the root do not reach target "node 200"
    engines = [_load("car_2000", 217) for _ in range(4)]
    with pytest.raises(nat.NativeError) as ex:                      # engine 1: a node whose chain falls short; engine 2: the far target
        Engine.reach_commit_multi(engines, [goals[1], goals[4], goals[6], goals[0]], [bufs[1], bufs[4], bufs[6], bufs[0]],
                                  [want[1][1], 0, 211, None], [H] * 4)
    assert ex.value.code == nat.E_STATE and ex.value.failed == [1, 2]
    res = ex.value.results
    assert res[1] is None and res[2] is None and res[3] == [] and [e.size for e in engines[1:]] == [217] * 3
    con = ref.connector(goals[1], bufs[1])
    _compare_commit(_Batched(engines[0], res[0]), con, con.search(), H)
    assert Engine.connect_search_multi(engines[1:], [H] * 3, [NO] * 3) == [(951, 211)] * 3
    assert Engine.reach_search_multi(engines[1:], [goals[:5]] * 3, [bufs[:5]] * 3, [H] * 3) == [want[:5]] * 3
    for e in engines:
        e.close()
