"""
The rectangle clearance queries for several trees per launch on the device (csrc/clear_rects_multi.hpp through
lqrrt_tree_clear_rects_multi / lqrrt_tree_clear_rects_wait_multi, Engine.tree_clear_rects_multi / tree_clear_rects_wait_multi,
lqrrt_amd.avoids_rects).  Every member's answer must EQUAL that of the one-tree call on its engine -- counters and per-node arrays are
integers and masks -- and, for the hand-built trees and the fixtures, the reference of the rule (tests/clear_rects_reference.py,
tests/clear_rects_wait_reference.py).  tests/test_clear_rects_multi_cpu.py shows with the references alone that none of the inputs
(tests/clear_rects_multi_inputs.py) is degenerate.  Trees have at most 257 nodes, apart from the two committed fixtures.
"""
import ctypes as C

import numpy as np
import pytest

import clear_reference as cl
import clear_rects_reference as cr
import clear_rects_wait_reference as rw
import clear_rects_multi_inputs as mi
import retain_reference as rr
from clear_common import WAVE, _grown, _load

pytestmark = pytest.mark.gpu


def _load_case(c, system=None):
    return _load(c.native() if system is None else system, c.tree, cl.H_HAND, goal=c.tree.goal, goal_buffer=c.tree.goal_buffer)


def _same(got, want):
    assert got[0] == want[0]
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[2], want[2])
    assert got[1].dtype == want[1].dtype and got[2].dtype == want[2].dtype


def _close(engines):
    for e in engines:
        e.close()


# ------------------------------------------------------------------------------------------------ 1. every hand-built case at once

def test_every_hand_built_case_in_one_call():
    from lqrrt_amd.engine import Engine
    groups = mi.by_model(mi.plain_cases(), lambda c: c.tree.system)
    assert len(groups["boat_advanced"]) > 16 and {c.tree.size for c in groups["boat_advanced"]} >= {1, 11, 256, 257}
    for system, cases in sorted(groups.items()):
        engines = [_load_case(c) for c in cases]
        solo = [e.tree_clear_rects(c.tracks, c.extents, c.start, per_node=True) for e, c in zip(engines, cases)]
        for order in (list(range(len(cases))), list(range(len(cases)))[::-1]):
            pick = lambda seq: [seq[k] for k in order]
            args = (pick(engines), [c.tracks for c in pick(cases)], [c.extents for c in pick(cases)], [c.start for c in pick(cases)])
            got = Engine.tree_clear_rects_multi(*args, per_node=True)
            for k, g in zip(order, got):
                ref = cases[k].reference()
                _same(g, solo[k])
                _same(g, (ref["stats"], ref["first"], ref["dwell_first"]))
            assert Engine.tree_clear_rects_multi(*args) == [solo[k][0] for k in order]      # the counters alone: the same call without the arrays
        _close(engines)


# ------------------------------------------------------------------------------------------------ 2. every wait case at once

def test_every_hand_built_wait_case_in_one_call():
    from lqrrt_amd.engine import Engine
    groups = mi.by_model(mi.wait_cases(), lambda c: c.case.tree.system)
    assert len(groups["boat_advanced"]) > 32 and {c.W for c in groups["boat_advanced"]} >= {1, 8, 63, 64}      # (two chunks)
    for system, cases in sorted(groups.items()):
        engines = [_load_case(c.case) for c in cases]
        solo = [e.tree_clear_rects_wait(c.case.tracks, c.case.extents, c.case.start, c.W, per_node=True) for e, c in zip(engines, cases)]
        for order in (list(range(len(cases))), list(range(len(cases)))[::-1]):
            pick = lambda seq: [seq[k] for k in order]
            got = Engine.tree_clear_rects_wait_multi(pick(engines), [c.case.tracks for c in pick(cases)], [c.case.extents for c in pick(cases)],
                                                     [c.case.start for c in pick(cases)], [c.W for c in pick(cases)], per_node=True)
            for k, g in zip(order, got):
                ref = cases[k].reference()
                _same(g, solo[k])
                _same(g, (ref["stats"], ref["clear"], ref["dwell_ok"]))
        _close(engines)


# ------------------------------------------------------------------------------------------------ 3. chunk edges

@pytest.mark.parametrize("n", mi.CHUNK_SIZES)
def test_chunk_edges(n):
    """n fork trees, every member with a start and a W of its own: a member that read another's descriptor would answer for those."""
    from lqrrt_amd.engine import Engine
    c = cr.case(mi.FORK)
    engines = [_load_case(c) for _ in range(n)]
    starts, waits = mi.starts(n), mi.waits(n)
    assert n < 33 or starts[31] != starts[32]
    got = Engine.tree_clear_rects_multi(engines, [c.tracks] * n, [c.extents] * n, starts, per_node=True)
    for e, s, g in zip(engines, starts, got):
        ref = mi.fork_reference(s)
        _same(g, (ref["stats"], ref["first"], ref["dwell_first"]))
        _same(g, e.tree_clear_rects(c.tracks, c.extents, s, per_node=True))
    got = Engine.tree_clear_rects_wait_multi(engines, [c.tracks] * n, [c.extents] * n, starts, waits, per_node=True)
    for e, s, w, g in zip(engines, starts, waits, got):
        ref = mi.fork_wait_reference(s, w)
        _same(g, (ref["stats"], ref["clear"], ref["dwell_ok"]))
        _same(g, e.tree_clear_rects_wait(c.tracks, c.extents, s, w, per_node=True))
    _close(engines)


# ------------------------------------------------------------------------------------------------ 4. the largest hull wins the LDS

@pytest.mark.parametrize("big_first", [True, False])
def test_the_largest_hull_sizes_the_lds(big_first):
    from lqrrt_amd.engine import Engine
    big = cr.case("ros_boat on an occupied grid, 3073 hull points, D = 65")
    small = cr.case("ros_boat: the fork")
    assert big.vps().shape[1] == 3073 and small.vps().shape[1] < 64
    cases = [big, small] if big_first else [small, big]
    engines = [_load_case(c) for c in cases]
    args = (engines, [c.tracks for c in cases], [c.extents for c in cases], [c.start for c in cases])
    got = Engine.tree_clear_rects_multi(*args, per_node=True)
    gotw = Engine.tree_clear_rects_wait_multi(*args, 8, per_node=True)
    for e, c, g, gw in zip(engines, cases, got, gotw):
        ref, refw = c.reference(), rw.WaitCase(c, 8).reference()
        _same(g, (ref["stats"], ref["first"], ref["dwell_first"]))
        _same(g, e.tree_clear_rects(c.tracks, c.extents, c.start, per_node=True))
        _same(gw, (refw["stats"], refw["clear"], refw["dwell_ok"]))
        _same(gw, e.tree_clear_rects_wait(c.tracks, c.extents, c.start, 8, per_node=True))
    _close(engines)


# ------------------------------------------------------------------------------------------------ 5. a shared table

def test_members_that_share_a_table():
    from lqrrt_amd.engine import Engine
    c = cr.case(mi.FORK)
    other = mi.moved_tracks().copy()
    engines = [_load_case(c) for _ in range(5)]
    tables, extents = [c.tracks] * 4 + [other], [c.extents] * 4 + [c.extents.copy()]
    starts = list(mi.SHARE_STARTS)
    refs = [mi.fork_reference(s) for s in starts[:4]] + [mi.moved_reference(starts[4])]
    assert refs[0]["stats"] != refs[4]["stats"] and not np.array_equal(refs[0]["first"], refs[1]["first"])      # (of the inputs)
    got = Engine.tree_clear_rects_multi(engines, tables, extents, starts, per_node=True)
    for e, t, x, s, g, ref in zip(engines, tables, extents, starts, got, refs):
        _same(g, (ref["stats"], ref["first"], ref["dwell_first"]))
        _same(g, e.tree_clear_rects(t, x, s, per_node=True))
    # the copy in the middle: the members on both sides of it still share
    mid = [tables[0], tables[0], other, tables[0], tables[0]]
    mid_e = [extents[0], extents[0], extents[4], extents[0], extents[0]]
    got = Engine.tree_clear_rects_wait_multi(engines, mid, mid_e, starts, 8, per_node=True)
    for k, (e, t, x, s, g) in enumerate(zip(engines, mid, mid_e, starts, got)):
        ref = mi.fork_wait_reference(s, 8, moved=(k == 2))
        _same(g, (ref["stats"], ref["clear"], ref["dwell_ok"]))
        _same(g, e.tree_clear_rects_wait(t, x, s, 8, per_node=True))
    _close(engines)


def test_novice_boats_that_differ_in_inflation_do_not_share_a_table():
    """The same tracks and extents objects, equal L and D, but P.p[18] differs: the extents tail of the table differs, each its own."""
    from lqrrt_amd.engine import Engine
    c = cr.case("boat_novice: the fork")
    slim = c.native()
    slim.boat_length = slim.boat_length / 4
    systems = [c.native(), slim, c.native()]
    engines = [_load_case(c, s) for s in systems]
    t = c.tree
    lo, hi = t.box()
    refs = [cr.clear_rects(t.state, t.pID, t.elen, t.xedge, cr.row_test_of(s), c.tracks, c.extents, 0, lo, hi) for s in systems]
    assert refs[0]["stats"] == c.reference()["stats"] and not np.array_equal(refs[0]["first"], refs[1]["first"])      # (of the inputs)
    got = Engine.tree_clear_rects_multi(engines, [c.tracks] * 3, [c.extents] * 3, [0, 0, 0], per_node=True)
    gotw = Engine.tree_clear_rects_wait_multi(engines, [c.tracks] * 3, [c.extents] * 3, [0, 0, 0], 8, per_node=True)
    for e, g, gw, ref in zip(engines, got, gotw, refs):
        _same(g, (ref["stats"], ref["first"], ref["dwell_first"]))
        _same(g, e.tree_clear_rects(c.tracks, c.extents, 0, per_node=True))
        _same(gw, e.tree_clear_rects_wait(c.tracks, c.extents, 0, 8, per_node=True))
    _close(engines)


# ------------------------------------------------------------------------------------------------ 6. refusals

def _raw(call, stats, dtype, engines, tracks, extents, L, D, start, waits=None):
    """The ABI call itself, with output arrays that hold sentinels; returns (rc, stats bytes, per-node arrays)."""
    from lqrrt_amd import _native as nat
    n = len(engines)
    handles = (C.c_void_p * max(n, 1))(*[e.h for e in engines])
    tp = (C.c_void_p * max(n, 1))(*[None if t is None else t.ctypes.data for t in tracks])
    xp = (C.c_void_p * max(n, 1))(*[None if x is None else x.ctypes.data for x in extents])
    out = (stats * max(n, 1))()
    C.memset(out, 0x5a, C.sizeof(out))
    a = [np.full(max(e.size, 1), 77, dtype=dtype) for e in engines]
    b = [np.full(max(e.size, 1), 77, dtype=dtype) for e in engines]
    ap = (C.c_void_p * max(n, 1))(*[x.ctypes.data for x in a])
    bp = (C.c_void_p * max(n, 1))(*[x.ctypes.data for x in b])
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)
    L, D, start = i32(L), i32(D), i32(start)
    extra = () if waits is None else (nat.ptr(i32(waits)),)
    rc = getattr(nat.lib(), call)(handles, n, tp, xp, nat.ptr(L), nat.ptr(D), nat.ptr(start), *extra, out, ap, bp,
                                  engines[0]._stream() if engines else None)
    return rc, bytes(out), a, b


PLAIN = ("lqrrt_tree_clear_rects_multi", "ClearStats", np.int32)
WAIT = ("lqrrt_tree_clear_rects_wait_multi", "ClearWaitStats", np.uint64)


def test_refusals_on_the_device():
    import lqrrt_amd
    from lqrrt_amd import _native as nat
    from lqrrt_amd.engine import Engine
    c = cr.case(mi.FORK)
    engines = [_load_case(c) for _ in range(3)]
    tr, ex = np.ascontiguousarray(c.tracks), np.ascontiguousarray(c.extents)
    L, D = tr.shape[:2]
    good = Engine.tree_clear_rects_multi(engines, [tr] * 3, [ex] * 3, [0, 1, 2], per_node=True)
    goodw = Engine.tree_clear_rects_wait_multi(engines, [tr] * 3, [ex] * 3, [0, 1, 2], [8, 1, 64], per_node=True)
    fps = [e.footprint() for e in engines]
    badpos, badhead, negext, infext = tr.copy(), tr.copy(), ex.copy(), ex.copy()
    badpos[-1, -1, 1] = np.inf
    badhead[0, 0, 2] = np.nan
    negext[-1, 1] = -1e-300
    infext[0, 0] = np.inf

    def raw(which, *args, **kw):
        return _raw(which[0], getattr(nat, which[1]), which[2], *args, **kw)

    def refused(raw_, code, who, what=None):
        msg = (nat.lib().lqrrt_last_error() or b"").decode()
        rc, out, a, b = raw_
        assert rc == code, (rc, msg)
        if who is not None:
            assert msg.endswith("(engine %d)" % who), msg
        if what:
            assert what in msg, msg
        assert set(out) == {0x5a} and all((x == 77).all() for x in a + b)            # nothing was written into any output

    # any one member's bad argument refuses the whole call, with the solo call's message, and names the engine: one per check
    for who in (0, 2):
        def member(good_value, bad_value):
            return [bad_value if k == who else good_value for k in range(3)]
        for kw, what in ((dict(tracks=member(tr, None)), "null argument"), (dict(extents=member(ex, None)), "null argument"),
                         (dict(L=member(L, 0)), "L >= 1"), (dict(D=member(D, 0)), "D >= 1"), (dict(start=member(0, -1)), "start must be >= 0"),
                         (dict(L=member(L, 2 ** 20), D=member(D, 2 ** 10)), "too large"),
                         (dict(tracks=member(tr, badpos)), "position"), (dict(tracks=member(tr, badhead)), "heading"),
                         (dict(extents=member(ex, negext)), "half width"), (dict(extents=member(ex, infext)), "half length"),
                         (dict(start=member(0, 2 ** 31 - 16)), "31 bits")):
            args = dict(tracks=[tr] * 3, extents=[ex] * 3, L=[L] * 3, D=[D] * 3, start=[0] * 3)
            args.update(kw)
            refused(raw(PLAIN, engines, **args), nat.E_ARG, who, what)
            refused(raw(WAIT, engines, waits=[8] * 3, **args), nat.E_ARG, who, what)
        for w in (0, 65):
            refused(raw(WAIT, engines, [tr] * 3, [ex] * 3, [L] * 3, [D] * 3, [0] * 3, waits=member(8, w)), nat.E_ARG, who, "waits must be 1 .. 64")
        # start + the longest wait + the deepest cum (16) = 2^31
        refused(raw(WAIT, engines, [tr] * 3, [ex] * 3, [L] * 3, [D] * 3, member(0, 2 ** 31 - 17 - 6), waits=member(1, 8)), nat.E_ARG, who,
                "start + the longest wait + the deepest")
    # two bad members: the first in list order is named
    refused(raw(PLAIN, engines, [tr] * 3, [ex, negext, infext], [L] * 3, [D] * 3, [0] * 3), nat.E_ARG, 1, "half width")
    # the engine list: an engine twice, n = 0, n = 129, null arrays
    for which, extra in ((PLAIN, {}), (WAIT, dict(waits=[8] * 3))):
        refused(raw(which, [engines[0], engines[1], engines[0]], [tr] * 3, [ex] * 3, [L] * 3, [D] * 3, [0] * 3, **extra), nat.E_ARG, None, "twice")
    st = (nat.ClearStats * 1)()
    one = (C.c_void_p * 1)(engines[0].h)
    assert nat.lib().lqrrt_tree_clear_rects_multi(one, 0, None, None, None, None, None, st, None, None, None) == nat.E_ARG
    assert nat.lib().lqrrt_tree_clear_rects_multi(one, 1, None, None, None, None, None, st, None, None, None) == nat.E_ARG
    many = (C.c_void_p * 129)(*[engines[k % 3].h for k in range(129)])
    ptrs = (C.c_void_p * 129)(*[tr.ctypes.data] * 129)
    xptrs = (C.c_void_p * 129)(*[ex.ctypes.data] * 129)
    ints = np.zeros(129, dtype=np.int32)
    st129 = (nat.ClearStats * 129)()
    assert nat.lib().lqrrt_tree_clear_rects_multi(many, 129, ptrs, xptrs, nat.ptr(ints), nat.ptr(ints), nat.ptr(ints), st129, None, None, None) == nat.E_ARG
    stw = (nat.ClearWaitStats * 1)()
    i1 = np.array([L], dtype=np.int32)
    assert nat.lib().lqrrt_tree_clear_rects_wait_multi(one, 1, (C.c_void_p * 1)(tr.ctypes.data), (C.c_void_p * 1)(ex.ctypes.data), nat.ptr(i1),
                                                       nat.ptr(np.array([D], dtype=np.int32)), nat.ptr(np.zeros(1, dtype=np.int32)), None, stw,
                                                       None, None, None) == nat.E_ARG            # the wait call without waits
    with pytest.raises(ValueError, match="twice"):
        Engine.tree_clear_rects_multi([engines[0], engines[0]], [tr] * 2, [ex] * 2, [0, 0])
    with pytest.raises(ValueError, match=r"\(engine 1\)"):
        Engine.tree_clear_rects_wait_multi(engines, [tr] * 3, [ex] * 3, [0, 2 ** 31 - 16, 0], 1)
    # after all that the same engines answer as before, and no footprint has moved
    for g, w in zip(Engine.tree_clear_rects_multi(engines, [tr] * 3, [ex] * 3, [0, 1, 2], per_node=True), good):
        _same(g, w)
    for g, w in zip(Engine.tree_clear_rects_wait_multi(engines, [tr] * 3, [ex] * 3, [0, 1, 2], [8, 1, 64], per_node=True), goodw):
        _same(g, w)
    assert [e.footprint() for e in engines] == fps

    # two models in one call
    car = cr.case("car: the fork")
    ecar = _load_case(car)
    for call, extra in ((Engine.tree_clear_rects_multi, ()), (Engine.tree_clear_rects_wait_multi, (8,))):
        with pytest.raises(ValueError, match="share the device and the model"):
            call([engines[0], ecar], [tr, car.tracks], [ex, car.extents], [0, 0], *extra)
    ecar.close()
    # a member without a goal, and one with an empty tree (no resolution yet): named, E_STATE
    engines[1].set_resolution(0.1, 0.0, cl.H_HAND, np.ones(6), None, None)
    xe, ue = c.tree.packed()
    engines[1].tree_load(c.tree.state, c.tree.K, c.tree.pID, c.tree.elen, xe, ue)
    for call, extra in ((Engine.tree_clear_rects_multi, ()), (Engine.tree_clear_rects_wait_multi, (8,))):
        with pytest.raises(nat.NativeError) as err:
            call(engines, [tr] * 3, [ex] * 3, [0, 0, 0], *extra)
        assert err.value.code == nat.E_STATE and "goal" in str(err.value) and "(engine 1)" in str(err.value)
    empty = Engine(c.native(), capacity=64, max_wave=64)
    with pytest.raises(nat.NativeError) as err:
        Engine.tree_clear_rects_multi([engines[0], engines[2], empty], [tr] * 3, [ex] * 3, [0, 0, 0])
    assert err.value.code == nat.E_STATE and "no tree" in str(err.value) and "(engine 2)" in str(err.value)
    empty.close()
    # a hull beyond a workgroup's LDS, as the second member
    big = lqrrt_amd.systems.BoatAdvanced(0)
    big.vps = np.random.RandomState(0).uniform(-1, 1, (2, 20000))
    big.set_obstacles(np.zeros((0, 3)))
    big.goal, big.goal_buffer = [float(v) for v in c.tree.goal], [float(v) for v in c.tree.goal_buffer]
    e3 = _load(big, c.tree, cl.H_HAND, goal=c.tree.goal, goal_buffer=c.tree.goal_buffer)
    for call, extra in ((Engine.tree_clear_rects_multi, ()), (Engine.tree_clear_rects_wait_multi, (8,))):
        with pytest.raises(ValueError, match="LDS") as err:
            call([engines[0], e3], [tr] * 2, [ex] * 2, [0, 0], *extra)
        assert "(engine 1)" in str(err.value)
    e3.close()
    _close(engines)
    # models without a circle path
    s = lqrrt_amd.systems.DoubleIntegrator(n_boxes=8, seed=1)
    e2 = Engine(s, capacity=64, max_wave=64)
    e2.set_resolution(0.1, 0.0, 4, np.ones(s.nstates), s.goal, np.abs(np.asarray(s.goal_buffer, dtype=np.float64)))
    e2.tree_reset(s.x0)
    for call, name, extra in ((Engine.tree_clear_rects_multi, "lqrrt_tree_clear_rects:", ()),
                              (Engine.tree_clear_rects_wait_multi, "lqrrt_tree_clear_rects_wait:", (8,))):
        with pytest.raises(nat.NativeError) as err:
            call([e2], [np.zeros((2, 1, 3))], [(1.0, 0.5)], [0], *extra)
        assert err.value.code == nat.E_STATE and "circle" in str(err.value) and name in str(err.value) and "(engine 0)" in str(err.value)
    e2.close()


def test_a_generic_engine_is_refused():
    from lqrrt_amd import _native as nat
    from lqrrt_amd.engine import NodeTable
    table = NodeTable(4, 1, (2,), capacity=128)
    tr, ex, one, zero = np.zeros((2, 1, 3)), np.array([[1.0, 0.5]]), np.array([1], dtype=np.int32), np.array([0], dtype=np.int32)
    two = np.array([2], dtype=np.int32)
    for call, stats, extra in (("lqrrt_tree_clear_rects_multi", nat.ClearStats, ()),
                               ("lqrrt_tree_clear_rects_wait_multi", nat.ClearWaitStats, (nat.ptr(one),))):
        out = (stats * 1)()
        C.memset(out, 0x5a, C.sizeof(out))
        rc = getattr(nat.lib(), call)((C.c_void_p * 1)(table.h), 1, (C.c_void_p * 1)(tr.ctypes.data), (C.c_void_p * 1)(ex.ctypes.data),
                                      nat.ptr(two), nat.ptr(one), nat.ptr(zero), *extra, out, None, None, None)
        assert rc == nat.E_STATE and "GENERIC" in nat.lib().lqrrt_last_error().decode()
        assert set(bytes(out)) == {0x5a}
    table.close()


# ------------------------------------------------------------------------------------------------ 7. nothing is modified

def test_nothing_of_any_tree_is_modified_and_the_trees_grow_on_as_their_twins():
    from lqrrt_amd.engine import Engine
    made = [_grown(1), _grown(2)]
    s, engines = made[0][0], [m[1] for m in made]
    twins = [_grown(1)[1], _grown(2)[1]]
    before = [rr.engine_arrays(e) for e in engines]
    kept = [(e.ignored(), e.plan_best(), e.footprint(), e.counters().as_dict(), e.get_mt19937()) for e in engines]
    L = 300
    tables, extents = [], [np.array([[3.0, 1.0], [2.0, 0.5]]), np.array([[2.5, 0.8], [1.5, 0.6]])]
    for e in engines:
        states = e.states()
        tr = np.zeros((L, 2, 3))
        tr[:, 0, :2] = states[len(states) // 2, :2]
        tr[:, 0, 2] = 0.4
        tr[:, 1, 0] = states[len(states) // 3, 0]
        tr[:, 1, 1] = states[len(states) // 3, 1] + 0.2 * (np.arange(L) - 40)
        tr[:, 1, 2] = np.pi / 2
        tables.append(tr)
    lo, hi = rr.goal_box(s)
    got = Engine.tree_clear_rects_multi(engines, tables, extents, [3, 0], per_node=True)
    gotw = Engine.tree_clear_rects_wait_multi(engines, tables, extents, [3, 0], [16, 5], per_node=True)
    for k, (e, start, W) in enumerate(zip(engines, (3, 0), (16, 5))):
        ref = cr.clear_rects(before[k][0], before[k][2], before[k][3], before[k][4], cr.row_test_of(s), tables[k], extents[k], start, lo, hi)
        _same(got[k], (ref["stats"], ref["first"], ref["dwell_first"]))
        assert got[k][0]["conflicts"] > 0
        _same(got[k], e.tree_clear_rects(tables[k], extents[k], start, per_node=True))
        _same(gotw[k], e.tree_clear_rects_wait(tables[k], extents[k], start, W, per_node=True))
    assert any(g[0]["blocked"] > 0 for g in got)
    for k, e in enumerate(engines):
        for a, b in zip(before[k], rr.engine_arrays(e)):
            np.testing.assert_array_equal(a, b)
        ign, best, fp, counters, mt = kept[k]
        np.testing.assert_array_equal(e.ignored(), ign)
        assert e.plan_best() == best and e.footprint() == fp and e.counters().as_dict() == counters
        key, pos = e.get_mt19937()
        assert pos == mt[1] and np.array_equal(key, mt[0])
    for e, twin in zip(engines, twins):
        for x in (e, twin):
            x.extend(WAVE, node_limit=900)
        assert e.size == twin.size >= 900
        (sa, Ka, pa, la, xa, ua), (sb, Kb, pb, lb, xb, ub) = rr.engine_arrays(e), rr.engine_arrays(twin)
        for a, b in ((sa, sb), (Ka, Kb), (pa, pb), (la, lb)):
            np.testing.assert_array_equal(a, b)
        live = np.arange(xa.shape[1])[None, :] < la[:, None]       # (pool rows beyond an edge's length are never written)
        np.testing.assert_array_equal(xa[live], xb[live])
        np.testing.assert_array_equal(ua[live], ub[live])
        np.testing.assert_array_equal(e.ignored(), twin.ignored())
        assert e.plan_best() == twin.plan_best()
    _close(engines + twins)


# ------------------------------------------------------------------------------------------------ 8. fixtures

@pytest.mark.parametrize("name", ["car_2000", "boat_advanced_3000"])
def test_fixture_trees(name):
    """The fixture twice in one call, at start 0 and at start 3 (two models: they cannot share a call), plain and W = FIXTURE_W."""
    from lqrrt_amd.engine import Engine
    f = cl.fixture(name)
    s = f.native()
    engines = [_load(s, f, f.H, dt=s.plan_kwargs["dt"]) for _ in range(2)]
    tracks, extents = cr.fixture_tracks(f)
    W = rw.FIXTURE_W
    got = Engine.tree_clear_rects_multi(engines, [tracks] * 2, [extents] * 2, [0, 3], per_node=True)
    gotw = Engine.tree_clear_rects_wait_multi(engines, [tracks] * 2, [extents] * 2, [0, 3], W, per_node=True)
    for e, start, g, gw in zip(engines, (0, 3), got, gotw):
        _same(g, e.tree_clear_rects(tracks, extents, start, per_node=True))
        _same(gw, e.tree_clear_rects_wait(tracks, extents, start, W, per_node=True))
    ref, refw = cr.fixture_reference(name), rw.fixture_reference(name)
    _same(got[0], (ref["stats"], ref["first"], ref["dwell_first"]))
    _same(gotw[0], (refw["stats"], refw["clear"], refw["dwell_ok"]))
    assert not np.array_equal(got[0][1], got[1][1]) and not np.array_equal(gotw[0][1], gotw[1][1])      # the start matters
    assert got[0][0]["clear_hits"] > 0 and any(0 < int(m) < rw.all_mask(W) for m in gotw[0][1])
    _close(engines)


# ------------------------------------------------------------------------------------------------ 9. planner level

def _plan_of(p):
    return (list(p.node_seq), np.asarray(p.x_seq, dtype=np.float64), np.asarray(p.u_seq, dtype=np.float64), p.T, p.plan_wait,
            bool(p.plan_reached_goal), p.tree.size)


def _same_plans(planners, twins):
    for p, t in zip(planners, twins):
        a, b = _plan_of(p), _plan_of(t)
        assert a[0] == b[0] and a[3:] == b[3:]
        np.testing.assert_array_equal(a[1], b[1])
        np.testing.assert_array_equal(a[2], b[2])
        np.testing.assert_array_equal(np.asarray(p.t_seq), np.asarray(t.t_seq))


class _Counted(object):
    """Engine's two fleet calls wrapped so that every native call is counted."""

    def __init__(self, monkeypatch):
        from lqrrt_amd.engine import Engine
        self.calls = []
        for name in ("tree_clear_rects_multi", "tree_clear_rects_wait_multi"):
            inner = getattr(Engine, name)
            monkeypatch.setattr(Engine, name, staticmethod(lambda *a, _inner=inner, _name=name, **k: self.calls.append((_name, len(a[0]))) or _inner(*a, **k)))

    def take(self):
        out, self.calls = self.calls, []
        return out


def test_avoids_rects_is_the_loop_of_avoid_rects(monkeypatch):
    import lqrrt_amd as lqrrt
    import test_clear_rects_wait_gpu as trw
    seeds = (1, 2, 3)
    made, twins = [trw._car_planner(seed, 700) for seed in seeds], [trw._car_planner(seed, 700)[1] for seed in seeds]
    planners = [m[1] for m in made]
    _same_plans(planners, twins)
    # of the inputs, with the reference alone (as test_avoid_rects_waits_at_the_start): a gate on the shortest plan of the first
    # planner's tree that a wait of 1 .. 7 rows answers best
    s, p = made[0]
    state, pID, elen, xedge, _, _ = trw._tree_of(s, p)
    far = np.zeros((1, 1, 3))
    far[0, 0, :2] = 900.0
    short = trw._reference_of(s, p, far, (0.5, 0.5), 0, 1)["stats"]["best_end"]
    rows = np.concatenate([xedge[v, :elen[v]] for v in p._engine.climb(short)])
    speed = np.linalg.norm(np.diff(rows[:, :2], axis=0), axis=1)
    for c in np.argsort(-speed)[:40:8]:
        tracks, extents = trw._gate(rows, int(c))
        ref = trw._reference_of(s, p, tracks, extents, 0, 8)
        if ref["stats"]["best_wait"] >= 1:
            break
    assert ref["stats"]["best_wait"] >= 1 and not int(ref["clear"][short]) & 1
    counted = _Counted(monkeypatch)
    asked = []
    for t in twins:                                                               # every twin's solo plain call, noted
        mine, plain_call = [], t._engine.tree_clear_rects
        t._engine.tree_clear_rects = lambda *a, _mine=mine, _call=plain_call, **k: _mine.append(a[2]) or _call(*a, **k)
        asked.append(mine)
    changed = False
    for max_wait, adopt in ((0, False), (7, False), (7, True), (0, True)):
        want = [t.avoid_rects(tracks, extents, 0, adopt, max_wait) for t in twins]
        assert counted.take() == []                                               # (the loop goes through the solo calls)
        again = sum(len(a) for a in asked) if max_wait else 0                     # the twins that needed the plain query for plan_first
        for a in asked:
            del a[:]
        got = lqrrt.avoids_rects(planners, tracks, extents, 0, adopt, max_wait)
        print(max_wait, adopt, got)
        assert got == want
        _same_plans(planners, twins)
        # one native call for the group, and with max_wait ONE more, for the planners whose plan does not hold
        calls = counted.take()
        if max_wait == 0:
            assert calls == [("tree_clear_rects_multi", 3)]
        else:
            assert calls == [("tree_clear_rects_wait_multi", 3)] + ([("tree_clear_rects_multi", again)] if again else [])
        if max_wait == 7 and not changed:
            assert {k: got[0][k] for k in rw.STAT_KEYS} == ref["stats"]
        changed = changed or adopt
    assert any(g["best_end"] >= 0 for g in got)
    # a gate on the plan the first planner HOLDS now (wait rows included), where it is fastest: by the reference that plan is hit at
    # its departure, so the wait query cannot show it to hold and the second, plain call is made -- for that planner at least
    held = np.asarray(p.x_seq, dtype=np.float64)
    speed = np.linalg.norm(np.diff(held[:, :2], axis=0), axis=1)
    tracks2, extents2 = trw._gate(held, int(np.argmax(speed)) + 1)
    hit = trw._plain_reference_of(s, p, tracks2, extents2, p.plan_wait)
    assert hit["first"][p.node_seq[-1]] >= 0
    want = [t.avoid_rects(tracks2, extents2, 0, False, 7) for t in twins]
    again = sum(len(a) for a in asked)
    for a in asked:
        del a[:]
    assert again >= 1 and want[0]["plan_first"] is not None
    assert lqrrt.avoids_rects(planners, tracks2, extents2, 0, False, 7) == want
    assert counted.take() == [("tree_clear_rects_wait_multi", 3), ("tree_clear_rects_multi", again)]
    _same_plans(planners, twins)
    # tracks per planner: each its own table (the second one far away from everything), one launch all the same
    far = np.zeros((5, 2, 3))
    far[:, :, :2] = 900.0
    per_t, per_e = [tracks, far, tracks[:, :, :]], [extents, np.array([[0.5, 0.25], [0.3, 0.3]]), extents]
    want = [t.avoid_rects(per_t[k], per_e[k], 2, True, 7) for k, t in enumerate(twins)]
    assert lqrrt.avoids_rects(planners, per_t, per_e, start=2, adopt=True, max_wait=7) == want
    assert 1 <= len(counted.take()) <= 2
    _same_plans(planners, twins)
    # a planner whose goal has changed since its tree was grown: refused for everybody, as a ValueError, nobody touched
    planners[1].set_goal(np.asarray(planners[1].goal) + 1.0)
    snapshot = [_plan_of(q) for q in (planners[0], planners[2])]
    with pytest.raises(ValueError, match="avoids_rects: the goal changed"):
        lqrrt.avoids_rects(planners, tracks, extents)
    assert counted.take() == []
    for q, (seq, x, _, T, wait, _, _) in zip((planners[0], planners[2]), snapshot):
        assert list(q.node_seq) == seq and np.array_equal(np.asarray(q.x_seq), x) and q.T == T and q.plan_wait == wait
