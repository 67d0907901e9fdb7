"""
The clearance queries for several trees per launch on the device (csrc/clear_multi.hpp through lqrrt_tree_clear_multi /
lqrrt_tree_clear_wait_multi, Engine.tree_clear_multi / tree_clear_wait_multi, lqrrt_amd.avoids, deconflict(batched=True)).  Every
member's answer must EQUAL that of the one-tree call on its engine -- counters and per-node arrays are integers and masks -- and,
for the hand-built trees, the reference of the rule (tests/clear_reference.py, tests/clear_wait_reference.py).
"""
import ctypes as C

import numpy as np
import pytest

import clear_reference as cl
import clear_wait_reference as cw
import retain_reference as rr
from clear_common import WAVE, _grown, _load

pytestmark = pytest.mark.gpu


def _load_case(c):
    return _load(c.native(), c.tree, cl.H_HAND, goal=c.tree.goal, goal_buffer=c.tree.goal_buffer)


def _by_model(cases, system_of):
    groups = {}
    for c in cases:
        groups.setdefault(system_of(c), []).append(c)
    return groups


def _same(got, want):
    assert got[0] == want[0]
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[2], want[2])
    assert got[1].dtype == want[1].dtype and got[2].dtype == want[2].dtype


# ------------------------------------------------------------------------------------------------ 1. every hand-built case at once

def test_every_hand_built_case_in_one_call():
    from lqrrt_amd.engine import Engine
    groups = _by_model(cl.cases(), lambda c: c.tree.system)
    assert len(groups["boat_advanced"]) > 16 and {c.tree.size for c in groups["boat_advanced"]} >= {1, 11, 33, 256}
    for system, cases in sorted(groups.items()):
        engines = [_load_case(c) for c in cases]
        solo = [e.tree_clear(c.tracks, c.radii, c.start, per_node=True) for e, c in zip(engines, cases)]
        for order in (list(range(len(cases))), list(range(len(cases)))[::-1]):
            pick = lambda seq: [seq[k] for k in order]
            got = Engine.tree_clear_multi(pick(engines), [c.tracks for c in pick(cases)], [c.radii for c in pick(cases)],
                                          [c.start for c in pick(cases)], per_node=True)
            for k, g in zip(order, got):
                ref = cases[k].reference()
                _same(g, solo[k])
                _same(g, (ref["stats"], ref["first"], ref["dwell_first"]))
            counters = Engine.tree_clear_multi(pick(engines), [c.tracks for c in pick(cases)], [c.radii for c in pick(cases)],
                                               [c.start for c in pick(cases)])
            assert counters == [solo[k][0] for k in order]                        # the counters alone: the same call without the arrays
        for e in engines:
            e.close()


def test_every_hand_built_wait_case_in_one_call():
    from lqrrt_amd.engine import Engine
    one = cw.WaitCase(cl.case("fork, the disc crosses the short branch"), 1)      # W = 1 next to W = 8, 63 and 64
    groups = _by_model(list(cw.cases()) + [one], lambda c: c.case.tree.system)
    assert len(groups["boat_advanced"]) > 32 and {c.W for c in groups["boat_advanced"]} >= {1, 8, 63, 64}      # (two chunks)
    for system, cases in sorted(groups.items()):
        engines = [_load_case(c.case) for c in cases]
        solo = [e.tree_clear_wait(c.case.tracks, c.case.radii, c.case.start, c.W, per_node=True) for e, c in zip(engines, cases)]
        for order in (list(range(len(cases))), list(range(len(cases)))[::-1]):
            pick = lambda seq: [seq[k] for k in order]
            got = Engine.tree_clear_wait_multi(pick(engines), [c.case.tracks for c in pick(cases)], [c.case.radii for c in pick(cases)],
                                               [c.case.start for c in pick(cases)], [c.W for c in pick(cases)], per_node=True)
            for k, g in zip(order, got):
                ref = cases[k].reference()
                _same(g, solo[k])
                _same(g, (ref["stats"], ref["clear"], ref["dwell_ok"]))
        for e in engines:
            e.close()


# ------------------------------------------------------------------------------------------------ 2. chunk edges

@pytest.mark.parametrize("n", [1, 32, 33])
def test_chunk_edges(n):
    """n fork trees, every member with a start of its own: a member that read another's descriptor would answer for that start."""
    from lqrrt_amd.engine import Engine
    c = cl.case("fork, the disc crosses the short branch")
    engines = [_load_case(c) for _ in range(n)]
    starts = [(5 * k) % 23 for k in range(n)]
    assert len(set(starts[:23])) == min(n, 23) and (n < 33 or starts[31] != starts[32])
    solo = [e.tree_clear(c.tracks, c.radii, s, per_node=True) for e, s in zip(engines, starts)]
    assert n == 1 or len({tuple(s[1].tolist()) for s in solo}) > 2                 # (of the inputs: the starts do change the answer)
    got = Engine.tree_clear_multi(engines, [c.tracks] * n, [c.radii] * n, starts, per_node=True)
    for g, s in zip(got, solo):
        _same(g, s)
    waits = [1 + (3 * k) % 9 for k in range(n)]
    solo = [e.tree_clear_wait(c.tracks, c.radii, s, w, per_node=True) for e, s, w in zip(engines, starts, waits)]
    got = Engine.tree_clear_wait_multi(engines, [c.tracks] * n, [c.radii] * n, starts, waits, per_node=True)
    for g, s in zip(got, solo):
        _same(g, s)
    for e in engines:
        e.close()


# ------------------------------------------------------------------------------------------------ 3. the largest hull wins the LDS

@pytest.mark.parametrize("big_first", [True, False])
def test_the_largest_hull_sizes_the_lds(big_first):
    from lqrrt_amd.engine import Engine
    big = cl.case("ros_boat on an occupied grid, 3073 hull points")
    small = cl._fork_case("ros_boat: the fork, lattice hull", system="ros_boat")
    assert big.vps().shape[1] == 3073 and small.vps().shape[1] < 64
    cases = [big, small] if big_first else [small, big]
    engines = [_load_case(c) for c in cases]
    got = Engine.tree_clear_multi(engines, [c.tracks for c in cases], [c.radii for c in cases], [c.start for c in cases], per_node=True)
    gotw = Engine.tree_clear_wait_multi(engines, [c.tracks for c in cases], [c.radii for c in cases], [c.start for c in cases], 8, per_node=True)
    for e, c, g, gw in zip(engines, cases, got, gotw):
        ref = c.reference()
        _same(g, (ref["stats"], ref["first"], ref["dwell_first"]))
        _same(g, e.tree_clear(c.tracks, c.radii, c.start, per_node=True))
        _same(gw, e.tree_clear_wait(c.tracks, c.radii, c.start, 8, per_node=True))
    for e in engines:
        e.close()


# ------------------------------------------------------------------------------------------------ 4. a shared table

def test_members_that_share_a_table():
    from lqrrt_amd.engine import Engine
    c = cl.case("fork, the disc crosses the short branch")
    other = c.tracks.copy()
    other[7, -1] = (7.0, 40.0)                                      # the crossing disc is elsewhere at the instant it met the short branch
    engines = [_load_case(c) for _ in range(5)]
    tables, radii = [c.tracks] * 4 + [other], [c.radii] * 4 + [c.radii.copy()]
    starts = [0, 4, 0, 1, 0]
    solo = [e.tree_clear(t, r, s, per_node=True) for e, t, r, s in zip(engines, tables, radii, starts)]
    assert solo[0][0] != solo[4][0] and solo[0][0] != solo[1][0]                   # (of the inputs: the changed row and the start matter)
    for g, s in zip(Engine.tree_clear_multi(engines, tables, radii, starts, per_node=True), solo):
        _same(g, s)
    # the copy in the middle: the members on both sides of it still share
    mid = [tables[0], tables[0], other, tables[0], tables[0]]
    solo = [e.tree_clear_wait(t, c.radii, s, 8, per_node=True) for e, t, s in zip(engines, mid, starts)]
    for g, s in zip(Engine.tree_clear_wait_multi(engines, mid, [c.radii] * 5, starts, 8, per_node=True), solo):
        _same(g, s)
    for e in engines:
        e.close()


# ------------------------------------------------------------------------------------------------ 5. refusals

def _raw(call, stats, dtype, engines, tracks, radii, L, D, start, waits=None):
    """The ABI call itself, with output arrays that hold sentinels; returns (rc, stats array, per-node arrays)."""
    from lqrrt_amd import _native as nat
    n = len(engines)
    handles = (C.c_void_p * max(n, 1))(*[e.h for e in engines])
    tp = (C.c_void_p * max(n, 1))(*[None if t is None else t.ctypes.data for t in tracks])
    rp = (C.c_void_p * max(n, 1))(*[r.ctypes.data for r in radii])
    out = (stats * max(n, 1))()
    C.memset(out, 0x5a, C.sizeof(out))
    a = [np.full(max(e.size, 1), 77, dtype=dtype) for e in engines]
    b = [np.full(max(e.size, 1), 77, dtype=dtype) for e in engines]
    ap = (C.c_void_p * max(n, 1))(*[x.ctypes.data for x in a])
    bp = (C.c_void_p * max(n, 1))(*[x.ctypes.data for x in b])
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)
    L, D, start = i32(L), i32(D), i32(start)
    extra = () if waits is None else (nat.ptr(i32(waits)),)
    rc = getattr(nat.lib(), call)(handles, n, tp, rp, nat.ptr(L), nat.ptr(D), nat.ptr(start), *extra, out, ap, bp,
                                  engines[0]._stream() if engines else None)
    return rc, bytes(out), a, b


def test_refusals_on_the_device():
    import lqrrt_amd
    from lqrrt_amd import _native as nat
    from lqrrt_amd.engine import Engine
    c = cl.case("fork, the disc crosses the short branch")
    engines = [_load_case(c) for _ in range(3)]
    tr, ra = np.ascontiguousarray(c.tracks), np.ascontiguousarray(c.radii)
    L, D = tr.shape[:2]
    good = Engine.tree_clear_multi(engines, [tr] * 3, [ra] * 3, [0, 1, 2], per_node=True)
    goodw = Engine.tree_clear_wait_multi(engines, [tr] * 3, [ra] * 3, [0, 1, 2], [8, 1, 64], per_node=True)
    fps = [e.footprint() for e in engines]
    nanpos = tr.copy()
    nanpos[-1, -1, 1] = np.nan
    negr = ra.copy()
    negr[-1] = -1e-300

    def refused(rc, raw, code, who, what=None):
        msg = (nat.lib().lqrrt_last_error() or b"").decode()
        assert rc == code, (rc, msg)
        if who is not None:
            assert "(engine %d)" % who in msg, msg
        if what:
            assert what in msg, msg
        _, out, a, b = raw
        assert set(out) == {0x5a} and all((x == 77).all() for x in a + b)            # nothing was written into any output

    # any one member's bad argument refuses the whole call and names the engine
    for who in (0, 2):
        def member(good_value, bad_value):
            return [bad_value if k == who else good_value for k in range(3)]
        for kw in (dict(L=member(L, 0)), dict(D=member(D, 0)), dict(start=member(0, -1)), dict(tracks=member(tr, nanpos)),
                   dict(radii=member(ra, negr)), dict(start=member(0, 2 ** 31 - 16)), dict(tracks=member(tr, None))):
            args = dict(tracks=[tr] * 3, radii=[ra] * 3, L=[L] * 3, D=[D] * 3, start=[0] * 3)
            args.update(kw)
            raw = _raw("lqrrt_tree_clear_multi", nat.ClearStats, np.int32, engines, **args)
            refused(raw[0], raw, nat.E_ARG, who)
            raw = _raw("lqrrt_tree_clear_wait_multi", nat.ClearWaitStats, np.uint64, engines, waits=[8] * 3, **args)
            refused(raw[0], raw, nat.E_ARG, who)
        for w in (0, 65):
            raw = _raw("lqrrt_tree_clear_wait_multi", nat.ClearWaitStats, np.uint64, engines, [tr] * 3, [ra] * 3, [L] * 3, [D] * 3, [0] * 3,
                       waits=member(8, w))
            refused(raw[0], raw, nat.E_ARG, who, "waits")
        # start + the longest wait + the deepest cum (16) = 2^31
        raw = _raw("lqrrt_tree_clear_wait_multi", nat.ClearWaitStats, np.uint64, engines, [tr] * 3, [ra] * 3, [L] * 3, [D] * 3,
                   member(0, 2 ** 31 - 17 - 6), waits=member(1, 8))
        refused(raw[0], raw, nat.E_ARG, who, "31 bits")
    # the engine list: an engine twice, n = 0, n = 129
    raw = _raw("lqrrt_tree_clear_multi", nat.ClearStats, np.int32, [engines[0], engines[1], engines[0]], [tr] * 3, [ra] * 3, [L] * 3, [D] * 3, [0] * 3)
    refused(raw[0], raw, nat.E_ARG, None, "twice")
    st = (nat.ClearStats * 1)()
    assert nat.lib().lqrrt_tree_clear_multi((C.c_void_p * 1)(engines[0].h), 0, None, None, None, None, None, st, None, None, None) == nat.E_ARG
    many = (C.c_void_p * 129)(*[engines[k % 3].h for k in range(129)])
    ptrs = (C.c_void_p * 129)(*[tr.ctypes.data] * 129)
    rptrs = (C.c_void_p * 129)(*[ra.ctypes.data] * 129)
    ints = np.zeros(129, dtype=np.int32)
    st129 = (nat.ClearStats * 129)()
    assert nat.lib().lqrrt_tree_clear_multi(many, 129, ptrs, rptrs, nat.ptr(ints), nat.ptr(ints), nat.ptr(ints), st129, None, None, None) == nat.E_ARG
    with pytest.raises(ValueError, match="twice"):
        Engine.tree_clear_multi([engines[0], engines[0]], [tr] * 2, [ra] * 2, [0, 0])
    with pytest.raises(ValueError, match=r"\(engine 1\)"):
        Engine.tree_clear_wait_multi(engines, [tr] * 3, [ra] * 3, [0, 2 ** 31 - 16, 0], 1)
    # after all that the same engines answer as before, and no footprint has moved
    for g, w in zip(Engine.tree_clear_multi(engines, [tr] * 3, [ra] * 3, [0, 1, 2], per_node=True), good):
        _same(g, w)
    for g, w in zip(Engine.tree_clear_wait_multi(engines, [tr] * 3, [ra] * 3, [0, 1, 2], [8, 1, 64], per_node=True), goodw):
        _same(g, w)
    assert [e.footprint() for e in engines] == fps

    # two models in one call
    car = cl.case("car: the fork")
    ecar = _load_case(car)
    with pytest.raises(ValueError, match="share the device and the model"):
        Engine.tree_clear_multi([engines[0], ecar], [tr, car.tracks], [ra, car.radii], [0, 0])
    ecar.close()
    # a member without a goal, and one with an empty tree (no resolution yet): named, E_STATE
    engines[1].set_resolution(0.1, 0.0, cl.H_HAND, np.ones(6), None, None)
    xe, ue = c.tree.packed()
    engines[1].tree_load(c.tree.state, c.tree.K, c.tree.pID, c.tree.elen, xe, ue)
    for call, extra in ((Engine.tree_clear_multi, ()), (Engine.tree_clear_wait_multi, (8,))):
        with pytest.raises(nat.NativeError) as ex:
            call(engines, [tr] * 3, [ra] * 3, [0, 0, 0], *extra)
        assert ex.value.code == nat.E_STATE and "goal" in str(ex.value) and "(engine 1)" in str(ex.value)
    empty = Engine(c.native(), capacity=64, max_wave=64)
    with pytest.raises(nat.NativeError) as ex:
        Engine.tree_clear_multi([engines[0], engines[2], empty], [tr] * 3, [ra] * 3, [0, 0, 0])
    assert ex.value.code == nat.E_STATE and "no tree" in str(ex.value) and "(engine 2)" in str(ex.value)
    empty.close()
    # a hull beyond a workgroup's LDS, as the second member
    big = lqrrt_amd.systems.BoatAdvanced(0)
    big.vps = np.random.RandomState(0).uniform(-1, 1, (2, 20000))
    big.set_obstacles(np.zeros((0, 3)))
    big.goal, big.goal_buffer = [float(v) for v in c.tree.goal], [float(v) for v in c.tree.goal_buffer]
    e3 = _load(big, c.tree, cl.H_HAND, goal=c.tree.goal, goal_buffer=c.tree.goal_buffer)
    for call, extra in ((Engine.tree_clear_multi, ()), (Engine.tree_clear_wait_multi, (8,))):
        with pytest.raises(ValueError, match="LDS") as ex:
            call([engines[0], e3], [tr] * 2, [ra] * 2, [0, 0], *extra)
        assert "(engine 1)" in str(ex.value)
    e3.close()
    for e in engines:
        e.close()
    # models without a circle path, and the generic engine
    s = lqrrt_amd.systems.DoubleIntegrator(n_boxes=8, seed=1)
    e2 = Engine(s, capacity=64, max_wave=64)
    e2.set_resolution(0.1, 0.0, 4, np.ones(s.nstates), s.goal, np.abs(np.asarray(s.goal_buffer, dtype=np.float64)))
    e2.tree_reset(s.x0)
    with pytest.raises(nat.NativeError) as ex:
        Engine.tree_clear_multi([e2], [np.zeros((2, 1, 2))], [0.5], [0])
    assert ex.value.code == nat.E_STATE and "circle" in str(ex.value) and "(engine 0)" in str(ex.value)
    e2.close()


def test_a_generic_engine_is_refused():
    from lqrrt_amd import _native as nat
    from lqrrt_amd.engine import NodeTable
    table = NodeTable(4, 1, (2,), capacity=128)
    tr, ra, one, zero = np.zeros((2, 1, 2)), np.array([0.5]), np.array([1], dtype=np.int32), np.array([0], dtype=np.int32)
    two = np.array([2], dtype=np.int32)
    for call, stats, extra in (("lqrrt_tree_clear_multi", nat.ClearStats, ()), ("lqrrt_tree_clear_wait_multi", nat.ClearWaitStats, (nat.ptr(one),))):
        out = (stats * 1)()
        C.memset(out, 0x5a, C.sizeof(out))
        rc = getattr(nat.lib(), call)((C.c_void_p * 1)(table.h), 1, (C.c_void_p * 1)(tr.ctypes.data), (C.c_void_p * 1)(ra.ctypes.data),
                                      nat.ptr(two), nat.ptr(one), nat.ptr(zero), *extra, out, None, None, None)
        assert rc == nat.E_STATE and "GENERIC" in nat.lib().lqrrt_last_error().decode()
        assert set(bytes(out)) == {0x5a}
    table.close()


# ------------------------------------------------------------------------------------------------ 6. nothing is modified

def test_nothing_of_any_tree_is_modified_and_the_trees_grow_on_as_their_twins():
    from lqrrt_amd.engine import Engine
    made = [_grown(1), _grown(2)]
    s, engines = made[0][0], [m[1] for m in made]
    twins = [_grown(1)[1], _grown(2)[1]]
    before = [rr.engine_arrays(e) for e in engines]
    kept = [(e.ignored(), e.plan_best(), e.footprint(), e.counters().as_dict(), e.get_mt19937()) for e in engines]
    L = 300
    tables, radii = [], [np.array([2.0, 1.0]), np.array([1.5, 0.8])]
    for e in engines:
        states = e.states()
        tr = np.zeros((L, 2, 2))
        tr[:, 0] = states[len(states) // 2, :2]
        tr[:, 1, 0] = states[len(states) // 3, 0]
        tr[:, 1, 1] = states[len(states) // 3, 1] + 0.2 * (np.arange(L) - 40)
        tables.append(tr)
    lo, hi = rr.goal_box(s)
    got = Engine.tree_clear_multi(engines, tables, radii, [3, 0], per_node=True)
    gotw = Engine.tree_clear_wait_multi(engines, tables, radii, [3, 0], [16, 5], per_node=True)
    for k, (e, start, W) in enumerate(zip(engines, (3, 0), (16, 5))):
        ref = cl.clear(before[k][0], before[k][2], before[k][3], before[k][4], cl.row_test_of(s), tables[k], radii[k], start, lo, hi)
        _same(got[k], (ref["stats"], ref["first"], ref["dwell_first"]))
        assert got[k][0]["conflicts"] > 0 and got[k][0]["blocked"] > 0
        _same(got[k], e.tree_clear(tables[k], radii[k], start, per_node=True))
        _same(gotw[k], e.tree_clear_wait(tables[k], radii[k], start, W, per_node=True))
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
    for e in engines + twins:
        e.close()


# ------------------------------------------------------------------------------------------------ 7. and 8. planner level

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


def test_avoids_is_the_loop_of_avoid():
    import lqrrt_amd as lqrrt
    import test_clear_wait_gpu as tcw
    seeds = (1, 2, 3)
    made, twins = [tcw._car_planner(seed, 700) for seed in seeds], [tcw._car_planner(seed, 700)[1] for seed in seeds]
    planners = [m[1] for m in made]
    _same_plans(planners, twins)
    # of the inputs, with the reference alone (as test_avoid_waits_at_the_start): a gate on the shortest plan of the first planner's
    # tree that a wait of 1 .. 7 rows answers best
    s, p = made[0]
    state, pID, elen, xedge, _, _ = tcw._tree_of(s, p)
    short = tcw._reference_of(s, p, np.full((1, 1, 2), 900.0), 0.5, 0, 1)["stats"]["best_end"]
    rows = np.concatenate([xedge[v, :elen[v]] for v in p._engine.climb(short)])
    speed = np.linalg.norm(np.diff(rows[:, :2], axis=0), axis=1)
    for c in np.argsort(-speed)[:40:8]:
        tracks, radii = tcw._gate(rows, int(c))
        ref = tcw._reference_of(s, p, tracks, radii, 0, 8)
        if ref["stats"]["best_wait"] >= 1:
            break
    assert ref["stats"]["best_wait"] >= 1 and not int(ref["clear"][short]) & 1
    changed = False
    for max_wait, adopt in ((0, False), (7, False), (7, True), (0, True)):
        want = [t.avoid(tracks, radii, 0, adopt, max_wait) for t in twins]
        got = lqrrt.avoids(planners, tracks, radii, 0, adopt, max_wait)
        print(max_wait, adopt, got)
        assert got == want
        _same_plans(planners, twins)
        if max_wait == 7 and not changed:
            assert {k: got[0][k] for k in cw.STAT_KEYS} == ref["stats"]
        changed = changed or adopt
    assert any(g["best_end"] >= 0 for g in got)
    # tracks per planner: each its own table (the second one far away from everything), one launch all the same
    far = np.full((5, 2, 2), 900.0)
    per_t, per_r = [tracks, far, tracks[:, :, :]], [radii, np.array([0.5, 0.25]), radii]
    want = [t.avoid(per_t[k], per_r[k], 2, True, 7) for k, t in enumerate(twins)]
    assert lqrrt.avoids(planners, per_t, per_r, start=2, adopt=True, max_wait=7) == want
    _same_plans(planners, twins)
    # a planner whose goal has changed since its tree was grown: refused for everybody, as a ValueError, nobody touched
    planners[1].set_goal(np.asarray(planners[1].goal) + 1.0)
    snapshot = [_plan_of(q) for q in (planners[0], planners[2])]
    with pytest.raises(ValueError, match="avoids: the goal changed"):
        lqrrt.avoids(planners, tracks, radii)
    for q, (seq, x, _, T, wait, _, _) in zip((planners[0], planners[2]), snapshot):
        assert list(q.node_seq) == seq and np.array_equal(np.asarray(q.x_seq), x) and q.T == T and q.plan_wait == wait


def test_batched_deconflict_is_deconflict():
    import lqrrt_amd as lqrrt
    import test_clear_gpu as tcg
    from lqrrt_amd import planner as planner_mod
    spec = ((2, (0.0, 0.0)), (3, (0.0, 30.0)), (4, (30.0, 0.0)))
    planners = [tcg._car_planner(seed, 700, small_hull=True, x0=x0)[1] for seed, x0 in spec]
    twins = [tcg._car_planner(seed, 700, small_hull=True, x0=x0)[1] for seed, x0 in spec]
    order, radii = [1, 2, 0], np.array([0.8, 0.6, 0.7])
    entry = [list(p.node_seq) for p in planners]
    want = lqrrt.deconflict(twins, radii, order=order)
    got = lqrrt.deconflict(planners, radii, order=order, batched=True)
    print(want)
    assert got == want and got[1] is None
    assert any(w["best_end"] >= 0 for w in (want[2], want[0])) and any(w["conflicts"] > 0 for w in (want[2], want[0]))      # (of the inputs)
    assert any(list(p.node_seq) != e for p, e in zip(planners, entry))            # ... and a plan did change
    _same_plans(planners, twins)
    # once more on the plans as they now stand, with waits: the counts of rounds and native calls come with it
    want = lqrrt.deconflict(twins, radii, order=order, max_wait=5)
    got, rounds, calls = planner_mod._deconflict_batched(planners, np.broadcast_to(radii, (3,)), order, 0, 5)
    assert got == want and 1 <= rounds <= 2 and rounds <= calls <= 2 * rounds
    _same_plans(planners, twins)


@pytest.mark.parametrize("max_wait", [0, 8])
def test_batched_deconflict_passes_the_wait_on(max_wait):
    """The two cars of test_deconflict_passes_the_wait_on: without waits the second has no clear plan and keeps the one it came
    with; leaving up to 8 rows late it finds one."""
    import lqrrt_amd as lqrrt
    import test_clear_wait_gpu as tcw
    import feasibility_reference as fr

    def pair():
        sa, a = tcw._car_planner(2, 700)
        A = np.asarray(a.x_seq, dtype=np.float64)
        m = (6 * len(A)) // 10
        n = np.array([-np.sin(A[m, 2]), np.cos(A[m, 2])])
        sb, b = tcw._car_planner(3, 700, x0=tuple(A[m, :2] + 22.0 * n), goal=A[m, :2], goal_buffer=3.0)
        return (sa, a), (sb, b), A
    (sa, a), (sb, b), A = pair()
    (_, a2), (_, b2), _ = pair()
    radii = np.array([10.0, 0.5])
    # `start` as that test places it: the first car's passage through the second one's goal box, from the reference
    state, pID, elen, xedge, lo, hi = tcw._tree_of(sb, b)
    probe = cw.clear_wait_direct(state, pID, elen, xedge, cl.row_test_of(sb), A[:, None, :2], radii[:1], 0, 1, lo, hi)
    test = cl.row_test_of(sb)
    discs = np.concatenate((A[:, None, :2], np.full((len(A), 1, 1), radii[0])), axis=2)
    ds = []
    for i in np.flatnonzero(probe["hit"]):
        x = np.repeat(xedge[i, elen[i] - 1][None, :], len(A), axis=0)
        c_, s_ = fr.portable_sincos(x[:, 2])
        bad = np.flatnonzero(~test(x, c_, s_, discs))
        ds.append(int(bad[-1]) - int(probe["cum"][i]))
    for start0 in range(max(min(ds), 0), max(min(ds), 0) + 640, 64):
        r64 = tcw._reference_of(sb, b, [A[:, :2]], radii[:1], start0, 64)
        if r64["stats"]["best_end"] >= 0:
            break
    first_clear = min((int(m) & -int(m)).bit_length() - 1 for m in (r64["clear"] & r64["dwell_ok"]) if int(m))
    start = start0 + first_clear - 1
    assert start >= 0
    want = lqrrt.deconflict([a2, b2], radii, start=start, max_wait=max_wait)
    got = lqrrt.deconflict([a, b], radii, start=start, max_wait=max_wait, batched=True)
    print(start, want)
    assert got == want and got[0] is None
    assert (want[1]["best_end"] == -1) == (max_wait == 0) and (max_wait == 0 or want[1]["best_wait"] >= 1)       # (of the inputs)
    _same_plans([a, b], [a2, b2])
