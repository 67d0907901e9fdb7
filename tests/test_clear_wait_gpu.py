"""
The clearance query with departure delays on the device (csrc/clear_wait.hpp through lqrrt_tree_clear_wait, Engine.tree_clear_wait,
Planner.avoid(max_wait), deconflict(max_wait)) against the reference of the rule (tests/clear_wait_reference.py) and against the
device's own unchanged tree_clear.  Everything compared is an integer and must be EQUAL: the per-node masks, the counters, the
best plan.  Trees are put on the device with tree_load (hand-built ones, the committed fixtures); tests/test_clear_wait_cpu.py
shows with the reference alone that none of the inputs is degenerate.
"""
import numpy as np
import pytest

import clear_reference as cl
import clear_wait_reference as cw
import feasibility_reference as fr
import retain_reference as rr
from clear_common import WAVE, _grown, _load

pytestmark = pytest.mark.gpu


def _load_case(c):
    return _load(c.native(), c.tree, cl.H_HAND, goal=c.tree.goal, goal_buffer=c.tree.goal_buffer)


def _compare(eng, ref, tracks, radii, start, W):
    st, clear, dwell = eng.tree_clear_wait(tracks, radii, start, W, per_node=True)
    print(st)
    assert clear.dtype == np.uint64 and dwell.dtype == np.uint64
    np.testing.assert_array_equal(clear, ref["clear"])
    np.testing.assert_array_equal(dwell, ref["dwell_ok"])
    assert st == ref["stats"] and tuple(st) == cw.STAT_KEYS
    assert eng.tree_clear_wait(tracks, radii, start, W) == ref["stats"]           # the counters alone: the same call without the arrays
    return st, clear, dwell


@pytest.mark.parametrize("case", cw.cases(), ids=lambda c: c.name)
def test_hand_built_trees(case):
    c = case.case
    eng = _load_case(c)
    assert eng.size == c.tree.size
    _compare(eng, case.reference(), c.tracks, c.radii, c.start, case.W)
    eng.close()


@pytest.mark.parametrize("case", cl.cases(), ids=lambda c: c.name)
def test_one_delay_is_tree_clear(case):
    """W = 1 against the device's own plain query."""
    eng = _load_case(case)
    plain, first, dfirst = eng.tree_clear(case.tracks, case.radii, case.start, per_node=True)
    st, clear, dwell = eng.tree_clear_wait(case.tracks, case.radii, case.start, 1, per_node=True)
    np.testing.assert_array_equal(clear, (first == -1).astype(np.uint64))
    np.testing.assert_array_equal(dwell, (dfirst == -1).astype(np.uint64))
    none = plain["best_end"] < 0
    assert st == dict(size=plain["size"], hits=plain["hits"], clear_hits=plain["clear_hits"], clear_now=plain["clear_hits"],
                      best_end=plain["best_end"], best_wait=-1 if none else 0, best_steps=plain["best_steps"], best_arrival=plain["best_steps"])
    eng.close()


@pytest.mark.parametrize("name", ["car_2000", "boat_advanced_3000"])
def test_fixture_trees(name):
    """One call with W = 16 is 16 calls of the device's own tree_clear at start + w (joined with root_ok), and is the reference."""
    f = cl.fixture(name)
    s = f.native()
    eng = _load(s, f, f.H, dt=s.plan_kwargs["dt"])
    tracks, radii = f.tracks()
    W = cw.FIXTURE_W
    ref = cw.fixture_reference(name)
    st, clear, dwell = _compare(eng, ref, tracks, radii, 0, W)
    want_clear, want_dwell = np.zeros(len(clear), dtype=np.uint64), np.zeros(len(clear), dtype=np.uint64)
    root_ok, alive, hit = 0, True, None
    for w in range(W):
        _, first, dfirst = eng.tree_clear(tracks, radii, w, per_node=True)
        alive = alive and first[0] == -1                            # (node 0's root path is the root's row alone)
        root_ok |= int(alive) << w
        hit = dfirst != -2
        want_clear |= ((first == -1) & alive).astype(np.uint64) << np.uint64(w)
        want_dwell |= (dfirst == -1).astype(np.uint64) << np.uint64(w)
    np.testing.assert_array_equal(clear, want_clear)
    np.testing.assert_array_equal(dwell, want_dwell)
    assert root_ok == ref["root_ok"] == int(clear[0]) and st["hits"] == int(hit.sum())
    assert st["clear_hits"] > 0 and st["hits"] > st["clear_hits"]
    assert any(0 < int(m) < cw.all_mask(W) for m in clear)          # (of the inputs: the delays differ somewhere)
    eng.close()


# ------------------------------------------------------------------------------------------------ refusals

def test_refusals_on_the_device():
    import lqrrt_amd
    from lqrrt_amd import _native as nat
    from lqrrt_amd.engine import Engine
    c = cl.case("fork, the disc crosses the short branch")
    eng = _load_case(c)
    good = eng.tree_clear_wait(c.tracks, c.radii, 0, 8)
    fp = eng.footprint()
    for bad in (dict(tracks=np.zeros((0, 1, 2)), radii=0.5), dict(tracks=np.zeros((3, 0, 2)), radii=0.5),
                dict(tracks=c.tracks, radii=c.radii, start=-1), dict(tracks=np.full((3, 2, 2), np.nan), radii=0.5),
                dict(tracks=c.tracks, radii=-c.radii - 1.0), dict(tracks=c.tracks, radii=c.radii, waits=0),
                dict(tracks=c.tracks, radii=c.radii, waits=65), dict(tracks=c.tracks, radii=c.radii, waits=2.0),
                dict(tracks=c.tracks, radii=c.radii, start=2 ** 31 - 16, waits=1),        # start + the deepest cum (16) = 2^31
                dict(tracks=c.tracks, radii=c.radii, start=2 ** 31 - 17, waits=2),        # ... and the longest wait counts
                dict(tracks=c.tracks, radii=c.radii, start=2 ** 31 - 17 - 62, waits=64)):
        with pytest.raises(ValueError):
            eng.tree_clear_wait(**bad)
    assert eng.tree_clear_wait(c.tracks, c.radii, 2 ** 31 - 17, 1)["size"] == 11   # 2^31 - 1 still fits
    assert eng.tree_clear_wait(c.tracks, c.radii, 2 ** 31 - 17 - 63, 64)["size"] == 11
    # the ABI's own checks (the wrapper above refuses most of them first)
    st = nat.ClearWaitStats()
    tr, ra = np.ascontiguousarray(c.tracks), np.ascontiguousarray(c.radii)
    L, D = tr.shape[:2]
    nanpos = tr.copy()
    nanpos[-1, -1, 1] = np.inf
    negr = ra.copy()
    negr[-1] = -1e-300
    for args in ((tr, ra, 0, D, 0, 8), (tr, ra, L, 0, 0, 8), (tr, ra, L, D, -1, 8), (nanpos, ra, L, D, 0, 8), (tr, negr, L, D, 0, 8),
                 (tr, ra, L, D, 0, 0), (tr, ra, L, D, 0, 65), (tr, ra, L, D, 0, -1), (tr, ra, L, D, 2 ** 31 - 17, 2)):
        rc = nat.lib().lqrrt_tree_clear_wait(eng.h, nat.ptr(args[0]), nat.ptr(args[1]), args[2], args[3], args[4], args[5], st, None, None,
                                             eng._stream())
        assert rc == nat.E_ARG, args[2:]
    assert eng.tree_clear_wait(c.tracks, c.radii, 0, 8) == good and eng.footprint() == fp
    # no goal
    eng.set_resolution(0.1, 0.0, cl.H_HAND, np.ones(6), None, None)
    xe, ue = c.tree.packed()
    eng.tree_load(c.tree.state, c.tree.K, c.tree.pID, c.tree.elen, xe, ue)
    with pytest.raises(nat.NativeError) as ex:
        eng.tree_clear_wait(c.tracks, c.radii, 0, 8)
    assert ex.value.code == nat.E_STATE and "goal" in str(ex.value)
    eng.close()
    # models without a circle path
    for s in (lqrrt_amd.systems.DoublePendulum(), lqrrt_amd.systems.DoubleIntegrator(n_boxes=8, seed=1)):
        e2 = Engine(s, capacity=64, max_wave=64)
        e2.set_resolution(0.1, 0.0, 4, np.ones(s.nstates), s.goal, np.abs(np.asarray(s.goal_buffer, dtype=np.float64)))
        e2.tree_reset(s.x0)
        with pytest.raises(nat.NativeError) as ex:
            e2.tree_clear_wait(np.zeros((2, 1, 2)), 0.5, 0, 8)
        assert ex.value.code == nat.E_STATE and "circle" in str(ex.value)
        e2.close()


# ------------------------------------------------------------------------------------------------ nothing is modified

def test_the_tree_is_not_modified_and_grows_on_as_its_twin():
    s, eng = _grown()
    _, twin = _grown()
    before = rr.engine_arrays(eng)
    ign, best, fp, counters, mt = eng.ignored(), eng.plan_best(), eng.footprint(), eng.counters().as_dict(), eng.get_mt19937()
    states = eng.states()
    W, start = 12, 3
    # two discs that are far away except for four instants each, when they stand on a node's state: the instants that node has at
    # the delays 3 .. 6 (cum from the parents and edge lengths).  Whoever is there earlier or later passes: the delays differ.
    cum = np.zeros(len(states), dtype=np.int64)
    cum[0] = before[3][0]
    for i in range(1, len(states)):
        cum[i] = cum[before[2][i]] + before[3][i]
    picked = (len(states) // 3, len(states) // 2)
    L = start + int(max(cum[j] for j in picked)) + 40
    tracks = np.full((L, 2, 2), 900.0)
    for d, j in enumerate(picked):
        at = start + int(cum[j]) - 1
        tracks[at + 3:at + 7, d] = states[j, :2]
    st, clear, dwell = eng.tree_clear_wait(tracks, [2.0, 1.0], start, W, per_node=True)
    lo, hi = rr.goal_box(s)
    ref = cw.clear_wait_direct(before[0], before[2], before[3], before[4], cl.row_test_of(s), tracks, [2.0, 1.0], start, W, lo, hi)
    np.testing.assert_array_equal(clear, ref["clear"])
    np.testing.assert_array_equal(dwell, ref["dwell_ok"])
    assert st == ref["stats"] and any(0 < int(m) < cw.all_mask(W) for m in clear)
    after = rr.engine_arrays(eng)
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(eng.ignored(), ign)
    assert eng.plan_best() == best and eng.footprint() == fp and eng.counters().as_dict() == counters
    key, pos = eng.get_mt19937()
    assert pos == mt[1] and np.array_equal(key, mt[0])
    for e in (eng, twin):
        e.extend(WAVE, node_limit=900)
    assert eng.size == twin.size >= 900
    (sa, Ka, pa, la, xa, ua), (sb, Kb, pb, lb, xb, ub) = rr.engine_arrays(eng), rr.engine_arrays(twin)
    for a, b in ((sa, sb), (Ka, Kb), (pa, pb), (la, lb)):
        np.testing.assert_array_equal(a, b)
    live = np.arange(xa.shape[1])[None, :] < la[:, None]           # (pool rows beyond an edge's length are never written)
    np.testing.assert_array_equal(xa[live], xb[live])
    np.testing.assert_array_equal(ua[live], ub[live])
    np.testing.assert_array_equal(eng.ignored(), twin.ignored())
    assert eng.plan_best() == twin.plan_best()
    eng.close()
    twin.close()


# ------------------------------------------------------------------------------------------------ planner level

def _car_planner(seed, max_nodes, x0=(0.0, 0.0), goal=None, goal_buffer=None):
    """A car with the small hull; `goal` (x, y) and `goal_buffer` (one number for x and y) move and shrink the demo's goal box, and
    the sample space follows as the demo builds it."""
    import lqrrt_amd as lqrrt
    s = lqrrt.systems.Car(0)
    s.vps = fr.lattice_hull(1.0, 0.5, 0.25)
    s.set_obstacles(np.zeros((0, 3)))
    s.x0 = np.array([x0[0], x0[1], 0.0, 0.0, 0.0])
    if goal is not None:
        s.goal = [float(goal[0]), float(goal[1])] + [float(v) for v in s.goal[2:]]
        s.goal_buffer = [float(goal_buffer), float(goal_buffer)] + list(s.goal_buffer[2:])
        s.error_tol = np.copy(s.goal_buffer) / 2
        lo = np.minimum(s.x0[:2], s.goal[:2]) - 10.0
        hi = np.maximum(s.x0[:2], s.goal[:2]) + 10.0
        s.sample_space = [(lo[0], hi[0]), (lo[1], hi[1])] + list(s.sample_space[2:])
    cons = lqrrt.Constraints(s.nstates, s.ncontrols, s.goal_buffer, s.is_feasible)
    p = lqrrt.Planner(s.dynamics, s.lqr, cons, error_tol=s.error_tol, erf=s.erf, min_time=1.0, max_time=2.0, max_nodes=max_nodes,
                      goal0=s.goal, sys_time=lambda: 0.0, printing=False, wave_size=1024, **s.plan_kwargs)
    np.random.seed(seed)
    p.update_plan(s.x0, s.sample_space, goal_bias=s.goal_bias, xrand_gen=10)
    return s, p


def _tree_of(s, p):
    state, _, pID, elen, xedge, _ = rr.engine_arrays(p._engine)
    lo, hi = rr.goal_box(s)
    return state, pID, elen, xedge, lo, hi


def _reference_of(s, p, tracks, radii, start, W):
    state, pID, elen, xedge, lo, hi = _tree_of(s, p)
    table, radii, start = p._engine.track_table(tracks, radii, start)
    return cw.clear_wait_direct(state, pID, elen, xedge, cw.culled_test_of(s), table, radii, start, W, lo, hi)


def _gate(rows, c):
    """A disc of 1 cm that is far away except at instant c, when it stands on the bow point (0.5, 0) of the hull of the vehicle
    that follows `rows` on time.  The hull points lie on a 0.25 m lattice: who is there one row later, a few centimetres further
    back, has no hull point within the disc -- unless it moves less than 1 cm per row, or a multiple of 0.25 m."""
    tracks = np.full((len(rows) + 40, 1, 2), 900.0)
    tracks[c, 0] = rows[c, :2] + 0.5 * np.array([np.cos(rows[c, 2]), np.sin(rows[c, 2])])
    return tracks, np.array([0.01])


def test_avoid_waits_at_the_start():
    s, p = _car_planner(1, 700)
    assert p.plan_reached_goal and p.plan_wait == 0
    old_seq, old_x = list(p.node_seq), np.array(p.x_seq)
    # of the inputs, with the reference alone: a gate on the tree's shortest plan -- not always the one the planner holds, which is
    # the first it found -- that a wait of 1 .. 7 rows answers best
    state, pID, elen, xedge, _, _ = _tree_of(s, p)
    short = _reference_of(s, p, np.full((1, 1, 2), 900.0), 0.5, 0, 1)["stats"]["best_end"]
    rows = np.concatenate([xedge[v, :elen[v]] for v in p._engine.climb(short)])
    speed = np.linalg.norm(np.diff(rows[:, :2], axis=0), axis=1)
    for c in np.argsort(-speed)[:40:8]:                             # where the vehicle is fastest: it is out of the way in a row
        tracks, radii = _gate(rows, int(c))
        ref = _reference_of(s, p, tracks, radii, 0, 8)
        print(c, speed[c], ref["stats"])
        if ref["stats"]["best_wait"] >= 1:
            break
    want = ref["stats"]
    assert want["best_wait"] >= 1 and not int(ref["clear"][short]) & 1
    # max_wait = 0: the plain query, its dict, its adoption -- asked first without adopting
    plain = p.avoid(tracks, radii, adopt=False)
    assert set(plain) == set(cl.STAT_KEYS) | {"plan_first"} and {k: plain[k] for k in cl.STAT_KEYS} == p._engine.tree_clear(tracks, radii, 0)
    assert plain == p.avoid(tracks, radii, adopt=False, max_wait=0)
    assert list(p.node_seq) == old_seq and p.plan_wait == 0
    # adopt=False with waits: the answer, and nothing else
    out = p.avoid(tracks, radii, adopt=False, max_wait=7)
    assert {k: out[k] for k in cw.STAT_KEYS} == want and out["plan_first"] == plain["plan_first"] and set(out) == set(cw.STAT_KEYS) | {"plan_first"}
    assert list(p.node_seq) == old_seq and np.array_equal(np.array(p.x_seq), old_x) and p.plan_wait == 0
    # adopt
    out = p.avoid(tracks, radii, max_wait=7)
    best, wait = want["best_end"], want["best_wait"]
    assert {k: out[k] for k in cw.STAT_KEYS} == want
    assert p.node_seq == p._engine.climb(best) and p.plan_wait == wait and p.plan_reached_goal
    assert len(p.x_seq) == want["best_arrival"] == want["best_steps"] + wait == len(p.u_seq) == len(p.t_seq)
    X = np.asarray(p.x_seq, dtype=np.float64)
    for k in range(1, wait + 1):
        np.testing.assert_array_equal(X[k], X[0])
        np.testing.assert_array_equal(np.asarray(p.u_seq[k]), np.asarray(p.u_seq[0]))
    state, pID, elen, xedge, _, _ = _tree_of(s, p)
    np.testing.assert_array_equal(X[wait:], np.concatenate([xedge[v, :elen[v]] for v in p.node_seq]))
    np.testing.assert_array_equal(X[0], state[0])
    assert p.T == len(X) * p.dt and np.array_equal(p.t_seq, np.arange(len(X)) * p.dt)
    np.testing.assert_array_equal(p.get_state(0.5 * wait * p.dt), state[0])      # the root's state during the wait
    np.testing.assert_array_equal(p.get_state(p.T + 5.0), X[-1])
    assert p.plan_node_after(0.0)[2] == wait * p.dt                              # the root is "reached" when the wait is over
    # the adopted plan is clear row by row with the plain model, the wait at the start and at the goal included
    test = cl.row_test_of(s)
    c_, s_ = fr.portable_sincos(X[:, 2])
    discs = np.concatenate((tracks, np.broadcast_to(radii[None, :, None], tracks.shape[:2] + (1,))), axis=2)
    assert test(X, c_, s_, discs[np.minimum(np.arange(len(X)), len(discs) - 1)]).all()
    rest = np.arange(len(X), len(discs))
    assert test(np.repeat(X[-1:], len(rest), axis=0), np.repeat(c_[-1], len(rest)), np.repeat(s_[-1], len(rest)), discs[rest]).all()
    # ... and so says the next call, which leaves it alone
    again = p.avoid(tracks, radii, max_wait=7)
    assert again["plan_first"] is None and (again["best_end"], again["best_wait"]) == (best, wait) and p.plan_wait == wait
    # any other call that sets a plan drops the wait
    p.avoid(np.full((2, 1, 2), 900.0), 0.5)
    assert p.plan_wait == 0 and len(p.x_seq) == len(np.concatenate([xedge[v, :elen[v]] for v in p.node_seq]))


def test_deconflict_passes_the_wait_on():
    """Two cars: the first drives through the second one's goal box and is given a radius that covers the box while it is there.
    Without waits the second has no clear plan -- whenever it arrives, the first is still there or comes later; leaving up to 8
    rows late, its latest arrival finds the box free.  `start` places the first one's passage in time so; both halves are shown
    with the reference before the device is asked."""
    import lqrrt_amd as lqrrt
    sa, a = _car_planner(2, 700)
    A = np.asarray(a.x_seq, dtype=np.float64)
    m = (6 * len(A)) // 10
    n = np.array([-np.sin(A[m, 2]), np.cos(A[m, 2])])               # at right angles to the first one's heading there
    sb, b = _car_planner(3, 700, x0=tuple(A[m, :2] + 22.0 * n), goal=A[m, :2], goal_buffer=3.0)
    assert a.plan_reached_goal and b.plan_reached_goal and a.dt == b.dt
    radii = np.array([10.0, 0.5])
    # when does the first one stop touching a vehicle parked at each of the second one's goal hits?  d_i = that row - cum[i]
    state, pID, elen, xedge, lo, hi = _tree_of(sb, b)
    probe = cw.clear_wait_direct(state, pID, elen, xedge, cl.row_test_of(sb), A[:, None, :2], radii[:1], 0, 1, lo, hi)
    test = cl.row_test_of(sb)
    discs = np.concatenate((A[:, None, :2], np.full((len(A), 1, 1), radii[0])), axis=2)
    ds = []
    for i in np.flatnonzero(probe["hit"]):
        x = np.repeat(xedge[i, elen[i] - 1][None, :], len(A), axis=0)
        c_, s_ = fr.portable_sincos(x[:, 2])
        bad = np.flatnonzero(~test(x, c_, s_, discs))
        assert len(bad) and bad[-1] < len(A) - 1                    # the first one covers every hit for a while and parks clear of it
        ds.append(int(bad[-1]) - int(probe["cum"][i]))
    # with start0 the hit that is free first is free one row after it arrives -- but the second car also has to get there past
    # the first: the reference says which delay is the first clear one at start0, and moving `start` on by one row moves every
    # delay back by one (only the first one's track is shifted against the second one's tree)
    tracks = [A[:, :2]]
    for start0 in range(max(min(ds), 0), max(min(ds), 0) + 640, 64):
        r64 = _reference_of(sb, b, tracks, radii[:1], start0, 64)
        if r64["stats"]["best_end"] >= 0:
            break
    assert r64["root_ok"] == cw.all_mask(64) and r64["stats"]["best_end"] >= 0
    first_clear = min((int(m) & -int(m)).bit_length() - 1 for m in (r64["clear"] & r64["dwell_ok"]) if int(m))
    start = start0 + first_clear - 1
    assert start >= 0, "the first car passes too early for this test"
    ref0, ref8 = _reference_of(sb, b, tracks, radii[:1], start, 1), _reference_of(sb, b, tracks, radii[:1], start, 9)
    print(start, ref0["stats"], ref8["stats"])
    assert ref0["stats"]["best_end"] == -1 and ref0["stats"]["hits"] > 0 and ref8["stats"]["best_wait"] >= 1       # both halves, on the CPU
    old = list(b.node_seq)
    got = lqrrt.deconflict([a, b], radii, start=start)
    assert got[0] is None and got[1]["best_end"] == -1 and got[1]["clear_hits"] == 0 and list(b.node_seq) == old and b.plan_wait == 0
    got = lqrrt.deconflict([a, b], radii, start=start, max_wait=8)
    assert got[0] is None and {k: got[1][k] for k in cw.STAT_KEYS} == ref8["stats"]
    assert b.node_seq[-1] == ref8["stats"]["best_end"] and b.plan_wait == ref8["stats"]["best_wait"] == got[1]["best_wait"]
    assert len(b.x_seq) == ref8["stats"]["best_arrival"]
    # a third planner after it sees the wait rows of the second in its track
    np.testing.assert_array_equal(np.asarray(b.x_seq)[:b.plan_wait + 1], np.repeat(np.asarray(b.x_seq)[:1], b.plan_wait + 1, axis=0))
