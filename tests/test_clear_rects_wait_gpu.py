"""
The clearance query against moving oriented rectangles with departure delays on the device (csrc/clear_rects_wait.hpp through
lqrrt_tree_clear_rects_wait, Engine.tree_clear_rects_wait, Planner.avoid_rects(max_wait)) against the reference of the rule
(tests/clear_rects_wait_reference.py) and against the device's own unchanged tree_clear_rects.  Everything compared is an integer
and must be EQUAL: both masks per node, every counter, the best plan.  Trees are put on the device with tree_load (hand-built ones
of at most 257 nodes, the two committed fixtures); tests/test_clear_rects_wait_cpu.py shows with the reference alone that none of
the inputs is degenerate.
"""
import importlib.util
import os
import re

import numpy as np
import pytest

import clear_reference as cl
import clear_rects_reference as cr
import clear_rects_wait_reference as rw
import feasibility_reference as fr
import retain_reference as rr
from clear_common import WAVE, _grown, _load

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _engine(case):
    return _load(case.native(), case.tree, cl.H_HAND, goal=case.tree.goal, goal_buffer=case.tree.goal_buffer)


def _compare(eng, ref, tracks, extents, start, W):
    st, clear, dwell = eng.tree_clear_rects_wait(tracks, extents, start, W, per_node=True)
    print(st)
    assert clear.dtype == np.uint64 and dwell.dtype == np.uint64
    np.testing.assert_array_equal(clear, ref["clear"])
    np.testing.assert_array_equal(dwell, ref["dwell_ok"])
    assert st == ref["stats"] and tuple(st) == rw.STAT_KEYS
    assert eng.tree_clear_rects_wait(tracks, extents, start, W) == ref["stats"]   # the counters alone: the same call without the arrays
    return st, clear, dwell


@pytest.mark.parametrize("case", rw.cases(), ids=lambda c: c.name)
def test_hand_built_trees(case):
    """Every case of clear_rects_reference.cases() at W = 8 and the delays' own edges, against the composed reference."""
    c = case.case
    eng = _engine(c)
    assert eng.size == c.tree.size <= 257
    _compare(eng, case.reference(), c.tracks, c.extents, c.start, case.W)
    eng.close()


@pytest.mark.parametrize("case", cr.cases(), ids=lambda c: c.name)
def test_one_delay_is_tree_clear_rects(case):
    """W = 1 against the device's own plain query."""
    eng = _engine(case)
    plain, first, dfirst = eng.tree_clear_rects(case.tracks, case.extents, case.start, per_node=True)
    st, clear, dwell = eng.tree_clear_rects_wait(case.tracks, case.extents, case.start, 1, per_node=True)
    np.testing.assert_array_equal(clear, (first == -1).astype(np.uint64))
    np.testing.assert_array_equal(dwell, (dfirst == -1).astype(np.uint64))
    none = plain["best_end"] < 0
    assert st == dict(size=plain["size"], hits=plain["hits"], clear_hits=plain["clear_hits"], clear_now=plain["clear_hits"],
                      best_end=plain["best_end"], best_wait=-1 if none else 0, best_steps=plain["best_steps"], best_arrival=plain["best_steps"])
    eng.close()


def test_a_tie_on_arrival_goes_to_the_smaller_id():
    """Wait 5 on the short branch (11 steps) arrives exactly when the long branch (16 steps) does at delay 0: node 2 wins over 5."""
    case = rw.case("fork, a tie: wait 5 on the short branch arrives with the long one | W = 8")
    ref = case.reference()
    assert int(ref["clear"][5]) & int(ref["dwell_ok"][5]) & 1 and ref["cum"][5] == 16 == ref["cum"][2] + 5       # the tie, by the reference
    eng = _engine(case.case)
    st, _, _ = _compare(eng, ref, case.case.tracks, case.case.extents, 0, 8)
    assert (st["best_end"], st["best_wait"], st["best_arrival"]) == (2, 5, 16)
    eng.close()


def test_what_a_disc_cannot_say_with_time():
    """The 6 m x 0.4 m rectangle at heading pi/2 across the short branch: as a rectangle a wait of 4 rows clears it; the covering
    disc on the same centre track needs a strictly longer wait, or finds nothing within W.  Both sides by the references first."""
    case = rw.case("fork, a 6 x 0.4 rectangle at heading pi/2 crosses the short branch | W = 8")
    c = case.case
    rect, disc = case.reference(), case.disc_reference()
    assert rect["stats"]["best_wait"] == 4 and rect["stats"]["best_end"] == 2
    assert disc["stats"] != rect["stats"] and (disc["stats"]["best_end"] == -1 or disc["stats"]["best_arrival"] > rect["stats"]["best_arrival"])
    assert not np.array_equal(disc["clear"], rect["clear"])
    eng = _engine(c)
    _compare(eng, rect, c.tracks, c.extents, 0, 8)
    st, clear, dwell = eng.tree_clear_wait(np.ascontiguousarray(c.tracks[:, :, :2]), c.radii, 0, 8, per_node=True)
    np.testing.assert_array_equal(clear, disc["clear"])
    np.testing.assert_array_equal(dwell, disc["dwell_ok"])
    assert st == disc["stats"]
    eng.close()


@pytest.mark.parametrize("name", ["car_2000", "boat_advanced_3000"])
def test_fixture_trees(name):
    """One call with W = 16 against the direct reference."""
    f = cl.fixture(name)
    s = f.native()
    eng = _load(s, f, f.H, dt=s.plan_kwargs["dt"])
    tracks, extents = cr.fixture_tracks(f)
    W = rw.FIXTURE_W
    st, clear, dwell = _compare(eng, rw.fixture_reference(name), tracks, extents, 0, W)
    assert st["clear_hits"] > 0 and st["hits"] > st["clear_hits"]
    assert any(0 < int(m) < rw.all_mask(W) for m in clear)          # (of the inputs: the delays differ somewhere)
    eng.close()


# ------------------------------------------------------------------------------------------------ refusals

def test_refusals_on_the_device():
    import lqrrt_amd
    from lqrrt_amd import _native as nat
    from lqrrt_amd.engine import Engine, NodeTable
    c = cr.case("fork, the rectangle crosses the short branch")
    eng = _engine(c)
    good = eng.tree_clear_rects_wait(c.tracks, c.extents, 0, 8)
    fp = eng.footprint()
    for bad in (dict(tracks=np.zeros((0, 1, 3)), extents=(1.0, 0.5)), dict(tracks=c.tracks, extents=c.extents, start=-1),
                dict(tracks=c.tracks, extents=-c.extents - 1.0), dict(tracks=c.tracks, extents=c.extents, waits=0),
                dict(tracks=c.tracks, extents=c.extents, waits=65), dict(tracks=c.tracks, extents=c.extents, waits=2.0),
                dict(tracks=c.tracks, extents=c.extents, start=2 ** 31 - 16, waits=1)):       # start + the deepest cum (16) = 2^31
        with pytest.raises(ValueError):
            eng.tree_clear_rects_wait(**bad)
    for start, waits in ((2 ** 31 - 17, 2), (2 ** 31 - 17 - 62, 64)):                        # ... and the longest wait counts
        with pytest.raises(ValueError, match="start \\+ the longest wait \\+ the deepest"):
            eng.tree_clear_rects_wait(c.tracks, c.extents, start, waits)
    assert eng.tree_clear_rects_wait(c.tracks, c.extents, 2 ** 31 - 17, 1)["size"] == 11      # 2^31 - 1 still fits
    assert eng.tree_clear_rects_wait(c.tracks, c.extents, 2 ** 31 - 17 - 63, 64)["size"] == 11
    with pytest.raises(ValueError, match="^(?!.*longest wait).*leave 31 bits"):               # the plain call's text is what it was
        eng.tree_clear_rects(c.tracks, c.extents, 2 ** 31 - 16)
    # the ABI's own checks (the wrapper above refuses most of them first): each its code, and in clear_rects_check's order -- bad
    # extents are named before bad waits, bad waits before a missing goal
    st = nat.ClearWaitStats()
    tr, ex = np.ascontiguousarray(c.tracks), np.ascontiguousarray(c.extents)
    L, D = tr.shape[:2]
    badhead, negext = tr.copy(), ex.copy()
    badhead[0, 0, 2] = np.nan
    negext[-1, 1] = -1e-300

    def last():
        return nat.lib().lqrrt_last_error().decode()

    def call(tracks, extents, L_, D_, start, waits, out=st, h=None):
        return nat.lib().lqrrt_tree_clear_rects_wait(eng.h if h is None else h, None if tracks is None else nat.ptr(tracks),
                                                     None if extents is None else nat.ptr(extents), L_, D_, start, waits, out, None, None,
                                                     eng._stream())
    for args in ((None, ex, L, D, 0, 8), (tr, None, L, D, 0, 8), (tr, ex, 0, D, 0, 8), (tr, ex, L, 0, 0, 8), (tr, ex, L, D, -1, 8),
                 (badhead, ex, L, D, 0, 8), (tr, negext, L, D, 0, 8), (tr, ex, L, D, 0, 0), (tr, ex, L, D, 0, 65), (tr, ex, L, D, 0, -1),
                 (tr, ex, L, D, 2 ** 31 - 17, 2)):
        assert call(*args) == nat.E_ARG, args[2:]
    assert call(tr, ex, L, D, 0, 8, None) == nat.E_ARG
    assert call(tr, negext, L, D, 0, 65) == nat.E_ARG and "half width" in last()
    assert call(tr, ex, L, D, 0, 65) == nat.E_ARG and "waits must be 1 .. 64 delays (65)" in last()
    assert eng.tree_clear_rects_wait(c.tracks, c.extents, 0, 8) == good and eng.footprint() == fp
    # a generic engine
    table = NodeTable(4, 1, (2,), capacity=128)
    assert call(tr, ex, L, D, 0, 8, h=table.h) == nat.E_STATE and "lqrrt_tree_clear_rects_wait: not available for LQRRT_MODEL_GENERIC" in last()
    table.close()
    # no goal; bad waits are still named first
    eng.set_resolution(0.1, 0.0, cl.H_HAND, np.ones(6), None, None)
    xe, ue = c.tree.packed()
    eng.tree_load(c.tree.state, c.tree.K, c.tree.pID, c.tree.elen, xe, ue)
    with pytest.raises(nat.NativeError) as ex_:
        eng.tree_clear_rects_wait(c.tracks, c.extents, 0, 8)
    assert ex_.value.code == nat.E_STATE and "goal" in str(ex_.value)
    assert call(tr, ex, L, D, 0, 65) == nat.E_ARG
    eng.close()
    # models without the path
    for s in (lqrrt_amd.systems.DoublePendulum(), lqrrt_amd.systems.DoubleIntegrator(n_boxes=8, seed=1)):
        e2 = Engine(s, capacity=64, max_wave=64)
        e2.set_resolution(0.1, 0.0, 4, np.ones(s.nstates), s.goal, np.abs(np.asarray(s.goal_buffer, dtype=np.float64)))
        e2.tree_reset(s.x0)
        with pytest.raises(nat.NativeError) as ex_:
            e2.tree_clear_rects_wait(np.zeros((2, 1, 3)), (1.0, 0.5), 0, 8)
        assert ex_.value.code == nat.E_STATE and "lqrrt_tree_clear_rects_wait" in str(ex_.value) and "circle" in str(ex_.value)
        e2.close()
    # a hull that does not fit in a workgroup's LDS -- and one whose 16 V bytes are exactly the limit: the check's 64 bytes of its
    # own come on top.  The engine answers a good call afterwards all the same.
    big = lqrrt_amd.systems.BoatIntermediate(0)
    big.vps = np.random.RandomState(0).uniform(-1, 1, (2, 20000))
    big.set_obstacles(np.zeros((0, 3)))
    e3 = _load(big, c.tree, cl.H_HAND, goal=c.tree.goal, goal_buffer=c.tree.goal_buffer)
    with pytest.raises(ValueError, match="LDS") as ex_:
        e3.tree_clear_rects_wait(c.tracks, c.extents, 0, 8)
    limit = int(re.search(r"the device's limit is (\d+)", str(ex_.value)).group(1))
    assert e3.size == 11 and limit % 16 == 0 and limit // 16 < 20000
    e3.close()
    big.vps = np.random.RandomState(0).uniform(-1, 1, (2, limit // 16))
    big.set_obstacles(np.zeros((0, 3)))
    e3 = _load(big, c.tree, cl.H_HAND, goal=c.tree.goal, goal_buffer=c.tree.goal_buffer)
    with pytest.raises(ValueError, match="16 V = %d bytes \\(V = %d\\), the device's limit is %d" % (limit, limit // 16, limit)):
        e3.tree_clear_rects_wait(c.tracks, c.extents, 0, 8)
    e3.close()
    e4 = _engine(c)
    assert e4.tree_clear_rects_wait(c.tracks, c.extents, 0, 8) == good
    e4.close()


# ------------------------------------------------------------------------------------------------ nothing is modified

def test_the_tree_is_not_modified_and_grows_on_as_its_twin():
    s, eng = _grown()
    _, twin = _grown()
    before = rr.engine_arrays(eng)
    ign, best, fp, counters, mt = eng.ignored(), eng.plan_best(), eng.footprint(), eng.counters().as_dict(), eng.get_mt19937()
    states = eng.states()
    W, start = 12, 3
    # two rectangles that are far away except for four instants each, when they lie on a node's state: the instants that node has
    # at the delays 3 .. 6.  Whoever is there earlier or later passes: the delays differ.
    cum = np.zeros(len(states), dtype=np.int64)
    cum[0] = before[3][0]
    for i in range(1, len(states)):
        cum[i] = cum[before[2][i]] + before[3][i]
    picked = (len(states) // 3, len(states) // 2)
    L = start + int(max(cum[j] for j in picked)) + 40
    tracks = np.zeros((L, 2, 3))
    tracks[:, :, :2] = 900.0
    tracks[:, :, 2] = (0.4, np.pi / 2)
    for d, j in enumerate(picked):
        at = start + int(cum[j]) - 1
        tracks[at + 3:at + 7, d, :2] = states[j, :2]
    extents = np.array([[3.0, 1.0], [2.0, 0.5]])
    st, clear, dwell = eng.tree_clear_rects_wait(tracks, extents, start, W, per_node=True)
    lo, hi = rr.goal_box(s)
    ref = rw.clear_rects_wait_direct(before[0], before[2], before[3], before[4], rw.culled_test_of(s), tracks, extents, start, W, lo, hi)
    np.testing.assert_array_equal(clear, ref["clear"])
    np.testing.assert_array_equal(dwell, ref["dwell_ok"])
    assert st == ref["stats"] and any(0 < int(m) < rw.all_mask(W) for m in clear)
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

def _car_planner(seed, max_nodes):
    """A car with the small hull and no static obstacle, its tree grown on the device."""
    import lqrrt_amd as lqrrt
    s = lqrrt.systems.Car(0)
    s.vps = fr.lattice_hull(1.0, 0.5, 0.25)
    s.set_obstacles(np.zeros((0, 3)))
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


def _reference_of(s, p, tracks, extents, start, W):
    state, pID, elen, xedge, lo, hi = _tree_of(s, p)
    table, extents, start = p._engine.rect_table(tracks, extents, start)
    return rw.clear_rects_wait_direct(state, pID, elen, xedge, rw.culled_test_of(s), table, extents, start, W, lo, hi)


def _plain_reference_of(s, p, tracks, extents, start=0):
    state, pID, elen, xedge, lo, hi = _tree_of(s, p)
    table, extents, start = p._engine.rect_table(tracks, extents, start)
    return cr.clear_rects(state, pID, elen, xedge, rw.culled_test_of(s), table, extents, start, lo, hi)


def _plan_first(ref, end, dt, start=0):
    taus = [int(t) for t in (ref["first"][end], ref["dwell_first"][end]) if t >= 0]
    return (min(taus) - start) * dt if taus else None


def _gate(rows, c):
    """A square of half side 1 cm, heading 0, that is far away except at instant c, when its centre stands on the bow point (0.5, 0)
    of the hull of the vehicle that follows `rows` on time.  The hull points lie on a 0.25 m lattice: who is there one row later, a
    few centimetres further back, has no hull point within the square -- unless it moves less than 1 cm per row, or a multiple of
    0.25 m."""
    tracks = np.zeros((len(rows) + 40, 1, 3))
    tracks[:, 0, :2] = 900.0
    tracks[c, 0, :2] = rows[c, :2] + 0.5 * np.array([np.cos(rows[c, 2]), np.sin(rows[c, 2])])
    return tracks, np.array([[0.01, 0.01]])


def test_avoid_rects_waits_at_the_start():
    s, p = _car_planner(1, 700)
    assert p.plan_reached_goal and p.plan_wait == 0
    old_seq, old_x = list(p.node_seq), np.array(p.x_seq)
    # of the inputs, with the reference alone: a gate on the tree's shortest plan that a wait of 1 .. 7 rows answers best
    state, pID, elen, xedge, _, _ = _tree_of(s, p)
    far = np.zeros((1, 1, 3))
    far[0, 0, :2] = 900.0
    short = _reference_of(s, p, far, (0.5, 0.5), 0, 1)["stats"]["best_end"]
    rows = np.concatenate([xedge[v, :elen[v]] for v in p._engine.climb(short)])
    speed = np.linalg.norm(np.diff(rows[:, :2], axis=0), axis=1)
    for c in np.argsort(-speed)[:40:8]:                             # where the vehicle is fastest: it is out of the way in a row
        tracks, extents = _gate(rows, int(c))
        ref = _reference_of(s, p, tracks, extents, 0, 8)
        print(c, speed[c], ref["stats"])
        if ref["stats"]["best_wait"] >= 1:
            break
    want = ref["stats"]
    assert want["best_wait"] >= 1 and not int(ref["clear"][short]) & 1
    # max_wait = 0: the plain query, its dict, its adoption, as before -- the reference supplies the values
    plain_ref = _plain_reference_of(s, p, tracks, extents)
    plain = p.avoid_rects(tracks, extents, adopt=False)
    assert list(plain) == list(cl.STAT_KEYS) + ["plan_first"] and {k: plain[k] for k in cl.STAT_KEYS} == plain_ref["stats"]
    assert plain["plan_first"] == _plan_first(plain_ref, old_seq[-1], p.dt)
    assert plain == p.avoid_rects(tracks, extents, adopt=False, max_wait=0) == p.avoid_rects(tracks, extents, 0, False, 0)
    assert list(p.node_seq) == old_seq and p.plan_wait == 0
    # adopt=False with waits: the answer, and nothing else
    out = p.avoid_rects(tracks, extents, adopt=False, max_wait=7)
    assert {k: out[k] for k in rw.STAT_KEYS} == want and out["plan_first"] == plain["plan_first"] and list(out) == list(rw.STAT_KEYS) + ["plan_first"]
    assert list(p.node_seq) == old_seq and np.array_equal(np.array(p.x_seq), old_x) and p.plan_wait == 0
    # adopt
    out = p.avoid_rects(tracks, extents, max_wait=7)
    best, wait = want["best_end"], want["best_wait"]
    assert {k: out[k] for k in rw.STAT_KEYS} == want and out["plan_first"] == plain["plan_first"]
    assert p.node_seq == p._engine.climb(best) and p.plan_wait == wait and p.plan_reached_goal
    assert len(p.x_seq) == want["best_arrival"] == want["best_steps"] + wait == len(p.u_seq) == len(p.t_seq)
    X = np.asarray(p.x_seq, dtype=np.float64)
    for k in range(1, wait + 1):
        np.testing.assert_array_equal(X[k], X[0])
        np.testing.assert_array_equal(np.asarray(p.u_seq[k]), np.asarray(p.u_seq[0]))
    np.testing.assert_array_equal(X[wait:], np.concatenate([xedge[v, :elen[v]] for v in p.node_seq]))
    np.testing.assert_array_equal(X[0], state[0])
    assert p.T == len(X) * p.dt and np.array_equal(p.t_seq, np.arange(len(X)) * p.dt)
    # the adopted plan is clear row by row with the plain model, the wait at the start and at the goal included
    test = cr.row_test_of(s)
    c_, s_ = fr.portable_sincos(X[:, 2])
    table = cr.rect_table(tracks, extents)
    assert test(X, c_, s_, table[np.minimum(np.arange(len(X)), len(table) - 1)]).all()
    rest = np.arange(len(X), len(table))
    assert test(np.repeat(X[-1:], len(rest), axis=0), np.repeat(c_[-1], len(rest)), np.repeat(s_[-1], len(rest)), table[rest]).all()
    # ... and so says the next call, which leaves it alone: no plain call is made for plan_first
    calls = []
    plain_call = p._engine.tree_clear_rects
    p._engine.tree_clear_rects = lambda *a, **k: calls.append(a) or plain_call(*a, **k)
    again = p.avoid_rects(tracks, extents, max_wait=7)
    del p._engine.tree_clear_rects
    assert calls == [] and again["plan_first"] is None and (again["best_end"], again["best_wait"]) == (best, wait) and p.plan_wait == wait
    np.testing.assert_array_equal(np.asarray(p.x_seq, dtype=np.float64), X)
    # any other call that sets a plan drops the wait
    p.avoid_rects(far, (0.5, 0.5))
    assert p.plan_wait == 0 and len(p.x_seq) == len(np.concatenate([xedge[v, :elen[v]] for v in p.node_seq]))


def _scene():
    spec = importlib.util.spec_from_file_location("channel_wait_gpu", os.path.join(ROOT, "examples", "channel_wait_gpu.py"))
    scene = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(scene)
    return scene


def test_channel_scene_the_loop_with_waits_takes_the_channel():
    """The narrowed channel of examples/channel_wait_gpu.py: the hand loop over avoid_rects.  Without a wait B is sent the way
    round; with max_wait B and C hold three ticks and take the channel, and every later plan is clear of the earlier hulls -- per
    the reference, which also supplies every answer's values."""
    scene = _scene()
    (plain, _), (waited, planners) = scene.run(printing=False)
    print(plain, waited)
    assert plain[0] is None and (plain[1]["best_steps"], plain[1]["best_wait"] if "best_wait" in plain[1] else 0) == (scene.ROUND_STEPS, 0)
    assert [(a["best_steps"], a["best_wait"], a["best_arrival"]) for a in waited[1:]] == [(scene.SHORT_STEPS, 3, scene.SHORT_STEPS + 3)] * 2
    assert [p.plan_wait for p in planners] == [0, 3, 3]
    plans = [np.asarray(p.x_seq, dtype=np.float64) for p in planners]
    for k in (1, 2):
        p = planners[k]
        state, _, pID, elen, xedge, _ = rr.engine_arrays(p._engine)
        buf = np.abs(np.asarray(p.constraints.goal_buffer, dtype=np.float64))
        lo, hi = np.asarray(p.goal, dtype=np.float64) - buf, np.asarray(p.goal, dtype=np.float64) + buf
        table, ext, _ = p._engine.rect_table([q[:, :3] for q in plans[:k]], [scene.EXTENT] * k, 0)
        test = cr.row_test("hull", scene.hull_points())
        ref = rw.clear_rects_wait(state, pID, elen, xedge, test, table, ext, 0, scene.MAX_WAIT + 1, lo, hi)
        assert {key: waited[k][key] for key in rw.STAT_KEYS} == ref["stats"]
        # the adopted plan, wait rows included, row by row against the earlier hulls at their instants, and while it waits at the goal
        X = plans[k]
        c_, s_ = fr.portable_sincos(X[:, 2])
        rects = cr.rect_table(table, ext)
        assert test(X, c_, s_, rects[np.minimum(np.arange(len(X)), len(rects) - 1)]).all()
        rest = np.arange(len(X), len(rects))
        assert test(np.repeat(X[-1:], len(rest), axis=0), np.repeat(c_[-1], len(rest)), np.repeat(s_[-1], len(rest)), rects[rest]).all()
        np.testing.assert_array_equal(X[:p.plan_wait + 1], np.repeat(X[:1], p.plan_wait + 1, axis=0))
