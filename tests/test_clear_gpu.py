"""
The clearance query on the device (csrc/clear.hpp through lqrrt_tree_clear, Engine.tree_clear, Planner.avoid, deconflict) against
the reference of the rule (tests/clear_reference.py).  Everything compared is an integer or a flag and must be EQUAL: the per-node
first / dwell_first arrays, the counters, the best plan.  Trees are put on the device with tree_load (hand-built ones, the committed
fixtures); tests/test_clear_cpu.py shows with the reference alone that none of the inputs is degenerate.
"""
import numpy as np
import pytest

import clear_reference as cl
import feasibility_reference as fr
import retain_reference as rr
from clear_common import WAVE, _grown, _load

pytestmark = pytest.mark.gpu


def _compare(eng, ref, tracks, radii, start):
    st, first, dwell = eng.tree_clear(tracks, radii, start, per_node=True)
    print(st)
    np.testing.assert_array_equal(first, ref["first"])
    np.testing.assert_array_equal(dwell, ref["dwell_first"])
    assert first.dtype == np.int32 and dwell.dtype == np.int32
    assert st == ref["stats"]
    assert eng.tree_clear(tracks, radii, start) == ref["stats"]                   # the counters alone: the same call without the arrays
    return st, first, dwell


@pytest.mark.parametrize("case", cl.cases(), ids=lambda c: c.name)
def test_hand_built_trees(case):
    eng = _load(case.native(), case.tree, cl.H_HAND, goal=case.tree.goal, goal_buffer=case.tree.goal_buffer)
    assert eng.size == case.tree.size
    _compare(eng, case.reference(), case.tracks, case.radii, case.start)
    eng.close()


def test_time_decides_the_fork():
    """The same disc, the same tree: with start = 0 the best plan moves to the long branch, with start = 4 the disc has passed before
    the vehicle arrives and the short branch wins again.  An implementation that ignores time cannot give both."""
    a, b = cl.case("fork, the disc crosses the short branch"), cl.case("fork, the disc has passed (start = 4)")
    assert np.array_equal(a.tracks, b.tracks) and np.array_equal(a.tree.xedge, b.tree.xedge) and (a.start, b.start) == (0, 4)
    eng = _load(a.native(), a.tree, cl.H_HAND, goal=a.tree.goal, goal_buffer=a.tree.goal_buffer)
    sa, sb = eng.tree_clear(a.tracks, a.radii, 0), eng.tree_clear(a.tracks, a.radii, 4)
    assert (sa["best_end"], sa["best_steps"]) == (5, 16) and (sb["best_end"], sb["best_steps"]) == (2, 11)
    # a list of per-disc tracks of different lengths is padded by holding the last row
    short = [a.tracks[:, 0][:1], a.tracks[:, 1]]
    assert eng.tree_clear(short, a.radii, 0) == sa
    eng.close()


def test_a_standing_disc_is_the_same_circle_in_the_static_map():
    """L = 1, one disc: first[i] == -1 exactly for the nodes that tree_retain(0, revalidate=True) keeps on a twin engine whose
    static map holds the same circle."""
    f = cl.fixture("boat_advanced_3000")
    rows = f.plan_rows()
    disc = np.array([rows[(3 * len(rows)) // 4, 0], rows[(3 * len(rows)) // 4, 1], 1.25])
    s = f.native()
    s.set_obstacles(np.zeros((0, 3)))                               # (the clearance check does not look at the static map anyway)
    eng = _load(s, f, f.H, dt=s.plan_kwargs["dt"])
    st, first, _ = eng.tree_clear(disc[None, None, :2], disc[2], 0, per_node=True)
    twin_s = f.native()
    twin_s.set_obstacles(disc[None, :])
    twin = _load(twin_s, f, f.H, dt=s.plan_kwargs["dt"])
    stats, old_to_new = twin.tree_retain(0, revalidate=True)
    print(st, stats)
    np.testing.assert_array_equal(first == -1, old_to_new >= 0)
    assert 0 < stats["kept"] < stats["old_size"] and stats["infeasible"] == st["conflicts"] and stats["orphaned"] == st["blocked"]
    eng.close()
    twin.close()


@pytest.mark.parametrize("name", ["car_2000", "boat_advanced_3000"])
def test_fixture_trees(name):
    f = cl.fixture(name)
    s = f.native()
    eng = _load(s, f, f.H, dt=s.plan_kwargs["dt"])
    tracks, radii = f.tracks()
    st, first, dwell = _compare(eng, cl.fixture_reference(name), tracks, radii, 0)
    assert st["clear_hits"] > 0 and st["hits"] > st["clear_hits"] and first[f.plan[-1]] >= 0
    eng.close()


# ------------------------------------------------------------------------------------------------ refusals

def test_refusals_on_the_device():
    import lqrrt_amd
    from lqrrt_amd import _native as nat
    from lqrrt_amd.engine import Engine
    c = cl.case("fork, the disc crosses the short branch")
    eng = _load(c.native(), c.tree, cl.H_HAND, goal=c.tree.goal, goal_buffer=c.tree.goal_buffer)
    good = eng.tree_clear(c.tracks, c.radii, 0)
    fp = eng.footprint()
    for bad in (dict(tracks=np.zeros((0, 1, 2)), radii=0.5), dict(tracks=np.zeros((3, 0, 2)), radii=0.5),
                dict(tracks=c.tracks, radii=c.radii, start=-1), dict(tracks=np.full((3, 2, 2), np.nan), radii=0.5),
                dict(tracks=c.tracks, radii=-c.radii - 1.0), dict(tracks=c.tracks, radii=c.radii, start=2 ** 31 - 1),
                dict(tracks=c.tracks, radii=c.radii, start=2 ** 31 - 16)):        # start + the deepest cum (16) = 2^31
        with pytest.raises(ValueError):
            eng.tree_clear(**bad)
    assert eng.tree_clear(c.tracks, c.radii, 2 ** 31 - 17)["size"] == 11           # ... and 2^31 - 1 still fits
    # the ABI's own checks (the wrapper above refuses most of them first): L, D, start, a position, a radius
    st = nat.ClearStats()
    tr, ra = np.ascontiguousarray(c.tracks), np.ascontiguousarray(c.radii)
    L, D = tr.shape[:2]
    nanpos = tr.copy()
    nanpos[-1, -1, 1] = np.inf
    negr = ra.copy()
    negr[-1] = -1e-300
    for args in ((tr, ra, 0, D, 0), (tr, ra, L, 0, 0), (tr, ra, L, D, -1), (nanpos, ra, L, D, 0), (tr, negr, L, D, 0)):
        rc = nat.lib().lqrrt_tree_clear(eng.h, nat.ptr(args[0]), nat.ptr(args[1]), args[2], args[3], args[4], st, None, None, eng._stream())
        assert rc == nat.E_ARG, args[2:]
    assert eng.tree_clear(c.tracks, c.radii, 0) == good and eng.footprint() == fp
    # no goal
    eng.set_resolution(0.1, 0.0, cl.H_HAND, np.ones(6), None, None)
    xe, ue = c.tree.packed()
    eng.tree_load(c.tree.state, c.tree.K, c.tree.pID, c.tree.elen, xe, ue)
    with pytest.raises(nat.NativeError) as ex:
        eng.tree_clear(c.tracks, c.radii, 0)
    assert ex.value.code == nat.E_STATE and "goal" in str(ex.value)
    eng.close()
    # models without a circle path
    for s in (lqrrt_amd.systems.DoublePendulum(), lqrrt_amd.systems.DoubleIntegrator(n_boxes=8, seed=1)):
        e2 = Engine(s, capacity=64, max_wave=64)
        e2.set_resolution(0.1, 0.0, 4, np.ones(s.nstates), s.goal, np.abs(np.asarray(s.goal_buffer, dtype=np.float64)))
        e2.tree_reset(s.x0)
        with pytest.raises(nat.NativeError) as ex:
            e2.tree_clear(np.zeros((2, 1, 2)), 0.5)
        assert ex.value.code == nat.E_STATE and "circle" in str(ex.value)
        e2.close()
    # a hull that does not fit in a workgroup's LDS
    big = lqrrt_amd.systems.BoatIntermediate(0)
    big.vps = np.random.RandomState(0).uniform(-1, 1, (2, 20000))
    big.set_obstacles(np.zeros((0, 3)))
    e3 = _load(big, c.tree, cl.H_HAND, goal=c.tree.goal, goal_buffer=c.tree.goal_buffer)
    with pytest.raises(ValueError, match="LDS"):
        e3.tree_clear(c.tracks, c.radii, 0)
    e3.close()


# ------------------------------------------------------------------------------------------------ nothing is modified

def test_the_tree_is_not_modified_and_grows_on_as_its_twin():
    s, eng = _grown()
    _, twin = _grown()
    before = rr.engine_arrays(eng)
    ign, best, fp, counters, mt = eng.ignored(), eng.plan_best(), eng.footprint(), eng.counters().as_dict(), eng.get_mt19937()
    states = eng.states()
    mid = states[len(states) // 2]
    L = 300
    tracks = np.zeros((L, 2, 2))
    tracks[:, 0] = mid[:2]
    tracks[:, 1, 0] = states[len(states) // 3, 0]
    tracks[:, 1, 1] = states[len(states) // 3, 1] + 0.2 * (np.arange(L) - 40)
    st, first, dwell = eng.tree_clear(tracks, [2.0, 1.0], 3, per_node=True)
    lo, hi = rr.goal_box(s)
    ref = cl.clear(before[0], before[2], before[3], before[4], cl.row_test_of(s), tracks, [2.0, 1.0], 3, lo, hi)
    np.testing.assert_array_equal(first, ref["first"])
    np.testing.assert_array_equal(dwell, ref["dwell_first"])
    assert st == ref["stats"] and st["conflicts"] > 0 and st["blocked"] > 0
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

def _car_planner(seed, max_nodes, small_hull=False, x0=(0.0, 0.0)):
    import lqrrt_amd as lqrrt
    s = lqrrt.systems.Car(0)
    if small_hull:
        s.vps = fr.lattice_hull(1.0, 0.5, 0.25)
    s.x0 = np.array([x0[0], x0[1], 0.0, 0.0, 0.0])
    cons = lqrrt.Constraints(s.nstates, s.ncontrols, s.goal_buffer, s.is_feasible)
    p = lqrrt.Planner(s.dynamics, s.lqr, cons, error_tol=s.error_tol, erf=s.erf, min_time=1.0, max_time=2.0, max_nodes=max_nodes,
                      goal0=s.goal, sys_time=lambda: 0.0, printing=False, wave_size=1024, **s.plan_kwargs)
    np.random.seed(seed)
    p.update_plan(s.x0, s.sample_space, goal_bias=s.goal_bias, xrand_gen=10)
    return s, p


def _reference_of(s, p, tracks, radii, start=0):
    state, _, pID, elen, xedge, _ = rr.engine_arrays(p._engine)
    lo, hi = rr.goal_box(s)
    table, radii, start = p._engine.track_table(tracks, radii, start)
    return cl.clear(state, pID, elen, xedge, cl.row_test_of(s), table, radii, start, lo, hi)


def _plan_tracks(p):
    """Two discs on the plan as it stands: one crosses it at 75 % of its rows when the vehicle is there, one parks on its end 20 rows
    after the vehicle has arrived."""
    rows = np.asarray(p.x_seq, dtype=np.float64)
    P = len(rows)
    L, c = P + 60, (75 * P) // 100
    t = np.arange(L, dtype=np.float64)
    tracks = np.zeros((L, 2, 2))
    tracks[:, 0, 0] = rows[c, 0] + 0.05 * (t - c)
    tracks[:, 0, 1] = rows[c, 1] + 0.5 * (t - c)
    tracks[:, 1] = (900.0, 900.0)
    tracks[P + 20:, 1] = rows[-1, :2]
    return tracks, np.array([0.6, 0.5])


def test_avoid_adopts_the_references_best_and_reports_the_plans_first_conflict():
    s, p = _car_planner(1, 2000)
    assert p.plan_reached_goal and p.tree.size == 2001
    old_seq, old_x, old_T = list(p.node_seq), np.array(p.x_seq), p.T
    tracks, radii = _plan_tracks(p)
    ref = _reference_of(s, p, tracks, radii)
    print(ref["stats"])
    end = old_seq[-1]
    assert ref["stats"]["best_end"] not in (-1, end) and ref["first"][end] >= 0    # (of the inputs: the plan is hit, another one is clear)
    want_first = min(int(ref["first"][end]), int(ref["dwell_first"][end]) if ref["dwell_first"][end] >= 0 else 2 ** 31) * p.dt
    # adopt=False: the answer, and nothing else
    out = p.avoid(tracks, radii, adopt=False)
    assert {k: out[k] for k in cl.STAT_KEYS} == ref["stats"] and out["plan_first"] == want_first
    assert list(p.node_seq) == old_seq and np.array_equal(np.array(p.x_seq), old_x) and p.T == old_T
    # no clear hit: a disc as large as the goal box parked on the goal for good
    none = p.avoid(np.tile(np.asarray(s.goal, dtype=np.float64)[None, None, :2], (4, 1, 1)), 30.0)
    assert none["best_end"] == -1 and none["clear_hits"] == 0 and none["plan_first"] is not None
    assert list(p.node_seq) == old_seq and p.T == old_T and p.plan_reached_goal
    # adopt
    out = p.avoid(tracks, radii)
    best = ref["stats"]["best_end"]
    assert {k: out[k] for k in cl.STAT_KEYS} == ref["stats"] and out["plan_first"] == want_first
    assert p.node_seq == p._engine.climb(best) and p.node_seq[-1] == best and p.plan_reached_goal
    assert len(p.x_seq) == ref["stats"]["best_steps"] == len(p.u_seq) == len(p.t_seq) and p.T == len(p.x_seq) * p.dt
    np.testing.assert_array_equal(p.get_state(p.T + 5.0), np.asarray(p.x_seq[-1]))
    # the adopted plan is clear, and so says the next call
    again = p.avoid(tracks, radii)
    assert again["plan_first"] is None and again["best_end"] == best and p.node_seq[-1] == best
    # ... checked row by row with the plain model: no row of the new plan meets a disc at its instant, nor does the wait at the goal
    test = cl.row_test_of(s)
    X = np.asarray(p.x_seq, dtype=np.float64)
    c_, s_ = fr.portable_sincos(X[:, 2])
    discs = np.concatenate((tracks, np.broadcast_to(radii[None, :, None], tracks.shape[:2] + (1,))), axis=2)
    assert test(X, c_, s_, discs[np.minimum(np.arange(len(X)), len(discs) - 1)]).all()
    wait = np.arange(len(X), len(discs))
    assert test(np.repeat(X[-1:], len(wait), axis=0), np.repeat(c_[-1], len(wait)), np.repeat(s_[-1], len(wait)), discs[wait]).all()


def test_deconflict_is_the_loop_of_reference_calls_in_its_order():
    import lqrrt_amd as lqrrt
    made = [_car_planner(seed, 700, small_hull=True, x0=x0) for seed, x0 in ((2, (0.0, 0.0)), (3, (0.0, 30.0)), (4, (30.0, 0.0)))]
    systems, planners = [m[0] for m in made], [m[1] for m in made]
    order, radii = [1, 2, 0], np.array([0.8, 0.6, 0.7])
    plans = [np.asarray(p.x_seq, dtype=np.float64)[:, :2].copy() for p in planners]
    ends = [p.node_seq[-1] for p in planners]
    # the loop of reference calls: every planner against the plans of those before it, as the reference leaves them
    want = [None] * 3
    for at, k in enumerate(order):
        if at == 0:
            continue
        before = order[:at]
        ref = _reference_of(systems[k], planners[k], [plans[j] for j in before], radii[before])
        want[k] = ref["stats"]
        if ref["stats"]["best_end"] >= 0:
            state, _, pID, elen, xedge, _ = rr.engine_arrays(planners[k]._engine)
            chain = planners[k]._engine.climb(ref["stats"]["best_end"])
            plans[k] = np.concatenate([xedge[v, :elen[v]] for v in chain])[:, :2]
            ends[k] = ref["stats"]["best_end"]
    got = lqrrt.deconflict(planners, radii, order=order)
    print(want, [None if g is None else g["plan_first"] for g in got])
    assert got[1] is None
    assert any(want[k]["best_end"] >= 0 for k in (2, 0)) and any(want[k]["conflicts"] > 0 for k in (2, 0))      # (of the inputs)
    for k in (2, 0):
        assert {key: got[k][key] for key in cl.STAT_KEYS} == want[k]
    for k in range(3):
        assert planners[k].node_seq[-1] == ends[k]
        np.testing.assert_array_equal(np.asarray(planners[k].x_seq, dtype=np.float64)[:, :2], plans[k])
    # mixed dt
    other = lqrrt.Planner(systems[0].dynamics, systems[0].lqr, planners[0].constraints, error_tol=systems[0].error_tol, erf=systems[0].erf,
                          goal0=systems[0].goal, printing=False, horizon=systems[0].plan_kwargs["horizon"], dt=2 * planners[0].dt)
    with pytest.raises(ValueError, match="share dt"):
        lqrrt.deconflict(planners[:2] + [other], 0.5)
