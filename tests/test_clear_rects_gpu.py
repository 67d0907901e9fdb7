"""
The clearance query against moving oriented rectangles on the device (csrc/clear_rects.hpp through lqrrt_tree_clear_rects,
Engine.tree_clear_rects, Planner.avoid_rects, deconflict(extents=...)) against the reference of the rule
(tests/clear_rects_reference.py).  Everything compared is an integer or a flag and must be EQUAL: the per-node first / dwell_first
arrays, the counters, the best plan.  The reference culls nothing; the kernel's cull must not show.  Trees are put on the device with
tree_load; tests/test_clear_rects_cpu.py shows with the reference alone that none of the inputs is degenerate.
"""
import numpy as np
import pytest

import clear_reference as cl
import clear_rects_reference as cr
import feasibility_reference as fr
import retain_reference as rr
from clear_common import WAVE, _grown, _load

pytestmark = pytest.mark.gpu


def _engine(case):
    return _load(case.native(), case.tree, cl.H_HAND, goal=case.tree.goal, goal_buffer=case.tree.goal_buffer)


def _compare(eng, ref, tracks, extents, start):
    st, first, dwell = eng.tree_clear_rects(tracks, extents, start, per_node=True)
    print(st)
    np.testing.assert_array_equal(first, ref["first"])
    np.testing.assert_array_equal(dwell, ref["dwell_first"])
    assert first.dtype == np.int32 and dwell.dtype == np.int32
    assert st == ref["stats"]
    assert eng.tree_clear_rects(tracks, extents, start) == ref["stats"]            # the counters alone: the same call without the arrays
    return st, first, dwell


@pytest.mark.parametrize("case", cr.cases(), ids=lambda c: c.name)
def test_hand_built_trees(case):
    eng = _engine(case)
    assert eng.size == case.tree.size
    _compare(eng, case.reference(), case.tracks, case.extents, case.start)
    eng.close()


def test_what_a_disc_cannot_say_and_the_heading_decides():
    """A 6 m x 0.4 m rectangle comes down y = 0.6 beside the short branch: node 2 stays the best plan, 11 steps.  The disc that covers
    it (tree_clear, radius sqrt(a^2 + b^2), the same centre track) sweeps the short branch.  Turned by pi/2 the rectangle does too."""
    c, turned = cr.case("fork, a 6 x 0.4 rectangle passes beside the short branch"), cr.case("fork, the same track, heading pi/2")
    eng = _engine(c)
    st = eng.tree_clear_rects(c.tracks, c.extents, 0)
    assert (st["best_end"], st["best_steps"]) == (2, 11)
    disc, first, _ = eng.tree_clear(np.ascontiguousarray(c.tracks[:, :, :2]), c.radii, 0, per_node=True)
    assert disc == c.disc_reference()["stats"] and disc["best_end"] != 2 and first[2] >= 0
    st, first, _ = eng.tree_clear_rects(turned.tracks, turned.extents, 0, per_node=True)
    assert first[2] == 7 and (st["best_end"], st["best_steps"]) == (5, 16)
    # a list of per-rectangle tracks of different lengths is padded by holding the last row
    short = [c.tracks[:, 0][:1], c.tracks[:, 1]]
    assert eng.tree_clear_rects(short, c.extents, 0) == eng.tree_clear_rects(c.tracks, c.extents, 0)
    eng.close()


def test_the_inclusive_edge_and_zero_extents():
    """One engine, the extents alone differ: a hull point on the edge is a hit, one ulp less of the extent and the branch is clear."""
    on = cr.case("edge: a hull point on |xi| == a")
    eng = _engine(on)
    for hit, miss in (("edge: a hull point on |xi| == a", "edge: |xi| one ulp beyond a"), ("edge: a hull point on |eta| == b", "edge: |eta| one ulp beyond b")):
        a, b = cr.case(hit), cr.case(miss)
        sa, fa, _ = eng.tree_clear_rects(a.tracks, a.extents, 0, per_node=True)
        sb, fb, _ = eng.tree_clear_rects(b.tracks, b.extents, 0, per_node=True)
        assert fa[2] == 7 and fb[2] == -1 and sa["best_end"] == 5 and sb["best_end"] == 2
    z = cr.case("zero extents on a hull point")
    _, fz, _ = eng.tree_clear_rects(z.tracks, z.extents, 0, per_node=True)
    assert fz[2] == 7
    eng.close()


@pytest.mark.parametrize("name", ["car_2000", "boat_advanced_3000"])
def test_fixture_trees(name):
    f = cl.fixture(name)
    s = f.native()
    eng = _load(s, f, f.H, dt=s.plan_kwargs["dt"])
    tracks, extents = cr.fixture_tracks(f)
    st, first, dwell = _compare(eng, cr.fixture_reference(name), tracks, extents, 0)
    assert st["clear_hits"] > 0 and st["hits"] > st["clear_hits"] and first[f.plan[-1]] >= 0
    eng.close()


# ------------------------------------------------------------------------------------------------ refusals

def test_refusals_on_the_device():
    import lqrrt_amd
    from lqrrt_amd import _native as nat
    from lqrrt_amd.engine import Engine
    c = cr.case("fork, the rectangle crosses the short branch")
    eng = _engine(c)
    good = eng.tree_clear_rects(c.tracks, c.extents, 0)
    fp = eng.footprint()
    for bad in (dict(tracks=np.zeros((0, 1, 3)), extents=(1.0, 0.5)), dict(tracks=np.zeros((3, 0, 3)), extents=(1.0, 0.5)),
                dict(tracks=c.tracks, extents=c.extents, start=-1), dict(tracks=np.full((3, 2, 3), np.nan), extents=(1.0, 0.5)),
                dict(tracks=c.tracks, extents=-c.extents - 1.0), dict(tracks=c.tracks, extents=c.extents, start=2 ** 31 - 1),
                dict(tracks=c.tracks, extents=c.extents, start=2 ** 31 - 16)):     # start + the deepest cum (16) = 2^31
        with pytest.raises(ValueError):
            eng.tree_clear_rects(**bad)
    assert eng.tree_clear_rects(c.tracks, c.extents, 2 ** 31 - 17)["size"] == 11   # ... and 2^31 - 1 still fits
    # the ABI's own checks (the wrapper above refuses most of them first): null, L, D, start, a position, a heading, an extent
    st = nat.ClearStats()
    tr, ex = np.ascontiguousarray(c.tracks), np.ascontiguousarray(c.extents)
    L, D = tr.shape[:2]
    badpos, badhead, negext, infext = tr.copy(), tr.copy(), ex.copy(), ex.copy()
    badpos[-1, -1, 1] = np.inf
    badhead[0, 0, 2] = np.nan
    negext[-1, 1] = -1e-300
    infext[0, 0] = np.inf

    def call(tracks, extents, L_, D_, start, out=st):
        return nat.lib().lqrrt_tree_clear_rects(eng.h, None if tracks is None else nat.ptr(tracks), None if extents is None else nat.ptr(extents),
                                                L_, D_, start, out, None, None, eng._stream())
    for args in ((None, ex, L, D, 0), (tr, None, L, D, 0), (tr, ex, 0, D, 0), (tr, ex, L, 0, 0), (tr, ex, L, D, -1), (tr, ex, 2 ** 20, 2 ** 10, 0),
                 (badpos, ex, L, D, 0), (badhead, ex, L, D, 0), (tr, negext, L, D, 0), (tr, infext, L, D, 0)):
        assert call(*args) == nat.E_ARG, args[2:]
    assert call(tr, ex, L, D, 0, None) == nat.E_ARG
    assert eng.tree_clear_rects(c.tracks, c.extents, 0) == good and eng.footprint() == fp
    # no goal
    eng.set_resolution(0.1, 0.0, cl.H_HAND, np.ones(6), None, None)
    xe, ue = c.tree.packed()
    eng.tree_load(c.tree.state, c.tree.K, c.tree.pID, c.tree.elen, xe, ue)
    with pytest.raises(nat.NativeError) as ex_:
        eng.tree_clear_rects(c.tracks, c.extents, 0)
    assert ex_.value.code == nat.E_STATE and "goal" in str(ex_.value)
    eng.close()
    # models without the path
    for s in (lqrrt_amd.systems.DoublePendulum(), lqrrt_amd.systems.DoubleIntegrator(n_boxes=8, seed=1)):
        e2 = Engine(s, capacity=64, max_wave=64)
        e2.set_resolution(0.1, 0.0, 4, np.ones(s.nstates), s.goal, np.abs(np.asarray(s.goal_buffer, dtype=np.float64)))
        e2.tree_reset(s.x0)
        with pytest.raises(nat.NativeError) as ex_:
            e2.tree_clear_rects(np.zeros((2, 1, 3)), (1.0, 0.5))
        assert ex_.value.code == nat.E_STATE and "circle" in str(ex_.value)
        e2.close()
    # a hull that does not fit in a workgroup's LDS, and the engine answers a good call afterwards all the same
    big = lqrrt_amd.systems.BoatIntermediate(0)
    big.vps = np.random.RandomState(0).uniform(-1, 1, (2, 20000))
    big.set_obstacles(np.zeros((0, 3)))
    e3 = _load(big, c.tree, cl.H_HAND, goal=c.tree.goal, goal_buffer=c.tree.goal_buffer)
    with pytest.raises(ValueError, match="LDS"):
        e3.tree_clear_rects(c.tracks, c.extents, 0)
    assert e3.size == 11
    e3.close()
    e4 = _engine(c)
    assert e4.tree_clear_rects(c.tracks, c.extents, 0) == good
    e4.close()


# ------------------------------------------------------------------------------------------------ nothing is modified

def test_the_tree_is_not_modified_and_grows_on_as_its_twin():
    s, eng = _grown()
    _, twin = _grown()
    before = rr.engine_arrays(eng)
    ign, best, fp, counters, mt = eng.ignored(), eng.plan_best(), eng.footprint(), eng.counters().as_dict(), eng.get_mt19937()
    states = eng.states()
    mid = states[len(states) // 2]
    L = 300
    tracks = np.zeros((L, 2, 3))
    tracks[:, 0, :2] = mid[:2]
    tracks[:, 0, 2] = 0.4
    tracks[:, 1, 0] = states[len(states) // 3, 0]
    tracks[:, 1, 1] = states[len(states) // 3, 1] + 0.2 * (np.arange(L) - 40)
    tracks[:, 1, 2] = np.pi / 2
    extents = np.array([[3.0, 1.0], [2.0, 0.5]])
    st, first, dwell = eng.tree_clear_rects(tracks, extents, 3, per_node=True)
    lo, hi = rr.goal_box(s)
    ref = cr.clear_rects(before[0], before[2], before[3], before[4], cr.row_test_of(s), tracks, extents, 3, lo, hi)
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


def _reference_of(s, p, tracks, extents, start=0):
    state, _, pID, elen, xedge, _ = rr.engine_arrays(p._engine)
    lo, hi = rr.goal_box(s)
    table, extents, start = p._engine.rect_table(tracks, extents, start)
    return cr.clear_rects(state, pID, elen, xedge, cr.row_test_of(s), table, extents, start, lo, hi)


def _plan_tracks(p):
    """Two rectangles on the plan as it stands: one crosses it at 75 % of its rows when the vehicle is there, heading along its
    motion, one parks on its end 20 rows after the vehicle has arrived."""
    rows = np.asarray(p.x_seq, dtype=np.float64)
    P = len(rows)
    L, c = P + 60, (75 * P) // 100
    t = np.arange(L, dtype=np.float64)
    tracks = np.zeros((L, 2, 3))
    tracks[:, 0, 0] = rows[c, 0] + 0.05 * (t - c)
    tracks[:, 0, 1] = rows[c, 1] + 0.5 * (t - c)
    tracks[:, 0, 2] = np.arctan2(0.5, 0.05)
    tracks[:, 1, :2] = (900.0, 900.0)
    tracks[P + 20:, 1, :2] = rows[-1, :2]
    tracks[:, 1, 2] = 0.3
    return tracks, np.array([[1.2, 0.4], [0.6, 0.4]])


def test_avoid_rects_adopts_the_references_best_and_reports_the_plans_first_conflict():
    s, p = _car_planner(1, 2000)
    assert p.plan_reached_goal and p.tree.size == 2001
    old_seq, old_x, old_T = list(p.node_seq), np.array(p.x_seq), p.T
    tracks, extents = _plan_tracks(p)
    ref = _reference_of(s, p, tracks, extents)
    print(ref["stats"])
    end = old_seq[-1]
    assert ref["stats"]["best_end"] not in (-1, end) and ref["first"][end] >= 0    # (of the inputs: the plan is hit, another one is clear)
    want_first = min(int(ref["first"][end]), int(ref["dwell_first"][end]) if ref["dwell_first"][end] >= 0 else 2 ** 31) * p.dt
    # adopt=False: the answer, and nothing else
    out = p.avoid_rects(tracks, extents, adopt=False)
    assert {k: out[k] for k in cl.STAT_KEYS} == ref["stats"] and out["plan_first"] == want_first
    assert list(p.node_seq) == old_seq and np.array_equal(np.array(p.x_seq), old_x) and p.T == old_T
    # adopt
    out = p.avoid_rects(tracks, extents)
    best = ref["stats"]["best_end"]
    assert {k: out[k] for k in cl.STAT_KEYS} == ref["stats"] and out["plan_first"] == want_first
    assert p.node_seq == p._engine.climb(best) and p.node_seq[-1] == best and p.plan_reached_goal
    assert len(p.x_seq) == ref["stats"]["best_steps"] == len(p.u_seq) == len(p.t_seq) and p.T == len(p.x_seq) * p.dt
    # the adopted plan is clear, and so says the next call: plan_first of the held plan
    again = p.avoid_rects(tracks, extents)
    assert again["plan_first"] is None and again["best_end"] == best and p.node_seq[-1] == best
    # ... checked row by row with the plain model
    test = cr.row_test_of(s)
    X = np.asarray(p.x_seq, dtype=np.float64)
    c_, s_ = fr.portable_sincos(X[:, 2])
    table = cr.rect_table(tracks, extents)
    assert test(X, c_, s_, table[np.minimum(np.arange(len(X)), len(table) - 1)]).all()
    wait = np.arange(len(X), len(table))
    assert test(np.repeat(X[-1:], len(wait), axis=0), np.repeat(c_[-1], len(wait)), np.repeat(s_[-1], len(wait)), table[wait]).all()


def test_deconflict_with_extents_is_the_loop_of_reference_calls_in_its_order():
    import lqrrt_amd as lqrrt
    made = [_car_planner(seed, 700, small_hull=True, x0=x0) for seed, x0 in ((2, (0.0, 0.0)), (3, (0.0, 30.0)), (4, (30.0, 0.0)))]
    systems, planners = [m[0] for m in made], [m[1] for m in made]
    order, extents = [1, 2, 0], np.array([[1.6, 0.5], [1.2, 0.4], [1.4, 0.6]])
    plans = [np.asarray(p.x_seq, dtype=np.float64)[:, :3].copy() for p in planners]
    ends = [p.node_seq[-1] for p in planners]
    want = [None] * 3
    for at, k in enumerate(order):
        if at == 0:
            continue
        before = order[:at]
        ref = _reference_of(systems[k], planners[k], [plans[j] for j in before], extents[before])
        want[k] = ref["stats"]
        if ref["stats"]["best_end"] >= 0:
            state, _, pID, elen, xedge, _ = rr.engine_arrays(planners[k]._engine)
            chain = planners[k]._engine.climb(ref["stats"]["best_end"])
            plans[k] = np.concatenate([xedge[v, :elen[v]] for v in chain])[:, :3]
            ends[k] = ref["stats"]["best_end"]
    got = lqrrt.deconflict(planners, None, order=order, extents=extents)
    print(want, [None if g is None else g["plan_first"] for g in got])
    assert got[1] is None
    assert any(want[k]["best_end"] >= 0 for k in (2, 0)) and any(want[k]["conflicts"] > 0 for k in (2, 0))      # (of the inputs)
    for k in (2, 0):
        assert {key: got[k][key] for key in cl.STAT_KEYS} == want[k]
    for k in range(3):
        assert planners[k].node_seq[-1] == ends[k]
        np.testing.assert_array_equal(np.asarray(planners[k].x_seq, dtype=np.float64)[:, :3], plans[k])


def _channel_planner(tree, system="boat_intermediate"):
    """A planner that holds `tree` (a HandTree) on the device and, as its plan, the tree's best goal hit."""
    import lqrrt_amd as lqrrt
    s = cl.Case("channel", tree, np.zeros((1, 1, 2)), 0.0).native()
    cons = lqrrt.Constraints(s.nstates, s.ncontrols, s.goal_buffer, s.is_feasible)
    p = lqrrt.Planner(s.dynamics, s.lqr, cons, error_tol=s.error_tol, erf=s.erf, goal0=s.goal, printing=False, horizon=cl.H_HAND * 0.1, dt=0.1)
    return s, p


def test_channel_scene_rectangles_pass_where_covering_discs_do_not():
    """Two 6 m x 0.4 m vessels meet in a channel, each keeping 0.6 m to its side of the centre line, with a long way round in each
    tree.  As covering discs (radius 3.007 m) the second one finds no clear plan or must go round; as rectangles they pass."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("fleet_channel_gpu", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                  "examples", "fleet_channel_gpu.py"))
    scene = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(scene)
    discs, rects = scene.run(printing=False)
    print(discs, rects)
    assert rects["best_end"] >= 0 and rects["best_steps"] == scene.SHORT_STEPS
    assert discs["best_end"] == -1 or discs["best_steps"] > rects["best_steps"]
