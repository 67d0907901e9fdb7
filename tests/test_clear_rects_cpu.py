"""
The clearance query against moving oriented rectangles (Planner.avoid_rects / Engine.tree_clear_rects, csrc/clear_rects.hpp) on the
CPU: the reference of the rule (tests/clear_rects_reference.py) on the fork against hand-computed answers, its point test against an
independent statement of it, every input of tests/test_clear_rects_gpu.py shown not to be degenerate with the reference alone, the
host side of the public calls and their refusals, the ABI's declaration, and what the sources and the compiler say about the kernel.
"""
import os
import re
import shutil
import sys

import numpy as np
import pytest

import lqrrt_amd
from lqrrt_amd import _native as nat
from lqrrt_amd.engine import Engine
import clear_reference as cl
import clear_rects_reference as cr
from clear_common import FORBIDDEN
import feasibility_reference as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The fork (clear_reference.fork_nodes): cum by hand -- the short branch 1 + 5 + 5 = 11 (node 2), 6 below it 14, 9 and 10 below that
# 15; the long branch 6, 11, 16 (node 5); the twig 8, 9.
FORK_CUM = [1, 6, 11, 6, 11, 16, 14, 8, 9, 15, 15]
# (own_first, first, dwell_first, best_end, best_steps), worked out by hand.  The hull is 1.0 x 0.5 m around the pose (x +- 0.5,
# y +- 0.25).  The crossing rectangle is a square of half side 0.4 at (7, tau - 7): at tau = 7 it covers x 6.6 .. 7.4, y -0.4 .. 0.4
# and holds the hull points of the vehicle at (7, 0) (row 1 of node 2, tau = 6 + 1); at tau = 6 it covers y -1.4 .. -0.6, below the
# hull of the vehicle at (6, 0), and at tau = 8 the vehicle at (8, 0) begins at x = 7.5, beyond 7.4.  The parked rectangle at (11, 0)
# covers x 10.65 .. 11.35, y -0.2 .. 0.2: the bow of node 6's first row (10.1 + 0.5) stays short of it, that of its second row
# (10.7) is inside at tau = 11 + 1 = 12; node 9 (bow 10.85) in its only row at 14; both again the instant after they arrive
# (14, 15).  Nodes 2 and 5 end with their bows at 10.5.
PINNED = {
    "fork, the rectangle crosses the short branch":
        ([-1, -1, 7, -1, -1, -1, 12, -1, -1, 14, -1], [-1, -1, 7, -1, -1, -1, 7, -1, -1, 7, 7],
         [-2, -2, -1, -2, -2, -1, 14, -2, -2, 15, -2], 5, 16),
    # start = 4: every row 4 later; at tau = 11 the square is at (7, 4), long past the short branch
    "fork, the rectangle has passed (start = 4)":
        ([-1, -1, -1, -1, -1, -1, 16, -1, -1, 18, -1], [-1, -1, -1, -1, -1, -1, 16, -1, -1, 16, 16],
         [-2, -2, -1, -2, -2, -1, 18, -2, -2, 19, -2], 2, 11),
    # L = 14: the square jumps to (10, -0.6) in the last row and covers y -1.0 .. -0.2: the hull of a vehicle parked at (10, 0)
    # reaches down to -0.25 (node 2, arrived at 10: dwell conflict at 13 = L - 1), that of one at (10, 0.2) to -0.05 (node 5, which
    # arrives at 15 >= L - 1 anyway); nodes 6 and 9 arrive at 13 and 14: nothing left to wait against
    "fork, dwell conflict at L - 1, the long branch arrives later":
        ([-1, -1, -1, -1, -1, -1, 12, -1, -1, 14, -1], [-1, -1, -1, -1, -1, -1, 12, -1, -1, 12, 12],
         [-2, -2, 13, -2, -2, -1, -1, -2, -2, -1, -2], 5, 16),
    # L = 7: the track ends at (7, -1); at tau = 7 = L the square is still there, y -1.4 .. -0.6
    "fork, L = 7: the rectangle stops short, tau = L is clamped":
        ([-1, -1, -1, -1, -1, -1, 12, -1, -1, 14, -1], [-1, -1, -1, -1, -1, -1, 12, -1, -1, 12, 12],
         [-2, -2, -1, -2, -2, -1, -1, -2, -2, -1, -2], 2, 11),
    # start = 8 = L: every row sees the last row of the tracks, the square parked at (7, 0)
    "fork, start >= L":
        ([-1, -1, 15, -1, -1, -1, 20, -1, -1, 22, -1], [-1, -1, 15, -1, -1, -1, 15, -1, -1, 15, 15],
         [-2, -2, -1, -2, -2, -1, -1, -2, -2, -1, -2], 5, 16),
    # the 6 x 0.4 m rectangle comes down y = 0.6 and covers y 0.4 .. 0.8, beside the hull (y <= 0.25) of the short branch: only the
    # parked one matters
    "fork, a 6 x 0.4 rectangle passes beside the short branch":
        ([-1, -1, -1, -1, -1, -1, 12, -1, -1, 14, -1], [-1, -1, -1, -1, -1, -1, 12, -1, -1, 12, 12],
         [-2, -2, -1, -2, -2, -1, 14, -2, -2, 15, -2], 2, 11),
    # ... turned by pi/2 it covers x +- 0.2 about 14 - tau and y -2.4 .. 3.6: at tau = 7 it is at x = 7, as the vehicle
    "fork, the same track, heading pi/2":
        ([-1, -1, 7, -1, -1, -1, 12, -1, -1, 14, -1], [-1, -1, 7, -1, -1, -1, 7, -1, -1, 7, 7],
         [-2, -2, -1, -2, -2, -1, 14, -2, -2, 15, -2], 5, 16),
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_reference_gives_the_hand_computed_answers(name):
    own, first, dwell, best_end, best_steps = PINNED[name]
    r = cr.case(name).reference()
    print(name, r["stats"])
    assert r["cum"].tolist() == FORK_CUM
    assert r["own_first"].tolist() == own and r["first"].tolist() == first and r["dwell_first"].tolist() == dwell
    hits = [2, 5, 6, 9]
    assert np.flatnonzero(r["hit"]).tolist() == hits
    clear_hits = [i for i in hits if first[i] == -1 and dwell[i] == -1]
    assert r["stats"] == dict(size=11, conflicts=sum(v >= 0 for v in own), blocked=sum(o == -1 and f >= 0 for o, f in zip(own, first)),
                              hits=4, clear_hits=len(clear_hits), best_end=best_end, best_steps=best_steps)
    assert best_end in clear_hits and best_steps == FORK_CUM[best_end]


def test_what_a_disc_cannot_say():
    """Of the inputs, with the two references alone: the rectangle leaves the short branch clear, the disc that covers it does not."""
    c = cr.case("fork, a 6 x 0.4 rectangle passes beside the short branch")
    assert c.extents[-1].tolist() == [3.0, 0.2] and c.radii[-1] == np.sqrt(3.0 ** 2 + 0.2 ** 2)
    rect, disc = c.reference()["stats"], c.disc_reference()["stats"]
    assert (rect["best_end"], rect["best_steps"]) == (2, 11) and disc["best_end"] != 2 and c.disc_reference()["first"][2] >= 0
    turned = cr.case("fork, the same track, heading pi/2")
    assert np.array_equal(turned.tracks[:, :, :2], c.tracks[:, :, :2]) and np.array_equal(turned.extents, c.extents)
    assert turned.reference()["own_first"][2] == 7


def test_point_test_against_an_independent_statement():
    """Axis-aligned rectangles are interval tests; arbitrary ones: rotate the point into the rectangle's frame with numpy."""
    rs = np.random.RandomState(11)
    R, P, D = 300, 7, 5
    pts = rs.uniform(-3, 3, (R, P, 2))
    centre = rs.uniform(-3, 3, (R, D, 2))
    ext = rs.uniform(0.0, 1.5, (R, D, 2))
    # heading 0: co = 1, so = 0 exactly
    c0, s0 = fr.portable_sincos(np.zeros(R * D))
    assert np.all(c0 == 1.0) and np.all(s0 == 0.0)
    rects = np.concatenate((centre, np.ones((R, D, 1)), np.zeros((R, D, 1)), ext), axis=2)
    want = np.zeros(R, dtype=bool)
    for r in range(R):
        for d in range(D):
            lo, hi = centre[r, d] - ext[r, d], centre[r, d] + ext[r, d]
            for p in pts[r]:
                # (|p - c| <= e is c - e <= p <= c + e up to the rounding of c +- e: random points do not sit on an edge)
                want[r] |= bool(lo[0] <= p[0] <= hi[0] and lo[1] <= p[1] <= hi[1])
    got = cr.rects_hit(pts, rects)
    assert np.array_equal(got, want) and 0 < want.sum() < R
    # arbitrary headings: p' = R(h)^T (p - c) with a 2 x 2 matrix of the portable cos / sin
    h = rs.uniform(-np.pi, np.pi, (R, D))
    co, so = (v.reshape(R, D) for v in fr.portable_sincos(h.reshape(-1)))
    rects = np.concatenate((centre, co[:, :, None], so[:, :, None], ext), axis=2)
    want = np.zeros(R, dtype=bool)
    slack = 0
    for r in range(R):
        for d in range(D):
            rot = np.array([[co[r, d], so[r, d]], [-so[r, d], co[r, d]]])
            q = (rot @ (pts[r] - centre[r, d]).T).T
            inside = np.all(np.abs(q) <= ext[r, d], axis=1)
            slack += int(np.sum(np.abs(np.abs(q) - ext[r, d]) < 1e-12))
            want[r] |= bool(inside.any())
    assert slack == 0                                                 # (no point within rounding of an edge: the two agree exactly)
    assert np.array_equal(cr.rects_hit(pts, rects), want) and 0 < want.sum() < R
    # the edge is inside, one ulp beyond it is not; a = b = 0 holds its own centre
    edge = np.array([[[1.0, 0.5]]])
    assert cr.rects_hit(edge, np.array([[[0.0, 0.0, 1.0, 0.0, 1.0, 0.5]]]))[0]
    assert not cr.rects_hit(edge, np.array([[[0.0, 0.0, 1.0, 0.0, np.nextafter(1.0, 0.0), 0.5]]]))[0]
    assert not cr.rects_hit(edge, np.array([[[0.0, 0.0, 1.0, 0.0, 1.0, np.nextafter(0.5, 0.0)]]]))[0]
    assert cr.rects_hit(edge, np.array([[[1.0, 0.5, 0.6, 0.8, 0.0, 0.0]]]))[0]


def test_row_test_places_the_hull_as_the_plain_model_and_inflates_for_the_novice():
    rs = np.random.RandomState(3)
    vps = fr.lattice_hull(1.0, 0.5, 0.25)
    R, D = 100, 4
    X = np.zeros((R, 6))
    X[:, :2] = rs.uniform(-3, 3, (R, 2))
    X[:, 2] = rs.uniform(-np.pi, np.pi, R)
    X[:, 3:] = 9.0                                                     # far outside any speed box: not looked at
    c, s = fr.portable_sincos(X[:, 2])
    table = cr.rect_table(np.concatenate((rs.uniform(-3, 3, (R, D, 2)), rs.uniform(-3, 3, (R, D, 1))), axis=2), rs.uniform(0, 1, (D, 2)))
    hull = cr.row_test("hull", vps)(X, c, s, table)
    nov = cr.row_test("novice", half_length=fr.HALF_LENGTH)(X, c, s, table)
    grown = table.copy()
    grown[:, :, 4:] = table[:, :, 4:] + fr.HALF_LENGTH
    for k in range(R):
        verts = fr.vertices(vps, X[k], c[k], s[k])
        assert hull[k] == (not cr.rects_hit(verts[None], table[k:k + 1])[0])
        assert nov[k] == (not cr.rects_hit(X[k:k + 1, None, :2], grown[k:k + 1])[0])
    assert 0 < hull.sum() < R and 0 < nov.sum() < R


@pytest.mark.parametrize("case", cr.cases(), ids=lambda c: c.name)
def test_no_gpu_case_is_degenerate(case):
    """A condition on the INPUTS, shown with the reference alone: every case has a conflicting node, a blocked node, a clear hit and
    a hit that is not clear -- unless it exists to show 'none'."""
    r = case.reference()
    print(case.name, r["stats"])
    if case.none:
        assert cl.degenerate(r), "marked as a none-case, but it is not"
        assert r["stats"]["clear_hits"] == 0
    else:
        assert cl.degenerate(r) == []
    L = len(case.tracks)
    assert case.tracks.shape == (L, len(case.extents), 3) and case.extents.shape[1] == 2 and 11 <= case.tree.size <= 257


def test_the_edge_cases_are_what_their_names_say():
    by = {c.name: c for c in cr.cases()}
    # the edge: with the exact extent node 2 conflicts at tau = 7, one ulp less and its whole edge is clear
    for on, off, col in (("edge: a hull point on |xi| == a", "edge: |xi| one ulp beyond a", 0),
                         ("edge: a hull point on |eta| == b", "edge: |eta| one ulp beyond b", 1)):
        a, b = by[on], by[off]
        assert np.array_equal(a.tracks, b.tracks) and b.extents[-1, col] == np.nextafter(a.extents[-1, col], 0.0)
        assert a.extents[-1, 1 - col] == b.extents[-1, 1 - col] and np.all(a.tracks[:, :, 2] == 0.0)
        assert a.reference()["own_first"][2] == 7 and b.reference()["own_first"][2] == -1
        assert a.reference()["stats"]["best_end"] == 5 and b.reference()["stats"]["best_end"] == 2
    z = by["zero extents on a hull point"]
    assert z.extents[-1].tolist() == [0.0, 0.0] and z.reference()["own_first"][2] == 7
    verts = fr.vertices(z.vps(), np.array([7.0, 0.0]), 1.0, 0.0)
    assert any(np.array_equal(v, z.tracks[7, -1, :2]) for v in verts)
    # lane tiles: the crossing rectangle is the last of its table (lane 63 of the first cull tile, lane 0 of the second), or the first,
    # and without it nothing conflicts
    for name, where, D in (("fork, D = 64, the crossing rectangle last", 63, 64), ("fork, D = 65, the crossing rectangle last", 64, 65),
                           ("fork, D = 65, the crossing rectangle first", 0, 65)):
        c = by[name]
        assert c.tracks.shape[1] == D and np.array_equal(c.tracks[:, where, :2], cl.crossing(len(c.tracks)))
        others = np.delete(np.arange(D), where)
        t = c.tree
        lo, hi = t.box()
        rest = cr.clear_rects(t.state, t.pID, t.elen, t.xedge, c.test(), c.tracks[:, others], c.extents[others], 0, lo, hi)
        assert rest["stats"]["conflicts"] == 0
    assert by["boat_novice, D = 65: one point, inflated extents"].tracks.shape[1] == 65
    big = by["ros_boat on an occupied grid, 3073 hull points, D = 65"]
    assert big.grid and big.vps().shape == (2, 3073) and 2 * 3073 * 8 > fr.OG_LDS_BYTES and big.tracks.shape[1] == 65
    assert by["boat_intermediate: the fork"].vps().shape == (2, 15)
    # time edges
    assert len(by["fork, L = 1: the square stands on the short branch"].tracks) == 1
    c = by["fork, start >= L"]
    assert c.start >= len(c.tracks)
    c = by["fork, L = 8: the crossing is the last row (tau = L - 1)"]
    assert c.reference()["own_first"][2] == len(c.tracks) - 1
    c = by["fork, dwell conflict at L - 1, the long branch arrives later"]
    r = c.reference()
    assert r["dwell_first"][2] == len(c.tracks) - 1 and r["cum"][5] - 1 + c.start >= len(c.tracks) - 1 and r["dwell_first"][5] == -1
    # the chain of 2^8 nodes: the conflict is the root's
    r = by["chain of 256, conflict on the root"].reference()
    assert r["own_first"].tolist() == [0] + [-1] * 255 and r["first"].tolist() == [0] * 256
    # the car's vertex at 2p lies in a rectangle and nothing comes of it; the disc rule of the same model does fail that row
    c = by["car: a rectangle over the 2p vertex of node 7's last row"]
    p2 = 2.0 * c.tree.xedge[7, 1, :2]
    assert np.all(np.abs(p2 - c.tracks[7, 0, :2]) <= c.extents[0]) and c.tracks[7, 0, 2] == 0.0
    assert c.reference()["own_first"][7] == -1 and c.disc_reference()["own_first"][7] == 7
    # a row outside BoatAdvanced's planning speed box is not failed; the disc rule fails it
    c = by["boat_advanced: a row outside the planning speed box"]
    assert c.tree.xedge[4, 2, 3] > fr.PLAN_BOX[0][0] and c.reference()["own_first"][4] == -1 and c.reference()["stats"]["best_end"] == 5
    assert c.disc_reference()["own_first"][4] == 6 + 2
    # general position: headings of rows and rectangles are all over the circle, every instant has poses of its own
    c = by["general position: assorted headings, 8 rectangles"]
    assert c.tracks.shape[1] == 8 and len(np.unique(c.tracks[:, :, 2])) == c.tracks.shape[0] * 8
    assert len(np.unique(np.round(c.tree.xedge[:, :, 2], 6))) > 100


@pytest.mark.parametrize("name", ["car_2000", "boat_advanced_3000"])
def test_fixture_inputs_are_not_degenerate(name):
    r = cr.fixture_reference(name)
    f = cl.fixture(name)
    print(name, r["stats"])
    assert cl.degenerate(r) == []
    end = f.plan[-1]
    assert r["hit"][end] and r["first"][end] >= 0                                 # the rectangles stand on the fixture's own plan
    tracks, extents = cr.fixture_tracks(f)
    assert tracks.shape == (len(f.plan_rows()) + 60, 4, 3) and extents.shape == (4, 2) and r["stats"]["best_end"] != end
    moving = np.diff(tracks[:2, [0, 2], :2], axis=0)[0]
    np.testing.assert_allclose(np.arctan2(moving[:, 1], moving[:, 0]), tracks[0, [0, 2], 2])       # headings along their motion


# ------------------------------------------------------------------------------------------------ the host side

def _native_planner(dt=None):
    car = lqrrt_amd.systems.Car(0)
    cons = lqrrt_amd.Constraints(car.nstates, car.ncontrols, car.goal_buffer, car.is_feasible)
    kw = dict(car.plan_kwargs)
    if dt is not None:
        kw["dt"] = dt
    return car, lqrrt_amd.Planner(car.dynamics, car.lqr, cons, error_tol=car.error_tol, erf=car.erf, goal0=car.goal, printing=False, **kw)


E = (1.0, 0.5)
BAD_TRACKS = [dict(tracks=np.zeros((0, 1, 3)), extents=E),                       # L = 0
              dict(tracks=np.zeros((3, 0, 3)), extents=E),                       # D = 0
              dict(tracks=np.zeros((3, 2, 2)), extents=E),                       # no heading
              dict(tracks=np.zeros((3, 3)), extents=E),
              dict(tracks=[], extents=E),
              dict(tracks=[np.zeros((0, 3))], extents=E),
              dict(tracks=[np.zeros((4, 2))], extents=E),
              dict(tracks=np.zeros((3, 2, 3)), extents=E, start=-1),
              dict(tracks=np.zeros((3, 2, 3)), extents=E, start=1.5),
              dict(tracks=np.full((3, 2, 3), np.nan), extents=E),
              dict(tracks=np.array([[[0.0, 0.0, np.inf]]]), extents=E),          # the heading
              dict(tracks=np.zeros((3, 2, 3)), extents=(1.0, -0.1)),
              dict(tracks=np.zeros((3, 2, 3)), extents=[[1.0, 0.5], [np.nan, 0.5]]),
              dict(tracks=np.zeros((3, 2, 3)), extents=(np.inf, 0.5)),
              dict(tracks=np.zeros((3, 2, 3)), extents=0.5),
              dict(tracks=np.zeros((3, 2, 3)), extents=[[1.0, 0.5]] * 3)]


@pytest.mark.parametrize("bad", BAD_TRACKS, ids=lambda b: "%s e=%s start=%s" % (np.shape(b["tracks"]), b["extents"], b.get("start", 0)))
def test_refusals(bad):
    """Every argument is checked on the host before anything else is looked at: also without a tree, also without a device."""
    with pytest.raises(ValueError):
        Engine.rect_table(**bad)
    car, p = _native_planner()
    with pytest.raises(ValueError):
        p.avoid_rects(**bad)
    assert p.tree is None and not p.plan_reached_goal


def test_rect_table_pads_by_holding_the_last_row():
    a, b = np.arange(12.0).reshape(4, 3), np.array([[9.0, 9.5, 0.25]])
    table, ext, start = Engine.rect_table([a, b], (1.0, 0.5), 2)
    assert table.shape == (4, 2, 3) and start == 2 and ext.tolist() == [[1.0, 0.5], [1.0, 0.5]]
    assert np.array_equal(table[:, 0], a) and np.array_equal(table[:, 1], np.tile(b, (4, 1)))
    t2, e2, _ = Engine.rect_table(table, [[0.0, 1.0], [2.0, 0.0]])
    assert np.array_equal(t2, table) and e2.tolist() == [[0.0, 1.0], [2.0, 0.0]] and t2.flags["C_CONTIGUOUS"] and e2.flags["C_CONTIGUOUS"]


def test_without_a_plan_nothing_happens():
    car, p = _native_planner()
    assert p.avoid_rects(np.zeros((3, 1, 3)), E) is None
    assert p.avoid_rects([np.zeros((3, 3))], [E], start=2, adopt=False) is None
    assert p.tree is None and not hasattr(p, "node_seq") and not p.plan_reached_goal


def test_callback_mode_is_refused():
    cons = lqrrt_amd.Constraints(2, 1, [0.1, 0.1], lambda x, u: True)
    p = lqrrt_amd.Planner(lambda x, u, dt: x + dt * np.array([x[1], u[0]]), lambda x, u: (np.eye(2), np.array([[1.0, 1.0]])), cons,
                          horizon=1, dt=0.1, goal0=[1.0, 0.0], printing=False)
    assert p.callback_mode
    with pytest.raises(NotImplementedError, match="Python"):
        p.avoid_rects(np.zeros((3, 1, 3)), E)
    with pytest.raises(NotImplementedError, match="Python"):
        lqrrt_amd.deconflict([p], None, extents=E)


def test_deconflict_extents_refusals():
    (_, a), (_, b) = _native_planner(), _native_planner()
    with pytest.raises(ValueError, match="radii must be None"):
        lqrrt_amd.deconflict([a, b], 0.5, extents=E)
    for bad in (0.5, [E], [E, E, E], (1.0, -0.5), (np.nan, 0.5), (np.inf, 0.5)):
        with pytest.raises(ValueError, match="extent"):
            lqrrt_amd.deconflict([a, b], None, extents=bad)
    for kw in (dict(max_wait=1), dict(batched=True), dict(connect=2)):
        with pytest.raises(ValueError, match="not covered"):
            lqrrt_amd.deconflict([a, b], None, extents=E, **kw)
    with pytest.raises(ValueError, match="permutation"):
        lqrrt_amd.deconflict([a, b], None, order=[0, 0], extents=E)
    with pytest.raises(ValueError, match="no plan"):
        lqrrt_amd.deconflict([a, b], None, extents=[E, (2.0, 0.1)])
    # without extents nothing changes: radii are still asked for
    with pytest.raises((ValueError, TypeError)):
        lqrrt_amd.deconflict([a, b], None)
    assert "avoid_rects" in lqrrt_amd.Planner.avoid.__doc__ and "extents" in lqrrt_amd.deconflict.__doc__


# ------------------------------------------------------------------------------------------------ ABI and sources

def test_header_declares_the_call_and_states_the_rule():
    import ctypes as C
    text = open(os.path.join(ROOT, "include", "lqrrt_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint lqrrt_tree_clear_rects\s*\((.*?)\);", code, re.S)
    assert m and len(m.group(1).split(",")) == 10 and "lqrrt_clear_stats* out" in m.group(1) and "extents_host" in m.group(1)
    comment = text[text.index("/* lqrrt_tree_clear against D oriented RECTANGLES"):text.index("int lqrrt_tree_clear_rects(")]
    for words in ("xi = co*dx + so*dy", "eta = co*dy + (-so)*dx", "fabs(xi) <= a'", "lq_sincos", "params[18]", "2p", "speed box",
                  "no occupancy grid", "min(tau, L - 1)"):
        assert words in comment, words
    I, P = C.c_int, C.c_void_p
    assert nat.SIGNATURES["lqrrt_tree_clear_rects"] == (I, [P, P, P, I, I, I, C.POINTER(nat.ClearStats), P, P, P])
    assert hasattr(nat.lib(), "lqrrt_tree_clear_rects") and nat.lib().lqrrt_abi_version() == 1
    assert C.sizeof(nat.ClearStats) == 6 * 4 + 8 and [f[0] for f in nat.ClearStats._fields_] == list(cl.STAT_KEYS)
    assert callable(Engine.tree_clear_rects) and callable(Engine.rect_table) and callable(lqrrt_amd.Planner.avoid_rects)
    doc = cr.__doc__
    for words in ("2p", "speed box", "no occupancy grid", "portable_sincos", "half the boat length"):
        assert words in doc, words


def test_the_fragments_stay_plain_launches_on_the_existing_host_path():
    csrc = os.path.join(ROOT, "lqrrt_amd", "csrc")
    kern, host = (open(os.path.join(csrc, f)).read() for f in ("clear_rects.hpp", "engine_clear_rects.hpp"))
    for text in (kern, host):
        for word in FORBIDDEN:
            assert word not in text, word
        assert "dalloc(" not in text and "__shared__ int" not in text
    assert kern.count("__launch_bounds__(64)") == 1 and "k_clear_rects_check" in kern
    for reused in ("clear_stage_hull(", "clear_load_row<S>(", "goal_hit<S>(", "link[tv.pID[i]].steps", "lane_read(", "__ballot("):
        assert reused in kern, reused
    assert "S::feasible(" not in kern and "stage_geo(" not in kern
    # the traits, the run, the order of the refusals; nothing is allocated or enqueued by the fragment itself but the check's launch
    assert "clear_run<ClearRects>(" in host and "ClearPlain::select(" in host and "ClearPlain::stats(" in host and "NOT_GENERIC(e);" in host
    assert host.count("hipLaunchKernelGGL(") == 1 and "hipMemcpy" not in host and "hipMalloc" not in host
    assert "k_clear_rects_check<S>), dim3((unsigned)N), dim3(64), hull_bytes, st" in host
    check = host[host.index("static int clear_rects_check("):host.index('extern "C" int lqrrt_tree_clear_rects(')]
    order = [check.index(r) for r in ("null argument", "L < 1 || D < 1", "start < 0", "track table too large", "std::isfinite(tracks_host[q])",
                                      "extents_host[d] >= 0.0", "has_discs<S>::value", "!e->has_res", "!e->has_goal",
                                      "the root's edge has no row", "p < 0 || p >= v", "leave 31 bits", "> e->lds_limit", "table.resize(")]
    assert order == sorted(order)
    export = host[host.index('extern "C" int lqrrt_tree_clear_rects('):]
    assert export.index("TRY(clear_rects_check(") < export.index("clear_run<ClearRects>(")
    systems = open(os.path.join(csrc, "systems.hpp")).read()
    assert systems.count("static constexpr bool DISCS = true;") == 2
    kernels = open(os.path.join(csrc, "kernels.hpp")).read()
    for before in ('#include "clear.hpp"', '#include "clear_wait.hpp"', '#include "clear_multi.hpp"', '#include "clear_connect.hpp"'):
        assert kernels.index(before) < kernels.index('#include "clear_rects.hpp"')
    engine = open(os.path.join(csrc, "engine.hip")).read()
    assert engine.index('#include "engine_clear.hpp"') < engine.index('#include "engine_clear_rects.hpp"')


def test_check_kernel_has_no_private_segment_and_no_static_lds():
    """k_clear_rects_check<S> exists for exactly the models k_clear_check<S> exists for; its private segment is 0 bytes and its LDS
    is the launch's alone (the hull points)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    assert shutil.which(kr.HIPCC) or os.path.exists(kr.HIPCC), "hipcc is what builds the package: it cannot be missing here"
    user = os.path.join(ROOT, "examples", "user_system", "unicycle.hpp")
    rows = kr.parse(kr.remarks(["-DLQRRT_USER_SYSTEM=\"%s\"" % user]))

    def by_model(kernel):
        out = {}
        for r in rows:
            m = re.match(r"void lq::%s<lq::(.+?) ?>\(" % kernel, r["name"])
            if m:
                out[m.group(1)] = r
        return out
    clear, rects = by_model("k_clear_check"), by_model("k_clear_rects_check")
    assert sorted(rects) == sorted(clear) == ["BoatAdvanced", "BoatIntermediate", "BoatNovice", "BoatNoviceLqr", "Car", "RosBoat"]
    for model in sorted(rects):
        print("%-18s disc check %3d B occ %d vgpr %3d sgpr %3d   rect check %3d B occ %d vgpr %3d sgpr %3d" % (
            model, clear[model]["scratch"], clear[model]["occupancy"], clear[model]["vgpr"], clear[model].get("sgpr", -1),
            rects[model]["scratch"], rects[model]["occupancy"], rects[model]["vgpr"], rects[model].get("sgpr", -1)))
        assert rects[model]["scratch"] == 0 and rects[model]["lds"] == 0
