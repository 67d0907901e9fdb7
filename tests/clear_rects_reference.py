"""
Reference of the clearance query against moving oriented rectangles (Engine.tree_clear_rects / Planner.avoid_rects,
csrc/clear_rects.hpp) in plain NumPy: one sequential pass.

The rule.  Items 1, 2, 4, 5 and 6 of tests/clear_reference.py hold word for word, with "disc" read as "rectangle": cum[0] = elen[0],
cum[i] = cum[pID[i]] + elen[i]; row k of node i > 0 has time index tau = start + cum[pID[i]] + k and the root's one row (its last)
tau = start; at tau the rectangles are at table row min(tau, L - 1); own_first[i] = the smallest tau of a failing row of node i's own
edge or -1, first[i] = the smallest own_first >= 0 from i up to and including the root or -1; for a goal hit (a non-root node
strictly inside the goal box) dwell_first[i] = the smallest tau' in (cum[i] - 1 + start, L - 1] at which its LAST row fails, or -1,
and -2 for every other node; best = the smallest (cum, id) among the hits with first == dwell_first == -1; the counters are the same.

Only the row test (item 3) is new.
  Input.  tracks[L][D][3] = world x, y and heading of rectangle d at each instant; extents[D][2] = (a, b), the half length along the
    heading and the half width, both >= 0.
  Table.  Per (instant, rectangle) co, so = portable_sincos(heading) -- the function the vehicle's own heading goes through.  For the
    novice boats a' = a + half the boat length, b' = b + half the boat length (what inflates their circles); for every other model
    a' = a, b' = b.
  Vehicle points.  The hull sweepers (BoatAdvanced, BoatIntermediate, RosBoat, Car): the hull points vps placed as
    feasibility_reference.vertices places them, vx = px + (c*bx + (-s)*by), vy = py + (s*bx + c*by).  The novice boats: the one
    point (px, py).
  Test.  dx = vx - ox; dy = vy - oy; xi = co*dx + so*dy; eta = co*dy + (-so)*dx; inside = (|xi| <= a') and (|eta| <= b'), in fp64,
    these operations in this order.  A row fails when some point is inside some rectangle of its instant.
  Left out on purpose.  The test is geometry only: no static map and no occupancy grid; the car's extra vertex at 2p is not used (it
    restates a quirk of the reference's circle test, and the reference has no rectangle); BoatAdvanced's planning speed box is not
    used (rows in a tree have passed it).
This reference culls nothing: every (point, rectangle) pair of a row is tested.

CASES: every hand-built input of tests/test_clear_rects_gpu.py, built once here and shared with tests/test_clear_rects_cpu.py, which
shows with this reference alone that none of them is degenerate.
"""
import functools

import numpy as np

import clear_reference as cl
import feasibility_reference as fr
from clear_reference import HandTree, fork_nodes, portable_sincos, degenerate, STAT_KEYS      # noqa: F401


# ------------------------------------------------------------------------------------------------ the row test

def rects_hit(points, rects):
    """points (R, P, 2), rects (R, D, 6) as [ox, oy, co, so, a', b'] -> (R,) bool: some point of row r lies inside some rectangle of
    row r, edge included."""
    with np.errstate(invalid="ignore", over="ignore"):
        dx = points[:, None, :, 0] - rects[:, :, None, 0]
        dy = points[:, None, :, 1] - rects[:, :, None, 1]
        co, so = rects[:, :, None, 2], rects[:, :, None, 3]
        xi = co * dx + so * dy
        eta = co * dy + (-so) * dx
        inside = (np.abs(xi) <= rects[:, :, None, 4]) & (np.abs(eta) <= rects[:, :, None, 5])
    return np.any(inside, axis=(1, 2))


def row_test(kind, vps=None, half_length=None):
    """The test of R rows: callable (X [R][n], c [R], s [R], rects [R][D][6]) -> (R,) bool, True = the row passes; row r is tested
    against rects[r] alone.  kind: 'hull' (every hull sweeper, the car and BoatAdvanced included: no 2p vertex, no speed box) or
    'novice' (the centre point against extents grown by half_length).  rects holds the extents as given: a, b."""
    if kind == "novice":
        hl = np.float64(half_length)

        def novice(X, c, s, rects):
            grown = rects.copy()
            grown[:, :, 4] = rects[:, :, 4] + hl
            grown[:, :, 5] = rects[:, :, 5] + hl
            return ~rects_hit(X[:, None, :2], grown)
        return novice
    assert kind == "hull"
    vps = np.asarray(vps, dtype=np.float64).reshape(2, -1)

    def hull(X, c, s, rects):
        c, s = np.asarray(c)[:, None], np.asarray(s)[:, None]
        vx = X[:, 0:1] + (c * vps[0] + (-s) * vps[1])              # feasibility_reference.vertices, row by row
        vy = X[:, 1:2] + (s * vps[0] + c * vps[1])
        return ~rects_hit(np.stack((vx, vy), axis=2), rects)
    return hull


def row_test_of(system):
    """row_test for an lqrrt_amd.systems object (its hull points and parameters as they are now)."""
    name = type(system).__name__
    if name in ("BoatNovice", "BoatNoviceLqr"):
        return row_test("novice", half_length=system.boat_length / 2)
    if name in ("BoatAdvanced", "BoatIntermediate", "RosBoat", "Car"):
        return row_test("hull", system.vps)
    raise ValueError("no rectangle path: %s" % name)


# ------------------------------------------------------------------------------------------------ the rule

def rect_table(tracks, extents):
    """tracks (L, D, 3), extents (D, 2) or (2,) -> [L][D][ox, oy, co, so, a, b]."""
    tracks = np.asarray(tracks, dtype=np.float64)
    L, D = tracks.shape[:2]
    assert tracks.shape == (L, D, 3) and L >= 1 and D >= 1
    extents = np.broadcast_to(np.asarray(extents, dtype=np.float64), (D, 2))
    co, so = (v.reshape(L, D) for v in portable_sincos(tracks[:, :, 2].reshape(-1)))      # (it takes a flat array)
    return np.concatenate((tracks[:, :, :2], co[:, :, None], so[:, :, None], np.broadcast_to(extents[None], (L, D, 2))), axis=2)


def clear_rects(state, pID, elen, xedge, test, tracks, extents, start, goal_lo, goal_hi, heading=2):
    """clear_reference.clear with the rectangles' table: state (N, n), pID (N,), elen (N,), xedge (N, H, n); test: row_test();
    tracks (L, D, 3), extents (D, 2) or (2,); start >= 0; goal_lo / goal_hi (n,).  Returns dict(cum, own_first, first, dwell_first,
    hit, stats)."""
    state, xedge = np.asarray(state, dtype=np.float64), np.asarray(xedge, dtype=np.float64)
    pID, elen = np.asarray(pID, dtype=np.int64), np.asarray(elen, dtype=np.int64)
    table = rect_table(tracks, extents)
    L = len(table)
    assert int(start) == start and start >= 0
    N = len(state)

    def rects_at(taus):
        return table[np.minimum(np.asarray(taus, dtype=np.int64), L - 1)]

    cum = np.zeros(N, dtype=np.int64)
    own = np.full(N, -1, dtype=np.int64)
    first = np.full(N, -1, dtype=np.int64)
    dwell = np.full(N, -2, dtype=np.int64)
    hit = np.zeros(N, dtype=bool)
    best = None
    for i in range(N):
        ln = int(elen[i])
        if i == 0:
            cum[0] = ln
            rows = [(ln - 1, start)]
        else:
            assert 0 <= pID[i] < i
            cum[i] = cum[pID[i]] + ln
            rows = [(k, start + int(cum[pID[i]]) + k) for k in range(ln)]
        c, s = portable_sincos(xedge[i, :ln, heading])
        ks = [k for k, _ in rows]
        ok = test(xedge[i, ks], c[ks], s[ks], rects_at([tau for _, tau in rows]))
        bad = np.flatnonzero(~ok)
        if len(bad):
            own[i] = rows[bad[0]][1]                                  # the first failing row of the edge, in order
        up = first[pID[i]] if i > 0 else -1
        first[i] = min([t for t in (own[i], up) if t >= 0], default=-1)
        hit[i] = i > 0 and bool(np.all((goal_lo < state[i]) & (state[i] < goal_hi)))
        if hit[i]:
            dwell[i] = -1
            taus = list(range(int(cum[i]) - 1 + start + 1, L))         # empty when the hit arrives at or after L - 1
            if taus:
                R = len(taus)
                ok = test(np.repeat(xedge[i, ln - 1:ln], R, axis=0), np.repeat(c[ln - 1], R), np.repeat(s[ln - 1], R), rects_at(taus))
                bad = np.flatnonzero(~ok)
                if len(bad):
                    dwell[i] = taus[bad[0]]
            if first[i] == -1 and dwell[i] == -1 and (best is None or (int(cum[i]), i) < best):
                best = (int(cum[i]), i)
    stats = dict(size=N, conflicts=int(np.sum(own >= 0)), blocked=int(np.sum((own == -1) & (first >= 0))), hits=int(np.sum(hit)),
                 clear_hits=int(np.sum(hit & (first == -1) & (dwell == -1))), best_end=-1 if best is None else best[1],
                 best_steps=-1 if best is None else best[0])
    return dict(cum=cum, own_first=own, first=first.astype(np.int32), dwell_first=dwell.astype(np.int32), hit=hit, stats=stats)


# ------------------------------------------------------------------------------------------------ hand-built cases

def with_heading(xy, heading):
    """(L, 2) centres -> (L, 3) with a constant heading."""
    xy = np.asarray(xy, dtype=np.float64)
    return np.column_stack((xy, np.full(len(xy), float(heading))))


def oncoming(L, x0=14.0, y=0.6, speed=1.0, heading=0.0):
    """A rectangle that comes down the line y = const from x0: at row t its centre is at (x0 - speed t, y)."""
    t = np.arange(L, dtype=np.float64)
    return with_heading(np.column_stack((x0 - speed * t, np.full(L, float(y)))), heading)


def only_at(L, row, x, y, heading=0.0):
    """Far away but for the one row `row`, where it is at (x, y)."""
    t = cl.parked(L, 50.0, 50.0)
    t[row] = (x, y)
    return with_heading(t, heading)


def far_rects(L, count):
    """count rectangles that stand far from everything: (L, count, 3), headings assorted."""
    out = np.zeros((L, count, 3))
    out[:, :, :2] = cl.far_discs(L, count)
    out[:, :, 2] = 0.37 * np.arange(count)
    return out


SQUARE, PARKED = (0.4, 0.4), (0.35, 0.2)                            # the crossing rectangle; the one parked beyond the goal at (11, 0)


class Case(cl.Case):
    """One (system, tree, tracks (L, D, 3), extents (D, 2), start); `none`: the case exists to show that nothing is clear."""

    def __init__(self, name, tree, tracks, extents, start=0, none=False, vps="small", grid=False):
        self.name, self.tree, self.start, self.none, self.vps_kind, self.grid = name, tree, int(start), none, vps, grid
        self.tracks = np.ascontiguousarray(tracks, dtype=np.float64)
        if self.tracks.ndim == 2:
            self.tracks = self.tracks[:, None, :]
        D = self.tracks.shape[1]
        self.extents = np.ascontiguousarray(np.broadcast_to(np.asarray(extents, dtype=np.float64), (D, 2)))
        self.radii = np.sqrt(np.sum(self.extents ** 2, axis=1))      # the discs that cover the rectangles

    def test(self):
        if self.tree.system == "boat_novice":
            return row_test("novice", half_length=fr.HALF_LENGTH)
        return row_test("hull", self.vps())

    @functools.lru_cache(maxsize=None)
    def reference(self):
        t = self.tree
        lo, hi = t.box()
        return clear_rects(t.state, t.pID, t.elen, t.xedge, self.test(), self.tracks, self.extents, self.start, lo, hi)

    @functools.lru_cache(maxsize=None)
    def disc_reference(self):
        """clear_reference's answer for the covering discs on the same centre tracks (the disc row test of the case's model)."""
        t = self.tree
        lo, hi = t.box()
        return cl.clear(t.state, t.pID, t.elen, t.xedge, cl.Case.test(self), self.tracks[:, :, :2], self.radii, self.start, lo, hi)


def _fork(name, system="boat_advanced", L=20, start=0, cross=None, e_cross=SQUARE, second=(11.0, 0.0), pad=0, cross_last=True, far=6.0,
          parked=True, **kw):
    """clear_reference's fork with rectangles: the crossing one (default: a square of half side 0.4 that moves up the line x = 7 and
    crosses y = 0 at row 7, heading along its motion), one parked beyond the goal that catches node 6 (unless parked=False), and
    `pad` far away."""
    cross = with_heading(cl.crossing(L), np.pi / 2) if cross is None else cross
    cols, ext = [], []
    if parked:
        cols.append(with_heading(cl.parked(L, *second), 0.0)[:, None, :])
        ext.append(PARKED)
    cols.append(far_rects(L, pad))
    ext += [(0.3, 0.1 + 0.01 * q) for q in range(pad)]
    if cross_last:
        cols.append(cross[:, None, :])
        ext.append(e_cross)
    else:
        cols.insert(0, cross[:, None, :])
        ext.insert(0, e_cross)
    return Case(name, HandTree(system, fork_nodes(far)), np.concatenate(cols, axis=1), np.array(ext, dtype=np.float64), start, **kw)


def _dwell_track(L):
    return with_heading(cl._dwell_track(L), 0.0)


def _novice_cross(L):
    """The crossing square for the novice boats, whose extents grow by 2.667 m: up the line x = 6, so that it stays more than that
    from the long branch (which goes round at y = 12)."""
    return with_heading(cl.crossing(L, x=6.0, at=6), np.pi / 2)


def _general_position(seed=5, N=48, L=40, D=8):
    """A hand tree whose rows have assorted headings, and D rectangles whose poses are drawn anew at every instant."""
    rs = np.random.RandomState(seed)
    nodes = [(-1, [(5.0, 5.0, 0.3)])]
    ends = [np.array([5.0, 5.0])]
    for i in range(1, N):
        p = int(rs.randint(0, i))
        rows, at = [], ends[p].copy()
        for _ in range(int(rs.randint(1, cl.H_HAND + 1))):
            at = np.clip(at + rs.uniform(-0.8, 0.8, 2), 0.0, 10.0)
            rows.append((at[0], at[1], rs.uniform(-np.pi, np.pi)))
        nodes.append((p, rows))
        ends.append(at)
    t = HandTree("boat_intermediate", nodes)
    t.goal[:2] = (5.0, 5.0)
    t.goal_buffer[:2] = 2.5
    at = np.arange(L, dtype=np.float64)[:, None, None]
    tracks = np.zeros((L, D, 3))                                     # every rectangle drifts and turns: a new pose at every instant
    tracks[:, :, :2] = rs.uniform(0.0, 10.0, (1, D, 2)) + at * rs.uniform(-0.3, 0.3, (1, D, 2))
    tracks[:, :, 2] = (rs.uniform(-np.pi, np.pi, (1, D, 1)) + at * rs.uniform(-0.4, 0.4, (1, D, 1)))[:, :, 0]
    extents = rs.uniform(0.05, 0.9, (D, 2))
    return Case("general position: assorted headings, 8 rectangles", t, tracks, extents)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    # 1, 2: what a disc cannot say, and the heading decides
    for name, h in (("fork, a 6 x 0.4 rectangle passes beside the short branch", 0.0), ("fork, the same track, heading pi/2", np.pi / 2)):
        out.append(_fork(name, cross=oncoming(20, heading=h), e_cross=(3.0, 0.2)))
    # time: clear_reference's cases, the discs replaced by squares
    out.append(_fork("fork, the rectangle crosses the short branch"))
    out.append(_fork("fork, the rectangle has passed (start = 4)", start=4))
    out.append(_fork("fork, dwell conflict at L - 1, the long branch arrives later", L=14, cross=_dwell_track(14)))
    out.append(_fork("fork, L = 8: the crossing is the last row (tau = L - 1)", L=8))
    out.append(_fork("fork, L = 7: the rectangle stops short, tau = L is clamped", L=7))
    out.append(_fork("fork, start >= L", L=8, start=8))
    out.append(_fork("fork, L = 1: the square stands on the short branch", L=1, cross=with_heading(cl.parked(1, 7.0, 0.0), np.pi / 2)))
    # 3: the inclusive edge.  Heading 0: co = 1, so = 0, xi = dx and eta = dy exactly; the rectangle exists at tau = 7 only, when the
    # vehicle of the short branch is at (7, 0) with its bow points at x = 7.5 and its port points at y = 0.25
    one = np.nextafter(1.0, 0.0)
    half = np.nextafter(0.5, 0.0)
    out.append(_fork("edge: a hull point on |xi| == a", cross=only_at(20, 7, 8.5, 0.0), e_cross=(1.0, 0.125)))
    out.append(_fork("edge: |xi| one ulp beyond a", cross=only_at(20, 7, 8.5, 0.0), e_cross=(one, 0.125)))
    out.append(_fork("edge: a hull point on |eta| == b", cross=only_at(20, 7, 7.0, 0.75), e_cross=(0.125, 0.5)))
    out.append(_fork("edge: |eta| one ulp beyond b", cross=only_at(20, 7, 7.0, 0.75), e_cross=(0.125, half)))
    # 4: a = b = 0 on the hull point (7.5, 0.25)
    out.append(_fork("zero extents on a hull point", cross=only_at(20, 7, 7.5, 0.25, heading=0.9), e_cross=(0.0, 0.0)))
    # 5: lane tiles
    out.append(_fork("fork, D = 64, the crossing rectangle last", pad=63, parked=False))
    out.append(_fork("fork, D = 65, the crossing rectangle last", pad=64, parked=False))
    out.append(_fork("fork, D = 65, the crossing rectangle first", pad=64, parked=False, cross_last=False))
    out.append(_fork("boat_novice, D = 65: one point, inflated extents", system="boat_novice", pad=64, parked=False, far=12.0,
                     cross=_novice_cross(20)))
    out.append(_fork("ros_boat on an occupied grid, 3073 hull points, D = 65", system="ros_boat", vps="big", grid=True, pad=63,
                     second=(11.75, 0.0)))
    # 7: propagation
    deep = cl.case("chain of 256, conflict on the root")
    out.append(Case("chain of 256, conflict on the root", deep.tree, with_heading(deep.tracks[:, 0], 0.0), SQUARE, none=True))
    out.append(Case("N = 257, the spine blocked at node 1", cl.case("N = 257, the spine blocked at node 1").tree,
                    with_heading(cl.case("N = 257, the spine blocked at node 1").tracks[:, 0], 0.0), SQUARE))
    # 8: models
    for system in ("boat_advanced", "boat_intermediate", "ros_boat", "car"):
        out.append(_fork("%s: the fork" % system, system=system))
    out.append(_fork("boat_novice: the fork", system="boat_novice", second=(30.0, 30.0), far=12.0, cross=_novice_cross(20)))
    out.append(_fork("car: a rectangle over the 2p vertex of node 7's last row", system="car", second=(10.0, -4.0)))
    fast = _fork("boat_advanced: a row outside the planning speed box")
    fast.tree.xedge[4, 2, 3] = 5.0                                   # node 4 of the long branch, its middle row: 5 m/s > 1.1
    out.append(fast)
    # 9: general position
    out.append(_general_position())
    return out


def case(name):
    for c in cases():
        if c.name == name:
            return c
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------ fixture trees

FIXTURE_EXTENTS = np.array([[1.0, 0.4], [1.5, 0.6], [1.0, 0.4], [0.8, 0.5]])


def fixture_tracks(f):
    """Four rectangles laid on the fixture's plan as FixtureTree.tracks lays its discs, headings along their motion (a rectangle that
    stands has heading 0).  Returns (tracks (L, 4, 3), extents (4, 2))."""
    xy, _ = f.tracks()
    L = len(xy)
    out = np.zeros((L, 4, 3))
    out[:, :, :2] = xy
    out[:, 0, 2] = np.arctan2(0.05, 0.5)
    out[:, 2, 2] = np.arctan2(0.5, 0.05)
    return out, FIXTURE_EXTENTS.copy()


@functools.lru_cache(maxsize=None)
def fixture_reference(name):
    f = cl.fixture(name)
    s = f.native()
    lo, hi = f.box(s)
    tracks, extents = fixture_tracks(f)
    return clear_rects(f.state, f.pID, f.elen, f.xedge, row_test_of(s), tracks, extents, 0, lo, hi)
