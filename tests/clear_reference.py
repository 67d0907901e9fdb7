"""
Reference of the clearance query (Engine.tree_clear / Planner.avoid, csrc/clear.hpp) in plain NumPy: one sequential pass.

The rule, exactly as the engine implements it.  A tree of N nodes with root 0 and pID[i] < i, edge lengths elen and recorded edge
rows xedge; a track table tracks[L][D][2] -- the world x, y of D discs of radii[D] at L consecutive instants spaced by the engine's
dt; an integer start >= 0, the track row that coincides with the root's row; the current goal box.

  1. Time.  cum[0] = elen[0] (= 1), cum[i] = cum[pID[i]] + elen[i].  Row k of node i > 0 has time index
     tau = start + cum[pID[i]] + k -- its index in a plan's x_seq plus start -- and the root's one row (its last) has tau = start.
  2. Discs.  At tau the discs are at tracks[min(tau, L - 1)]: a track that has ended stays where it ended.
  3. Row test.  The system's feasibility test of that row with the obstacle set replaced by the D discs of its instant, no
     occupancy grid, cos / sin of the heading the portable lq_sincos: row_test() below (it takes the rows of an edge at once; the
     first failing one in order counts).  A disc is a circular obstacle as the static
     map has them: norm(vertex - centre) <= r for the hull sweepers (the car keeps its 2p vertex, BoatAdvanced its planning
     speed box), norm(p - centre) <= half_length + r for the novice boats.
  4. own_first[i] = the smallest tau of a failing row of node i's own edge, or -1; first[i] = the smallest own_first >= 0 over the
     nodes from i up to and including the root, or -1.  A node is clear when first[i] == -1.
  5. A goal hit is a non-root node whose state is strictly inside the goal box.  For a hit only, dwell_first[i] = the smallest tau'
     with cum[i] - 1 + start < tau' <= L - 1 at which the node's LAST row fails against the discs of tau', or -1 (the loop is empty
     when the hit arrives at or after L - 1); -2 for every other node.  A dwell conflict does not make descendants unclear.
  6. Best = the hit with first == -1 and dwell_first == -1 of the smallest (cum, id).  Counters: size, conflicts (own_first >= 0),
     blocked (own_first == -1, first >= 0), hits, clear_hits, best_end, best_steps (-1 / -1 without a clear hit).

CASES: every hand-built input of tests/test_clear_gpu.py, built once here and shared with tests/test_clear_cpu.py, which shows with
this reference alone that none of them is degenerate.
"""
import functools
import os

import numpy as np

import feasibility_reference as fr
from feasibility_reference import circles_feasible, novice_feasible, portable_sincos      # noqa: F401  (the models restated below are held against them)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STAT_KEYS = ("size", "conflicts", "blocked", "hits", "clear_hits", "best_end", "best_steps")


# ------------------------------------------------------------------------------------------------ the row test

def discs_hit(points, discs):
    """points (R, P, 2), discs (R, D, 3) as [x, y, r] -> (R,) bool: some point of row r lies within some disc of row r,
    np.linalg.norm(point - centre) <= r (circles_feasible's test, pair by pair, for R rows at once)."""
    if points.shape[1] == 0:
        return np.zeros(len(points), dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.linalg.norm(points[:, None, :, :] - discs[:, :, None, :2], axis=3)
        return np.any(d <= discs[:, :, 2:3], axis=(1, 2))


def row_test(kind, vps=None, half_length=None, speed_box=None):
    """The test of R rows for a system of that kind: callable (X [R][n], c [R], s [R], discs [R][D][3]) -> (R,) bool, True = the row
    passes; row r is tested against discs[r] alone.  kind: 'hull' (BoatIntermediate, RosBoat), 'car' (hull + the 2p vertex),
    'advanced' (BoatAdvanced: speed_box = (velmax_pos_plan, velmax_neg_plan) first, then the hull), 'novice' (the centre point
    against radii inflated by half_length).  Per (row, vertex, disc) the arithmetic is that of feasibility_reference's
    circles_feasible / novice_feasible: tests/test_clear_cpu.py holds them together."""
    if kind == "novice":
        hl = np.float64(half_length)

        def novice(X, c, s, discs):
            with np.errstate(invalid="ignore", over="ignore"):
                d = np.linalg.norm(X[:, None, :2] - discs[:, :, :2], axis=2)
                return ~np.any(d <= hl + discs[:, :, 2], axis=1)
        return novice
    vps = np.asarray(vps, dtype=np.float64).reshape(2, -1)

    def hull(X, c, s, discs):
        c, s = np.asarray(c)[:, None], np.asarray(s)[:, None]
        with np.errstate(invalid="ignore", over="ignore"):
            vx = X[:, 0:1] + (c * vps[0] + (-s) * vps[1])          # feasibility_reference.vertices, row by row
            vy = X[:, 1:2] + (s * vps[0] + c * vps[1])
            verts = np.stack((vx, vy), axis=2)
            if kind == "car":
                verts = np.concatenate((verts, (X[:, :2] + X[:, :2])[:, None, :]), axis=1)      # demo_car.py:175
        ok = ~discs_hit(verts, discs)
        if kind == "advanced":
            ok &= ~(np.any(X[:, 3:6] > speed_box[0], axis=1) | np.any(X[:, 3:6] < speed_box[1], axis=1))   # demo_boat_advanced.py:211-213
        return ok
    return hull


def row_test_of(system):
    """row_test for an lqrrt_amd.systems object (its hull points and parameters as they are now)."""
    name = type(system).__name__
    if name in ("BoatNovice", "BoatNoviceLqr"):
        return row_test("novice", half_length=system.boat_length / 2)
    if name == "BoatAdvanced":
        return row_test("advanced", system.vps, speed_box=(np.asarray(system.velmax_pos_plan, dtype=np.float64),
                                                           np.asarray(system.velmax_neg_plan, dtype=np.float64)))
    if name == "Car":
        return row_test("car", system.vps)
    if name in ("BoatIntermediate", "RosBoat"):
        return row_test("hull", system.vps)
    raise ValueError("no circle path: %s" % name)


# ------------------------------------------------------------------------------------------------ the rule

def clear(state, pID, elen, xedge, test, tracks, radii, start, goal_lo, goal_hi, heading=2):
    """state (N, n), pID (N,), elen (N,), xedge (N, H, n) -- rows beyond elen[i] are not read; test: row_test(); tracks (L, D, 2),
    radii (D,) or a scalar; start >= 0; goal_lo / goal_hi (n,).  Returns dict(cum, own_first, first, dwell_first, hit, stats)."""
    state, xedge = np.asarray(state, dtype=np.float64), np.asarray(xedge, dtype=np.float64)
    pID, elen = np.asarray(pID, dtype=np.int64), np.asarray(elen, dtype=np.int64)
    tracks = np.asarray(tracks, dtype=np.float64)
    L, D = tracks.shape[:2]
    assert tracks.shape == (L, D, 2) and L >= 1 and D >= 1 and int(start) == start and start >= 0
    radii = np.broadcast_to(np.asarray(radii, dtype=np.float64), (D,))
    N = len(state)

    table = np.concatenate((tracks, np.broadcast_to(radii[None, :, None], (L, D, 1))), axis=2)      # [L][D][x, y, r]

    def discs_at(taus):
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
        ok = test(xedge[i, ks], c[ks], s[ks], discs_at([tau for _, tau in rows]))
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
                ok = test(np.repeat(xedge[i, ln - 1:ln], R, axis=0), np.repeat(c[ln - 1], R), np.repeat(s[ln - 1], R),
                          discs_at(taus))
                bad = np.flatnonzero(~ok)
                if len(bad):
                    dwell[i] = taus[bad[0]]
            if first[i] == -1 and dwell[i] == -1 and (best is None or (int(cum[i]), i) < best):
                best = (int(cum[i]), i)
    stats = dict(size=N, conflicts=int(np.sum(own >= 0)), blocked=int(np.sum((own == -1) & (first >= 0))), hits=int(np.sum(hit)),
                 clear_hits=int(np.sum(hit & (first == -1) & (dwell == -1))), best_end=-1 if best is None else best[1],
                 best_steps=-1 if best is None else best[0])
    return dict(cum=cum, own_first=own, first=first.astype(np.int32), dwell_first=dwell.astype(np.int32), hit=hit, stats=stats)


def degenerate(res):
    """What a case lacks of: a conflicting node, a blocked node, a clear hit, a hit that is not clear."""
    st = res["stats"]
    lacks = []
    if st["conflicts"] < 1:
        lacks.append("conflict")
    if st["blocked"] < 1:
        lacks.append("blocked")
    if st["clear_hits"] < 1:
        lacks.append("clear hit")
    if st["hits"] - st["clear_hits"] < 1:
        lacks.append("hit that is not clear")
    return lacks


# ------------------------------------------------------------------------------------------------ hand-built trees

H_HAND = 5                                                           # horizon_iters of the hand-built trees: an edge of 5 rows is full
NSTATES = dict(boat_advanced=6, boat_intermediate=6, boat_novice=6, ros_boat=6, car=5)
NCONTROLS = dict(boat_advanced=3, boat_intermediate=3, boat_novice=3, ros_boat=3, car=2)
GOAL_XY, GOAL_BUF = (10.0, 0.0), 0.5


class HandTree(object):
    """Nodes given as (parent, [(x, y, heading), ...]): the rows of the edge; the node's state is its last row.  Velocities zero."""

    def __init__(self, system, nodes):
        n, m = NSTATES[system], NCONTROLS[system]
        N = len(nodes)
        self.system, self.n, self.m = system, n, m
        self.pID = np.array([p for p, _ in nodes], dtype=np.int32)
        self.elen = np.array([len(r) for _, r in nodes], dtype=np.int32)
        assert self.pID[0] == -1 and self.elen[0] == 1 and np.all(self.pID[1:] < np.arange(1, N)) and self.elen.max() <= H_HAND
        self.xedge = np.zeros((N, H_HAND, n))
        for i, (_, rows) in enumerate(nodes):
            self.xedge[i, :len(rows), :3] = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
        self.uedge = np.zeros((N, H_HAND, m))
        self.state = np.array([self.xedge[i, self.elen[i] - 1] for i in range(N)])
        self.K = np.zeros((N, m, n))
        self.goal = np.zeros(n)
        self.goal[:2] = GOAL_XY
        self.goal_buffer = np.array([GOAL_BUF, GOAL_BUF] + [np.inf] * (n - 2))

    @property
    def size(self):
        return len(self.pID)

    def box(self):
        return self.goal - self.goal_buffer, self.goal + self.goal_buffer

    def packed(self):
        """(xedge, uedge) back to back in node order: the form Engine.tree_load takes."""
        live = np.arange(H_HAND)[None, :] < self.elen[:, None]
        return self.xedge[live], self.uedge[live]


def fork_nodes(far=6.0):
    """A fork: the short branch 0-1-2 runs along y = 0 to the goal at (10, 0) in 11 steps, with 6 and 9 beyond node 2 inside the
    goal box, 10 below 6 outside it again, and the side twig 7-8; the long branch 0-3-4-5 goes round at y = far and reaches the box in 16."""
    row = lambda x, y: (float(x), float(y), 0.0)
    return [(-1, [row(0, 0)]),
            (0, [row(x, 0) for x in (1, 2, 3, 4, 5)]),                                              # 1
            (1, [row(x, 0) for x in (6, 7, 8, 9, 10)]),                                             # 2  hit, cum 11
            (0, [row(0, 0.25 * far), row(0, 0.5 * far), row(0, 0.75 * far), row(0, far), row(1, far)]),   # 3
            (3, [row(x, far) for x in (2, 3, 4, 5, 6)]),                                            # 4
            (4, [row(7, far), row(8, far), row(9, far - 1.0), row(10, 0.5 * far), row(10, 0.2)]),    # 5  hit, cum 16
            (2, [row(10.1, 0), row(10.2, 0), row(10.3, 0)]),                                        # 6  hit, cum 14
            (1, [row(5, -1), row(5, -2)]),                                                          # 7
            (7, [row(5, -3)]),                                                                      # 8  an edge of one row
            (6, [row(10.35, 0)]),                                                                   # 9  hit, cum 15
            (6, [row(9.5, -1.5)])]                                                                  # 10 leaves the box again


def crossing(L, x=7.0, at=7, speed=1.0):
    """A disc that moves up the line x = const and crosses y = 0 at row `at`: (L, 2)."""
    t = np.arange(L, dtype=np.float64)
    return np.column_stack((np.full(L, float(x)), speed * (t - at)))


def parked(L, x, y):
    return np.tile(np.array([[float(x), float(y)]]), (L, 1))


def far_discs(L, count):
    """count discs that stand far from everything: (L, count, 2)."""
    out = np.zeros((L, count, 2))
    out[:, :, 0] = 500.0 + 3.0 * (np.arange(count) % 50)
    out[:, :, 1] = 500.0 + 3.0 * (np.arange(count) // 50)
    return out


def chain_nodes(count, step=0.05, rows=1):
    """A spine 1 .. count along +x from the root, `rows` rows per node."""
    nodes, x = [], 0.0
    for j in range(count):
        r = []
        for _ in range(rows):
            x += step
            r.append((x, 0.0, 0.0))
        nodes.append((j, r))
    return nodes


def spine_and_branch(N, system="boat_advanced"):
    """N nodes: the root, a spine of N - 4 one-row nodes along +x that ends inside the goal box (the goal is moved onto its end), and
    a branch 0 - a - b - c that leaves the root by 3 m, runs beside the spine and ends inside the box too."""
    spine = N - 4
    nodes = [(-1, [(0.0, 0.0, 0.0)])] + chain_nodes(spine)
    end = 0.05 * spine
    a = len(nodes)
    nodes.append((0, [(0.0, -3.0, 0.0), (0.25 * end, -3.0, 0.0)]))
    nodes.append((a, [(0.5 * end, -3.0, 0.0), (0.75 * end, -3.0, 0.0), (end, -3.0, 0.0)]))
    nodes.append((a + 1, [(end, -1.5, 0.0), (end, -0.3, 0.0)]))
    t = HandTree(system, nodes)
    t.goal[:2] = (end, 0.0)
    return t


class Case(object):
    """One (system, tree, tracks, radii, start); `none`: the case exists to show that nothing is clear (or nothing conflicts)."""

    def __init__(self, name, tree, tracks, radii, start=0, none=False, vps="small", grid=False):
        self.name, self.tree, self.start, self.none, self.vps_kind, self.grid = name, tree, int(start), none, vps, grid
        self.tracks = np.ascontiguousarray(tracks, dtype=np.float64)
        if self.tracks.ndim == 2:
            self.tracks = self.tracks[:, None, :]
        self.radii = np.ascontiguousarray(np.broadcast_to(np.asarray(radii, dtype=np.float64), (self.tracks.shape[1],)))

    def vps(self):
        return fr.big_lattice_hull() if self.vps_kind == "big" else fr.lattice_hull(1.0, 0.5, 0.25)

    def test(self):
        sysname = self.tree.system
        if sysname == "boat_novice":
            return row_test("novice", half_length=fr.HALF_LENGTH)
        if sysname == "boat_advanced":
            return row_test("advanced", self.vps(), speed_box=fr.PLAN_BOX)
        return row_test("car" if sysname == "car" else "hull", self.vps())

    def native(self):
        """The lqrrt_amd system of this case: the small hull, no static obstacle; grid: an occupancy grid that is occupied everywhere."""
        import lqrrt_amd
        S = lqrrt_amd.systems
        s = S.RosBoat("boat") if self.tree.system == "ros_boat" else S.SYSTEMS[self.tree.system](0)
        if self.tree.system != "boat_novice":
            s.vps = self.vps()
        s.set_obstacles(np.zeros((0, 3)))
        if self.grid:
            s.set_occupancy_grid(fr.empty_map(64, 64, fr.OCC), (-20.0, -20.0), cpm=1.0, threshold=fr.THR, vps=self.vps())
        s.goal = [float(v) for v in self.tree.goal]
        s.goal_buffer = [float(v) for v in self.tree.goal_buffer]
        return s

    @functools.lru_cache(maxsize=None)
    def reference(self):
        t = self.tree
        lo, hi = t.box()
        return clear(t.state, t.pID, t.elen, t.xedge, self.test(), self.tracks, self.radii, self.start, lo, hi)


def _fork_case(name, system="boat_advanced", L=20, start=0, cross=None, r_cross=0.4, second=(11.0, 0.0), pad=0, cross_last=True, far=6.0,
               **kw):
    """The fork with the crossing disc, a parked second disc beyond the goal that catches node 6, and `pad` discs far away."""
    cross = crossing(L) if cross is None else cross
    cols = [parked(L, *second)[:, None, :], far_discs(L, pad)] + ([cross[:, None, :]] if cross_last else [])
    if not cross_last:
        cols.insert(0, cross[:, None, :])
    tracks = np.concatenate(cols, axis=1)
    radii = np.full(tracks.shape[1], 0.4)
    radii[-1 if cross_last else 0] = r_cross
    return Case(name, HandTree(system, fork_nodes(far)), tracks, radii, start, **kw)


def _dwell_track(L):
    """Far away until the last row, then just below the goal: 0.35 from the hull of a vehicle parked at (10, 0), 0.55 from one at (10, 0.2)."""
    t = parked(L, 50.0, 50.0)
    t[L - 1] = (10.0, -0.6)
    return t


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    root_only = HandTree("boat_advanced", [(-1, [(0.0, 0.0, 0.0)])])
    out.append(Case("N=1, a disc on the root", root_only, parked(3, 0.2, 0.0), 0.4, none=True))
    out.append(Case("N=1, nothing near", root_only, parked(3, 9.0, 9.0), 0.4, none=True))
    out.append(_fork_case("fork, the disc crosses the short branch"))
    out.append(_fork_case("fork, the disc has passed (start = 4)", start=4))
    out.append(_fork_case("fork, conflict on the first row of an edge", cross=crossing(20, x=6.0, at=6)))
    out.append(_fork_case("fork, conflict on the last row of an edge", cross=crossing(20, x=10.0, at=10)))
    out.append(_fork_case("fork, dwell conflict at L - 1, the long branch arrives later", L=14, cross=_dwell_track(14)))
    out.append(_fork_case("fork, L = 8: the crossing is the last row (tau = L - 1)", L=8))
    out.append(_fork_case("fork, L = 7: the disc stops short, tau = L is clamped", L=7))
    out.append(_fork_case("fork, start >= L", L=8, start=8))
    out.append(_fork_case("fork, a radius-0 disc through a hull point", r_cross=0.0))
    out.append(_fork_case("fork, D = 64, the crossing disc last", pad=62))
    out.append(_fork_case("fork, D = 65, the crossing disc last", pad=63))
    out.append(_fork_case("fork, D = 65, the crossing disc first", pad=63, cross_last=False))
    # L = 1, D = 1, equal steps: nodes 1 and 2 reach the box in 6 steps, node 3 in 4 through the disc, node 4 hangs below it
    row = lambda x, y: (float(x), float(y), 0.0)
    tie = HandTree("boat_advanced", [(-1, [row(0, 0)]),
                                     (0, [row(2, 0), row(4, 0), row(6, 0), row(8, 0), row(10, 0.1)]),
                                     (0, [row(2, -1), row(4, -1), row(6, -1), row(8, -1), row(10, -0.1)]),
                                     (0, [row(3, 3), row(6, 3), row(10, 0.3)]),
                                     (3, [row(10, 0.35)])])
    out.append(Case("L = 1, D = 1, two clear hits with equal steps", tie, parked(1, 6.0, 3.0), 0.4))
    # 33 nodes in a chain, two rows each, a parked disc 2 m ahead of the root that only node 1's rows reach... every hit is blocked
    chain = HandTree("boat_advanced", [(-1, [row(0, 0)])] + chain_nodes(32, step=1.0, rows=2))
    chain.goal[:2] = (64.0, 0.0)
    chain.goal_buffer[:2] = 2.2
    out.append(Case("chain of 33, conflict at node 1", chain, parked(1, 2.0, 0.6), 0.4, none=True))
    for N in (255, 256, 257):
        t = spine_and_branch(N)
        track = parked(4, 80.0, 80.0)
        track[1] = (0.05, 0.0)                                       # on the spine's first node at ITS instant only
        out.append(Case("N = %d, the spine blocked at node 1" % N, t, track, 0.4))
    # a chain of 2^8 nodes whose ROOT row is hit: depth 255, the root's conflict reaches the last node in the last round
    deep = HandTree("boat_advanced", [(-1, [row(0, 0)])] + chain_nodes(255))
    deep.goal[:2] = (0.05 * 255, 0.0)
    track = parked(2, 80.0, 80.0)
    track[0] = (0.0, 0.0)
    out.append(Case("chain of 256, conflict on the root", deep, track, 0.4, none=True))
    # systems
    out.append(_fork_case("car: the fork", system="car"))
    car = _fork_case("car: a disc on the 2p vertex of node 7's last row", system="car", second=(10.0, -4.0))
    out.append(car)
    out.append(_fork_case("boat_advanced: a disc on what would be a car's 2p vertex", second=(10.0, -4.0)))
    out.append(_fork_case("boat_novice: the inflated radius", system="boat_novice", second=(30.0, 30.0), far=12.0))
    out.append(_fork_case("boat_intermediate: the fork", system="boat_intermediate"))
    out.append(_fork_case("ros_boat on an occupied grid, 3073 hull points", system="ros_boat", vps="big", grid=True, second=(11.6, 0.0)))
    return out


def case(name):
    for c in cases():
        if c.name == name:
            return c
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------ fixture trees

class FixtureTree(object):
    """The final tree of a committed run (traj_<name>.npz + edges_<name>.npz) in clear()'s layout."""

    def __init__(self, name):
        g = np.load(os.path.join(GOLDEN, "traj_%s.npz" % name))
        e = np.load(os.path.join(GOLDEN, "edges_%s.npz" % name))
        self.name, self.system = name, name.rsplit("_", 1)[0]
        self.state, self.K, self.pID = g["state"], g["K"], g["pID"].astype(np.int32)
        self.elen = e["edge_len"].astype(np.int32)
        self.x_cat, self.u_cat = e["x_cat"], e["u_cat"]
        self.plan = [int(v) for v in g["node_seq"]]
        N, self.H = len(self.state), int(self.elen.max())
        off = np.concatenate(([0], np.cumsum(self.elen)))
        self.xedge = np.zeros((N, self.H, self.state.shape[1]))
        for i in range(N):
            self.xedge[i, :self.elen[i]] = self.x_cat[off[i]:off[i + 1]]

    def native(self):
        """The fixture's system.  The boat's run ended before its tree reached the demo's goal: there the goal is moved onto the end
        of the fixture's own plan (x, y; the box keeps its size), so that the tree holds goal hits."""
        import lqrrt_amd
        s = lqrrt_amd.systems.SYSTEMS[self.system](0)
        if self.name == "boat_advanced_3000":
            s.goal = [float(self.state[self.plan[-1], 0]), float(self.state[self.plan[-1], 1])] + [float(v) for v in s.goal[2:]]
        return s

    def box(self, s):
        goal = np.asarray(s.goal, dtype=np.float64)
        buf = np.abs(np.asarray(s.goal_buffer, dtype=np.float64))
        return goal - buf, goal + buf

    def packed(self):
        """(xedge, uedge) back to back in node order: the form Engine.tree_load takes."""
        return self.x_cat, self.u_cat

    def plan_rows(self):
        """x_seq of the fixture's own plan: its edges end to end."""
        return np.concatenate([self.xedge[v, :self.elen[v]] for v in self.plan])

    def tracks(self, L=None):
        """Four discs placed on and beside the fixture's own best plan, late enough on it that other goal hits have left it: one
        that crosses it along x at 85 % of its rows exactly when the vehicle is there, one that stands 7 m beside it at 60 % while
        the vehicle passes (30 rows either side; far away before and after), one that crosses it along y at 75 %, one that is far
        away and parks on the plan's end 20 rows after the vehicle has arrived.
        Returns (tracks (L, 4, 2), radii)."""
        rows = self.plan_rows()
        P = len(rows)
        L = P + 60 if L is None else L
        t = np.arange(L, dtype=np.float64)
        a, b, c, end = (85 * P) // 100, (60 * P) // 100, (75 * P) // 100, rows[-1, :2]
        out = np.zeros((L, 4, 2))
        out[:, 0, 0] = rows[a, 0] + 0.5 * (t - a)
        out[:, 0, 1] = rows[a, 1] + 0.05 * (t - a)
        out[:, 1] = (-900.0, 900.0)
        out[max(b - 30, 0):b + 30, 1] = rows[b, :2] + np.array([7.0, 0.0])
        out[:, 2, 0] = rows[c, 0] + 0.05 * (t - c)
        out[:, 2, 1] = rows[c, 1] + 0.5 * (t - c)
        out[:, 3] = (900.0, 900.0)
        out[P + 20:, 3] = end
        return out, np.array([0.6, 1.0, 0.6, 0.5])


@functools.lru_cache(maxsize=None)
def fixture(name):
    return FixtureTree(name)


@functools.lru_cache(maxsize=None)
def fixture_reference(name):
    f = fixture(name)
    s = f.native()
    lo, hi = f.box(s)
    tracks, radii = f.tracks()
    return clear(f.state, f.pID, f.elen, f.xedge, row_test_of(s), tracks, radii, 0, lo, hi)
