"""
Reference of the clear goal chains (Engine.tree_clear_connect / Planner.avoid(connect), csrc/clear_connect.hpp), composed from the
two references it joins: clear_reference (clear, row_test / row_test_of) and connect_reference.Connector (depths, chain and with it
_edge and in_goal).  Neither is restated here.

The rule, exactly as the engine implements it.  Everything of clear_reference holds unchanged and comes first: cum, tau, the clamp
min(tau, L - 1), the row test against the D discs of that instant alone, own_first, first, dwell_first, best, the seven counters.

  1. Incumbent.  With b the best clear hit: incumbent = depth[b] in the connection's cost units -- depth[0] = 1,
     depth[v] = depth[pID[v]] + elen[v], so depth = cum - elen[0] + 1.  Without a clear hit: 2^31 - 1.  The caller passes none.
  2. Candidates.  A node v -- every node, or those of a caller's id list -- with first[v] == -1.  The propagated first counts, not
     own_first: a node below a conflict is no candidate.  The root is one when its own row passes at tau = start.
  3. Chain.  connect_reference's: up to `tries` steers at the goal against the static map with the fixed horizon, an empty edge
     ends it, valid when an edge ends strictly inside the goal box.  The discs cut no edge; they accept or reject the chain, so that
     connect_commit(v, H, tries) replays exactly the chain that was judged.
  4. Time.  Row k of the chain's j-th non-empty edge has tau = start + cum[v] + (rows of the chain's earlier edges) + k -- after a
     commit, clear_reference gives the same row the same time.  A chain is clear when every row of every edge passes at its tau, and
     its last row passes at every tau' in [start + cum[v] + chain rows, L - 1] (the dwell; an empty range passes).
  5. Winner.  The valid and clear candidate of smallest (cost, v) with cost = depth[v] + chain rows < incumbent, strictly.
  6. Early stop.  The engine abandons a chain once its running (cost, v) exceeds the best valid and clear one found so far; costs
     only grow along a chain, so the winner is the one of the full enumeration below.

Reported besides the counters: clear_candidates (candidates with first == -1), chain_from, chain_cost, chain_rows, chain_arrival
(= cum[v] + chain rows: best_steps after a commit); -1 for the last four without a winner.

cases(): every input of tests/test_clear_connect_gpu.py on the committed fixture trees, built once here and shared with
tests/test_clear_connect_cpu.py, which pins the answers and shows with this reference alone that none is degenerate.  The discs are
placed from the reference's own answers -- on a row of the unconstrained winner's chain, on the tree path of a node at its tau --
never from coordinates written down here.
"""
import functools
import os

import numpy as np

import clear_reference as cl
import connect_reference as cr
from feasibility_reference import portable_sincos

NO_INCUMBENT = cr.NO_INCUMBENT
CHAIN_KEYS = ("clear_candidates", "chain_from", "chain_cost", "chain_rows", "chain_arrival")
FAR = (-700.0, 700.0)                                               # where a disc stands when it is nowhere near the tree


class Tree(object):
    """A tree in both references' layouts: state, K, pID, elen, xedge [N][H][n] (and the packed rows x_cat, u_cat that
    Engine.tree_load takes), the system with its goal box, the row test, and the fixed steer horizon H."""

    def __init__(self, system, state, K, pID, elen, xedge, uedge, H, name=""):
        self.system, self.name, self.H = system, name, int(H)
        self.state, self.K = np.asarray(state, dtype=np.float64), np.asarray(K, dtype=np.float64)
        self.pID, self.elen = np.asarray(pID, dtype=np.int32), np.array(elen, dtype=np.int32)
        assert self.elen[0] == 1 and self.pID[0] == -1
        self.xedge, self.uedge = np.asarray(xedge, dtype=np.float64), np.asarray(uedge, dtype=np.float64)
        goal = np.asarray(system.goal, dtype=np.float64)
        buf = np.abs(np.asarray(system.goal_buffer, dtype=np.float64))
        self.lo, self.hi = goal - buf, goal + buf
        self.test = cl.row_test_of(system)
        self._con, self._chains, self._plain = None, {}, None

    @property
    def size(self):
        return len(self.pID)

    def packed(self):
        live = np.arange(self.xedge.shape[1])[None, :] < self.elen[:, None]
        return np.ascontiguousarray(self.xedge[live]), np.ascontiguousarray(self.uedge[live])

    def connector(self):
        if self._con is None:
            self._con = cr.Connector(self.system, self.state, self.K, self.pID, self.elen, self.H)
        return self._con

    def chain(self, v, tries=8):
        """connect_reference's chain of candidate v, unpruned: (cost, edges) or None.  It does not depend on the discs: kept."""
        key = (int(v), int(tries))
        if key not in self._chains:
            self._chains[key] = self.connector().chain(int(v), tries)
        return self._chains[key]

    def chain_rows(self, v, tries=8):
        """The rows of v's valid chain end to end [R][n], and the lengths of its edges."""
        cost, edges = self.chain(v, tries)
        return np.concatenate([xs for xs, _, _ in edges]), [len(xs) for xs, _, _ in edges]

    def touch(self, row, front=False):
        """A world point that a disc of any radius > 0 centred there hits when the vehicle stands on `row`: a hull vertex -- the
        first, or with `front` the foremost -- (the centre for the novice boats, whose test is the centre's)."""
        row = np.asarray(row, dtype=np.float64)
        if type(self.system).__name__ in ("BoatNovice", "BoatNoviceLqr"):
            return row[:2].copy()
        vps = np.asarray(self.system.vps, dtype=np.float64).reshape(2, -1)
        c, s = portable_sincos(row[2:3])
        q = int(np.argmax(vps[0])) if front else 0
        return np.array([row[0] + (c[0] * vps[0, q] + (-s[0]) * vps[1, q]), row[1] + (s[0] * vps[0, q] + c[0] * vps[1, q])])


def clear_connect(tree, tracks, radii, start, tries=8, nodes=None):
    """The rule on `tree`.  Returns clear_reference's dict with, added: chain (the five fields), incumbent, and verdicts -- per
    candidate with first == -1 one of ('invalid',), ('route', tau), ('dwell', tau), ('clear', cost, rows) --, and judge, which
    gives that verdict for any node."""
    tracks = np.asarray(tracks, dtype=np.float64)
    if tracks.ndim == 2:
        tracks = tracks[:, None, :]
    L, D = tracks.shape[:2]
    radii = np.broadcast_to(np.asarray(radii, dtype=np.float64), (D,))
    res = cl.clear(tree.state, tree.pID, tree.elen, tree.xedge, tree.test, tracks, radii, start, tree.lo, tree.hi)
    table = np.concatenate((tracks, np.broadcast_to(radii[None, :, None], (L, D, 1))), axis=2)
    depth = tree.connector().depths()
    cum, first = res["cum"], res["first"]
    assert all(depth[v] == cum[v] - tree.elen[0] + 1 for v in range(tree.size))
    b = res["stats"]["best_end"]
    incumbent = depth[b] if b >= 0 else NO_INCUMBENT
    ids = range(tree.size) if nodes is None else [int(v) for v in nodes]
    cands = [v for v in ids if first[v] == -1]

    def passes(rows, taus):
        c, s = portable_sincos(rows[:, 2])
        return tree.test(rows, c, s, table[np.minimum(np.asarray(taus, dtype=np.int64), L - 1)])

    def judge(v):
        """The verdict on node v's chain, whether or not v is a candidate."""
        got = tree.chain(v, tries)
        if got is None:
            return ("invalid",)
        cost, edges = got
        tau = start + int(cum[v])
        for xs, _, _ in edges:
            bad = np.flatnonzero(~passes(xs, tau + np.arange(len(xs))))
            if len(bad):
                return ("route", tau + int(bad[0]))
            tau += len(xs)
        if tau <= L - 1:
            taus = np.arange(tau, L)
            bad = np.flatnonzero(~passes(np.repeat(edges[-1][0][-1:], len(taus), axis=0), taus))
            if len(bad):
                return ("dwell", int(taus[bad[0]]))
        return ("clear", cost, cost - depth[v])

    verdicts, best = {}, None
    for v in cands:
        if v in verdicts:
            continue
        verdicts[v] = w = judge(v)
        if w[0] == "clear" and w[1] < incumbent and (best is None or (w[1], v) < best):
            best = (w[1], v)
    chain = dict(clear_candidates=len(cands), chain_from=-1, chain_cost=-1, chain_rows=-1, chain_arrival=-1)
    if best is not None:
        cost, v = best
        chain.update(chain_from=v, chain_cost=cost, chain_rows=cost - depth[v], chain_arrival=int(cum[v]) + cost - depth[v])
    return dict(res, chain=chain, incumbent=incumbent, verdicts=verdicts, judge=judge)


# ------------------------------------------------------------------------------------------------ tracks from the reference's answers

def far(L, count=1):
    return cl.far_discs(L, count)


def instant(L, at, point):
    """One disc that stands at `point` at table row `at` alone and far away at every other instant: (L, 2)."""
    t = np.tile(np.array([FAR], dtype=np.float64), (L, 1))
    t[at] = point
    return t


def with_far(track, pad, last=True):
    """`track` (L, 2) among `pad` far discs, as the last disc or the first: (L, pad + 1, 2)."""
    cols = [far(len(track), pad), track[:, None, :]] if pad else [track[:, None, :]]
    return np.concatenate(cols if last else cols[::-1], axis=1)


# ------------------------------------------------------------------------------------------------ fixture trees

@functools.lru_cache(maxsize=None)
def fixture_tree(name, size):
    """The first `size` nodes of a committed run that has edge rows (traj_<name>.npz + edges_<name>.npz)."""
    f = cl.fixture(name)
    s = f.native()
    off = np.concatenate(([0], np.cumsum(f.elen)))
    uedge = np.zeros((len(f.state), f.H, f.u_cat.shape[1]))
    for i in range(size):
        uedge[i, :f.elen[i]] = f.u_cat[off[i]:off[i + 1]]
    g = np.load(os.path.join(cr.GOLDEN, "traj_%s.npz" % name))
    return Tree(s, f.state[:size], f.K[:size], f.pID[:size], f.elen[:size], f.xedge[:size], uedge[:size], cr.horizon_of(s, g),
                "%s[:%d]" % (name, size))


class Case(object):
    """One (tree, tracks, radii, start, tries, nodes) and what it has to show: `winner` True / False (None: either), and `needs`, verdict kinds
    ('route', 'dwell') of which at least one candidate must have been rejected, or 'excluded' (a listed node with first >= 0)."""

    def __init__(self, name, tree, tracks, radii=0.3, start=0, nodes=None, winner=True, needs=(), tries=8):
        self.name, self.tree, self.start, self.tries, self.winner, self.needs = name, tree, int(start), int(tries), winner, tuple(needs)
        self.tracks = np.ascontiguousarray(tracks, dtype=np.float64)
        if self.tracks.ndim == 2:
            self.tracks = self.tracks[:, None, :]
        self.radii = np.ascontiguousarray(np.broadcast_to(np.asarray(radii, dtype=np.float64), (self.tracks.shape[1],)))
        self.nodes = None if nodes is None else [int(v) for v in nodes]

    @functools.lru_cache(maxsize=None)
    def reference(self):
        return clear_connect(self.tree, self.tracks, self.radii, self.start, self.tries, self.nodes)

    def lacks(self):
        """What the case fails to show, from the reference alone."""
        ref = self.reference()
        out = []
        if self.winner is not None and (ref["chain"]["chain_from"] >= 0) != self.winner:
            out.append("a winner" if self.winner else "no winner")
        kinds = [v[0] for v in ref["verdicts"].values()]
        for need in self.needs:
            if need == "excluded":
                ids = range(self.tree.size) if self.nodes is None else self.nodes
                if not any(ref["first"][v] >= 0 for v in ids):
                    out.append("excluded")
            elif need not in kinds:
                out.append(need)
        return out


def plain(tree):
    """clear_reference's answer with nothing near the tree: cum, and which nodes are goal hits."""
    if tree._plain is None:
        tree._plain = cl.clear(tree.state, tree.pID, tree.elen, tree.xedge, tree.test, far(1), 0.3, 0, tree.lo, tree.hi)
    return tree._plain


def chain_times(tree, v, start, tries=8):
    """Of candidate v's valid chain: rows [R][n], edge lengths, and tau of row 0."""
    rows, lens = tree.chain_rows(v, tries)
    return rows, lens, start + int(plain(tree)["cum"][v])


def cross_hits(tree, L=None, start=0, extra=0):
    """Every goal hit of the tree crossed: one disc per hit, on the hit's last row at the instant it arrives (tau = start + cum - 1)
    and far away at every other instant, so that no goal hit is clear and little else is touched.  (L, hits, 2), L by default just
    long enough (+ extra); one far disc for a tree without hits."""
    res = plain(tree)
    hits = np.flatnonzero(res["hit"])
    taus = [start + int(res["cum"][h]) - 1 for h in hits]
    L = (max(taus + [0]) + 2 + extra) if L is None else L
    if not len(hits):
        return far(L, 1)
    return np.stack([instant(L, t, tree.touch(tree.xedge[h, tree.elen[h] - 1])) for h, t in zip(hits, taus)], axis=1)


def generic_cases(tree, label, tries=8):
    """For any tree: every goal hit crossed, which leaves the chains; and, when a chain then wins, a further disc on the first
    row of that chain at its tau."""
    H = tree.H
    base = cross_hits(tree, extra=(tries + 1) * H)
    L = len(base)
    out = [Case("%s: every goal hit crossed" % label, tree, base, winner=None, tries=tries)]
    free = out[0].reference()["chain"]
    if free["chain_from"] >= 0:
        rows, lens, t0 = chain_times(tree, free["chain_from"], 0, tries)
        more = np.concatenate((base, instant(L, t0, tree.touch(rows[0]))[:, None, :]), axis=1)
        out.append(Case("%s: ... and a disc on the first row of the winner's chain" % label, tree, more, needs=("route",), winner=None,
                        tries=tries))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    car = fixture_tree("car_2000", 217)
    free = clear_connect(car, far(1), 0.3, 0)
    v = free["chain"]["chain_from"]
    assert (free["chain"]["chain_cost"], v) == (951, 211)           # connect_reference's winner on this prefix
    rows, lens, t0 = chain_times(car, v, 0)
    R = len(rows)
    assert len(lens) >= 2
    L = t0 + R + 8
    out = [Case("far discs", car, far(L, 3))]
    # 2: the first row of the first chain edge, at tau = start + cum[v]
    # (on this prefix the other valid chains leave from v's children, whose own edges are goal steers from v's state: the same rows
    # at the same instants, so that they are blocked with it and no winner remains; the winner MOVES in case 3)
    first_row = instant(L, t0, car.touch(rows[0]))
    r1 = 0.3
    out.append(Case("first row of the first chain edge", car, first_row, r1, nodes=[v], winner=False, needs=("route",)))
    out.append(Case("first row of the first chain edge, every node", car, first_row, r1, winner=None, needs=("route",)))
    out.append(Case("first row of the first chain edge, start = 7", car, instant(L + 7, t0 + 7, car.touch(rows[0])), r1, start=7,
                    nodes=[v], winner=False, needs=("route",)))
    # 3: the last row of the last edge at its tau, nowhere near one instant earlier (nor later: the dwell is clear)
    out.append(Case("last row of the last edge", car, instant(L, t0 + R - 1, car.touch(rows[-1])), needs=("route",)))
    # 4: a row of the SECOND edge of v's chain; at the row's time without the first edge's rows the disc is far away -- and the same
    # disc one edge early decides nothing (the foremost hull point: one edge earlier the vehicle has not reached it yet)
    k = lens[0] + int(np.argmax(np.linalg.norm(rows[lens[0]:, :2] - rows[:lens[1], :2], axis=1)))      # where the vehicle was farthest away one edge earlier
    out.append(Case("second edge of the chain", car, instant(L, t0 + k, car.touch(rows[k], True)), nodes=[v], winner=False, needs=("route",)))
    out.append(Case("second edge of the chain, the disc one edge early", car, instant(L, t0 + k - lens[0], car.touch(rows[k], True)), nodes=[v]))
    # 5: the dwell: a disc arrives on the chain's last row at exactly L - 1
    dwell = instant(L, L - 1, car.touch(rows[-1]))
    out.append(Case("dwell conflict at exactly L - 1", car, dwell, nodes=[v], winner=False, needs=("dwell",)))
    out.append(Case("the same track, L - 1 rows", car, dwell[:-1], nodes=[v]))
    # 6: arrival at or after L - 1: the dwell range is empty and late rows clamp to the last table row
    short = t0 + R // 2
    out.append(Case("arrival after L - 1, far discs", car, far(short, 1), nodes=[v]))
    out.append(Case("arrival after L - 1, the last table row on a late chain row", car, instant(short, short - 1, car.touch(rows[R - 3])),
                    nodes=[v], winner=False, needs=("route",)))
    out.append(Case("arrival exactly at L - 1", car, instant(t0 + R, t0 + R - 1, car.touch(rows[-1])), nodes=[v], winner=False,
                    needs=("route",)))
    out.append(Case("start >= L", car, instant(4, 3, car.touch(rows[R - 3])), start=9, nodes=[v], winner=False, needs=("route",)))
    # 7: a candidate below a conflict: a disc on the edge of one of v's ancestors at that row's tau; v's own edge and chain are clear
    path = car.connector().climb(v)
    p = path[-2]
    cum = free["cum"]
    kp = int(car.elen[p]) // 2
    below = instant(L, int(cum[car.pID[p]]) + kp, car.touch(car.xedge[p, kp]))
    out.append(Case("candidate below a conflict", car, below, winner=None, needs=("excluded",)))
    out.append(Case("candidate below a conflict, listed alone", car, below, nodes=[v], winner=False, needs=("excluded",)))
    # 8: a disc on the root's row at tau = start
    out.append(Case("disc on the root's row", car, instant(L, 0, car.touch(car.xedge[0, 0])), winner=False, needs=("excluded",)))
    out.append(Case("disc on the root's row one instant late", car, instant(L, 1, car.touch(car.xedge[0, 0])), winner=None))
    # 9: the chain must beat the best clear hit: the prefix extended by its first goal node
    hit = fixture_tree("car_2000", 218)
    ref = clear_connect(hit, far(1), 0.3, 0)
    b = ref["stats"]["best_end"]
    assert b == 217 and ref["incumbent"] == hit.connector().depths()[b]
    Lh = int(ref["cum"][b]) + 10
    out.append(Case("a chain strictly shorter than the best clear hit", hit, far(Lh, 2)))
    ties = sorted(u for u, w in ref["verdicts"].items() if w[0] == "clear" and w[1] == ref["incumbent"])
    assert ties, "no chain costs exactly what the best clear hit does"
    out.append(Case("a chain that only ties with the best clear hit", hit, far(Lh, 2), nodes=ties, winner=False))
    # 10: a tie between two clear chains: the smaller id wins, whatever the order of the list
    # (the prefix of 217 offers no two chains of equal cost; a longer one does, behind goal hits that a disc each crosses)
    longer = fixture_tree("car_2000", TIE_PREFIX)
    crossed = cross_hits(longer, extra=9 * longer.H)
    by_cost = {}
    for u, w in sorted(clear_connect(longer, crossed, 0.3, 0)["verdicts"].items()):
        if w[0] == "clear":
            by_cost.setdefault(w[1], []).append(u)
    pair = next(us for _, us in sorted(by_cost.items()) if len(us) >= 2)
    out.append(Case("tie: the smaller id wins", longer, crossed, nodes=[pair[1], pair[0]]))
    # 11: disc counts on case 3, where the winner moves
    last_row = instant(L, t0 + R - 1, car.touch(rows[-1]))
    for D, last in ((64, True), (65, True), (65, False)):
        out.append(Case("last row, D = %d, the deciding disc %s" % (D, "last" if last else "first"), car, with_far(last_row, D - 1, last),
                        needs=("route",)))
    # 12: L = 1: every row is tested against the one table row
    out.append(Case("L = 1, far", car, far(1, 1)))
    out.append(Case("L = 1, a disc on a chain row", car, instant(1, 0, car.touch(rows[R - 3])), nodes=[v], winner=False, needs=("route",)))
    # 13: another system on the CPU: a prefix of boat_advanced_3000 (the speed box comes before the hull)
    boat = fixture_tree("boat_advanced_3000", BOAT_PREFIX)
    out.extend(generic_cases(boat, "boat_advanced"))
    # ... whose chains all leave from goal hits: the best hit is caught while it waits, 20 instants after it has arrived, so that it is
    # no clear hit and still a candidate; its chain waits next to it
    pb = plain(boat)
    b = pb["stats"]["best_end"]
    tb = int(pb["cum"][b]) + 20
    caught = instant(tb + 40, tb, boat.touch(boat.xedge[b, boat.elen[b] - 1]))
    caught[tb:] = caught[tb]
    out.append(Case("boat_advanced: the best hit caught while it waits", boat, caught, winner=None, needs=("dwell",)))
    return out


BOAT_PREFIX = 600
TIE_PREFIX = 446


def case(name):
    for c in cases():
        if c.name == name:
            return c
    raise KeyError(name)
