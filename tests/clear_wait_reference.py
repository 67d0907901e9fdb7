"""
Reference of the clearance query with departure delays (Engine.tree_clear_wait / Planner.avoid(max_wait), csrc/clear_wait.hpp) in
plain NumPy, on top of tests/clear_reference.py, which it leaves alone.

The rule.  Everything of clear_reference holds (cum, tau, the clamp min(tau, L - 1), the row test, the goal hit), and there is one
more integer W, 1 <= W <= 64: the delays w = 0 .. W - 1 in rows of dt.  For delay w:

  1. Wait.  The vehicle holds the root's row from tau = start through start + w; the root's row is tested at each of those w + 1
     instants.  root_ok bit w = all of them pass: root_ok is prefix-closed.
  2. Edges.  Row k of node i > 0 has tau = start + w + cum[pID[i]] + k; own_ok[i] bit w = every row of i's edge passes;
     own_ok[0] = root_ok.
  3. Root path.  clear[i] = own_ok[i] & clear[pID[i]].
  4. Dwell.  For a goal hit dwell_ok[i] bit w = its last row passes at every tau' in [start + w + cum[i], L - 1] (an empty range
     passes); 0 for every other node.
  5. Best.  Over hits i and delays w set in clear[i] & dwell_ok[i]: the smallest (w + cum[i], i).
  6. Counters.  size, hits, clear_hits (hits with clear & dwell_ok != 0), clear_now (hits with bit 0 set in both), best_end,
     best_wait, best_steps (= cum[best_end]), best_arrival; -1 without a best.

clear_wait() below is W runs of clear_reference.clear at start + w: bit w of clear[i] is (first[i] == -1 of run w) and root_ok bit
w, where root_ok bit w is that the root's own row passed in the runs 0 .. w (run v tests it at tau = start + v); bit w of
dwell_ok[i] is dwell_first[i] == -1 of run w.

CASES: every case of clear_reference.cases() with W = 8, and the hand-built ones of the delays' own edges.
"""
import functools

import numpy as np

import clear_reference as cl

STAT_KEYS = ("size", "hits", "clear_hits", "clear_now", "best_end", "best_wait", "best_steps", "best_arrival")


def all_mask(W):
    return (1 << W) - 1


def clear_wait(state, pID, elen, xedge, test, tracks, radii, start, W, goal_lo, goal_hi):
    """clear_reference.clear's arguments and W.  Returns dict(cum, root_ok (int), own_ok, clear, dwell_ok (uint64 [N]), hit,
    stats, runs -- the W results of clear_reference.clear)."""
    assert int(W) == W and 1 <= W <= 64
    runs = [cl.clear(state, pID, elen, xedge, test, tracks, radii, start + w, goal_lo, goal_hi) for w in range(W)]
    N = len(runs[0]["cum"])
    cum, hit = runs[0]["cum"], runs[0]["hit"]
    root_ok, alive = 0, True
    for w in range(W):
        alive = alive and runs[w]["own_first"][0] == -1
        root_ok |= int(alive) << w
    own = [0] * N
    clear = [0] * N
    dwell = [0] * N
    for w in range(W):
        r = runs[w]
        for i in range(N):
            if i > 0 and r["own_first"][i] == -1:
                own[i] |= 1 << w
            if r["first"][i] == -1 and (root_ok >> w) & 1:
                clear[i] |= 1 << w
            if hit[i] and r["dwell_first"][i] == -1:
                dwell[i] |= 1 << w
    own[0] = root_ok
    for i in range(1, N):                                           # rule 3 as it is written, against the composition above
        assert clear[i] == own[i] & clear[int(pID[i])], i
    assert clear[0] == root_ok
    best = None
    for i in range(N):
        m = clear[i] & dwell[i]
        if hit[i] and m:
            w = (m & -m).bit_length() - 1                           # of one node only its lowest set bit can win
            if best is None or (w + int(cum[i]), i) < best[:2]:
                best = (w + int(cum[i]), i, w)
    stats = dict(size=N, hits=int(np.sum(hit)), clear_hits=sum(1 for i in range(N) if hit[i] and clear[i] & dwell[i]),
                 clear_now=sum(1 for i in range(N) if hit[i] and clear[i] & dwell[i] & 1),
                 best_end=-1 if best is None else best[1], best_wait=-1 if best is None else best[2],
                 best_steps=-1 if best is None else int(cum[best[1]]), best_arrival=-1 if best is None else best[0])
    assert stats["clear_now"] == runs[0]["stats"]["clear_hits"]
    return dict(cum=cum, root_ok=root_ok, own_ok=np.array(own, dtype=np.uint64), clear=np.array(clear, dtype=np.uint64),
                dwell_ok=np.array(dwell, dtype=np.uint64), hit=hit, stats=stats, runs=runs)


def _bits(flags):
    return sum(1 << w for w, f in enumerate(flags) if f)


def clear_wait_direct(state, pID, elen, xedge, test, tracks, radii, start, W, goal_lo, goal_hi, heading=2):
    """The same rule written out as it stands above, one sequential pass, the W delays of a node in one call of the row test: what
    the large fixture trees are held against (W runs of clear_reference.clear over 3 000 nodes take a minute).
    tests/test_clear_wait_cpu.py holds it against clear_wait() on every hand-built case."""
    assert int(W) == W and 1 <= W <= 64
    state, xedge = np.asarray(state, dtype=np.float64), np.asarray(xedge, dtype=np.float64)
    pID, elen = np.asarray(pID, dtype=np.int64), np.asarray(elen, dtype=np.int64)
    tracks = np.asarray(tracks, dtype=np.float64)
    L, D = tracks.shape[:2]
    radii = np.broadcast_to(np.asarray(radii, dtype=np.float64), (D,))
    table = np.concatenate((tracks, np.broadcast_to(radii[None, :, None], (L, D, 1))), axis=2)
    discs_at = lambda taus: table[np.minimum(np.asarray(taus, dtype=np.int64), L - 1)]
    N = len(state)
    ws = np.arange(W, dtype=np.int64)
    cum = np.zeros(N, dtype=np.int64)
    hit = np.zeros(N, dtype=bool)
    own, clear, dwell = [0] * N, [0] * N, [0] * N
    best = None
    for i in range(N):
        ln = int(elen[i])
        c, s = cl.portable_sincos(xedge[i, :ln, heading])
        if i == 0:
            cum[0] = ln
            ks = np.full(W, ln - 1)
            ok = test(xedge[0, ks], c[ks], s[ks], discs_at(start + ws))            # the root's row at tau = start + w
            own[0] = clear[0] = _bits(np.logical_and.accumulate(ok))              # ... all of start .. start + w: the prefix
        else:
            p = int(pID[i])
            assert 0 <= p < i
            cum[i] = cum[p] + ln
            ks, w_of = np.tile(np.arange(ln), W), np.repeat(ws, ln)
            ok = test(xedge[i, ks], c[ks], s[ks], discs_at(start + w_of + cum[p] + ks))
            own[i] = _bits(ok.reshape(W, ln).all(axis=1))
            clear[i] = own[i] & clear[p]
        hit[i] = i > 0 and bool(np.all((goal_lo < state[i]) & (state[i] < goal_hi)))
        if hit[i]:
            first = start + int(cum[i])                                           # the first instant of the wait at delay 0
            taus = np.arange(first, L)
            if len(taus):
                R = len(taus)
                ok = test(np.repeat(xedge[i, ln - 1:ln], R, axis=0), np.repeat(c[ln - 1], R), np.repeat(s[ln - 1], R), discs_at(taus))
                suffix = np.logical_and.accumulate(ok[::-1])[::-1]                # suffix[j]: every tau' in [first + j, L - 1] passes
                dwell[i] = _bits([w >= R or bool(suffix[w]) for w in range(W)])   # (w >= R: the range is empty)
            else:
                dwell[i] = all_mask(W)
            m = clear[i] & dwell[i]
            if m:
                w = (m & -m).bit_length() - 1
                if best is None or (w + int(cum[i]), i) < best[:2]:
                    best = (w + int(cum[i]), i, w)
    stats = dict(size=N, hits=int(np.sum(hit)), clear_hits=sum(1 for i in range(N) if hit[i] and clear[i] & dwell[i]),
                 clear_now=sum(1 for i in range(N) if hit[i] and clear[i] & dwell[i] & 1),
                 best_end=-1 if best is None else best[1], best_wait=-1 if best is None else best[2],
                 best_steps=-1 if best is None else int(cum[best[1]]), best_arrival=-1 if best is None else best[0])
    return dict(cum=cum, root_ok=own[0], own_ok=np.array(own, dtype=np.uint64), clear=np.array(clear, dtype=np.uint64),
                dwell_ok=np.array(dwell, dtype=np.uint64), hit=hit, stats=stats)


def degenerate(res, W):
    """What a case lacks of: a mask that is neither 0 nor all-ones, a hit whose lowest clear delay is > 0."""
    lacks = []
    full = all_mask(W)
    if not any(0 < int(m) < full for m in res["clear"]):
        lacks.append("partial mask")
    both = [int(c) & int(d) for c, d, h in zip(res["clear"], res["dwell_ok"], res["hit"]) if h]
    if not any(m and not m & 1 for m in both):
        lacks.append("hit that is clear only after a wait")
    return lacks


# ------------------------------------------------------------------------------------------------ cases

class WaitCase(object):
    """A clear_reference.Case and a W; `none`: nothing becomes clear by waiting (or nothing conflicts)."""

    def __init__(self, case, W, name=None, none=False):
        self.case, self.W, self.none = case, int(W), none
        self.name = "%s | W = %d" % (case.name if name is None else name, W)

    @functools.lru_cache(maxsize=None)
    def reference(self):
        c, t = self.case, self.case.tree
        lo, hi = t.box()
        return clear_wait(t.state, t.pID, t.elen, t.xedge, c.test(), c.tracks, c.radii, c.start, self.W, lo, hi)


def _once(L, at, x, y):
    """A disc that is far away except at row `at`, where it stands on (x, y): (L, 2)."""
    t = cl.parked(L, 80.0, 80.0)
    t[at] = (float(x), float(y))
    return t


# Of clear_reference.cases(): the ones where no wait of 0 .. 7 rows changes anything -- the hand-computed table of the issue (the
# best stays what it is) and the cases that exist to show `none`.
UNCHANGED = ("N=1, a disc on the root", "N=1, nothing near", "fork, the disc has passed (start = 4)",
             "fork, dwell conflict at L - 1, the long branch arrives later", "fork, L = 8: the crossing is the last row (tau = L - 1)",
             "fork, L = 7: the disc stops short, tau = L is clamped", "fork, start >= L",
             "L = 1, D = 1, two clear hits with equal steps", "chain of 33, conflict at node 1", "chain of 256, conflict on the root",
             # the disc that stands on spine node 1 at tau = 1 covers the root as well: root_ok = 0b1, waiting is not possible
             "N = 255, the spine blocked at node 1", "N = 256, the spine blocked at node 1", "N = 257, the spine blocked at node 1")


@functools.lru_cache(maxsize=None)
def cases():
    out = [WaitCase(c, 8, none=c.name in UNCHANGED) for c in cl.cases()]
    fork = lambda: cl.HandTree("boat_advanced", cl.fork_nodes())
    # the root fails at tau = start + 3 only: root_ok = 0b111, every mask within it; the crossing disc makes waiting pay
    tr = np.stack((cl.crossing(20), _once(20, 3, 0.0, 0.0)), axis=1)
    out.append(WaitCase(cl.Case("fork, the root is hit at start + 3", fork(), tr, 0.4), 8))
    tr = np.stack((cl.crossing(20, at=9), _once(20, 5, 0.0, 0.0)), axis=1)
    out.append(WaitCase(cl.Case("fork, start = 2, the root is hit at start + 3", fork(), tr, 0.4, start=2), 8))
    # W = 64 and 63: L = 80, one disc crosses the short branch at x = 7 at row 7 (delay 0 meets it) and one late, at row 66, when
    # the vehicle that left 59 rows late is there -- the delays 60 .. 63 are clear again, and bit 63 exists only where W = 64
    tr = np.stack((cl.crossing(80), cl.crossing(80, at=66)), axis=1)
    for W in (64, 63):
        out.append(WaitCase(cl.Case("fork, L = 80, discs cross at rows 7 and 66", fork(), tr, 0.4), W))
    # the clamp memo: for some rows part of the delays are before L - 1 and part are clamped
    for name in ("fork, L = 8: the crossing is the last row (tau = L - 1)", "fork, L = 7: the disc stops short, tau = L is clamped"):
        c = cl.case(name)
        L = len(c.tracks)
        out.append(WaitCase(cl.Case(name + ", start = L - 2", c.tree, c.tracks, c.radii, start=L - 2), 8, none=True))
    # the same tracks two rows longer: delay 0 meets the disc on the short branch at tau = 7, the rows of the later delays run past
    # L - 1 = 9 and see it parked at (7, 2), clear of them
    out.append(WaitCase(cl._fork_case("fork, L = 10, start = 0: delays on both sides of the clamp", L=10), 8))
    # dwell suffix: dwell_ok of node 2 is exactly the delays with start + w + 11 > 13
    out.append(WaitCase(cl._fork_case("fork, dwell conflict at L - 1 (suffix)", L=14, cross=cl._dwell_track(14)), 8, none=True))
    # AND over deep chains: a disc stands on spine node j at one instant, for three j; different ancestors remove different bits
    for N in (255, 256, 257):
        t = cl.spine_and_branch(N)
        tr = _spine_tracks(t, N - 4)
        out.append(WaitCase(cl.Case("N = %d, three spine nodes hit at one instant each" % N, t, tr, SPINE_R), 8))
    row = lambda x, y: (float(x), float(y), 0.0)
    deep = cl.HandTree("boat_advanced", [(-1, [row(0, 0)])] + cl.chain_nodes(255))
    deep.goal[:2] = (0.05 * 255, 0.0)
    out.append(WaitCase(cl.Case("chain of 256, three nodes hit at one instant each", deep, _spine_tracks(deep, 255), SPINE_R), 8))
    out.append(WaitCase(cl.Case("chain of 256, the root fails at start + 1", deep, _once(4, 1, 0.0, 0.0), 0.4), 8, none=True))
    return out


SPINE_HITS = ((0.25, 2), (0.5, 5), (0.75, 1))                       # (where along the spine, the delay that node loses)
SPINE_R = 0.01


def spine_hit_nodes(spine):
    return [max(int(frac * spine), 1) for frac, _ in SPINE_HITS]


def _spine_tracks(tree, spine):
    """Three discs of radius 0.01.  Disc d stands exactly on the position of spine node j_d -- on the hull point at the pose -- at
    tau = j_d + w_d, the instant that node (one row, cum = j_d + 1) has at delay w_d, and is far away at every other instant.  The
    spine steps by 0.05 m and the hull points lie on a 0.25 m lattice 1 m long, so at that instant the disc also sits on a hull
    point of the vehicle 5 or 10 nodes further back or on, which is there at delay w_d + 5 (node j_d - 5) or w_d - 5 (node
    j_d + 5) when that is a delay of the call; every other node is at least 0.05 m off a hull point.  With the delays 2, 5, 1 and
    W = 8: bits 2 and 7, bits 5 and 0, bits 1 and 6 -- each removed at another ancestor; the end of the spine keeps 3 and 4."""
    L = spine + 12
    cols = []
    for j, (_, w) in zip(spine_hit_nodes(spine), SPINE_HITS):
        cols.append(_once(L, j + w, tree.xedge[j, 0, 0], tree.xedge[j, 0, 1]))
    return np.stack(cols, axis=1)


def case(name):
    for c in cases():
        if c.name == name:
            return c
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------ fixture trees

FIXTURE_W = 16


def culled(test, reach, car=False, rest=None):
    """`test` for rows most of which no disc can reach (the fixture trees: thousands of rows of a hull of up to 187 points, four
    discs): a row whose pose is more than `reach` (the farthest hull point from the pose) + r + 1e-6 from every disc centre -- for
    the car also its vertex at 2 p -- cannot touch a disc and is decided by `rest`, the part of the test that does not look at
    the discs (BoatAdvanced's speed box; None: there is none, the row passes).  Every other row goes through `test` unchanged."""
    def rows(X, c, s, discs):
        X, c, s = np.asarray(X), np.asarray(c), np.asarray(s)
        gap = np.hypot(X[:, None, 0] - discs[:, :, 0], X[:, None, 1] - discs[:, :, 1]) - discs[:, :, 2]
        near = np.any(gap <= reach + 1e-6, axis=1)
        if car:
            gap2 = np.hypot(2.0 * X[:, None, 0] - discs[:, :, 0], 2.0 * X[:, None, 1] - discs[:, :, 1]) - discs[:, :, 2]
            near |= np.any(gap2 <= 1e-6, axis=1)
        out = np.empty(len(X), dtype=bool)
        if near.any():
            out[near] = test(X[near], c[near], s[near], discs[near])
        if not near.all():
            out[~near] = True if rest is None else rest(X[~near], c[~near], s[~near], discs[~near])
        return out
    return rows


def culled_test_of(system):
    """clear_reference.row_test_of(system) behind culled()."""
    name = type(system).__name__
    novice = name in ("BoatNovice", "BoatNoviceLqr")
    reach = system.boat_length / 2 if novice else float(np.max(np.hypot(*np.asarray(system.vps, dtype=np.float64).reshape(2, -1))))
    rest = None
    if name == "BoatAdvanced":                                      # the same test with a hull of no points: the speed box alone
        rest = cl.row_test("advanced", np.zeros((2, 0)), speed_box=(np.asarray(system.velmax_pos_plan, dtype=np.float64),
                                                                    np.asarray(system.velmax_neg_plan, dtype=np.float64)))
    return culled(cl.row_test_of(system), reach, car=name == "Car", rest=rest)


@functools.lru_cache(maxsize=None)
def fixture_reference(name):
    f = cl.fixture(name)
    s = f.native()
    lo, hi = f.box(s)
    tracks, radii = f.tracks()
    return clear_wait_direct(f.state, f.pID, f.elen, f.xedge, culled_test_of(s), tracks, radii, 0, FIXTURE_W, lo, hi)
