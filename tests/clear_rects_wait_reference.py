"""
Reference of the clearance query against moving oriented rectangles with departure delays (Engine.tree_clear_rects_wait /
Planner.avoid_rects(max_wait), csrc/clear_rects_wait.hpp) in plain NumPy, on top of tests/clear_rects_reference.py and
tests/clear_wait_reference.py, which it leaves alone.

The rule takes nothing new.  It is clear_wait_reference's rule, items 1 to 6 -- the wait on the root's row (root_ok, prefix-closed),
the edges (own_ok), the root path (clear = own_ok & clear of the parent), the dwell (dwell_ok), the best (the smallest
(w + cum[i], i) over hits and the bits of clear & dwell_ok) and the counters -- with "the row test" read as clear_rects_reference's:
the hull points of the row's pose (the novice boats: the centre against extents grown by half the boat length) in the rectangles of
its instant, point in rectangle with the edge included, geometry only.

clear_rects_wait() below is W runs of clear_rects_reference.clear_rects at start + w, composed exactly as
clear_wait_reference.clear_wait composes the disc runs: bit w of clear[i] is (first[i] == -1 of run w) and root_ok bit w, where
root_ok bit w is that the root's own row passed in the runs 0 .. w; bit w of dwell_ok[i] is dwell_first[i] == -1 of run w.
clear_rects_wait_direct() is the rule written out, one pass, all delays of a node in one call of the row test.

CASES: every case of clear_rects_reference.cases() with W = 8, and the hand-built ones of the delays' own edges -- the additions of
clear_wait_reference.cases(), built with rectangles.
"""
import functools

import numpy as np

import clear_reference as cl
import clear_rects_reference as cr
import clear_wait_reference as cw
from clear_wait_reference import STAT_KEYS, all_mask, degenerate, SPINE_HITS, spine_hit_nodes      # noqa: F401


def compose(runs, pID, W):
    """clear_wait_reference.clear_wait's composition of W plain runs (dicts of cum, own_first, first, dwell_first, hit, stats), with
    its assertions of rule 3 and of clear_now == run 0's clear_hits."""
    N = len(runs[0]["cum"])
    cum, hit = runs[0]["cum"], runs[0]["hit"]
    root_ok, alive = 0, True
    for w in range(W):
        alive = alive and runs[w]["own_first"][0] == -1
        root_ok |= int(alive) << w
    own, clear, dwell = [0] * N, [0] * N, [0] * N
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
    stats = _stats(N, hit, clear, dwell, cum, best)
    assert stats["clear_now"] == runs[0]["stats"]["clear_hits"]
    return dict(cum=cum, root_ok=root_ok, own_ok=np.array(own, dtype=np.uint64), clear=np.array(clear, dtype=np.uint64),
                dwell_ok=np.array(dwell, dtype=np.uint64), hit=hit, stats=stats, runs=runs)


def _stats(N, hit, clear, dwell, cum, best):
    return dict(size=N, hits=int(np.sum(hit)), clear_hits=sum(1 for i in range(N) if hit[i] and clear[i] & dwell[i]),
                clear_now=sum(1 for i in range(N) if hit[i] and clear[i] & dwell[i] & 1),
                best_end=-1 if best is None else best[1], best_wait=-1 if best is None else best[2],
                best_steps=-1 if best is None else int(cum[best[1]]), best_arrival=-1 if best is None else best[0])


def clear_rects_wait(state, pID, elen, xedge, test, tracks, extents, start, W, goal_lo, goal_hi):
    """clear_rects_reference.clear_rects's arguments and W.  Returns clear_wait_reference.clear_wait's dict."""
    assert int(W) == W and 1 <= W <= 64
    return compose([cr.clear_rects(state, pID, elen, xedge, test, tracks, extents, start + w, goal_lo, goal_hi) for w in range(W)], pID, W)


def _bits(flags):
    return sum(1 << w for w, f in enumerate(flags) if f)


def clear_rects_wait_direct(state, pID, elen, xedge, test, tracks, extents, start, W, goal_lo, goal_hi, heading=2):
    """The rule as it stands in clear_wait_reference, one sequential pass, the W delays of a node in one call of the rectangles' row
    test: what the large trees are held against.  tests/test_clear_rects_wait_cpu.py holds it against clear_rects_wait() on every
    hand-built case."""
    assert int(W) == W and 1 <= W <= 64
    state, xedge = np.asarray(state, dtype=np.float64), np.asarray(xedge, dtype=np.float64)
    pID, elen = np.asarray(pID, dtype=np.int64), np.asarray(elen, dtype=np.int64)
    table = cr.rect_table(tracks, extents)
    L = len(table)
    rects_at = lambda taus: table[np.minimum(np.asarray(taus, dtype=np.int64), L - 1)]
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
            ok = test(xedge[0, ks], c[ks], s[ks], rects_at(start + ws))             # the root's row at tau = start + w
            own[0] = clear[0] = _bits(np.logical_and.accumulate(ok))               # ... all of start .. start + w: the prefix
        else:
            p = int(pID[i])
            assert 0 <= p < i
            cum[i] = cum[p] + ln
            ks, w_of = np.tile(np.arange(ln), W), np.repeat(ws, ln)
            ok = test(xedge[i, ks], c[ks], s[ks], rects_at(start + w_of + cum[p] + ks))
            own[i] = _bits(ok.reshape(W, ln).all(axis=1))
            clear[i] = own[i] & clear[p]
        hit[i] = i > 0 and bool(np.all((goal_lo < state[i]) & (state[i] < goal_hi)))
        if hit[i]:
            first = start + int(cum[i])                                            # the first instant of the wait at delay 0
            taus = np.arange(first, L)
            if len(taus):
                R = len(taus)
                ok = test(np.repeat(xedge[i, ln - 1:ln], R, axis=0), np.repeat(c[ln - 1], R), np.repeat(s[ln - 1], R), rects_at(taus))
                suffix = np.logical_and.accumulate(ok[::-1])[::-1]                 # suffix[j]: every tau' in [first + j, L - 1] passes
                dwell[i] = _bits([w >= R or bool(suffix[w]) for w in range(W)])    # (w >= R: the range is empty)
            else:
                dwell[i] = all_mask(W)
            m = clear[i] & dwell[i]
            if m:
                w = (m & -m).bit_length() - 1
                if best is None or (w + int(cum[i]), i) < best[:2]:
                    best = (w + int(cum[i]), i, w)
    return dict(cum=cum, root_ok=own[0], own_ok=np.array(own, dtype=np.uint64), clear=np.array(clear, dtype=np.uint64),
                dwell_ok=np.array(dwell, dtype=np.uint64), hit=hit, stats=_stats(N, hit, clear, dwell, cum, best))


def culled(test, reach, grow=0.0):
    """`test` for rows most of which no rectangle can reach: every vehicle point is within `reach` of the pose and every point of a
    rectangle within its half diagonal hypot(a + grow, b + grow) of its centre (grow: what the novice boats' test adds to the
    extents), so a row whose pose is more than reach + half diagonal + 1e-6 from every centre passes; every other row goes
    through `test` unchanged.  The rectangles' test looks at nothing but the rectangles: there is no rest."""
    def rows(X, c, s, rects):
        X, c, s = np.asarray(X), np.asarray(c), np.asarray(s)
        gap = np.hypot(X[:, None, 0] - rects[:, :, 0], X[:, None, 1] - rects[:, :, 1]) - np.hypot(rects[:, :, 4] + grow, rects[:, :, 5] + grow)
        near = np.any(gap <= reach + 1e-6, axis=1)
        out = np.ones(len(X), dtype=bool)
        if near.any():
            out[near] = test(X[near], c[near], s[near], rects[near])
        return out
    return rows


def culled_test_of(system):
    """clear_rects_reference.row_test_of(system) behind culled()."""
    if type(system).__name__ in ("BoatNovice", "BoatNoviceLqr"):
        return culled(cr.row_test_of(system), 0.0, grow=system.boat_length / 2)
    return culled(cr.row_test_of(system), float(np.max(np.hypot(*np.asarray(system.vps, dtype=np.float64).reshape(2, -1)))))


# ------------------------------------------------------------------------------------------------ cases

class WaitCase(object):
    """A clear_rects_reference.Case and a W; `none`: nothing becomes clear by waiting (or nothing conflicts)."""

    def __init__(self, case, W, none=False):
        self.case, self.W, self.none = case, int(W), none
        self.name = "%s | W = %d" % (case.name, W)

    @functools.lru_cache(maxsize=None)
    def reference(self):
        c, t = self.case, self.case.tree
        lo, hi = t.box()
        return clear_rects_wait(t.state, t.pID, t.elen, t.xedge, c.test(), c.tracks, c.extents, c.start, self.W, lo, hi)

    @functools.lru_cache(maxsize=None)
    def disc_reference(self):
        """clear_wait_reference's answer for the covering discs on the same centre tracks."""
        c, t = self.case, self.case.tree
        lo, hi = t.box()
        return cw.clear_wait(t.state, t.pID, t.elen, t.xedge, cl.Case.test(c), c.tracks[:, :, :2], c.radii, c.start, self.W, lo, hi)


# Of clear_rects_reference.cases() at W = 8: the ones where no wait of 0 .. 7 rows changes anything.  This tuple is the cap: a case
# outside it that lacks a partial mask or a hit that is clear only after a wait fails tests/test_clear_rects_wait_cpu.py.
UNCHANGED = ("fork, a 6 x 0.4 rectangle passes beside the short branch",     # heading 0: it never touches the short branch, best (2, 0, 11)
             "fork, the rectangle has passed (start = 4)",
             "fork, dwell conflict at L - 1, the long branch arrives later",
             "fork, L = 8: the crossing is the last row (tau = L - 1)",      # parked on the short branch from tau = 7 on
             "fork, L = 7: the rectangle stops short, tau = L is clamped",   # parked below it: nothing conflicts
             "fork, start >= L",
             "fork, L = 1: the square stands on the short branch",
             "edge: |xi| one ulp beyond a", "edge: |eta| one ulp beyond b",  # nothing conflicts
             # the two deep trees (more than 60 nodes): the square on the root, and the one that stands on spine node 1 at tau = 1
             # and covers the root as well (root_ok = 0b1), as the discs of clear_wait_reference.UNCHANGED
             "chain of 256, conflict on the root", "N = 257, the spine blocked at node 1")

SPINE_E = (0.01, 0.01)                                              # the squares of the spine cases: half side 1 cm, heading 0


def _once(L, at, x, y, heading=0.0):
    """A rectangle that is far away except at row `at`, where its centre stands on (x, y): (L, 3)."""
    t = cl.parked(L, 80.0, 80.0)
    t[at] = (float(x), float(y))
    return cr.with_heading(t, heading)


def _spine_tracks(tree, spine):
    """clear_wait_reference._spine_tracks with squares of half side 1 cm at heading 0 for its discs of radius 1 cm: square d stands
    exactly on the position of spine node j_d -- on a hull point at that pose -- at tau = j_d + w_d, and is far away at every other
    instant.  What is said there of the hull's 0.25 m lattice and the 0.05 m steps holds for a square inside the disc's bounding
    box as well: every other node is at least 0.05 m off a hull point along x, five times the half side."""
    L = spine + 12
    return np.stack([_once(L, j + w, tree.xedge[j, 0, 0], tree.xedge[j, 0, 1]) for j, (_, w) in zip(spine_hit_nodes(spine), SPINE_HITS)], axis=1)


def _with_root_hit(case, name, at, start=0):
    """`case` with one more square, on the root at row `at` only."""
    L = len(case.tracks)
    tracks = np.concatenate((case.tracks, _once(L, at, 0.0, 0.0)[:, None, :]), axis=1)
    return cr.Case(name, case.tree, tracks, np.concatenate((case.extents, [cr.SQUARE])), start=start)


TIE_WAIT = 5                                                         # 11 + 5 = 16: the short branch's arrival equals the long one's


@functools.lru_cache(maxsize=None)
def cases():
    out = [WaitCase(c, 8, none=c.name in UNCHANGED) for c in cr.cases()]
    ch = lambda L, at=7: cr.with_heading(cl.crossing(L, at=at), np.pi / 2)
    # the root fails at tau = start + 3 only: root_ok = 0b111, every mask within it; the crossing square makes waiting pay
    out.append(WaitCase(_with_root_hit(cr._fork("", parked=False), "fork, the root is hit at start + 3", 3), 8))
    out.append(WaitCase(_with_root_hit(cr._fork("", parked=False, cross=ch(20, 9)), "fork, start = 2, the root is hit at start + 3", 5, start=2), 8))
    # W = 64 and 63: L = 80, one square crosses the short branch at x = 7 at row 7 (delay 0 meets it) and one late, at row 66, when
    # the vehicle that left 59 rows late is there; bit 63 exists only where W = 64
    two = cr._fork("", L=80, parked=False)
    tr = np.concatenate((two.tracks, ch(80, 66)[:, None, :]), axis=1)
    for W in (64, 63):
        out.append(WaitCase(cr.Case("fork, L = 80, squares cross at rows 7 and 66", two.tree, tr, cr.SQUARE), W))
    # few delays: wavefronts without a delay (W = 2, 3), an uneven share (W = 5)
    for W in (2, 3, 5):
        out.append(WaitCase(cr.case("fork, the rectangle crosses the short branch"), W))
    # the clamp: with start = L - 2 the root's delay 0 reads row L - 2 and every later one row L - 1
    for name in ("fork, L = 8: the crossing is the last row (tau = L - 1)", "fork, L = 7: the rectangle stops short, tau = L is clamped"):
        c = cr.case(name)
        L = len(c.tracks)
        out.append(WaitCase(cr.Case(name + ", start = L - 2", c.tree, c.tracks, c.extents, start=L - 2), 8, none=True))
    # two rows longer: delay 0 meets the square on the short branch at tau = 7, the rows of the later delays run past L - 1 = 9 and
    # see it parked at (7, 2), clear of them
    out.append(WaitCase(cr._fork("fork, L = 10, start = 0: delays on both sides of the clamp", L=10), 8))
    # dwell suffix: dwell_ok of node 2 is exactly the delays with start + w + 11 > 13
    out.append(WaitCase(cr._fork("fork, dwell conflict at L - 1 (suffix)", L=14, cross=cr._dwell_track(14)), 8, none=True))
    # a hit that arrives after L - 1 at every delay: the dwell range is empty, dwell_ok is all ones (L = 8, start = 0: cum >= 11);
    # the square crosses node 1's edge at x = 3 at row 3, where delay 0 meets it, and parks at (3, 4)
    early = cr.with_heading(cl.crossing(8, x=3.0, at=3), np.pi / 2)
    out.append(WaitCase(cr._fork("fork, L = 8, every hit arrives after L - 1", L=8, cross=early, parked=False), 8))
    # the tie: the square parks on the short branch at (7, 0) and leaves at row 12 -- the vehicle of delay w is at x = 7 at
    # tau = w + 7, so w = 0 .. 4 meet it and w = 5 arrives at 16, exactly when the long branch (node 5, 16 steps) does at delay 0
    tie = cr.with_heading(cl.parked(20, 7.0, 0.0), 0.0)
    tie[7 + TIE_WAIT:, :2] = (50.0, 50.0)
    out.append(WaitCase(cr._fork("fork, a tie: wait 5 on the short branch arrives with the long one", cross=tie, parked=False), 8))
    # what a disc cannot say, with time: the 6 x 0.4 rectangle across the short branch
    out.append(WaitCase(cr._fork("fork, a 6 x 0.4 rectangle at heading pi/2 crosses the short branch", e_cross=(3.0, 0.2), parked=False), 8))
    # AND over deep chains: a square stands on spine node j at one instant, for three j; different ancestors remove different bits
    for N in (255, 256, 257):
        t = cl.spine_and_branch(N)
        out.append(WaitCase(cr.Case("N = %d, three spine nodes hit at one instant each" % N, t, _spine_tracks(t, N - 4), SPINE_E), 8))
    deep = cr.case("chain of 256, conflict on the root").tree
    out.append(WaitCase(cr.Case("chain of 256, three nodes hit at one instant each", deep, _spine_tracks(deep, 255), SPINE_E), 8))
    out.append(WaitCase(cr.Case("chain of 256, the root fails at start + 1", deep, _once(4, 1, 0.0, 0.0), cr.SQUARE), 8, none=True))
    return out


def case(name):
    for c in cases():
        if c.name == name:
            return c
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------ fixture trees

FIXTURE_W = 16


@functools.lru_cache(maxsize=None)
def fixture_reference(name):
    f = cl.fixture(name)
    s = f.native()
    lo, hi = f.box(s)
    tracks, extents = cr.fixture_tracks(f)
    return clear_rects_wait_direct(f.state, f.pID, f.elen, f.xedge, culled_test_of(s), tracks, extents, 0, FIXTURE_W, lo, hi)
