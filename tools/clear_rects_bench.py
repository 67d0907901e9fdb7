"""
Time of the rectangle clearance query (Engine.tree_clear_rects: Planner.avoid_rects's device call) on the grown boat_advanced trees
of tools/clear_bench.py, next to the disc query (Engine.tree_clear) on the same trees and the same centre tracks with the radii that
cover the rectangles.  The D rectangles are 6 m x 0.4 m (a = 3.0, b = 0.2), move on clear_bench's straight lines for L = 600
instants and head along their motion.  Times are host wall clock around the synchronous calls (argument checks, table upload,
every launch and the read-back of the per-node arrays included), warmed, median of `--reps` with the lowest and the highest;
`rect_turning_ms` is the same call with headings that change at every instant (the host then derives cos / sin per pose).  On
trees of up to `--host-max` nodes the per-node arrays and counters are also held against tests/clear_rects_reference.py.

    python tools/clear_rects_bench.py [--nodes 10000,100000] [--rects 15,63] [--reps 3] [--host-max 0] [--out DIR]
                                                            ->  one JSON line per (nodes, D); DIR/clear_rects_bench.jsonl
    python tools/clear_rects_bench.py --once --nodes 100000 --rects 15   ->  one untimed call of each query (for a kernel trace)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import clear_bench as cb                               # noqa: E402
import clear_rects_reference as cr                     # noqa: E402
import retain_reference as rr                          # noqa: E402

EXTENT = (3.0, 0.2)


def rects_of(D):
    """clear_bench's centre tracks with the heading of each line: (tracks (L, D, 3), extents (D, 2), covering radii (D,))."""
    xy, _ = cb.tracks_of(D)
    step = xy[-1] - xy[0]
    tracks = np.concatenate((xy, np.broadcast_to(np.arctan2(step[:, 1], step[:, 0])[None, :, None], xy.shape[:2] + (1,))), axis=2)
    return np.ascontiguousarray(tracks), np.tile(np.array(EXTENT), (D, 1)), np.full(D, float(np.hypot(*EXTENT)))


def timed(call, reps):
    ts, got = [], None
    for rep in range(reps + 1):                                       # (the first pass warms up and is not counted)
        t0 = time.perf_counter()
        got = call()
        if rep:
            ts.append(1e3 * (time.perf_counter() - t0))
    return got, ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", default="10000,100000")
    ap.add_argument("--rects", default="15,63")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-max", type=int, default=0)
    ap.add_argument("--once", action="store_true", help="one untimed call of each query per configuration (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for nodes in [int(v) for v in a.nodes.split(",")]:
        s, eng = cb.grown(nodes)
        N = eng.size
        lo, hi = rr.goal_box(s)
        for D in [int(v) for v in a.rects.split(",")]:
            tracks, extents, radii = rects_of(D)
            centres = np.ascontiguousarray(tracks[:, :, :2])
            if a.once:
                rect, disc = eng.tree_clear_rects(tracks, extents, 0), eng.tree_clear(centres, radii, 0)
                print(json.dumps(dict(nodes=N, rects=D, rect_stats=rect, disc_stats=disc)), flush=True)
                continue
            rect, tr = timed(lambda: eng.tree_clear_rects(tracks, extents, 0, per_node=True), a.reps)
            disc, td = timed(lambda: eng.tree_clear(centres, radii, 0, per_node=True), a.reps)
            # the same rectangles, slowly turning: every pose has a heading of its own, and the host derives cos / sin for each
            turning = tracks.copy()
            turning[:, :, 2] += 1e-3 * np.arange(cb.L)[:, None]
            _, tt = timed(lambda: eng.tree_clear_rects(turning, extents, 0, per_node=True), a.reps)
            row = dict(case="boat_advanced grown", nodes=N, rects=D, instants=cb.L, extent=list(EXTENT), covering_radius=round(float(radii[0]), 4),
                       rect_ms=round(float(np.median(tr)), 3), rect_ms_min=round(min(tr), 3), rect_ms_max=round(max(tr), 3),
                       disc_ms=round(float(np.median(td)), 3), disc_ms_min=round(min(td), 3), disc_ms_max=round(max(td), 3),
                       rect_over_disc=round(float(np.median(tr) / np.median(td)), 2),
                       rect_turning_ms=round(float(np.median(tt)), 3), rect_turning_ms_min=round(min(tt), 3), rect_turning_ms_max=round(max(tt), 3),
                       rect=dict((k, rect[0][k]) for k in ("conflicts", "blocked", "hits", "clear_hits", "best_steps")),
                       disc=dict((k, disc[0][k]) for k in ("conflicts", "blocked", "hits", "clear_hits", "best_steps")))
            if N <= a.host_max + 1:
                state, _, pID, elen, xedge, _ = rr.engine_arrays(eng)
                ref = cr.clear_rects(state, pID, elen, xedge, cr.row_test_of(s), tracks, extents, 0, lo, hi)
                assert rect[0] == ref["stats"] and np.array_equal(rect[1], ref["first"]) and np.array_equal(rect[2], ref["dwell_first"])
                row["reference"] = "equal"
            rows.append(row)
            print(json.dumps(row), flush=True)
        eng.close()
    if a.out and rows:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "clear_rects_bench.jsonl"), "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    main()
