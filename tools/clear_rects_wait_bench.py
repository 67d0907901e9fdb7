"""
Time of the rectangle clearance query with departure delays (Engine.tree_clear_rects_wait: the device call of
Planner.avoid_rects(max_wait)) on the grown boat_advanced trees of tools/clear_bench.py, next to
  (i)  what it replaces in the same process: W successive calls of the plain rectangle query, Engine.tree_clear_rects at start + w
       (its code is untouched by the wait call), and
  (ii) the disc query with delays, Engine.tree_clear_wait, on the same centre tracks with the radii that cover the rectangles.
The D rectangles are tools/clear_rects_bench.py's: 6 m x 0.4 m, on clear_bench's straight lines for L = 600 instants, heading
along their motion.  (i) must give the same per-node answers (bit w of clear: first == -1 of call w, joined with root_ok; bit w of
dwell_ok: dwell_first == -1 of call w).  On trees of up to `--host-max` nodes, with W <= 16, masks and counters are also held
against the direct form of tests/clear_rects_wait_reference.py before anything is timed.  Times are host wall clock around the
synchronous calls (argument checks, table upload, every launch and the read-back of both per-node arrays included), warmed, median
of `--reps` with the lowest and the highest.

    python tools/clear_rects_wait_bench.py [--nodes 10000,100000] [--rects 15,63] [--waits 16,64] [--reps 3] [--host-max 0] [--out DIR]
                                                            ->  one JSON line per (nodes, D, W); DIR/clear_rects_wait_bench.jsonl
    python tools/clear_rects_wait_bench.py --once --nodes 100000 --rects 15 --waits 16
                                                            ->  one untimed call of each of the three queries (for a kernel trace)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import clear_bench as cb                               # noqa: E402
from clear_rects_bench import rects_of, timed          # noqa: E402
from clear_wait_bench import joined                    # noqa: E402
import clear_rects_wait_reference as rw                # noqa: E402
import retain_reference as rr                          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", default="10000,100000")
    ap.add_argument("--rects", default="15,63")
    ap.add_argument("--waits", default="16,64")
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
            for W in [int(v) for v in a.waits.split(",")]:
                if a.once:
                    print(json.dumps(dict(nodes=N, rects=D, waits=W, rect_wait=eng.tree_clear_rects_wait(tracks, extents, 0, W),
                                          disc_wait=eng.tree_clear_wait(centres, radii, 0, W), rect=eng.tree_clear_rects(tracks, extents, 0))),
                          flush=True)
                    continue
                held = None
                if N <= a.host_max + 1 and W <= 16:
                    state, _, pID, elen, xedge, _ = rr.engine_arrays(eng)
                    ref = rw.clear_rects_wait_direct(state, pID, elen, xedge, rw.culled_test_of(s), tracks, extents, 0, W, lo, hi)
                    got = eng.tree_clear_rects_wait(tracks, extents, 0, W, per_node=True)
                    assert got[0] == ref["stats"] and np.array_equal(got[1], ref["clear"]) and np.array_equal(got[2], ref["dwell_ok"])
                    held = "equal"
                one, t_one = timed(lambda: eng.tree_clear_rects_wait(tracks, extents, 0, W, per_node=True), a.reps)
                many, t_many = timed(lambda: [eng.tree_clear_rects(tracks, extents, w, per_node=True) for w in range(W)], a.reps)
                many = joined(many)
                assert np.array_equal(one[1], many[0]) and np.array_equal(one[2], many[1])
                disc, t_disc = timed(lambda: eng.tree_clear_wait(centres, radii, 0, W, per_node=True), a.reps)
                st = one[0]
                full = np.uint64(rw.all_mask(W))
                med = lambda ts: round(float(np.median(ts)), 3)
                row = dict(case="boat_advanced grown", nodes=N, rects=D, instants=cb.L, waits=W, hits=st["hits"], clear_hits=st["clear_hits"],
                           clear_now=st["clear_now"], best_wait=st["best_wait"], nodes_all_clear=int(np.sum(one[1] == full)),
                           nodes_none_clear=int(np.sum(one[1] == 0)),
                           one_call_ms=med(t_one), one_call_ms_min=round(min(t_one), 3), one_call_ms_max=round(max(t_one), 3),
                           w_calls_ms=med(t_many), w_calls_ms_min=round(min(t_many), 3), w_calls_ms_max=round(max(t_many), 3),
                           disc_wait_ms=med(t_disc), disc_wait_ms_min=round(min(t_disc), 3), disc_wait_ms_max=round(max(t_disc), 3),
                           disc_clear_hits=disc[0]["clear_hits"], disc_best_wait=disc[0]["best_wait"])
                row["w_calls_over_one"] = round(row["w_calls_ms"] / row["one_call_ms"], 2)
                row["rect_over_disc"] = round(row["one_call_ms"] / row["disc_wait_ms"], 2)
                if held:
                    row["reference"] = held
                rows.append(row)
                print(json.dumps(row), flush=True)
        eng.close()
    if a.out and rows:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "clear_rects_wait_bench.jsonl"), "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    main()
