"""
Time of the clearance query with departure delays (Engine.tree_clear_wait: the device call of Planner.avoid(max_wait)) on grown
boat_advanced trees, next to what it replaces in the same process: W successive calls of the plain query, Engine.tree_clear at
start + w.  Both must give the same per-node answers (bit w of clear: first == -1 of call w, joined with root_ok; bit w of dwell_ok:
dwell_first == -1 of call w).  The workload is tools/clear_bench.py's: D discs on straight lines through the square (8, 48)^2 around
the demo's goal for L = 600 instants, radius 0.5 m; and once more with the same discs moved 400 m away ("far": nothing conflicts, so
no delay of any node ever drops out of the check).  Times are host wall clock around the synchronous calls (argument checks, table
upload, every launch and the read-back of the per-node arrays included), warmed, median of `--reps` with the lowest and the highest.

    python tools/clear_wait_bench.py [--nodes 10000,100000] [--discs 15,63] [--waits 8,16,64] [--where near,far] [--reps 3] [--out DIR]
                                                            ->  one JSON line per (nodes, D, where, W); DIR/clear_wait_bench.jsonl
    python tools/clear_wait_bench.py --once --nodes 100000 --discs 15 --waits 16 --where near   ->  one untimed call (for a kernel trace)
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

from clear_bench import grown, tracks_of                # noqa: E402


def timed(fn, reps):
    ts, out = [], None
    for rep in range(reps + 1):                          # (the first pass warms up and is not counted)
        t0 = time.perf_counter()
        out = fn()
        if rep:
            ts.append(1e3 * (time.perf_counter() - t0))
    return out, ts


def by_calls(eng, tracks, radii, W):
    """The W calls of tree_clear (this is what is timed) ..."""
    return [eng.tree_clear(tracks, radii, w, per_node=True) for w in range(W)]


def joined(calls):
    """... and what one tree_clear_wait call answers, put together from them (not timed)."""
    clear = dwell = None
    alive = True
    for w, (_, first, dfirst) in enumerate(calls):
        if clear is None:
            clear, dwell = np.zeros(len(first), dtype=np.uint64), np.zeros(len(first), dtype=np.uint64)
        alive = alive and first[0] == -1
        clear |= ((first == -1) & alive).astype(np.uint64) << np.uint64(w)
        dwell |= (dfirst == -1).astype(np.uint64) << np.uint64(w)
    return clear, dwell


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", default="10000,100000")
    ap.add_argument("--discs", default="15,63")
    ap.add_argument("--waits", default="8,16,64")
    ap.add_argument("--where", default="near,far", help="near: the discs cross the tree; far: the same discs 400 m away")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--once", action="store_true", help="one untimed device call per configuration (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for nodes in [int(v) for v in a.nodes.split(",")]:
        s, eng = grown(nodes)
        N = eng.size
        for D in [int(v) for v in a.discs.split(",")]:
            near, radii = tracks_of(D)
            for where, tracks in (("near", near), ("far", near + 400.0)):
                if where not in a.where.split(","):
                    continue
                for W in [int(v) for v in a.waits.split(",")]:
                    if a.once:
                        print(json.dumps(dict(nodes=N, discs=D, where=where, waits=W, stats=eng.tree_clear_wait(tracks, radii, 0, W))), flush=True)
                        continue
                    one, t_one = timed(lambda: eng.tree_clear_wait(tracks, radii, 0, W, per_node=True), a.reps)
                    many, t_many = timed(lambda: by_calls(eng, tracks, radii, W), a.reps)
                    many = joined(many)
                    assert np.array_equal(one[1], many[0]) and np.array_equal(one[2], many[1])
                    st = one[0]
                    full = np.uint64((1 << W) - 1)
                    row = dict(case="boat_advanced grown", nodes=N, discs=D, instants=600, where=where, waits=W, hits=st["hits"],
                               clear_hits=st["clear_hits"], clear_now=st["clear_now"], best_wait=st["best_wait"],
                               nodes_all_clear=int(np.sum(one[1] == full)), nodes_none_clear=int(np.sum(one[1] == 0)),
                               one_call_ms=round(float(np.median(t_one)), 3), one_call_ms_min=round(min(t_one), 3),
                               one_call_ms_max=round(max(t_one), 3), w_calls_ms=round(float(np.median(t_many)), 3),
                               w_calls_ms_min=round(min(t_many), 3), w_calls_ms_max=round(max(t_many), 3))
                    row["w_calls_over_one"] = round(row["w_calls_ms"] / row["one_call_ms"], 2)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
        eng.close()
    if a.out and rows:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "clear_wait_bench.jsonl"), "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    main()
