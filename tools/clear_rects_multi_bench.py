"""
Time of the rectangle clearance queries for several trees per call (Engine.tree_clear_rects_multi / tree_clear_rects_wait_multi: the
device calls of lqrrt_amd.avoids_rects) next to what they replace in the same process: the loop of G one-tree calls
(Engine.tree_clear_rects / tree_clear_rects_wait), which is the yardstick -- the only route there was.  Both must give the same
per-node answers and counters, tree by tree; that is asserted before anything is timed.  The workload is
tools/clear_rects_bench.py's: boat_advanced trees grown on the device (tree k from MT19937 seed k + 1), D rectangles of 6 m x 0.4 m
on straight lines through the square (8, 48)^2 around the demo's goal for L = 600 instants, heading along their motion; every tree
is asked against the SAME table (shared traffic: built and uploaded once per launch by the batched call, once per tree by the
loop).  Times are host wall clock around the synchronous calls (argument checks, the host's cos / sin per turning pose, table
upload, every launch and the read-back of both per-node arrays included), warmed, median of `--reps` with the lowest and the
highest.

    python tools/clear_rects_multi_bench.py [--nodes 10000,100000] [--trees 4,16,64] [--rects 15] [--waits 16] [--reps 3] [--out DIR]
                                                            ->  one JSON line per (nodes, G, call); DIR/clear_rects_multi_bench.jsonl
    python tools/clear_rects_multi_bench.py --once --nodes 10000 --trees 16   ->  one untimed batched call of each kind (for a kernel trace)
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

from clear_multi_bench import grown, same, stats_row   # noqa: E402
from clear_rects_bench import rects_of, timed           # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", default="10000,100000")
    ap.add_argument("--trees", default="4,16,64")
    ap.add_argument("--rects", type=int, default=15)
    ap.add_argument("--waits", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--once", action="store_true", help="one untimed batched call of each kind per configuration (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from lqrrt_amd.engine import Engine
    rows = []
    tracks, extents, _ = rects_of(a.rects)
    trees = sorted(int(v) for v in a.trees.split(","))
    for nodes in [int(v) for v in a.nodes.split(",")]:
        engines = []
        for G in trees:
            while len(engines) < G:
                engines.append(grown(nodes, len(engines) + 1))
            tabs, exts, starts = [tracks] * G, [extents] * G, [0] * G
            if a.once:
                st = Engine.tree_clear_rects_multi(engines, tabs, exts, starts)
                sw = Engine.tree_clear_rects_wait_multi(engines, tabs, exts, starts, a.waits)
                print(json.dumps(dict(nodes=engines[0].size, trees=G, clear_hits=[s["clear_hits"] for s in st],
                                      clear_hits_wait=[s["clear_hits"] for s in sw])), flush=True)
                continue
            for call, batched, solo in (
                    ("tree_clear_rects", lambda: Engine.tree_clear_rects_multi(engines, tabs, exts, starts, per_node=True),
                     lambda: [e.tree_clear_rects(tracks, extents, 0, per_node=True) for e in engines]),
                    ("tree_clear_rects_wait W=%d" % a.waits,
                     lambda: Engine.tree_clear_rects_wait_multi(engines, tabs, exts, starts, a.waits, per_node=True),
                     lambda: [e.tree_clear_rects_wait(tracks, extents, 0, a.waits, per_node=True) for e in engines])):
                same(batched(), solo())                               # per tree, before anything is timed (this also warms both up)
                loop, t_loop = timed(solo, a.reps)
                one, t_one = timed(batched, a.reps)
                same(one, loop)
                row = dict(case="boat_advanced grown", call=call, nodes=engines[0].size, trees=G, rects=a.rects, instants=len(tracks),
                           hits=sum(s[0]["hits"] for s in one), clear_hits=sum(s[0]["clear_hits"] for s in one))
                row.update(stats_row("batched", t_one))
                row.update(stats_row("loop", t_loop))
                row["loop_over_batched"] = round(row["loop_ms"] / row["batched_ms"], 2)
                row["batched_median_below_loop_min"] = bool(row["batched_ms"] < row["loop_ms_min"])
                rows.append(row)
                print(json.dumps(row), flush=True)
        for e in engines:
            e.close()
    if a.out and rows:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "clear_rects_multi_bench.jsonl"), "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    main()
