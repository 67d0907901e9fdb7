"""
Time of the clear goal chains for a fleet (Engine.tree_clear_connect_multi: the device call of avoids(connect)) against the loop of
one-tree calls (Engine.tree_clear_connect, the device call of Planner.avoid(connect)) on the same engines, in the same process.
The workload is tools/clear_connect_bench.py's: a boat_advanced tree grown on the device, D = 15 discs of radius 0.5 m, placements
`far` (nothing near the tree) and `crossed, table to the last hit` (the discs share the tree's goal hits among them, each standing on
a hit's last row at the instant the vehicle arrives there).  The G engines of a row hold the same tree -- grown once, loaded G times
-- and every member passes the same track table, so the batched call uploads it once per chunk and the loop once per call.  The
answers of the two routes must be equal, member by member.  Times are host wall clock around the synchronous calls, warmed, median
of `--reps` with the lowest and the highest.

    python tools/clear_connect_multi_bench.py [--nodes 1000,10000] [--fleet 4,16,64] [--reps 3] [--out DIR]
                                                            ->  one JSON line per (nodes, G, placement); DIR/clear_connect_multi_bench.jsonl
    python tools/clear_connect_multi_bench.py --once --nodes 1000 --fleet 16 --placement far   ->  one untimed batched call per placement (for a kernel trace)
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

import retain_reference as rr                                        # noqa: E402
from clear_bench import L, grown                                     # noqa: E402
from clear_connect_bench import TRIES, crossed_tracks, twin_of       # noqa: E402

D = 15


def main():
    from lqrrt_amd.engine import Engine
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", default="1000,10000")
    ap.add_argument("--fleet", default="4,16,64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--once", action="store_true", help="one untimed batched call per configuration (for a kernel trace)")
    ap.add_argument("--placement", default=None, help="only this placement (far / crossed)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    fleets = [int(v) for v in a.fleet.split(",")]
    rows = []
    for nodes in [int(v) for v in a.nodes.split(",")]:
        s, eng = grown(nodes)
        N = eng.size
        H = int(s.plan_kwargs["horizon"] / s.plan_kwargs["dt"])
        arrays = rr.engine_arrays(eng)
        radii = np.full(D, 0.5)
        placements = (("far", np.full((L, D, 2), 1e4)), ("crossed, table to the last hit", crossed_tracks(s, eng, arrays, D, None)))
        placements = [p for p in placements if a.placement is None or p[0].startswith(a.placement)]
        engines = [eng] + [twin_of(s, eng, arrays, H) for _ in range(max(fleets) - 1)]
        for G in fleets:
            mine = engines[:G]
            for placement, tracks in placements:
                tracks = np.ascontiguousarray(tracks)
                args = ([tracks] * G, [radii] * G, [0] * G, [H] * G, TRIES)
                tb, tl, batched, loop = [], [], None, None
                for rep in range(1 if a.once else a.reps + 1):          # (the first pass warms up and is not counted)
                    t0 = time.perf_counter()
                    batched = Engine.tree_clear_connect_multi(mine, *args, per_node=True)
                    if rep:
                        tb.append(1e3 * (time.perf_counter() - t0))
                if a.once:
                    print(json.dumps(dict(nodes=N, fleet=G, placement=placement, stats=batched[0][0], chain=batched[0][1])), flush=True)
                    continue
                for rep in range(a.reps + 1):
                    t0 = time.perf_counter()
                    loop = [e.tree_clear_connect(tracks, radii, 0, H, TRIES, per_node=True) for e in mine]
                    if rep:
                        tl.append(1e3 * (time.perf_counter() - t0))
                for b, o in zip(batched, loop):
                    assert b[0] == o[0] and b[1] == o[1] and np.array_equal(b[2], o[2]) and np.array_equal(b[3], o[3]), (b[:2], o[:2])
                st, ch = batched[0][0], batched[0][1]
                row = dict(case="boat_advanced grown", nodes=N, fleet=G, discs=D, instants=len(tracks), placement=placement, hits=st["hits"],
                           clear_hits=st["clear_hits"], clear_candidates=ch["clear_candidates"], chain_from=ch["chain_from"],
                           chain_cost=ch["chain_cost"], batched_ms=round(float(np.median(tb)), 3), batched_ms_min=round(min(tb), 3),
                           batched_ms_max=round(max(tb), 3), loop_ms=round(float(np.median(tl)), 3), loop_ms_min=round(min(tl), 3),
                           loop_ms_max=round(max(tl), 3), loop_over_batched=round(float(np.median(tl) / np.median(tb)), 2),
                           batched_median_below_loop_lowest=bool(np.median(tb) < min(tl)))
                rows.append(row)
                print(json.dumps(row), flush=True)
        for e in engines:
            e.close()
    if a.out and rows:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "clear_connect_multi_bench.jsonl"), "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    main()
