"""
Time of a fleet's task-assignment matrix (fleet_goal_costs: Engine.reach_search_multi, ONE call for P trees x T targets) next to the
loop the API allowed before it: P solo Engine.reach_search calls, one per tree, on identically loaded twins in the same process.
Every tree is the whole boat_advanced_10k fixture tree (10 001 nodes); the T targets are shared by all trees, as the berths of a
fleet are: target 0 is the system's own goal, the others are the states of tree nodes spread evenly over the ids, all with the
system's goal buffer and no incumbent.  Both ways must give the same winners.  Times are host wall clock around the synchronous
calls (depth passes, uploads, launches, read-backs included), warmed, median of `--reps` with the lowest and the highest.

    python tools/reach_multi_bench.py [--sizes 4x8,16x8,16x64] [--reps 3] [--out DIR]  ->  one JSON line per size; DIR/reach_multi_bench.jsonl
    python tools/reach_multi_bench.py --once                                             ->  one untimed pass of both (for a kernel trace)
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

import connect_reference as cr                         # noqa: E402
from connect_bench import fixture_engine               # noqa: E402
from lqrrt_amd.engine import Engine                    # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4x8,16x8,16x64", help="P x T pairs: engines x targets")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--once", action="store_true", help="one untimed pass of both ways per size (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sizes = [tuple(int(v) for v in pair.split("x")) for pair in a.sizes.split(",")]
    s, g = cr.case("boat_advanced_10k")
    H = cr.horizon_of(s, g)
    most = max(P for P, _ in sizes)
    fleet = [fixture_engine(s, g, None) for _ in range(most)]
    twins = [fixture_engine(s, g, None) for _ in range(most)]
    N = fleet[0].size
    own = np.asarray(s.goal, dtype=np.float64)
    rows = []
    for P, T in sizes:
        ids = [int(round(k * (N - 1) / T)) for k in range(1, T)]
        goals = np.array([own] + [g["state"][k] for k in ids], dtype=np.float64)

        def one_call():
            return Engine.reach_search_multi(fleet[:P], [goals] * P, [s.goal_buffer] * P, [H] * P)

        def loop():
            return [twin.reach_search(goals, s.goal_buffer, H) for twin in twins[:P]]

        out, ts = {}, {}
        for name, fn in (("one_call", one_call), ("loop", loop)):
            ts[name] = []
            for rep in range(1 if a.once else a.reps + 1):          # (the first pass warms up and is not counted)
                t0 = time.perf_counter()
                out[name] = fn()
                if rep:
                    ts[name].append(1e3 * (time.perf_counter() - t0))
        assert out["one_call"] == out["loop"], (P, T)
        assert all(e.size == N for e in fleet + twins)
        if a.once:
            continue
        med = {k: float(np.median(v)) for k, v in ts.items()}
        rows.append(dict(case="boat_advanced_10k full", nodes=N, engines=P, targets=T, candidates=N * T * P,
                         winners=sum(w is not None for row in out["loop"] for w in row),
                         one_call_ms=round(med["one_call"], 3), one_call_ms_min=round(min(ts["one_call"]), 3),
                         one_call_ms_max=round(max(ts["one_call"]), 3), loop_ms=round(med["loop"], 3),
                         loop_ms_min=round(min(ts["loop"]), 3), loop_ms_max=round(max(ts["loop"]), 3),
                         one_call_ms_per_entry=round(med["one_call"] / (P * T), 4), loop_ms_per_entry=round(med["loop"] / (P * T), 4),
                         loop_over_one_call=round(med["loop"] / med["one_call"], 2)))
        print(json.dumps(rows[-1]), flush=True)
    for e in fleet + twins:
        e.close()
    if a.out and rows:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "reach_multi_bench.jsonl"), "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    main()
