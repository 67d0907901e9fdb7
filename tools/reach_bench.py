"""
Time of one tree asked about many goals (Planner.goal_costs: Engine.reach_search, ONE launch for T targets) next to the only way the
API had before it: per target one Engine.set_resolution(goal_t) plus one Engine.connect_search, on an identically loaded twin in the
same process.  The tree is the whole boat_advanced_10k fixture tree (10 001 nodes); target 0 is the system's own goal, the others
are the states of tree nodes spread evenly over the ids, all with the system's goal buffer and no incumbent.  Both ways must give
the same winners.  Times are host wall clock around the synchronous calls (depth pass, upload, launch, read-back included), warmed,
median of `--reps` with the lowest and the highest.

    python tools/reach_bench.py [--targets 1,8,64] [--reps 3] [--out DIR]   ->  one JSON line per T; DIR/reach_bench.jsonl
    python tools/reach_bench.py --once                                       ->  one untimed pass of both (for a kernel trace)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", default="1,8,64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--once", action="store_true", help="one untimed pass of both ways per T (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    s, g = cr.case("boat_advanced_10k")
    H = cr.horizon_of(s, g)
    kw = s.plan_kwargs
    tol = np.abs(np.asarray(s.error_tol, dtype=np.float64))
    eng, twin = fixture_engine(s, g, None), fixture_engine(s, g, None)
    Hpool = eng.horizon_iters
    N = eng.size
    own = np.asarray(s.goal, dtype=np.float64)
    rows = []
    for T in [int(v) for v in a.targets.split(",")]:
        ids = [int(round(k * (N - 1) / T)) for k in range(1, T)]
        goals = np.array([own] + [g["state"][k] for k in ids], dtype=np.float64)

        def one_call():
            return eng.reach_search(goals, s.goal_buffer, H)

        def loop():
            out = []
            for t in range(T):
                twin.set_resolution(kw["dt"], kw["FPR"], Hpool, tol, goals[t], s.goal_buffer)
                out.append(twin.connect_search(H, cr.NO_INCUMBENT))
            return out

        out, ts = {}, {}
        for name, fn in (("one_call", one_call), ("loop", loop)):
            ts[name] = []
            for rep in range(1 if a.once else a.reps + 1):          # (the first pass warms up and is not counted)
                t0 = time.perf_counter()
                out[name] = fn()
                if rep:
                    ts[name].append(1e3 * (time.perf_counter() - t0))
        assert out["one_call"] == out["loop"], (T, out)
        assert eng.size == twin.size == N
        if a.once:
            continue
        med = {k: float(np.median(v)) for k, v in ts.items()}
        rows.append(dict(case="boat_advanced_10k full", nodes=N, targets=T, candidates=N * T,
                         winners=sum(w is not None for w in out["loop"]),
                         one_call_ms=round(med["one_call"], 3), one_call_ms_min=round(min(ts["one_call"]), 3),
                         one_call_ms_max=round(max(ts["one_call"]), 3), loop_ms=round(med["loop"], 3),
                         loop_ms_min=round(min(ts["loop"]), 3), loop_ms_max=round(max(ts["loop"]), 3),
                         one_call_ms_per_target=round(med["one_call"] / T, 4), loop_ms_per_target=round(med["loop"] / T, 4),
                         loop_over_one_call=round(med["loop"] / med["one_call"], 2)))
        print(json.dumps(rows[-1]), flush=True)
    eng.close(), twin.close()
    if a.out and rows:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "reach_bench.jsonl"), "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    main()
