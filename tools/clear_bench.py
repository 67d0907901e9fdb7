"""
Time of the clearance query (Engine.tree_clear: Planner.avoid's device call) on grown boat_advanced trees, next to the host route in
the same process: read the tree's parents, edge lengths, states and edges back, then run the NumPy reference of the rule
(tests/clear_reference.py).  Both must give the same per-node arrays and counters.  The D discs move on straight lines through the
square (8, 48)^2 around the demo's goal for L = 600 instants, radius 0.5 m.  Times are host wall clock around the synchronous calls (argument checks, table
upload, every launch and the read-back of the per-node arrays included), warmed, median of `--reps` with the lowest and the highest;
the host route, which takes seconds to minutes, is run once per configuration, and only on trees of up to `--host-max` nodes.

    python tools/clear_bench.py [--nodes 10000,100000] [--discs 15,63] [--reps 3] [--host-max 100000] [--out DIR]
                                                            ->  one JSON line per (nodes, D); DIR/clear_bench.jsonl
    python tools/clear_bench.py --once --nodes 100000 --discs 15   ->  one untimed device call (for a kernel trace)
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

import clear_reference as cl                           # noqa: E402
import retain_reference as rr                          # noqa: E402

WAVE, L = 1024, 600


def grown(nodes):
    import lqrrt_amd
    from lqrrt_amd.engine import Engine
    s = lqrrt_amd.systems.BoatAdvanced(0)
    kw = s.plan_kwargs
    eng = Engine(s, capacity=nodes + 2 * WAVE + 8, max_wave=WAVE)
    eng.set_resolution(kw["dt"], kw["FPR"], int(kw["horizon"] / kw["dt"]), np.abs(s.error_tol), s.goal, np.abs(s.goal_buffer))
    space = np.array(s.sample_space, dtype=np.float64)
    eng.set_sampler(np.mean(space, axis=1), np.diff(space).flatten(), np.array(s.goal_bias, dtype=np.float64), 10)
    st = np.random.RandomState(1).get_state()
    eng.set_mt19937(st[1], st[2])
    eng.tree_reset(s.x0)
    eng.extend(WAVE, node_limit=nodes)
    return s, eng


def tracks_of(D, seed=7):
    rs = np.random.RandomState(seed)
    a, b = rs.uniform(8.0, 48.0, (D, 2)), rs.uniform(8.0, 48.0, (D, 2))
    t = np.linspace(0.0, 1.0, L)[:, None, None]
    return a[None] + t * (b - a)[None], np.full(D, 0.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", default="10000,100000")
    ap.add_argument("--discs", default="15,63")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-max", type=int, default=100000)
    ap.add_argument("--once", action="store_true", help="one untimed device call per configuration (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for nodes in [int(v) for v in a.nodes.split(",")]:
        s, eng = grown(nodes)
        N = eng.size
        lo, hi = rr.goal_box(s)
        for D in [int(v) for v in a.discs.split(",")]:
            tracks, radii = tracks_of(D)
            ts, dev = [], None
            for rep in range(1 if a.once else a.reps + 1):              # (the first pass warms up and is not counted)
                t0 = time.perf_counter()
                dev = eng.tree_clear(tracks, radii, 0, per_node=True)
                if rep:
                    ts.append(1e3 * (time.perf_counter() - t0))
            if a.once:
                print(json.dumps(dict(nodes=N, discs=D, stats=dev[0])), flush=True)
                continue
            row = dict(case="boat_advanced grown", nodes=N, discs=D, instants=L, hits=dev[0]["hits"], clear_hits=dev[0]["clear_hits"],
                       conflicts=dev[0]["conflicts"], blocked=dev[0]["blocked"], device_ms=round(float(np.median(ts)), 3),
                       device_ms_min=round(min(ts), 3), device_ms_max=round(max(ts), 3))
            if N <= a.host_max + 1:
                t0 = time.perf_counter()
                state, _, pID, elen, xedge, _ = rr.engine_arrays(eng)
                t1 = time.perf_counter()
                ref = cl.clear(state, pID, elen, xedge, cl.row_test_of(s), tracks, radii, 0, lo, hi)
                t2 = time.perf_counter()
                assert dev[0] == ref["stats"] and np.array_equal(dev[1], ref["first"]) and np.array_equal(dev[2], ref["dwell_first"])
                row.update(host_readback_ms=round(1e3 * (t1 - t0), 1), host_reference_ms=round(1e3 * (t2 - t1), 1),
                           host_over_device=round(1e3 * (t2 - t0) / row["device_ms"], 1))
            rows.append(row)
            print(json.dumps(row), flush=True)
        eng.close()
    if a.out and rows:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "clear_bench.jsonl"), "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    main()
