"""
Time of the clearance queries for several trees per call (Engine.tree_clear_multi / tree_clear_wait_multi: the device calls of
lqrrt_amd.avoids) next to what they replace in the same process: the loop of G one-tree calls (Engine.tree_clear / tree_clear_wait),
which is the yardstick -- the only route there was.  Both must give the same per-node answers and counters, tree by tree.  The
workload is tools/clear_bench.py's: boat_advanced trees grown on the device (tree k from MT19937 seed k + 1), D discs on straight
lines through the square (8, 48)^2 around the demo's goal for L = 600 instants, radius 0.5 m; every tree is asked against the SAME
table (shared traffic: uploaded once per launch by the batched call, once per tree by the loop).  Times are host wall clock around
the synchronous calls (argument checks, table upload, every launch and the read-back of the per-node arrays included), warmed,
median of `--reps` with the lowest and the highest.

    python tools/clear_multi_bench.py [--nodes 10000,100000] [--trees 4,16,64] [--discs 15] [--waits 16] [--reps 3] [--out DIR]
                                                            ->  one JSON line per (nodes, G, call); DIR/clear_multi_bench.jsonl
    python tools/clear_multi_bench.py --once --nodes 10000 --trees 16   ->  one untimed batched call of each kind (for a kernel trace)
    python tools/clear_multi_bench.py --deconflict          ->  deconflict(batched=True) against deconflict() on the fleet of
                                                                examples/fleet_deconflict_gpu.py: native calls, rounds, wall time
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

from clear_bench import WAVE, tracks_of                 # noqa: E402
from clear_wait_bench import timed                      # noqa: E402


def grown(nodes, seed):
    import lqrrt_amd
    from lqrrt_amd.engine import Engine
    s = lqrrt_amd.systems.BoatAdvanced(0)
    kw = s.plan_kwargs
    eng = Engine(s, capacity=nodes + 2 * WAVE + 8, max_wave=WAVE)
    eng.set_resolution(kw["dt"], kw["FPR"], int(kw["horizon"] / kw["dt"]), np.abs(s.error_tol), s.goal, np.abs(s.goal_buffer))
    space = np.array(s.sample_space, dtype=np.float64)
    eng.set_sampler(np.mean(space, axis=1), np.diff(space).flatten(), np.array(s.goal_bias, dtype=np.float64), 10)
    st = np.random.RandomState(seed).get_state()
    eng.set_mt19937(st[1], st[2])
    eng.tree_reset(s.x0)
    eng.extend(WAVE, node_limit=nodes)
    return eng


def same(batched, loop):
    for b, s in zip(batched, loop):
        assert b[0] == s[0] and np.array_equal(b[1], s[1]) and np.array_equal(b[2], s[2])


def stats_row(name, ts):
    return {name + "_ms": round(float(np.median(ts)), 3), name + "_ms_min": round(min(ts), 3), name + "_ms_max": round(max(ts), 3)}


def fleet():
    """The three cars of examples/fleet_deconflict_gpu.py, planned."""
    import lqrrt_amd as lqrrt
    planners = []
    for k, (x, y) in enumerate([(0.0, 0.0), (0.0, 30.0), (30.0, 0.0)]):
        car = lqrrt.systems.Car(0)
        cons = lqrrt.Constraints(nstates=car.nstates, ncontrols=car.ncontrols, goal_buffer=car.goal_buffer, is_feasible=car.is_feasible)
        p = lqrrt.Planner(car.dynamics, car.lqr, cons, horizon=5, dt=0.1, FPR=0, error_tol=car.error_tol, erf=car.erf, min_time=2,
                          max_time=3, max_nodes=1500, goal0=car.goal, sys_time=lambda: 0.0, printing=False, wave_size=256)
        np.random.seed(k + 1)
        p.update_plan(np.array([x, y, 0.0, 0.0, 0.0]), car.sample_space, goal_bias=car.goal_bias, xrand_gen=10)
        planners.append(p)
    return planners


def deconflict_rows(reps):
    """Each pass on a freshly planned fleet (a deconflicted fleet has nothing left to change); the first pass warms up."""
    import lqrrt_amd as lqrrt
    from lqrrt_amd import planner as planner_mod
    t_loop, t_batched, rounds, calls = [], [], None, None
    for rep in range(reps + 1):
        a, b = fleet(), fleet()
        t0 = time.perf_counter()
        want = lqrrt.deconflict(a, 2.0, order=[0, 1, 2])
        t1 = time.perf_counter()
        got, rounds, calls = planner_mod._deconflict_batched(b, np.broadcast_to(np.float64(2.0), (3,)), [0, 1, 2], 0, 0)
        t2 = time.perf_counter()
        assert got == want and all(list(p.node_seq) == list(q.node_seq) for p, q in zip(a, b))
        if rep:
            t_loop.append(1e3 * (t1 - t0))
            t_batched.append(1e3 * (t2 - t1))
    row = dict(case="deconflict, three cars of 1501 nodes", loop_calls=2, batched_rounds=rounds, batched_calls=calls,
               changed=[w is not None and w["best_end"] >= 0 for w in want])
    row.update(stats_row("loop", t_loop))
    row.update(stats_row("batched", t_batched))
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", default="10000,100000")
    ap.add_argument("--trees", default="4,16,64")
    ap.add_argument("--discs", type=int, default=15)
    ap.add_argument("--waits", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--once", action="store_true", help="one untimed batched call of each kind per configuration (for a kernel trace)")
    ap.add_argument("--deconflict", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from lqrrt_amd.engine import Engine
    rows = []
    if a.deconflict:
        rows = deconflict_rows(a.reps)
        print(json.dumps(rows[0]), flush=True)
    else:
        tracks, radii = tracks_of(a.discs)
        trees = sorted(int(v) for v in a.trees.split(","))
        for nodes in [int(v) for v in a.nodes.split(",")]:
            engines = []
            for G in trees:
                while len(engines) < G:
                    engines.append(grown(nodes, len(engines) + 1))
                tabs, rads, starts = [tracks] * G, [radii] * G, [0] * G
                if a.once:
                    st = Engine.tree_clear_multi(engines, tabs, rads, starts)
                    sw = Engine.tree_clear_wait_multi(engines, tabs, rads, starts, a.waits)
                    print(json.dumps(dict(nodes=engines[0].size, trees=G, clear_hits=[s["clear_hits"] for s in st],
                                          clear_hits_wait=[s["clear_hits"] for s in sw])), flush=True)
                    continue
                for call, batched, solo in (
                        ("tree_clear", lambda: Engine.tree_clear_multi(engines, tabs, rads, starts, per_node=True),
                         lambda: [e.tree_clear(tracks, radii, 0, per_node=True) for e in engines]),
                        ("tree_clear_wait W=%d" % a.waits,
                         lambda: Engine.tree_clear_wait_multi(engines, tabs, rads, starts, a.waits, per_node=True),
                         lambda: [e.tree_clear_wait(tracks, radii, 0, a.waits, per_node=True) for e in engines])):
                    loop, t_loop = timed(solo, a.reps)
                    one, t_one = timed(batched, a.reps)
                    same(one, loop)
                    row = dict(case="boat_advanced grown", call=call, nodes=engines[0].size, trees=G, discs=a.discs, instants=600,
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
        name = "clear_multi_deconflict.jsonl" if a.deconflict else "clear_multi_bench.jsonl"
        with open(os.path.join(a.out, name), "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    main()
