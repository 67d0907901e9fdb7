"""
Time of the plan refinement (Planner.refine_plan) on the device, next to the host time of the C-oracle reference of the same rule
(tests/refine_reference.py).  The fixture's final tree is loaded (Engine.tree_load) and its plan refined to the fix-point; every
round is one lqrrt_refine_search (one launch, candidates in parallel) and, when it finds something, one lqrrt_refine_commit.  Times
are host wall clock around the synchronous calls (upload, launch, read-back included), best of `--reps` repetitions.

    python tools/refine_bench.py [--reps 5] [--out DIR]   ->  one JSON line per case
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import lqrrt_amd                                       # noqa: E402
import refine_reference as rr                          # noqa: E402
from lqrrt_amd.engine import Engine                    # noqa: E402

CASES = [("boat_advanced_10k", "boat_advanced", 2.0), ("boat_advanced_10k", "boat_advanced", 1.0), ("car_2000", "car", 1.0)]


def run(fixture, name, factor, reps, with_reference):
    g = np.load(os.path.join(ROOT, "tests", "golden", "traj_%s.npz" % fixture))
    s = lqrrt_amd.systems.SYSTEMS[name](0)
    buf = factor * np.abs(np.asarray(s.goal_buffer, dtype=np.float64))
    ref, plan0 = rr.from_fixture(s, g, goal_buffer=buf)
    kw = s.plan_kwargs
    N = len(g["state"])
    el = np.array(g["edge_len"], dtype=np.int32)
    el[0] = 1
    eng = Engine(s, capacity=N + 256, max_wave=64)
    eng.set_resolution(kw["dt"], kw["FPR"], max(int(el.max()), ref.H), np.abs(np.asarray(s.error_tol, dtype=np.float64)), s.goal, buf)
    first_round, full = [], []
    for rep in range(reps + 1):                          # (the first pass warms the code objects up and is not counted)
        eng.tree_load(g["state"], g["K"], g["pID"], edge_len=el)
        plan = list(plan0)
        t_all = time.perf_counter()
        rounds = []
        for r in range(8):
            lens = eng.edge_lengths()
            C = 1 + sum(int(lens[v]) for v in plan[1:])
            t0 = time.perf_counter()
            win = eng.refine_round(plan, ref.H, C)
            t1 = time.perf_counter()
            if r == 0 and rep > 0:
                first_round.append(t1 - t0)
            if win is None:
                break
            ids = eng.refine_commit(plan, ref.H, win[1], win[2])
            plan = plan[:win[1] + 1] + ids
            rounds.append(win)
        if rep > 0:
            full.append(time.perf_counter() - t_all)
    out = dict(fixture=fixture, goal_box_factor=factor, plan_nodes=len(plan0), candidates=len(plan0) * (len(plan0) - 1) // 2,
               steps_before=int(ref.cost(plan0)), rounds=[list(w) for w in rounds],
               device_round1_ms=round(1e3 * min(first_round), 3), device_full_ms=round(1e3 * min(full), 3))
    if with_reference:
        t0 = time.perf_counter()
        ref.round(plan0)
        out["reference_round1_s"] = round(time.perf_counter() - t0, 3)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = [run(f, n, k, a.reps, not a.no_reference) for f, n, k in CASES]
    for r in rows:
        print(json.dumps(r))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "refine_bench.jsonl"), "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    main()
