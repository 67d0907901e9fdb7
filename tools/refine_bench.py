"""
Time of the plan refinement (Planner.refine_plan) on the device, next to the host time of the C-oracle reference of the same rule
(tests/refine_reference.py).  The fixture's final tree is loaded (Engine.tree_load) and its plan refined to the fix-point; every
round is one lqrrt_refine_search (one launch, candidates in parallel) and, when it finds something, one lqrrt_refine_commit.  Times
are host wall clock around the synchronous calls (upload, launch, read-back included), best of `--reps` repetitions.

    python tools/refine_bench.py [--reps 5] [--out DIR]   ->  one JSON line per case

Fleets (lqrrt_refine_search_multi / lqrrt_refine_commit_multi, refine_plans): the boat_advanced_10k fixture at goal box x 2 loaded
into n engines, all rounds to the fix-point through Engine.refine_round_multi / refine_commit_multi next to the loop of
refine_round / refine_commit over n identically loaded twins, same process, alternating, warmed, median of `--reps`:

    python tools/refine_bench.py --fleet 4,16,64 [--reps 3] [--out DIR]
        ->  one JSON line per fleet size; --out DIR also writes DIR/refine_multi_bench.jsonl
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


def _load(fixture, name, factor, n):
    g = np.load(os.path.join(ROOT, "tests", "golden", "traj_%s.npz" % fixture))
    s = lqrrt_amd.systems.SYSTEMS[name](0)
    buf = factor * np.abs(np.asarray(s.goal_buffer, dtype=np.float64))
    ref, plan0 = rr.from_fixture(s, g, goal_buffer=buf)
    kw = s.plan_kwargs
    el = np.array(g["edge_len"], dtype=np.int32)
    el[0] = 1
    engines = []
    for _ in range(n):
        eng = Engine(s, capacity=len(g["state"]) + 256, max_wave=64)
        eng.set_resolution(kw["dt"], kw["FPR"], max(int(el.max()), ref.H), np.abs(np.asarray(s.error_tol, dtype=np.float64)), s.goal, buf)
        engines.append(eng)
    return engines, (lambda eng: eng.tree_load(g["state"], g["K"], g["pID"], edge_len=el)), plan0, ref


def _cost(eng, plan):
    lens = eng.edge_lengths()
    return 1 + sum(int(lens[v]) for v in plan[1:])


def run_fleet(n, reps, fixture="boat_advanced_10k", name="boat_advanced", factor=2.0, once=False):
    """n plans through the batched calls / n twins through the one-engine calls one after the other.  The step counts the rounds
    have to beat are read before the clock starts and taken from the winners afterwards, on both routes."""
    fleet, load, plan0, ref = _load(fixture, name, factor, n)
    twins = _load(fixture, name, factor, n)[0]
    t_multi, t_solo, t_search, t_commit = [], [], [], []
    logs = None
    for rep in range(1 if once else reps + 1):           # (the first pass warms the code objects up and is not counted)
        for eng in fleet + twins:
            load(eng)
        c0 = _cost(fleet[0], plan0)
        # ---- batched
        plans, costs, log_m = [list(plan0) for _ in range(n)], [c0] * n, [[] for _ in range(n)]
        active, search_s, commit_s = list(range(n)), 0.0, 0.0
        t0 = time.perf_counter()
        for _ in range(8):
            ta = time.perf_counter()
            wins = Engine.refine_round_multi([fleet[k] for k in active], [plans[k] for k in active], [ref.H] * len(active),
                                             [costs[k] for k in active])
            tb = time.perf_counter()
            search_s += tb - ta
            winners = [(k, w) for k, w in zip(active, wins) if w is not None]
            if not winners:
                break
            new = Engine.refine_commit_multi([fleet[k] for k, _ in winners], [plans[k] for k, _ in winners], [ref.H] * len(winners),
                                             [(w[1], w[2]) for _, w in winners])
            commit_s += time.perf_counter() - tb
            for (k, w), ids in zip(winners, new):
                plans[k], costs[k] = plans[k][:w[1] + 1] + ids, w[0]
                log_m[k].append(list(w))
            active = [k for k, _ in winners]
        t1 = time.perf_counter()
        # ---- one by one
        log_s = [[] for _ in range(n)]
        for k, eng in enumerate(twins):
            plan, cost = list(plan0), c0
            for _ in range(8):
                win = eng.refine_round(plan, ref.H, cost)
                if win is None:
                    break
                ids = eng.refine_commit(plan, ref.H, win[1], win[2])
                plan, cost = plan[:win[1] + 1] + ids, win[0]
                log_s[k].append(list(win))
        t2 = time.perf_counter()
        assert log_m == log_s and all(np.array_equal(a.states(), b.states()) for a, b in zip(fleet, twins))
        logs = log_m
        if rep > 0:
            t_multi.append(t1 - t0); t_solo.append(t2 - t1); t_search.append(search_s); t_commit.append(commit_s)
    for eng in fleet + twins:
        eng.close()
    if once:
        return None
    m, so = float(np.median(t_multi)), float(np.median(t_solo))
    ms = lambda v: round(1e3 * v, 3)
    return dict(case="fleet", fixture=fixture, goal_box_factor=factor, plans=n, plan_nodes=len(plan0),
                candidates_per_plan=len(plan0) * (len(plan0) - 1) // 2, rounds=logs[0], batched_ms=ms(m), solo_loop_ms=ms(so),
                batched_per_plan_ms=ms(m / n), solo_per_plan_ms=ms(so / n), solo_over_batched=round(so / m, 2),
                batched_search_ms=ms(float(np.median(t_search))), batched_commit_ms=ms(float(np.median(t_commit))),
                batched_ms_all=[ms(v) for v in t_multi], solo_loop_ms_all=[ms(v) for v in t_solo])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--fleet", default=None, help="fleet sizes, e.g. 4,16,64: time the batched refinement against the loop of one-engine calls")
    ap.add_argument("--once", action="store_true", help="with --fleet: one untimed pass per size (for a kernel trace)")
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.fleet:
        rows = [run_fleet(int(n), a.reps or 3, once=a.once) for n in a.fleet.split(",")]
        rows = [r for r in rows if r is not None]
        for r in rows:
            print(json.dumps(r))
        if a.out and rows:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, "refine_multi_bench.jsonl"), "w") as f:
                f.write("".join(json.dumps(r) + "\n" for r in rows))
        return
    a.reps = a.reps or 5
    rows = [run(f, n, k, a.reps, not a.no_reference) for f, n, k in CASES]
    for r in rows:
        print(json.dumps(r))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "refine_bench.jsonl"), "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    main()
