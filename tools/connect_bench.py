"""
Time of the tree-wide goal connection (Planner.connect_goal: Engine.connect_search) on the device, next to the host time of the
C-oracle reference of the same rule (tests/connect_reference.py, one core) on the same tree.  Times are host wall clock around the
synchronous call (depth pass, upload, launch, read-back included), warmed, median of `--reps` with the lowest and the highest.

Trees: the boat_advanced_10k fixture cut off before its first goal node (3308 nodes, no incumbent); the whole fixture tree with no
incumbent and no id list (every chain runs until one wins); a boat_advanced tree of 10^5 nodes grown natively (no incumbent, the
found plan's cost as incumbent, and the 1024 nodes nearest the goal as id list).  One refine_round on the fixture's 113-node plan is
timed in the same process for scale.

    python tools/connect_bench.py [--reps 3] [--nodes 100000] [--out DIR]   ->  one JSON line per case; DIR/connect_bench.jsonl
    python tools/connect_bench.py --once                                     ->  one untimed search per case (for a kernel trace)

--fleet N[,N...]: the calls for several trees instead (lqrrt_amd.connect_goals: Engine.connect_search_multi + connect_commit_multi).
The boat_advanced_10k fixture is loaded into N engines, once cut at 3308 nodes (no incumbent) and once whole (the plan's cost as
incumbent), and ONE batched search plus ONE batched commit are timed against the loop of the one-tree calls over identically loaded
twins, in the same process: host wall clock, the trees loaded afresh (untimed) before every repetition, warmed, median of `--reps`
with the lowest and the highest.

    python tools/connect_bench.py --fleet 4,16,64 [--reps 3] [--out DIR]     ->  one JSON line per case; DIR/connect_multi_bench.jsonl
    python tools/connect_bench.py --fleet 16 --once                          ->  one untimed pass of both (for a kernel trace)

--via: the search through waypoints instead (Planner.connect_via: Engine.connect_via_search), next to tests/connect_via_reference.py
on the host with the same winner.  (a) the boat_advanced_10k fixture cut at 3308 nodes, the waypoints its plan's nodes beyond the
cut; (b) scenario A of the retain tests -- boat_advanced grown to 5001 nodes, one more obstacle beside plan node 45, a retain from
plan node 20 -- with the lost plan states as waypoints and the kept tree's best plan as incumbent; (c) case (a)'s tree without
waypoints, next to Engine.connect_search on the same tree in the same process.

    python tools/connect_bench.py --via [--reps 3] [--out DIR]               ->  one JSON line per case; DIR/connect_via_bench.jsonl

--via --fleet N[,N...]: the waypoint calls for several trees (lqrrt_amd.connect_vias: Engine.connect_via_search_multi +
connect_via_commit_multi).  Case (a) -- the tree and its waypoints -- is loaded into N engines, and ONE batched search plus ONE
batched commit are timed against the loop of the one-tree pair over identically loaded twins, in the same process: host wall clock,
the trees loaded afresh (untimed) before every repetition, warmed, median of `--reps` with the lowest and the highest.

    python tools/connect_bench.py --via --fleet 4,16 [--reps 3] [--out DIR]  ->  one JSON line per size; DIR/connect_vias_bench.jsonl
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
import connect_reference as cr                         # noqa: E402
from lqrrt_amd.engine import Engine                    # noqa: E402


def timed(fn, reps):
    fn()                                                 # (warms the code object up; not counted)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return out, dict(ms=round(float(np.median(ts)), 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3))


def reference(ref, **kw):
    t0 = time.perf_counter()
    win = ref.search(**kw)
    return (None if win is None else (win[0], win[1])), round(time.perf_counter() - t0, 3)


def search_case(label, eng, ref, H, reps, once, incumbent=cr.NO_INCUMBENT, nodes=None, with_reference=True, **extra):
    if once:
        eng.connect_search(H, incumbent, nodes=nodes)
        return None
    got, t = timed(lambda: eng.connect_search(H, incumbent, nodes=nodes), reps)
    row = dict(case=label, nodes=eng.size, candidates=eng.size if nodes is None else len(nodes),
               incumbent=None if incumbent == cr.NO_INCUMBENT else int(incumbent), winner=got, device_ms=t["ms"],
               device_ms_min=t["ms_min"], device_ms_max=t["ms_max"], **extra)
    print("device: " + json.dumps(row), file=sys.stderr, flush=True)   # (the reference of a large tree takes a while)
    if with_reference:
        want, secs = reference(ref, incumbent=incumbent, nodes=nodes)
        assert want == got, (label, want, got)
        row["reference_s"] = secs
    return row


def fixture_engine(s, g, size):
    kw = s.plan_kwargs
    N = len(g["state"]) if size is None else size
    el = np.array(g["edge_len"][:N], dtype=np.int32)
    el[0] = 1
    eng = Engine(s, capacity=N + 256, max_wave=64)
    eng.set_resolution(kw["dt"], kw["FPR"], max(int(el.max()), cr.horizon_of(s, g)), np.abs(np.asarray(s.error_tol, dtype=np.float64)),
                       s.goal, s.goal_buffer)
    eng.tree_load(g["state"][:N], g["K"][:N], g["pID"][:N], edge_len=el)
    return eng


def run_fixture(reps, once):
    s, g = cr.case("boat_advanced_10k")
    rows = []
    for label, size in (("boat_advanced_10k prefix", cr.first_goal_node(s, g)), ("boat_advanced_10k full", None)):
        ref = cr.from_fixture(s, g, size)
        eng = fixture_engine(s, g, size)
        row = search_case(label, eng, ref, ref.H, reps, once)
        rows.append(row)
        if size is None and not once:
            plan = [int(v) for v in g["node_seq"]]
            _, t = timed(lambda: eng.refine_round(plan, ref.H, ref.cost(plan)), reps)
            rows.append(dict(case="refine_round on the fixture plan, same tree", plan_nodes=len(plan), device_ms=t["ms"],
                             device_ms_min=t["ms_min"], device_ms_max=t["ms_max"]))
        if row is not None and size is not None:
            t0 = time.perf_counter()
            ids = eng.connect_commit(row["winner"][1], ref.H)
            row["commit_ms_once"] = round(1e3 * (time.perf_counter() - t0), 3)
            row["appended"] = len(ids)
        eng.close()
    return rows


def run_fleet(sizes, reps, once):
    s, g = cr.case("boat_advanced_10k")
    H = cr.horizon_of(s, g)
    rows = []
    for label, size in (("boat_advanced_10k prefix", cr.first_goal_node(s, g)), ("boat_advanced_10k full", None)):
        incumbent = cr.NO_INCUMBENT if size is not None else cr.from_fixture(s, g).cost([int(v) for v in g["node_seq"]])
        N = len(g["state"]) if size is None else size
        el = np.array(g["edge_len"][:N], dtype=np.int32)
        el[0] = 1
        pool = {}

        def load(eng):
            eng.tree_load(g["state"][:N], g["K"][:N], g["pID"][:N], edge_len=el)

        def batched(engines):
            n = len(engines)
            wins = Engine.connect_search_multi(engines, [H] * n, [incumbent] * n)
            ids = Engine.connect_commit_multi(engines, [None if w is None else w[1] for w in wins], [H] * n)
            return wins, ids

        def loop(engines):
            wins = [e.connect_search(H, incumbent) for e in engines]
            ids = [[] if w is None else e.connect_commit(w[1], H) for e, w in zip(engines, wins)]
            return wins, ids

        for n in sizes:
            while len(pool) < 2 * n:
                pool[len(pool)] = fixture_engine(s, g, size)
            fleet, twins = [pool[k] for k in range(n)], [pool[n + k] for k in range(n)]
            if once:
                batched(fleet)
                loop(twins)
                for e in fleet + twins:
                    load(e)
                continue
            out, ts = {}, {}
            for name, fn, engines in (("batched", batched, fleet), ("loop", loop, twins)):
                ts[name] = []
                for rep in range(reps + 1):                       # (the first pass warms up and is not counted)
                    for e in engines:
                        load(e)
                    t0 = time.perf_counter()
                    out[name] = fn(engines)
                    if rep:
                        ts[name].append(1e3 * (time.perf_counter() - t0))
            assert out["batched"] == out["loop"] and len(set(out["loop"][0])) == 1, (label, n)
            for a, b in zip(fleet, twins):                          # the same trees, whichever way
                assert a.size == b.size and np.array_equal(a.states(N, a.size - N), b.states(N, b.size - N))
            med = {k: float(np.median(v)) for k, v in ts.items()}
            rows.append(dict(case=label, engines=n, nodes=N, incumbent=None if incumbent == cr.NO_INCUMBENT else int(incumbent),
                             winner=out["loop"][0][0], appended=len(out["loop"][1][0]),
                             batched_ms=round(med["batched"], 3), batched_ms_min=round(min(ts["batched"]), 3),
                             batched_ms_max=round(max(ts["batched"]), 3), loop_ms=round(med["loop"], 3),
                             loop_ms_min=round(min(ts["loop"]), 3), loop_ms_max=round(max(ts["loop"]), 3),
                             batched_ms_per_tree=round(med["batched"] / n, 4), loop_ms_per_tree=round(med["loop"] / n, 4),
                             loop_over_batched=round(med["loop"] / med["batched"], 2)))
            print("fleet: " + json.dumps(rows[-1]), file=sys.stderr, flush=True)
        for e in pool.values():
            e.close()
    return rows


def via_case(label, eng, ref, way, H, reps, once, incumbent=cr.NO_INCUMBENT, **extra):
    if once:
        eng.connect_via_search(way, H, incumbent)
        return None
    got, t = timed(lambda: eng.connect_via_search(way, H, incumbent), reps)
    row = dict(case=label, nodes=eng.size, waypoints=len(way), candidates=eng.size * (len(way) + 1),
               incumbent=None if incumbent == cr.NO_INCUMBENT else int(incumbent), winner=got, device_ms=t["ms"],
               device_ms_min=t["ms_min"], device_ms_max=t["ms_max"], **extra)
    print("device: " + json.dumps(row), file=sys.stderr, flush=True)   # (the reference of a large search takes minutes)
    t0 = time.perf_counter()
    want = ref.search_via(way, incumbent=incumbent)
    row["reference_s"] = round(time.perf_counter() - t0, 3)
    assert (None if want is None else want[:3]) == got, (label, None if want is None else want[:3], got)
    return row


def run_via(reps, once):
    import connect_via_reference as cvr
    rows = []
    # (a) and (c): the fixture cut off before its first goal node
    s, g = cr.case("boat_advanced_10k")
    size = cr.first_goal_node(s, g)
    ref = cvr.from_fixture(s, g, size)
    _, way = cvr.plan_states(g, size)
    eng = fixture_engine(s, g, size)
    rows.append(via_case("(a) boat_advanced_10k prefix, its plan beyond the cut", eng, ref, way, ref.H, reps, once))
    none = np.zeros((0, s.nstates))
    rows.append(via_case("(c) the same tree, no waypoints", eng, ref, none, ref.H, reps, once))
    rows.append(search_case("(c) connect_search on the same tree", eng, ref, ref.H, reps, once, with_reference=False))
    eng.close()
    # (b): scenario A of tests/test_retain_gpu.py
    s = lqrrt_amd.systems.BoatAdvanced(0)
    kw = s.plan_kwargs
    H = int(kw["horizon"] / kw["dt"])
    eng = Engine(s, capacity=5000 + 2 * 256 + 8, max_wave=256)
    eng.set_resolution(kw["dt"], kw["FPR"], H, np.abs(s.error_tol), s.goal, np.abs(s.goal_buffer))
    space = np.array(s.sample_space, dtype=np.float64)
    eng.set_sampler(np.mean(space, axis=1), np.diff(space).flatten(), np.array(s.goal_bias, dtype=np.float64), 10)
    st = np.random.RandomState(1).get_state()
    eng.set_mt19937(st[1], st[2])
    eng.tree_reset(s.x0)
    eng.extend(256, node_limit=5000)
    plan = eng.climb(eng.plan_best()[0])
    old = eng.states()
    mid = old[plan[45]]
    s.set_obstacles(np.vstack((np.asarray(s.obs, dtype=np.float64).reshape(-1, 3), [mid[0] + 4.0, mid[1], 1.0])))
    eng.sync_geometry()
    stats, old_to_new = eng.tree_retain(plan[20], revalidate=True)
    way = old[[v for v in plan[20:] if old_to_new[v] < 0]]
    ref = cvr.ViaConnector(s, eng.states(), eng.gains(), eng.parents(), eng.edge_lengths(), H)
    incumbent = stats["best_steps"] if stats["goal_hits"] else cr.NO_INCUMBENT
    rows.append(via_case("(b) retain scenario A, the lost plan states", eng, ref, way, H, reps, once, incumbent=incumbent,
                         kept=stats["kept"]))
    eng.close()
    return rows


def run_via_fleet(sizes, reps, once):
    import connect_via_reference as cvr
    s, g = cr.case("boat_advanced_10k")
    H = cr.horizon_of(s, g)
    N = cr.first_goal_node(s, g)
    _, way = cvr.plan_states(g, N)
    el = np.array(g["edge_len"][:N], dtype=np.int32)
    el[0] = 1
    label = "(a) boat_advanced_10k prefix, its plan beyond the cut"
    pool, rows = {}, []

    def load(eng):
        eng.tree_load(g["state"][:N], g["K"][:N], g["pID"][:N], edge_len=el)

    def batched(engines):
        n = len(engines)
        wins = Engine.connect_via_search_multi(engines, [way] * n, [H] * n, [cr.NO_INCUMBENT] * n)
        ids = Engine.connect_via_commit_multi(engines, [None if w is None else (w[1], w[2]) for w in wins], [way] * n, [H] * n)
        return wins, ids

    def loop(engines):
        wins = [e.connect_via_search(way, H, cr.NO_INCUMBENT) for e in engines]
        ids = [[] if w is None else e.connect_via_commit(w[1], w[2], way, H) for e, w in zip(engines, wins)]
        return wins, ids

    for n in sizes:
        while len(pool) < 2 * n:
            pool[len(pool)] = fixture_engine(s, g, N)
        fleet, twins = [pool[k] for k in range(n)], [pool[n + k] for k in range(n)]
        if once:
            batched(fleet)
            loop(twins)
            for e in fleet + twins:
                load(e)
            continue
        out, ts = {}, {}
        for name, fn, engines in (("batched", batched, fleet), ("loop", loop, twins)):
            ts[name] = []
            for rep in range(reps + 1):                           # (the first pass warms up and is not counted)
                for e in engines:
                    load(e)
                t0 = time.perf_counter()
                out[name] = fn(engines)
                if rep:
                    ts[name].append(1e3 * (time.perf_counter() - t0))
        assert out["batched"] == out["loop"] and len(set(out["loop"][0])) == 1 and out["loop"][0][0] is not None, (label, n)
        for a, b in zip(fleet, twins):                              # the same trees, whichever way
            assert a.size == b.size and np.array_equal(a.states(N, a.size - N), b.states(N, b.size - N))
        med = {k: float(np.median(v)) for k, v in ts.items()}
        rows.append(dict(case=label, engines=n, nodes=N, waypoints=len(way), candidates=N * (len(way) + 1), winner=out["loop"][0][0],
                         appended=len(out["loop"][1][0]),
                         batched_ms=round(med["batched"], 3), batched_ms_min=round(min(ts["batched"]), 3),
                         batched_ms_max=round(max(ts["batched"]), 3), loop_ms=round(med["loop"], 3),
                         loop_ms_min=round(min(ts["loop"]), 3), loop_ms_max=round(max(ts["loop"]), 3),
                         batched_ms_per_tree=round(med["batched"] / n, 4), loop_ms_per_tree=round(med["loop"] / n, 4),
                         loop_over_batched=round(med["loop"] / med["batched"], 2)))
        print("fleet: " + json.dumps(rows[-1]), file=sys.stderr, flush=True)
    for e in pool.values():
        e.close()
    return rows


def run_native(max_nodes, reps, once):
    s = lqrrt_amd.systems.BoatAdvanced(0)
    cons = lqrrt_amd.Constraints(s.nstates, s.ncontrols, s.goal_buffer, s.is_feasible)
    p = lqrrt_amd.Planner(s.dynamics, s.lqr, cons, error_tol=s.error_tol, erf=s.erf, goal0=s.goal, printing=False, min_time=2, max_time=3,
                          max_nodes=max_nodes, sys_time=lambda: 0.0, wave_size=1024, **s.plan_kwargs)
    np.random.seed(1)
    t0 = time.perf_counter()
    p.update_plan(s.x0, s.sample_space, goal_bias=s.goal_bias, xrand_gen=10)
    grow_s = time.perf_counter() - t0
    eng, H = p._engine, p.horizon_iters
    ref = cr.Connector(s, eng.states(), eng.gains(), eng.parents(), eng.edge_lengths(), H)
    label = "boat_advanced native %d" % eng.size
    extra = dict(grow_s=round(grow_s, 2))
    rows = [search_case(label + ", no incumbent", eng, ref, H, reps, once, **extra)]
    if p.plan_reached_goal:
        lens = eng.edge_lengths()
        cost = 1 + int(sum(int(lens[v]) for v in p.node_seq[1:]))
        rows.append(search_case(label + ", the plan's cost as incumbent", eng, ref, H, reps, once, incumbent=cost, **extra))
    near = np.argsort(eng.costs_to_go(np.asarray(s.goal, dtype=np.float64)), kind="stable")[:1024].astype(np.int32)
    rows.append(search_case(label + ", the 1024 nodes nearest the goal", eng, ref, H, reps, once, nodes=near, **extra))
    # one candidate: what the call costs before any chain runs (the host's depth pass over the mirrors, the upload, one launch)
    rows.append(search_case(label + ", the root alone", eng, ref, H, reps, once, nodes=np.zeros(1, dtype=np.int32), **extra))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--nodes", type=int, default=100000, help="size of the natively grown tree (0: leave it out)")
    ap.add_argument("--once", action="store_true", help="one untimed search per case, no reference (for a kernel trace)")
    ap.add_argument("--fleet", default=None, help="engines per call, e.g. 4,16,64: time the batched calls against the loop of solo calls instead")
    ap.add_argument("--via", action="store_true", help="time the search through waypoints (Engine.connect_via_search) instead; with --fleet: the batched pair")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.via and a.fleet:
        rows, name = run_via_fleet([int(v) for v in a.fleet.split(",")], a.reps, a.once), "connect_vias_bench.jsonl"
    elif a.via:
        rows, name = run_via(a.reps, a.once), "connect_via_bench.jsonl"
    elif a.fleet:
        rows, name = run_fleet([int(v) for v in a.fleet.split(",")], a.reps, a.once), "connect_multi_bench.jsonl"
    else:
        rows, name = run_fixture(a.reps, a.once), "connect_bench.jsonl"
        if a.nodes > 0:
            rows += run_native(a.nodes, a.reps, a.once)
    rows = [r for r in rows if r is not None]
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out and rows:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, name), "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    main()
