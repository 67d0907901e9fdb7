"""
Time of the tree retention (lqrrt_tree_retain: re-root, re-validate, compact on the device; Planner.replan) next to the host
route it replaces -- read the arrays back, cut the tree in NumPy (tests/retain_reference.py without the feasibility pass),
Engine.tree_load -- measured in the same process on the same tree.  Host wall clock around the synchronous calls, warmed, median of
`--reps` repeats; the tree is restored with Engine.tree_load between repeats.  The world changes between growth and retain (one
more obstacle beside the best plan), so a revalidating retain has something to find; the kept fraction is stated.

    python tools/retain_bench.py [--reps 3] [--cases boat_1e4,boat_1e5,config5] [--no-host] [--out DIR]
        ->  one JSON line per case; --out DIR also writes DIR/retain_bench.jsonl

The share of the check stage comes from a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/retain_bench.py --cases boat_1e5 --reps 1 --no-host

Fleets (lqrrt_tree_retain_multi, update_plans jobs with a `root`): n boat_advanced trees of `--fleet-nodes` nodes from n seeds, each
with its root a fifth of the way down its best plan and one more obstacle, revalidating -- ONE Engine.tree_retain_multi call next to
the loop of Engine.tree_retain calls over identically grown twins, same process, warmed, median of `--reps`:
    python tools/retain_bench.py --fleet 4,16,64,16x100000 [--fleet-nodes 10000] [--reps 3] [--out DIR]
        ->  one JSON line per fleet size; --out DIR also writes DIR/retain_multi_bench.jsonl
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
import retain_reference as rr                          # noqa: E402
from lqrrt_amd.engine import Engine                    # noqa: E402

CASES = {"boat_1e4": ("boat_advanced", 10000), "boat_1e5": ("boat_advanced", 100000), "config5": ("double_integrator", 50000)}


def grow(name, nodes):
    if name == "double_integrator":
        s = lqrrt_amd.systems.DoubleIntegrator(n_boxes=100000, seed=0)
    else:
        s = lqrrt_amd.systems.SYSTEMS[name](0)
    kw = s.plan_kwargs
    eng = Engine(s, capacity=nodes + 2048, max_wave=1024)
    eng.set_resolution(kw["dt"], kw["FPR"], int(kw["horizon"] / kw["dt"]), np.abs(s.error_tol), s.goal, np.abs(s.goal_buffer))
    space = np.array(s.sample_space, dtype=np.float64)
    eng.set_sampler(np.mean(space, axis=1), np.diff(space).flatten(), np.array(s.goal_bias, dtype=np.float64), 10)
    st = np.random.RandomState(1).get_state()
    eng.set_mt19937(st[1], st[2])
    eng.tree_reset(s.x0)
    eng.extend(1024, node_limit=nodes - 1)
    return s, eng


def change_world(s, eng, plan):
    """One more obstacle beside the middle of the plan (a circle for the boats, a box for the double integrator)."""
    mid = eng.states(plan[len(plan) // 2], 1)[0]
    if s.obs_stride == 6:
        c = mid[:3] + np.array([2.0, 0.0, 0.0])
        s.set_obstacles(np.vstack((s.obs, np.concatenate((c - 1.5, c + 1.5)))))
    else:
        s.set_obstacles(np.vstack((np.asarray(s.obs, dtype=np.float64).reshape(-1, 3), [mid[0] + 4.0, mid[1], 1.0])))
    eng.sync_geometry()


def run(case, reps, host):
    name, nodes = CASES[case]
    s, eng = grow(name, nodes)
    N = eng.size
    end = eng.plan_best()[0]
    plan = eng.climb(end if end >= 0 else N - 1)
    root = plan[max(1, len(plan) // 5)] if len(plan) > 1 else 0
    change_world(s, eng, plan)
    arr = rr.engine_arrays(eng)
    ign = eng.ignored()
    lo, hi = rr.goal_box(s)
    live = np.arange(arr[4].shape[1])[None, :] < arr[3][:, None]
    packed = (arr[4][live], arr[5][live])

    def restore():
        eng.tree_load(arr[0], arr[1], arr[2], edge_len=arr[3], xedge=packed[0], uedge=packed[1], ignored=ign)

    out = dict(case=case, system=name, nodes=N, root=int(root), plan_nodes=len(plan), obstacles=int(len(s.obs)))
    for revalidate in (False, True):
        times, stats = [], None
        for rep in range(reps + 1):                      # (the first pass warms the code objects up and is not counted)
            restore()
            t0 = time.perf_counter()
            stats, _ = eng.tree_retain(root, revalidate=revalidate)
            if rep > 0:
                times.append(time.perf_counter() - t0)
        key = "revalidate" if revalidate else "plain"
        out["device_%s_ms" % key] = round(1e3 * float(np.median(times)), 3)
        out["kept_%s" % key] = stats["kept"]
        out["kept_fraction_%s" % key] = round(stats["kept"] / float(N), 4)
        out["stats_%s" % key] = stats
    if host:
        parts = []
        for rep in range(reps + 1):
            restore()
            t0 = time.perf_counter()
            a = rr.engine_arrays(eng)
            t1 = time.perf_counter()
            ref = rr.retain(*a, root, None, lo, hi)
            t2 = time.perf_counter()
            xe, ue = rr.packed_edges(ref)
            eng.tree_load(ref["state"], ref["K"], ref["pID"], edge_len=ref["elen"], xedge=xe, uedge=ue, ignored=ref["ignored"])
            t3 = time.perf_counter()
            if rep > 0:
                parts.append((t1 - t0, t2 - t1, t3 - t2, t3 - t0))
        med = np.median(np.array(parts), axis=0)
        out.update(host_read_back_ms=round(1e3 * med[0], 1), host_numpy_ms=round(1e3 * med[1], 1), host_tree_load_ms=round(1e3 * med[2], 1),
                   host_route_ms=round(1e3 * med[3], 1), host_route_without_numpy_ms=round(1e3 * (med[0] + med[2]), 1))
        assert ref["stats"]["kept"] == out["kept_plain"]
    eng.close()
    return out


def run_fleet(n, nodes, reps):
    """n trees through one tree_retain_multi call / n twins through tree_retain one after the other."""
    fleet, twins, saved, roots = [], [], [], []
    for k in range(n):
        pair = []
        for _ in range(2):
            s = lqrrt_amd.systems.BoatAdvanced(0)
            kw = s.plan_kwargs
            eng = Engine(s, capacity=nodes + 2048, max_wave=1024)
            eng.set_resolution(kw["dt"], kw["FPR"], int(kw["horizon"] / kw["dt"]), np.abs(s.error_tol), s.goal, np.abs(s.goal_buffer))
            space = np.array(s.sample_space, dtype=np.float64)
            eng.set_sampler(np.mean(space, axis=1), np.diff(space).flatten(), np.array(s.goal_bias, dtype=np.float64), 10)
            st = np.random.RandomState(1 + k).get_state()
            eng.set_mt19937(st[1], st[2])
            eng.tree_reset(s.x0)
            eng.extend(1024, node_limit=nodes - 1)
            pair.append((s, eng))
        (s, eng), (s2, twin) = pair
        end = eng.plan_best()[0]
        plan = eng.climb(end if end >= 0 else eng.size - 1)
        roots.append(int(plan[max(1, len(plan) // 5)]) if len(plan) > 1 else 0)
        change_world(s, eng, plan)
        change_world(s2, twin, plan)
        arr = rr.engine_arrays(eng)
        live = np.arange(arr[4].shape[1])[None, :] < arr[3][:, None]
        saved.append((arr[0], arr[1], arr[2], arr[3], arr[4][live], arr[5][live], eng.ignored()))
        fleet.append(eng)
        twins.append(twin)

    def restore(engines):
        for e, a in zip(engines, saved):
            e.tree_load(a[0], a[1], a[2], edge_len=a[3], xedge=a[4], uedge=a[5], ignored=a[6])

    t_multi, t_solo, stats_multi, stats_solo = [], [], None, None
    for rep in range(reps + 1):                          # (the first pass warms the code objects up and is not counted)
        restore(fleet)
        restore(twins)
        t0 = time.perf_counter()
        done = Engine.tree_retain_multi(fleet, roots, True)
        t1 = time.perf_counter()
        solo = [twin.tree_retain(root, revalidate=True) for twin, root in zip(twins, roots)]
        t2 = time.perf_counter()
        stats_multi, stats_solo = [d[0] for d in done], [d[0] for d in solo]
        assert stats_multi == stats_solo
        if rep > 0:
            t_multi.append(t1 - t0)
            t_solo.append(t2 - t1)
    sizes = [s["old_size"] for s in stats_multi]
    kept = [s["kept"] for s in stats_multi]
    for e in fleet + twins:
        e.close()
    m, so = float(np.median(t_multi)), float(np.median(t_solo))
    return dict(case="fleet", system="boat_advanced", trees=n, nodes_per_tree=int(np.median(sizes)), nodes_total=int(sum(sizes)),
                kept_total=int(sum(kept)), kept_fraction=round(sum(kept) / float(sum(sizes)), 4), revalidate=True,
                multi_call_ms=round(1e3 * m, 3), solo_loop_ms=round(1e3 * so, 3), solo_per_tree_ms=round(1e3 * so / n, 3),
                multi_per_tree_ms=round(1e3 * m / n, 3), solo_over_multi=round(so / m, 2),
                multi_call_ms_all=[round(1e3 * v, 3) for v in t_multi], solo_loop_ms_all=[round(1e3 * v, 3) for v in t_solo])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default="boat_1e4,boat_1e5,config5")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--fleet", default=None, help="fleet sizes, e.g. 4,16,64 or 16x100000 (trees x nodes): time tree_retain_multi against the loop of tree_retain")
    ap.add_argument("--fleet-nodes", type=int, default=10000)
    a = ap.parse_args()
    if a.fleet:
        rows = []
        for item in a.fleet.split(","):                  # "16" = 16 trees of --fleet-nodes nodes, "16x100000" = of 100000
            n, _, nodes = item.partition("x")
            rows.append(run_fleet(int(n), int(nodes) if nodes else a.fleet_nodes, a.reps))
            print(json.dumps(rows[-1]), flush=True)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, "retain_multi_bench.jsonl"), "w") as f:
                f.write("".join(json.dumps(r) + "\n" for r in rows))
        return
    rows = []
    for case in a.cases.split(","):
        rows.append(run(case, a.reps, not a.no_host))
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "retain_bench.jsonl"), "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    main()
