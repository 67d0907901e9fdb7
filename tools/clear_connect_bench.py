"""
Time of the clear goal chains (Engine.tree_clear_connect: the device call of Planner.avoid(connect)) on grown boat_advanced trees,
next to what the calls before it offer for the same answer, in the same process: ONE pass of tree_clear(per_node) +
connect_search(nodes = the ids with first == -1, incumbent = the best clear hit's depth) + connect_commit + tree_clear again, which
tells whether the appended chain is clear at its times.  When it is not, that route has to strike the winner from the id list and go
round again with a useless chain in the tree: one pass is its LOWER bound.  Whenever the first pass's chain happens to be clear, it
must be the new call's winner.

Discs, L = 600 instants, radius 0.5 m: `crossed` -- the D discs share the tree's own goal hits among them, each standing on a hit's
last row at the instant the vehicle arrives there and far away otherwise (hits beyond the table, or that collide with another hit of
the same disc at the same instant, stay clear: the row reports how many) --, `far`, nothing near the tree, and `crossed, table to the
last hit`, the first placement with as many instants as the hit that arrives last needs (these trees reach the goal in more than 600
steps: only there is a hit crossed at all).  Times are host wall
clock around the synchronous calls, warmed, median of `--reps` with the lowest and the highest.  The old pass commits, so each of its
repetitions runs on a twin engine freshly loaded with the same tree (outside the timing).

    python tools/clear_connect_bench.py [--nodes 10000,100000] [--discs 15,63] [--reps 3] [--out DIR]
                                                            ->  one JSON line per (nodes, D, placement); DIR/clear_connect_bench.jsonl
    python tools/clear_connect_bench.py --once --nodes 100000 --discs 15   ->  one untimed new call per placement (for a kernel trace)
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

import retain_reference as rr                          # noqa: E402
from clear_bench import L, WAVE, grown                 # noqa: E402

TRIES, NO_INCUMBENT = 8, 2 ** 31 - 1


def twin_of(s, eng, arrays, H):
    """A second engine with the same tree, loaded from the first one's arrays."""
    from lqrrt_amd.engine import Engine
    state, K, pID, elen, xedge, uedge = arrays
    kw = s.plan_kwargs
    twin = Engine(s, capacity=len(pID) + 2 * WAVE + 8, max_wave=WAVE)
    twin.set_resolution(kw["dt"], kw["FPR"], H, np.abs(s.error_tol), s.goal, np.abs(s.goal_buffer))
    live = np.arange(xedge.shape[1])[None, :] < elen[:, None]
    twin.tree_load(state, K, pID, elen, np.ascontiguousarray(xedge[live]), np.ascontiguousarray(uedge[live]))
    return twin


def crossed_tracks(s, eng, arrays, D, instants=L):
    """The tree's goal hits shared among D discs (see the module's text).  instants None: a table just long enough for the hit that
    arrives last."""
    state, _, pID, elen, _, _ = arrays
    _, _, dwell = eng.tree_clear(np.full((1, 1, 2), 1e4), 0.5, per_node=True)
    arrival = np.zeros(len(pID), dtype=np.int64)
    for v in range(1, len(pID)):
        arrival[v] = arrival[pID[v]] + elen[v]
    hits = np.flatnonzero(dwell != -2)
    if instants is None:
        instants = int(arrival[hits].max()) + 2 if len(hits) else L
    hits = [int(h) for h in hits if arrival[h] < instants]
    hits.sort(key=lambda h: (arrival[h], h))
    tracks = np.full((instants, D, 2), 1e4)
    corner = np.asarray(s.vps, dtype=np.float64).reshape(2, -1)[:, 0]
    for k, h in enumerate(hits):
        x, y, a = state[h, :3]
        tracks[arrival[h], k % D] = (x + np.cos(a) * corner[0] - np.sin(a) * corner[1], y + np.sin(a) * corner[0] + np.cos(a) * corner[1])
    return tracks


def old_pass(twin, tracks, radii, H, elen0):
    """One pass of the route the earlier calls offer.  Returns (winner or None, its chain is clear)."""
    st, first, _ = twin.tree_clear(tracks, radii, 0, per_node=True)
    ids = np.flatnonzero(first == -1).astype(np.int32)
    incumbent = st["best_steps"] - elen0 + 1 if st["best_end"] >= 0 else NO_INCUMBENT
    win = twin.connect_search(H, incumbent, TRIES, ids) if len(ids) else None
    if win is None:
        return None, False
    new = twin.connect_commit(win[1], H, TRIES)
    _, first, dwell = twin.tree_clear(tracks, radii, 0, per_node=True)
    return win, bool(first[new[-1]] == -1 and dwell[new[-1]] == -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", default="10000,100000")
    ap.add_argument("--discs", default="15,63")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--once", action="store_true", help="one untimed new call per configuration (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for nodes in [int(v) for v in a.nodes.split(",")]:
        s, eng = grown(nodes)
        N = eng.size
        H = int(s.plan_kwargs["horizon"] / s.plan_kwargs["dt"])
        arrays = rr.engine_arrays(eng)
        elen0 = int(arrays[3][0])
        for D in [int(v) for v in a.discs.split(",")]:
            radii = np.full(D, 0.5)
            for placement, tracks in (("crossed", crossed_tracks(s, eng, arrays, D)), ("far", np.full((L, D, 2), 1e4)),
                                      ("crossed, table to the last hit", crossed_tracks(s, eng, arrays, D, None))):
                ts, new = [], None
                for rep in range(1 if a.once else a.reps + 1):          # (the first pass warms up and is not counted)
                    t0 = time.perf_counter()
                    new = eng.tree_clear_connect(tracks, radii, 0, H, TRIES, per_node=True)
                    if rep:
                        ts.append(1e3 * (time.perf_counter() - t0))
                st, ch = new[0], new[1]
                if a.once:
                    print(json.dumps(dict(nodes=N, discs=D, placement=placement, stats=st, chain=ch)), flush=True)
                    continue
                told, olds = [], []
                for rep in range(a.reps + 1):
                    twin = twin_of(s, eng, arrays, H)
                    twin.tree_clear(tracks, radii, 0)                   # (the twin's first call: not the pass's to pay)
                    t0 = time.perf_counter()
                    got = old_pass(twin, tracks, radii, H, elen0)
                    if rep:
                        told.append(1e3 * (time.perf_counter() - t0))
                    olds.append(got)
                    twin.close()
                win, clear = olds[-1]
                assert all(o == olds[-1] for o in olds)
                if clear:                                               # the first pass's chain is clear: it is the new call's winner
                    assert win == (ch["chain_cost"], ch["chain_from"]), (win, ch)
                row = dict(case="boat_advanced grown", nodes=N, discs=D, instants=len(tracks), placement=placement, hits=st["hits"],
                           clear_hits=st["clear_hits"], clear_candidates=ch["clear_candidates"], chain_from=ch["chain_from"],
                           chain_cost=ch["chain_cost"], new_ms=round(float(np.median(ts)), 3), new_ms_min=round(min(ts), 3),
                           new_ms_max=round(max(ts), 3), old_pass_ms=round(float(np.median(told)), 3), old_pass_ms_min=round(min(told), 3),
                           old_pass_ms_max=round(max(told), 3), old_pass_winner=None if win is None else list(win), old_pass_chain_clear=clear,
                           new_median_below_old_lowest=bool(np.median(ts) < min(told)))
                rows.append(row)
                print(json.dumps(row), flush=True)
        eng.close()
    if a.out and rows:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "clear_connect_bench.jsonl"), "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    main()
