#!/usr/bin/env python
"""
A fleet of cars, each with a tree of its own, checks its plans against tracked traffic in ONE call: avoids(connect=8).  Two of the
vehicles find every plan of their tree crossed -- a disc sweeps over each goal hit at the instant the vehicle would arrive there --
and adopt a goal chain that leaves from a node whose root path is clear; the others see far traffic and keep the best clear hit
their trees already hold.  The whole fleet costs one query on the device (the clearance stages, one seed and one search launch over
all trees) and one commit over the vehicles whose chain won, instead of a loop of Planner.avoid(connect=8) calls (INTEGRATION.md
section 7).

    python examples/fleet_clear_connect_gpu.py
"""
from __future__ import division

import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lqrrt_amd as lqrrt  # noqa: E402
from lqrrt_amd.engine import Engine  # noqa: E402

car = lqrrt.systems.Car(0)


def plan(seed):
    np.random.seed(seed)
    constraints = lqrrt.Constraints(nstates=car.nstates, ncontrols=car.ncontrols, goal_buffer=car.goal_buffer,
                                    is_feasible=car.is_feasible)
    p = lqrrt.Planner(car.dynamics, car.lqr, constraints, horizon=5, dt=0.1, FPR=0, error_tol=car.error_tol, erf=car.erf,
                      min_time=2, max_time=3, max_nodes=300, goal0=car.goal, sys_time=lambda: 0.0, printing=False, wave_size=256)
    p.update_plan(car.x0, car.sample_space, goal_bias=car.goal_bias, xrand_gen=10, finish_on_goal=False)
    return p


def crossing_traffic(p):
    """One disc per goal hit of p's tree: on the hit at the instant the vehicle arrives there, far away at every other instant."""
    eng = p._engine
    _, _, dwell = eng.tree_clear(np.full((1, 1, 2), 1e3), 0.3, per_node=True)
    parents, lengths, states = eng.parents(), eng.edge_lengths(), eng.states()
    arrival = np.zeros(len(parents), dtype=np.int64)                # index of a node's last row in a plan's x_seq
    for v in range(1, len(parents)):
        arrival[v] = arrival[parents[v]] + lengths[v]
    hits = np.flatnonzero(dwell != -2)
    tracks = np.full((int(arrival.max()) + 9 * p.horizon_iters, len(hits), 2), 1e3)
    for d, h in enumerate(hits):
        x, y, heading = states[h, :3]
        corner = car.vps[:, 0]
        tracks[arrival[h], d] = (x + np.cos(heading) * corner[0] - np.sin(heading) * corner[1],
                                 y + np.sin(heading) * corner[0] + np.cos(heading) * corner[1])
    return tracks


fleet = [plan(seed) for seed in (1, 2, 3, 4)]
print("planned: trees of %s nodes" % [p.tree.size for p in fleet])
far = np.full((40, 2, 2), 1e3)
tracks = [crossing_traffic(fleet[0]), far, crossing_traffic(fleet[2]), far]
radii = [0.3] * len(fleet)

plain = lqrrt.avoids(fleet, tracks, radii, adopt=False)
print("avoids alone: clear hits per vehicle %s" % [out["clear_hits"] for out in plain])

# count the native calls the fleet makes
calls = dict(query=0, commit=0)
for name, key in (("tree_clear_connect_multi", "query"), ("connect_commit_multi", "commit")):
    def counted(*a, _real=getattr(Engine, name), _key=key, **kw):
        calls[_key] += 1
        return _real(*a, **kw)
    setattr(Engine, name, staticmethod(counted))

sizes = [p.tree.size for p in fleet]
t0 = time.perf_counter()
outs = lqrrt.avoids(fleet, tracks, radii, connect=8)
ms = 1e3 * (time.perf_counter() - t0)
for k, (p, out) in enumerate(zip(fleet, outs)):
    if out["chain_committed"]:
        print("vehicle %d adopted a chain: from node %d, %d rows, cost %d steps, tree %d -> %d nodes, T = %.1f s" % (
            k, out["chain_from"], out["chain_rows"], out["chain_cost"], sizes[k], p.tree.size, p.T))
    elif out["best_end"] < 0:
        print("vehicle %d found neither a clear hit nor a clear chain and keeps its plan" % k)
    else:
        print("vehicle %d kept its best clear hit: node %d of %d clear hits, T = %.1f s" % (k, out["best_end"], out["clear_hits"], p.T))
words = {1: "one"}
print("avoids(connect=8) in %.1f ms: %s query, %s commit for %d vehicles" % (
    ms, words.get(calls["query"], calls["query"]), words.get(calls["commit"], calls["commit"]), len(fleet)))

again = lqrrt.avoids(fleet, tracks, radii, adopt=False)
print("checked again: plan_first per vehicle %s" % [out["plan_first"] for out in again])
