#!/usr/bin/env python
"""
Every plan the tree holds is crossed by traffic: a disc sweeps over each goal hit at the instant the vehicle would arrive there.
Planner.avoid alone reports that no hit is clear and keeps the plan.  Planner.avoid(connect=8) asks, in the same one call on the
device, every node whose root path IS clear whether a short chain of goal-directed steers reaches the goal and stays clear of the
discs at the times the vehicle would be on it -- and adopts the shortest such chain.

    python examples/clear_connect_gpu.py
"""
from __future__ import division

import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lqrrt_amd as lqrrt  # noqa: E402

np.random.seed(1)
car = lqrrt.systems.Car(0)
constraints = lqrrt.Constraints(nstates=car.nstates, ncontrols=car.ncontrols, goal_buffer=car.goal_buffer,
                                is_feasible=car.is_feasible)
planner = lqrrt.Planner(car.dynamics, car.lqr, constraints, horizon=5, dt=0.1, FPR=0, error_tol=car.error_tol, erf=car.erf,
                        min_time=2, max_time=3, max_nodes=300, goal0=car.goal, sys_time=lambda: 0.0, printing=False, wave_size=256)
planner.update_plan(car.x0, car.sample_space, goal_bias=car.goal_bias, xrand_gen=10, finish_on_goal=False)
print("planned: tree of %d nodes, reached goal: %s, T = %.1f s" % (planner.tree.size, planner.plan_reached_goal, planner.T))

# which nodes are goal hits, and when the vehicle arrives there: the clearance query itself says so (dwell_first != -2)
eng = planner._engine
_, _, dwell = eng.tree_clear(np.full((1, 1, 2), 1e3), 0.3, per_node=True)
parents, lengths, states = eng.parents(), eng.edge_lengths(), eng.states()
arrival = np.zeros(len(parents), dtype=np.int64)                    # index of a node's last row in a plan's x_seq
for v in range(1, len(parents)):
    arrival[v] = arrival[parents[v]] + lengths[v]
hits = np.flatnonzero(dwell != -2)
L = int(arrival.max()) + 9 * planner.horizon_iters
tracks = np.full((L, len(hits), 2), 1e3)                            # far away ...
for d, h in enumerate(hits):                                        # ... but for the one instant at which hit h is reached
    x, y, heading = states[h, :3]
    corner = car.vps[:, 0]
    tracks[arrival[h], d] = (x + np.cos(heading) * corner[0] - np.sin(heading) * corner[1],
                             y + np.sin(heading) * corner[0] + np.cos(heading) * corner[1])

out = planner.avoid(tracks, 0.3)
print("avoid alone: clear_hits %d of %d hits, best_end %d, the plan's first conflict at t = %.1f s" % (
    out["clear_hits"], out["hits"], out["best_end"], out["plan_first"]))

t0 = time.perf_counter()
out = planner.avoid(tracks, 0.3, connect=8)
print("avoid(connect=8) in %.1f ms: %d clear candidates, chain from node %d, %d rows, cost %d steps, chain committed: %s" % (
    1e3 * (time.perf_counter() - t0), out["clear_candidates"], out["chain_from"], out["chain_rows"], out["chain_cost"],
    out["chain_committed"]))
print("the plan: %d nodes, T = %.1f s, reached goal: %s" % (len(planner.node_seq), planner.T, planner.plan_reached_goal))

out = planner.avoid(tracks, 0.3, adopt=False)
print("checked again: clear_hits %d, best_end %d (the plan's last node: %d), plan_first %s" % (
    out["clear_hits"], out["best_end"], planner.node_seq[-1], out["plan_first"]))
