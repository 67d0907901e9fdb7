#!/usr/bin/env python
"""
A fleet in a plan-drive-plan loop on ONE MI355X: lqrrt_amd.update_plans with a `root` per boat.

Every tick each boat has driven a little further along its plan.  Instead of planning from scratch (update_plan: the tree is thrown
away and the goal has to be found again) each boat keeps the part of its tree that hangs below the plan node it will have reached
when the new plan is ready -- `planner.plan_node_after(t)` -- and grows that on: Planner.replan for a whole fleet.  One boat's map
gains an obstacle every tick; with `revalidate` (the default) the kept edges are tested against the map as it is now and whatever
hangs below a blocked edge is dropped.  All trees of the fleet are kept by one batched native call and grown by shared ones.

    python examples/fleet_replan_gpu.py [n_boats] [ticks]
"""
from __future__ import division

import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lqrrt_amd as lqrrt  # noqa: E402

n_boats = int(sys.argv[1]) if len(sys.argv) > 1 else 16
ticks = int(sys.argv[2]) if len(sys.argv) > 2 else 4
tick_time = 0.25                                                  # seconds of planning per tick, and of driving between two plans
budget = dict(min_time=tick_time, max_time=tick_time, max_nodes=100000)


def make_planner():
    boat = lqrrt.systems.BoatAdvanced(obstacle_seed=0)
    constraints = lqrrt.Constraints(nstates=boat.nstates, ncontrols=boat.ncontrols, goal_buffer=boat.goal_buffer,
                                    is_feasible=boat.is_feasible)
    planner = lqrrt.Planner(boat.dynamics, boat.lqr, constraints, horizon=2, dt=0.1, FPR=0.9, error_tol=boat.error_tol,
                            erf=boat.erf, goal0=boat.goal, printing=False, wave_size=256, **budget)
    return boat, planner


fleet = [make_planner() for _ in range(n_boats)]
starts = [np.array(boat.x0, dtype=np.float64) + np.array([0.5 * k, 0.0, 0.0, 0.0, 0.0, 0.0]) for k, (boat, _) in enumerate(fleet)]

# the first plan of every boat: from its start state
t0 = time.time()
lqrrt.update_plans([dict(planner=planner, x0=starts[k], sample_space=boat.sample_space, goal_bias=boat.goal_bias, seed=100 + k)
                    for k, (boat, planner) in enumerate(fleet)])
print("first plans: %d boats in %.2f s, tree sizes %s, %d reached the goal" % (
    n_boats, time.time() - t0, [p.tree.size for _, p in fleet], sum(bool(p.plan_reached_goal) for _, p in fleet)))

for tick in range(1, ticks + 1):
    # where every boat will be when its next plan is ready: the first node of its plan at or after one tick of driving
    roots = [planner.plan_node_after(tick_time)[1] for _, planner in fleet]
    # one boat sees something new: a circle 4 m beside the middle of the plan it is driving
    boat, planner = fleet[tick % n_boats]
    mid = planner.tree.state[planner.node_seq[len(planner.node_seq) // 2]]
    boat.set_obstacles(np.vstack((np.asarray(boat.obs, dtype=np.float64).reshape(-1, 3), [mid[0] + 4.0, mid[1], 1.0])))
    t0 = time.time()
    results = lqrrt.update_plans([dict(planner=planner, root=roots[k], sample_space=boat.sample_space, goal_bias=boat.goal_bias,
                                       seed=1000 * tick + k) for k, (boat, planner) in enumerate(fleet)])
    dt_tick = time.time() - t0
    kept = [p.retained["kept"] for _, p in fleet]
    grown = [p.tree.size - p.retained["kept"] for _, p in fleet]
    print("tick %d: %.2f s, boat %d saw a new obstacle; kept %s of %s nodes, grown %s; dropped by the new map %s; plans %s s, %d reach the goal"
          % (tick, dt_tick, tick % n_boats, kept, [p.retained["old_size"] for _, p in fleet], grown,
             [p.retained["infeasible"] + p.retained["orphaned"] for _, p in fleet], [round(float(p.T), 1) for _, p in fleet],
             sum(bool(p.plan_reached_goal) for _, p in fleet)))
