#!/usr/bin/env python
"""
A plan-drive-plan loop often holds the rest of a good plan that its current tree no longer contains: the tree was cut back by a
replan, or this tick's budget ran out on a tree that has not grown as far as the last one did.  Planner.connect_via takes those
states as waypoints: from ANY node of the tree, steer through the waypoints and then at the goal (one kernel launch, one wavefront
per (node, first waypoint) pair).  Here a long run finds a plan; a run stopped at 107 nodes finds none, and connect_goal cannot
help it either -- no short chain of goal steers reaches the goal from so small a tree; the long run's plan beyond the small tree
does.  What connect_via cannot do: a chain does not steer round an obstacle that blocks it.

    python examples/connect_via_gpu.py
"""
from __future__ import division

import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lqrrt_amd as lqrrt  # noqa: E402


def run(max_nodes):
    np.random.seed(1)
    car = lqrrt.systems.Car(0)
    constraints = lqrrt.Constraints(nstates=car.nstates, ncontrols=car.ncontrols, goal_buffer=car.goal_buffer,
                                    is_feasible=car.is_feasible)
    planner = lqrrt.Planner(car.dynamics, car.lqr, constraints, horizon=5, dt=0.1, FPR=0, error_tol=car.error_tol, erf=car.erf,
                            min_time=2, max_time=3, max_nodes=max_nodes, goal0=car.goal, sys_time=lambda: 0.0, printing=False,
                            wave_size=256)
    planner.update_plan(car.x0, car.sample_space, goal_bias=car.goal_bias, xrand_gen=10)
    return planner


long_run = run(500)
print("long run: tree of %d nodes, reached goal: %s, T = %.1f s" % (long_run.tree.size, long_run.plan_reached_goal, long_run.T))

planner = run(107)
print("budget spent: tree of %d nodes, reached goal: %s, T = %.1f s, the plan ends at %s" % (
    planner.tree.size, planner.plan_reached_goal, planner.T, np.round(planner.x_seq[-1], 2)))
print("connect_goal: %s" % planner.connect_goal(goal_tries=8))

# the long run's plan beyond what the small tree holds (the same seed grows the same first nodes)
start = next(k for k, v in enumerate(long_run.node_seq) if v >= planner.tree.size)
waypoints = long_run.plan_waypoints(start)
t0 = time.perf_counter()
found = planner.connect_via(waypoints, goal_tries=8)
print("connect_via over %d waypoints in %.1f ms: %s, reached goal: %s, T = %.1f s, the plan ends at %s" % (
    len(waypoints), 1e3 * (time.perf_counter() - t0), found, planner.plan_reached_goal, planner.T, np.round(planner.x_seq[-1], 2)))

t0 = time.perf_counter()
rounds = planner.refine_plan(max_rounds=8, goal_tries=8)
print("refine_plan in %.1f ms, %d round(s): T = %.1f s" % (1e3 * (time.perf_counter() - t0), rounds, planner.T))
print("state at t = T:", np.round(planner.get_state(planner.T), 3))
