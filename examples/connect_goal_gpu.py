#!/usr/bin/env python
"""
A planner that runs out of budget before its first goal hit hands back the fallback: the path to the node nearest the goal, which
does not reach it.  Planner.connect_goal asks the tree it has just grown whether a short chain of goal-directed steers from ANY of
its nodes reaches the goal (one kernel launch, one wavefront per node), and refine_plan then shortens what it found
(INTEGRATION.md section 7).

    python examples/connect_goal_gpu.py
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
# a budget of 215 nodes: this seed's first goal hit would be node 217
planner = lqrrt.Planner(car.dynamics, car.lqr, constraints, horizon=5, dt=0.1, FPR=0, error_tol=car.error_tol, erf=car.erf,
                        min_time=2, max_time=3, max_nodes=215, goal0=car.goal, sys_time=lambda: 0.0, printing=False, wave_size=256)

planner.update_plan(car.x0, car.sample_space, goal_bias=car.goal_bias, xrand_gen=10)
print("budget spent: tree of %d nodes, reached goal: %s, T = %.1f s, the plan ends at %s" % (
    planner.tree.size, planner.plan_reached_goal, planner.T, np.round(planner.x_seq[-1], 2)))

t0 = time.perf_counter()
found = planner.connect_goal(goal_tries=8)
print("connect_goal in %.1f ms: %s, reached goal: %s, T = %.1f s, the plan ends at %s" % (
    1e3 * (time.perf_counter() - t0), found, planner.plan_reached_goal, planner.T, np.round(planner.x_seq[-1], 2)))

t0 = time.perf_counter()
rounds = planner.refine_plan(max_rounds=8, goal_tries=8)
print("refine_plan in %.1f ms, %d round(s): T = %.1f s" % (1e3 * (time.perf_counter() - t0), rounds, planner.T))
print("state at t = T:", np.round(planner.get_state(planner.T), 3))
