#!/usr/bin/env python
"""
A tree rooted at the vehicle answers more than the one question it was grown for.  A car plans to its goal; Planner.goal_costs then
asks the SAME tree what it would cost to drive to three other places instead (one kernel launch for all of them, one wavefront per
tree node and goal), and Planner.retarget makes the cheapest of them the planner's goal and plan without sampling again
(DESIGN.md section 14).

    python examples/retarget_gpu.py
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
                        min_time=2, max_time=3, max_nodes=400, goal0=car.goal, sys_time=lambda: 0.0, printing=False, wave_size=256)

planner.update_plan(car.x0, car.sample_space, goal_bias=car.goal_bias, xrand_gen=10)
print("plan to the first goal: reached goal: %s, tree of %d nodes, T = %.1f s, the plan ends at %s" % (
    planner.plan_reached_goal, planner.tree.size, planner.T, np.round(planner.x_seq[-1], 2)))

# three other places: x, y, heading, speed, steering
alternatives = np.array([[60.0, 10.0, 0.0, 0.0, 0.0],
                         [20.0, 20.0, 0.0, 0.0, 0.0],
                         [30.0, 10.0, 0.0, 0.0, 0.0]])
t0 = time.perf_counter()
steps, nodes = planner.goal_costs(alternatives, goal_tries=8)
print("goal_costs of %d goals in %.1f ms (tree, plan and goal unchanged: T = %.1f s)" % (
    len(alternatives), 1e3 * (time.perf_counter() - t0), planner.T))
for k in range(len(alternatives)):
    if steps[k] < 0:
        print("  alternative %d: no chain from this tree reaches %s" % (k + 1, alternatives[k][:2]))
    else:
        print("  alternative %d: %.1f s, leaving the tree at node %d, to %s" % (k + 1, steps[k] * planner.dt, nodes[k], alternatives[k][:2]))

reachable = [k for k in range(len(alternatives)) if steps[k] >= 0]
if reachable:
    best = min(reachable, key=lambda k: (steps[k], k))
    t0 = time.perf_counter()
    moved = planner.retarget(alternatives[best], goal_tries=8)
    print("retarget to alternative %d in %.1f ms: %s, reached goal: %s, T = %.1f s, the plan ends at %s" % (
        best + 1, 1e3 * (time.perf_counter() - t0), moved, planner.plan_reached_goal, planner.T, np.round(planner.x_seq[-1], 2)))
    rounds = planner.refine_plan(max_rounds=8, goal_tries=8)
    print("refine_plan toward the new goal, %d round(s): T = %.1f s" % (rounds, planner.T))
    print("state at t = T:", np.round(planner.get_state(planner.T), 3))
