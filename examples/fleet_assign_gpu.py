#!/usr/bin/env python
"""
A fleet and a shared list of berths, on ONE MI355X: every car grows a tree toward its first goal (lqrrt_amd.update_plans).
lqrrt_amd.fleet_goal_costs then asks EVERY tree what it would cost to drive to EVERY berth instead -- the cars x berths assignment
matrix, the searches of all trees for all berths in ONE kernel launch, every (tree, berth) pair with a best key of its own; row k is
exactly planners[k].goal_costs(berths).  A greedy assignment is drawn from the matrix in plain Python (cheapest pair first; an
optimal solver is the caller's business), and lqrrt_amd.retargets gives every car its berth as goal and plan without sampling
again: one search launch and one commit launch for the fleet.

    python examples/fleet_assign_gpu.py [n_cars]
"""
from __future__ import division

import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lqrrt_amd as lqrrt  # noqa: E402

n_cars = int(sys.argv[1]) if len(sys.argv) > 1 else 4


def make_planner():
    car = lqrrt.systems.Car(0)
    constraints = lqrrt.Constraints(nstates=car.nstates, ncontrols=car.ncontrols, goal_buffer=car.goal_buffer,
                                    is_feasible=car.is_feasible)
    # the clock stands still: the budget is the node limit, and the run repeats
    planner = lqrrt.Planner(car.dynamics, car.lqr, constraints, horizon=5, dt=0.1, FPR=0, error_tol=car.error_tol, erf=car.erf,
                            min_time=2, max_time=3, max_nodes=400, goal0=car.goal, sys_time=lambda: 0.0, printing=False, wave_size=256)
    return car, planner


fleet = [make_planner() for _ in range(n_cars)]
planners = [planner for _, planner in fleet]

t0 = time.perf_counter()
lqrrt.update_plans([dict(planner=planner, x0=car.x0, sample_space=car.sample_space, goal_bias=car.goal_bias, xrand_gen=10, seed=1 + k)
                    for k, (car, planner) in enumerate(fleet)])
print("update_plans in %.1f ms: trees of %s nodes, %d of %d plans reach the first goal" % (
    1e3 * (time.perf_counter() - t0), [p.tree.size for p in planners], sum(bool(p.plan_reached_goal) for p in planners), n_cars))

# the berths: x, y, heading, speed, steering
berths = np.array([[60.0, 10.0, 0.0, 0.0, 0.0],
                   [20.0, 20.0, 0.0, 0.0, 0.0],
                   [30.0, 10.0, 0.0, 0.0, 0.0],
                   [45.0, 15.0, 0.0, 0.0, 0.0],
                   [35.0, 25.0, 0.0, 0.0, 0.0]])
t0 = time.perf_counter()
steps, nodes = lqrrt.fleet_goal_costs(planners, berths, goal_tries=8)
print("fleet_goal_costs, %d cars x %d berths in %.1f ms (trees, plans and goals unchanged); seconds to each berth, -: no chain:" % (
    n_cars, len(berths), 1e3 * (time.perf_counter() - t0)))
for k, p in enumerate(planners):
    print("  car %d: %s" % (k + 1, "  ".join("%6.1f" % (steps[k, t] * p.dt) if steps[k, t] >= 0 else "     -" for t in range(len(berths)))))

# greedy: the cheapest (car, berth) pair first, every car and every berth at most once
pairs = sorted((int(steps[k, t]), k, t) for k in range(n_cars) for t in range(len(berths)) if steps[k, t] >= 0)
berth_of, taken = {}, set()
for cost, k, t in pairs:
    if k not in berth_of and t not in taken:
        berth_of[k] = t
        taken.add(t)
print("assignment (car -> berth): %s" % ", ".join("%d -> %d" % (k + 1, berth_of[k] + 1) for k in sorted(berth_of)))

t0 = time.perf_counter()
moved = lqrrt.retargets(planners, [berths[berth_of[k]] if k in berth_of else None for k in range(n_cars)], goal_tries=8)
print("retargets in %.1f ms: %s" % (1e3 * (time.perf_counter() - t0), [bool(m) for m in moved]))
for k, p in enumerate(planners):
    if moved[k]:
        print("  car %d: berth %d, reached goal: %s, T = %.1f s (the matrix said %.1f s), the plan ends at %s" % (
            k + 1, berth_of[k] + 1, p.plan_reached_goal, p.T, steps[k, berth_of[k]] * p.dt, np.round(p.x_seq[-1], 2)))
    else:
        print("  car %d: stays with its first goal, T = %.1f s" % (k + 1, p.T))
rounds = lqrrt.refine_plans(planners, max_rounds=8, goal_tries=8)
print("refine_plans toward the new goals, rounds %s: T = %s s" % (rounds, [round(float(p.T), 1) for p in planners]))
