#!/usr/bin/env python
"""
A fleet whose budgets are too small for a goal hit, on ONE MI355X: every car plans with a node budget that ends before most of
the trees have reached the goal (lqrrt_amd.update_plans), so most plans are the fallback -- the path to the node nearest the goal.
lqrrt_amd.connect_goals then asks every car's WHOLE tree whether a short chain of goal-directed steers from any of its nodes reaches
the goal: the searches of all trees share ONE kernel launch (every tree with a best key of its own) and the winners' chains are
appended in ONE more; per car the result is exactly that of its own planner.connect_goal().  lqrrt_amd.refine_plans shortens what
was found, again through shared launches.

    python examples/fleet_connect_gpu.py [n_cars]
"""
from __future__ import division

import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lqrrt_amd as lqrrt  # noqa: E402

n_cars = int(sys.argv[1]) if len(sys.argv) > 1 else 8


max_nodes = 215                                                   # seed 1's first goal hit would be node 217


def make_planner():
    car = lqrrt.systems.Car(0)
    constraints = lqrrt.Constraints(nstates=car.nstates, ncontrols=car.ncontrols, goal_buffer=car.goal_buffer,
                                    is_feasible=car.is_feasible)
    # the clock stands still: the budget is the node limit, and the run repeats
    planner = lqrrt.Planner(car.dynamics, car.lqr, constraints, horizon=5, dt=0.1, FPR=0, error_tol=car.error_tol, erf=car.erf,
                            min_time=2, max_time=3, max_nodes=max_nodes, goal0=car.goal, sys_time=lambda: 0.0, printing=False,
                            wave_size=256)
    return car, planner


fleet = [make_planner() for _ in range(n_cars)]
planners = [planner for _, planner in fleet]


def report(label, seconds, extra=""):
    print("%s in %.1f ms: %d of %d plans reach the goal%s; T = %s s" % (
        label, 1e3 * seconds, sum(bool(p.plan_reached_goal) for p in planners), n_cars, extra, [round(float(p.T), 1) for p in planners]))


t0 = time.perf_counter()
lqrrt.update_plans([dict(planner=planner, x0=car.x0, sample_space=car.sample_space, goal_bias=car.goal_bias, xrand_gen=10, seed=1 + k)
                    for k, (car, planner) in enumerate(fleet)])
report("update_plans", time.perf_counter() - t0, ", trees of %s nodes" % [p.tree.size for p in planners])

t0 = time.perf_counter()
found = lqrrt.connect_goals(planners, goal_tries=8)
report("connect_goals", time.perf_counter() - t0, ", connected %s" % [int(f) for f in found])

t0 = time.perf_counter()
rounds = lqrrt.refine_plans(planners, max_rounds=8, goal_tries=8)
report("refine_plans", time.perf_counter() - t0, ", rounds %s" % rounds)
