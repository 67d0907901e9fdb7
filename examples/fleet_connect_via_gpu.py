#!/usr/bin/env python
"""
A fleet that replans every tick and keeps what it found, on ONE MI355X.  Tick one: every car plans until its tree reaches the goal
(lqrrt_amd.update_plans) and saves the states of its plan (planner.plan_waypoints()).  Tick two: the same query with a tenth of the
node budget -- update_plans grows new trees, the old ones and their plans are gone, and most budgets end before a goal hit: the
plans are the fallback.  lqrrt_amd.connect_vias then asks every car's WHOLE new tree from which node a chain through the rest of
that car's OWN saved plan reaches the goal: the searches of all trees share ONE kernel launch (every tree with its own waypoint
table and best key) and the winners' chains are appended in ONE more; per car the result is exactly that of its own
planner.connect_via(saved).  lqrrt_amd.refine_plans shortens what was found, again through shared launches (INTEGRATION.md
section 7).

    python examples/fleet_connect_via_gpu.py [n_cars]
"""
from __future__ import division

import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lqrrt_amd as lqrrt  # noqa: E402

n_cars = int(sys.argv[1]) if len(sys.argv) > 1 else 8

small_budget = 107                                                # seed 1's first goal hit is node 217


def make_planner():
    car = lqrrt.systems.Car(0)
    constraints = lqrrt.Constraints(nstates=car.nstates, ncontrols=car.ncontrols, goal_buffer=car.goal_buffer,
                                    is_feasible=car.is_feasible)
    # the clock stands still: tick one ends at the first goal hit (min_time = 0), and every run repeats
    planner = lqrrt.Planner(car.dynamics, car.lqr, constraints, horizon=5, dt=0.1, FPR=0, error_tol=car.error_tol, erf=car.erf,
                            min_time=0, max_time=10, max_nodes=3000, goal0=car.goal, sys_time=lambda: 0.0, printing=False,
                            wave_size=256)
    return car, planner


fleet = [make_planner() for _ in range(n_cars)]
planners = [planner for _, planner in fleet]


def jobs():
    return [dict(planner=planner, x0=car.x0, sample_space=car.sample_space, goal_bias=car.goal_bias, xrand_gen=10, seed=1 + k)
            for k, (car, planner) in enumerate(fleet)]


def report(label, seconds, extra=""):
    print("%s in %.1f ms: %d of %d plans reach the goal%s; T = %s s" % (
        label, 1e3 * seconds, sum(bool(p.plan_reached_goal) for p in planners), n_cars, extra, [round(float(p.T), 1) for p in planners]))


t0 = time.perf_counter()
lqrrt.update_plans(jobs())
report("tick one: update_plans", time.perf_counter() - t0, ", trees of %s nodes" % [p.tree.size for p in planners])
saved = [p.plan_waypoints() if p.plan_reached_goal else None for p in planners]    # the plans' states outlive their trees

for p in planners:
    p.set_runtime(min_time=2, max_time=3, max_nodes=small_budget)                  # the budget is now the node limit
t0 = time.perf_counter()
lqrrt.update_plans(jobs())
report("tick two: update_plans", time.perf_counter() - t0, ", trees of %s nodes" % [p.tree.size for p in planners])

t0 = time.perf_counter()
found = lqrrt.connect_vias(planners, saved, goal_tries=8)
report("connect_vias", time.perf_counter() - t0, " over %s waypoints, connected %s" % ([0 if w is None else len(w) for w in saved],
                                                                                      [int(f) for f in found]))

t0 = time.perf_counter()
rounds = lqrrt.refine_plans(planners, max_rounds=8, goal_tries=8)
report("refine_plans", time.perf_counter() - t0, ", rounds %s" % rounds)
