#!/usr/bin/env python
"""
Three cars start in three corners and plan to the same goal region against the static map only, each as if it were alone.
lqrrt_amd.deconflict then treats the cars as obstacles to each other, in priority order: the first keeps its plan; every later car
asks its OWN tree, as it stands, for the best plan that stays clear of the plans of the cars before it -- discs that move along
those plans and then sit where they arrived (Planner.avoid: every recorded row of every edge tested at its own time, one call on
the device per car, the tree untouched).

    python examples/fleet_deconflict_gpu.py
"""
from __future__ import division

import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lqrrt_amd as lqrrt  # noqa: E402

RADIUS = 2.0                                            # every car, seen by the others, is a disc of this radius around its pose
starts = [(0.0, 0.0), (0.0, 30.0), (30.0, 0.0)]
planners = []
for k, (x, y) in enumerate(starts):
    car = lqrrt.systems.Car(0)
    constraints = lqrrt.Constraints(nstates=car.nstates, ncontrols=car.ncontrols, goal_buffer=car.goal_buffer,
                                    is_feasible=car.is_feasible)
    p = lqrrt.Planner(car.dynamics, car.lqr, constraints, horizon=5, dt=0.1, FPR=0, error_tol=car.error_tol, erf=car.erf,
                      min_time=2, max_time=3, max_nodes=1500, goal0=car.goal, sys_time=lambda: 0.0, printing=False, wave_size=256)
    np.random.seed(k + 1)
    p.update_plan(np.array([x, y, 0.0, 0.0, 0.0]), car.sample_space, goal_bias=car.goal_bias, xrand_gen=10)
    print("car %d from %s: reached goal: %s, tree of %d nodes, T = %.1f s" % (k, (x, y), p.plan_reached_goal, p.tree.size, p.T))
    planners.append(p)


def closest(a, b):
    """Smallest distance between two plans at the same instant, each car waiting at its last pose once it has arrived."""
    n = max(len(a.x_seq), len(b.x_seq))
    pa = np.array([a.x_seq[min(t, len(a.x_seq) - 1)][:2] for t in range(n)])
    pb = np.array([b.x_seq[min(t, len(b.x_seq) - 1)][:2] for t in range(n)])
    return float(np.min(np.linalg.norm(pa - pb, axis=1)))


print("closest approach of the plans before:", [round(closest(planners[i], planners[j]), 2) for i, j in ((0, 1), (0, 2), (1, 2))])
t0 = time.perf_counter()
results = lqrrt.deconflict(planners, RADIUS, order=[0, 1, 2])
print("deconflict in %.1f ms" % (1e3 * (time.perf_counter() - t0)))
for k, r in enumerate(results):
    if r is None:
        print("  car %d: first in the order, keeps its plan (T = %.1f s)" % (k, planners[k].T))
    elif r["best_end"] < 0:
        print("  car %d: no plan in its tree is clear (%d of %d goal hits), it keeps its plan; first conflict at %s s"
              % (k, r["clear_hits"], r["hits"], r["plan_first"]))
    else:
        print("  car %d: %d nodes in conflict, %d below them, %d of %d goal hits clear; its plan had %s; now T = %.1f s, ending at node %d"
              % (k, r["conflicts"], r["blocked"], r["clear_hits"], r["hits"],
                 "no conflict" if r["plan_first"] is None else "its first conflict at %.1f s" % r["plan_first"], planners[k].T, r["best_end"]))
print("closest approach of the plans after: ", [round(closest(planners[i], planners[j]), 2) for i, j in ((0, 1), (0, 2), (1, 2))])
