#!/usr/bin/env python
"""
A fleet checks its plans against tracked traffic every tick.  Six cars plan to the same goal region against the static map only.
Then traffic appears that is no part of the fleet -- three discs on straight lines through the map, known for the next 90 s -- and
at every tick of 1 s all six trees are asked, as they stand, for their best plan that stays clear of it: lqrrt_amd.avoids, ONE
native call for the whole fleet whose every stage is one kernel launch over all the trees, the traffic table uploaded once
(DESIGN.md section 18).  A car may answer by leaving up to 10 rows of dt later (max_wait).  The loop of planner.avoid calls that
this replaces is timed next to it on a second, identical fleet, and must leave the same plans.

    python examples/fleet_avoid_gpu.py
"""
from __future__ import division

import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lqrrt_amd as lqrrt  # noqa: E402

STARTS = [(0.0, 0.0), (0.0, 30.0), (30.0, 0.0), (0.0, 15.0), (15.0, 0.0), (5.0, 5.0)]
DT, TICK, MAX_WAIT = 0.1, 10, 10                         # a tick is 10 rows of dt


def fleet():
    planners = []
    for k, (x, y) in enumerate(STARTS):
        car = lqrrt.systems.Car(0)
        constraints = lqrrt.Constraints(nstates=car.nstates, ncontrols=car.ncontrols, goal_buffer=car.goal_buffer,
                                        is_feasible=car.is_feasible)
        p = lqrrt.Planner(car.dynamics, car.lqr, constraints, horizon=5, dt=DT, FPR=0, error_tol=car.error_tol, erf=car.erf,
                          min_time=2, max_time=3, max_nodes=1500, goal0=car.goal, sys_time=lambda: 0.0, printing=False, wave_size=256)
        np.random.seed(k + 1)
        p.update_plan(np.array([x, y, 0.0, 0.0, 0.0]), car.sample_space, goal_bias=car.goal_bias, xrand_gen=10)
        planners.append(p)
    return planners


def traffic(planners, L=900):
    """Three discs, each on a straight line that crosses one car's plan at the moment that car is there."""
    tracks = np.zeros((L, 3, 2))
    t = np.arange(L, dtype=np.float64)
    for d, p in enumerate(planners[:3]):
        rows = np.asarray(p.x_seq, dtype=np.float64)
        c = len(rows) // 4                              # (T is 110 .. 200 s here: row c lies well inside the L instants)
        heading = rows[c, 2] + np.pi / 2
        tracks[:, d] = rows[c, :2] + 0.3 * (t - c)[:, None] * np.array([np.cos(heading), np.sin(heading)])
    return tracks, np.array([1.5, 1.0, 2.0])


planners, twins = fleet(), fleet()
for k, p in enumerate(planners):
    print("car %d from %s: reached goal: %s, tree of %d nodes, T = %.1f s" % (k, STARTS[k], p.plan_reached_goal, p.tree.size, p.T))
tracks, radii = traffic(planners)
t_fleet = t_loop = 0.0
for tick in range(4):
    start = tick * TICK                                 # the plans' first row is the traffic's row `start`: the world has moved on, the cars have not yet
    t0 = time.perf_counter()
    got = lqrrt.avoids(planners, tracks, radii, start=start, max_wait=MAX_WAIT)
    t1 = time.perf_counter()
    want = [q.avoid(tracks, radii, start=start, max_wait=MAX_WAIT) for q in twins]
    t2 = time.perf_counter()
    assert got == want and all(list(p.node_seq) == list(q.node_seq) and p.plan_wait == q.plan_wait for p, q in zip(planners, twins))
    if tick:                                            # (the first tick warms up)
        t_fleet, t_loop = t_fleet + (t1 - t0), t_loop + (t2 - t1)
    print("tick %d (traffic row %d):" % (tick, start))
    for k, r in enumerate(got):
        if r["best_end"] < 0:
            print("  car %d: no plan of its tree is clear (%d goal hits); first conflict of its plan at %s s" % (k, r["hits"], None if r["plan_first"] is None else round(r["plan_first"], 1)))
        else:
            print("  car %d: %d of %d goal hits clear (%d at once); its plan had %s; leaves after %d rows, arrives after %d (node %d)"
                  % (k, r["clear_hits"], r["hits"], r["clear_now"], "no conflict" if r["plan_first"] is None else
                     "its first conflict at %.1f s" % r["plan_first"], r["best_wait"], r["best_arrival"], r["best_end"]))
print("three ticks: avoids %.2f ms, the loop of avoid %.2f ms" % (1e3 * t_fleet, 1e3 * t_loop))
