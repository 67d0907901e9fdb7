#!/usr/bin/env python
"""
Two boats whose routes cross: one plans from (0, 0) to (40, 40), the other from (40, 0) to (0, 40), each against the static map
only, as if it were alone, and they would be in the middle at about the same time.  The first keeps its plan.  The second asks
its own tree for the best plan that stays clear of the first (lqrrt_amd.deconflict, DESIGN.md sections 16 and 17) -- once as the
tree stands, where the only answers are "another way round" or "none", and once with max_wait: it may also hold station at its
start for up to MAX_WAIT rows of dt and leave later.  All delays are answered by one call on the device; the rows of the wait
are part of the adopted plan (planner.plan_wait of them, in front of x_seq), so a third boat would see the second one waiting.

    python examples/fleet_wait_gpu.py
"""
from __future__ import division

import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lqrrt_amd as lqrrt  # noqa: E402

MAX_WAIT = 63                                           # rows of dt = 0.1 s the second boat may stand at its start
routes = [(np.array([0.0, 0.0]), np.array([40.0, 40.0])), (np.array([40.0, 0.0]), np.array([0.0, 40.0]))]


def boat(k):
    s = lqrrt.systems.BoatAdvanced(0)
    s.set_obstacles(np.zeros((0, 3)))                   # open water: the other boat is the only obstacle
    a, b = routes[k]
    heading = float(np.arctan2(b[1] - a[1], b[0] - a[0]))
    s.x0 = np.array([a[0], a[1], heading, 0.0, 0.0, 0.0])
    s.goal = [float(b[0]), float(b[1]), heading, 0.0, 0.0, 0.0]
    s.goal_buffer = [4.0, 4.0] + list(s.goal_buffer[2:])
    constraints = lqrrt.Constraints(nstates=s.nstates, ncontrols=s.ncontrols, goal_buffer=s.goal_buffer, is_feasible=s.is_feasible)
    p = lqrrt.Planner(s.dynamics, s.lqr, constraints, error_tol=s.error_tol, erf=s.erf, min_time=2, max_time=3, max_nodes=3000,
                      goal0=s.goal, sys_time=lambda: 0.0, printing=False, wave_size=256, **s.plan_kwargs)
    np.random.seed(k + 1)
    space = [(-5.0, 45.0), (-5.0, 45.0)] + list(s.sample_space[2:])
    p.update_plan(s.x0, space, goal_bias=s.goal_bias, xrand_gen=10)
    print("boat %d: reached goal: %s, tree of %d nodes, T = %.1f s" % (k, p.plan_reached_goal, p.tree.size, p.T))
    return p


def closest(a, b):
    """Smallest distance between two plans at the same instant, each boat waiting at its last pose once it has arrived."""
    n = max(len(a.x_seq), len(b.x_seq))
    pa = np.array([a.x_seq[min(t, len(a.x_seq) - 1)][:2] for t in range(n)])
    pb = np.array([b.x_seq[min(t, len(b.x_seq) - 1)][:2] for t in range(n)])
    return float(np.min(np.linalg.norm(pa - pb, axis=1)))


planners = [boat(0), boat(1)]
RADIUS = 1.15 * closest(*planners)                      # each boat, seen by the other, is a disc: the plans as they are just touch
print("closest approach of the plans before: %.2f m; the boats keep %.2f m apart" % (closest(*planners), RADIUS))
t0 = time.perf_counter()
plain = planners[1].avoid([np.asarray(planners[0].x_seq)[:, :2]], RADIUS, adopt=False)
t1 = time.perf_counter()
print("as the tree stands (%.1f ms): %d of %d goal hits clear, best %s" % (
    1e3 * (t1 - t0), plain["clear_hits"], plain["hits"],
    "none" if plain["best_end"] < 0 else "node %d after %.1f s" % (plain["best_end"], plain["best_steps"] * planners[1].dt)))
t0 = time.perf_counter()
r = lqrrt.deconflict(planners, RADIUS, max_wait=MAX_WAIT)[1]
t1 = time.perf_counter()
if r["best_end"] < 0:
    print("with up to %d rows of waiting (%.1f ms): still nothing clear" % (MAX_WAIT, 1e3 * (t1 - t0)))
else:
    dt = planners[1].dt
    print("with up to %d rows of waiting (%.1f ms): %d of %d goal hits clear at some delay (%d at once); best: wait %.1f s, then node %d, "
          "arriving after %.1f s" % (MAX_WAIT, 1e3 * (t1 - t0), r["clear_hits"], r["hits"], r["clear_now"], r["best_wait"] * dt,
                                     r["best_end"], r["best_arrival"] * dt))
    print("the second boat's plan now stands still for its first %d rows; closest approach after: %.2f m" % (planners[1].plan_wait, closest(*planners)))
