#!/usr/bin/env python
"""
A fleet tick on ONE MI355X: replan every boat from the node it will have reached (lqrrt_amd.update_plans with a `root` per boat),
then shorten every found plan (lqrrt_amd.refine_plans).

The tree path of a goal hit wanders: it is made of the edges the samples happened to produce.  refine_plans tries every shortcut
of every boat's plan -- from plan node i steer toward node j, the ones behind it and the goal -- and keeps the cheapest chain that
still ends in the goal region, round after round until nothing gets shorter.  The rounds of all boats share their kernel launches
(one search launch and one commit launch per round, whatever the number of boats); per boat the result is exactly that of its own
planner.refine_plan().  The shortcut's edges are appended to the boat's tree, so the next tick's replan keeps them.

    python examples/fleet_refine_gpu.py [n_boats] [ticks]
"""
from __future__ import division

import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lqrrt_amd as lqrrt  # noqa: E402

n_boats = int(sys.argv[1]) if len(sys.argv) > 1 else 16
ticks = int(sys.argv[2]) if len(sys.argv) > 2 else 3
tick_time = 0.25                                                  # seconds of planning per tick, and of driving between two plans
budget = dict(min_time=tick_time, max_time=tick_time, max_nodes=20000)


def make_planner():
    boat = lqrrt.systems.BoatAdvanced(obstacle_seed=0)
    constraints = lqrrt.Constraints(nstates=boat.nstates, ncontrols=boat.ncontrols, goal_buffer=boat.goal_buffer,
                                    is_feasible=boat.is_feasible)
    planner = lqrrt.Planner(boat.dynamics, boat.lqr, constraints, horizon=2, dt=0.1, FPR=0.9, error_tol=boat.error_tol,
                            erf=boat.erf, goal0=boat.goal, printing=False, wave_size=256, **budget)
    return boat, planner


fleet = [make_planner() for _ in range(n_boats)]
starts = [np.array(boat.x0, dtype=np.float64) + np.array([0.5 * k, 0.0, 0.0, 0.0, 0.0, 0.0]) for k, (boat, _) in enumerate(fleet)]
planners = [planner for _, planner in fleet]


def refine(label):
    before = [float(p.T) for p in planners]
    t0 = time.time()
    rounds = lqrrt.refine_plans(planners)
    print("%s: refined in %.3f s, rounds %s; plans %s s -> %s s" % (label, time.time() - t0, rounds, [round(v, 1) for v in before],
                                                                   [round(float(p.T), 1) for p in planners]))
    return rounds


t0 = time.time()
lqrrt.update_plans([dict(planner=planner, x0=starts[k], sample_space=boat.sample_space, goal_bias=boat.goal_bias, seed=100 + k)
                    for k, (boat, planner) in enumerate(fleet)])
print("first plans: %d boats in %.2f s, tree sizes %s, %d reached the goal" % (
    n_boats, time.time() - t0, [p.tree.size for p in planners], sum(bool(p.plan_reached_goal) for p in planners)))
refine("first plans")

for tick in range(1, ticks + 1):
    roots = [planner.plan_node_after(tick_time)[1] for planner in planners]
    t0 = time.time()
    lqrrt.update_plans([dict(planner=planner, root=roots[k], sample_space=boat.sample_space, goal_bias=boat.goal_bias,
                             seed=1000 * tick + k) for k, (boat, planner) in enumerate(fleet)])
    print("tick %d: replanned in %.2f s, kept %s nodes, trees %s, %d reach the goal" % (
        tick, time.time() - t0, [p.retained["kept"] for p in planners], [p.tree.size for p in planners],
        sum(bool(p.plan_reached_goal) for p in planners)))
    rounds = refine("tick %d" % tick)
    assert len(rounds) == n_boats
