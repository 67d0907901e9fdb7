#!/usr/bin/env python
"""
Plan, then shorten the plan on the GPU (Planner.refine_plan).  The reference keeps the tree path of its
first goal hit, which zig-zags; refine_plan searches every shortcut of that path in one kernel launch per round.

    python examples/refine_plan_gpu.py
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
                        min_time=0, max_time=5, max_nodes=3000, goal0=car.goal, printing=False, wave_size=256)

planner.update_plan(car.x0, car.sample_space, goal_bias=car.goal_bias)
print("found: %d nodes on the plan, T = %.1f s (tree of %d nodes)" % (len(planner.node_seq), planner.T, planner.tree.size))

t0 = time.perf_counter()
rounds = planner.refine_plan(max_rounds=8, goal_tries=8)
print("refined in %.1f ms, %d round(s): %d nodes on the plan, T = %.1f s" % (
    1e3 * (time.perf_counter() - t0), rounds, len(planner.node_seq), planner.T))
# get_state / get_effort now follow the shorter plan
print("state at t = T/2:", np.round(planner.get_state(planner.T / 2), 3))
