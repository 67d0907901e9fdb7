#!/usr/bin/env python
"""
Replanning that keeps its tree: the loop of examples/tree_chain_gpu.py (the ROS node's `tree_chain`,
demos/lqrrt_ros/nodes/lqrrt_node.py:389-500) with Planner.replan instead of a fresh update_plan per move.

The first move plans from the vehicle's state.  Every later move is seeded with a NODE of the plan being driven -- the first one
reached after the next planning budget has elapsed (`plan_node_after`) -- so the subtree below it, goal hits included, stays on the
device and only has to be re-checked against the map as it is now: edges that a new obstacle cuts are dropped with everything
below them, the rest is the starting tree of the next search.  `planner.retained` says what was kept.

    python examples/replan_gpu.py [moves] [budget_s]
"""
from __future__ import division

import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lqrrt_amd as lqrrt  # noqa: E402


def run(moves=6, basic_duration=0.3, seed=0, verbose=True):
    rng = np.random.RandomState(seed)
    boat = lqrrt.systems.RosBoat("car")
    goal = np.array([60.0, 45.0, 0.0, 0.0, 0.0, 0.0])
    cpm = 2.0
    origin = (-20.0, -20.0)
    grid = np.zeros((int(100 * cpm), int(100 * cpm)), dtype=np.int8)

    def add_blob(cx, cy, r):
        c0, r0 = int(cpm * (cx - origin[0])), int(cpm * (cy - origin[1]))
        k = int(r * cpm)
        grid[max(r0 - k, 0):r0 + k, max(c0 - k, 0):c0 + k] = 100

    for _ in range(12):
        cx, cy = rng.uniform(5, 55), rng.uniform(0, 45)
        if np.hypot(cx - goal[0], cy - goal[1]) > 8 and np.hypot(cx, cy) > 8:
            add_blob(cx, cy, rng.uniform(1.0, 2.5))
    boat.set_occupancy_grid(grid, origin, cpm=cpm, threshold=90)

    constraints = lqrrt.Constraints(nstates=6, ncontrols=3, goal_buffer=boat.goal_buffer, is_feasible=boat.is_feasible)
    planner = lqrrt.Planner(boat.dynamics, boat.lqr, constraints, erf=boat.erf, error_tol=boat.error_tol,
                            min_time=basic_duration, max_time=basic_duration, max_nodes=4E5, goal0=goal,
                            printing=False, **boat.plan_kwargs)

    state = np.zeros(6)
    root, next_runtime = None, basic_duration
    log = []
    for move in range(moves):
        np.random.seed(100 + move)
        t0 = time.time()
        if root is None:
            clean = planner.update_plan(x0=state, sample_space=boat.gen_ss(state, goal), goal_bias=boat.goal_bias,
                                        guide=goal, pruning=True, specific_time=next_runtime)
        else:
            clean = planner.replan(root, sample_space=boat.gen_ss(state, goal), goal_bias=boat.goal_bias,
                                   guide=goal, pruning=True, specific_time=next_runtime)
        took = time.time() - t0
        if not clean:
            raise RuntimeError("the plan update was halted")
        x_seq = np.array(planner.x_seq)
        # chain: the next tree is rooted at the plan node the vehicle reaches first once the next budget has elapsed
        next_runtime = planner.T if planner.T <= basic_duration else 0.75 * planner.T
        next_runtime = float(np.clip(next_runtime, basic_duration, 4 * basic_duration))
        k, root, t_k = planner.plan_node_after(next_runtime)
        if root >= planner._engine.size:                     # (a finish_on_goal node lives on the host: take the one before it)
            k, root = k - 1, planner.node_seq[k - 1]
        state = np.array(planner.tree.state[root])
        kept = planner.retained
        entry = dict(move=move, nodes=planner.tree.size, attempts=planner.stats["attempts"], seconds=took, plan_T=planner.T,
                     reached=bool(planner.plan_reached_goal), start=np.copy(x_seq[0]), retained=kept, next_root=int(root), next_root_time=t_k)
        log.append(entry)
        if verbose:
            print("move %d: %6d nodes / %7d attempts in %.2f s -> plan of %5.1f s, reaches goal: %s; %s" % (
                move, entry["nodes"], entry["attempts"], took, entry["plan_T"], entry["reached"],
                "fresh tree" if kept is None else "kept %(kept)d of %(old_size)d nodes (%(outside)d outside the subtree, %(infeasible)d "
                "edges cut by the new map, %(orphaned)d below them), %(goal_hits)d goal hits kept" % kept))
        # the world changes while we drive: something appears near the path ahead
        ahead = x_seq[min(len(x_seq) - 1, int(0.6 * len(x_seq)))]
        if np.hypot(ahead[0] - goal[0], ahead[1] - goal[1]) > 10:
            add_blob(ahead[0] + rng.uniform(-3, 3), ahead[1] + rng.uniform(-3, 3), 1.0)
            boat.set_occupancy_grid(grid, origin, cpm=cpm, threshold=90)
        if np.all(np.abs(state[:2] - goal[:2]) < np.array(boat.goal_buffer[:2])):
            break
    return log


if __name__ == "__main__":
    run(moves=int(sys.argv[1]) if len(sys.argv) > 1 else 6, basic_duration=float(sys.argv[2]) if len(sys.argv) > 2 else 0.3)
