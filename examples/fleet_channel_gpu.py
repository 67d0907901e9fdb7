#!/usr/bin/env python
"""
Two 6 m x 0.4 m vessels meet in a channel.  Vessel A runs east along y = -0.6, vessel B west along y = +0.6: their hulls pass
0.8 m apart.  B's tree also holds a long way round, out to y = 8 and back.

lqrrt_amd.deconflict makes every earlier planner an obstacle that moves along its plan.  As a DISC, a 6 m x 0.4 m hull needs a
radius of 3.007 m: A's disc sweeps the whole channel, B's short plan is in conflict and B is sent the long way round.  As an
oriented RECTANGLE (extents=(3.0, 0.2): Planner.avoid_rects) A covers y -0.8 .. -0.4 only, and B keeps the
short plan that is geometrically free.

The two trees are laid out by hand, row by row, and put on the planners' engines with Engine.tree_load, so that the geometry can be
read off and the outcome does not depend on a sample stream; deconflict, avoid and avoid_rects see them as they see grown trees.

    python examples/fleet_channel_gpu.py
"""
from __future__ import division

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lqrrt_amd as lqrrt  # noqa: E402
from lqrrt_amd.tree import Tree  # noqa: E402

HALF_LENGTH, HALF_WIDTH = 3.0, 0.2
COVERING = float(np.hypot(HALF_LENGTH, HALF_WIDTH))       # the smallest disc that holds the hull
DT, H = 0.1, 5                                            # an edge holds up to 5 rows
LANE = 0.6
SHORT_STEPS = 21                                          # B's short plan: the root's row and 20 rows of 1 m


def hull_points():
    """Body-frame points on the 6 m x 0.4 m hull, every 0.25 m along it: (2, 75)."""
    bx, by = np.meshgrid(np.linspace(-HALF_LENGTH, HALF_LENGTH, 25), np.array([-HALF_WIDTH, 0.0, HALF_WIDTH]))
    return np.vstack((bx.ravel(), by.ravel()))


def lay_out(root, branches):
    """root: one pose (x, y, heading); branches: lists of poses that each leave the root, cut into edges of up to H rows, one node
    per edge.  Returns (pID, rows per node)."""
    pID, rows = [-1], [[root]]
    for poses in branches:
        at = 0
        for chunk in (poses[k:k + H] for k in range(0, len(poses), H)):
            pID.append(at)
            rows.append(chunk)
            at = len(pID) - 1
    return pID, rows


def vessel_a():
    """East along y = -LANE, 1 m per row, from x = 0 to x = 20."""
    return (20.0, -LANE), lay_out((0.0, -LANE, 0.0), [[(float(x), -LANE, 0.0) for x in range(1, 21)]])


def vessel_b():
    """West from (20, +LANE).  The short branch runs along y = +LANE; the long one leaves the channel northward, runs west along
    y = 8 and comes back down on the goal."""
    short = [(20.0 - x, LANE, np.pi) for x in range(1, 21)]
    north = [(20.0, LANE + 0.25 * (8.0 - LANE) * k, np.pi / 2) for k in range(1, 5)]
    west = [(20.0 - x, 8.0, np.pi) for x in range(1, 21)]
    south = [(0.0, 8.0 - 0.25 * (8.0 - LANE - 0.1) * k, -np.pi / 2) for k in range(1, 5)]
    return (0.0, LANE), lay_out((20.0, LANE, np.pi), [short, north + west + south])


def planner_with(goal_xy, layout):
    """A planner of a BoatIntermediate with the 6 m x 0.4 m hull and no static obstacle that holds the hand-laid tree on its engine
    and, as its plan, the tree's shortest goal hit -- the state update_plan leaves behind."""
    pID, rows = layout
    boat = lqrrt.systems.BoatIntermediate(0)
    boat.vps = hull_points()
    boat.set_obstacles(np.zeros((0, 3)))
    n, m = boat.nstates, boat.ncontrols
    boat.goal = [goal_xy[0], goal_xy[1]] + [0.0] * (n - 2)
    boat.goal_buffer = [0.5, 0.5] + [np.inf] * (n - 2)
    constraints = lqrrt.Constraints(nstates=n, ncontrols=m, goal_buffer=boat.goal_buffer, is_feasible=boat.is_feasible)
    p = lqrrt.Planner(boat.dynamics, boat.lqr, constraints, horizon=H * DT, dt=DT, FPR=0, error_tol=boat.error_tol, erf=boat.erf,
                      max_nodes=64, goal0=boat.goal, sys_time=lambda: 0.0, printing=False, wave_size=64)
    N = len(pID)
    elen = np.array([len(r) for r in rows], dtype=np.int32)
    x_cat = np.zeros((int(elen.sum()), n))
    x_cat[:, :3] = np.concatenate([np.asarray(r, dtype=np.float64).reshape(-1, 3) for r in rows])
    state = x_cat[np.cumsum(elen) - 1]
    eng = p._get_engine()
    p._engine_resolution(eng)
    eng.tree_load(state, np.zeros((N, m, n)), np.array(pID, dtype=np.int32), elen, x_cat, np.zeros((len(x_cat), m)))
    S0 = p.system.Smatrix()
    p.tree = Tree(state[0], (S0, np.zeros((m, n))))
    p.tree._bind(eng, S0)
    p._grown_with, p._grown_goal = p._tree_resolution(), np.array(p.goal, dtype=np.float64)
    lo, hi = np.asarray(boat.goal) - np.asarray(boat.goal_buffer), np.asarray(boat.goal) + np.asarray(boat.goal_buffer)
    hits = [i for i in range(1, N) if np.all((lo < state[i]) & (state[i] < hi))]
    cum = np.zeros(N, dtype=np.int64)
    for i in range(N):
        cum[i] = elen[i] + (cum[pID[i]] if i else 0)
    p._adopt_plan(min(hits, key=lambda i: (cum[i], i)))
    p.plan_reached_goal = True
    p._prepare_interpolators()
    return p


def run(printing=True):
    """deconflict of [A, B] with covering discs, then (on fresh planners) with rectangles.  Returns B's two answers."""
    answers = []
    for kind in ("discs", "rectangles"):
        a, b = planner_with(*vessel_a()), planner_with(*vessel_b())
        assert len(b.x_seq) == SHORT_STEPS
        if kind == "discs":
            res = lqrrt.deconflict([a, b], COVERING)
        else:
            res = lqrrt.deconflict([a, b], None, extents=(HALF_LENGTH, HALF_WIDTH))
        out = res[1]
        answers.append(out)
        if printing:
            if out["best_end"] < 0:
                print("%-10s B finds no clear plan (%d of %d goal hits clear); first conflict of its plan at %.1f s"
                      % (kind, out["clear_hits"], out["hits"], out["plan_first"]))
            else:
                print("%-10s B takes the plan that ends at node %d: %d steps, T = %.1f s (%s)"
                      % (kind, out["best_end"], out["best_steps"], b.T, "the short one" if out["best_steps"] == SHORT_STEPS else "the long way round"))
    return answers


if __name__ == "__main__":
    print("two %.1f m x %.1f m vessels, lanes %.1f m apart; covering disc radius %.3f m" % (2 * HALF_LENGTH, 2 * HALF_WIDTH, 2 * LANE, COVERING))
    run()
