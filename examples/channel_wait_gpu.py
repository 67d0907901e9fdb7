#!/usr/bin/env python
"""
The channel of examples/fleet_channel_gpu.py narrowed until the lanes overlap: the 6 m x 0.4 m vessels keep only 0.1 m to their
side of the centre line, so two of them cannot pass.  Vessel A runs east for 8 rows and then backs out of the channel into a berth
to the south; vessel B comes west down the whole channel, and vessel C follows B from 7 m further east and stops short of it.

Prioritised planning: every vessel plans against the hulls of the ones before it, as oriented rectangles that move along their
plans (Planner.avoid_rects, DESIGN.md sections 21 and 22).  Leaving now, B meets A head-on and is sent the 29-step way round
(with no way round in its tree it would find nothing).  With max_wait the answer is the one a pilot would give: hold the berth three
ticks -- A is then out of the channel when B gets there -- and take the 21-step channel; C, whose tree holds the channel alone, then
holds three ticks as well, to stay off B's stern.
All delays of a vessel are answered by ONE call on the device.  The loop is plan():

    tracks = []
    for p, extent in zip(planners, extents):
        if tracks:
            p.avoid_rects([t for t, _ in tracks], [e for _, e in tracks], max_wait=max_wait)
        tracks.append((np.asarray(p.x_seq)[:, :3], extent))

The trees are laid out by hand, row by row, as in fleet_channel_gpu.py, so that the geometry can be read off.

    python examples/channel_wait_gpu.py
"""
from __future__ import division

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fleet_channel_gpu import HALF_LENGTH, HALF_WIDTH, hull_points, lay_out, planner_with  # noqa: E402,F401

LANE = 0.1                                                # 0.1 m to each side of the centre line: the 0.4 m hulls overlap
SHORT_STEPS, ROUND_STEPS = 21, 29                         # the root's row and 20 rows of 1 m; the way round
MAX_WAIT = 8
EXTENT = (HALF_LENGTH, HALF_WIDTH)


def vessel_a():
    """East along y = -LANE from x = 0 to x = 8, then out of the channel: south to (8, -4.1), the hull along the berth."""
    east = [(float(x), -LANE, 0.0) for x in range(1, 9)]
    berth = [(8.0, -LANE - float(k), -np.pi / 2) for k in range(1, 5)]
    return (8.0, -LANE - 4.0), lay_out((0.0, -LANE, 0.0), [east + berth])


def vessel_b():
    """West from (20, +LANE) to (0, +LANE): the channel, or north out of it, west along y = 8 and back down on the goal."""
    short = [(20.0 - x, LANE, np.pi) for x in range(1, 21)]
    north = [(20.0, LANE + 0.25 * (8.0 - LANE) * k, np.pi / 2) for k in range(1, 5)]
    west = [(20.0 - x, 8.0, np.pi) for x in range(1, 21)]
    south = [(0.0, 8.0 - 0.25 * (8.0 - LANE - 0.1) * k, -np.pi / 2) for k in range(1, 5)]
    return (0.0, LANE), lay_out((20.0, LANE, np.pi), [short, north + west + south])


def vessel_c():
    """West from (27, +LANE) to (7, +LANE), behind B; its tree holds nothing else."""
    return (7.0, LANE), lay_out((27.0, LANE, np.pi), [[(27.0 - x, LANE, np.pi) for x in range(1, 21)]])


def plan(planners, extents, max_wait):
    """Prioritised planning with waits: each planner against the plans adopted before it.  Returns avoid_rects's answers."""
    tracks, answers = [], []
    for p, extent in zip(planners, extents):
        answers.append(p.avoid_rects([t for t, _ in tracks], [e for _, e in tracks], max_wait=max_wait) if tracks else None)
        tracks.append((np.asarray(p.x_seq, dtype=np.float64)[:, :3], extent))
    return answers


def run(printing=True):
    """The loop without waits, then (on fresh planners) with up to MAX_WAIT rows.  Returns (answers, planners) of both."""
    out = []
    for max_wait in (0, MAX_WAIT):
        planners = [planner_with(*v()) for v in (vessel_a, vessel_b, vessel_c)]
        answers = plan(planners, [EXTENT] * 3, max_wait)
        out.append((answers, planners))
        if printing:
            for name, ans, p in zip("BC", answers[1:], planners[1:]):
                if ans["best_end"] < 0:
                    print("max_wait %d  %s finds no clear plan (%d goal hits); first conflict of its plan at %.1f s"
                          % (max_wait, name, ans["hits"], ans["plan_first"]))
                else:
                    print("max_wait %d  %s holds %d ticks and takes %d steps: T = %.1f s (%s)"
                          % (max_wait, name, p.plan_wait, ans["best_steps"], p.T, "the channel" if ans["best_steps"] == SHORT_STEPS else "the way round"))
    return out


if __name__ == "__main__":
    print("three %.1f m x %.1f m vessels, lanes %.1f m apart" % (2 * HALF_LENGTH, 2 * HALF_WIDTH, 2 * LANE))
    run()
