#!/usr/bin/env python
"""
A fleet in the narrowed channel of examples/channel_wait_gpu.py checks its plans every tick against TRACKED traffic: the hull of
vessel A, a 6 m x 0.4 m rectangle that runs east down the channel for 8 rows and then backs out of it into a berth to the south.
A is not planned here; its track (x, y, heading per instant) is what a tracker would hand over, one table for the whole fleet.

Three vessels want to come west through the channel: B down the whole of it (its tree also holds a 29-step way round), C from 7 m
further east, D from 4 m further east still.  Each tick every vessel asks "which plan of my tree stays clear of that hull, and if I
held my berth for up to MAX_WAIT ticks?" -- Planner.avoid_rects with max_wait.  For a fleet that is one loop of solo calls,

    for p in fleet:
        p.avoid_rects(traffic, EXTENT, start=tick, max_wait=MAX_WAIT)

or ONE call that shares the device work (lqrrt_amd.avoids_rects): the table is built and uploaded once, and
every stage of the query is one launch over all the trees,

    lqrrt.avoids_rects(fleet, traffic, EXTENT, start=tick, max_wait=MAX_WAIT)

Both are run here, on twin fleets, and must give the same dicts and leave the same plans.  As the ticks pass A gets out of the way,
and the wait that B's answer asks for shrinks from three ticks to none; C and D, further east, reach A's stretch after it has left
and never wait.

    python examples/fleet_channel_avoid_gpu.py
"""
from __future__ import division

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lqrrt_amd as lqrrt  # noqa: E402
from fleet_channel_gpu import lay_out, planner_with  # noqa: E402
from channel_wait_gpu import EXTENT, LANE, MAX_WAIT, SHORT_STEPS, vessel_a, vessel_b, vessel_c  # noqa: E402

TICKS = 4


def vessel_d():
    """West from (31, +LANE) to (11, +LANE), behind C; its tree holds the channel alone."""
    return (11.0, LANE), lay_out((31.0, LANE, np.pi), [[(31.0 - x, LANE, np.pi) for x in range(1, 21)]])


def traffic():
    """Vessel A's hull as a tracker reports it: (L, 1, 3), its pose at consecutive instants; it stays in its berth afterwards."""
    a = planner_with(*vessel_a())
    return np.ascontiguousarray(np.asarray(a.x_seq, dtype=np.float64)[:, None, :3])


def fleet():
    return [planner_with(*v()) for v in (vessel_b, vessel_c, vessel_d)]


def run(printing=True):
    """TICKS ticks of the batched call on one fleet and of the loop on its twin.  Returns the batched answers per tick."""
    tracks = traffic()
    batched, looped = fleet(), fleet()
    answers = []
    for tick in range(TICKS):
        got = lqrrt.avoids_rects(batched, tracks, EXTENT, start=tick, max_wait=MAX_WAIT)
        want = [p.avoid_rects(tracks, EXTENT, start=tick, max_wait=MAX_WAIT) for p in looped]
        assert got == want, (tick, got, want)
        for p, q in zip(batched, looped):
            assert list(p.node_seq) == list(q.node_seq) and p.plan_wait == q.plan_wait and p.T == q.T
            assert np.array_equal(np.asarray(p.x_seq), np.asarray(q.x_seq))
        answers.append(got)
        if printing:
            print("tick %d  " % tick + "   ".join(
                "%s holds %d, %d steps (%s)" % (name, p.plan_wait, g["best_steps"], "channel" if g["best_steps"] == SHORT_STEPS else "round")
                for name, p, g in zip("BCD", batched, got)))
    return answers


if __name__ == "__main__":
    print("three vessels against one tracked %.1f m x %.1f m hull, up to %d ticks of waiting" % (2 * EXTENT[0], 2 * EXTENT[1], MAX_WAIT))
    run()
