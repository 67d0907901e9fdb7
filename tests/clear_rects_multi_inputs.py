"""
The inputs that tests/test_clear_rects_multi_gpu.py hands to the rectangle clearance calls for several trees
(Engine.tree_clear_rects_multi / tree_clear_rects_wait_multi), built once here and shared with tests/test_clear_rects_multi_cpu.py,
which shows with the NumPy references alone (tests/clear_rects_reference.py, tests/clear_rects_wait_reference.py) that none of them
is degenerate.  Nothing here needs a device.
"""
import functools

import numpy as np

import clear_reference as cl
import clear_rects_reference as cr
import clear_rects_wait_reference as rw

FORK = "fork, the rectangle crosses the short branch"
CHUNK_SIZES = (1, 32, 33)                                            # one member, a full chunk, a chunk and one more


def starts(n):
    return [(5 * k) % 23 for k in range(n)]


def waits(n):
    return [1 + (3 * k) % 9 for k in range(n)]


@functools.lru_cache(maxsize=None)
def one_node_cases():
    """The tree that is its root alone, with the square on the root and with it far away."""
    tree = cl.case("N=1, a disc on the root").tree
    return (cr.Case("N = 1, the square on the root", tree, cr.with_heading(cl.parked(3, 0.0, 0.0), 0.0), cr.SQUARE, none=True),
            cr.Case("N = 1, the square far away", tree, cr.with_heading(cl.parked(3, 50.0, 50.0), 0.0), cr.SQUARE, none=True))


@functools.lru_cache(maxsize=None)
def plain_cases():
    """Every hand-built case of the plain call and the one-node trees: they stand next to the chain of 256 and the 257-node spine."""
    return tuple(cr.cases()) + one_node_cases()


@functools.lru_cache(maxsize=None)
def wait_cases():
    """Every hand-built case of the wait call, and one W = 1 member next to W = 2 .. 64."""
    return tuple(rw.cases()) + (rw.WaitCase(cr.case(FORK), 1),)


def by_model(cases, system_of):
    groups = {}
    for c in cases:
        groups.setdefault(system_of(c), []).append(c)
    return groups


@functools.lru_cache(maxsize=None)
def fork_reference(start):
    c = cr.case(FORK)
    t = c.tree
    lo, hi = t.box()
    return cr.clear_rects(t.state, t.pID, t.elen, t.xedge, c.test(), c.tracks, c.extents, start, lo, hi)


@functools.lru_cache(maxsize=None)
def fork_wait_reference(start, W, moved=False):
    c = cr.case(FORK)
    t = c.tree
    lo, hi = t.box()
    return rw.clear_rects_wait(t.state, t.pID, t.elen, t.xedge, c.test(), moved_tracks() if moved else c.tracks, c.extents, start, W, lo, hi)


@functools.lru_cache(maxsize=None)
def moved_tracks():
    """The fork's tracks with the crossing square elsewhere at the instant it met the short branch."""
    other = cr.case(FORK).tracks.copy()
    other[7, -1, :2] = (7.0, 40.0)
    return other


@functools.lru_cache(maxsize=None)
def moved_reference(start):
    c = cr.case(FORK)
    t = c.tree
    lo, hi = t.box()
    return cr.clear_rects(t.state, t.pID, t.elen, t.xedge, c.test(), moved_tracks(), c.extents, start, lo, hi)


SHARE_STARTS = (0, 4, 0, 1, 0)                                       # of the five members of the table-sharing test
