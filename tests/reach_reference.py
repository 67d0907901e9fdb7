"""
Reference of one tree asked about many goals (Planner.goal_costs / Planner.retarget, csrc/reach.hpp): a thin wrapper that builds one
connect_reference.Connector per target over ONE tree.

The rule is connect_reference's, with a target's goal state g_t and goal buffer b_t in place of the system's own, for every target
independently: the winner of target t is exactly what
    Connector(system, states, K, pID, edge_len, H, goal=g_t, goal_buffer=b_t).search(goal_tries, incumbent_t, nodes)
returns.  Targets never interact: no key, no early stop and no tie is shared between them.
"""
import numpy as np

import connect_reference as cr

NO_INCUMBENT = cr.NO_INCUMBENT


class Reach(object):
    """A host copy of a tree and the connection rule on it for any number of targets."""

    def __init__(self, system, states, K, pID, edge_len, horizon_iters):
        self.system = system
        self.states = np.array(states, dtype=np.float64)
        self.K = np.array(K, dtype=np.float64)
        self.pID = np.array(pID)
        self.edge_len = np.array(edge_len)
        self.H = int(horizon_iters)

    @property
    def size(self):
        return len(self.states)

    def connector(self, goal=None, goal_buffer=None):
        """The Connector of one target over a fresh copy of the tree (None: the system's own goal / goal buffer)."""
        return cr.Connector(self.system, self.states, self.K, self.pID, self.edge_len, self.H, goal=goal, goal_buffer=goal_buffer)

    def buffers(self, T, goal_buffers=None):
        b = self.system.goal_buffer if goal_buffers is None else goal_buffers
        return np.broadcast_to(np.asarray(b, dtype=np.float64), (T, self.system.nstates))

    def wins(self, goals, goal_buffers=None, goal_tries=8, incumbents=None, nodes=None):
        """Per target the Connector's winner (cost, v, edges), or None."""
        goals = np.asarray(goals, dtype=np.float64).reshape(-1, self.system.nstates)
        bufs = self.buffers(len(goals), goal_buffers)
        incs = [None] * len(goals) if incumbents is None else list(incumbents)
        return [self.connector(goals[t], bufs[t]).search(goal_tries, incs[t], nodes) for t in range(len(goals))]

    def search(self, goals, goal_buffers=None, goal_tries=8, incumbents=None, nodes=None):
        """[(cost, v) or None] per target: what Engine.reach_search returns."""
        return [None if w is None else (w[0], w[1]) for w in self.wins(goals, goal_buffers, goal_tries, incumbents, nodes)]


def from_fixture(system, g, size=None):
    """Reach over the first `size` nodes of a fixture's final tree (None: all of them)."""
    n = len(g["state"]) if size is None else int(size)
    return Reach(system, g["state"][:n], g["K"][:n], g["pID"][:n], g["edge_len"][:n], cr.horizon_of(system, g))


def node_target(g, k):
    """Target "node k": the state of fixture node k as the goal (with the system's goal buffer)."""
    return np.array(g["state"][int(k)], dtype=np.float64)


# The pinned rows: per fixture prefix (name, nodes kept) the targets in the order of one reach_search call, and their winners.
# A target is ("own", scale) -- the system's goal with its goal buffer times `scale` --, ("node", k), or ("far",) -- the system's
# goal with 1e4 added to state 0.
PINNED = {
    ("car_2000", 217): [(("own", 1.0), (951, 211)), (("node", 40), (351, 12)), (("node", 90), (551, 16)), (("node", 150), (551, 16)),
                        (("node", 200), (251, 10)), (("own", 0.25), None), (("far",), None)],
    ("boat_novice_300", 107): [(("own", 1.0), (781, 77)), (("node", 20), (81, 0)), (("node", 50), (401, 41)), (("node", 80), (461, 41)),
                               (("node", 100), (538, 55)), (("own", 0.25), None), (("far",), None)],
    ("boat_novice_lqr_400", 144): [(("own", 1.0), (481, 73)), (("node", 30), (301, 17)), (("node", 70), (21, 0)),
                                   (("node", 110), (341, 17)), (("node", 140), (241, 4)), (("own", 0.25), (549, 132)), (("far",), None)],
}


def pinned_targets(system, g, rows):
    """(goals [T][n], buffers [T][n]) of a PINNED entry."""
    goal = np.asarray(system.goal, dtype=np.float64)
    buf = np.abs(np.asarray(system.goal_buffer, dtype=np.float64))
    goals, bufs = [], []
    for spec, _ in rows:
        if spec[0] == "own":
            goals.append(goal.copy()), bufs.append(buf * spec[1])
        elif spec[0] == "node":
            goals.append(node_target(g, spec[1])), bufs.append(buf.copy())
        else:
            far = goal.copy()
            far[0] += 1e4
            goals.append(far), bufs.append(buf.copy())
    return np.array(goals), np.array(bufs)
