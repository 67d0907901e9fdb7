"""
Reference of the device node table (lqrrt_amd.engine.NodeTable, csrc/generic.hpp) in plain NumPy.

The table of a tree whose plugins are host callables: node states, parents and an ignore set, and the nearest selection of
planner.py:239-247 over the costs-to-go of planner.py:340-350.  The rule, exactly as the engine implements it:

  1. e[i] = x - state[i]; for an angular state d the difference is wrapped,
     e[i][d] = arctan2(sin x_d cos v_d - cos x_d sin v_d, cos x_d cos v_d + sin x_d sin v_d)  (demo_car.py:115-126).
  2. cost[i] = np.sum(np.tensordot(e, S, axes=1) * e, axis=1)[i], S = identity when none is given.
  3. nearest = np.argmin over the nodes that are not ignored (lowest id among equal costs: the stable order of planner.py:240);
     with `use_ignore` off, or with every node ignored, over all nodes (planner.py:241,245,247).
  4. reset(x0): one node, parent -1, nothing ignored.  append(parent, x): a new node, not ignored.  load(states, pID, ignored):
     the table is replaced, flags included.  truncate(size): nodes size.. go, and their flags with them; kept flags stay.
"""
import numpy as np


class NodeTableModel(object):
    def __init__(self, nstates, angle_dims=()):
        self.n = int(nstates)
        self.angle_dims = tuple(int(d) for d in angle_dims)
        self.state = np.zeros((0, self.n))
        self.pID = np.zeros(0, dtype=np.int32)
        self.ign = np.zeros(0, dtype=bool)

    @property
    def size(self):
        return len(self.state)

    def reset(self, x0):
        self.state = np.array(x0, dtype=np.float64).reshape(1, self.n)
        self.pID = np.array([-1], dtype=np.int32)
        self.ign = np.zeros(1, dtype=bool)

    def append(self, parent, state):
        if not 0 <= int(parent) < self.size:
            raise ValueError("The given parent ID, {}, doesn't exist.".format(parent))
        self.state = np.vstack((self.state, np.asarray(state, dtype=np.float64).reshape(1, self.n)))
        self.pID = np.append(self.pID, np.int32(parent))
        self.ign = np.append(self.ign, False)

    def load(self, states, pID, ignored=None):
        self.state = np.array(states, dtype=np.float64).reshape(-1, self.n)
        self.pID = np.array(pID, dtype=np.int32)
        self.ign = np.zeros(len(self.state), dtype=bool) if ignored is None else np.array(ignored, dtype=bool)

    def ignore(self, ids):
        for i in ids:
            if not 0 <= int(i) < self.size:
                raise ValueError("node {} does not exist".format(i))
            self.ign[int(i)] = True

    def ignored(self):
        return self.ign.copy()

    def truncate(self, size):
        if not 1 <= int(size) <= self.size:
            raise ValueError("cannot truncate a tree of {} nodes to {}".format(self.size, size))
        self.state, self.pID, self.ign = self.state[:size], self.pID[:size], self.ign[:size]

    def errors(self, x):
        x = np.asarray(x, dtype=np.float64)
        v = self.state
        e = x - v
        for d in self.angle_dims:
            e[:, d] = np.arctan2(np.sin(x[d]) * np.cos(v[:, d]) - np.cos(x[d]) * np.sin(v[:, d]),
                                 np.cos(x[d]) * np.cos(v[:, d]) + np.sin(x[d]) * np.sin(v[:, d]))
        return e

    def costs_of_errors(self, e, S=None):
        e = np.ascontiguousarray(e, dtype=np.float64)
        S = np.eye(self.n) if S is None else np.asarray(S, dtype=np.float64)
        return np.sum(np.tensordot(e, S, axes=1) * e, axis=1)

    def costs(self, x, S=None):
        return self.costs_of_errors(self.errors(x), S)

    def select(self, costs, use_ignore=True):
        """(id, cost) of the nearest eligible node for a given cost vector."""
        if use_ignore and not np.all(self.ign):
            ok = np.flatnonzero(~self.ign)
            i = int(ok[np.argmin(costs[ok])])
        else:
            i = int(np.argmin(costs))
        return i, float(costs[i])

    def nearest(self, x, S=None, use_ignore=True):
        return self.select(self.costs(x, S), use_ignore)
