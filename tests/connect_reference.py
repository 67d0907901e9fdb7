"""
Reference of the tree-wide goal connection (Planner.connect_goal, csrc/connect.hpp), composed from the C oracle's primitives:
refine_reference.Refiner's tree and its one-steer `_edge`.

The rule, exactly as the engine implements it.  The tree has N nodes with pID[v] < v; L_v is the edge length of node v, and
depth[0] = 1, depth[v] = depth[pID[v]] + L_v (the plan's cost prefix of the refinement, extended from the plan to the tree).

  * Candidates.  A candidate is a node v -- every node, or those of a caller's id list.  It starts at v's state and gain, at cost
    depth[v].
  * Chain.  Its targets are the goal, up to `goal_tries` times, one edge per target: the reference's _steer(force_arrive=False)
    (planner.py:354-438) with the fixed horizon, the FPR cut and no hfactor heuristic -- Refiner._edge.  An empty edge adds nothing
    (and, the chain's node and the target being what they were, neither does any later try).  A non-empty edge moves the chain to
    xs[-1] with the gain lqr(xs[-1], us[-1])[1].
  * Validity.  The chain is valid when an edge ends strictly inside the goal box, and ends there; when the tries run out first it
    is invalid.  A candidate that itself lies in the goal box is an ordinary candidate: it needs a non-empty edge like any other.
  * Winner.  The valid candidate of smallest (cost, node id) with cost < incumbent.
  * Early stop.  A chain is abandoned as soon as its running (cost, id) exceeds the best found so far: costs only grow along a
    chain, so the winner depends neither on the order of the candidates nor on that of an id list.
  * Commit.  The winner's non-empty edges become a parent chain of new nodes below v; the plan becomes climb(v) + the new nodes.
"""
import os

import numpy as np

import refine_reference as rr

NO_INCUMBENT = 2 ** 31 - 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class Connector(rr.Refiner):
    """Refiner's host copy of a tree, and the connection rule on it."""

    def depths(self):
        d = [1] * self.size
        for v in range(1, self.size):
            assert 0 <= self.pID[v] < v
            d[v] = d[self.pID[v]] + self.elen[v]
        return d

    def climb(self, v):
        chain = [int(v)]
        while self.pID[chain[-1]] != -1:
            chain.append(self.pID[chain[-1]])
        return chain[::-1]

    def chain(self, v, goal_tries=8, depth=None, stop=None):
        """The goal chain of candidate v: (cost, edges) with edges = [(xs, us, K_end)] when it is valid, else None.  `depth`: v's,
        when the caller has it; `stop`, a (cost, id) pair: the chain is abandoned once its running pair exceeds it."""
        x, K = self.states[v], self.K[v]
        cost = self.depths()[v] if depth is None else int(depth)
        edges = []
        for _ in range(goal_tries):
            ln, xs, us, Ke = self._edge(x, K, self.goal)
            if ln == 0:
                break
            cost += ln
            if stop is not None and (cost, v) > stop:
                return None
            edges.append((xs, us, Ke.copy()))
            x, K = xs[-1], Ke.copy()
            if self.in_goal(x):
                return cost, edges
        return None

    def search(self, goal_tries=8, incumbent=None, nodes=None):
        """The winner (cost, v, edges) over every node (or `nodes`), or None when no valid chain costs less than `incumbent`."""
        inc = NO_INCUMBENT if incumbent is None else int(incumbent)
        depth = self.depths()
        best, win = (inc, -1), None
        for v in (range(self.size) if nodes is None else [int(k) for k in nodes]):
            if (depth[v], v) > best:
                continue
            got = self.chain(v, goal_tries, depth=depth[v], stop=best)
            if got is not None and (got[0], v) < best:
                best, win = (got[0], v), (got[0], v, got[1])
        return win

    def commit_chain(self, win):
        """Appends the winner's edges below its node; returns the new plan and the ids of the new nodes."""
        plan = self.climb(win[1])
        plan, ids = self.commit(plan, (win[0], len(plan) - 1, None, win[2]))
        return plan, ids


def case(name):
    """(system, fixture) of a committed fixture whose final tree is searched (tests/test_refine_gpu.py _case)."""
    import lqrrt_amd
    S = lqrrt_amd.systems
    if name == "ros_boat":
        g = np.load(os.path.join(GOLDEN, "ros_boat.npz"))
        s = S.RosBoat("boat")
        s.set_occupancy_grid(g["grid"], g["origin"], cpm=float(g["cpm"]), threshold=float(g["threshold"]))
        s.goal = [float(v) for v in g["goal"]]
        s.sample_space = [tuple(r) for r in g["sample_space"]]
        return s, g
    path = os.path.join(GOLDEN, "traj_%s.npz" % name)
    if not os.path.exists(path):
        raise AssertionError("fixture missing: tests/golden is committed, a lost fixture must not turn into a pass")
    g = np.load(path)
    if name.startswith("double_integrator"):
        return S.DoubleIntegrator(n_boxes=int(g["n_boxes"]), seed=int(g["box_seed"])), g
    return S.SYSTEMS[name.rsplit("_", 1)[0]](0), g


def horizon_of(system, g):
    kw = system.plan_kwargs
    return int(g["horizon_iters_final"]) if "horizon_iters_final" in g.files else int(kw["horizon"] / kw["dt"])


def first_goal_node(system, g):
    """Index of the first node of the fixture's tree that lies in the goal box (None: none does)."""
    goal = np.asarray(system.goal, dtype=np.float64)
    buf = np.abs(np.asarray(system.goal_buffer, dtype=np.float64))
    inside = np.all((goal - buf < g["state"]) & (g["state"] < goal + buf), axis=1)
    hits = np.flatnonzero(inside)
    return int(hits[0]) if len(hits) else None


def from_fixture(system, g, size=None):
    """Connector over the first `size` nodes of a fixture's final tree (None: all of them)."""
    n = len(g["state"]) if size is None else int(size)
    return Connector(system, g["state"][:n], g["K"][:n], g["pID"][:n], g["edge_len"][:n], horizon_of(system, g))
