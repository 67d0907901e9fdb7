"""
Reference of the tree-wide goal chains through waypoints (Planner.connect_via, csrc/connect_via.hpp), composed from
connect_reference.Connector -- that is from refine_reference.Refiner._edge (the C oracle's one steer), depths, climb and commit.

The rule, exactly as the engine implements it.  The tree has N nodes with pID[v] < v and connect_reference's depth table.  The
waypoints are w_0 .. w_{Q-1}, Q >= 0, each a state of n doubles; a waypoint need be neither a tree node nor a feasible state.

  * Candidates.  A candidate is a pair (v, j), 0 <= j <= Q: v every node, or those of a caller's id list.  It starts at v's state
    and gain, at cost depth[v].
  * Chain.  Its targets are w_j .. w_{Q-1} in order, one edge each, then the goal up to `goal_tries` times: Refiner._edge, the
    reference's _steer(force_arrive=False) with the fixed horizon, the FPR cut and no hfactor heuristic.  An empty edge adds nothing
    and the chain goes on to its next target.  A non-empty edge moves the chain to xs[-1] with the gain lqr(xs[-1], us[-1])[1].
  * Validity.  After every non-empty edge, a waypoint's included, the chain ends valid if its end lies strictly inside the goal
    box; when the targets run out first it is invalid.  j = Q is exactly connect_reference's candidate.
  * Winner.  The valid candidate of smallest (cost, v, j) with cost < incumbent.
  * Early stop.  A chain is abandoned once its running (cost, v, j) exceeds the best found so far: costs only grow along a chain,
    so the winner depends neither on the order of the candidates nor on that of an id list.
  * Commit.  The winner's non-empty edges become a parent chain of new nodes below v; the plan becomes climb(v) + the new nodes.
"""
import numpy as np

import connect_reference as cr

NO_INCUMBENT = cr.NO_INCUMBENT


class ViaConnector(cr.Connector):
    """Connector's host copy of a tree, and the waypoint rule on it."""

    def chain_via(self, v, j, waypoints, goal_tries=8, depth=None, stop=None):
        """The chain of candidate (v, j): (cost, edges) with edges = [(xs, us, K_end)] when it is valid, else None.  `stop`, a
        (cost, v, j) triple: the chain is abandoned once its running triple exceeds it."""
        x, K = self.states[v], self.K[v]
        cost = self.depths()[v] if depth is None else int(depth)
        targets = [np.asarray(w, dtype=np.float64) for w in waypoints[j:]] + [self.goal] * int(goal_tries)
        edges = []
        for tgt in targets:
            ln, xs, us, Ke = self._edge(x, K, tgt)
            if ln == 0:
                continue
            cost += ln
            if stop is not None and (cost, v, j) > stop:
                return None
            edges.append((xs, us, Ke.copy()))
            x, K = xs[-1], Ke.copy()
            if self.in_goal(x):
                return cost, edges
        return None

    def search_via(self, waypoints, goal_tries=8, incumbent=None, nodes=None):
        """The winner (cost, v, j, edges) over every node (or `nodes`) and every j, or None when no valid chain costs less than
        `incumbent`."""
        way = np.asarray(waypoints, dtype=np.float64).reshape(-1, self.n)
        Q = len(way)
        inc = NO_INCUMBENT if incumbent is None else int(incumbent)
        depth = self.depths()
        best, win = (inc, -1, -1), None
        for v in (range(self.size) if nodes is None else [int(k) for k in nodes]):
            for j in range(Q + 1):
                if (depth[v], v, j) > best:
                    continue
                got = self.chain_via(v, j, way, goal_tries, depth=depth[v], stop=best)
                if got is not None and (got[0], v, j) < best:
                    best, win = (got[0], v, j), (got[0], v, j, got[1])
        return win

    def commit_via(self, win):
        """Appends the winner's edges below its node; returns the new plan and the ids of the new nodes."""
        plan = self.climb(win[1])
        return self.commit(plan, (win[0], len(plan) - 1, None, win[3]))


def from_fixture(system, g, size=None):
    """ViaConnector over the first `size` nodes of a fixture's final tree (None: all of them)."""
    n = len(g["state"]) if size is None else int(size)
    return ViaConnector(system, g["state"][:n], g["K"][:n], g["pID"][:n], g["edge_len"][:n], cr.horizon_of(system, g))


def plan_states(g, from_node):
    """The states of the fixture plan's nodes with id >= from_node, in plan order: the part of the plan a tree cut at `from_node`
    nodes no longer holds."""
    ids = [int(v) for v in g["node_seq"] if int(v) >= int(from_node)]
    return ids, np.array([g["state"][v] for v in ids], dtype=np.float64).reshape(-1, g["state"].shape[1])


# Fixture trees cut off early, the waypoints the fixture plan's nodes beyond the cut: name, nodes kept, the plan nodes that serve as
# waypoints (None: every plan node >= the cut; their number is checked), goal tries, winner of connect_goal's rule (cost, v) or None,
# winner of the waypoint rule (cost, v, j), lengths of the winner's edges.  A reference that drifts, or inputs that stop exercising
# the rule, fail here instead of passing vacuously.
ROWS = [("car_500", 217, [217], 1, None, (1050, 213, 0), [49, 50]),
        ("car_500", 217, [217], 8, (951, 211), (951, 211, 1), [50, 50]),                       # j = Q wins: connect_goal's candidate
        ("car_500", 108, [208, 209, 211, 212, 213, 214, 215, 217], 1, None, (992, 63, 0), [41] + [50] * 6),
        ("car_500", 108, [208, 209, 211, 212, 213, 214, 215, 217], 8, None, (992, 63, 0), [41] + [50] * 6),
        ("boat_novice_300", 107, 16, 1, (821, 106), (679, 55, 5), [20] * 8 + [6, 12, 20, 20]),
        ("boat_novice_300", 107, 16, 8, (781, 77), (679, 55, 5), [20] * 8 + [6, 12, 20, 20]),
        ("boat_novice_300", 53, 32, 1, None, (698, 41, 16), 17),                               # two edges cut short: 1 and 16 steps
        ("boat_novice_300", 53, 32, 8, None, (698, 41, 16), 17)]


def row_inputs(name, size, way_ids):
    """(system, fixture, reference, waypoints) of a row of ROWS."""
    s, g = cr.case(name)
    ids, way = plan_states(g, size)
    if isinstance(way_ids, int):
        assert len(ids) == way_ids and ids[-1] == int(g["node_seq"][-1])
    else:
        assert ids == way_ids
    return s, g, from_fixture(s, g, size), way
