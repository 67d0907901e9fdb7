"""
Reference of the plan refinement (Planner.refine_plan, csrc/refine.hpp), composed from the C oracle's primitives.

The rule, exactly as the engine implements it.  The plan is the node sequence p_0 .. p_{P-1} (p_0 the root); L_k is the
edge length of p_k with L_0 = 1, and the plan's step count is C = sum(L_k).

  * Candidate (i, j) for every 0 <= i < j <= P-1 starts at the state and gain of p_i, at cost sum_{k<=i} L_k.
  * Its targets are the states of p_j .. p_{P-2}, then the goal up to `goal_tries` times.
  * One edge per target: the reference's _steer(force_arrive=False) (planner.py:354-438) with a fixed horizon (no hfactor
    heuristic) -- orc_steer_from of a one-node tree holding the chain's current state and gain.
  * An empty edge adds nothing.  A non-empty edge moves the chain to xs[-1] with the gain lqr(xs[-1], us[-1])[1]
    (what tree.add_node stores, planner.py:257).
  * The chain ends after the first edge whose end state lies strictly inside the goal box (planner.py:442-447); a chain
    whose targets run out first is invalid.
  * The winner is the valid candidate of smallest cost, ties to the smaller i, then the smaller j; it is accepted only if
    its cost is below C.  Its non-empty edges become a chain of new nodes below p_i, and the plan becomes
    p_0 .. p_i + the new nodes.

Candidates are visited in (i, j) order and a chain is abandoned as soon as its running cost reaches the best cost found so
far (or C): costs only grow along a chain and a later candidate loses every tie, so this never changes the winner.
"""
import numpy as np

import coracle


class Refiner(object):
    """A host copy of a tree (states, gains, parents, edge lengths, and the edges of the nodes it appends) and the
    refinement rule on it.  `system` is an lqrrt_amd.systems object; `horizon_iters` the fixed steer horizon."""

    def __init__(self, system, states, K, pID, edge_len, horizon_iters, goal=None, goal_buffer=None):
        kw = system.plan_kwargs
        n, m = system.nstates, system.ncontrols
        self.n, self.m = n, m
        self.H = int(horizon_iters)
        self.o = coracle.COracle(system, 4)
        goal = np.asarray(system.goal if goal is None else goal, dtype=np.float64)
        self.goal = goal
        buf = np.abs(np.asarray(system.goal_buffer if goal_buffer is None else goal_buffer, dtype=np.float64))
        self.lo, self.hi = goal - buf, goal + buf
        self.o.configure(kw["dt"], kw["FPR"], self.H, system.error_tol, goal, buf, np.zeros((n, 2)), np.zeros(n))
        self.o.reset(np.zeros(n))
        self.states = [np.array(s, dtype=np.float64) for s in states]
        self.K = [np.array(k, dtype=np.float64).reshape(m, n) for k in K]
        self.pID = [int(p) for p in pID]
        self.elen = [int(v) for v in edge_len]
        self.elen[0] = 1
        self.edges = {}                              # appended node -> (xs, us)

    @property
    def size(self):
        return len(self.states)

    def in_goal(self, x):
        return bool(np.all((self.lo < x) & (x < self.hi)))

    def _edge(self, x, K, target):
        """one steer from (x, K) toward target: (len, xs, us, K at the end)"""
        self.o.load_tree(x[None, :], K[None, :, :], np.array([-1], dtype=np.int32))
        return self.o.steer_from(0, target)

    def cost(self, plan):
        return int(sum(self.elen[p] if k > 0 else 1 for k, p in enumerate(plan)))

    def round(self, plan, goal_tries=8, incumbent=None):
        """The winner of one round on `plan` (node ids): (cost, i, j, edges) with edges = [(xs, us, K_end)], or None when no
        candidate beats the plan's own cost (or `incumbent` steps, when given)."""
        P = len(plan)
        L = [1] + [self.elen[p] for p in plan[1:]]
        prefix = np.cumsum(L)
        C = int(prefix[-1])
        best = None
        best_cost = C if incumbent is None else int(incumbent)
        targets = [self.states[p] for p in plan[:-1]]
        for i in range(P - 1):
            if prefix[i] >= best_cost:
                break
            for j in range(i + 1, P):
                x, K = self.states[plan[i]], self.K[plan[i]]
                cost = int(prefix[i])
                edges = []
                done = False
                for t in range(j, P - 1 + goal_tries):
                    tgt = targets[t] if t < P - 1 else self.goal
                    ln, xs, us, Ke = self._edge(x, K, tgt)
                    if ln == 0:
                        continue
                    cost += ln
                    if cost >= best_cost:
                        break
                    edges.append((xs, us, Ke.copy()))
                    x, K = xs[-1], Ke.copy()
                    if self.in_goal(x):
                        done = True
                        break
                if done and cost < best_cost:
                    best_cost, best = cost, (cost, i, j, edges)
        return best

    def commit(self, plan, win):
        """Appends the winner's edges below p_i; returns the new plan and the ids of the new nodes."""
        _, i, _, edges = win
        parent = plan[i]
        ids = []
        for xs, us, Ke in edges:
            nid = self.size
            self.states.append(np.array(xs[-1]))
            self.K.append(Ke)
            self.pID.append(parent)
            self.elen.append(len(xs))
            self.edges[nid] = (xs, us)
            ids.append(nid)
            parent = nid
        return list(plan[:i + 1]) + ids, ids

    def refine(self, plan, max_rounds=8, goal_tries=8, capacity=None):
        """Rounds until no improvement, max_rounds, or (capacity) the tree cannot hold the next chain.
        Returns (plan, [(cost, i, j, new ids)] per accepted round)."""
        plan = list(plan)
        log = []
        for _ in range(max_rounds):
            win = self.round(plan, goal_tries)
            if win is None:
                break
            if capacity is not None and self.size + len(win[3]) > capacity:
                break
            plan, ids = self.commit(plan, win)
            log.append((win[0], win[1], win[2], ids))
        return plan, log


def from_fixture(system, g, horizon_iters=None, goal_buffer=None):
    """Refiner over a traj_* / ros_* fixture's final tree, and the fixture's plan."""
    H = horizon_iters
    if H is None:
        kw = system.plan_kwargs
        H = int(g["horizon_iters_final"]) if "horizon_iters_final" in g.files else int(kw["horizon"] / kw["dt"])
    r = Refiner(system, g["state"], g["K"], g["pID"], g["edge_len"], H, goal_buffer=goal_buffer)
    return r, [int(v) for v in g["node_seq"]]
