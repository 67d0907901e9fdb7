"""
A plain sequential reference for ANY list of samples, and the census of one wave of them (CPU only).

`Replay` restates the loop of planner.py:233-290 in Python over the sequential C oracle's SINGLE-DECISION primitives --
COracle.nearest_prefix, steer_from, load_tree, costs_prefix -- and never calls orc_extend: for each sample the nearest node of
the current tree (under the ignore set when pruning), the steer from it, the append of end state / end gain / parent / length
when the edge has rows, the strict goal box on the end state, and on a hit the root path into the ignore set and the best plan
(steps < best_steps).  After every append the oracle's tree is loaded again, so the next decision sees it.
tests/test_wave_cpu.py shows that it reproduces orc_extend on the oracle's own traced samples bit for bit.

`census` runs one wave of samples on the replay's current tree and says, from the reference alone, what an exact-mode wave of
the engine has to report for it: the committed prefix C under max_commit / node_limit / the first goal hit, the accepted count,
the hits, the chain depth of every sample (deepest + 1 = lqrrt_extend_stats.chain_slots), which samples are rejected, which
would hit the goal when steered from their SNAPSHOT nearest (a second oracle that keeps the wave-start tree) and which do so
sequentially, and the exact cost ties at the minimum.  The replay itself is left where it was.
"""
import numpy as np

import coracle


def configure(o, system, horizon=None):
    """coracle.make's configuration for an oracle built by hand (resolution, goal box, sampler)."""
    kw = system.plan_kwargs
    horizon = kw["horizon"] if horizon is None else horizon
    o.configure(kw["dt"], kw["FPR"], int(horizon / kw["dt"]), system.error_tol, system.goal, system.goal_buffer,
                system.sample_space, system.goal_bias, 10)


class Replay(object):
    """The sequential planner over explicit samples.  `root`: the tree's first node (default: the system's x0)."""

    def __init__(self, system, capacity, root=None, pruning=True):
        self.system, self.pruning = system, bool(pruning)
        self.n, self.m = system.nstates, system.ncontrols
        self.capacity = int(capacity)
        self.o = coracle.COracle(system, self.capacity + 8)
        self.o0 = coracle.COracle(system, self.capacity + 8)          # keeps a wave-start tree (census)
        for o in (self.o, self.o0):
            configure(o, system)
        root = np.array(system.x0 if root is None else root, dtype=np.float64)
        self.o.reset(root)
        self.o0.reset(root)
        g = np.asarray(system.goal, dtype=np.float64)
        b = np.abs(np.asarray(system.goal_buffer, dtype=np.float64))
        self.glo, self.ghi = g - b, g + b                             # as COracle.configure makes the box
        self.states = [self.o.states()[0]]
        self.K = [self.o.gains()[0]]
        self.pid, self.elen, self.ign = [-1], [1], [False]
        self.edges = [(root.reshape(1, -1).copy(), np.zeros((1, self.m)))]
        self.hits, self.best_end, self.best_steps = 0, -1, -1
        self.iterations = 0
        self.near, self.lens = [], []                                 # per iteration: nearest id, recorded rows

    # ------------------------------------------------------------------ the tree as arrays
    @property
    def size(self):
        return len(self.pid)

    def parents(self):
        return np.array(self.pid, dtype=np.int32)

    def edge_lengths(self):
        return np.array(self.elen, dtype=np.int32)

    def ignored(self):
        return np.array(self.ign, dtype=bool)

    def node_states(self):
        return np.array(self.states)

    def gains(self):
        return np.array(self.K)

    def best(self):
        return self.best_end, self.best_steps

    def _load(self, o):
        o.load_tree(np.array(self.states), np.array(self.K), self.parents(), np.array(self.ign, dtype=np.uint8))

    # ------------------------------------------------------------------ one iteration of planner.py:233-290
    def in_goal(self, x):
        return bool(np.all((self.glo < x) & (x < self.ghi)))

    def step(self, x):
        """One sample: (nearest id, rows, hit)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        near = self.o.nearest_prefix(x, self.size, self.pruning)
        ln, xs, us, K = self.o.steer_from(near, x)
        self.iterations += 1
        self.near.append(near)
        self.lens.append(ln)
        hit = False
        if ln > 0:
            ID = self.size
            self.states.append(xs[-1].copy())
            self.K.append(K.copy())
            self.pid.append(near)
            self.elen.append(ln)
            self.ign.append(False)
            self.edges.append((xs, us))
            if self.in_goal(xs[-1]):
                hit = True
                steps, v = 0, ID
                while v != -1:
                    steps += self.elen[v]
                    if self.pruning:
                        self.ign[v] = True
                    v = self.pid[v]
                self.hits += 1
                if self.best_end < 0 or steps < self.best_steps:
                    self.best_end, self.best_steps = ID, steps
            self._load(self.o)
        return near, ln, hit

    def run(self, xs):
        return [self.step(x) for x in xs]

    # ------------------------------------------------------------------ going back (census)
    def mark(self):
        return (self.size, list(self.ign), self.hits, self.best_end, self.best_steps, self.iterations)

    def rewind(self, mk):
        size, ign, self.hits, self.best_end, self.best_steps, self.iterations = mk
        for a in (self.states, self.K, self.pid, self.elen, self.edges):
            del a[size:]
        self.ign = list(ign)
        del self.near[self.iterations:]
        del self.lens[self.iterations:]
        self._load(self.o)


class Census(object):
    """What `census` found; the fields are listed there."""

    def __repr__(self):
        return ("Census(W=%d C=%d accepted=%d goal_hits=%d tree_size=%d chain_slots=%d rejected=%d first_hit=%s ties=%r)"
                % (self.W, self.C, self.accepted, self.goal_hits, self.tree_size, self.chain_slots, int(self.rejected.sum()),
                   self.first_hit, self.ties[:4]))


def census(rp, samples, max_commit=None, node_limit=-1):
    """One wave `samples` [W][n] on rp's current tree, sequentially and in full; rp is rewound afterwards.

    Fields, all [W] unless noted.  Of the whole wave: near (sequential parent), length, in_wave (the parent was born in this wave),
    depth (length of the chain of in-wave parents above the sample), rejected (no rows), spec_hit (steered from its nearest node
    of the wave-start tree it ends inside the goal box), seq_hit (it does so sequentially; after the first hit the later samples
    are replayed under the ignore set that hit left), ties (list of (t, ids): the nodes whose cost for sample t is bit-equal and
    the minimum over the nodes its search may choose, where there is more than one), first_hit (index or None).
    Of the committed prefix: C -- the first of W, max_commit, the first t at which the accepted count before t has reached
    node_limit + 1 - N0, first hit + 1 --, accepted, goal_hits, tree_size, deepest and chain_slots = deepest + 1."""
    samples = np.ascontiguousarray(samples, dtype=np.float64).reshape(-1, rp.n)
    W = len(samples)
    N0 = rp.size
    mk = rp.mark()
    rp._load(rp.o0)
    c = Census()
    c.W, c.N0 = W, N0
    c.near = np.zeros(W, dtype=np.int64)
    c.length = np.zeros(W, dtype=np.int64)
    c.in_wave = np.zeros(W, dtype=bool)
    c.depth = np.zeros(W, dtype=np.int64)
    c.rejected = np.zeros(W, dtype=bool)
    c.spec_hit = np.zeros(W, dtype=bool)
    c.seq_hit = np.zeros(W, dtype=bool)
    c.ties = []
    born = {}                                                         # node id -> the sample that made it
    for t in range(W):
        x = samples[t]
        near0 = rp.o0.nearest_prefix(x, N0, rp.pruning)
        ln0, xs0, _, _ = rp.o0.steer_from(near0, x)
        c.spec_hit[t] = ln0 > 0 and rp.in_goal(xs0[-1])
        cost = rp.o.costs_prefix(x, rp.size)
        ign = rp.ignored()
        cand = np.flatnonzero(~ign) if (rp.pruning and not ign.all()) else np.arange(rp.size)
        low = cost[cand].min()
        ids = cand[cost[cand] == low]
        if len(ids) > 1:
            c.ties.append((t, [int(i) for i in ids]))
        near, ln, hit = rp.step(x)
        assert near == int(ids[0]), "the oracle's nearest is not the lowest id of the minimum cost"
        c.near[t], c.length[t], c.seq_hit[t] = near, ln, hit
        c.rejected[t] = ln == 0
        if near >= N0:
            c.in_wave[t] = True
            c.depth[t] = c.depth[born[near]] + 1
        if ln > 0:
            born[rp.size - 1] = t
    rp.rewind(mk)
    hits = np.flatnonzero(c.seq_hit)
    c.first_hit = int(hits[0]) if len(hits) else None
    max_commit = W if max_commit is None else int(max_commit)
    room = node_limit + 1 - N0
    C = acc = 0
    for t in range(W):
        if C >= max_commit:
            break
        if node_limit >= 0 and acc >= room:
            break
        C = t + 1
        if c.length[t] > 0:
            acc += 1
            if c.seq_hit[t]:
                break
    c.C, c.accepted = C, acc
    c.goal_hits = int(c.seq_hit[:C].sum())
    c.tree_size = N0 + acc
    c.deepest = int(c.depth[:C].max()) if C else 0
    c.chain_slots = c.deepest + 1
    return c
