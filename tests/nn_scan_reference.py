"""
NumPy float64 model of "nearest node of a compiled-in system" (csrc/nn_scan.hpp k_nn_scan / k_nn_reduce behind lqrrt_nn_argmin),
the two table builders of tests/test_nn_scan_gpu.py, and a restatement of the few host lines that choose the scan's launch shape.

Model (planner.py:340-350, :240-245):
  errors     xq - node, the wrapped dimensions in the form of oracle/systems_np.py wrap_err
  costs      np.sum(np.tensordot(d, S, axes=1) * d, axis=1); S identity, one matrix, or one matrix per query
  selection  first id in stable-argsort order that is not ignored; every node ignored -> the overall first

Builders:
  periodic_table(base, N)   nodes[j] = base[j % s]: the query base[r] has bit-equal costs at r, r + s, r + 2s, ... in every angle
                            mode and for every S (identical states), so the answer is the lowest eligible id congruent to r, exactly
  self_table(system, N)     nodes drawn from the system's sample space (zero-width dimensions widened), no two alike: node k is the
                            unique nearest of query k, at cost 0

Launch plan: pick_chunks / launch_plan restate csrc/engine_launch.hpp pick_chunks, nn_wg4_default and the wg4 / XCD conditions of
launch_nn and nn_scan_body, so that a GPU case can assert that it reaches the path it is named after; tests/test_nn_scan_cpu.py
checks the restatement against hand-computed values.
"""
import numpy as np

from systems_np import wrap_err

MAXCH = 1024                 # csrc/engine_state.hpp lqrrt_engine::MAXCH
WG4_FROM = 32768             # csrc/engine_launch.hpp nn_wg4_default

# forms of S a scan launch is instantiated for (csrc/kernels.hpp quad_cost); which of them have the four-wavefront form (launch_nn wg4_has)
FORMS = ("ident", "dense", "diag", "band2", "persample")
WG4_FORMS = ("ident", "dense", "band2")


class ScanModel(object):
    """The node table of one compiled-in system: states (N, n), the system's wrapped dimensions, ignore flags."""

    def __init__(self, nodes, wrap_dims, ignored=None):
        self.nodes = np.array(nodes, dtype=np.float64)
        self.N, self.n = self.nodes.shape
        self.wrap_dims = tuple(wrap_dims)
        self.ign = np.zeros(self.N, dtype=bool) if ignored is None else np.array(ignored, dtype=bool)
        assert self.ign.shape == (self.N,)

    def errors(self, xq):
        d = np.asarray(xq, dtype=np.float64) - self.nodes
        for w in self.wrap_dims:
            d[:, w] = wrap_err(xq[w], self.nodes[:, w])
        return d

    def costs(self, xq, S=None):
        """Cost of every node for ONE query (planner.py:350)."""
        S = np.eye(self.n) if S is None else np.asarray(S)
        d = self.errors(xq)
        return np.sum(np.tensordot(d, S, axes=1) * d, axis=1)

    def cost_rows(self, xs, S=None):
        """(W, N) costs; S None, (n, n), or (W, n, n) = one matrix per query."""
        xs = np.asarray(xs, dtype=np.float64)
        per = S is not None and np.ndim(S) == 3
        return np.array([self.costs(x, S[t] if per else S) for t, x in enumerate(xs)]).reshape(len(xs), self.N)

    def select(self, costs, use_ignore=True):
        """planner.py:240-245."""
        order = np.argsort(costs, kind="stable")
        if use_ignore:
            live = order[~self.ign[order]]
            if len(live):
                return int(live[0])
        return int(order[0])

    def answers(self, rows, use_ignore=True):
        """select() of every row.  (The first minimum among the eligible nodes IS the first eligible id in stable-argsort order;
        np.argmin returns the first minimum -- one pass per row instead of a sort; tests/test_nn_scan_cpu.py holds the two together.)"""
        rows = np.asarray(rows)
        if use_ignore and not self.ign.all():
            rows = np.where(self.ign[None, :], np.inf, rows)
        return np.argmin(rows, axis=1).astype(np.int64)

    def assert_rows_unique(self, rows, ids):
        """Row t has its only zero at ids[t] and nothing else below 1e-6: node ids[t] is the unique nearest of its own state."""
        for c, k in zip(rows, ids):
            c = c.copy()
            assert c[k] == 0.0, (k, c[k])
            c[k] = np.inf
            assert c.min() > 1e-6, "nodes %d and %d coincide (cost %g)" % (k, int(np.argmin(c)), c.min())

    def assert_distinct(self, S=None):
        """No two nodes coincide under the metric S (wrapped dimensions modulo a turn): a node's own row has one zero."""
        self.assert_rows_unique(self.cost_rows(self.nodes, S), range(self.N))


def periodic_table(base, N):
    base = np.asarray(base, dtype=np.float64)
    return base[np.arange(N) % len(base)].copy()


def velocity_table(system, base, N, free_dims, rs):
    """periodic_table(base, N) with the states in `free_dims` drawn afresh for every node: under an S whose rows and columns of
    those states are zero (ros_boat 'car': S = diag(1,1,1,0,0,0)) the copies r, r + s, ... still have bit-equal costs for ANY
    query -- the differing errors only ever meet a zero of S -- although the nodes themselves differ."""
    nodes = periodic_table(base, N)
    lo, hi = widened_space(system)
    fd = list(free_dims)
    nodes[:, fd] = lo[fd] + (hi[fd] - lo[fd]) * rs.random_sample((N, len(fd)))
    return nodes


def velocity_queries(system, base, res, rs, offset=1e-3):
    """Two queries per residue r, each with a velocity of its own: ON the position of base[r] (cost 0 at every copy), and `offset`
    beside it in the first state (the same non-zero cost at every copy; base[r] still the nearest position by far)."""
    lo, hi = widened_space(system)
    on = base[list(res)].copy()
    on[:, 3:] = lo[3:] + (hi[3:] - lo[3:]) * rs.random_sample((len(on), len(lo) - 3))
    beside = on.copy()
    beside[:, 3:] = lo[3:] + (hi[3:] - lo[3:]) * rs.random_sample((len(on), len(lo) - 3))
    beside[:, 0] += offset
    return np.vstack((on, beside))


def lowest_congruent(N, s, r, ign=None):
    """The lowest id j = r (mod s), j < N, that is not ignored; None if every copy is (or r has no copy)."""
    for j in range(r, N, s):
        if ign is None or not ign[j]:
            return j
    return None


def widened_space(system):
    """The system's sample_space with zero-width dimensions opened: a full turn for a wrapped one, +-1 otherwise."""
    lo, hi = (np.array(v, dtype=np.float64) for v in zip(*system.sample_space))
    for d in range(len(lo)):
        if hi[d] == lo[d]:
            w = 3.0 if d in system.wrap_dims else 1.0          # (+-3 rad: short of a full turn, two angles never alias)
            lo[d], hi[d] = lo[d] - w, hi[d] + w
        elif d in system.wrap_dims and hi[d] - lo[d] > 6.0:
            c = 0.5 * (lo[d] + hi[d])
            lo[d], hi[d] = c - 3.0, c + 3.0
    return lo, hi


def self_table(system, N, rs):
    lo, hi = widened_space(system)
    return lo + (hi - lo) * rs.random_sample((N, len(lo)))


# ------------------------------------------------------------------------------------------------ launch plan

def pick_chunks(count, W, nn_waves=0, min_chunk=16):
    """csrc/engine_launch.hpp pick_chunks: (chunk, n_chunks).  nn_waves / min_chunk: LQRRT_NN_WAVES / LQRRT_NN_MIN_CHUNK."""
    groups = (W + 63) // 64
    target = nn_waves if nn_waves > 0 else (4096 if groups >= 8 else 2048)
    want = max(1, min(target // max(groups, 1), MAXCH))
    c = (count + want - 1) // want
    c = max((c + 7) // 8 * 8, max(8, min_chunk // 8 * 8))
    return c, max(1, (count + c - 1) // c)


def launch_plan(count, W, form="ident", wg4_env=-1, nn_waves=0, min_chunk=16):
    """What launch_nn launches for a tree scan of `count` nodes and W queries with S of `form`:
         chunk, n_sub      nodes per wavefront, wavefronts over the table
         wg4               four wavefronts per workgroup (WPB = 4), one partial per four chunks
         parts             partials per query, what k_nn_reduce reads (gy)
         last_group        real chunks in the last workgroup (WPB = 4: 1..4)
         gx, gy, xcd       the grid; xcd: the workgroups are re-indexed (gx * gy % 8 == 0)
         reduce_stride     k_nn_reduce's lanes loop (more than 64 partials)"""
    assert form in FORMS
    chunk, n_sub = pick_chunks(count, W, nn_waves, min_chunk)
    wg4 = form in WG4_FORMS and n_sub >= 8 and (wg4_env != 0 if wg4_env >= 0 else count >= WG4_FROM)
    parts = (n_sub + 3) // 4 if wg4 else n_sub
    gx = (W + 63) // 64
    return dict(chunk=chunk, n_sub=n_sub, wg4=wg4, parts=parts, last_group=(n_sub - 4 * (parts - 1)) if wg4 else 1,
                gx=gx, gy=parts, xcd=(gx * parts) % 8 == 0, reduce_stride=parts > 64)


def angle_mode(xs, wrap_dims, fixed=None):
    """nn_scan_body's mode of every 64-query wavefront of xs (padded lanes repeat the last query): 2 = all carry the sampler's
    fixed angles (`fixed`: those angles, or None when the sampler fixes none), 1 = all carry the same angles, else 0."""
    xs = np.asarray(xs, dtype=np.float64)
    if not wrap_dims:
        return [0] * ((len(xs) + 63) // 64)
    out = []
    for lo in range(0, len(xs), 64):
        a = xs[lo:lo + 64][:, list(wrap_dims)]
        if fixed is not None and np.all(a == np.asarray(fixed, dtype=np.float64)):
            out.append(2)
        elif np.all(a == a[0]):
            out.append(1)
        else:
            out.append(0)
    return out


# ------------------------------------------------------------------------------------------------ the cases, shared by the CPU and GPU tests

SELF_SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 144, 1023, 1024)
W_CUTS = (1, 2, 63, 64, 65, 129)                       # queries taken from the END of the table
PERIODS = (1, 2, 3, 4, 5, 63, 64, 65, 16, 24, 4 * 16, 64 * 16)
TIE_SIZES = (1025, 16400 + 7)
BIG_N = 32768 + 37                                     # the smallest default WPB = 4 table with a lone chunk in its last workgroup
BIG_PERIODS = (40, 160, 2560, 32768)
DIAG_PERIODS = (1, 3, 4, 16, 64, 65)                   # velocity_table at N = 1025: copies in one quad, one chunk, other chunks


def tie_residues(s, seed=0):
    """Residues r whose query base[r] is asked of a period-s table: every r < 8 and 64 more (all of them when s is small)."""
    rs = np.random.RandomState(1000 + s + seed)
    more = rs.choice(s, min(64, s), replace=False)
    return sorted(set(range(min(8, s))) | set(int(r) for r in more))


def tie_ignore_sets(N, s, seed=0):
    """[(name, flags)]: none, a random half, every copy but the highest of its residue, all."""
    rs = np.random.RandomState(2000 + N + s + seed)
    return [("none", np.zeros(N, dtype=bool)), ("half", rs.random_sample(N) < 0.5),
            ("all but the highest copy", np.arange(N) + s < N), ("all", np.ones(N, dtype=bool))]


def self_ignore_sets(N):
    """[(name, flags)]: none, all but the last node, ids 0..63, all."""
    but_last = np.ones(N, dtype=bool)
    but_last[N - 1] = False
    word0 = np.zeros(N, dtype=bool)
    word0[:64] = True
    return [("none", np.zeros(N, dtype=bool)), ("all but the last", but_last), ("ids 0..63", word0), ("all", np.ones(N, dtype=bool))]
