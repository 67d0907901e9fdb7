"""
The directed case list of the tree retention (test infrastructure; shared by tests/test_retain_edges_cpu.py and
tests/test_retain_edges_gpu.py): small hand-built trees, one per mechanism csrc/retain.hpp is made of, at the shape where that
mechanism can fail -- the doubling rounds on a chain tight against 2^rounds, the three-launch scan at its block edges and past
its first tile of block sums, the goal stage at a tie in steps, on both strict sides of the box and on nested root paths, the
edge moves at one row, at a full horizon of more than 64 doubles and at "nothing moves", the check at first / last rows.

A case is a Case record: the system's name (and its obstacle table, None = the demo's), horizon_iters, the tree as
Engine.tree_load takes it (state, K, pID, elen, packed xedge / uedge), the goal and goal buffer to set (None = no goal), the
new root and the revalidate flag; `props` holds what the builder promises about it (checked from the reference alone in
tests/test_retain_edges_cpu.py).  dense(case) gives the (N, H, n) edges tests/retain_reference.py retain() takes.

State, gain and every edge row are functions of the node id (values(...)): a row moved to the wrong slot cannot compare equal.
They are not dynamically meaningful -- a retain only moves them.  The builders need NumPy alone and no engine is imported;
make_system / feasible_of / reference load the system classes, the C oracle and the reference when they are called.
"""
import collections
import functools

import numpy as np

Case = collections.namedtuple("Case", "name system obstacles H state K pID elen xedge uedge goal buf root revalidate props")

DIMS = {"pendulum": (4, 1), "boat_advanced": (6, 3)}
# the goal boxes: bounded in the last two dimensions only (binary fractions: lo and hi are exact), open elsewhere.  A node's
# id-derived values of those dimensions (0.25 * (d + 1) + ...) lie far outside; mark_hit() puts a node inside.
BOX = {"pendulum": {2: (32.0, 0.25), 3: (64.0, 0.5)}, "boat_advanced": {4: (32.0, 0.25), 5: (64.0, 0.5)}}
EPS = 2.0 ** -24
OBSTACLE = np.array([[500.0, 500.0, 3.0]])                    # revalidate cases: one circle, far from every passing row


def values(system, H, pID, elen, salt=0):
    """(state, K, packed xedge, packed uedge) of a tree: every entry a function of (node, row, component), all exact."""
    n, m = DIMS[system]
    N = len(pID)
    elen = np.asarray(elen, dtype=np.int64)
    i = np.arange(N, dtype=np.float64)
    state = 0.25 * (np.arange(n) + 1.0)[None, :] + (i[:, None] * n + np.arange(n)[None, :] + salt) * EPS
    K = -((i[:, None, None] * m + np.arange(m)[None, :, None]) * n + np.arange(n)[None, None, :] + 1.0 + salt) * 2.0 ** -22
    owner = np.repeat(np.arange(N), elen)
    k = np.arange(len(owner)) - np.repeat(np.cumsum(elen) - elen, elen)
    row = (owner * H + k).astype(np.float64)
    xedge = 1000.0 + salt + row[:, None] * n + np.arange(n)[None, :] + 0.5
    uedge = -(1000.0 + salt + row[:, None] * m + np.arange(m)[None, :]) - 0.25
    return state, K, xedge, uedge


def goal_of(system):
    """(goal, buffer) of the system's box."""
    n = DIMS[system][0]
    goal, buf = np.zeros(n), np.full(n, np.inf)
    for d, (c, h) in BOX[system].items():
        goal[d], buf[d] = c, h
    return goal, buf


def mark_hit(system, state, i):
    for d, (c, _) in BOX[system].items():
        state[i, d] = c + (i + 1) * EPS


def dense(case):
    """(xedge (N, H, n), uedge (N, H, m)) of a case: rows beyond an edge's length zero."""
    n, m = DIMS[case.system]
    N = len(case.pID)
    live = np.arange(case.H)[None, :] < np.asarray(case.elen)[:, None]
    xe, ue = np.zeros((N, case.H, n)), np.zeros((N, case.H, m))
    xe[live], ue[live] = case.xedge, case.uedge
    return xe, ue


def reference_arguments(case):
    """The first six arguments of retain_reference.retain."""
    xe, ue = dense(case)
    return case.state, case.K, case.pID, case.elen, xe, ue


def goal_box(case):
    """(lo, hi) as Engine.set_resolution forms them, or (None, None)."""
    if case.goal is None:
        return None, None
    return case.goal - np.abs(case.buf), case.goal + np.abs(case.buf)


def make_system(case):
    import lqrrt_amd
    if case.system == "pendulum":
        return lqrrt_amd.systems.DoublePendulum(0)
    return lqrrt_amd.systems.BoatAdvanced(0, obstacles=case.obstacles)


def _case(name, system, H, pID, elen, root, revalidate, hits=(), goal=True, obstacles=None, salt=0, props=None, edit=None):
    pID = np.asarray(pID, dtype=np.int32)
    elen = np.asarray(elen, dtype=np.int32)
    assert pID[0] == -1 and np.all(pID[1:] < np.arange(1, len(pID))) and np.all(pID[1:] >= 0)
    assert elen.min() >= 1 and elen.max() <= H
    state, K, xedge, uedge = values(system, H, pID, elen, salt)
    for i in hits:
        mark_hit(system, state, int(i))
    if edit is not None:
        edit(state, xedge, uedge)
    g, b = goal_of(system) if goal else (None, None)
    return Case(name, system, obstacles, H, state, K, pID, elen, xedge, uedge, g, b, int(root), bool(revalidate), dict(props or {}))


# ------------------------------------------------------------------------------------------------ chain_tight

CHAIN_N = (2, 3, 4, 5, 256, 257, 1024, 1025)


def chain(N, root, H=3, revalidate=False, name=None):
    """A pure chain pID[i] = i - 1: with root 0 and N = 2^k its depth N - 1 needs every one of the k doubling rounds.  The goal
    box holds the last node only: best_steps is the whole chain's sum."""
    i = np.arange(N)
    elen = 1 + (i * i + i // 4 + 1) % H
    hits = [N - 1] if N - 1 > root else []
    steps = 1 + int(elen[root + 1:].sum())
    return _case(name or "chain_tight-N%d-r%d" % (N, root), "pendulum", H, i - 1, elen, root, revalidate, hits,
                 props=dict(depth=N - 1 - root, best_steps=steps if hits else -1))


# ------------------------------------------------------------------------------------------------ block_edges

BLOCK_N = (1, 2, 255, 256, 257, 511, 512, 513)


def block(N, kind, root, H=3, name=None, goal=True, revalidate=False):
    """Bushy trees at the scan's block edges.  heap: pID[i] = (i - 1) // 2 -- the subtree of node r is the heap's, so its size is
    known in closed form (N = 512: root 1 keeps 256, root 3 keeps 128, root 7 keeps 64).  comb: pID[i] = i - 2 -- two interleaved
    chains, a root keeps every other node above it, so kept and dropped nodes alternate through every block."""
    i = np.arange(N)
    pID = (i - 1) // 2 if kind == "heap" else np.maximum(i - 2, 0)
    pID[0] = -1
    elen = 1 + (i * 7 + i // 3) % H
    hits = sorted(set([j for j in range(N) if j % 37 == 5] + [N - 1]))
    props = {}
    if kind == "heap" and N == 512 and root in (1, 3, 7):
        props["kept"] = {1: 256, 3: 128, 7: 64}[root]
    if N == 1 or root == N - 1:
        props["kept"] = 1
    return _case(name or "block_edges-%s-N%d-r%d" % (kind, N, root), "pendulum", H, pID, elen, root, revalidate, hits, goal=goal,
                 props=props)


def _block_names():
    out = []
    for N in BLOCK_N:
        for kind in ("heap", "comb"):
            for root in sorted(set(r for r in (0, 255, 256, N - 1) if 0 <= r < N)):
                out.append(("block_edges-%s-N%d-r%d" % (kind, N, root), functools.partial(block, N, kind, root)))
    for root in (1, 3, 7):
        out.append(("block_edges-heap-N512-r%d" % root, functools.partial(block, 512, "heap", root)))
    return out


# ------------------------------------------------------------------------------------------------ scan_carry

SCAN_N = 65537 + 300


def scan_carry():
    """65837 nodes = 258 blocks: the second tile of retain_scan_sums_body and its carry.  Node 1 (the new root) is the hub of a
    star of 4-node chains; every seventh chain hangs off node 0 instead and is dropped with it.  Chain heads in blocks >= 256
    have their kept parent (node 1) in block 0, the first scan tile."""
    N, H = SCAN_N, 2
    i = np.arange(N)
    c = (i - 2) // 4
    head = (i - 2) % 4 == 0
    pID = np.where(head, np.where(c % 7 == 3, 0, 1), i - 1)
    pID[0], pID[1] = -1, 0
    elen = 1 + (i // 3) % 2
    hits = [j for j in range(777, N, 1000)]
    return _case("scan_carry", "pendulum", H, pID, elen, 1, False, hits)


# ------------------------------------------------------------------------------------------------ goal_ties

def goal_ties(variant):
    """Node 1 is the hub of 60 chains of 10 nodes (heads 11 + 10 c); node 0 and a chain below node 2 are dropped, so new id =
    old id - 10.  Hits A = old 115 (new 105) and B = old 415 (new 405) lie in different 256-blocks of the goal launch.
    'tie': both 11 steps from the new root along different edge lengths -- the lower id wins.  'fewer_high': B has 9 steps --
    the higher id wins.  Four nodes 20 or more steps deep sit on the box: exactly on lo (dimension 2) and exactly on hi
    (dimension 3) -- no hits -- and their np.nextafter twins one ulp inside -- hits."""
    H = 3
    N = 11 + 600
    i = np.arange(N)
    pID = np.where((i - 11) % 10 == 0, 1, i - 1)
    pID[:3] = (-1, 0, 0)
    elen = 2 + i % 2
    elen[111:116] = (3, 1, 2, 3, 1)
    elen[411:416] = (2, 2, 2, 2, 2) if variant == "tie" else (2, 1, 2, 2, 1)
    on_lo, in_lo, on_hi, in_hi = 11 + 210 + 9, 11 + 200 + 9, 11 + 510 + 9, 11 + 500 + 9
    (d_lo, (c_lo, h_lo)), (d_hi, (c_hi, h_hi)) = sorted(BOX["pendulum"].items())

    def edit(state, xedge, uedge):
        state[on_lo, d_lo] = c_lo - h_lo
        state[in_lo, d_lo] = np.nextafter(c_lo - h_lo, np.inf)
        state[on_hi, d_hi] = c_hi + h_hi
        state[in_hi, d_hi] = np.nextafter(c_hi + h_hi, -np.inf)
    props = dict(pair=(105, 405), pair_steps=(11, 11 if variant == "tie" else 9), best_end=105 if variant == "tie" else 405,
                 on_box=(on_lo - 10, on_hi - 10), inside=(in_lo - 10, in_hi - 10))
    return _case("goal_ties-" + variant, "pendulum", H, pID, elen, 1, False, [115, 415, on_lo, in_lo, on_hi, in_hi], props=props,
                 edit=edit)


# ------------------------------------------------------------------------------------------------ goal_nested

def goal_nested():
    """A spine of 219 nodes below the new root (node 1), ids interleaved with what leaves it: hits on the spine at depths 10, 70
    and 199, two 5-node side branches that leave it at depths 65 and 130 and end in a hit, leaf twigs every tenth depth that
    nothing ignores.  Nodes 0, 2, 3 are dropped; fillers bring the kept count to exactly 256 = four full ignore words (the
    host copies kept / 64 + 1 = 5)."""
    H = 2
    pid = [-1, 0, 0, 2]
    spine = {0: 1}
    hits, union = [], set()
    for d in range(1, 220):
        spine[d] = len(pid)
        pid.append(spine[d - 1])
        if d in (10, 70, 199):
            hits.append(spine[d])
            union.update(spine[q] for q in range(d + 1))
        if d in (65, 130):
            prev = spine[d]
            union.update(spine[q] for q in range(d + 1))
            for _ in range(5):
                pid.append(prev)
                prev = len(pid) - 1
                union.add(prev)
            hits.append(prev)
        elif d % 10 == 5:
            pid.append(spine[d])
    while len(pid) - 3 < 256:
        pid.append(spine[100])
    i = np.arange(len(pid))
    return _case("goal_nested", "pendulum", H, pid, 1 + i % 2, 1, False, hits,
                 props=dict(kept=256, union=len(union), hits=5))


# ------------------------------------------------------------------------------------------------ move_widths

def move_widths(variant):
    """boat_advanced with horizon_iters 11: a full edge is 66 doubles of states (two passes of the 64-lane copy) and 33 of
    efforts.  'moves': root 1 drops nodes 0, 3 and 5, so every kept node moves, and the kept neighbours have edges of 1, 11,
    6, 11 and 1 rows.  'identity': root 0 without revalidation keeps everything; the old root's edge has 7 rows, so the only
    thing written is elen[0] (and the seed's one-row edge)."""
    H = 11
    pID = [-1, 0, 1, 0, 2, 0, 4, 1, 7]
    elen = [7, 5, 1, 3, 11, 2, 6, 11, 1]
    root = 1 if variant == "moves" else 0
    return _case("move_widths-" + variant, "boat_advanced", H, pID, elen, root, False, [4, 8],
                 props=dict(kept=6 if variant == "moves" else 9))


# ------------------------------------------------------------------------------------------------ revalidate_small

def revalidate_tree(N=300, root=3, salt=0):
    """(pID, elen, fail) of the revalidation cases: fail[i] = 'last' / 'first' / 'only' (a one-row edge) / None.  Nodes 0, 1, 2
    lie below the new root 3; nodes 4 and 5 and every 25th node after them hang off node 2's side (outside), the rest forms a
    heap-shaped subtree of node 3.  With root 3 the root's own edge fails in its last row; node 4 (outside of it) fails too; the
    subtree node `clean` fails above descendants that all pass."""
    pid = [-1, 0, 0, 1, 2, 4]
    sub = [3]
    for i in range(6, N):
        if i % 25 == 0:
            pid.append(4 + i % 2)
        else:
            pid.append(sub[(len(sub) - 1) // 2])
            sub.append(i)
    clean = sub[60]
    below, inside = set([clean]), set(sub)
    for i in range(clean + 1, N):
        if pid[i] in below:
            below.add(i)
    fail = [None] * N
    fail[4] = "last"
    if root == 3:
        fail[3] = "last"
    for k, i in enumerate(j for j in sub[1:] if j % 11 == 7 and j not in below):
        fail[i] = ("last", "first", "only")[k % 3]
    fail[clean] = "first"
    elen = [3 if fail[i] in ("last", "first") else 1 if fail[i] == "only" else 1 + (i + salt) % 3 for i in range(N)]
    return pid, elen, fail, clean, sorted(below - set([clean])), inside


def revalidate(name, N, root, flag, salt=0):
    """boat_advanced beside one circle (OBSTACLE), horizon_iters 3.  A passing row lies a kilometre away, a failing row has the
    hull over the circle's centre; velocities stay inside the planning speed box."""
    H = 3
    pid, elen, fail, clean, below, inside = revalidate_tree(N, root, salt)

    def edit(state, xedge, uedge):
        r = 0
        for i in range(N):
            for k in range(elen[i]):
                bad = fail[i] == "only" or (fail[i] == "last" and k == elen[i] - 1) or (fail[i] == "first" and k == 0)
                xedge[r] = (2000.0 + 8 * i + k, -1000.0 - 0.5 * i, 0.125 * (i % 7), (k + 1) * 2.0 ** -10, (i % 5) * 2.0 ** -12, -(i % 3) * 2.0 ** -12)
                if bad:
                    xedge[r, 0], xedge[r, 1] = OBSTACLE[0, 0] + (i * H + k) * 2.0 ** -10, OBSTACLE[0, 1]
                r += 1
    hits = [i for i in sorted(inside) if i % 13 == 4] + [4]
    return _case(name, "boat_advanced", H, pid, elen, root, flag, hits, obstacles=OBSTACLE, salt=salt, edit=edit,
                 props=dict(fail=fail, clean=clean, below_clean=below))


# ------------------------------------------------------------------------------------------------ the registry

def _registry():
    reg = collections.OrderedDict()
    for N in CHAIN_N:
        for root in sorted(set((0, 1, N - 2))):
            reg["chain_tight-N%d-r%d" % (N, root)] = functools.partial(chain, N, root, 3, root == 1)
    reg.update(_block_names())
    reg["scan_carry"] = scan_carry
    reg["goal_ties-tie"] = functools.partial(goal_ties, "tie")
    reg["goal_ties-fewer_high"] = functools.partial(goal_ties, "fewer_high")
    reg["goal_nested"] = goal_nested
    reg["move_widths-moves"] = functools.partial(move_widths, "moves")
    reg["move_widths-identity"] = functools.partial(move_widths, "identity")
    reg["revalidate_small"] = functools.partial(revalidate, "revalidate_small", 300, 3, True)
    # members of the batched calls.  Pendulum, horizon_iters 2 (scan_carry's): sizes from 1 to 65837 in one call.
    reg["multi-one"] = functools.partial(block, 1, "heap", 0, 2, "multi-one")
    reg["multi-two"] = functools.partial(chain, 2, 0, 2, True, "multi-two")
    reg["multi-comb257"] = functools.partial(block, 257, "comb", 255, 2, "multi-comb257", False, True)      # (no goal)
    reg["multi-chain1024"] = functools.partial(chain, 1024, 0, 2, False, "multi-chain1024")
    reg["multi-heap513-r1"] = functools.partial(block, 513, "heap", 1, 2, "multi-heap513-r1")
    reg["multi-heap513-r2"] = functools.partial(block, 513, "heap", 2, 2, "multi-heap513-r2")
    # boat_advanced beside the circle, horizon_iters 3: with / without revalidation, moving / keeping all, hits / one node kept
    reg["multi-reval-a"] = functools.partial(revalidate, "multi-reval-a", 300, 3, True)
    reg["multi-reval-b"] = functools.partial(revalidate, "multi-reval-b", 277, 0, True, 1)
    reg["multi-noreval-moves"] = functools.partial(revalidate, "multi-noreval-moves", 190, 3, False, 2)
    reg["multi-keeps-all"] = functools.partial(revalidate, "multi-keeps-all", 261, 0, False, 3)
    reg["multi-leaf"] = functools.partial(revalidate, "multi-leaf", 130, 129, True, 4)
    return reg


REGISTRY = _registry()


def names(prefix):
    return [k for k in REGISTRY if k.startswith(prefix)]


@functools.lru_cache(maxsize=None)
def case(name):
    c = REGISTRY[name]()
    assert c.name == name, (c.name, name)
    return c


def feasible_of(c):
    """The C oracle's feasibility test of the case's world (None: the case does not revalidate)."""
    if not c.revalidate:
        return None
    import coracle
    return coracle.COracle(make_system(c), 16).feasible


@functools.lru_cache(maxsize=None)
def reference(name):
    """retain_reference.retain of a case: computed once per process, shared, never written to."""
    import retain_reference as rr
    c = case(name)
    lo, hi = goal_box(c)
    return rr.retain(*reference_arguments(c), c.root, feasible_of(c), lo, hi)


# The batched calls (Engine.tree_retain_multi): lists of member cases that share model, horizon and form of S.
MULTI_MIXED = ("multi-one", "multi-two", "multi-comb257", "multi-chain1024", "scan_carry")
# a member with a zero workgroup count BETWEEN two members with a non-zero one, per launch grid (grid_counts below)
MULTI_ZERO = {
    "check": ("multi-reval-a", "multi-noreval-moves", "multi-reval-b"),
    "move": ("multi-reval-a", "multi-keeps-all", "multi-reval-b"),
    "goal": ("multi-reval-a", "multi-leaf", "multi-noreval-moves"),
    "all": ("multi-reval-a", "multi-keeps-all", "multi-reval-b", "multi-leaf", "multi-noreval-moves"),
}
MULTI_SHARED = ("multi-heap513-r1", "multi-heap513-r2")


def grid_counts(name):
    """Workgroups a member takes in the check, move and goal launches of the batched call (engine_retain.hpp c_check, c_old,
    c_goal), from the reference's result."""
    c, st = case(name), reference(name)["stats"]
    N, kept = st["old_size"], st["kept"]
    return dict(check=N - c.root if c.revalidate else 0, move=N if kept < N else 0,
                goal=(kept - 1 + 255) // 256 if c.goal is not None and kept > 1 else 0)
