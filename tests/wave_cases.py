"""
Crafted exact-mode waves: explicit sample lists (Engine.push_samples) that put one hard thing at a chosen place of a wave -- a
dependency chain as deep as the wave, an exact cost tie between two in-wave records or with a snapshot node, a duplicate, a
speculative goal hit that repair takes away, a goal hit at a chosen index -- each with the condition it has to satisfy ACCORDING
TO THE CENSUS ALONE (tests/wave_reference.py).  tests/test_wave_cpu.py checks every condition on the CPU; a case that lost its
point fails there instead of testing less.  tests/test_wave_gpu.py runs the cases through the engine's repair paths.

All on the 12-state double integrator with 50 boxes (dense S, linear dynamics that mirror exactly in y) unless noted.  Host only.
"""
import numpy as np

import lqrrt_amd
from wave_reference import Replay, census

_systems = {}


def system(name):
    if name not in _systems:
        mk = lqrrt_amd.systems.SYSTEMS[name]
        _systems[name] = mk(n_boxes=50, seed=0) if name == "double_integrator" else mk(0)
    return _systems[name]


def pt(n, *xyz):
    x = np.zeros(n)
    x[:len(xyz)] = xyz
    return x


def fillers(root, count, first=0):
    """`count` distinct samples far away in z (40 below the root), fanned out a little in x and y: their nodes leave the root
    downwards, away from everything a case is about."""
    out = np.tile(np.asarray(root, dtype=np.float64), (count, 1))
    k = np.arange(first, first + count)
    out[:, 0] += 0.37 * (k % 11) - 1.85
    out[:, 1] += 0.29 * (k % 7) - 0.87
    out[:, 2] -= 40.0 + 0.013 * k
    return out


def place(W, root, placed):
    """A wave of W samples: `placed` {index: sample}, fillers everywhere else."""
    xs = fillers(root, W)
    for i, x in placed.items():
        assert 0 <= i < W
        xs[i] = x
    return xs


class Case(object):
    """name; system name; root; pre: sample lists committed as waves of their own before; samples [W][n]; check(census) asserts
    the case's condition; pruning."""

    def __init__(self, name, samples, check, root, sysname="double_integrator", pre=(), pruning=True):
        self.name, self.sysname, self.root, self.pre, self.pruning = name, sysname, np.asarray(root, dtype=np.float64), list(pre), pruning
        self.samples = np.ascontiguousarray(samples, dtype=np.float64)
        self.W = len(self.samples)
        self.check = check

    def __repr__(self):
        return self.name

    @property
    def system(self):
        return system(self.sysname)

    def replay(self, extra=0):
        """A Replay holding the case's start tree (root + the `pre` waves)."""
        rp = Replay(self.system, 1 + sum(len(p) for p in self.pre) + self.W + extra + 8, root=self.root, pruning=self.pruning)
        for p in self.pre:
            rp.run(p)
        return rp

    def census(self, **kw):
        c = census(self.replay(), self.samples, **kw)
        return c


# ---------------------------------------------------------------------------------------------- chain
P = pt(12, 50, 50, 50)


def zigzag(root, count):
    """A march in x with spacing 1.5 from the root, y alternating by 1.5: every sample's nearest node is the one its predecessor
    made (at spacing 1.0 the two sides of the zigzag grow a chain each, of half the depth)."""
    out = np.tile(np.asarray(root, dtype=np.float64), (count, 1))
    k = np.arange(count)
    out[:, 0] += 1.5 * (k + 1)
    out[:, 1] += np.where(k % 2 == 0, 1.5, -1.5)
    return out


def chain_case(W):
    def check(c):
        assert c.deepest == W - 1 and not c.rejected.any(), c
    return Case("chain_%d" % W, zigzag(P, W), check, P)


def chain_car_case():
    s = system("car")
    root = np.array(s.x0, dtype=np.float64)
    xs = np.tile(root, (256, 1))
    k = np.arange(256)
    xs[:, 0] += 1.0 * (k + 1)
    xs[:, 1] += np.where(k % 2 == 0, 1.5, -1.5)
    xs[:, 3] = 1.0

    def check(c):
        rej = np.flatnonzero(c.rejected)
        made = np.flatnonzero(~c.rejected)
        assert len(rej) >= 1 and c.deepest >= 8, c
        # a rejected sample with in-wave successors: something after it has an in-wave parent
        assert any(c.in_wave[r + 1:].any() for r in rej[:1]), c
        assert len(made) >= 8
    return Case("chain_car_256", xs, check, root, sysname="car")


def chain_padded_case(W):
    """The chain's links at wave indices 28..35 and 252..259 (those below W), fillers elsewhere: its in-wave parents cross the
    indices 31/32 (k_decide's chunks of 32) and 255/256 (the fused rounds' limit, the TRI scan's fourth 64-sample group)."""
    where = [i for i in list(range(28, 36)) + list(range(252, 260)) if i < W]
    z = zigzag(P, len(where))

    def check(c):
        for a, b in zip(where, where[1:]):
            assert c.near[b] == c.N0 + int((~c.rejected[:a + 1]).sum()) - 1, (a, b, c)      # b's parent is the node a made
        assert not c.rejected[where].any()
        assert c.depth[where[-1]] >= len(where) - 1
    return Case("chain_padded_%d" % W, place(W, P, dict(zip(where, z))), check, P)


# ---------------------------------------------------------------------------------------------- ties
A = P + pt(12, 5, +6, 0)
B = P + pt(12, 5, -6, 0)
Cc = P + pt(12, 14, 0, 0)


def _tie_check(first, second, last):
    def check(c):
        tie = [ids for t, ids in c.ties if t == last]
        assert tie, "no exact tie at the last sample: %r" % c
        n_first = c.N0 + int((~c.rejected[:first + 1]).sum()) - 1
        n_second = c.N0 + int((~c.rejected[:second + 1]).sum()) - 1
        assert tie[0] == [n_first, n_second], (tie, n_first, n_second)
        assert c.near[last] == n_first and not c.rejected[[first, second, last]].any()
    return check


def tie_case(W, i, j, swap=False):
    a, b = (B, A) if swap else (A, B)
    return Case("tie_%d_%d_%d%s" % (W, i, j, "_swapped" if swap else ""), place(W, P, {i: a, j: b, W - 1: Cc}),
                _tie_check(i, j, W - 1), P)


def snapshot_tie_case(W=2, swap=False):
    """[A] committed as a wave of its own, then [fillers.., B, C]: B's record ties with A's snapshot node; the older node wins."""
    a, b = (B, A) if swap else (A, B)

    def check(c):
        tie = [ids for t, ids in c.ties if t == W - 1]
        n_b = c.N0 + int((~c.rejected[:W - 1]).sum()) - 1
        assert tie and tie[0] == [1, n_b], (tie, c)
        assert c.N0 == 2 and c.near[W - 1] == 1 and not c.in_wave[W - 1]
    return Case("snapshot_tie_%d%s" % (W, "_swapped" if swap else ""), place(W, P, {W - 2: b, W - 1: Cc}), check, P, pre=[[a]])


def duplicates_case(W=3, at=0):
    D = P + pt(12, 9, 4, 0)

    def check(c):
        ln = c.length[at:at + 3]
        assert ln[0] > 0 and ln[1] > 0 and ln[2] == 0, c.length
        assert c.in_wave[at + 1] and c.in_wave[at + 2]
    return Case("duplicates_%d_%d" % (W, at), place(W, P, {at: D, at + 1: D, at + 2: D}), check, P)


# ---------------------------------------------------------------------------------------------- vanishing goal hit
G = pt(12, 90, 85, 90)                                       # a root inside reach of the goal box (82, 98)^3


def vanishing_case(form, W=4, at=1, true_hit=False):
    """Form 1: S = (90, 78, 90), T = (90, 81.8, 90): T hits the goal from the snapshot root, sequentially it steers from S's node
    and does not.  Form 2: S = (90, 79, 90), T = (90, 81.5, 90): T's sequential edge is rejected.  F1, F2 follow with in-wave
    parents; `true_hit` appends a sample at the goal centre.  T sits at wave index `at`, S right before it."""
    s = system("double_integrator")
    S_ = pt(12, 90, 78, 90) if form == 1 else pt(12, 90, 79, 90)
    T_ = pt(12, 90, 81.8, 90) if form == 1 else pt(12, 90, 81.5, 90)
    F1, F2 = pt(12, 95, 78, 90), pt(12, 90, 75, 90)
    placed = {at - 1: S_, at: T_, at + 1: F1, at + 2: F2}
    if true_hit:
        placed[at + 3] = np.array(s.goal, dtype=np.float64)
    assert W >= at + 3 + (1 if true_hit else 0)

    def check(c):
        assert c.spec_hit[at] and not c.seq_hit[at], c
        assert c.in_wave[at + 1:at + 3].any()
        if form == 2:
            assert c.rejected[at]
        else:
            assert not c.rejected[at] and c.in_wave[at]
        if true_hit:
            assert c.seq_hit[at + 3] and c.first_hit == at + 3
        else:
            assert c.first_hit is None
    return Case("vanishing%d_%d_at%d%s" % (form, W, at, "_hit" if true_hit else ""), place(W, G, placed), check, G)


# ---------------------------------------------------------------------------------------------- goal hits at chosen indices
def hit_case(W, t, second=None):
    s = system("double_integrator")
    goal = np.array(s.goal, dtype=np.float64)
    placed = {t: goal}
    if second is not None:
        placed[second] = goal

    def check(c):
        assert c.first_hit == t, c
        if second is not None:
            assert c.C == t + 1
    return Case("hit_%d_at%d%s" % (W, t, "" if second is None else "_and%d" % second), place(W, G, placed), check, G)


# ---------------------------------------------------------------------------------------------- the lists
CHAIN_SIZES = (2, 63, 64, 65, 129, 193, 255, 256)
TRI_SIZES = (257, 288, 289, 511, 1000)


def small_cases():
    """Every crafted wave of at most 256 samples."""
    out = [chain_case(W) for W in CHAIN_SIZES]
    out.append(chain_car_case())
    out += [tie_case(3, 0, 1), tie_case(3, 0, 1, swap=True), tie_case(66, 63, 64), tie_case(256, 0, 255 - 1), tie_case(256, 190, 200)]
    out += [snapshot_tie_case(2), snapshot_tie_case(2, swap=True), snapshot_tie_case(65), snapshot_tie_case(256)]
    out += [duplicates_case(3, 0), duplicates_case(66, 62)]
    for form in (1, 2):
        out += [vanishing_case(form), vanishing_case(form, W=5, true_hit=True), vanishing_case(form, W=70, at=63),
                vanishing_case(form, W=70, at=64), vanishing_case(form, W=70, at=63, true_hit=True),
                vanishing_case(form, W=70, at=64, true_hit=True)]
    for W in (65, 256):
        out += [hit_case(W, t) for t in sorted({0, 1, 63, 64, W - 1})]
    out += [hit_case(65, 1, second=40), hit_case(256, 64, second=65)]
    return out


def tri_cases():
    """Crafted waves above 256 samples: the TRI scan's sizes, W % 4 != 0 among them."""
    out = [chain_padded_case(W) for W in TRI_SIZES]
    out += [tie_case(257, 0, 255), tie_case(289, 255, 256), tie_case(1000, 31, 998)]
    out += [snapshot_tie_case(289), vanishing_case(1, W=288, at=256), vanishing_case(2, W=511, at=255, true_hit=True)]
    out += [hit_case(257, 256), hit_case(1000, 64, second=700), duplicates_case(511, 254)]
    return out


def limit_cases():
    """(case, max_commit, node_limit): the chain and hit waves cut by max_commit in {0, 1, t, t + 1, W}, by a node limit that leaves
    room for 0, 1 and W // 2 nodes, and by one that falls on the hit sample and on the sample before it.  None = no limit."""
    out = []
    ch = chain_case(65)
    for mc in (0, 1, 64, 65):
        out.append((ch, mc, -1))
    for room in (0, 1, 32):
        out.append((ch, None, room))                          # node_limit = N0 + room - 1
    for W, t in ((65, 63), (256, 64)):
        h = hit_case(W, t)
        for mc in (0, 1, t, t + 1, W):
            out.append((h, mc, -1))
        out.append((h, None, 0))
        out.append((h, None, 1))
        out.append((h, None, "hit"))                          # the room ends ON the hit sample: it is the last node that fits
        out.append((h, None, "before"))                       # the room ends on the accepted sample before the hit
    return out


def limit_of(case, max_commit, node_limit):
    """(max_commit, node_limit) of an entry of wave_cases.limit_cases as wave_commit takes them."""
    c = case.census()
    mc = case.W if max_commit is None else max_commit
    if node_limit == "hit":                                   # room for exactly the nodes up to the hit sample's own
        node_limit = c.N0 - 1 + int((c.length[:c.first_hit + 1] > 0).sum())
    elif node_limit == "before":                              # ... up to the accepted sample before the hit
        node_limit = c.N0 - 1 + int((c.length[:c.first_hit] > 0).sum())
    elif node_limit != -1:
        node_limit = c.N0 - 1 + int(node_limit)               # room = node_limit + 1 - N0
    return mc, node_limit


# ---------------------------------------------------------------------------------------------- sampler-driven lockstep
SCHEDULE = (1, 2, 3, 5, 63, 64, 65, 127, 129, 255, 256)          # off the controller's lattice (8..63, multiples of 64)
SCHEDULE_BIG = (257, 289, 1000)                                   # the TRI scan's waves, on a larger engine
LOCKSTEP = ("car", "boat_advanced", "pendulum", "double_integrator", "pendulum_lqr", "car_adaptive")


def lockstep_system(name):
    """A fresh system object that starts near its goal, so that goal hits cut waves often.  The pendulums get a goal box a
    sampler-driven run can hit at all (the demo's is 1 degree and 1 mrad/s wide); both sides are configured from this object."""
    base = "car" if name == "car_adaptive" else name
    mk = lqrrt_amd.systems.SYSTEMS[base]
    s = mk(n_boxes=50, seed=0) if base == "double_integrator" else mk(0)
    if base == "car":
        s.x0 = np.array([26.0, 40.0, np.pi / 2, 0, 0])
    elif base == "boat_advanced":
        s.x0 = np.array([34.0, 34.0, np.pi / 2, 0, 0, 0])
    elif base == "double_integrator":
        s.x0 = pt(12, 60, 60, 60)
    else:
        s.goal_buffer = [0.5, 0.5, 3.0, 3.0]
        s.x0 = np.array([np.pi / 2 - 0.45, -0.3, 0.5, 0])
    return s


def lockstep_limits(i, W, size):
    """(max_commit, node_limit) of wave i of a schedule: max_commit alternates between W and a value inside the wave; every third
    wave may add W // 4 + 1 nodes."""
    mc = W if i % 2 == 0 else max(1, (2 * W) // 3)
    nl = size + W // 4 if i % 3 == 2 else -1
    return mc, nl


def lockstep_horizon(name):
    return (0.1, 3) if name == "car_adaptive" else None


def lockstep_oracle(name, part, system=None):
    """(system, oracle, waves) of part 1 (SCHEDULE from the root) or 2 (200 iterations grown first, then SCHEDULE_BIG)."""
    import coracle
    s = lockstep_system(name) if system is None else system
    seed = (60 if name == "car_adaptive" else 0) + part
    o = coracle.make(s, 2600, seed=seed, horizon=lockstep_horizon(name))
    return s, o, seed, (SCHEDULE if part == 1 else SCHEDULE_BIG)


LOCKSTEP_GROWN = 200                                              # iterations before part 2's waves
