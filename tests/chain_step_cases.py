"""
Directed cases of one rollout step of the torque boat (test infrastructure; shared by tests/test_chain_step_cpu.py and
tests/test_chain_step_gpu.py): what the chain rollout of k_steer<BoatAdvanced> decides per step -- which arm of the heading
torque runs, which thruster saturates, which side of zero each velocity lies on, what the car-like rule does -- where its
horizon ends, and what the feasibility sweep finds around the hull.

A WORLD is a BoatAdvanced with a hull of V points and a table of O obstacles, its sequential C oracle and a tree of parents
(state, gain).  A batch is one resolution (H, FPR, adaptive; tol = 0, no goal) with W <= 64 (parent, target) pairs.  What every
pair must give comes from tests/steer_reference.py over the C oracle's single-call operators, never from the code under test.

Categories are assigned by CLASSIFY, from the reference's own trajectory: step k of a rollout is evaluated at state s_k-1 (the
parent, then the recorded states) and COUNTS when it leaves a mark in the outputs -- the state it produces is recorded, or it
is the step whose verdict ends the edge.  The predicates restate csrc/systems.hpp in plain Python floats (IEEE double, no
contraction: the device's comparisons bit for bit); where a category needs an elementary function (the torque that loads
the thrusters) it keeps a margin that libm's last bits cannot cross.  required() lists what must hold two cases per world.
"""
import collections
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import feasibility_reference as F                              # noqa: E402
import steer_cases as SC                                       # noqa: E402
import steer_reference as R                                    # noqa: E402

TAN_PI_8 = float.fromhex("0x1.a827999fcef32p-2")              # include/lqrrt_pmath.h LQ_TAN_PI_8
HS = (1, 2, 3)
FPRS = (0.5, 0.9, 1.0)
DT = 0.1
# (V, O) of the worlds: the flagship's 28 points / 36 obstacles; 33 points (past half a wavefront) with two cull tiles; 65
# points (two hull tiles) with one cull tile and with two
WORLDS = ((28, 36), (33, 65), (65, 36), (65, 65))

Batch = collections.namedtuple("Batch", "tag H FPR adaptive tol goal buf parents targets")


def up(v):
    return float(np.nextafter(v, np.inf))


def down(v):
    return float(np.nextafter(v, -np.inf))


# ---------------------------------------------------------------------------------------------------- hulls and tables

def lattice(xs, ys):
    gx, gy = np.meshgrid(np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64), indexing="ij")
    return np.ascontiguousarray(np.vstack((gx.ravel(), gy.ravel())))


def hull(V):
    """Body-frame hull points on binary fractions (0.5 m apart along the boat); None: the demo's own 28 points."""
    if V == 28:
        return None
    if V == 33:
        return lattice(np.arange(-2.5, 2.75, 0.5), (-1.0, 0.0, 1.0))
    assert V == 65
    return lattice(np.arange(-3.0, 3.25, 0.5), (-1.0, -0.5, 0.0, 0.5, 1.0))


# Sites of a directed table, 128 m apart along x (y = 0): at site n a boat at the site's centre, heading 0, has exactly n
# obstacles inside its cull box, pebbles of radius 1/16 m that lie between its hull points and touch none; the last row of
# the table is a buoy of radius 1 m in open water (site "buoy"), the one the threshold cases stand next to.  The rest of the
# table lies out of everybody's reach.
SITE_N = (1, 2, 3, 6)
SITE_X = {1: 128.0, 2: 256.0, 3: 384.0, 6: 512.0, "buoy": 640.0, "open": 768.0}
PEBBLE_R = 0.0625


def pebble_offsets(vps):
    """Body-frame places for pebbles: centres of the hull lattice's cells, nearest the hull's centre first."""
    xs, ys = np.unique(vps[0]), np.unique(vps[1])
    cx, cy = (xs[:-1] + xs[1:]) / 2, (ys[:-1] + ys[1:]) / 2
    cells = sorted(((x, y) for x in cx for y in cy), key=lambda c: (c[0] * c[0] + c[1] * c[1], c))
    return cells


def directed_table(vps, O):
    rows = []
    cells = pebble_offsets(vps)
    for n in SITE_N:
        rows += [(SITE_X[n] + bx, by, PEBBLE_R) for bx, by in cells[:n]]
    far = O - 1 - len(rows)
    assert far >= 0
    rows += [(2000.0 + 16.0 * i, 2000.0, 1.0) for i in range(far)]
    rows.append((SITE_X["buoy"], 0.0, 1.0))
    return np.array(rows, dtype=np.float64)


# ---------------------------------------------------------------------------------------------------- the step, restated

def wrap_libm(ang, h):
    """wrap_err(ang, h) with libm: the angle from heading h to direction ang."""
    c, s = math.cos(h), math.sin(h)
    return math.atan2(math.sin(ang) * c - math.cos(ang) * s, math.cos(ang) * c + math.sin(ang) * s)


def rudder_libm(rudder, vmin2, x):
    """BoatCommon::rudder_term with libm."""
    if x[3] >= 0.0 and x[3] * x[3] + x[4] * x[4] > vmin2:
        return rudder * math.atan2(x[4], x[3])
    c, s = math.cos(x[2]), math.sin(x[2])
    return rudder * wrap_libm(math.atan2(s * x[3] + c * x[4], c * x[3] - s * x[4]), x[2])


class Model(object):
    """The parameters of csrc/systems.hpp BoatAdvanced and its per-step predicates."""

    def __init__(self, s):
        self.P = P = np.asarray(s.params(), dtype=np.float64)
        self.invM, self.Dpos, self.Dneg = P[0:3], P[3:6], P[6:9]
        self.B, self.invB, self.tmax = P[9:21].reshape(3, 4), P[21:33].reshape(4, 3), P[33:37]
        self.rudder, self.vpos0, self.vneg0 = P[37], P[38], P[39]
        self.vmax, self.vmin, self.vmin2 = P[46:49], P[49:52], float(P[52])

    def direct(self, x):
        """torque_direct: the one-atan2 arm."""
        return bool(x[3] >= 0.0 and x[3] * x[3] + x[4] * x[4] > self.vmin2)

    def torque(self, x):
        """The heading torque with libm (categories that use it keep a margin)."""
        return rudder_libm(self.rudder, self.vmin2, x)

    def thrusts(self, x, u):
        """invB (u + torque) before the clip."""
        return self.invB.dot([u[0], u[1], u[2] + self.torque(x)])

    def surge_before_clamp(self, x, u):
        """xn[3] before `if (xn[3] < 0) xn[3] = 0` (libm's bits inside: compared with a margin)."""
        t = np.clip(self.thrusts(x, u), -self.tmax, self.tmax)
        us = self.B.dot(t)
        D = self.Dpos[0] if x[3] >= 0.0 else self.Dneg[0]
        return x[3] + self.invM[0] * (us[0] - D * x[3]) * DT

    def speed_ok(self, x):
        return not any(x[3 + i] > self.vmax[i] or x[3 + i] < self.vmin[i] for i in range(3))


def torque_labels(vmin2, x):
    """Which arm of BoatCommon::rudder_term runs at state x, and where inside lq_atan2 the one-atan2 arm lands."""
    out = set()
    vx, vy = float(x[3]), float(x[4])
    v2 = vx * vx + vy * vy
    if vx < 0.0:
        out.add("torque:vx<0")
    elif vx == 0.0 and vy == 0.0:
        out.add("torque:v=-0" if (math.copysign(1.0, vx) < 0 or math.copysign(1.0, vy) < 0) else "torque:v=+0")
    elif v2 <= vmin2:
        out.add("torque:slow")
        if v2 == vmin2:
            out.add("torque:on-vmin2")
    if vx >= 0.0 and v2 > vmin2:                               # torque_direct
        out.add("torque:direct")
        if v2 == up(vmin2):
            out.add("torque:vmin2+1ulp")
        ax, ay = abs(vx), abs(vy)
        if ay > ax:
            out.add("torque:|vy|>|vx|")
        t = (ax / ay) if ay > ax else (ay / ax)
        if t == TAN_PI_8:
            out.add("torque:t=tan(pi/8)")
        elif t == up(TAN_PI_8):
            out.add("torque:t=tan(pi/8)+1ulp")
        out.add("torque:t>tan(pi/8)" if t > TAN_PI_8 else "torque:t<=tan(pi/8)")
    else:
        out.add("torque:reference")
    return out


def thruster_labels(t, tmax):
    """One thruster beyond its limit alone, or none (1e-6 either side of the limit: libm's last bits cannot cross it)."""
    out = set()
    hi = [t[j] > tmax[j] * (1 + 1e-6) for j in range(4)]
    lo = [t[j] < -tmax[j] * (1 + 1e-6) for j in range(4)]
    inside = [abs(t[j]) < tmax[j] * (1 - 1e-6) for j in range(4)]
    for j in range(4):
        if (hi[j] or lo[j]) and all(inside[k] for k in range(4) if k != j):
            out.add("thruster%d:%s-alone" % (j, "upper" if hi[j] else "lower"))
    if all(inside):
        out.add("thrusters:none-saturated")
    return out


def drag_labels(x):
    return {"drag%d:%s" % (i, "v>=0" if x[3 + i] >= 0.0 else "v<0") for i in range(3)}


def carlike_labels(x):
    return {"carlike:x3>0" if x[3] > 0.0 else "carlike:x3<0" if x[3] < 0.0 else "carlike:x3==0"}


def step_labels(m, x, u):
    """Categories of ONE step evaluated at state x with effort u = K e."""
    out = torque_labels(m.vmin2, x)
    assert ("torque:direct" in out) == m.direct(x)
    # ---- lane rows: thrusters, drag, car-like rule
    out |= thruster_labels(m.thrusts(x, u), m.tmax)
    out |= drag_labels(x)
    out |= carlike_labels(x)
    return out


TORQUE_ARMS = ["torque:vx<0", "torque:v=+0", "torque:v=-0", "torque:slow", "torque:on-vmin2", "torque:vmin2+1ulp", "torque:direct",
               "torque:reference", "torque:|vy|>|vx|", "torque:t=tan(pi/8)", "torque:t=tan(pi/8)+1ulp", "torque:t>tan(pi/8)",
               "torque:t<=tan(pi/8)", "torque:arm-changes"]


def torque_seeds(vmin):
    """Body-frame velocities (v_x, v_y) that between them take every arm of TORQUE_ARMS (vmin: the system's torque_vmin)."""
    vmin2 = vmin * vmin
    seeds = [(-0.3, 0.1), (-0.5, -0.05), (-0.01, 0.3),                        # v_x < 0: only a seed state can have it
             (0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0),                 # atan2 of signed zeros
             (vmin, 0.0), (0.0, vmin), (vmin, -0.0), (0.0, -vmin),               # |v|^2 == vmin^2: the reference's sequence
             (0.005, 0.002), (0.002, -0.006),                                    # slower
             (0.5, TAN_PI_8 / 2), (0.25, -TAN_PI_8 / 4), (0.5, up(TAN_PI_8) / 2), (0.25, -up(TAN_PI_8) / 4),
             (0.5, 0.05), (0.1, 0.3), (0.05, -0.2), (0.3, 0.3), (0.2, up(0.2)),  # both sides of the fold, |v_y| > |v_x|
             (0.0, 0.2), (0.0, -0.1), (-0.0, 0.15)]                              # v_x = 0 with a sway: direct, car-like rule idle
    # |v|^2 one ulp above vmin^2: a sway v_y with fl(vmin^2 + v_y^2) = vmin^2 + 1 ulp
    ulp = up(vmin2) - vmin2
    for k in (0.75, 1.0, 1.25):
        for sign in (1.0, -1.0):
            vy = sign * math.sqrt(k * ulp)
            if vmin * vmin + vy * vy == up(vmin2):
                seeds.append((vmin, vy))
    return seeds


def required():
    req = list(TORQUE_ARMS)
    req += ["thruster%d:%s-alone" % (j, w) for j in range(4) for w in ("upper", "lower")]
    req += ["drag%d:%s" % (i, w) for i in range(3) for w in ("v>=0", "v<0")]
    req += ["carlike:x3>0", "carlike:x3<0", "carlike:x3==0", "carlike:clamped"]
    for H in HS:
        req += ["end:H%d:feasible" % H, "end:H%d:adaptive" % H] + ["end:H%d:infeasible/FPR%g" % (H, f) for f in FPRS]
    return req


def required_sweep(V, O):
    req = ["sweep:near=%s" % n for n in ("0", "1", "2", "3", ">4")]
    req += ["sweep:near-and-clear", "sweep:hit", "sweep:thr-1ulp", "sweep:thr", "sweep:thr+1ulp"]
    if O > 64:
        req += ["sweep:near-in-tile-2", "sweep:hit-in-tile-2"]
    if V > 64:
        req += ["sweep:hit-by-point>=64"]
    if V > 32:
        req += ["sweep:hit-by-point>=32"]
    return req


# ---------------------------------------------------------------------------------------------------- worlds

Case = collections.namedtuple("Case", "pid target H FPR adaptive rollout labels")


class WorldBase(object):
    """What every world of directed step cases shares (tests/packed_step_cases.py builds its worlds on it too): a system `s` of
    the planar boats, its C oracle, the tree of parents, the case list with its coverage count, and the batches.  A subclass sets
    `name`, `ident` (what plain() hands a child process to find the world again), `m` (its restated model: speed_ok) and
    `required`, and provides classify() and _build()."""

    def _open(self, s):
        self.s = s
        self.n, self.m_ = s.nstates, s.ncontrols
        self.o = SC.make_oracle(s, 4096)
        self.ops = R.coracle_ops(self.o, DT)
        self.geo = F.CircleGeo(s.vps, s.obs) if len(s.obs) else None
        self.states, self.K = [np.array(s.x0, dtype=np.float64)], [self.o.gain(s.x0, np.zeros(3))]
        self.cases = []
        self.coverage = collections.Counter()

    def _close(self):
        self.states, self.K = np.array(self.states), np.array(self.K)
        self.pID = np.arange(len(self.states), dtype=np.int32) - 1
        self.batches, self.batch_cases = self._batches()

    # -- the reference and its classification ---------------------------------------------------------------------------
    def gain(self, x):
        return self.o.gain(x, np.zeros(3))

    def sweep_labels(self, x):
        """What hull_hits meets at state x (empty when the speed box ends the test before it)."""
        if self.geo is None or not self.m.speed_ok(x):
            return set(), None
        g = self.geo
        c, s = F.portable_sincos(float(x[2]))
        near = F.circle_near(g, x, c, s)
        n = int(near.sum())
        out = {"sweep:near=%s" % (n if n <= 3 else ">4" if n > 4 else "4")}
        verts = F.vertices(self.s.vps, x, c, s)
        hits = []                                              # (obstacle, hull point)
        d2s = []
        for o in np.nonzero(near)[0]:
            dx, dy = verts[:, 0] - g.oc[o, 0], verts[:, 1] - g.oc[o, 1]
            d2 = dx * dx + dy * dy
            hits += [(int(o), int(v)) for v in np.nonzero(d2 <= g.oc[o, 2])[0]]
            d2s.append((d2, g.oc[o, 2]))
        if hits:
            out.add("sweep:hit")
            if all(o >= 64 for o, _ in hits):
                out.add("sweep:hit-in-tile-2")
            if all(v >= 64 for _, v in hits):
                out.add("sweep:hit-by-point>=64")
            if all(v >= 32 for _, v in hits):
                out.add("sweep:hit-by-point>=32")
        elif n:
            out.add("sweep:near-and-clear")
        if near[64:].any():
            out.add("sweep:near-in-tile-2")
        for d2, thr in d2s:
            if np.any(d2 == thr):
                out.add("sweep:thr")
            if np.any(d2 == down(thr)):
                out.add("sweep:thr-1ulp")
            if np.any(d2 == up(thr)) and not hits:
                out.add("sweep:thr+1ulp")
        return out, not hits

    def offer(self, x, K, xt, H=2, FPR=0.9, adaptive=False, keep=False):
        """Rolls the pair out with the reference; it becomes a case if it is the first or second of a required category (or keep)."""
        x, K, xt = (np.array(a, dtype=np.float64) for a in (x, K, xt))
        # (no goal is set: engine.py set_resolution then takes the box (-inf, inf), and every node lies inside)
        r = R.steer(self.ops, x, K, xt, DT, FPR, H, np.zeros(self.n), adaptive, np.full(self.n, -np.inf), np.full(self.n, np.inf))
        labels = self.classify(x, K, xt, H, FPR, adaptive, r)
        new = [c for c in labels if c in self.required and self.coverage[c] < 2]
        if not (new or keep):
            return False
        self.states.append(x)
        self.K.append(K)
        self.cases.append(self.case_of(len(self.states) - 1, xt, H, FPR, adaptive, r, labels))
        self.coverage.update(labels)
        return True

    def case_of(self, pid, xt, H, FPR, adaptive, r, labels):
        return Case(pid, xt, H, FPR, adaptive, r, labels)

    def aim(self, x, u0, u1):
        """A target whose error asks the parent's own gain for the body-frame force (u0, u1), roughly."""
        x = np.asarray(x, dtype=np.float64)
        c, s = math.cos(x[2]), math.sin(x[2])
        kp = np.diag(self.s.kp)
        eb = (u0 / kp[0], u1 / kp[1])
        xt = x.copy()
        xt[0] += c * eb[0] - s * eb[1]
        xt[1] += s * eb[0] + c * eb[1]
        return xt

    def _batches(self):
        groups = collections.OrderedDict()
        for c in self.cases:
            groups.setdefault((c.H, c.FPR, c.adaptive), []).append(c)
        batches, members = [], []
        for (H, FPR, adaptive), cs in groups.items():
            for i in range(0, len(cs), 64):
                part = cs[i:i + 64]
                batches.append(Batch("%s/H%d/FPR%g/%d" % (self.name, H, FPR, adaptive), H, FPR, adaptive, np.zeros(self.n), None, None,
                                     np.array([c.pid for c in part], dtype=np.int32), np.array([c.target for c in part])))
                members.append(part)
        return batches, members

    def expected_arrays(self, bi):
        b, rs = self.batches[bi], [c.rollout for c in self.batch_cases[bi]]
        W, n, m = len(rs), self.n, self.m_
        ln = np.array([len(r.xs) for r in rs], dtype=np.int32)
        xseq, useq = np.zeros((W, b.H, n)), np.zeros((W, b.H, m))
        xend, Kend = np.zeros((W, n)), np.zeros((W, m, n))
        for t, r in enumerate(rs):
            xseq[t, :ln[t]], useq[t, :ln[t]] = r.xs, r.us
            if ln[t]:
                xend[t], Kend[t] = r.xs[-1], r.K_end
        return dict(len=ln, xseq=xseq, useq=useq, xend=xend, Kend=Kend, goal=np.array([int(r.in_goal) for r in rs]),
                    grew=np.array([int(r.reason[0] == "grew") for r in rs]), steps=np.array([r.steps for r in rs]))

    def plain(self):
        """What a child process needs to run the batches (tests/test_steer_gpu.py run_batches)."""
        return dict(self.ident, dt=DT, states=self.states, K=self.K, pID=self.pID,
                    batches=[dict(H=b.H, FPR=b.FPR, adaptive=b.adaptive, tol=b.tol, goal=b.goal, buf=b.buf, parents=b.parents,
                                  targets=b.targets) for b in self.batches])


class World(WorldBase):
    """kind "demo": demo_boat_advanced's own obstacle field; "directed": directed_table() with the buoy moved to the origin,
    where a hull point's distance to it resolves to one ulp of the squared threshold."""

    def __init__(self, kind, V, O):
        import lqrrt_amd
        self.kind, self.V, self.O = kind, V, O
        self.name = "%s-V%d-O%d" % (kind, V, O)
        self.ident = dict(kind=kind, V=V, O=O)
        s = lqrrt_amd.systems.BoatAdvanced(0)
        if hull(V) is not None:
            s.vps = hull(V)
        if kind == "directed":
            table = directed_table(s.vps, O)
            table[-1, :2] = 0.0
            s.set_obstacles(table)
        assert s.vps.shape[1] == V and len(s.obs) == O, (s.vps.shape, len(s.obs))
        self._open(s)
        self.m = Model(s)
        self.required = (required() if kind == "demo" else []) + self.required_sweep()
        self._build()
        self._close()

    def required_sweep(self):
        if self.kind == "demo":                                # (centimetre coordinates tens of metres out: no one-ulp cases there)
            return ["sweep:near=0", "sweep:near=1", "sweep:near-and-clear", "sweep:hit"]
        return required_sweep(self.V, self.O)

    def classify(self, x0, K0, xt, H, FPR, adaptive, r):
        m, labels = self.m, set()
        xt = np.asarray(xt, dtype=np.float64)
        x, K = np.asarray(x0, dtype=np.float64), np.asarray(K0, dtype=np.float64)
        arms = set()
        for k in range(1, len(r.xall) + 1):
            u = R.effort(K, self.ops.erf(xt, x))
            xn = r.xall[k - 1]
            if k <= len(r.xs):                                 # the step's arithmetic is in the outputs
                st = step_labels(m, x, u)
                if xn[3] == 0.0 and m.surge_before_clamp(x, u) < -1e-9:
                    st.add("carlike:clamped")
                arms.add("torque:direct" in st)
                labels |= st
            sw, clear = self.sweep_labels(xn)                  # the verdict on every evaluated state is in the outputs
            labels |= sw
            if clear is not None:                              # the restated sweep and the oracle agree
                assert clear == self.ops.feasible(xn, u), (self.name, xn)
            x, K = xn, (self.o.gain(xn, u) if k < len(r.xall) else K)
        if len(arms) == 2:
            labels.add("torque:arm-changes")
        if H in HS:
            if r.reason == ("horizon", H + 1):
                labels.add("end:H%d:%s" % (H, "adaptive" if adaptive else "feasible"))
            if r.reason == ("infeasible", H + 1) and not adaptive and FPR in FPRS:
                labels.add("end:H%d:infeasible/FPR%g" % (H, FPR))
        return labels

    # -- construction ---------------------------------------------------------------------------------------------------
    def _build(self):
        if self.kind == "demo":
            self._torque_arm()
            self._lane_rows()
            self._horizon_end()
            self._natural()
        else:
            self._sites()
            self._buoy()

    def _moving(self, pos, h, vx, vy, vh=0.0):
        return np.array([pos[0], pos[1], h, vx, vy, vh])

    OPEN = (-20.0, -20.0)                                      # demo world: 35 m from the nearest obstacle

    def _torque_arm(self):
        vmin = self.s.torque_vmin
        assert vmin * vmin == self.m.vmin2
        seeds = torque_seeds(vmin)
        for i, (vx, vy) in enumerate(seeds):
            for h in (0.0, 0.7, -2.5):
                x = self._moving(self.OPEN, h, vx, vy, 0.05 * ((i % 3) - 1))
                for f in ((200.0, 10.0), (-150.0, -20.0)):
                    self.offer(x, self.gain(x), self.aim(x, *f), H=3)
                    if vx < 0.0:                               # (the torque of a boat that backs up soon makes a step infeasible:
                        self.offer(x, self.gain(x), self.aim(x, *f), H=3, FPR=1.0)      # only FPR = 1 keeps the steps before it)

    def _lane_rows(self):
        """One thruster saturating alone: the force the target asks for and the torque of the sway are searched over a seeded
        box; a stopping boat for the clamp of a negative surge; every sign of every velocity."""
        rs = np.random.RandomState(3)
        want = ["thruster%d:%s-alone" % (j, w) for j in range(4) for w in ("upper", "lower")]
        for _ in range(4000):
            if all(self.coverage[c] >= 2 for c in want):
                break
            u0, u1, M = rs.uniform(-900, 900), rs.uniform(-900, 900), rs.uniform(-1500, 1500)
            t = self.m.invB.dot([u0, u1, M])
            a = np.sort(np.abs(t))
            if not (a[3] > 1.05 * self.m.tmax[0] and a[2] < 0.9 * self.m.tmax[0]):
                continue
            vx = 0.5
            x = self._moving(self.OPEN, rs.choice([0.0, 1.1]), vx, vx * math.tan(M / self.m.rudder), 0.0)
            self.offer(x, self.gain(x), self.aim(x, u0, u1), H=2)
        for vx, vy, vh, f in ((0.02, 0.0, 0.0, -800.0), (0.01, 0.05, -0.1, -600.0), (0.0, 0.0, 0.0, -500.0), (0.3, -0.2, -0.15, 100.0),
                              (0.4, 0.1, 0.1, 50.0), (-0.2, -0.1, -0.1, 300.0), (-0.4, 0.2, 0.1, 400.0), (0.6, -0.3, 0.15, 0.0)):
            for h in (0.0, 2.0):
                x = self._moving(self.OPEN, h, vx, vy, vh)
                self.offer(x, self.gain(x), self.aim(x, f, 5.0), H=3)

    def _horizon_end(self):
        """Rollouts that end on step H + 1: feasible there (the horizon, fixed and adaptive) and infeasible there under every
        FPR -- parents on the trajectory of a seed pair of tests/steer_cases.py whose first infeasible step comes late."""
        c = SC.cases("boat_advanced")
        assert np.array_equal(c.s.params(), self.s.params()) and np.array_equal(c.s.obs, self.s.obs)
        for H in HS:
            for i in sorted(c.inf_at, key=lambda i: (-min(c.inf_at[i], 9), i))[:4]:
                j = c.inf_at[i] - (H + 1)
                if j < 0:
                    continue
                tr = c.trace[i]
                x, K = (c.spar[i], c.sK[i]) if j == 0 else (tr.xs[j - 1], c.o.gain(tr.xs[j - 1], tr.us[j - 1]))
                for FPR in FPRS:
                    self.offer(x, K, c.star[i], H=H, FPR=FPR)
            for i in c.clean_all[:6]:
                for adaptive in (False, True):
                    self.offer(c.spar[i], c.sK[i], c.star[i], H=H, adaptive=adaptive)

    def _natural(self):
        """Seed pairs of the demo's sample space as they come: obstacles met on the way."""
        c = SC.cases("boat_advanced")
        for i in range(len(c.spar)):
            if all(self.coverage[k] >= 2 for k in self.required_sweep()):
                break
            self.offer(c.spar[i], c.sK[i], c.star[i], H=3)

    def _sites(self):
        zero = np.zeros((3, 6))
        for key in ("open",) + SITE_N:
            X = SITE_X[key]
            for h in (0.0, 0.0625):
                x = self._moving((X, 0.0), h, 0.0, 0.0)
                self.offer(x, zero, x + [1.0, 0, 0, 0, 0, 0], H=2)                     # the pose itself is swept: u = 0, v = 0
                x = self._moving((X - 0.125, 0.0), h, 0.5, 0.0)
                self.offer(x, self.gain(x), x + [3.0, 0, 0, 0, 0, 0], H=3)             # ... and poses on the way across the site

    def _buoy(self):
        """The hull's last point (its +x +y corner, heading 0) beside the buoy at the origin: on the threshold of the squared
        distance, one ulp inside and one ulp outside -- searched over a few ulps of the pose."""
        zero = np.zeros((3, 6))
        bx, by = self.s.vps[0, -1], self.s.vps[1, -1]
        assert bx == self.s.vps[0].max() and by == self.s.vps[1].max()
        ulp = 2.0 ** -52
        px0 = -1.0 - bx
        for kx in (0, 1, -1, 2, -2, 3, -3):
            px = px0
            for _ in range(abs(kx)):
                px = up(px) if kx > 0 else down(px)
            for k in (0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0):
                for sign in (1.0, -1.0):
                    x = self._moving((px, -by + sign * math.sqrt(k * ulp)), 0.0, 0.0, 0.0)
                    self.offer(x, zero, x + [-1.0, 0, 0, 0, 0, 0], H=2)
        # deeper in and well clear
        for d in (0.5, 0.99, 1.01, 1.5):
            x = self._moving((-d - bx, -by), 0.0, 0.0, 0.0)
            self.offer(x, zero, x + [-1.0, 0, 0, 0, 0, 0], H=2, keep=True)


_CACHE = {}
KINDS = (("demo", 28, 36), ("directed", 28, 36)) + tuple(("directed", V, O) for V, O in WORLDS[1:])


def world(kind, V, O):
    key = (kind, V, O)
    if key not in _CACHE:
        _CACHE[key] = World(kind, V, O)
    return _CACHE[key]
