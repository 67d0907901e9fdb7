"""
Directed cases of one rollout step of the ROS boat and of the intermediate boat (test infrastructure; shared by
tests/test_packed_step_cpu.py and tests/test_packed_step_gpu.py): what csrc/systems.hpp RosBoat and BoatIntermediate decide per
step -- RosBoat's heading mode (P[38]: none, stare at a focus point, along the velocity), its saturation rule (P[41]: even
down-scaling with its `any ratio < 1` test and 1e-6 floor, or per-thruster clip) and its no-reverse rule (P[42]); the
intermediate boat's per-axis saturation on |u| == u_max and its branching car-like rule -- and where a rollout's horizon ends.

A WORLD (SPECS) is one of those systems with an obstacle table, its sequential C oracle and a tree of parents (state, gain); the
machinery is tests/chain_step_cases.py WorldBase.  What every (parent, target) pair must give comes from
tests/steer_reference.py over the C oracle's single-call operators, never from the code under test.  A gain of the tree need not
be the system's own: K = a single 1.0 makes u = K e one error component exactly, K = 0 makes u = 0 with e != 0; the rollout takes
such a gain for its first step and the system's own from then on.

Categories are assigned from the reference's trajectory by predicates restated in plain Python floats from s.params(), with the
device's left-to-right sums.  Categories that compare for equality ("sat0:on-limit", "axis0:=+umax", ...) are only assigned where
no elementary function feeds the compared value (heading mode 0; the intermediate boat's axes 0 and 1, and its axis 2 where the
torque is exactly zero); where one does, the category keeps a margin of 1e-6 of the limit (1e-9 m/s on a surge) that libm's last
bits cannot cross.  A step COUNTS when the state it produces is recorded.  required(key) lists what must hold two cases.

No category was dropped as unreachable.  Two exist because the plain ones cannot show a wrong predicate:
  * "sat0:on-limit:B.t!=u": a boat at rest asked for a pure surge force puts all four thrusts on 220 N, but there B t equals u
    bit for bit and a remap at ratio == 1.0 would go unseen; with a sway force as well one thrust is on its limit and B t is
    not u.
  * "sat0:floor-binds": with the shipped thrust limit (220 N) the 1e-6 floor of the ratio's divisor can never decide a step (a
    ratio it changes is >= 2.2e8 either way), so a world with a limit of 1e-7 N, below the floor, is where the floor alone
    switches the remap on.
The intermediate boat's `fabs(u) > u_max` has no such case: on |u| == u_max the saturated value u_max * (+-1.0) is u itself, so
`>` and `>=` give the same bits; "axis*:=+-umax" and their one-ulp twins pin the value on either side of the comparison.
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

import chain_step_cases as CC                                  # noqa: E402
import steer_cases as SC                                       # noqa: E402
import steer_reference as R                                    # noqa: E402
from chain_step_cases import DT, HS, down, up                  # noqa: E402

FPRS = (0.0, 0.5, 0.9, 1.0)                                    # 0: the ROS setting, an infeasible step cuts the edge to nothing
ATOL = 1e-9                                                    # tests/test_ros_behaviors.py, tests/test_hip_parity.py
MAX_CASES = 128

# steps: every evaluated step of the rollout, the last (unrecorded) one included, as (state, effort u = K e, labels); the
# labels of a step that left no recorded state are empty
Case = collections.namedtuple("Case", "pid target H FPR adaptive rollout labels steps")

# key -> the system.  behavior / focus: RosBoat's constructor; cross: instance attributes set before the engine and the oracle
# are built (both read the same params()); table: "grid" = the obstacle grid of steer_cases.make_system("ros_boat"), "none" = an
# empty table (RosBoat: `g.O == 0 -> feasible`), "demo" = the demo's own
SPECS = collections.OrderedDict([
    ("boat", dict(behavior="boat", table="grid")),                                           # mode 0, sat 0
    ("stare", dict(behavior="boat", focus=(-0.0, -0.0), table="grid")),                      # mode 1, sat 0
    ("stare-far", dict(behavior="boat", focus=(1e6, 3e5), table="grid")),
    ("car", dict(behavior="car", table="grid")),                                             # mode 2, sat 1, no-reverse
    ("escape", dict(behavior="escape", table="grid")),                                       # mode 0, rudder gain 0
    ("stare-clip", dict(behavior="boat", focus=(-0.0, -0.0), table="grid", cross=dict(sat_mode=1, no_reverse=1))),
    ("velocity-scale", dict(behavior="car", table="grid", cross=dict(sat_mode=0, no_reverse=0))),
    ("empty", dict(behavior="boat", table="none")),
    ("floor", dict(behavior="boat", table="grid", cross=dict(thrust_max=np.full(4, 1e-7)))),
    ("intermediate", dict(table="demo")),
])
KEYS = tuple(SPECS)


def make_system(key):
    import lqrrt_amd
    spec = SPECS[key]
    if key == "intermediate":
        return lqrrt_amd.systems.BoatIntermediate(0)
    s = lqrrt_amd.systems.RosBoat(spec["behavior"], focus=spec.get("focus"))
    for k, v in spec.get("cross", {}).items():
        assert hasattr(s, k)
        setattr(s, k, v)
    if spec["table"] == "grid":
        s.set_obstacles(SC.make_system("ros_boat").obs)
    return s


def make_np_system(key):
    """The NumPy port of the reference's behaviour (oracle/systems_np.py) for the same world."""
    import systems_np
    spec = SPECS[key]
    if key == "intermediate":
        return systems_np.BoatIntermediate(0)
    s = systems_np.RosBoat(spec["behavior"], focus=spec.get("focus"))
    for k, v in spec.get("cross", {}).items():
        assert hasattr(s, k)
        setattr(s, k, v)
    return s


def sgn(v):
    return "-" if math.copysign(1.0, v) < 0 else "+"


def dot3(a, b):
    """a . b summed left to right."""
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


# ---------------------------------------------------------------------------------------------------- the steps, restated

class RosModel(object):
    """The parameters of csrc/systems.hpp RosBoat and its per-step predicates."""

    def __init__(self, s):
        self.P = P = np.asarray(s.params(), dtype=np.float64)
        self.invM, self.Dpos, self.Dneg = P[0:3], P[3:6], P[6:9]
        self.B, self.invB, self.tmax = P[9:21].reshape(3, 4), P[21:33].reshape(4, 3), P[33:37]
        self.rudder, self.mode, self.focus = float(P[37]), int(P[38]), (float(P[39]), float(P[40]))
        self.sat, self.norev, self.vmin2 = int(P[41]), int(P[42]), float(P[49])
        self.exact = self.mode == 0                            # no elementary function between u = K e and the thrusts

    def speed_ok(self, x):
        return True

    def yaw(self, x, u):
        """The yaw effort the step integrates: u[2] itself (mode 0) or what REPLACES it (with libm)."""
        if self.mode == 1:
            return self.rudder * CC.wrap_libm(math.atan2(self.focus[1] - x[1], self.focus[0] - x[0]), x[2])
        if self.mode == 2:
            return CC.rudder_libm(self.rudder, self.vmin2, x)
        return float(u[2])

    def thrusts(self, x, u):
        w = (float(u[0]), float(u[1]), self.yaw(x, u))
        return [dot3(self.invB[j], w) for j in range(4)], w

    def ratios(self, t):
        return [self.tmax[j] / max(abs(t[j]), 1e-6) for j in range(4)]

    def surge(self, x, u):
        """xn[3] before the no-reverse rule."""
        t, w = self.thrusts(x, u)
        us0 = w[0]
        if self.sat == 0:
            r = self.ratios(t)
            if any(v < 1.0 for v in r):
                t = [min(r) * v for v in t]
                us0 = None
        else:
            t = [min(max(t[j], -self.tmax[j]), self.tmax[j]) for j in range(4)]
            us0 = None
        if us0 is None:
            us0 = ((self.B[0, 0] * t[0] + self.B[0, 1] * t[1]) + self.B[0, 2] * t[2]) + self.B[0, 3] * t[3]
        D = self.Dpos[0] if x[3] >= 0.0 else self.Dneg[0]
        return float(x[3] + (self.invM[0] * (us0 - D * x[3])) * DT)

    def labels(self, x, u, xn):
        out = CC.drag_labels(x)
        # ---- heading: a yaw effort K e that add-versus-replace would show (the torques are thousands of N m)
        if abs(u[2]) > 1.0:
            out.add("heading:Ke-used" if self.mode == 0 else "heading:Ke-replaced")
        if self.mode == 1:
            yb, xb = self.focus[1] - x[1], self.focus[0] - x[0]
            if yb == 0.0 and xb == 0.0:
                out.add("focus:on-boat(yb=%s0,xb=%s0)" % (sgn(yb), sgn(xb)))
            elif yb == 0.0 and xb < 0.0:
                out.add("focus:astern(yb=%s0)" % sgn(yb))
            else:
                b = CC.wrap_libm(math.atan2(yb, xb), x[2])
                if abs(b) < 0.2:
                    out.add("focus:ahead")
                if abs(abs(b) - math.pi / 2) < 0.2:
                    out.add("focus:abeam")
            if math.hypot(yb, xb) >= 1e6:
                out.add("focus:far")
        if self.mode == 2:
            out |= CC.torque_labels(self.vmin2, x)
        # ---- saturation
        t, _ = self.thrusts(x, u)
        above = [abs(t[j]) > self.tmax[j] * (1 + 1e-6) for j in range(4)]
        inside = [abs(t[j]) < self.tmax[j] * (1 - 1e-6) for j in range(4)]
        if self.sat == 0:
            r = self.ratios(t)
            any_, rmin = any(v < 1.0 for v in r), min(r)
            if all(inside) and not any_:
                out.add("sat0:no-ratio<1")
            if any(above):
                out.add("sat0:remap")
            if sum(above) == 1 and sum(inside) == 3:
                out.add("sat0:one-alone")
            if all(above):
                out.add("sat0:all-four")
            if self.exact:
                if not any_ and any(abs(t[j]) == self.tmax[j] for j in range(4)):
                    out.add("sat0:on-limit")                   # ratio == 1.0: still the step integrates u itself
                    bt = [((self.B[i, 0] * t[0] + self.B[i, 1] * t[1]) + self.B[i, 2] * t[2]) + self.B[i, 3] * t[3] for i in range(3)]
                    if any(float(bt[i]) != float(u[i]) for i in range(3)):
                        out.add("sat0:on-limit:B.t!=u")        # ... and a remap (by the ratio 1.0) would show in its bits
                if any_ and max(abs(t[j]) - up(self.tmax[j]) for j in range(4)) == 0.0:
                    out.add("sat0:limit+1ulp")
                if any_ and sum(v == rmin for v in r) >= 2:
                    out.add("sat0:tie")
                if any(0.0 < abs(v) < 1e-6 for v in t):
                    out.add("sat0:floor")
                if any(v == 0.0 for v in t):
                    out.add("sat0:t=0")
                if any_ and all(abs(t[j]) <= self.tmax[j] for j in range(4)):
                    out.add("sat0:floor-binds")                # no thrust beyond its limit: the ratio's floor alone remaps
        else:
            out |= CC.thruster_labels(t, self.tmax)
            if any(above):
                out.add("sat1:clipped")
        # ---- no-reverse
        pre = self.surge(x, u)
        if abs(pre) <= ATOL:                                   # libm decides whether the rule fires: no category ...
            if self.norev and abs(x[3]) > ATOL:                # ... and where firing moves the surge by more than that, not
                out.add("surge:near-zero")                     # for the NumPy port either
        elif self.norev:
            if pre < 0.0:
                assert xn[3] == abs(x[3]), (x, u, xn)
                out.add("norev:fires-from-forward" if x[3] > 0.0 else "norev:fires-from-x3<0" if x[3] < 0.0 else "norev:x3=%s0" % sgn(x[3]))
            else:
                out.add("norev:idle")
        elif pre < 0.0:
            assert xn[3] < 0.0, (x, u, xn)
            out.add("norev-off:negative-kept")
        return out


class IntModel(object):
    """The parameters of csrc/systems.hpp BoatIntermediate and its per-step predicates."""

    def __init__(self, s):
        self.P = P = np.asarray(s.params(), dtype=np.float64)
        self.invM, self.Dpos, self.Dneg, self.umax = P[0:3], P[3:6], P[6:9], P[9:12]
        self.rudder, self.vpos0, self.vneg0, self.vmin2 = float(P[12]), float(P[13]), float(P[14]), float(P[21])

    def speed_ok(self, x):
        return True

    def labels(self, x, u, xn):
        out = CC.torque_labels(self.vmin2, x) | CC.drag_labels(x) | CC.carlike_labels(x)
        um = self.umax
        for i in (0, 1):                                       # u[i] = K e alone: compared for equality
            v = float(u[i])
            if abs(v) < 0.5 * um[i]:
                out.add("axis%d:inside" % i)
            for name, ref in (("=+umax", um[i]), ("+umax+1ulp", up(um[i])), ("=-umax", -um[i]), ("-umax-1ulp", down(-um[i]))):
                if v == ref:
                    out.add("axis%d:%s" % (i, name))
        tq = CC.rudder_libm(self.rudder, self.vmin2, x)
        w2 = float(u[2]) + tq
        if w2 > um[2] * (1 + 1e-6):
            out.add("axis2:upper")
        if w2 < -um[2] * (1 + 1e-6):
            out.add("axis2:lower")
        if "torque:direct" in out and x[4] == 0.0:             # atan2(+-0, v_x > 0) = +-0: the torque adds nothing to u[2]
            assert tq == 0.0
            if u[2] == um[2]:
                out.add("axis2:=+umax")
            if u[2] == up(um[2]):
                out.add("axis2:+umax+1ulp")
        # ---- the car-like rule on the surge (axis 0 has no elementary function in it)
        us0 = float(u[0])
        if abs(us0) > um[0]:
            us0 = um[0] * (1.0 if us0 > 0.0 else -1.0)
        D = self.Dpos[0] if x[3] >= 0.0 else self.Dneg[0]
        pre = float(x[3] + (self.invM[0] * (us0 - D * x[3])) * DT)
        if x[3] != 0.0:
            q = abs(pre / (self.vpos0 if x[3] > 0.0 else self.vneg0))
            if q > 1 + 1e-9:
                out.add("carlike:scale-clipped")
            if q < 1 - 1e-9:
                out.add("carlike:scale<1")
        if pre < -ATOL:
            assert xn[3] == 0.0, (x, u, xn)
            out.add("carlike:clamped")
        return out


# ---------------------------------------------------------------------------------------------------- what must be there

ENDS = [e for H in HS for e in ["end:H%d:feasible" % H, "end:H%d:adaptive" % H] + ["end:H%d:infeasible/FPR%g" % (H, f) for f in FPRS]]
DRAG = ["drag%d:%s" % (i, w) for i in range(3) for w in ("v>=0", "v<0")]
SWEEP = ["sweep:hit", "sweep:near-and-clear"]
ALONE = ["thruster%d:%s-alone" % (j, w) for j in range(4) for w in ("upper", "lower")]
NOREV = ["norev:fires-from-forward", "norev:fires-from-x3<0", "norev:x3=+0", "norev:x3=-0", "norev:idle"]
ON_BOAT = ["focus:on-boat(yb=%s0,xb=%s0)" % (a, b) for a in "+-" for b in "+-"]
ASTERN = ["focus:astern(yb=+0)", "focus:astern(yb=-0)"]
SAT0_EXACT = ["sat0:no-ratio<1", "sat0:on-limit", "sat0:on-limit:B.t!=u", "sat0:limit+1ulp", "sat0:one-alone", "sat0:all-four", "sat0:tie", "sat0:floor", "sat0:t=0"]

REQUIRED = {
    "boat": ["heading:Ke-used"] + SAT0_EXACT + ["norev-off:negative-kept"] + DRAG + ENDS + SWEEP,
    "stare": ["heading:Ke-replaced", "focus:ahead", "focus:abeam"] + ASTERN + ON_BOAT + ["sat0:no-ratio<1", "sat0:remap"] + DRAG + SWEEP,
    "stare-far": ["heading:Ke-replaced", "focus:far"] + SWEEP,
    "car": ["heading:Ke-replaced"] + CC.TORQUE_ARMS + ALONE + ["thrusters:none-saturated"] + NOREV + DRAG + SWEEP,
    "escape": ["heading:Ke-used", "sat0:no-ratio<1", "sat0:remap"] + SWEEP,
    "stare-clip": ["heading:Ke-replaced", "focus:ahead", "focus:abeam", "sat1:clipped", "thrusters:none-saturated",
                   "norev:fires-from-forward", "norev:idle"] + SWEEP,
    "velocity-scale": ["heading:Ke-replaced", "torque:direct", "torque:reference", "torque:arm-changes", "sat0:no-ratio<1", "sat0:remap",
                       "norev-off:negative-kept"] + SWEEP,
    "empty": ["heading:Ke-used", "empty:through-obstacle"],
    "floor": ["sat0:floor-binds", "sat0:remap"],
    "intermediate": CC.TORQUE_ARMS + ["axis%d:%s" % (i, w) for i in (0, 1) for w in ("inside", "=+umax", "+umax+1ulp", "=-umax", "-umax-1ulp")]
    + ["axis2:upper", "axis2:lower", "axis2:=+umax", "axis2:+umax+1ulp", "carlike:x3>0", "carlike:x3<0", "carlike:x3==0",
       "carlike:scale-clipped", "carlike:scale<1", "carlike:clamped"] + DRAG + ENDS + SWEEP,
}

# Labels that put a libm result on a threshold: the only ones whose steps the comparison with the NumPy port may leave out -- a
# surge within 1e-9 of zero before a no-reverse rule that would move it by more than that.  The torque's own thresholds
# (|v|^2 on vmin^2, |v_y| / |v_x| on tan(pi/8)) are not among them: the first is decided without libm and both forms of the
# torque agree to rounding either side of it, the second lies inside lq_atan2, where the port has no fold.
LIBM_THRESHOLD = ("surge:near-zero",)


def required(key):
    return REQUIRED[key]


# ---------------------------------------------------------------------------------------------------- worlds

class World(CC.WorldBase):
    def __init__(self, key):
        self.key, self.name, self.ident = key, key, dict(key=key)
        self._open(make_system(key))
        self.m = IntModel(self.s) if key == "intermediate" else RosModel(self.s)
        self.required = required(key)
        self.open = (-20.0, -20.0) if key == "intermediate" else (0.25, 0.125)   # no obstacle within reach of the hull, any heading
        self.seeds = SC.cases("boat_intermediate" if key == "intermediate" else "ros_boat")
        self._build()
        self._close()

    # -- the reference and its classification ---------------------------------------------------------------------------
    def classify(self, x0, K0, xt, H, FPR, adaptive, r):
        labels, steps, arms = set(), [], set()
        xt = np.asarray(xt, dtype=np.float64)
        x, K = np.asarray(x0, dtype=np.float64), np.asarray(K0, dtype=np.float64)
        through = False
        for k in range(1, len(r.xall) + 1):
            u = R.effort(K, self.ops.erf(xt, x))
            xn = r.xall[k - 1]
            st = set()
            if k <= len(r.xs):                                 # the step's arithmetic is in the outputs
                st = self.m.labels(x, u, xn)
                if "torque:direct" in st or "torque:reference" in st:
                    arms.add("torque:direct" in st)
                labels |= st
            steps.append((x, u, st))
            sw, clear = self.sweep_labels(xn)                  # the verdict on every evaluated state is in the outputs
            labels |= {c for c in sw if c in SWEEP}
            if clear is not None:                              # the restated sweep and the oracle agree
                assert clear == self.ops.feasible(xn, u), (self.name, xn)
            if self.key == "empty" and k <= len(r.xs) and not world("boat").ops.feasible(xn, u):
                through = True                                 # recorded here, inside an obstacle of the world that has them
            x, K = xn, (self.o.gain(xn, u) if k < len(r.xall) else K)
        if through:
            labels.add("empty:through-obstacle")
        if len(arms) == 2:
            labels.add("torque:arm-changes")
        if H in HS:
            if r.reason == ("horizon", H + 1):
                labels.add("end:H%d:%s" % (H, "adaptive" if adaptive else "feasible"))
            if r.reason == ("infeasible", H + 1) and not adaptive and FPR in FPRS:
                labels.add("end:H%d:infeasible/FPR%g" % (H, FPR))
        self._steps = steps
        return labels

    def case_of(self, pid, xt, H, FPR, adaptive, r, labels):
        return Case(pid, xt, H, FPR, adaptive, r, labels, self._steps)

    # -- construction ---------------------------------------------------------------------------------------------------
    def _build(self):
        key = self.key
        if key == "intermediate":
            self._torque_arm()
            self._axes()
            self._signs(((1.3, 0.1, 0.1, 600.0), (1.2, -0.1, -0.1, 0.0), (-0.9, 0.1, 0.1, -600.0), (-0.8, 0.0, -0.1, 0.0)))
            self._horizon_end("boat_intermediate")
            self._natural()
            return
        m = self.m
        self._heading()
        if m.mode == 1:
            self._focus()
        if m.mode == 2:
            self._torque_arm()
        if key in ("boat", "floor"):
            self._thrust_exact()
        if key in ("boat", "car"):
            self._thruster_alone()
        self._signs(())
        self._braking()
        if key == "boat":
            self._horizon_end("ros_boat")
        if key == "empty":
            for c in world("boat").cases:
                if "sweep:hit" in c.labels:
                    w = world("boat")
                    self.offer(w.states[c.pid], w.K[c.pid], c.target, H=3, FPR=c.FPR)
        self._natural()

    def _moving(self, h, vx, vy, vh=0.0, pos=None):
        pos = self.open if pos is None else pos
        return np.array([pos[0], pos[1], h, vx, vy, vh])

    def _heading(self):
        """A yaw effort K e of some hundred N m (a heading error times a gain of the tree's that need not be the system's own:
        the car behaviour's is zero), which mode 0 uses and modes 1 and 2 record and replace."""
        for h, vx in ((0.0, 0.3), (0.9, 0.5), (-2.0, 0.1)):
            x = self._moving(h, vx, 0.02)
            K = self.gain(x)
            K[2, 2] += 500.0
            xt = self.aim(x, 60.0, 10.0)
            xt[2] += 0.3
            self.offer(x, K, xt, H=2)

    def _focus(self):
        """The focus ahead, abeam, dead astern on either side of the +-pi cut, and on the boat itself with each pair of signed
        zeros the two subtractions can give (focus - x = -0 only for focus = -0, x = +0)."""
        f = self.m.focus
        if f != (0.0, 0.0):
            return
        z = {"+": 0.0, "-": -0.0}
        for h in (0.0, 0.7):
            for a in "+-":
                for b in "+-":
                    x = np.array([z[a], z[b], h, 0.0, 0.0, 0.0])
                    self.offer(x, self.gain(x), self.aim(x, 40.0, 5.0), H=2)
        for vx in (0.3, 0.0):
            for y in (0.0, -0.0):
                x = np.array([1.5, y, 0.0, vx, 0.0, 0.0])                                   # dead astern: yb = -+0, xb < 0
                self.offer(x, self.gain(x), self.aim(x, 40.0, 0.0), H=2)
        for pos, h in (((-1.5, 0.0), 0.0), ((-1.0, -1.0), math.pi / 4), ((0.0, -1.5), 0.0), ((0.0, 1.5), 0.0), ((1.0, 0.5), 2.0)):
            x = self._moving(h, 0.2, 0.0, pos=pos)
            self.offer(x, self.gain(x), self.aim(x, 40.0, 5.0), H=2)

    def _torque_arm(self):
        vmin = self.s.torque_vmin
        assert vmin * vmin == self.m.vmin2
        for i, (vx, vy) in enumerate(CC.torque_seeds(vmin)):
            for h in (0.0, 0.7, -2.5):
                x = self._moving(h, vx, vy, 0.05 * ((i % 3) - 1))
                for f in ((200.0, 10.0), (-150.0, -20.0)):
                    self.offer(x, self.gain(x), self.aim(x, *f), H=3)

    def _one(self, row, col, e, x=None, H=2):
        """A parent whose gain is a single 1.0 at (row, col), toward a target with error e in component col: u[row] = e exactly."""
        x = np.zeros(6) if x is None else x
        K = np.zeros((3, 6))
        K[row, col] = 1.0
        xt = x.copy()
        xt[col] = x[col] + e
        assert xt[col] - x[col] == e
        return self.offer(x, K, xt, H=H)

    def _thrust_exact(self):
        """Mode 0, u = (e, 0, 0) from a boat at rest at the origin: thrust j is invB[j][0] * e, nothing else.  On the limit, one
        ulp above, far above (all four tie), below the 1e-6 floor, and zero (K = 0).  Searched a few ulps of e each way."""
        ib, tmax = self.m.invB[:, 0], self.m.tmax
        for target in (tmax[0], up(tmax[0]), 2.0 * tmax[0], 5e-7, 0.9 * tmax[0]):
            e = target / ib[0]
            cands = [e]
            for _ in range(4):
                cands = [down(cands[0])] + cands + [up(cands[-1])]
            for e in sorted(cands, key=lambda v: abs(v - target / ib[0])):
                self._one(0, 0, e)
                self._one(0, 0, e, x=np.array([0.0, 0.0, 0.0, 0.0, 0.01, 0.0]))
        # u = (e0, e1, 0): the thrusts differ, one of them on its limit, and B t is not u bit for bit
        K = np.zeros((3, 6))
        K[0, 0] = K[1, 1] = 1.0
        for e1 in (100.0, -37.5, 61.25, -140.0, 12.0, 77.0):
            j = int(np.argmax(np.abs(self.m.invB[:, 0] * 600.0 + self.m.invB[:, 1] * e1)))
            e0 = (tmax[j] - self.m.invB[j, 1] * e1) / self.m.invB[j, 0]
            cands = [e0]
            for _ in range(8):
                cands = [down(cands[0])] + cands + [up(cands[-1])]
            for e in cands:
                self.offer(np.zeros(6), K, np.array([e, e1, 0.0, 0.0, 0.0, 0.0]), H=2)
        x = np.zeros(6)
        for d in (1.0, -2.0):                                  # K = 0, e != 0: every thrust is zero
            xt = x.copy()
            xt[0] = d
            self.offer(x, np.zeros((3, 6)), xt, H=2)

    def _thruster_alone(self):
        """One thruster beyond its limit alone: the force the target asks for and the yaw effort (mode 0: K e of a heading error;
        mode 2: the torque of a sway) are searched over a seeded box."""
        rs = np.random.RandomState(3)
        want = ["sat0:one-alone"] if self.m.sat == 0 else ALONE
        kp2 = self.s.kp[2, 2]
        for _ in range(4000):
            if all(self.coverage[c] >= 2 for c in want):
                break
            u0, u1, M = rs.uniform(-900, 900), rs.uniform(-900, 900), rs.uniform(-1500, 1500)
            a = np.sort(np.abs(self.m.invB.dot([u0, u1, M])))
            if not (a[3] > 1.05 * self.m.tmax[0] and a[2] < 0.9 * self.m.tmax[0]):
                continue
            h = rs.choice([0.0, 1.1])
            if self.m.mode == 0:
                x = self._moving(h, 0.0, 0.0)
                xt = self.aim(x, u0, u1)
                xt[2] += M / kp2
            else:
                x = self._moving(h, 0.5, 0.5 * math.tan(M / self.m.rudder))
                xt = self.aim(x, u0, u1)
            self.offer(x, self.gain(x), xt, H=2)

    def _signs(self, more):
        """Every sign of every velocity; for the boats with a car-like rule, surges beyond the speed that scales the yaw rate."""
        for vx, vy, vh, f in ((0.3, -0.2, -0.15, 100.0), (0.4, 0.1, 0.1, 50.0), (-0.2, -0.1, -0.1, 300.0), (-0.4, 0.2, 0.1, 400.0),
                              (0.6, -0.3, 0.15, 0.0)) + tuple(more):
            for h in (0.0, 2.0):
                x = self._moving(h, vx, vy, vh)
                self.offer(x, self.gain(x), self.aim(x, f, 5.0), H=3)

    def _braking(self):
        """A surge driven below zero: from a slow forward boat, from one that backs up, from +0 and -0; and one left alone.
        (Mode 2 at rest: v = (-0, +0) points astern for atan2, and the torque of half a turn, clipped per thruster, pushes the boat
        forward; v = (-0, -0) points ahead.)"""
        for vx, vy, f in ((0.02, 0.0, -800.0), (0.01, 0.0, -600.0), (-0.3, 0.0, -100.0), (-0.2, 0.0, 50.0), (0.0, 0.0, -500.0),
                          (-0.0, 0.0, -500.0), (-0.0, -0.0, -500.0), (-0.0, -0.0, -300.0), (0.5, 0.0, 100.0)):
            for h in (0.0, 2.0):
                x = self._moving(h, vx, vy)
                self.offer(x, self.gain(x), self.aim(x, f, 0.0), H=2)

    def _axes(self):
        """u[i] = K e on u_max, one ulp beyond it, the same below zero, and well inside: a single 1.0 in the gain on the velocity
        error of the axis, from a boat whose velocity on that axis is zero.  Axis 2 from a boat that moves straight ahead
        (v_y = +0: the direct arm's atan2(+0, v_x) = 0 adds nothing)."""
        um = self.m.umax
        for i in (0, 1):
            for e in (um[i], up(um[i]), -um[i], down(-um[i]), 0.25 * um[i], -0.125 * um[i]):
                for h in (0.0, 0.5):
                    self._one(i, 3 + i, e, x=self._moving(h, 0.0, 0.0))
        for e in (um[2], up(um[2])):
            for vx in (0.5, 0.25):
                self._one(2, 5, e, x=self._moving(0.0, vx, 0.0))

    def _horizon_end(self, name):
        """Rollouts that end on step H + 1: feasible there (the horizon, fixed and adaptive) and infeasible there under every
        FPR -- parents on the trajectory of a seed pair of tests/steer_cases.py whose first infeasible step comes late."""
        c = self.seeds
        assert c.name == name and np.array_equal(c.s.params(), self.s.params()) and np.array_equal(c.s.obs, self.s.obs)
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
        """Seed pairs of the sample space as they come, with this world's own gain: obstacles met on the way, and whatever
        saturation the behaviour runs into."""
        c = self.seeds
        for i in range(len(c.spar)):
            if all(self.coverage[k] >= 2 for k in self.required) or len(self.cases) >= MAX_CASES:
                break
            self.offer(c.spar[i], self.gain(c.spar[i]), c.star[i], H=3)


_CACHE = {}


def world(key):
    if key not in _CACHE:
        _CACHE[key] = World(key)
    return _CACHE[key]
