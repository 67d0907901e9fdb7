"""
NumPy float64 model of the planar vehicles' collision tests (csrc/systems.hpp hull_hits, grid_hits, BoatNovice::feasible), the hull,
map and obstacle-table builders of tests/test_feasibility_gpu.py, and a restatement of what the two device culls read and decide.

Model (no cull, no squared threshold, no ballot loop):
  circles_feasible   verts = p + R(h) vps; a hit iff any np.linalg.norm(vert - c) <= r (demo_boat_advanced.py:216-224); `extra2p`
                     adds the car's accidental vertex at 2p (demo_car.py:175)
  novice_feasible    a hit iff norm(p - c) <= half_length + r (demo_boat_novice.py:160-164)
  grid_feasible      demos/lqrrt_ros/nodes/lqrrt_node.py:730-745 word for word: indices (cpm * (points - origin)).astype(np.int64),
                     grid[iy, ix] under try / except IndexError -> False, all(values < thr) -- with the integer rules spelled out
                     (truncation towards zero, ONE wrap of an index in [-dim, -1], anything else outside = IndexError), so that the
                     answer does not depend on what this host's NumPy makes of a non-finite cast: a non-finite coordinate, or one of
                     magnitude >= 2^63, is outside the map
The vertices are formed as the C oracle forms them, px + (c bx + (-s) by), one rounding per operation; c and s are ARGUMENTS: the
portable lq_sincos values (portable_sincos) make the model bit-comparable with oracle/lqrrt_oracle.c and the device, np.cos / np.sin
give the reference's own.

Restated culls (csrc/engine_geometry.hpp upload_geometry, csrc/systems.hpp):
  GridGeo / grid_cull     the coarse 8x8 map, reach and bounding box the host derives; which stage decides a pose -- `coarse`, `fine`
                          or `sweep` -- and the coarse block range and fine cell range it reads.  bounded=False is the rule before the
                          fine stage got its bounds condition: tests/test_feasibility_cpu.py holds the two apart.
  CircleGeo / circle_near the derived circle table [x, y, thr, padded r] with exact_sq_threshold restated, the padded hull box, and the
                          `near` predicate per obstacle
so that a GPU case can assert that it reaches the path it is named after.

CASES: every pose set of tests/test_feasibility_gpu.py, built once here and shared with tests/test_feasibility_cpu.py, which holds the
model, the NumPy twin (oracle/systems_np.py) and the C oracle together on all of them.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from systems_np import hull_grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO63 = 2.0 ** 63
OG_COARSE_SHIFT = 3          # csrc/systems.hpp
OG_LDS_BYTES = 48 * 1024     # csrc/engine_geometry.hpp: hull points beyond this stay in HBM (og_lds = 0)
FINE_CELLS_MAX = 1024        # csrc/systems.hpp grid_hits


# ------------------------------------------------------------------------------------------------ portable sine / cosine

_pm = None


def portable_sincos(h):
    """(c, s) of include/lqrrt_pmath.h lq_sincos -- what the C oracle and the device use -- for a scalar or an array of headings."""
    global _pm
    if _pm is None:
        d = tempfile.mkdtemp()
        with open(os.path.join(d, "t.c"), "w") as f:
            f.write('#include "lqrrt_pmath.h"\n'
                    "void v_sincos(const double* x, int n, double* s, double* c){ for(int i=0;i<n;i++) lq_sincos(x[i], &s[i], &c[i]); }\n")
        so = os.path.join(d, "t.so")
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-mfma", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"),
                               os.path.join(d, "t.c"), "-o", so, "-lm"])
        _pm = C.CDLL(so)
    x = np.ascontiguousarray(np.atleast_1d(h), dtype=np.float64)
    s, c = np.empty_like(x), np.empty_like(x)
    P = C.POINTER(C.c_double)
    _pm.v_sincos(x.ctypes.data_as(P), len(x), s.ctypes.data_as(P), c.ctypes.data_as(P))
    return (c, s) if np.ndim(h) else (float(c[0]), float(s[0]))


def numpy_sincos(h):
    return np.cos(h), np.sin(h)


# ------------------------------------------------------------------------------------------------ the model

def vertices(vps, x, c, s):
    """(V, 2) world positions of the hull points for the pose x = [px, py, ...], in the C oracle's operation order."""
    vps = np.asarray(vps, dtype=np.float64).reshape(2, -1)
    with np.errstate(invalid="ignore", over="ignore"):
        vx = x[0] + (c * vps[0] + (-s) * vps[1])
        vy = x[1] + (s * vps[0] + c * vps[1])
    return np.stack((vx, vy), axis=1)


def circles_feasible(vps, obs, x, c, s, extra2p=False):
    """The plain double loop of demo_boat_advanced.py:216-224: per obstacle, npl.norm(verts - centre, axis=1) <= r."""
    verts = vertices(vps, x, c, s)
    with np.errstate(invalid="ignore", over="ignore"):
        if extra2p:
            verts = np.vstack((verts, [[x[0] + x[0], x[1] + x[1]]]))
        for ob in np.asarray(obs, dtype=np.float64).reshape(-1, 3):
            if len(verts) and np.any(np.linalg.norm(verts - ob[:2], axis=1) <= ob[2]):
                return False
    return True


def novice_feasible(obs, half_length, x):
    p = np.asarray(x[:2], dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for ob in np.asarray(obs, dtype=np.float64).reshape(-1, 3):
            if np.linalg.norm(p - ob[:2]) <= half_length + ob[2]:
                return False
    return True


def cell_indices(f, dim):
    """(index, valid) of float cell coordinates f along an axis of length dim under `.astype(np.int64)` and NumPy's index rules:
    truncation towards zero; an index in [-dim, -1] wraps ONCE; anything else outside raises IndexError (valid = False).  A
    coordinate whose cast is undefined (NaN, inf, magnitude >= 2^63) is outside."""
    f = np.asarray(f, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        wild = ~np.isfinite(f) | (np.abs(f) >= TWO63)
    i = np.trunc(np.where(wild, 0.0, f)).astype(np.int64)
    i = np.where(i < 0, i + dim, i)
    valid = ~wild & (i >= 0) & (i < dim)
    return np.where(valid, i, 0), valid


def grid_feasible(vps, grid, origin, cpm, thr, x, c, s):
    grid = np.asarray(grid)
    rows, cols = grid.shape
    points = vertices(vps, x, c, s)
    with np.errstate(invalid="ignore", over="ignore"):
        f = cpm * (points - np.asarray(origin, dtype=np.float64))
    ix, okx = cell_indices(f[:, 0], cols)
    iy, oky = cell_indices(f[:, 1], rows)
    if not (np.all(okx) and np.all(oky)):
        return False                                      # IndexError
    values = grid[iy, ix].astype(np.float64)
    return bool(np.all(values < float(thr)))


# ------------------------------------------------------------------------------------------------ hulls

def point_hull():
    """One point at the origin: the rotation drops out exactly, the pose IS the vertex."""
    return np.zeros((2, 1))


def lattice_hull(length=2.0, width=1.0, spacing=0.25):
    """A hull_grid lattice (the demos' hulls): the corners of its bounding box are hull points."""
    return hull_grid(length, width, 0.0, spacing)


def disc_hull(n=96, radius=1.0):
    """n points on a circle: the corners of the bounding box lie sqrt(2) radius from the centre, beyond every hull point."""
    a = 2.0 * np.pi * np.arange(n) / n
    return np.vstack((radius * np.cos(a), radius * np.sin(a)))


def diamond_hull(a=1.5, b=0.6, per_side=8):
    """Points on |x| / a + |y| / b = 1: a pointed bow and stern."""
    t = np.arange(per_side) / float(per_side)
    xs = np.concatenate((a * (1 - t), -a * t, -a * (1 - t), a * t))
    ys = np.concatenate((b * t, b * (1 - t), -b * t, -b * (1 - t)))
    return np.vstack((xs, ys))


def sparse_hull(length=1.0, width=0.6):
    """The four corners of a rectangle several cells long: it straddles cells that none of its points touches."""
    return np.array([[-length / 2, length / 2, length / 2, -length / 2], [-width / 2, -width / 2, width / 2, width / 2]])


def big_lattice_hull(nx=439, ny=7, length=2.0, width=0.6):
    """nx * ny = 3073 points: one more than fits in LDS next to the edge history (og_lds = 0: the sweep reads the hull from HBM)."""
    gx, gy = np.meshgrid(np.linspace(-length / 2, length / 2, nx), np.linspace(-width / 2, width / 2, ny), indexing="ij")
    return np.vstack((gx.ravel(), gy.ravel()))


def cluster_hull(V, special, at=(0.0, 2.0), seed=0):
    """V points of which V - 1 lie within 0.2 m of the origin and number `special` at `at`: at heading 0 it alone reaches a cell
    planted 2 m away."""
    rs = np.random.RandomState(100 + V + seed)
    vps = rs.uniform(-0.2, 0.2, (2, V))
    if special is not None:
        vps[0, special], vps[1, special] = at
    return vps


# ------------------------------------------------------------------------------------------------ maps and obstacle tables

def empty_map(rows, cols, value=0):
    return np.full((rows, cols), value, dtype=np.int8)


def planted_map(rows, cols, cells, value=100, fill=0):
    """(rows, cols) int8 map of `fill` with value at every (row, col) of cells."""
    g = empty_map(rows, cols, fill)
    for r, c in cells:
        g[r, c] = value
    return g


def placeholder_rows(n):
    """The demos' never-hit rows [-9999, -9999, -9999] (noisy_obstacle_grid): negative radius."""
    return np.full((n, 3), -9999.0)


def planted_table(O, hits, far=(500.0, 500.0)):
    """O circles: radius 0.5 far away from everything, except {slot: (x, y, r)} of hits."""
    obs = np.zeros((O, 3))
    for o in range(O):
        obs[o] = [far[0] + 3.0 * (o % 50), far[1] + 3.0 * (o // 50), 0.5]
    for o, row in hits.items():
        obs[o] = row
    return obs


# ------------------------------------------------------------------------------------------------ restated culls: the occupancy grid

def _cvt_i32(v):
    """(int) of a double as gfx950 converts it: truncation, saturating, NaN -> 0.  (In range it is C's; grid_hits casts values that are
    not only where the heading is non-finite, and then its bounds condition keeps it off the map's memory whatever this yields.)"""
    if np.isnan(v):
        return 0
    return int(max(-2.0 ** 31, min(2.0 ** 31 - 1, np.trunc(v))))


class GridGeo(object):
    """What upload_geometry derives from (hull, map, threshold)."""

    def __init__(self, vps, grid, thr):
        vps = np.asarray(vps, dtype=np.float64).reshape(2, -1)
        grid = np.asarray(grid)
        self.vps, self.grid, self.thr = vps, grid, float(thr)
        self.V = vps.shape[1]
        self.rows, self.cols = grid.shape
        self.occupied = ~(grid.astype(np.float64) < self.thr)                     # "not (value < threshold)", as the sweep reads it
        B = 1 << OG_COARSE_SHIFT
        self.crows, self.ccols = (self.rows + B - 1) >> OG_COARSE_SHIFT, (self.cols + B - 1) >> OG_COARSE_SHIFT
        self.coarse = np.zeros((self.crows, self.ccols), dtype=bool)
        for r, c in zip(*np.nonzero(self.occupied)):
            self.coarse[r >> OG_COARSE_SHIFT, c >> OG_COARSE_SHIFT] = True
        hull_r = float(np.max(np.sqrt(vps[0] * vps[0] + vps[1] * vps[1]))) if self.V else 0.0
        self.reach = hull_r * (1.0 + 1e-9) + 1e-9
        self.bb = [float(vps[0].min()), float(vps[0].max()), float(vps[1].min()), float(vps[1].max())] if self.V else [0.0] * 4
        self.og_lds = 2 * self.V * 8 <= OG_LDS_BYTES


def grid_cull(geo, origin, cpm, x, c, s, bounded=True):
    """The two cull stages of grid_hits for one pose.  Returns dict(
         stage   'coarse' / 'fine': that stage answered "free"; 'sweep': the exact sweep decides
         why     for 'sweep': 'border' (reach box not strictly inside the map), 'cells' (more than 1024 fine cells), 'bounds' (the fine
                 box leaves the map), 'occupied' (the fine box holds an occupied cell)
         coarse  (cy0, cy1, cx0, cx1) block range read, or None
         fine    (fy0, fy1, fx0, fx1) cell range computed, or None;  fine_read: whether those cells are read)
    bounded=False: the rule before the bounds condition -- the fine cells are read wherever they lie."""
    px, py = float(x[0]), float(x[1])
    ox, oy = float(origin[0]), float(origin[1])
    out = dict(stage="sweep", why="border", coarse=None, fine=None, fine_read=False)
    with np.errstate(invalid="ignore", over="ignore"):
        x0, x1 = cpm * ((px - geo.reach) - ox), cpm * ((px + geo.reach) - ox)
        y0, y1 = cpm * ((py - geo.reach) - oy), cpm * ((py + geo.reach) - oy)
    if not (x0 >= 2.0 and y0 >= 2.0 and x1 < float(geo.cols - 2) and y1 < float(geo.rows - 2)):
        return out
    cx0, cx1 = (int(x0) - 1) >> OG_COARSE_SHIFT, (int(x1) + 1) >> OG_COARSE_SHIFT
    cy0, cy1 = (int(y0) - 1) >> OG_COARSE_SHIFT, (int(y1) + 1) >> OG_COARSE_SHIFT
    out["coarse"] = (cy0, cy1, cx0, cx1)
    if not (0 <= cy0 and cy1 < geo.crows and 0 <= cx0 and cx1 < geo.ccols):
        raise AssertionError("the coarse stage reads outside the coarse map: %r of %d x %d" % (out["coarse"], geo.crows, geo.ccols))
    if not geo.coarse[cy0:cy1 + 1, cx0:cx1 + 1].any():
        out["stage"], out["why"] = "coarse", None
        return out
    bb = geo.bb
    with np.errstate(invalid="ignore", over="ignore"):
        ax0, ax1, bx0, bx1 = c * bb[0], c * bb[1], s * bb[0], s * bb[1]
        ay0, ay1, by0, by1 = s * bb[2], s * bb[3], c * bb[2], c * bb[3]
        fmin, fmax = np.fmin, np.fmax
        wx_lo, wx_hi = fmin(ax0, ax1) - fmax(ay0, ay1), fmax(ax0, ax1) - fmin(ay0, ay1)
        wy_lo, wy_hi = fmin(bx0, bx1) + fmin(by0, by1), fmax(bx0, bx1) + fmax(by0, by1)
        m = 1e-9 * (1.0 + geo.reach)
        fx0, fx1 = _cvt_i32(cpm * ((px + wx_lo - m) - ox)) - 1, _cvt_i32(cpm * ((px + wx_hi + m) - ox)) + 1
        fy0, fy1 = _cvt_i32(cpm * ((py + wy_lo - m) - oy)) - 1, _cvt_i32(cpm * ((py + wy_hi + m) - oy)) + 1
    out["fine"] = (fy0, fy1, fx0, fx1)
    fcells = (fx1 - fx0 + 1) * (fy1 - fy0 + 1)
    if fcells > FINE_CELLS_MAX:
        out["why"] = "cells"
        return out
    inside = 0 <= fx0 and fx1 < geo.cols and 0 <= fy0 and fy1 < geo.rows
    if bounded and not inside:
        out["why"] = "bounds"
        return out
    out["fine_read"] = True
    if not inside:                                        # (the previous rule reads them all the same: the caller looks at `fine`)
        out["why"] = "outside"
        return out
    if geo.occupied[fy0:fy1 + 1, fx0:fx1 + 1].any():
        out["why"] = "occupied"
        return out
    out["stage"], out["why"] = "fine", None
    return out


# ------------------------------------------------------------------------------------------------ restated culls: circles

def exact_sq_threshold(r):
    """csrc/engine_launch.hpp: the largest T with fl(sqrt(T)) <= r, -1 for a radius that is not >= 0, inf for inf."""
    r = np.float64(r)
    if not (r >= 0.0):
        return np.float64(-1.0)
    if np.isinf(r):
        return r
    with np.errstate(over="ignore"):
        T = r * r
    while np.sqrt(np.nextafter(T, np.inf)) <= r:
        T = np.nextafter(T, np.inf)
    while T > 0.0 and np.sqrt(T) > r:
        T = np.nextafter(T, -np.inf)
    return T


class CircleGeo(object):
    """upload_geometry's circle table [x, y, thr, padded r] and padded hull box.  inflate: BoatNovice's half length (added to r)."""

    def __init__(self, vps, obs, inflate=None):
        vps = np.asarray(vps, dtype=np.float64).reshape(2, -1)
        obs = np.asarray(obs, dtype=np.float64).reshape(-1, 3)
        self.V, self.O = vps.shape[1], len(obs)
        self.oc = np.zeros((self.O, 4))
        self.raw_r = np.zeros(self.O)
        for o, (x, y, r) in enumerate(obs):
            with np.errstate(invalid="ignore", over="ignore"):
                r = inflate + r if inflate is not None else r
                self.oc[o] = [x, y, exact_sq_threshold(r), r * (1.0 + 1e-9) + 1e-9 if r >= 0.0 else -1e300]
            self.raw_r[o] = r if r >= 0.0 else -1e300
        bb = [float(vps[0].min()), float(vps[0].max()), float(vps[1].min()), float(vps[1].max())] if self.V else [0.0] * 4
        self.raw_bb = bb
        self.bb = [b + 1e-9 * (1.0 + abs(b)) if k & 1 else b - 1e-9 * (1.0 + abs(b)) for k, b in enumerate(bb)]
        self.lds_bytes = 8 * (2 * self.V + 4 * self.O)


def circle_near(geo, x, c, s, padded=True):
    """hull_hits' `near` per obstacle: the centre, seen from the vehicle's frame, lies within the hull's box grown by the padded
    radius.  padded=False: the raw box and the raw radius (what the padding is there to cover)."""
    px, py = float(x[0]), float(x[1])
    near = np.zeros(geo.O, dtype=bool)
    bb = geo.bb if padded else geo.raw_bb
    for o in range(geo.O):
        ox, oy, rp = geo.oc[o, 0], geo.oc[o, 1], (geo.oc[o, 3] if padded else geo.raw_r[o])
        with np.errstate(invalid="ignore", over="ignore"):
            dx, dy = ox - px, oy - py
            cbx, cby = c * dx + s * dy, c * dy + (-s) * dx
            near[o] = (cbx >= bb[0] - rp) and (cbx <= bb[1] + rp) and (cby >= bb[2] - rp) and (cby <= bb[3] + rp)
    return near


# ------------------------------------------------------------------------------------------------ pose helpers

def ulp_trio(v):
    """v and its two neighbours."""
    v = np.float64(v)
    return [float(np.nextafter(v, -np.inf)), float(v), float(np.nextafter(v, np.inf))]


def poses(xy_h, n=6):
    """[(x, y, h)] -> (B, n) states with zero velocities."""
    X = np.zeros((len(xy_h), n))
    if len(xy_h):
        X[:, :3] = np.asarray(xy_h, dtype=np.float64)
    return X


# ------------------------------------------------------------------------------------------------ the cases, shared by the CPU and GPU tests

NSTATES = dict(boat_advanced=6, boat_intermediate=6, boat_novice=6, ros_boat=6, car=5)
HALF_LENGTH = 210 * 0.0254 / 2                                  # BoatNovice's inflation (demo_boat_novice.py:160-164)
PLAN_BOX = (np.array([1.1, 0.4, 0.2]), np.array([-0.65, -0.4, -0.2]))     # BoatAdvanced's planning speed box (demo_boat_advanced.py:211-213)
OCC, FREE, THR = 100, 0, 90.0


class Case(object):
    """One (system, geometry, pose set).  grid is None: the circle model with `obs`.  expect: answers planted by construction (or
    None); stages: the cull stage every pose is built to reach -- one string for all, a list, or None -- as 'stage' or 'stage:why'."""

    def __init__(self, name, system, X, vps, grid=None, origin=(0.0, 0.0), cpm=10.0, thr=THR, obs=None, expect=None, stages=None,
                 parked=True):
        self.name, self.system = name, system
        self.X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, NSTATES[system])
        self.vps = None if vps is None else np.ascontiguousarray(vps, dtype=np.float64).reshape(2, -1)
        self.grid = None if grid is None else np.ascontiguousarray(grid, dtype=np.int8)
        self.origin, self.cpm, self.thr = (float(origin[0]), float(origin[1])), float(cpm), float(thr)
        self.obs = None if obs is None else np.ascontiguousarray(obs, dtype=np.float64).reshape(-1, 3)
        self.expect = None if expect is None else np.asarray(expect, dtype=bool)
        self.stages = [stages] * len(self.X) if isinstance(stages, str) else stages
        self.parked = parked
        assert self.expect is None or len(self.expect) == len(self.X), name
        assert self.stages is None or len(self.stages) == len(self.X), name
        assert (self.grid is None) != (self.obs is None), name

    @property
    def kind(self):
        return "grid" if self.grid is not None else ("novice" if self.system == "boat_novice" else "circle")

    # -- the model
    def model(self, sincos=portable_sincos):
        c, s = sincos(self.X[:, 2])
        out = np.zeros(len(self.X), dtype=bool)
        for t, x in enumerate(self.X):
            if self.system == "boat_advanced" and not self.parked and (np.any(x[3:] > PLAN_BOX[0]) or np.any(x[3:] < PLAN_BOX[1])):
                continue
            if self.kind == "grid":
                out[t] = grid_feasible(self.vps, self.grid, self.origin, self.cpm, self.thr, x, c[t], s[t])
            elif self.kind == "novice":
                out[t] = novice_feasible(self.obs, HALF_LENGTH, x)
            else:
                out[t] = circles_feasible(self.vps, self.obs, x, c[t], s[t], extra2p=self.system == "car")
        return out

    # -- the restated culls
    def geo(self):
        if self.kind == "grid":
            return GridGeo(self.vps, self.grid, self.thr)
        return CircleGeo(self.vps if self.kind == "circle" else np.zeros((2, 0)), self.obs, HALF_LENGTH if self.kind == "novice" else None)

    def culls(self, bounded=True):
        g = self.geo()
        c, s = portable_sincos(self.X[:, 2])
        return [grid_cull(g, self.origin, self.cpm, x, c[t], s[t], bounded) for t, x in enumerate(self.X)]

    def stage_names(self):
        return ["%s:%s" % (d["stage"], d["why"]) if d["why"] else d["stage"] for d in self.culls()]

    def nears(self, padded=True):
        g = self.geo()
        c, s = portable_sincos(self.X[:, 2])
        return np.array([circle_near(g, x, c[t], s[t], padded) for t, x in enumerate(self.X)]).reshape(len(self.X), g.O)

    # -- the three implementations
    def native(self, into=None):
        """The lqrrt_amd system of this case; into: an existing system of the same model whose geometry is replaced (live engine)."""
        import lqrrt_amd
        s = into
        if s is None:
            s = lqrrt_amd.systems.RosBoat("car") if self.system == "ros_boat" else lqrrt_amd.systems.SYSTEMS[self.system](0)
        if self.system == "boat_advanced":
            s.velmax_pos_plan = np.full(3, 1e9) if self.parked else PLAN_BOX[0].copy()
            s.velmax_neg_plan = np.full(3, -1e9) if self.parked else PLAN_BOX[1].copy()
        if self.kind == "grid":
            s.set_occupancy_grid(self.grid, self.origin, cpm=self.cpm, threshold=self.thr, vps=self.vps)
        else:
            if self.vps is not None:
                s.vps = self.vps.copy()
            if s.ogrid is not None:
                s.clear_occupancy_grid()
            s.set_obstacles(self.obs)
        return s

    def twin(self):
        from systems_np import SYSTEMS
        t = SYSTEMS["ros_boat"]("car") if self.system == "ros_boat" else SYSTEMS[self.system](0)
        if self.system == "boat_advanced":
            t.velmax_pos_plan = np.full(3, 1e9) if self.parked else PLAN_BOX[0].copy()
            t.velmax_neg_plan = np.full(3, -1e9) if self.parked else PLAN_BOX[1].copy()
        if self.kind == "grid":
            t.set_occupancy_grid(self.grid, self.origin, self.cpm, self.thr, vps=self.vps)
        else:
            if self.vps is not None:
                t.vps = self.vps.copy()
            t.obs = self.obs.copy()
        return t

    def twin_answers(self):
        """oracle/systems_np.py: is_feasible where the class knows the map, its shared _grid_feasible (the method text of
        lqrrt_node.py:730-745) where it does not (boat_intermediate, car)."""
        import warnings
        t = self.twin()
        u = np.zeros(t.ncontrols)
        grid_only = self.kind == "grid" and self.system in ("boat_intermediate", "car")
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            return np.array([bool(t._grid_feasible(np.copy(x)) if grid_only else t.is_feasible(np.copy(x), u)) for x in self.X], dtype=bool)

    def oracle_answers(self):
        import coracle
        s = self.native()
        o = coracle.make(s, 16)
        u = np.zeros(s.ncontrols)
        return np.array([o.feasible(x, u) for x in self.X], dtype=bool)


def edge_coord(k, o, cpm):
    """The smallest double p whose cell coordinate cpm * (p - o), as computed, is >= k: p and its predecessor lie either side of k."""
    p = np.float64(o + k / cpm)
    while cpm * (p - o) >= k:
        p = np.nextafter(p, -np.inf)
    while cpm * (p - o) < k:
        p = np.nextafter(p, np.inf)
    return float(p)


def centre_coord(k, o, cpm):
    return o + (k + 0.5) / cpm


MAPS = {"64x64": dict(rows=64, cols=64, cpm=8.0, origin=(0.0, 0.0)),            # cpm a power of two, origin 0: the products are exact
        "61x75": dict(rows=61, cols=75, cpm=10.0, origin=(-0.7, 0.35))}         # sizes that are no multiple of 8, every product rounds


def _random_map(rows, cols, seed, p=0.5):
    return np.where(np.random.RandomState(seed).random_sample((rows, cols)) < p, OCC, FREE).astype(np.int8)


def _intended(k, side):
    """The index NumPy's rules give a coordinate just below (-1), on (0) or just above (+1) the integer k: truncation towards zero."""
    if side < 0:
        return k - 1 if k >= 1 else k
    if side > 0:
        return k if k >= 0 else k + 1
    return k


def _wrapped(i, dim):
    if i < 0:
        i += dim
    return i if 0 <= i < dim else None


def cases_a():
    """Index rules, one-point hull (the pose is the vertex): cell boundaries and one ulp either side, (-1, 0) truncating to cell 0
    without a wrap, -1 / -dim wrapping once, -dim - 1 and dim outside -- along a row and along a column of a random map whose cells
    next to each rule differ, and of its complement, so that the cell that is read decides in both directions."""
    out = []
    for mname, mp in sorted(MAPS.items()):
        rows, cols, cpm, (ox, oy) = mp["rows"], mp["cols"], mp["cpm"], mp["origin"]
        r0, c0 = 20, 30
        g = _random_map(rows, cols, 7)
        g[r0, [0, 1, 4, 5, cols - 2, cols - 1]] = [OCC, FREE, FREE, OCC, OCC, FREE]
        g[[0, 1, 4, 5, rows - 2, rows - 1], c0] = [FREE, OCC, OCC, FREE, FREE, OCC]
        for gname, grid in (("map", g), ("complement", (OCC - g).astype(np.int8))):
            for axis, dim, o in (("x", cols, ox), ("y", rows, oy)):
                xs, cells = [], []
                for k in (5, 0, -1, -dim, -dim - 1, dim - 1, dim, 1):
                    e = edge_coord(k, o, cpm)
                    on_k = cpm * (e - o) == k                     # (not every integer is met exactly when cpm (p - o) rounds twice:
                    for side, p in zip((-1, 0, 1), ulp_trio(e)):  #  then the edge pose lies just above k, like its upper neighbour)
                        xs.append(p)
                        cells.append(_wrapped(_intended(k, side if on_k or side else 1), dim))
                for f, cell in ((-0.5, 0), (0.5, 0), (-1.5, dim - 1), (-dim + 0.5, 1), (-dim - 0.5, 0), (-dim - 1.5, None),
                                (dim - 0.5, dim - 1), (dim + 0.5, None), (-2.0 * dim, None), (3.0 * dim, None)):
                    xs.append(o + f / cpm)
                    cells.append(cell)
                if axis == "x":
                    P = [(p, centre_coord(r0, oy, cpm), 0.7) for p in xs]
                    expect = [cl is not None and grid[r0, cl] == FREE for cl in cells]
                else:
                    P = [(centre_coord(c0, ox, cpm), p, -2.1) for p in xs]
                    expect = [cl is not None and grid[cl, c0] == FREE for cl in cells]
                out.append(Case("a %s %s along %s" % (mname, gname, axis), "boat_intermediate", poses(P), point_hull(), grid, (ox, oy), cpm,
                                expect=expect))
    return out


B_VALUES = (-128, -1, 0, 88, 89, 90, 91, 126, 127)
B_THRESHOLDS = (90.0, 89.5, 128.0, -128.0, float("nan"))


def cases_b():
    """Threshold: a row of cells holding B_VALUES, the pose on each, under every threshold in B_THRESHOLDS; `value < thr` decides (a NaN
    threshold occupies every cell, 128 frees them all: then the coarse map is empty and the first cull answers)."""
    out = []
    mp = MAPS["61x75"]
    for thr in B_THRESHOLDS:
        grid = empty_map(mp["rows"], mp["cols"], 0)
        P, expect = [], []
        for i, v in enumerate(B_VALUES):
            r, c = 11 + 2 * i, 9 + 5 * i
            grid[r, c] = v
            P.append((centre_coord(c, mp["origin"][0], mp["cpm"]), centre_coord(r, mp["origin"][1], mp["cpm"]), 0.3 * i))
            expect.append(bool(v < thr))
        P.append((centre_coord(40, mp["origin"][0], mp["cpm"]), centre_coord(5, mp["origin"][1], mp["cpm"]), 1.0))     # a cell holding 0
        expect.append(bool(0 < thr))
        out.append(Case("b thr %r" % thr, "boat_intermediate", poses(P), point_hull(), grid, mp["origin"], mp["cpm"], thr=thr, expect=expect))
    return out


SWEEP_V = (1, 63, 64, 65, 511, 512, 513, 1025)


def _sweep_cases(letter, sizes, system="boat_intermediate"):
    """The sweep's eight-points-per-lane groups: a hull of V points of which one -- the last, or the first of the last partial group of
    512 -- stands 2 m off (cluster_hull), heading 0, the pose 1.05 m from the map's corner so that the reach box leaves the map and the
    exact sweep decides.  'hit': the only occupied cell is the one under that vertex.  'free': every cell is occupied EXCEPT those
    under the V vertices -- a vertex read past the table, or a slot of the last group taken for a vertex, lands on an occupied one."""
    out = []
    cpm, origin = 10.0, (0.0, 0.0)
    px, py = 1.05, 1.05
    for V in sizes:
        for special in sorted(set((V - 1, 512 * ((V - 1) // 512)))):
            vps = cluster_hull(V, special)
            verts = vertices(vps, (px, py), 1.0, 0.0)
            ix, iy = (cpm * verts[:, 0]).astype(np.int64), (cpm * verts[:, 1]).astype(np.int64)
            sp = (int(iy[special]), int(ix[special]))
            assert sp == (30, 10) and all((int(r), int(c)) != sp for k, (r, c) in enumerate(zip(iy, ix)) if k != special)
            hit = planted_map(64, 64, [sp], OCC)
            free = empty_map(64, 64, OCC)
            free[iy, ix] = FREE
            X = poses([(px, py, 0.0)], NSTATES[system])
            out.append(Case("%s V=%d vertex %d hits" % (letter, V, special), system, X, vps, hit, origin, cpm, expect=[False], stages="sweep:border"))
            out.append(Case("%s V=%d vertex %d free" % (letter, V, special), system, X, vps, free, origin, cpm, expect=[True], stages="sweep:border"))
    return out


def cases_c():
    return _sweep_cases("c", SWEEP_V)


def cases_d():
    """og_lds = 0: 3073 hull points do not fit in LDS next to the edge history, the sweep reads them from HBM.  The planted hits of
    case c, and the 3073-point lattice alongside a wall."""
    out = _sweep_cases("d", (3073,))
    vps = big_lattice_hull()
    assert vps.shape[1] == 3073 and not GridGeo(vps, empty_map(8, 8), THR).og_lds and GridGeo(cluster_hull(3072, 0), empty_map(8, 8), THR).og_lds
    grid = empty_map(64, 64)
    grid[40, :] = OCC                                           # a wall along row 40: y in [4.0, 4.1)
    P = [(3.2, 3.2, 0.0), (3.2, 3.65, 0.0), (3.2, 3.75, 0.0), (3.2, 2.9, np.pi / 2), (3.2, 3.05, np.pi / 2), (3.2, 3.3, 0.9)]
    out.append(Case("d lattice of 3073 alongside a wall", "boat_intermediate", poses(P), vps, grid, (0.0, 0.0), 10.0))
    return out


E_HULL = (0.5, 0.25, 0.25)                                      # hull_grid(length, width, spacing): 3 x 2 points, binary fractions


def _reach_edge_poses(geo, origin, cpm, axis, C, side):
    """Two poses (as coordinates along `axis`) whose reach box, with its +-1 cell, just includes and just excludes coarse block C
    coming from `side` (-1: from below, the high edge x1 meets 8C - 1; +1: from above, the low edge x0 meets 8C + 9)."""
    o = origin[0 if axis == "x" else 1]
    if side < 0:
        inc = edge_coord(8 * C - 1, o - geo.reach, cpm)         # smallest p with cpm * ((p + reach) - o) >= 8C - 1 ...
        while cpm * ((inc + geo.reach) - o) >= 8 * C - 1:
            inc = float(np.nextafter(inc, -np.inf))
        while cpm * ((inc + geo.reach) - o) < 8 * C - 1:
            inc = float(np.nextafter(inc, np.inf))
        return inc, float(np.nextafter(inc, -np.inf))
    exc = edge_coord(8 * C + 9, o + geo.reach, cpm)
    while cpm * ((exc - geo.reach) - o) >= 8 * C + 9:
        exc = float(np.nextafter(exc, -np.inf))
    while cpm * ((exc - geo.reach) - o) < 8 * C + 9:
        exc = float(np.nextafter(exc, np.inf))
    return float(np.nextafter(exc, -np.inf)), exc


E_CELLS = ((24, 32), (31, 39), (24, 39), (31, 32), (58, 73))    # row / col mod 8 in {0, 7}; (58, 73): the partial last block of 61 x 75


def cases_e(mname="61x75"):
    """Coarse cull on the 61 x 75 map, one occupied cell per map: poses whose reach box just includes and just excludes the cell's
    8x8 block from either side along either axis (the hull itself stays clear: the fine stage, one level down, answers free), and
    poses with x0, y0, x1, y1 either side of the 2.0 / dim - 2 border condition."""
    mp = MAPS[mname]
    rows, cols, cpm, origin = mp["rows"], mp["cols"], mp["cpm"], mp["origin"]
    vps = lattice_hull(*E_HULL)
    out = []
    for (r, c) in E_CELLS:
        grid = planted_map(rows, cols, [(r, c)])
        geo = GridGeo(vps, grid, THR)
        P, stages = [], []
        # the other coordinate: the cell's own row / column, or the last one from which the reach box still stays inside the map
        for axis, C, other in (("x", c >> 3, centre_coord(min(r, rows - 7), origin[1], cpm)),
                               ("y", r >> 3, centre_coord(min(c, cols - 7), origin[0], cpm))):
            for side in (-1, 1):
                inc, exc = _reach_edge_poses(geo, origin, cpm, axis, C, side)
                for p, st in ((inc, "fine"), (exc, "coarse")):
                    P.append((p, other, 0.0) if axis == "x" else (other, p, 0.0))
                    stages.append(st)
        # (the partial last block cannot be met from above: that reach box is off the map.  Those poses are left out.)
        c_, s_ = portable_sincos(0.0)
        keep = [k for k, p in enumerate(P) if grid_cull(geo, origin, cpm, p, c_, s_)["why"] != "border"]
        assert len(keep) == (4 if (r, c) == (58, 73) else 8)
        P, stages = [P[k] for k in keep], [stages[k] for k in keep]
        out.append(Case("e cell (%d, %d)" % (r, c), "boat_intermediate", poses(P), vps, grid, origin, cpm, expect=[True] * len(P), stages=stages))
    # the border condition: the smallest coordinate with x0 >= 2.0 and its predecessor, the largest with x1 < dim - 2 and its successor
    grid = planted_map(rows, cols, [(4, 4), (rows - 5, cols - 5)])
    geo = GridGeo(vps, grid, THR)
    P, stages = [], []
    for axis, dim in (("x", cols), ("y", rows)):
        o = origin[0 if axis == "x" else 1]
        lo = edge_coord(2, o + geo.reach, cpm)
        while cpm * ((lo - geo.reach) - o) >= 2.0:
            lo = float(np.nextafter(lo, -np.inf))
        while cpm * ((lo - geo.reach) - o) < 2.0:
            lo = float(np.nextafter(lo, np.inf))
        hi = edge_coord(dim - 2, o - geo.reach, cpm)
        while cpm * ((hi + geo.reach) - o) >= dim - 2:
            hi = float(np.nextafter(hi, -np.inf))
        while cpm * ((hi + geo.reach) - o) < dim - 2:
            hi = float(np.nextafter(hi, np.inf))
        other_lo, other_hi = centre_coord(12, origin[1 if axis == "x" else 0], cpm), centre_coord((rows if axis == "x" else cols) - 20, origin[1 if axis == "x" else 0], cpm)
        for p, other, st in ((lo, other_lo, "coarse"), (float(np.nextafter(lo, -np.inf)), other_lo, "sweep:border"),
                             (float(np.nextafter(hi, -np.inf)), other_hi, "coarse"), (hi, other_hi, "sweep:border")):
            P.append((p, other, 0.0) if axis == "x" else (other, p, 0.0))
            stages.append(st)
    out.append(Case("e border condition", "boat_intermediate", poses(P), vps, grid, origin, cpm, expect=[True] * len(P), stages=stages))
    return out


BORDER_DISC_MAP = dict(rows=64, cols=64, cpm=10.0, origin=(0.0, 0.0))


def border_disc_case():
    """The out-of-bounds read of the fine cull: the 96-point disc at heading pi/4, the reach box just inside the map at the low corner (x0 = y0 = 2.0 and a
    little) and at the high one.  The rotated bounding box of the disc reaches cells -3 and 67 of the 64 x 64 map."""
    vps = disc_hull()
    grid = planted_map(64, 64, [(12, 12), (50, 50)])             # under the disc's centre: no point of the circle reaches it
    geo = GridGeo(vps, grid, THR)
    lo = 0.2000000001 + geo.reach
    hi = 6.2 - geo.reach - 1e-9
    P = [(lo, lo, np.pi / 4), (hi, hi, np.pi / 4)]
    return Case("f disc at the border", "boat_intermediate", poses(P), vps, grid, (0.0, 0.0), 10.0, expect=[True, True], stages="sweep:bounds")


def cases_f():
    """Fine cull: a vehicle closing in on a wall in steps of a quarter cell at headings 0, pi/4 and 1.234 (every stage is met on the way:
    coarse, fine, occupied-but-clear, hit); the sparse hull straddling an occupied cell (feasible: only points are tested); a hull
    of more than 1024 fine cells; the disc at the two border poses where the fine cull used to read off the map."""
    out = []
    vps = lattice_hull()                                         # 2.0 x 1.0, spacing 0.25: 45 points
    grid = empty_map(64, 64)
    grid[50, :] = OCC                                           # y in [5.0, 5.1)
    for h in (0.0, np.pi / 4, 1.234):
        P = [(3.2, 2.4 + 0.025 * i, h) for i in range(100)]     # the reach box stays inside the map up to y = 5.08
        out.append(Case("f wall heading %.3f" % h, "boat_intermediate", poses(P), vps, grid, (0.0, 0.0), 10.0))
    sp = sparse_hull()
    mp = MAPS["61x75"]
    cells = [(30, 40), (31, 40), (30, 41)]
    grid = planted_map(mp["rows"], mp["cols"], cells)
    P = [(centre_coord(40, mp["origin"][0], mp["cpm"]), centre_coord(30, mp["origin"][1], mp["cpm"]), h) for h in (0.0, 0.4, np.pi / 2, 2.0)]
    P += [(centre_coord(40 + 5, mp["origin"][0], mp["cpm"]), centre_coord(30 + 3, mp["origin"][1], mp["cpm"]), 0.0),       # a corner on cell (30, 40)
          (centre_coord(40 - 5, mp["origin"][0], mp["cpm"]), centre_coord(31 - 3, mp["origin"][1], mp["cpm"]), 0.0)]       # ... on (31, 40)
    out.append(Case("f sparse hull over occupied cells", "boat_intermediate", poses(P), sp, grid, mp["origin"], mp["cpm"],
                    expect=[True, True, True, True, False, False], stages="sweep:occupied"))
    big = lattice_hull(4.0, 3.0, 0.5)
    grid = planted_map(64, 64, [(10, 32), (32, 10)])
    P = [(3.25, 3.25, 0.0), (3.25, 3.25, 0.6), (3.05, 3.25, 0.0), (3.25, 3.05, np.pi / 2)]       # the last two: the stern row on a planted cell
    out.append(Case("f more than 1024 fine cells", "boat_intermediate", poses(P), big, grid, (0.0, 0.0), 10.0, stages="sweep:cells"))
    out.append(border_disc_case())
    return out


G_MODELS = (("boat_advanced", True), ("boat_advanced", False), ("boat_intermediate", True), ("car", True), ("ros_boat", True))


def _blob_map(rows, cols, seed, blobs=9):
    rs = np.random.RandomState(seed)
    g = empty_map(rows, cols)
    for _ in range(blobs):
        r, c, h, w = rs.randint(4, rows - 4), rs.randint(4, cols - 4), rs.randint(1, 6), rs.randint(1, 6)
        g[r:r + h, c:c + w] = rs.choice([91, 100, 127, 90])
    g[rs.randint(0, rows, 12), rs.randint(0, cols, 12)] = -1      # unknown cells: free
    return g


def cases_g():
    """Every model that calls grid_hits, on one shared pose set: 320 poses over and beyond the 61 x 75 blob map at any heading, the
    velocities drawn so that BoatAdvanced's planning speed box turns about a third of them away when it is not parked."""
    mp = MAPS["61x75"]
    rs = np.random.RandomState(11)
    grid = _blob_map(mp["rows"], mp["cols"], 3)
    vps = lattice_hull(1.0, 0.5, 0.25)
    B = 320
    X6 = np.zeros((B, 6))
    X6[:, 0] = mp["origin"][0] + rs.uniform(-0.6, mp["cols"] / mp["cpm"] + 0.6, B)
    X6[:, 1] = mp["origin"][1] + rs.uniform(-0.6, mp["rows"] / mp["cpm"] + 0.6, B)
    X6[:, 2] = rs.uniform(-np.pi, np.pi, B)
    X6[:, 3] = rs.uniform(-0.8, 1.3, B)
    X6[:, 4] = rs.uniform(-0.45, 0.45, B)
    X6[:, 5] = rs.uniform(-0.22, 0.22, B)
    out = []
    for system, parked in G_MODELS:
        X = X6 if NSTATES[system] == 6 else X6[:, [0, 1, 2, 3, 5]]
        out.append(Case("g %s%s" % (system, "" if parked else " with its speed box"), system, X, vps, grid, mp["origin"], mp["cpm"], parked=parked))
    return out


def cases_i():
    """Non-finite poses on a map whose cell (0, 0) is free: NaN or inf in x, y or the heading, and coordinates beyond the int64 range.
    The reference's cast-and-index raises IndexError for every one of them: infeasible.  The lattice poses stand next to an occupied
    blob, so that a non-finite HEADING passes the first cull (it only looks at x, y) and meets the second."""
    nan, inf = float("nan"), float("inf")
    grid = empty_map(64, 64)
    grid[30:34, 30:34] = OCC
    assert grid[0, 0] == FREE
    bad = [(nan, 3.2, 0.0), (3.2, nan, 0.0), (nan, nan, nan), (inf, 3.2, 0.0), (-inf, 3.2, 0.3), (3.2, inf, 0.0), (3.2, -inf, 1.0),
           (2.5, 2.5, nan), (2.5, 2.5, inf), (2.5, 2.5, -inf), (1e18, 3.2, 0.0), (-1e18, 3.2, 0.0), (3.2, 1e300, 0.0), (3.2, -1e300, 0.0),
           (2.0 ** 63 / 10.0, 3.2, 0.0), (0.05, 0.05, nan), (0.05, 0.05, inf)]
    good = [(2.5, 2.5, 0.0), (0.05, 0.05, 0.0)]
    out = []
    for hname, vps in (("point", point_hull()), ("lattice", lattice_hull(1.0, 0.5, 0.25))):
        expect = [False] * len(bad) + [True, True]          # (0.05, 0.05): the lattice's negative cells wrap once, to free cells
        out.append(Case("i non-finite poses, %s hull" % hname, "boat_intermediate", poses(bad + good), vps, grid, (0.0, 0.0), 10.0, expect=expect))
    out.append(Case("i non-finite poses, car", "car", poses(bad + good, 5), lattice_hull(1.0, 0.5, 0.25), grid, (0.0, 0.0), 10.0,
                    expect=[False] * len(bad) + [True, True]))
    return out


def grid_cases():
    return cases_a() + cases_b() + cases_c() + cases_d() + cases_e() + cases_f() + cases_g() + cases_i()


# -- circles

TANGENT_K = (0.125, 1.0, 3.0, 7.0, 1024.0, 2.0 ** 20 + 1.0)


def radius_for_sum(hl, target):
    """r with fl(hl + r) == target exactly."""
    r = np.float64(target - hl)
    for _ in range(64):
        if hl + r == target:
            return float(r)
        r = np.nextafter(r, np.inf if hl + r < target else -np.inf)
    raise AssertionError("no radius gives %r + r == %r" % (hl, target))


def cases_j():
    """Tangency: one-point hull at the origin, the obstacle at (3k, 4k): the distance is exactly 5k (9k^2 + 16k^2 and its root are
    exact for these k).  r = 5k and its two neighbours; BoatNovice with half_length + r landing on the same three values."""
    out = []
    for k in TANGENT_K:
        trio = ulp_trio(5.0 * k)
        assert (3.0 * k) ** 2 + (4.0 * k) ** 2 == (5.0 * k) ** 2 and np.sqrt((5.0 * k) ** 2) == 5.0 * k
        for system in ("boat_intermediate", "car", "boat_novice"):
            if system == "boat_novice" and 5.0 * k < HALF_LENGTH:
                continue                                        # (no radius makes half_length + r land on the neighbours of so small a sum)
            for h in (0.0, 2.5):
                rr = [radius_for_sum(HALF_LENGTH, t) for t in trio] if system == "boat_novice" else trio
                for r, hit in zip(rr, (False, True, True)):
                    obs = np.vstack((placeholder_rows(2), [[3.0 * k, 4.0 * k, r]], placeholder_rows(1)))
                    out.append(Case("j k=%g %s h=%g r=%r" % (k, system, h, r), system, poses([(0.0, 0.0, h)], NSTATES[system]),
                                    None if system == "boat_novice" else point_hull(), obs=obs, expect=[not hit]))
    return out


def cases_k():
    """Radii: 0 with a vertex on the centre (norm 0 <= 0: a hit), inf (everything hits), negative and NaN placeholders (never hit,
    not even from their own centre) interleaved with real obstacles."""
    nan, inf = float("nan"), float("inf")
    obs = np.array([[-9999.0, -9999.0, -9999.0], [5.0, 5.0, 0.0], [8.0, 5.0, nan], [11.0, 5.0, -1.0], [14.0, 5.0, 0.5],
                    [17.0, 5.0, -0.0], [20.0, 5.0, 5e-324], [-9999.0, -9999.0, -9999.0], [23.0, 5.0, -inf]])
    P = [(5.0, 5.0, 0.0), (float(np.nextafter(5.0, 6.0)), 5.0, 0.0), (8.0, 5.0, 0.0), (11.0, 5.0, 0.0), (14.0, 5.0, 0.0), (14.5, 5.0, 0.0),
         (float(np.nextafter(14.5, 15.0)), 5.0, 0.0), (17.0, 5.0, 0.0), (20.0, 5.0, 0.0), (23.0, 5.0, 0.0), (-9999.0, -9999.0, 0.0), (2.0, 2.0, 1.0)]
    expect = [False, True, True, True, False, False, True, False, False, True, True, True]
    out = [Case("k radii %s" % system, system, poses(P, NSTATES[system]), point_hull(), obs=obs, expect=expect) for system in ("boat_intermediate", "car")]
    obs_inf = np.vstack((placeholder_rows(3), [[100.0, -50.0, inf]], placeholder_rows(2)))
    out.append(Case("k an infinite radius", "boat_intermediate", poses(P), lattice_hull(), obs=obs_inf, expect=[False] * len(P)))
    out.append(Case("k an infinite radius, novice", "boat_novice", poses(P), None, obs=obs_inf, expect=[False] * len(P)))
    return out


BALLOT_O = (0, 1, 63, 64, 65, 129)
BALLOT_V = (1, 63, 64, 65, 187)


def cases_l(system="boat_intermediate"):
    """Ballot rounds: O obstacles of which only the LAST one is anywhere near, V hull points of which only the LAST one reaches it
    (cluster_hull: 2 m off the rest), heading 0.  Pose 0 hits, pose 1 stands 0.1 m further off and does not."""
    out = []
    for O in BALLOT_O:
        for V in BALLOT_V:
            vps = cluster_hull(V, V - 1)
            px, py = 40.0, 30.0
            obs = planted_table(O, {O - 1: (px, py + 2.03, 0.05)} if O else {})
            P = [(px, py, 0.0), (px, py - 0.1, 0.0)]
            out.append(Case("l O=%d V=%d" % (O, V), system, poses(P, NSTATES[system]), vps, obs=obs, expect=[O == 0, True]))
    return out


def rounding_poses(vps, n=6, seed=5):
    """[(pose, obstacle)] at heading 0 where rounding alone decides: the obstacle stands right of the hull's far corner row at a
    distance that exceeds its radius by a few ulps of the pose, the corner vertex px + bx rounds TOWARDS it and is inside, while
    the centre seen from the vehicle, ox - px, is beyond the UNPADDED box grown by the UNPADDED radius.  What the padding of
    hull_hits' cull (1e-9, against 1e-13 here) is there to cover."""
    rs = np.random.RandomState(seed)
    bx = float(np.max(vps[0]))
    by = float(vps[1][np.argmax(vps[0])])
    N = 200000
    px, py, r = rs.uniform(500.0, 1000.0, N), rs.uniform(-50.0, 50.0, N), rs.uniform(0.3, 2.0, N)
    ox = px + bx + r
    for _ in range(3):
        ox = np.where(rs.random_sample(N) < 0.5, np.nextafter(ox, np.inf), ox)
    cand = np.flatnonzero((np.abs((px + bx) - ox) <= r) & ((ox - px) > bx + r))         # candidates; the real functions decide below
    found = []
    for k in cand:
        x, ob = (float(px[k]), float(py[k]), 0.0), (float(ox[k]), float(py[k] + by), float(r[k]))
        if not circle_near(CircleGeo(vps, [ob]), x, 1.0, 0.0, padded=False)[0] and not circles_feasible(vps, [ob], x, 1.0, 0.0):
            found.append((x, ob))
            if len(found) == n:
                return found
    raise AssertionError("no pose found where rounding decides")


def cases_m():
    """The cull's edge, 2.0 x 1.0 lattice: an obstacle diagonal from a hull corner, inside the grown box but farther than r from the
    corner (near, no hit); one touching only the farthest corner (3-4-5 from it: tangent, and one ulp short); centres just outside
    and just inside the grown box at headings 0, pi/2, pi/4 and 1.234; poses where rounding alone puts a vertex inside."""
    vps = lattice_hull()
    out = []
    obs = np.vstack((placeholder_rows(1), [[1.4, 0.9, 0.5]], placeholder_rows(1)))
    out.append(Case("m diagonal from a corner", "boat_intermediate", poses([(0.0, 0.0, 0.0)]), vps, obs=obs, expect=[True], stages=None))
    for r, hit in zip(ulp_trio(1.25), (False, True, True)):
        out.append(Case("m touching the far corner r=%r" % r, "boat_intermediate", poses([(0.0, 0.0, 0.0)]), vps, obs=[[1.75, 1.5, r]], expect=[not hit]))
    for h in (0.0, np.pi / 2, np.pi / 4, 1.234):
        c, s = portable_sincos(h)
        px, py, r = 12.0, -7.0, 0.75
        for off, name in ((1e-8, "outside"), (-1e-3, "inside")):
            d = 1.0 + r + off                                   # along the body's x axis, past the bow row (1.0, 0.0)
            obs = np.vstack((placeholder_rows(1), [[px + c * d, py + s * d, r]]))
            out.append(Case("m centre just %s the grown box h=%.3f" % (name, h), "boat_intermediate", poses([(px, py, h)]), vps, obs=obs,
                            expect=[name == "outside"]))
    scaled = 1.1 * vps                                          # (coordinates that are no binary fractions: px + bx rounds)
    for i, (x, ob) in enumerate(rounding_poses(scaled)):
        out.append(Case("m rounding decides %d" % i, "boat_intermediate", poses([x]), scaled, obs=np.vstack((placeholder_rows(1), [ob])), expect=[False]))
    return out


def cases_n():
    """The car's stray vertex at 2p: an obstacle that contains 2p and is nowhere near the hull, in slot 66 of 70 (the second ballot
    round); the same with an empty hull; 2p just outside it."""
    out = []
    px, py = 10.0, 7.0
    from systems_np import hull_grid as hg
    for hname, vps in (("stock hull", hg(6, 3, 2, 0.5)), ("empty hull", np.zeros((2, 0))), ("point hull", point_hull())):
        for r, hit in ((0.3, True), (0.0, True), (-1.0, False)):
            obs = planted_table(70, {66: (2 * px, 2 * py, r)})
            out.append(Case("n %s, 2p in slot 66, r=%g" % (hname, r), "car", poses([(px, py, 0.8), (px + 0.25, py, 0.8)], 5), vps, obs=obs,
                            expect=[not hit, True]))
    return out


def cases_o():
    """A NaN pose is feasible (norm <= r is false); so is an infinite one against finite radii."""
    nan, inf = float("nan"), float("inf")
    P = [(nan, 5.0, 0.0), (5.0, nan, 0.0), (5.0, 5.0, nan), (nan, nan, nan), (inf, 5.0, 0.0), (5.0, -inf, 0.0), (5.0, 5.0, inf), (5.0, 5.0, 0.0)]
    obs = np.vstack((placeholder_rows(1), [[5.0, 5.0, 0.5], [0.0, 0.0, 3.0]]))
    out = []
    for system, vps in (("boat_intermediate", lattice_hull()), ("car", lattice_hull()), ("boat_advanced", point_hull()), ("boat_novice", None)):
        expect = [True] * 7 + [False]
        if system == "boat_novice":                             # the centre point has no heading: (5, 5, NaN) stands on the obstacle
            expect[2] = expect[6] = False
        out.append(Case("o non-finite poses %s" % system, system, poses(P, NSTATES[system]), vps, obs=obs, expect=expect))
    return out


def circle_cases():
    return cases_j() + cases_k() + cases_l() + cases_m() + cases_n() + cases_o()


# -- end to end

def tree_case():
    """p. boat_intermediate with the disc hull on a 61 x 75 map over the demo's 40 m square (1.5 cells per metre): blobs of occupied
    cells, the start and goal areas kept free."""
    rows, cols, cpm, origin = 61, 75, 1.5, (-5.0, -0.3)
    rs = np.random.RandomState(21)
    grid = empty_map(rows, cols)
    for _ in range(14):
        r, c = rs.randint(6, rows - 8), rs.randint(8, cols - 10)
        grid[r:r + rs.randint(2, 5), c:c + rs.randint(2, 5)] = OCC
    for px, py in ((0.0, 0.0), (40.0, 40.0)):
        c, r = int(cpm * (px - origin[0])), int(cpm * (py - origin[1]))
        grid[max(r - 6, 0):r + 7, max(c - 6, 0):c + 7] = FREE
    return dict(grid=grid, origin=origin, cpm=cpm, thr=THR, vps=disc_hull())
