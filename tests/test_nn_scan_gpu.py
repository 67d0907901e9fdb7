"""
The compiled-in nearest-neighbour scan (csrc/nn_scan.hpp k_nn_scan / k_nn_reduce, chosen by engine_launch.hpp launch_nn) at its tile,
tie and angle-mode edges, through lqrrt_nn_argmin on hand-built trees, against the NumPy model of tests/nn_scan_reference.py.

Bars (none of them new):
  * where the competing costs are bit-equal by construction -- periodic ties, one query in another angle mode, a forced launch form
    in a child process, the host form against the batched one -- ids and costs are demanded EXACTLY;
  * against the model: the id is the model's, or the model's costs of the two ids differ by a relative gap below 1e-12
    (tests/test_teacher_gpu.py), and the returned cost is within 1e-9 max(1, c) of the model's cost of the returned node
    (tests/test_hip_parity.py);
  * double_integrator with S = identity passed explicitly: nothing transcendental, zeros make the BLAS order irrelevant: exact.
Every planted answer is first asserted to be the model's own answer; every case asserts through the restated launch plan
(nn_scan_reference.launch_plan / angle_mode) that it reaches the path it is named after.
"""
import base64
import ctypes as C
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import nn_scan_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

# (system, S): "own" = the system's S (identity / S_DIAG / S_BAND2 / one Riccati solution per query), "dense" = a caller's matrix,
# "eye" = the identity passed as a caller's matrix
VARIANTS = [("boat_advanced", "own"), ("boat_advanced", "dense"), ("pendulum", "own"), ("pendulum", "dense"),
            ("double_integrator", "own"), ("double_integrator", "dense"), ("double_integrator", "eye"),
            ("ros_boat", "own"), ("ros_boat", "dense"), ("pendulum_lqr", "own"), ("pendulum_lqr", "dense")]
OWN_FORM = dict(boat_advanced="ident", pendulum="ident", double_integrator="band2", ros_boat="diag", pendulum_lqr="persample")


def _system(name):
    import lqrrt_amd
    if name == "ros_boat":
        return lqrrt_amd.systems.RosBoat("car")                   # S = diag(1,1,1,0,0,0): nodes that differ in velocity only tie
    if name == "double_integrator":
        return lqrrt_amd.systems.DoubleIntegrator(n_boxes=8, seed=0)
    return lqrrt_amd.systems.SYSTEMS[name](0)


def _dense(n, seed=5):
    A = np.random.RandomState(seed + n).uniform(-1, 1, (n, n))
    return A.dot(A.T) + n * np.eye(n)


class Bench(object):
    """One engine of a (system, S) variant with a hand-built tree: states only, K = 0, one-step edges."""

    def __init__(self, name, smode, capacity, max_wave=1024):
        from lqrrt_amd.engine import Engine
        self.name, self.smode = name, smode
        self.s = _system(name)
        self.n, self.m = self.s.nstates, self.s.ncontrols
        self.eng = Engine(self.s, capacity=capacity + 64, max_wave=max_wave)
        self.eng.set_resolution(self.s.plan_kwargs["dt"], 0.0, 2, np.abs(np.asarray(self.s.error_tol, dtype=np.float64)), None, None)
        self.form = OWN_FORM[name] if smode == "own" else "dense"
        self.S_call = None if smode == "own" else (np.eye(self.n) if smode == "eye" else _dense(self.n))
        self.exact = smode == "eye" and not self.s.wrap_dims
        self.model = None
        self.env = ()                    # launch_plan's (wg4_env, nn_waves, min_chunk) in a process that runs with forced forms

    def load(self, nodes, flags=None):
        N = len(nodes)
        pid = np.zeros(N, dtype=np.int32)
        pid[0] = -1
        self.eng.tree_load(nodes, np.zeros((N, self.m, self.n)), pid)
        self.model = R.ScanModel(nodes, self.s.wrap_dims)
        if flags is not None:
            self.flags(flags)

    def flags(self, flags):
        self.eng.set_ignored(np.asarray(flags, dtype=np.uint8))
        self.model.ign = np.array(flags, dtype=bool)

    def S_model(self, xs):
        """What the model contracts with: the caller's matrix, the system's constant S, or -- Riccati systems -- one matrix per query
        from lqr_dare_batch with the system's own Q, R, eps (that kernel has its own tests: tests/test_dare_gpu.py)."""
        if self.S_call is not None:
            return self.S_call
        if self.form == "persample":
            return self.eng.lqr_dare_batch(xs, np.zeros((len(xs), self.m)), self.s.Q, self.s.R, self.s.eps)[0]
        return None if self.s.S is None else np.asarray(self.s.S, dtype=np.float64)

    def ask(self, xs):
        return self.eng.nn_argmin(xs, self.S_call, use_ignore=True)

    def close(self):
        self.eng.close()


def _judge(b, rows, got, expect=None, what=""):
    """(ids, costs) of a batch against the model's cost rows.  expect: planted ids (-1: none planted for that query) -- asserted to be
    the model's own answers first, then demanded exactly."""
    m = b.model
    ids, cost = got
    ids = np.asarray(ids, dtype=np.int64)
    W = len(rows)
    assert ids.shape == (W,) and np.all((ids >= 0) & (ids < m.N)), (what, ids)
    want = m.answers(rows)
    t = np.arange(W)
    if expect is not None:
        expect = np.asarray(expect, dtype=np.int64)
        p = expect >= 0
        assert np.array_equal(want[p], expect[p]), "%s: the model does not select the planted nodes" % what
        assert np.array_equal(ids[p], expect[p]), (what, "planted", expect[p][ids[p] != expect[p]][:8], "got", ids[p][ids[p] != expect[p]][:8])
    cw, cg = rows[t, want], rows[t, ids]
    if b.exact:
        assert np.array_equal(ids, want) and np.array_equal(cost, cw), (what, "exact")
        return
    miss = ids != want
    gap = np.abs(cg - cw) / np.maximum(np.maximum(np.abs(cg), np.abs(cw)), 1e-300)
    assert np.all(gap[miss] < 1e-12), (what, "ids", ids[miss][:8], "model", want[miss][:8], "relative gap", gap[miss].max())
    if not m.ign.all():
        assert not m.ign[ids].any(), "%s: an ignored node was selected" % what
    assert np.all(np.abs(cost - cg) <= 1e-9 * np.maximum(1.0, cg)), (what, "cost", np.abs(cost - cg).max())


# ------------------------------------------------------------------------------------------------ a. self queries, exhaustive

def _self_nodes(b, N):
    return R.self_table(b.s, N, np.random.RandomState(7 * N + len(b.name)))


def _self_batches(N):
    """[(first, W)]: all N nodes in one call, then the last W of them."""
    return [(0, N)] + [(N - W, W) for W in R.W_CUTS if W < N]


def _run_self(b, judge):
    """Every node its own query, under the four ignore sets.  Returns {key: (ids, costs, planted ids or -1)}; judge(b, rows, got, expect, key) or None."""
    out, seen = {}, set()
    for N in R.SELF_SIZES:
        nodes = _self_nodes(b, N)
        b.load(nodes)
        rows = None
        if judge:
            rows = b.model.cost_rows(nodes, b.S_model(nodes))
            b.model.assert_rows_unique(rows, range(N))
        for sname, flags in R.self_ignore_sets(N):
            b.flags(flags)
            for first, W in _self_batches(N):
                plan = R.launch_plan(N, W, b.form, *b.env)
                seen.add(("xcd", plan["xcd"]))
                seen.add(("wg4", plan["wg4"]))
                seen.add(("partial last tile", N % plan["chunk"] != 0))
                seen.add(("padded lanes", W % 64 != 0))
                if plan["wg4"]:
                    seen.add(("last group", plan["last_group"]))
                key = "self/%d/%s/%d" % (N, sname, W)
                got = b.ask(nodes[first:])
                k = np.arange(first, N)
                expect = np.where(flags.all() | ~flags[k], k, -1)           # its own id unless it alone is ignored
                out[key] = (got[0], got[1], expect)
                if judge:
                    judge(b, rows[first:], got, expect, "%s %s %s" % (b.name, b.smode, key))
    return out, seen


@pytest.mark.parametrize("name,smode", VARIANTS)
def test_self_queries(name, smode):
    """N at the quad, tile, chunk and XCD-toggle edges; W = N and W cut to 1 .. 129 queries from the end of the table (winners in the
    last, partial tile; clamped lanes in the last wavefront); every node ignored: the fallback still answers k."""
    b = Bench(name, smode, 1024)
    _, seen = _run_self(b, _judge)
    assert {("xcd", True), ("xcd", False), ("partial last tile", True), ("partial last tile", False),
            ("padded lanes", True), ("padded lanes", False)} <= seen
    assert R.launch_plan(128, 64, b.form)["xcd"] and not R.launch_plan(144, 64, b.form)["xcd"]
    b.close()


# ------------------------------------------------------------------------------------------------ b. periodic ties

def _tie_base(b, s, N):
    return R.self_table(b.s, s, np.random.RandomState(13 * s + N + len(b.name)))


def _run_ties(b, N, periods, judge):
    out = {}
    for s in periods:
        base = _tie_base(b, s, N)
        nodes = R.periodic_table(base, N)
        b.load(nodes)
        res = R.tie_residues(s)
        xs = base[res]
        rows = b.model.cost_rows(xs, b.S_model(xs)) if judge else None
        full = {}
        for sname, flags in R.tie_ignore_sets(N, s):
            b.flags(flags)
            key = "tie/%d/%d/%s" % (N, s, sname)
            got = b.ask(xs)
            if sname == "all":
                expect = np.array(res)                                     # the overall first: the lowest copy
            else:
                expect = np.array([-1 if j is None else j for j in (R.lowest_congruent(N, s, r, flags) for r in res)])
            out[key] = (got[0], got[1], expect)
            if not judge:
                continue
            judge(b, rows, got, expect, "%s %s %s" % (b.name, b.smode, key))
            for t in range(len(xs)):                                       # the returned cost IS the device's cost of that node
                if t not in full:
                    full[t] = b.eng.costs_to_go(xs[t], b.S_call)
                assert got[1][t] == full[t][got[0][t]], (key, t, got[1][t], full[t][got[0][t]])
    return out


@pytest.mark.parametrize("N", R.TIE_SIZES)
@pytest.mark.parametrize("name,smode", VARIANTS)
def test_periodic_ties(name, smode, N):
    """nodes[j] = base[j % s]: the copies of a query's node have bit-equal costs in every quad, tile, chunk, reduce lane and stride,
    so the lowest eligible copy is THE answer."""
    b = Bench(name, smode, N)
    plan = R.launch_plan(N, 64, b.form)
    assert plan["reduce_stride"] and not plan["wg4"]                        # more than 64 partials per query
    assert plan["parts"] == (65 if N == 1025 else 684)
    _run_ties(b, N, sorted(set(R.PERIODS)), _judge)
    b.close()


def test_diagonal_S_ties_between_nodes_that_differ():
    """ros_boat 'car', S = diag(1,1,1,0,0,0) (the S_DIAG form): nodes that share position and heading and differ in velocity cost the
    same bit for bit -- in the kernel the skipped terms, in the model products with zero -- for a query on their position (cost 0)
    and for one beside it (cost > 0), whatever the query's own velocity.  The lowest eligible copy is the answer, exactly."""
    N = 1025
    b = Bench("ros_boat", "own", N)
    assert b.form == "diag" and R.launch_plan(N, 64, b.form)["reduce_stride"]
    S = b.S_model(None)
    assert np.array_equal(np.diag(S), [1, 1, 1, 0, 0, 0])
    for s in R.DIAG_PERIODS:
        rs = np.random.RandomState(500 + s)
        base = R.self_table(b.s, s, rs)
        nodes = R.velocity_table(b.s, base, N, (3, 4, 5), rs)
        assert len(np.unique(nodes, axis=0)) == N
        b.load(nodes)
        res = R.tie_residues(s)
        xs = R.velocity_queries(b.s, base, res, rs)
        rows = b.model.cost_rows(xs, S)
        for t, c in enumerate(rows):                                      # bit-equal in the model, zero only ON the position
            r = res[t % len(res)]
            assert np.all(c[r::s] == c[r]) and (c[r] == 0.0) == (t < len(res)) and c[r] == c.min()
        for sname, flags in R.tie_ignore_sets(N, s):
            b.flags(flags)
            got = b.ask(xs)
            if sname == "all":
                expect = np.array(res + res)
            else:
                expect = np.array([-1 if j is None else j for j in (R.lowest_congruent(N, s, r, flags) for r in res + res)])
            _judge(b, rows, got, expect, "ros_boat velocity ties s=%d %s" % (s, sname))
            for t in range(len(xs)):
                assert got[1][t] == b.eng.costs_to_go(xs[t])[got[0][t]], (s, sname, t)
    b.close()


# ------------------------------------------------------------------------------------------------ c. the natural WPB = 4 table

@pytest.mark.parametrize("name,smode", [("boat_advanced", "own"), ("double_integrator", "own"), ("boat_advanced", "dense")])
def test_default_four_wavefront_table(name, smode):
    N = R.BIG_N
    b = Bench(name, smode, N, max_wave=128)
    plan = R.launch_plan(N, 64, b.form)
    assert (plan["chunk"], plan["n_sub"], plan["wg4"], plan["parts"], plan["last_group"]) == (40, 821, True, 206, 1)
    assert R.launch_plan(N, 72, b.form)["wg4"]
    _run_ties(b, N, R.BIG_PERIODS, _judge)
    nodes = R.self_table(b.s, N, np.random.RandomState(99))
    ids = np.array([0, 39, 40, 159, 160] + list(range(N - 38, N)))
    b.load(nodes)
    xs = nodes[ids]
    rows = b.model.cost_rows(xs, b.S_model(xs))
    b.model.assert_rows_unique(rows, ids)
    for sname, flags in R.self_ignore_sets(N):
        b.flags(flags)
        expect = np.where(flags.all() | ~flags[ids], ids, -1)
        _judge(b, rows, b.ask(xs), expect, "%s %s big self %s" % (name, smode, sname))
    b.close()


# ------------------------------------------------------------------------------------------------ d. forced forms in child processes

FORCED = {"wg4": dict(LQRRT_NN_WG4="1", LQRRT_NN_MIN_CHUNK="8"), "wide": dict(LQRRT_NN_WG4="0", LQRRT_NN_WAVES="64")}
FORCED_PLAN = {"wg4": (1, 0, 8), "wide": (0, 64, 16)}                     # launch_plan's (wg4_env, nn_waves, min_chunk)
_small_cache = {}


def _run_small(judge, env=(), seen_by_form=None):
    """Cases (a) and (b) at N <= 1025 for every variant: {variant/key: (ids, costs, planted ids)}.  env: the forced launch form of
    this process; seen_by_form: collects what the restated plan says the self queries reached, per form of S."""
    out = {}
    for name, smode in VARIANTS:
        b = Bench(name, smode, 1025)
        b.env = env
        got, seen = _run_self(b, judge)
        if seen_by_form is not None:
            seen_by_form.setdefault(b.form, set()).update(seen)
        got.update(_run_ties(b, 1025, sorted(set(R.PERIODS)), judge))
        b.close()
        for k, v in got.items():
            out["%s/%s/%s" % (name, smode, k)] = v
    return out


def _child_main(forced):
    seen = {}
    out = _run_small(None, FORCED_PLAN[forced], seen)
    assert sorted(seen) == sorted(R.FORMS)
    for form, reached in seen.items():                                    # this process reaches the paths it was started for
        if forced == "wg4" and form in R.WG4_FORMS:                       # WPB = 4 from 8 chunks on, full and partial last groups
            assert {("wg4", True), ("wg4", False), ("last group", 1), ("last group", 4), ("xcd", True), ("xcd", False)} <= reached, (form, reached)
        else:
            assert ("wg4", True) not in reached, (form, reached)
    buf = io.BytesIO()
    flat = {}
    for k, (ids, cost, _) in out.items():
        flat["i:" + k] = np.asarray(ids, dtype=np.int32)
        flat["c:" + k] = np.asarray(cost, dtype=np.float64)
    np.savez(buf, **flat)
    sys.stdout.write("\nARRAYS " + base64.b64encode(buf.getvalue()).decode() + "\n")


@pytest.mark.parametrize("forced", sorted(FORCED))
def test_forced_launch_forms_same_bits(forced):
    """LQRRT_NN_WG4=1 with 8-node chunks (WPB = 4 from 8 chunks on, partial last groups) and LQRRT_NN_WG4=0 with 64 wavefronts per
    launch (long chunks, few partials), each in a process of its own (the switches are read once): the bits of the default form."""
    wg4_env, nn_waves, min_chunk = FORCED_PLAN[forced]
    env_plan = (wg4_env, nn_waves, min_chunk)
    if forced == "wg4":
        p = R.launch_plan(1025, 64, "ident", *env_plan)
        assert p["wg4"] and p["n_sub"] >= 8 and p["last_group"] == 1       # a last four-chunk group that is partial
        p = R.launch_plan(1024, 64, "dense", *env_plan)
        assert p["wg4"] and p["last_group"] == 4 and p["xcd"]
        assert R.launch_plan(65, 64, "band2", *env_plan)["last_group"] == 1 and not R.launch_plan(5, 5, "ident", *env_plan)["wg4"]
        assert not R.launch_plan(1025, 64, "persample", *env_plan)["wg4"] and not R.launch_plan(1025, 64, "diag", *env_plan)["wg4"]
    else:
        p = R.launch_plan(1025, 64, "ident", *env_plan)
        assert not p["wg4"] and p["parts"] == 43 and not p["reduce_stride"]
    if not _small_cache:                                                   # the in-process answers, judged against the model
        _small_cache.update(_run_small(_judge))
    env = dict(os.environ)
    for k in ("LQRRT_NN_WG4", "LQRRT_NN_MIN_CHUNK", "LQRRT_NN_WAVES"):
        env.pop(k, None)
    env.update(FORCED[forced])
    code = "import sys; sys.path[:0] = [%r, %r, %r]; import test_nn_scan_gpu as T; T._child_main(%r)" % (
        os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "oracle"), forced)
    run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    line = [l for l in run.stdout.splitlines() if l.startswith("ARRAYS ")][-1]
    child = np.load(io.BytesIO(base64.b64decode(line.split()[1])))
    assert len(child.files) == 2 * len(_small_cache)
    planted = 0
    for k, (ids, cost, expect) in _small_cache.items():
        assert np.array_equal(child["i:" + k], ids), (forced, k)
        assert np.array_equal(child["c:" + k], cost), (forced, k)
        p = expect >= 0                                                    # (the planted ids once more: _judge held them to the model)
        assert np.array_equal(child["i:" + k][p], expect[p]), (forced, k)
        planted += int(np.count_nonzero(p))
    assert planted > 100000


# ------------------------------------------------------------------------------------------------ e. angle modes

SPECIAL = [0.0, np.pi, -np.pi, np.pi - 1e-12, 100.0, -100.0, 0.5, 0.5 + np.pi, -2.0, -2.0 + np.pi]


def _angle_table(b, N, rs):
    nodes = R.self_table(b.s, N, rs)
    wd = list(b.s.wrap_dims)
    for i in range(0, N, 5):                                              # a fifth of the nodes: special angles
        for d in wd:
            nodes[i, d] = SPECIAL[rs.randint(len(SPECIAL))]
    for k, v in enumerate(SPECIAL):                                       # and each of them in the first tile, on every wrapped state
        nodes[k, wd] = v
    return nodes


def _sampler(b, fixed):
    """set_sampler with the wrapped dimensions in `fixed` {dim: angle} pinned (zero span, zero goal bias) and the others free."""
    lo, hi = R.widened_space(b.s)
    centers, spans = 0.5 * (lo + hi), hi - lo
    bias = np.array(b.s.goal_bias, dtype=np.float64)
    for d in b.s.wrap_dims:
        bias[d] = 0.0
        if d in fixed:
            centers[d], spans[d] = fixed[d], 0.0
        else:
            spans[d] = max(spans[d], 1.0)
    b.eng.set_sampler(centers, spans, bias, 10)


def _with_decoys(b, xs, decoy_angle):
    """The queries in wavefronts of 63 plus one query of another angle: every wavefront runs in mode 0.  Returns (ids, costs) of xs."""
    wd = list(b.s.wrap_dims)
    batch, keep = [], []
    for lo in range(0, len(xs), 63):
        part = xs[lo:lo + 63]
        decoy = part[0].copy()
        decoy[wd] = decoy_angle
        keep += list(range(len(batch), len(batch) + len(part)))
        batch += list(part) + [decoy]
        while len(batch) % 64:                                             # (a short last part: fill the wavefront with decoys)
            batch.append(decoy)
    batch = np.array(batch)
    assert set(R.angle_mode(batch, b.s.wrap_dims)) == {0}
    ids, cost = b.ask(batch)
    return ids[keep], cost[keep]


@pytest.mark.parametrize("name,fixes", [("boat_advanced", [(2,), ()]), ("pendulum", [(0, 1), (0,), ()])])
def test_angle_modes_same_bits(name, fixes):
    """One atan2 per pair (mode 0), one per node and wavefront pulled out of lanes (mode 1), the tree's table of errors to the
    sampler's fixed angles (mode 2): systems.hpp wrap_err_c and nn_scan.hpp claim the same bits.  63 queries that share their angles
    run in mode 2 on an engine whose sampler fixes exactly those angles, in mode 1 on one that fixes fewer or none, and in mode 0
    next to one query of another angle."""
    rs = np.random.RandomState(21)
    N = 1025
    b = Bench(name, "own", N)
    nodes = _angle_table(b, N, rs)
    b.load(nodes)
    wd = list(b.s.wrap_dims)
    lo, hi = R.widened_space(b.s)
    seen = set()
    for ang in (0.0, np.pi, -np.pi, np.pi - 1e-12, 100.0, -100.0, 0.5, -2.0, 0.3):   # 0.5 / -2.0: nodes exactly pi away exist
        xs = lo + (hi - lo) * rs.random_sample((63, b.n))
        xs[:, wd] = ang
        xs[0] = nodes[SPECIAL.index(ang)] if ang in SPECIAL else xs[0]     # (one self query where a node carries the angle)
        xs[0, wd] = ang
        rows = b.model.cost_rows(xs, None)
        ref = _with_decoys(b, xs, ang + 0.7)
        _judge(b, rows, ref, None, "%s mode 0 angle %r" % (name, ang))
        for fix in fixes:
            _sampler(b, {d: ang for d in fix})
            fixed = [ang] * len(wd) if len(fix) == len(wd) else None         # (fewer than all pinned: FixedAngles::on is off)
            mode = R.angle_mode(xs, b.s.wrap_dims, fixed)
            assert mode == [2 if fixed else 1]
            seen.add((len(fix), mode[0]))
            got = b.ask(xs)
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (name, ang, fix, mode)
            if fixed:                                                      # modes 2, 1 and 0 in ONE launch
                other = xs.copy()
                other[:, wd] = ang - 0.4
                mixed = lo + (hi - lo) * rs.random_sample((64, b.n))
                three = np.vstack((xs, xs[:1], other, other[:1], mixed))
                assert len(three) == 192 and R.angle_mode(three, b.s.wrap_dims, fixed) == [2, 1, 0]
                g3 = b.ask(three)
                r3 = _with_decoys(b, three, ang + 0.7)
                assert np.array_equal(g3[0], r3[0]) and np.array_equal(g3[1], r3[1]), (name, ang, "three modes")
                assert np.array_equal(g3[0][:63], ref[0]) and np.array_equal(g3[1][:63], ref[1])
                _judge(b, b.model.cost_rows(three, None), g3, None, "%s three modes angle %r" % (name, ang))
    assert seen == {(len(f), 2 if len(f) == len(wd) else 1) for f in fixes}
    b.close()


# ------------------------------------------------------------------------------------------------ f. no stale angle-error rows

def _append(b, parent, state):
    from lqrrt_amd import _native as nat
    state = nat.as_f64(state, (b.n,))
    K = np.zeros((b.m, b.n))
    nat.check(nat.lib().lqrrt_tree_append(b.eng.h, int(parent), nat.ptr(state), nat.ptr(K), 1, None, None, b.eng._stream()))
    b.model = R.ScanModel(np.vstack((b.model.nodes, state)), b.s.wrap_dims, np.append(b.model.ign, False))


@pytest.mark.parametrize("name", ["boat_advanced", "pendulum"])
def test_no_stale_angle_error_rows(name):
    """TreeView::werr (mode 2) after everything that changes the tree or the fixed angles behind it: each step is answered for the
    CURRENT tree and the CURRENT angles, self queries of the newest nodes included."""
    rs = np.random.RandomState(33)
    b = Bench(name, "own", 1024)
    wd = list(b.s.wrap_dims)
    lo, hi = R.widened_space(b.s)

    def draw(count, ang=None):
        x = lo + (hi - lo) * rs.random_sample((count, b.n))
        if ang is not None:
            x[:, wd] = ang
        return x

    def verify(ang, newest, step):
        """63 queries at the fixed angle `ang`: random ones and the newest nodes' states turned to that angle; then the newest nodes
        that carry the angle themselves as their own queries."""
        m = b.model
        assert b.eng.size == m.N
        np.testing.assert_array_equal(b.eng.states(), m.nodes)
        m.ign = b.eng.ignored()
        near = m.nodes[newest[-31:]].copy()
        near[:, wd] = ang
        xs = np.vstack((draw(63 - len(near), ang), near))
        assert R.angle_mode(xs, b.s.wrap_dims, [ang] * len(wd)) == [2]
        _judge(b, m.cost_rows(xs, None), b.ask(xs), None, "%s %s" % (name, step))
        own = [i for i in newest if np.all(m.nodes[i, wd] == ang) and not m.ign[i]][-63:]
        assert own, step
        xs = m.nodes[own]
        rows = m.cost_rows(xs, None)
        m.assert_rows_unique(rows, own)
        assert R.angle_mode(xs, b.s.wrap_dims, [ang] * len(wd)) == [2]
        _judge(b, rows, b.ask(xs), np.array(own), "%s %s (own)" % (name, step))

    def grow(count, ang):
        """Appends `count` nodes below random parents, every second one at the angle `ang`; returns their ids."""
        first = b.model.N
        for k in range(count):
            _append(b, rs.randint(0, b.model.N), draw(1, ang if k % 2 == 0 else None)[0])
        return list(range(first, first + count))

    a1, a2 = 0.3, -1.1
    _sampler(b, {d: a1 for d in wd})
    # 1. tree_load
    N = 500
    nodes = draw(N)
    nodes[N - 40:, wd] = a1
    pid = np.concatenate(([-1], [rs.randint(0, i) for i in range(1, N)])).astype(np.int32)
    b.eng.tree_load(nodes, np.zeros((N, b.m, b.n)), pid)
    b.model = R.ScanModel(nodes, b.s.wrap_dims)
    verify(a1, list(range(N - 40, N)), "1 load")
    #    ... and another table loaded over the valid rows of the first, asked before anything else touches the tree
    nodes = draw(N)
    nodes[N - 50:, wd] = a1
    b.eng.tree_load(nodes, np.zeros((N, b.m, b.n)), pid)
    b.model = R.ScanModel(nodes, b.s.wrap_dims)
    verify(a1, list(range(N - 50, N)), "1 second load")
    # 2. truncate, then appends over the old ids
    b.eng.tree_truncate(300)
    b.model = R.ScanModel(nodes[:300], b.s.wrap_dims)
    new = []
    for k in range(6):                                                    # ask after every append ...
        new += grow(1, a1)
        verify(a1, new, "2 truncate + append %d" % k)
    new += grow(150, a1)                                                  # ... and after many: ids 300..455 cover old rows
    verify(a1, new, "2 truncate + appends")
    at_a2 = grow(10, a2)                                                  # (nodes at the next fixed angle, for step 3)
    verify(a1, new, "2 more appends")
    # 3. another fixed angle: asked straight after the sampler call, then again after appends
    _sampler(b, {d: a2 for d in wd})
    verify(a2, at_a2, "3 other fixed angle")
    new = grow(8, a2)
    verify(a2, new, "3 other fixed angle + appends")
    # 4. a free angle, appends meanwhile, and back
    _sampler(b, {})
    free = draw(63, a2)
    assert R.angle_mode(free, b.s.wrap_dims, None) == [1]
    _judge(b, b.model.cost_rows(free, None), b.ask(free), None, "%s 4 free" % name)
    new = grow(9, a2)
    _sampler(b, {d: a2 for d in wd})
    verify(a2, new, "4 free and back")
    _sampler(b, {d: a1 for d in wd})
    verify(a1, list(range(300, 340)), "4 back to the first angle")
    # 5. retain a subtree (no revalidation): the kept nodes move to new ids
    from lqrrt_amd import _native as nat
    par = b.eng.parents()
    at_a1 = np.all(b.model.nodes[:, wd] == a1, axis=1)

    def subtree(root):
        below = np.zeros(len(par), dtype=bool)
        below[root] = True
        for i in range(root + 1, len(par)):
            below[i] = below[par[i]]
        return below
    root = max(range(1, 60), key=lambda r: int(np.count_nonzero(subtree(r) & at_a1)))   # the early node with most a1 nodes below it
    below = subtree(root)
    stats, old_to_new = b.eng.tree_retain(root, revalidate=False)
    kept = np.flatnonzero(below)
    assert 8 < len(kept) < len(par) and stats["kept"] == len(kept)
    np.testing.assert_array_equal(old_to_new[kept], np.arange(len(kept)))
    assert np.all(old_to_new[~below] == -1)
    b.model = R.ScanModel(b.model.nodes[kept], b.s.wrap_dims)
    moved = [int(i) for i in np.flatnonzero(at_a1[kept]) if kept[i] != i]
    assert len(moved) >= 3                                                # kept nodes at a1 whose ids changed: asked before any append
    verify(a1, moved, "5 retain")
    new = grow(12, a1)
    verify(a1, new, "5 retain + appends")
    # 6. reset: the seed as its own query before anything is appended, then appends
    x0 = draw(1, a1)[0]
    b.eng.tree_reset(x0)
    b.model = R.ScanModel(x0[None, :], b.s.wrap_dims)
    verify(a1, [0], "6 reset")
    new = [0] + grow(70, a1)
    verify(a1, new, "6 reset + appends")
    assert nat.lib().lqrrt_tree_size(b.eng.h) == 71
    b.close()


# ------------------------------------------------------------------------------------------------ g. one S per query

def test_per_sample_S_is_the_querys_own():
    """pendulum_lqr: query t is contracted with matrix t (Sd + t * s_stride), in the scan and in the every-node-ignored fallback.  The
    64 queries are spread over the whole sample space, so their Riccati solutions differ strongly: the model with the matrices
    shifted by one query selects other nodes."""
    rs = np.random.RandomState(44)
    N = 1025
    b = Bench("pendulum_lqr", "own", N)
    assert b.form == "persample"
    lo, hi = R.widened_space(b.s)
    nodes = R.self_table(b.s, N, rs)
    b.load(nodes)
    xs = lo + (hi - lo) * rs.random_sample((64, b.n))
    S = b.S_model(xs)
    assert S.shape == (64, b.n, b.n)
    spread = [np.linalg.norm(S[t] - S[t - 1]) / np.linalg.norm(S[t]) for t in range(64)]
    assert min(spread) > 1e-3 and max(spread) > 0.1, (min(spread), max(spread))
    rows = b.model.cost_rows(xs, S)
    shifted = b.model.cost_rows(xs, np.roll(S, 1, axis=0))
    assert np.count_nonzero(b.model.answers(rows) != b.model.answers(shifted)) >= 8      # a scan that reads another query's S shows
    first = b.model.cost_rows(xs, np.repeat(S[:1], 64, axis=0))                          # ... and so does one that reads query 0's
    assert np.count_nonzero(b.model.answers(rows) != b.model.answers(first)) >= 8
    assert np.count_nonzero(np.abs(first.min(axis=1) - rows.min(axis=1)) > 1e-6 * rows.min(axis=1)) >= 56
    for sname, flags in R.self_ignore_sets(N) + [("half", rs.random_sample(N) < 0.5)]:
        b.flags(flags)
        got = b.ask(xs)
        _judge(b, rows, got, None, "pendulum_lqr per-sample S %s" % sname)
        for t in (0, 1, 63):
            c = b.eng.costs_to_go(xs[t])
            assert got[1][t] == c[got[0][t]], (sname, t)
    b.close()


# ------------------------------------------------------------------------------------------------ h. host form

@pytest.mark.parametrize("name,smode", [("boat_advanced", "own"), ("boat_advanced", "dense"), ("pendulum", "own"),
                                        ("double_integrator", "own"), ("pendulum_lqr", "own"), ("pendulum_lqr", "dense")])
def test_host_form_is_the_batched_form(name, smode):
    """lqrrt_nn_argmin_host on a compiled-in engine returns the bits of lqrrt_nn_argmin with W = 1: on an engine whose sampler fixes
    the query's angles (mode 2) and on a free one (mode 1), with and without S_host, with and without the ignore set."""
    from lqrrt_amd import _native as nat
    rs = np.random.RandomState(55)
    N = 1025
    b = Bench(name, smode, N)
    wd = list(b.s.wrap_dims)
    nodes = R.self_table(b.s, N, rs)
    b.load(nodes, rs.random_sample(N) < 0.4)
    lo, hi = R.widened_space(b.s)
    ang = 0.25
    xs = lo + (hi - lo) * rs.random_sample((6, b.n))
    xs[:, wd] = ang
    rows = b.model.cost_rows(xs, b.S_model(xs))
    S_host = None if b.S_call is None else nat.as_f64(b.S_call, (b.n, b.n))
    Sp = None if S_host is None else nat.ptr(S_host)
    for fix in ([{d: ang for d in wd}, {}] if wd else [{}]):
        _sampler(b, fix)
        for x in xs:
            assert R.angle_mode(x[None, :], b.s.wrap_dims, [ang] * len(wd) if fix else None) == ([2 if fix else 1] if wd else [0])
        for use_ignore in (True, False):
            ids, cost = b.eng.nn_argmin(xs, b.S_call, use_ignore=use_ignore)
            if use_ignore:
                _judge(b, rows, (ids, cost), None, "%s %s host form" % (name, smode))
            for t, x in enumerate(xs):
                one = b.eng.nn_argmin(x[None, :], b.S_call, use_ignore=use_ignore)
                hid, hc = C.c_int32(-1), C.c_double(-1.0)
                xh = nat.as_f64(x, (b.n,))
                nat.check(nat.lib().lqrrt_nn_argmin_host(b.eng.h, nat.ptr(xh), Sp, 1 if use_ignore else 0, C.byref(hid), C.byref(hc),
                                                         b.eng._stream()))
                assert (hid.value, hc.value) == (int(one[0][0]), float(one[1][0])), (name, smode, bool(fix), use_ignore, t)
                assert (hid.value, hc.value) == (int(ids[t]), float(cost[t])), (name, smode, bool(fix), use_ignore, t)
    b.close()
