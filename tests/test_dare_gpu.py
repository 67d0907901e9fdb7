"""
GPU: lqrrt_lqr_dare_batch (finite-difference linearisation + doubling DARE on the device) against
SciPy.  The reference has no Riccati solver, so the golden for this build-added
operator is scipy.linalg.solve_discrete_are on Jacobians obtained from the ORACLE's dynamics with the
same central-difference step.  Tolerances: Jacobians 2e-7 (difference quotients), S and K 1e-8
relative to scipy on the device's own Jacobians (1e-6 for the 1 ms double pendulum, |S| ~ 1e9).

Below that first test, the solver at its pivot, size and iteration edges.  The kernel sums in a fixed order inside one lane and
is built without contraction, so the reference for everything after the linearisation is the plain sequential restatement
tests/dare_reference.py dare_solve run on the DEVICE'S OWN A, B, and the bar is equality of bits (S, K) and of the iteration
count -- never a tolerance.  tests/test_dare_cpu.py pins that restatement to the C oracle's orc_dare_solve and to 60-digit
arithmetic, and shows on the CPU that the case table exchanges rows and meets exact ties where it says; the same coverage
conditions are asserted again here from the runs on the device's matrices.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg

import dare_reference as D

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["boat_novice", "car", "double_integrator", "pendulum"])
def test_dare_batch_vs_scipy(name):
    import lqrrt_amd
    from systems_np import SYSTEMS
    s = lqrrt_amd.systems.SYSTEMS[name]() if name == "double_integrator" else lqrrt_amd.systems.SYSTEMS[name](0)
    rs = SYSTEMS[name]() if name == "double_integrator" else SYSTEMS[name](0)
    dt = s.plan_kwargs["dt"]
    eng = s._engine(dt)
    n, m = s.nstates, s.ncontrols
    rng = np.random.RandomState(0)
    Bn = 24
    if name == "pendulum":
        x = rng.uniform(-1, 1, (Bn, n))
        u = rng.uniform(-5, 5, (Bn, m))
    elif name == "double_integrator":
        x = rng.uniform(0, 50, (Bn, n))
        u = rng.uniform(-1, 1, (Bn, m))
    else:
        x = np.zeros((Bn, n))
        x[:, :2] = rng.uniform(0, 40, (Bn, 2))
        x[:, 2] = rng.uniform(-3, 3, Bn)
        x[:, 3] = rng.uniform(0.3, 1.0, Bn)                    # moving forward: heading stays controllable
        x[:, 4:] = rng.uniform(-0.1, 0.1, (Bn, n - 4))
        u = rng.uniform(-50, 50, (Bn, m))                       # inside the actuator limits (smooth region)
    Q, R = np.eye(n), np.eye(m) * (1e-4 if name in ("boat_novice", "car") else 1.0)
    eps = 1e-6
    S, K, A, B, it = eng.lqr_dare_batch(x, u, Q, R, eps=eps)
    assert it.max() <= 40
    for i in range(Bn):
        A_ref, B_ref = D.linearise_np(rs.dynamics, x[i], u[i], dt, eps)
        np.testing.assert_allclose(A[i], A_ref, rtol=0, atol=2e-7)
        np.testing.assert_allclose(B[i], B_ref, rtol=0, atol=2e-7)
        S_ref = scipy.linalg.solve_discrete_are(A[i], B[i], Q, R)
        K_ref = np.linalg.solve(R + B[i].T @ S_ref @ B[i], B[i].T @ S_ref @ A[i])
        scale = np.abs(S_ref).max()
        rtol = 1e-6 if name == "pendulum" else 1e-8          # dt = 1 ms makes the pendulum's DARE ill-conditioned (|S| ~ 1e9)
        assert np.abs(S[i] - S_ref).max() <= rtol * scale
        assert np.abs(K[i] - K_ref).max() <= rtol * max(1.0, np.abs(K_ref).max())
        np.testing.assert_allclose(S[i], S[i].T, rtol=0, atol=1e-12 * scale)
        # Riccati residual of the device solution
        res = A[i].T @ S[i] @ A[i] - S[i] - (A[i].T @ S[i] @ B[i]) @ K[i] + Q
        assert np.abs(res).max() <= (1e-5 if name == "pendulum" else 1e-7) * scale
    if name == "double_integrator":
        # host doubling on the EXACT A, B (lqrrt_amd/dare.py) agrees up to the difference-quotient noise
        # of the device Jacobians (|x| ~ 50, eps = 1e-6 -> ~5e-9 per entry)
        np.testing.assert_allclose(S[0], s.S, rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(K[0], s.K, rtol=1e-6, atol=1e-6)


# ================================================================================================ edges of the solver

EPS = 1e-6
_pairs, _runs = {}, {}


def _pair(name):
    """(lqrrt_amd system, NumPy twin, operator engine at the system's dt), one per session."""
    if name not in _pairs:
        import lqrrt_amd
        from systems_np import SYSTEMS
        if name == "double_integrator":
            s, rs = lqrrt_amd.systems.SYSTEMS[name](), SYSTEMS[name]()
        else:
            s, rs = lqrrt_amd.systems.SYSTEMS[name](0), SYSTEMS[name](0)
        _pairs[name] = (s, rs, s._engine(s.plan_kwargs["dt"]))
    return _pairs[name]


def _same_bits(got, want, what):
    """(S, K, iterations) against (S, K, iterations): NaN positions count as equal, everything else bit for bit."""
    np.testing.assert_array_equal(got[0], want[0], err_msg="S of %s" % (what,))
    np.testing.assert_array_equal(got[1], want[1], err_msg="K of %s" % (what,))
    assert int(got[2]) == int(want[2]), ("iterations of %s" % (what,), int(got[2]), int(want[2]))


def _alone(eng, x, u, Q, R, eps=EPS):
    """[(S, K, iterations)] of every item solved in a launch of its own."""
    out = []
    for i in range(len(x)):
        S, K, _, _, it = eng.lqr_dare_batch(x[i:i + 1], u[i:i + 1], Q, R, eps=eps)
        out.append((S[0], K[0], it[0]))
    return out


def _device_runs(name):
    """[(label, i, Q, R, device (S, K, A, B, it) of item i, dare_solve on the device's A, B)] over the system's case table."""
    if name not in _runs:
        eng = _pair(name)[2]
        x, u = D.case_states(name)
        out = []
        for label, Q, R in D.cases_for(name):
            S, K, A, B, it = eng.lqr_dare_batch(x, u, Q, R, eps=EPS)
            for i in range(len(x)):
                out.append((label, i, Q, R, (S[i], K[i], A[i], B[i], it[i]), D.dare_solve(A[i], B[i], Q, R)))
        _runs[name] = out
    return _runs[name]


# ------------------------------------------------------------------------------------------------ a. solver, bit for bit

@pytest.mark.parametrize("name", D.SYSTEM_NAMES)
def test_solver_equals_restatement_bit_for_bit(name):
    """Every (Q, R) of the case table at four interior states: S, K and the iteration count of the device equal the sequential
    restatement on the device's own A, B; S is exactly symmetric; the iteration converged."""
    for label, i, Q, R, (S, K, A, B, it), ref in _device_runs(name):
        _same_bits((S, K, it), ref, (name, label, i))
        np.testing.assert_array_equal(S, S.T)
        assert 1 <= it < 64, (name, label, i, it)


def test_device_matrices_reach_the_pivots_the_table_claims():
    """The coverage conditions of tests/test_dare_cpu.py once more, from the pivot logs of the runs above: row exchanges at p = 0
    and at a later p at each of the three eliminations, on the register path and on the fallback; an exact tie that keeps row p;
    an exact tie between two lower rows.  If the device's A, B shifted a pattern, this fails."""
    D.check_coverage([(D.DIMS[name][0], label, R, ref[3]) for name in D.SYSTEM_NAMES for label, _, _, R, _, ref in _device_runs(name)])


@pytest.mark.parametrize("name", ["pendulum_lqr", "boat_novice_lqr"])
def test_riccati_systems_equal_the_oracle_lqr(name):
    """The two Riccati systems at their own Q, R, eps: linearisation AND solver equal the C oracle's lqr(x, u) bit for bit.
    (The boat's lqr linearises about (x, 0) whatever u is: the operator gets zeros.)"""
    import coracle
    s, _, eng = _pair(name)
    o = coracle.make(s, 16)
    x, u = D.case_states(name, 6, seed=1)
    u_lin = np.zeros_like(u) if name == "boat_novice_lqr" else u
    S, K, _, _, it = eng.lqr_dare_batch(x, u_lin, s.Q, s.R, eps=s.eps)
    for i in range(len(x)):
        _same_bits((S[i], K[i], it[i]), o.lqr(x[i], u[i]), (name, i))


# ------------------------------------------------------------------------------------------------ b. linearisation at its edges

@pytest.mark.parametrize("name", D.SYSTEM_NAMES)
def test_linearisation_at_wraps_branches_and_clamps(name):
    """A, B against NumPy central differences of the systems_np dynamics at 2e-7: an angle within eps of +-pi and one beyond pi,
    forward speed exactly 0, efforts exactly at the actuator limits and far beyond them."""
    s, rs, eng = _pair(name)
    n, m = D.DIMS[name]
    edges = D.linearisation_edges(name, getattr(rs, "u_max", None))
    x, u = np.array([e[1] for e in edges]), np.array([e[2] for e in edges])
    _, _, A, B, _ = eng.lqr_dare_batch(x, u, np.eye(n), np.eye(m), eps=EPS)
    for i, (label, xi, ui) in enumerate(edges):
        A_ref, B_ref = D.linearise_np(rs.dynamics, xi, ui, s.plan_kwargs["dt"], EPS)
        np.testing.assert_allclose(A[i], A_ref, rtol=0, atol=2e-7, err_msg="A of %s, %s" % (name, label))
        np.testing.assert_allclose(B[i], B_ref, rtol=0, atol=2e-7, err_msg="B of %s, %s" % (name, label))
        if label == "efforts beyond the limit" and name != "pendulum" and name != "pendulum_lqr":
            assert np.all(B[i] == 0.0), (name, "a clamped effort has slope exactly 0")


@pytest.mark.parametrize("name", D.SYSTEM_NAMES)
def test_linearisation_step_sizes(name):
    """eps in {1e-4, 1e-6, 1e-8} at 2e-13 / eps: device and NumPy form the same difference quotient, so they differ by the
    rounding of values of order one divided by 2 eps, not by the truncation error.  Measured on the CPU between the C oracle's
    dynamics (the device's arithmetic) and the NumPy twin at eight such states per system: at most 5.6e-13, 5.6e-11 and 5.6e-9
    (the pendulums; boat_advanced 3.0e-13, 5.6e-11, 1.7e-9; the others 0), i.e. 5.6e-17 / eps against the bound's 2e-13 / eps."""
    s, rs, eng = _pair(name)
    n, m = D.DIMS[name]
    x, u = D.case_states(name, 8, seed=2)
    for eps in (1e-4, 1e-6, 1e-8):
        _, _, A, B, _ = eng.lqr_dare_batch(x, u, np.eye(n), np.eye(m), eps=eps)
        for i in range(len(x)):
            A_ref, B_ref = D.linearise_np(rs.dynamics, x[i], u[i], s.plan_kwargs["dt"], eps)
            np.testing.assert_allclose(A[i], A_ref, rtol=0, atol=2e-13 / eps, err_msg="A of %s, eps %g" % (name, eps))
            np.testing.assert_allclose(B[i], B_ref, rtol=0, atol=2e-13 / eps, err_msg="B of %s, eps %g" % (name, eps))


# ------------------------------------------------------------------------------------------------ c. / d. no convergence, NaN

def _between_neighbours(x_mid, u_mid):
    """boat_novice: (x, u, Q, R, device batch results, results of every item alone) of [interior, the given item, interior]."""
    eng = _pair("boat_novice")[2]
    xg, ug = D.case_states("boat_novice", 2, seed=3)
    x, u = np.array([xg[0], x_mid, xg[1]]), np.array([ug[0], u_mid, ug[1]])
    Q, R = np.eye(6), 1e-4 * np.eye(3)
    return x, u, Q, R, eng.lqr_dare_batch(x, u, Q, R, eps=EPS), _alone(eng, x, u, Q, R)


def test_exhausted_iteration():
    """boat_novice at rest at the origin with every effort far beyond its clamp: B = 0 exactly, the positions have eigenvalue
    exactly 1 and H doubles for ever.  The restatement gives (tests/test_dare_cpu.py): 64 iterations, K exactly 0, S finite with
    max|S| = 2^64.  The device must stop at max_iter with the same bits, and its neighbours in the batch must not notice."""
    x, u, Q, R, (S, K, A, B, it), alone = _between_neighbours(D.EXHAUSTED_X, D.EXHAUSTED_U)
    assert np.all(B[1] == 0.0)
    assert it[1] == 64
    ref = D.dare_solve(A[1], B[1], Q, R)
    assert ref[2] == 64 and np.all(ref[1] == 0.0) and np.abs(ref[0]).max() == 2.0 ** 64
    _same_bits((S[1], K[1], it[1]), ref, "the exhausted item")
    for i in range(3):
        _same_bits((S[i], K[i], it[i]), alone[i], "item %d of the batch against itself alone" % i)
    assert it[0] < 64 and it[2] < 64


@pytest.mark.parametrize("where", [0, 2, 3])
def test_non_finite_input(where):
    """One item of three has a NaN state component (a position: one row of A, B is NaN; the heading: the position rows; the
    forward speed: nearly everything).  The call returns, the item's outputs and iteration count are the restatement's (whose
    fmax ignores a NaN like the device's), and both neighbours keep their bits."""
    xm, um = D.case_states("boat_novice", 1, seed=4)
    xm[0, where] = np.nan
    x, u, Q, R, (S, K, A, B, it), alone = _between_neighbours(xm[0], um[0])
    assert np.isnan(A[1]).any()
    ref = D.dare_solve(A[1], B[1], Q, R)
    _same_bits((S[1], K[1], it[1]), ref, "the NaN item")
    assert np.isnan(S[1]).any()
    for i in (0, 2):
        _same_bits((S[i], K[i], it[i]), alone[i], "item %d of the batch against itself alone" % i)
        assert np.isfinite(S[i]).all() and np.isfinite(K[i]).all()


# ------------------------------------------------------------------------------------------------ e. / f. the native call

class _Native(object):
    """lqrrt_lqr_dare_batch itself on device tensors: any pointer may be None, the return code comes back unchecked."""

    def __init__(self, eng, Bn, fill=np.nan):
        import torch
        self.eng, self.Bn = eng, Bn
        dev, n, m, k = "cuda:%d" % eng.device, eng.n, eng.m, max(Bn, 1)
        self.S = torch.full((k, n, n), fill, dtype=torch.float64, device=dev)
        self.K = torch.full((k, m, n), fill, dtype=torch.float64, device=dev)
        self.A = torch.full((k, n, n), fill, dtype=torch.float64, device=dev)
        self.B = torch.full((k, n, m), fill, dtype=torch.float64, device=dev)
        self.it = torch.full((k,), -7, dtype=torch.int32, device=dev)

    def call(self, x, u, Q, R, eps, skip=(), null_Q=False):
        import torch
        from lqrrt_amd import _native as nat
        eng = self.eng
        k = max(self.Bn, 1)
        dx = eng._dev(np.resize(x, (k, eng.n)), (k, eng.n))
        du = None if u is None else eng._dev(np.resize(u, (k, eng.m)), (k, eng.m))
        dQ, dR = eng._dev(Q, (eng.n, eng.n)), eng._dev(R, (eng.m, eng.m))

        def p(t, name):
            return None if (t is None or name in skip) else C.c_void_p(t.data_ptr())

        rc = nat.lib().lqrrt_lqr_dare_batch(eng.h, p(dx, "x"), p(du, "u"), self.Bn, None if null_Q else p(dQ, "Q"), p(dR, "R"),
                                            float(eps), p(self.S, "S"), p(self.K, "K"), p(self.A, "A"), p(self.B, "B"),
                                            p(self.it, "it"), eng._stream())
        torch.cuda.synchronize(eng.device)
        return rc

    def host(self):
        return tuple(t.cpu().numpy() for t in (self.S, self.K, self.A, self.B, self.it))


def test_empty_batch_writes_nothing():
    eng = _pair("boat_novice")[2]
    x, u = D.case_states("boat_novice", 1)
    nat = _Native(eng, 0, fill=12345.0)
    assert nat.call(x, u, np.eye(6), np.eye(3), EPS) == 0
    S, K, A, B, it = nat.host()
    assert np.all(S == 12345.0) and np.all(K == 12345.0) and np.all(A == 12345.0) and np.all(B == 12345.0) and np.all(it == -7)


def _mixed(count):
    """boat_novice items of every kind: interior states, wraps and clamps, the exhausted item, a NaN."""
    rs = _pair("boat_novice")[1]
    x, u = D.case_states("boat_novice", count, seed=6)
    x, u = x.copy(), u.copy()
    edges = D.linearisation_edges("boat_novice", rs.u_max)
    for k, (_, xe, ue) in enumerate(edges):
        x[5 + 9 * k], u[5 + 9 * k] = xe, ue
    x[100], u[100] = D.EXHAUSTED_X, D.EXHAUSTED_U
    x[count - 1], u[count - 1] = D.EXHAUSTED_X, D.EXHAUSTED_U           # the last block of the grid
    x[200, 2] = np.nan
    return x, u


def test_batch_of_one_and_of_257():
    """B = 1 works; item i of 257 mixed items (one more than a multiple of every plausible tile) has the bits it has when solved
    alone, in the first call and in its repetition."""
    eng = _pair("boat_novice")[2]
    Q, R = D.dense_spd(6), D.R3_LOW
    x, u = _mixed(257)
    first = eng.lqr_dare_batch(x, u, Q, R, eps=EPS)
    again = eng.lqr_dare_batch(x, u, Q, R, eps=EPS)
    for a, b in zip(first, again):
        np.testing.assert_array_equal(a, b)
    S, K, A, B, it = first
    assert it[100] == 64 and it[256] == 64 and np.isnan(S[200]).any() and np.isfinite(S[[0, 1, 100, 256]]).all()
    alone = _alone(eng, x, u, Q, R)                                      # 257 batches of one
    for i in range(257):
        _same_bits((S[i], K[i], it[i]), alone[i], "item %d of 257 against itself alone" % i)
    _same_bits((S[0], K[0], it[0]), D.dare_solve(A[0], B[0], Q, R), "item 0")
    _same_bits((S[256], K[256], it[256]), D.dare_solve(A[256], B[256], Q, R), "item 256")


def test_optional_arguments():
    """u = NULL is u = zeros; with A, B and the iteration counts NULL, S and K keep their bits and nothing else is written."""
    eng = _pair("car")[2]
    Q, R = D.dense_spd(5), D.R2_MOVE
    x, u = D.case_states("car", 5)
    zeros = eng.lqr_dare_batch(x, np.zeros_like(u), Q, R, eps=EPS)
    null = eng.lqr_dare_batch(x, None, Q, R, eps=EPS)
    for a, b in zip(zeros, null):
        np.testing.assert_array_equal(a, b)
    full = eng.lqr_dare_batch(x, u, Q, R, eps=EPS)
    bare = eng.lqr_dare_batch(x, u, Q, R, eps=EPS, outputs=("S", "K"))
    assert bare[2] is None and bare[3] is None and bare[4] is None
    np.testing.assert_array_equal(bare[0], full[0])
    np.testing.assert_array_equal(bare[1], full[1])
    nat = _Native(eng, 5, fill=12345.0)                                  # the same through the native call, with sentinels behind NULL
    assert nat.call(x, u, Q, R, EPS, skip=("A", "B", "it")) == 0
    S, K, A, B, it = nat.host()
    np.testing.assert_array_equal(S, full[0])
    np.testing.assert_array_equal(K, full[1])
    assert np.all(A == 12345.0) and np.all(B == 12345.0) and np.all(it == -7)
    for one in ("A", "B", "it"):
        nat = _Native(eng, 5, fill=12345.0)
        assert nat.call(x, u, Q, R, EPS, skip=(one,)) == 0
        got = dict(zip(("S", "K", "A", "B", "it"), nat.host()))
        for k, name in enumerate(("S", "K", "A", "B", "it")):
            if name == one:
                assert np.all(got[name] == (-7 if name == "it" else 12345.0))
            else:
                np.testing.assert_array_equal(got[name], full[k])


def test_argument_errors_leave_the_engine_usable():
    from lqrrt_amd import _native as natmod
    from lqrrt_amd.engine import Engine
    s, _, eng = _pair("car")
    Q, R = np.eye(5), np.eye(2)
    x, u = D.case_states("car", 3)
    good = eng.lqr_dare_batch(x, u, Q, R, eps=EPS)

    def still_good(e):
        for a, b in zip(e.lqr_dare_batch(x, u, Q, R, eps=EPS), good):
            np.testing.assert_array_equal(a, b)

    for eps in (0.0, -1e-6, float("nan")):
        nat = _Native(eng, 3, fill=12345.0)
        assert nat.call(x, u, Q, R, eps) == natmod.E_ARG, eps
        assert all(np.all(t == 12345.0) for t in nat.host()[:4])
        with pytest.raises(ValueError):                                  # what the wrapper makes of E_ARG
            eng.lqr_dare_batch(x, u, Q, R, eps=eps)
        still_good(eng)
    nat = _Native(eng, 3, fill=12345.0)
    assert nat.call(x, u, Q, R, EPS, null_Q=True) == natmod.E_ARG
    assert all(np.all(t == 12345.0) for t in nat.host()[:4])
    still_good(eng)
    fresh = Engine(s, capacity=64, max_wave=64)                          # no set_resolution yet: no dt
    try:
        assert _Native(fresh, 3).call(x, u, Q, R, EPS) == natmod.E_STATE
        fresh.set_resolution(s.plan_kwargs["dt"], 0.0, 1, np.zeros(5), None, None)
        still_good(fresh)
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------------ g. three users, one set of bits

@pytest.mark.parametrize("name", ["pendulum_lqr", "boat_novice_lqr"])
def test_rollout_gain_operator_and_solver_give_the_same_bits(name):
    """What dare.hpp documents above dare_lqr: the rollouts (k_steer, 256 threads sharing one solve), lqrrt_gain_batch (64
    threads) and lqrrt_lqr_dare_batch (64 threads) produce the same bits.  Eight rollouts from a tree that is its root alone:
    the gain recorded at the end of each is the solver's K about the last recorded state and effort (the boat's lqr: about the
    state and zero effort).  (The per-sample S table: tests/test_nn_scan_gpu.py; one against four wavefronts:
    tests/test_switches_gpu.py.)"""
    from lqrrt_amd.engine import Engine
    s = _pair(name)[0]
    kw = s.plan_kwargs
    eng = Engine(s, capacity=64, max_wave=64)
    try:
        eng.set_resolution(kw["dt"], kw["FPR"], int(kw["horizon"] / kw["dt"]), np.abs(s.error_tol), None, None)
        eng.tree_reset(s.x0)
        space = np.array(s.sample_space, dtype=np.float64)
        xt = space[:, 0] + (space[:, 1] - space[:, 0]) * np.random.RandomState(12).random_sample((8, s.nstates))
        ln, xseq, useq, xend, Kend = eng.steer_batch(np.zeros(8, dtype=np.int32), xt)
        assert np.all(ln >= 1), ln                                       # every rollout recorded a step: there is an end gain
        ulast = np.array([useq[k, ln[k] - 1] for k in range(8)])
        for k in range(8):
            np.testing.assert_array_equal(xend[k], xseq[k, ln[k] - 1])
        u_lin = np.zeros_like(ulast) if name == "boat_novice_lqr" else ulast
        K = eng.lqr_dare_batch(xend, u_lin, s.Q, s.R, eps=s.eps)[1]
        np.testing.assert_array_equal(Kend, K, err_msg="rollout (256 threads) against lqrrt_lqr_dare_batch")
        np.testing.assert_array_equal(eng.gain_batch(xend, ulast), K, err_msg="lqrrt_gain_batch against lqrrt_lqr_dare_batch")
        assert len(np.unique(K.reshape(8, -1), axis=0)) == 8              # eight different problems
    finally:
        eng.close()
