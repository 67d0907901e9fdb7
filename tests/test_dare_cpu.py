"""
CPU: the sequential restatement of the device Riccati solver (tests/dare_reference.py dare_solve) against its compiled twin
(oracle/lqrrt_oracle.c orc_dare_solve) BIT FOR BIT, the pivot coverage the case table claims, and the accuracy of the algorithm
itself against 60-digit arithmetic.  A, B here are NumPy central differences of the oracle/systems_np.py dynamics; the GPU test
(tests/test_dare_gpu.py) repeats the bitwise comparison and the coverage conditions on the device's own A, B.
"""
import numpy as np
import pytest

import coracle
import dare_reference as D
from systems_np import SYSTEMS

EPS = 1e-6
_cache = {}


def _twin(name):
    return SYSTEMS[name]() if name == "double_integrator" else SYSTEMS[name](0)


def _runs(name):
    """[(label, state index, A, B, Q, R, (S, K, it, log))] of a system's case table, solved once per session."""
    if name not in _cache:
        rs = _twin(name)
        xs, us = D.case_states(name)
        out = []
        for label, Q, R in D.cases_for(name):
            for i in range(len(xs)):
                A, B = D.linearise_np(rs.dynamics, xs[i], us[i], rs.plan_kwargs["dt"], EPS)
                out.append((label, i, A, B, Q, R, D.dare_solve(A, B, Q, R)))
        _cache[name] = out
    return _cache[name]


def _assert_twins(A, B, Q, R, got=None):
    S, K, it, log = D.dare_solve(A, B, Q, R) if got is None else got
    S_c, K_c, it_c = coracle.dare_solve(A, B, Q, R)
    assert it == it_c
    np.testing.assert_array_equal(S, S_c)
    np.testing.assert_array_equal(K, K_c)
    return S, K, it, log


def test_weights_are_symmetric_positive_definite():
    for name in D.SYSTEM_NAMES:
        for label, Q, R in D.cases_for(name):
            for M in (Q, R):
                assert np.array_equal(M, M.T) and np.linalg.eigvalsh(M).min() > 0, (name, label)


@pytest.mark.parametrize("n,m", [(4, 1), (5, 2), (6, 3), (12, 6)])
def test_restatement_equals_oracle_on_random_systems(n, m):
    """Random dense (A, B) (controllable with probability one; spectral radius 1.1: unstable, so that the gain matters), dense
    symmetric positive definite Q and R."""
    rng = np.random.RandomState(100 * n + m)
    for _ in range(3):
        A = rng.uniform(-1, 1, (n, n))
        A *= 1.1 / np.abs(np.linalg.eigvals(A)).max()
        B = rng.uniform(-1, 1, (n, m))
        M = rng.uniform(-1, 1, (m, m))
        _, _, it, _ = _assert_twins(A, B, D.dense_spd(n, seed=int(rng.randint(1000))), M.dot(M.T) + 0.1 * np.eye(m))
        assert it < 64


@pytest.mark.parametrize("name", D.SYSTEM_NAMES)
def test_restatement_equals_oracle_on_case_table(name):
    for label, i, A, B, Q, R, got in _runs(name):
        _assert_twins(A, B, Q, R, got)
        assert got[2] < 64, (name, label, i)
        np.testing.assert_array_equal(got[0], got[0].T)


def test_case_table_reaches_the_pivots_it_claims():
    D.check_coverage([(D.DIMS[name][0], label, R, got[3]) for name in D.SYSTEM_NAMES for label, _, _, _, _, R, got in _runs(name)])


def test_fmax_ignores_nan_like_c():
    nan = float("nan")
    assert D.c_fmax(nan, 2.0) == 2.0 and D.c_fmax(2.0, nan) == 2.0 and D.c_fmax(1.0, 2.0) == 2.0 and D.c_fmax(2.0, 1.0) == 2.0
    assert D.c_fmax(nan, nan) != D.c_fmax(nan, nan)


def exhausted_case():
    """(A, B, Q, R) of boat_novice at rest at the origin about efforts far beyond the thruster clamp: both sides of every effort
    quotient are clamped to the same value, and the quotients of the positions are (eps - -eps) / (2 eps) = 1 exactly.  (Anywhere
    else their rounding leaves 1 - 1e-10 or so, and the iteration converges after ~40 steps.)"""
    rs = _twin("boat_novice")
    A, B = D.linearise_np(rs.dynamics, D.EXHAUSTED_X, D.EXHAUSTED_U, rs.plan_kwargs["dt"], EPS)
    return A, B, np.eye(6), 1e-4 * np.eye(3)


def test_exhausted_iteration():
    """B = 0 exactly and the position integrators have eigenvalue 1: H doubles in the position block for ever, the test
    dmax <= tol max(1, hmax) never holds, the loop ends at max_iter = 64.  Measured here: iterations 64, K exactly 0,
    S finite with max|S| = 2^64 exactly (the positions' Q[i, i] = 1 doubled 64 times)."""
    A, B, Q, R = exhausted_case()
    assert np.all(B == 0.0)
    S, K, it, log = _assert_twins(A, B, Q, R)
    assert it == 64
    assert np.all(K == 0.0)
    assert np.all(np.isfinite(S)) and np.abs(S).max() == 2.0 ** 64
    assert np.all(np.diag(A)[:3] == 1.0)
    assert len(log) == 0                                     # W = I: nothing moves
    assert _assert_twins(A, B, Q, R)[2] == 64 and coracle.dare_solve(A, B, Q, R, max_iter=7)[2] == 7
    assert D.dare_solve(A, B, Q, R, max_iter=7)[2] == 7


@pytest.mark.parametrize("where", [0, 2, 3])
def test_non_finite_input(where):
    """A NaN state component: the twins agree on every output (NaN positions equal) and on the iteration count, which depends on
    fmax ignoring a NaN."""
    rs = _twin("boat_novice")
    x, u = D.case_states("boat_novice", 1, seed=4)
    x[0, where] = np.nan
    A, B = D.linearise_np(rs.dynamics, x[0], u[0], rs.plan_kwargs["dt"], EPS)
    assert np.isnan(A).any()
    S, K, it, _ = _assert_twins(A, B, np.eye(6), 1e-4 * np.eye(3))
    assert np.isnan(S).any()


# Measured worst max|X_fp64 - X_mp| / max|X_mp| over the case table (first two states of every case):
#                        S          K
MEASURED = {
    "pendulum":          (4.88e-08, 4.81e-08),
    "car":               (8.77e-14, 9.10e-14),
    "boat_novice":       (1.30e-13, 4.13e-14),
    "boat_advanced":     (6.99e-14, 8.44e-14),
    "double_integrator": (4.75e-15, 3.60e-15),
    "pendulum_lqr":      (4.88e-08, 4.81e-08),
    "boat_novice_lqr":   (1.30e-13, 4.13e-14),
}


@pytest.mark.parametrize("name", D.SYSTEM_NAMES)
def test_algorithm_against_mpmath(name):
    """The fp64 doubling iteration against the same iteration in 60-digit arithmetic on the same (A, B, Q, R), relative to the
    largest entry: the rounding error of the ALGORITHM at these weights (the device adds nothing: it has the same bits).  The
    bounds are 10 x the worst value measured per system (MEASURED above; deterministic fp64, the margin only absorbs edits to the
    case table).  Measured: car 8.8e-14 / 9.1e-14 (S / K), boat_novice and boat_novice_lqr 1.3e-13 / 4.1e-14, boat_advanced
    7.0e-14 / 8.4e-14, double_integrator 4.8e-15 / 3.6e-15.  The pendulums stand apart, 4.9e-8 / 4.8e-8: dt = 1 ms makes
    |S| ~ 1e9 and the equation ill-conditioned.  The exhausted and the non-finite case have no solution to compare with and are
    left out here (and nowhere else)."""
    worst_S = worst_K = 0.0
    for label, i, A, B, Q, R, (S, K, it, _) in _runs(name):
        if i >= 2:
            continue
        S_mp, K_mp = D.dare_mp(A, B, Q, R)
        worst_S = max(worst_S, np.abs(S - S_mp).max() / np.abs(S_mp).max())
        worst_K = max(worst_K, np.abs(K - K_mp).max() / np.abs(K_mp).max())
    print("%s: worst S %.2e, worst K %.2e" % (name, worst_S, worst_K))
    assert worst_S <= 10 * MEASURED[name][0] and worst_K <= 10 * MEASURED[name][1]
