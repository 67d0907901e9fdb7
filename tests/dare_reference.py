"""
The device Riccati solver (lqrrt_amd/csrc/dare.hpp dare_lqr, after its linearisation) restated as plain sequential fp64: Python
floats in scalar loops, so that no BLAS reorders a sum.  Every sum, quotient and elimination runs in the order of
oracle/lqrrt_oracle.c dmm / dsolve / dare_solve, which is the order the kernel uses inside one lane; device, C oracle and this file
are built or written without contraction, so the three agree BIT FOR BIT (tests/test_dare_cpu.py: this file against
orc_dare_solve; tests/test_dare_gpu.py: the kernel against this file).

  dare_solve(A, B, Q, R)    -> (S, K, iterations, pivot_log): the doubling iteration, symmetrised S, K = (R + B'SB)^-1 B'SA
  dare_mp(A, B, Q, R)       -> (S, K) of the same iteration in 60-digit arithmetic (mpmath): what the fp64 result is measured against
  linearise_np(dyn, x, u, dt, eps) -> (A, B): central differences of a NumPy dynamics function (oracle/systems_np.py)

The case table cases_for() / case_states() and the coverage conditions check_coverage() are shared by the CPU and the GPU test.
"""
import math

import numpy as np

SITES = ("R", "W", "RBSB")                  # R^-1 B' | (I + G H)^-1 [A_k | G] | (R + B'SB)^-1 B'SA


class PivotLog(list):
    """The row exchanges of one solve, [(site, iteration, p, chosen_row)] (iteration -1 for the two m x m sites), and in `.ties`
    every pivot whose largest magnitude was held by two or more candidate rows: [(site, iteration, p, chosen_row, tied_rows)]."""

    def __init__(self):
        list.__init__(self)
        self.ties = []


def c_fmax(a, b):
    """fmax of C: a NaN operand is ignored (Python's max keeps or drops it depending on the order)."""
    if a != a:
        return b
    if b != b:
        return a
    return a if a > b else b


def _div(a, b):
    """a / b of IEEE-754 (Python raises on a zero divisor)."""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return float("nan")
        return math.copysign(float("inf"), a) * math.copysign(1.0, b)


def _mm(A, B, r, k, c, ta, tb):
    """C[r x c] = A[r x k] B[k x c] on flat row-major lists (ta / tb: the stored operand is the transpose): dmm."""
    C = [0.0] * (r * c)
    for idx in range(r * c):
        i, j = divmod(idx, c)
        acc = 0.0
        for p in range(k):
            acc += (A[p * r + i] if ta else A[i * k + p]) * (B[j * k + p] if tb else B[p * c + j])
        C[idx] = acc
    return C


def _solve(W, RHS, n, q, site, it, log):
    """W X = RHS by Gauss-Jordan with partial pivoting (largest |entry| of the column, lowest row on ties), in place on flat lists:
    dsolve.  (The oracle eliminates [W | A_k] and [W | G] one after the other and the kernel [W | A_k | G] at once: a right-hand
    column never looks at another one, so the bits are the same; here q counts all of them.)"""
    for p in range(n):
        best, brow = -1.0, p
        for r in range(p, n):
            v = abs(W[r * n + p])
            if v > best:
                best, brow = v, r
        tied = [r for r in range(p, n) if abs(W[r * n + p]) == best]
        if len(tied) > 1:
            log.ties.append((site, it, p, brow, tuple(tied)))
        if brow != p:
            log.append((site, it, p, brow))
            for j in range(n):
                W[p * n + j], W[brow * n + j] = W[brow * n + j], W[p * n + j]
            for j in range(q):
                RHS[p * q + j], RHS[brow * q + j] = RHS[brow * q + j], RHS[p * q + j]
        piv = W[p * n + p]
        for j in range(n):
            W[p * n + j] = _div(W[p * n + j], piv)
        for j in range(q):
            RHS[p * q + j] = _div(RHS[p * q + j], piv)
        for r in range(n):
            if r == p:
                continue
            f = W[r * n + p]
            for j in range(n):
                if j != p:
                    W[r * n + j] -= f * W[p * n + j]
            for j in range(q):
                RHS[r * q + j] -= f * RHS[p * q + j]
        for r in range(n):
            if r != p:
                W[r * n + p] = 0.0


def dare_solve(A, B, Q, R, tol=1e-14, max_iter=64):
    """(S, K, iterations, pivot_log) of the structure-preserving doubling iteration on (A, B, Q, R), in the kernel's order."""
    A, B, Q, R = (np.ascontiguousarray(M, dtype=np.float64) for M in (A, B, Q, R))
    n, m = B.shape
    assert A.shape == (n, n) and Q.shape == (n, n) and R.shape == (m, m)
    log = PivotLog()
    Af, Bf, Rm = A.ravel().tolist(), B.ravel().tolist(), R.ravel().tolist()
    Hm, Ak = Q.ravel().tolist(), list(Af)
    X = [Bf[(i % n) * m + (i // n)] for i in range(m * n)]                  # X = B' (m x n)
    _solve(list(Rm), X, m, n, "R", -1, log)                                # X = R^-1 B'
    G = _mm(Bf, X, n, m, n, False, False)
    it = 0
    while it < max_iter:
        W = _mm(G, Hm, n, n, n, False, False)
        for i in range(n):
            W[i * n + i] += 1.0
        AG = [0.0] * (n * 2 * n)                                            # [A_k | G]
        for i in range(n * n):
            r, c = divmod(i, n)
            AG[r * 2 * n + c], AG[r * 2 * n + n + c] = Ak[i], G[i]
        _solve(W, AG, n, 2 * n, "W", it, log)
        T1 = [AG[(i // n) * 2 * n + i % n] for i in range(n * n)]            # (I + G H)^-1 A
        T2 = [AG[(i // n) * 2 * n + n + i % n] for i in range(n * n)]        # (I + G H)^-1 G
        T3 = _mm(Ak, _mm(Hm, T1, n, n, n, False, False), n, n, n, True, False)      # A' H (I + G H)^-1 A
        dmax, hmax = 0.0, 0.0
        for i in range(n * n):
            hn = Hm[i] + T3[i]
            dmax, hmax = c_fmax(dmax, abs(T3[i])), c_fmax(hmax, abs(hn))
            Hm[i] = hn
        T3 = _mm(_mm(Ak, T2, n, n, n, False, False), Ak, n, n, n, False, True)      # A (I + G H)^-1 G A'
        for i in range(n * n):
            G[i] += T3[i]
        Ak = _mm(Ak, T1, n, n, n, False, False)
        it += 1
        if dmax <= tol * c_fmax(1.0, hmax):
            break
    S = [0.5 * (Hm[i] + Hm[(i % n) * n + (i // n)]) for i in range(n * n)]
    X = _mm(Bf, S, m, n, n, True, False)                                    # B' S
    Z = _mm(X, Bf, m, n, m, False, False)
    for i in range(m * m):
        Z[i] += Rm[i]
    Y = _mm(X, Af, m, n, n, False, False)                                   # B' S A
    _solve(Z, Y, m, n, "RBSB", -1, log)
    return np.array(S).reshape(n, n), np.array(Y).reshape(m, n), it, log


def dare_mp(A, B, Q, R, dps=60):
    """(S, K) of the doubling iteration in `dps`-digit arithmetic (mpmath), rounded to fp64 at the end."""
    import mpmath as mp
    with mp.workdps(dps):
        A, B, Q, R = (mp.matrix(np.asarray(M, dtype=np.float64).tolist()) for M in (A, B, Q, R))
        n = A.rows
        G, H, Ak, I = B * mp.inverse(R) * B.T, Q, A, mp.eye(n)
        for _ in range(80):
            W = mp.inverse(I + G * H)
            A1, G1, H1 = Ak * W * Ak, G + Ak * W * G * Ak.T, H + Ak.T * H * W * Ak
            d = max(abs(H1[i, j] - H[i, j]) for i in range(n) for j in range(n))
            Ak, G, H = A1, G1, H1
            if d < mp.mpf(10) ** (-(3 * dps) // 4) * max(abs(H[i, j]) for i in range(n) for j in range(n)):
                break
        K = mp.inverse(R + B.T * H * B) * (B.T * H * A)
        return (np.array(H.tolist(), dtype=np.float64).reshape(n, n),
                np.array(K.tolist(), dtype=np.float64).reshape(B.cols, n))


def linearise_np(dyn, x, u, dt, eps):
    """(A, B) = (df/dx, df/du) about (x, u) by central differences of dyn(x, u, dt) with step eps."""
    x, u = np.asarray(x, dtype=np.float64), np.asarray(u, dtype=np.float64)
    n, m = len(x), len(u)
    A, B = np.zeros((n, n)), np.zeros((n, m))
    for j in range(n):
        d = np.zeros(n); d[j] = eps
        A[:, j] = (dyn(x + d, np.copy(u), dt) - dyn(x - d, np.copy(u), dt)) / (2 * eps)
    for j in range(m):
        d = np.zeros(m); d[j] = eps
        B[:, j] = (dyn(np.copy(x), u + d, dt) - dyn(np.copy(x), u - d, dt)) / (2 * eps)
    return A, B


# ------------------------------------------------------------------------------------------------ the case table
# Weights chosen so that the three eliminations exchange rows and meet exact ties; every claim below is asserted from pivot_log by
# check_coverage (tests/test_dare_cpu.py on NumPy's A, B; tests/test_dare_gpu.py again on the device's own A, B).
#   R2_MOVE   |R[1,0]| = 2 > R[0,0] = 1: the pivot of R^-1 B' moves at p = 0.
#   R2_STAY   |R[1,0]| = R[0,0] = 2: an exact tie, row 0 stays.
#   R3_LOW    |R[1,0]| = |R[2,0]| = 2 > R[0,0] = 1: an exact tie between the two lower rows, row 1 wins; p = 1 then moves too.
#   R3_P1     row 0 stays (4 > 1); the reduced column 1 is (1.75, 2.75): the pivot moves at p = 1 only.
# All four are symmetric positive definite by their leading minors (1, 1 | 2, 6 | 1, 5, 16 | 4, 7, 31).
# (Which of two tied rows wins shows in the bits of the 12-state R_blocks_small runs only: for the boats' B' either choice rounds to
# the same R^-1 B', so there the rule is pinned by the pivot log of this restatement and by its C twin, not by the device's bits.)
R2_MOVE = np.array([[1.0, 2.0], [2.0, 5.0]])
R2_STAY = np.array([[2.0, 2.0], [2.0, 5.0]])
R3_LOW = np.array([[1.0, 2.0, 2.0], [2.0, 9.0, 1.0], [2.0, 1.0, 9.0]])
R3_P1 = np.array([[4.0, 1.0, 1.0], [1.0, 2.0, 3.0], [1.0, 3.0, 9.0]])

SYSTEM_NAMES = ("pendulum", "car", "boat_novice", "boat_advanced", "double_integrator", "pendulum_lqr", "boat_novice_lqr")
DIMS = dict(pendulum=(4, 1), car=(5, 2), boat_novice=(6, 3), boat_advanced=(6, 3), double_integrator=(12, 6), pendulum_lqr=(4, 1),
            boat_novice_lqr=(6, 3))


def _blocks(*Ms):
    k = sum(len(M) for M in Ms)
    out, at = np.zeros((k, k)), 0
    for M in Ms:
        out[at:at + len(M), at:at + len(M)] = M
        at += len(M)
    return out


def dense_spd(n, seed=5):
    """A dense symmetric positive definite n x n matrix with entries of order one (diagonally dominant by construction)."""
    M = np.random.RandomState(seed + n).uniform(-1, 1, (n, n))
    return 0.5 * (M + M.T) + n * np.eye(n)


def _coupled(n, pairs):
    """Identity plus off-diagonal 0.5 at the listed (velocity row, position column) pairs, symmetric: positive definite (every
    row's off-diagonal sum is 0.5 < 1).  W = I + G H then has G[v, v] * 0.5 in column `position` below a diagonal 1."""
    Q = np.eye(n)
    for i, j in pairs:
        Q[i, j] = Q[j, i] = 0.5
    return Q


def cases_for(name):
    """[(label, Q, R)] of a system: the comfortable diagonal case, dense weights whose R moves or ties the m x m pivots, and a
    position-velocity coupled Q over a small R, which makes G H dominate the diagonal of W = I + G H."""
    n, m = DIMS[name]
    out = [("diag", np.eye(n), np.eye(m) * (1e-4 if m > 1 and n < 12 else 1.0))]
    if m == 1:
        out.append(("dense_Q", dense_spd(n), np.array([[0.3]])))
        out.append(("W_moves", _coupled(n, [(2, 0), (3, 1)]), np.array([[1e-9]])))
    elif m == 2:
        out.append(("R_moves_p0", dense_spd(n), R2_MOVE))
        out.append(("R_tie_stays", dense_spd(n), R2_STAY))
        out.append(("W_moves", _coupled(n, [(3, 0), (4, 1)]), np.diag([1e-10, 1e-9])))
    elif m == 3:
        out.append(("R_tie_lower", dense_spd(n), R3_LOW))
        out.append(("R_moves_p1", dense_spd(n), R3_P1))
        out.append(("W_moves", _coupled(n, [(3, 0), (4, 1)]), np.diag([1e-10, 1e-10, 1e-6])))
    else:
        out.append(("R_blocks", dense_spd(n), _blocks(R3_LOW, R3_P1)))
        out.append(("R_blocks_small", np.eye(n), 1e-4 * _blocks(R3_LOW, R3_P1)))
        out.append(("W_moves", _coupled(n, [(6, 0), (8, 1)]), 1e-4 * np.eye(m)))
    return out


TIE_STAYS = ("R_tie_stays",)                     # labels whose R holds an exact tie that keeps row p
TIE_LOWER = ("R_tie_lower", "R_blocks", "R_blocks_small")      # ... an exact tie between two lower rows


def case_states(name, count=4, seed=0):
    """(x [count][n], u [count][m]): interior states (moving forward, efforts inside the actuator limits)."""
    n, m = DIMS[name]
    rng = np.random.RandomState(seed)
    if n == 4:
        return rng.uniform(-1, 1, (count, n)), rng.uniform(-5, 5, (count, m))
    if n == 12:
        return rng.uniform(0, 50, (count, n)), rng.uniform(-1, 1, (count, m))
    x = np.zeros((count, n))
    x[:, :2] = rng.uniform(0, 40, (count, 2))
    x[:, 2] = rng.uniform(-3, 3, count)
    x[:, 3] = rng.uniform(0.3, 1.0, count)
    x[:, 4:] = rng.uniform(-0.1, 0.1, (count, n - 4))
    return x, rng.uniform(-50, 50, (count, m))


# boat_novice at rest at the origin with every effort far beyond its clamp: B = 0 exactly and the position quotients are exactly 1,
# so the doubling never converges (tests/test_dare_cpu.py test_exhausted_iteration)
EXHAUSTED_X = np.zeros(6)
EXHAUSTED_U = np.full(3, 1e6)


def check_coverage(runs):
    """runs: [(n, label, R, pivot_log)].  Asserts that the runs exchange rows at p = 0 and at some p >= 1 at each of the three
    elimination sites, on the register path (n <= 6) and on the fallback (n = 12), that an exact tie keeps row p, that an exact tie
    between two lower rows goes to the lower one, and that the ties of the labelled cases are those of R's own entries."""
    for path, on_path in (("register", lambda n: n <= 6), ("fallback", lambda n: n == 12)):
        for site in SITES:
            ps = set(p for n, _, _, log in runs if on_path(n) for s, _, p, _ in log if s == site)
            assert 0 in ps, "%s path: no run exchanges rows at p = 0 of site %s" % (path, site)
            assert any(p >= 1 for p in ps), "%s path: no run exchanges rows at a p >= 1 of site %s" % (path, site)
    stays = [t for _, _, _, log in runs for t in log.ties if t[3] == t[2]]
    lower = [t for _, _, _, log in runs for t in log.ties if min(t[4]) > t[2] and t[3] == min(t[4])]
    assert stays, "no exact tie that keeps row p"
    assert lower, "no exact tie between two lower rows"
    for n, label, R, log in runs:
        if label in TIE_STAYS + TIE_LOWER:
            ties = [t for t in log.ties if t[0] == "R" and t[2] == 0]
            assert len(ties) == 1, (label, log.ties)
            _, _, _, chosen, tied = ties[0]
            col = np.abs(np.asarray(R)[:, 0])
            assert tuple(np.flatnonzero(col == col.max())) == tied and len(tied) >= 2, (label, "the tie is not R's own", tied)
            assert chosen == min(tied) and (chosen == 0) == (label in TIE_STAYS), (label, chosen, tied)


def linearisation_edges(name, u_max=None):
    """[(label, x, u)]: where the central differences of a system's dynamics meet a wrap, a branch or a clamp.  u_max: the
    system's symmetric effort limits where it has them (boat_novice: per axis; car: forward and steering)."""
    n, m = DIMS[name]
    pi, near = np.pi, 3e-7                                   # within eps = 1e-6 of the wrap
    out = []
    if n == 4:
        base, u = np.array([0.3, -0.4, 0.5, 0.2]), np.array([1.5])
        for d in (0, 1):
            for tag, a in (("near +pi", pi - near), ("near -pi", -pi + near), ("beyond pi", 4.0)):
                x = base.copy()
                x[d] = a
                out.append(("angle %d %s" % (d, tag), x, u))
        return out
    if n == 12:
        rng = np.random.RandomState(8)
        return [("interior", rng.uniform(0, 50, n), rng.uniform(-1, 1, m))]
    base = np.array([10.0, 20.0, 1.0, 0.7, 0.05, -0.05])[:n]
    u = np.array([10.0, -20.0, 30.0])[:m]
    for tag, a in (("near +pi", pi - near), ("near -pi", -pi + near), ("beyond pi", 4.0)):
        x = base.copy()
        x[2] = a
        out.append(("heading %s" % tag, x, u))
    x = base.copy()
    x[3] = 0.0
    out.append(("forward speed 0", x, u))
    if u_max is not None:
        lim = np.asarray(u_max, dtype=np.float64)
        out.append(("efforts at the limit", base, lim.copy()))
        out.append(("efforts at minus the limit", base, -lim))
    out.append(("efforts beyond the limit", base, np.array([1e4, -1e4, 1e4])[:m]))
    return out
