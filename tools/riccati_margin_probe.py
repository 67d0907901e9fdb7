#!/usr/bin/env python
"""Whose error is the "solver disagreement" of the Riccati pendulum?  (container, CPU; profiles/r05_riccati_margin.txt)

For samples of the reference's 600-node run (tests/golden/traj_pendulum_lqr_600.npz): S about the sample from
  * SciPy's solve_discrete_are on NumPy's central differences (the fixture's S_samples: what the reference compared),
  * the doubling solver of the sequential C oracle (= the device's, bit for bit) on ITS central differences,
  * an fp64 doubling written in NumPy on NumPy's (A, B)                          -> the solver's own error,
each against a 60-digit mpmath doubling solution of NumPy's (A, B), plus the sensitivity of the true solution to a 1e-16
relative perturbation of A.  Then the decision margin (tests/test_pendulum_lqr.py test_riccati_decision_margin) of the run
with eps = 1e-6 and of its twin with eps = 1e-4."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("oracle", "tests", ""):
    sys.path.insert(0, os.path.join(ROOT, p))
import coracle  # noqa: E402
from dare_reference import dare_mp  # noqa: E402
import lqrrt_amd  # noqa: E402
import teacher  # noqa: E402
from systems_np import SYSTEMS  # noqa: E402


def mp_dare(A, B, Q, R):
    return dare_mp(A, B, Q, R, dps=60)[0]


def np_dare(A, B, Q, R, tol=1e-14):
    n = A.shape[0]
    G, H, Ak, I = B @ np.linalg.inv(R) @ B.T, Q.copy(), A.copy(), np.eye(n)
    for _ in range(64):
        W = np.linalg.solve(I + G @ H, np.hstack([Ak, G]))
        A1, G1, H1 = Ak @ W[:, :n], G + Ak @ W[:, n:] @ Ak.T, H + Ak.T @ (H @ W[:, :n])
        d = np.abs(H1 - H).max()
        Ak, G, H = A1, G1, H1
        if d <= tol * np.abs(H).max():
            break
    return H


def main():
    g = np.load(os.path.join(ROOT, "tests", "golden", "traj_pendulum_lqr_600.npz"))
    s, rs = lqrrt_amd.systems.SYSTEMS["pendulum_lqr"](0), SYSTEMS["pendulum_lqr"](0)
    o = coracle.make(s, 16, seed=1)
    idx = sorted(set(np.random.RandomState(0).choice(len(g["S_samples"]), 12, replace=False).tolist()))
    print("relative to max|S_true|; columns: SciPy - true | C doubling (own A, B) - true | NumPy doubling (NumPy's A, B) - true | "
          "true(A (1 + 1e-16)) - true(A)")
    for t in idx:
        x = g["xrand_all"][t]
        A, B = rs.linearize(x, np.zeros(1))
        St = mp_dare(A, B, rs.Q, rs.R)
        sc = np.abs(St).max()
        S_c = o.lqr(x, np.zeros(1))[0]
        S_n = np_dare(A, B, rs.Q, rs.R)
        A2 = A * (1 + 1e-16 * np.sign(np.random.RandomState(1).randn(*A.shape)))
        print("  sample %3d  max|S| %.1e   %.1e | %.1e | %.1e | %.1e" % (
            t, sc, np.abs(g["S_samples"][t] - St).max() / sc, np.abs(S_c - St).max() / sc, np.abs(S_n - St).max() / sc,
            np.abs(mp_dare(A2, B, rs.Q, rs.R) - St).max() / sc))
    print()
    for tag, eps in (("600", 1e-6), ("600_eps1e-4", 1e-4)):
        g = np.load(os.path.join(ROOT, "tests", "golden", "traj_pendulum_lqr_%s.npz" % tag))
        s, rs = lqrrt_amd.systems.SYSTEMS["pendulum_lqr"](0, eps=eps), SYSTEMS["pendulum_lqr"](0, eps=eps)
        sch = teacher.Schedule(g, s.goal, s.goal_buffer)
        o = coracle.make(s, 16, seed=1)
        safety, flips, sdis = np.inf, 0, 0.0
        for t in range(sch.iters):
            size = int(sch.size_before[t])
            ign = sch.ignored_at(size)[:size].astype(bool)
            x = sch.xrand[t]
            d = np.array([rs.erf(x, xi) for xi in sch.state[:size]])
            S_dbl = o.lqr(x, np.zeros(o.m))[0]
            sdis = max(sdis, np.abs(S_dbl - g["S_samples"][t]).max() / np.abs(g["S_samples"][t]).max())
            c_ref = np.einsum("ij,jk,ik->i", d, g["S_samples"][t], d)
            c_dbl = np.einsum("ij,jk,ik->i", d, S_dbl, d)
            cand = np.flatnonzero(~ign) if (~ign).any() else np.arange(size)
            w = int(cand[np.argmin(c_ref[cand])])
            flips += int(not (w == int(sch.nearest[t]) == int(cand[np.argmin(c_dbl[cand])])))
            others = np.array([j for j in cand if j != w and not np.array_equal(d[j], d[w])], dtype=np.int64)
            if len(others):
                gap = c_ref[others] - c_ref[w]
                dis = np.abs(c_dbl[others] - c_ref[others]) + abs(c_dbl[w] - c_ref[w])
                safety = min(safety, float(np.min(gap / np.maximum(dis, 1e-300))))
        print("run %-12s (eps = %g): %d decisions, %d flipped, smallest gap / disagreement %.2f, max |S_doubling - S_scipy| / max|S| %.1e" % (
            tag, eps, sch.iters, flips, safety, sdis))


if __name__ == "__main__":
    main()
