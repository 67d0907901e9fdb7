"""
The rollout rule, restated plainly (test infrastructure): Planner._steer of the reference (planner.py:354-447) for both
force_arrive modes, written over four primitive callables

    erf(xt, x) -> e[n]      dynamics(x, u, dt) -> x'[n]      feasible(x, u) -> bool      gain(x, u) -> K[m][n]

so that the only thing restated here is the ORDER of the rules inside a step:

    error -> effort -> dynamics -> feasibility (cut to int(FPR * len), stop) -> count the step -> error growth (adaptive:
    discard the edge, stop) -> horizon / convergence (stop, step not recorded) -> record -> next gain.

Instantiated with coracle.COracle's single-call operators (Ops), which evaluate the same portable libm in the same order as
the device, every value is the device's bit for bit; u = K e is a left-to-right sum per row (np.dot's pairwise / BLAS order is
not the loop's).  The adaptive mode is the device's: the horizon compared against is the fixed H (horizon_iters), i.e. the
oracle with hspan = (1, H) and horizon_iters = H, where doubling is clipped back to H and halving only matters to the next call.
"""
import collections

import numpy as np

Ops = collections.namedtuple("Ops", "erf dynamics feasible gain")

# xs [len][n], us [len][m]: the recorded steps.  K_end = gain(xs[-1], us[-1]) (None without a node).  steps: completed (feasible,
# counted) steps.  reason = (category, step): the step, counted from 1, on which the rule fired; categories: infeasible, grew,
# horizon, conv (normal), infeasible, close, max_steps (forced).  in_goal: strict lo < xs[-1] < hi.  emag [evaluated steps][n] =
# |e| of every evaluated step and xall [evaluated steps][n] = the state it produced, the last (unrecorded) one included: what
# the case builder derives boundary tolerances from.
Rollout = collections.namedtuple("Rollout", "xs us K_end steps reason in_goal emag xall")


def coracle_ops(o, dt):
    """The primitives of a configured coracle.COracle (its dynamics carries the dt it was configured with)."""
    def dynamics(x, u, dt_):
        assert dt_ == dt
        return o.dynamics(x, u)
    return Ops(o.erf, dynamics, o.feasible, o.gain)


def effort(K, e):
    """u = K e, every row summed left to right (the loop of the kernels and of oracle/lqrrt_oracle.c)."""
    K = np.asarray(K, dtype=np.float64)
    u = np.empty(K.shape[0])
    for i in range(K.shape[0]):
        a = K[i, 0] * e[0]
        for j in range(1, K.shape[1]):
            a += K[i, j] * e[j]
        u[i] = a
    return u


def in_goal(x, lo, hi):
    """planner.py:442-447: strict on both sides."""
    return bool(all(l < v < h for l, v, h in zip(lo, x, hi)))


def _finish(ops, n, m, xs, us, steps, reason, lo, hi, emag, xall):
    K_end = ops.gain(xs[-1], us[-1]) if xs else None
    flag = bool(xs) and lo is not None and in_goal(xs[-1], lo, hi)
    return Rollout(np.array(xs, dtype=np.float64).reshape(len(xs), n), np.array(us, dtype=np.float64).reshape(len(us), m),
                   K_end, steps, reason, flag, np.array(emag).reshape(len(emag), n), np.array(xall).reshape(len(xall), n))


def steer(ops, x0, K0, xt, dt, FPR, H, tol, adaptive=False, lo=None, hi=None):
    """Planner._steer(ID, xtar, force_arrive=False) from state x0 with gain K0 toward xt."""
    x = np.array(x0, dtype=np.float64)
    K = np.array(K0, dtype=np.float64)
    xt = np.array(xt, dtype=np.float64)
    tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), x.shape)
    xs, us, emag, xall = [], [], [], []
    last = np.full(x.shape, np.inf)
    steps = 0
    while True:
        e = ops.erf(xt, x)
        u = effort(K, e)
        x = ops.dynamics(x, u, dt)
        mag = np.abs(e)
        emag.append(mag)
        xall.append(x)
        if not ops.feasible(x, u):                               # planner.py:393-396
            keep = int(FPR * len(xs))
            xs, us = xs[:keep], us[:keep]
            reason = ("infeasible", steps + 1)
            break
        steps += 1                                               # planner.py:414
        if adaptive:                                             # planner.py:418-425
            if np.all(mag >= last):
                xs, us = [], []
                reason = ("grew", steps)
                break
            last = mag
        if steps > H:                                            # planner.py:428
            reason = ("horizon", steps)
            break
        if np.all(mag <= tol):
            reason = ("conv", steps)
            break
        xs.append(x)                                             # planner.py:432-436
        us.append(u)
        K = ops.gain(x, u)
    return _finish(ops, len(xt), K.shape[0], xs, us, steps, reason, lo, hi, emag, xall)


def steer_force(ops, x0, K0, xt, dt, FPR, rtol, atol, max_steps):
    """Planner._steer(ID, xtar, force_arrive=True) with the wall-clock timeout (planner.py:402-406) replaced by a cap of
    max_steps RECORDED steps: np.allclose(x, xtar, rtol, atol) ends the rollout and that step is not recorded."""
    x = np.array(x0, dtype=np.float64)
    K = np.array(K0, dtype=np.float64)
    xt = np.array(xt, dtype=np.float64)
    xs, us, emag, xall = [], [], [], []
    steps = 0
    reason = ("max_steps", max_steps)
    while len(xs) < max_steps:
        e = ops.erf(xt, x)
        u = effort(K, e)
        x = ops.dynamics(x, u, dt)
        emag.append(np.abs(e))
        xall.append(x)
        if not ops.feasible(x, u):
            keep = int(FPR * len(xs))
            xs, us = xs[:keep], us[:keep]
            reason = ("infeasible", steps + 1)
            break
        steps += 1
        if np.all(np.abs(x - xt) <= atol + rtol * np.abs(xt)):    # np.allclose, planner.py:409
            reason = ("close", steps)
            break
        xs.append(x)
        us.append(u)
        K = ops.gain(x, u)
    return _finish(ops, len(xt), K.shape[0], xs, us, steps, reason, None, None, emag, xall)
