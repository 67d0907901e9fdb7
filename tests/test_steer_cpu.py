"""
CPU: anchors tests/steer_reference.py -- the plain restatement of Planner._steer that tests/test_steer_gpu.py holds the rollout
kernels to -- and proves that the directed case list (tests/steer_cases.py) reaches every stop, cut and goal-flag edge.

  * The reference equals the sequential C oracle's orc_steer_from BIT FOR BIT (length, states, efforts, end gain) for every
    compiled-in system: on a seeded pool of 600 moving parents steered toward 600 targets at H = 6, fixed and adaptive, and on
    every pair of every batch of the case list under that batch's own resolution.  Same portable libm, same order: no tolerance.
  * The forced mode, which the C oracle does not have, against the NumPy oracle's _steer(force_arrive=True) under a clock that
    never times out, within the project's 1e-9 (states) / 1e-6 (efforts) bars.
  * Coverage is a condition: every category of steer_cases.required() holds at least two cases, as the reference alone
    classifies them.  An empty category fails; nothing here skips.
"""
import numpy as np
import pytest

import steer_cases as SC
import steer_reference as R


def _same(o, ID, xt, r):
    ln, xs, us, Ke = o.steer_from(ID, xt)
    assert ln == len(r.xs)
    np.testing.assert_array_equal(xs, r.xs)
    np.testing.assert_array_equal(us, r.us)
    if ln:
        np.testing.assert_array_equal(Ke, r.K_end)


@pytest.mark.parametrize("name", SC.NAMES)
def test_reference_equals_c_oracle_on_the_seed_pool(name):
    c = SC.cases(name)
    H, tol = 6, np.zeros(c.n)
    assert len(c.spar) == 600
    pid = np.arange(len(c.spar), dtype=np.int32) - 1
    for adaptive in (False, True):
        o = SC.make_oracle(c.s, len(c.spar) + 8, H=H, FPR=0.5, tol=tol, adaptive=adaptive)
        o.load_tree(c.spar, c.sK, pid)
        reasons = set()
        for i in range(len(c.spar)):
            if adaptive:
                o.set_adaptive(1, H, H)                 # (a growth event halves the oracle's horizon state: the device compares with H)
            r = c.ref(c.spar[i], c.sK[i], c.star[i], H, 0.5, tol, adaptive)
            _same(o, i, c.star[i], r)
            reasons.add(r.reason[0])
        assert "horizon" in reasons and (not adaptive or "grew" in reasons)
        assert name in SC.NO_OBSTACLES or "infeasible" in reasons


@pytest.mark.parametrize("name", SC.NAMES)
def test_reference_equals_c_oracle_on_every_case(name):
    c = SC.cases(name)
    oracles = {}
    pairs = 0
    for bi, b in enumerate(c.batches):
        if b.adaptive not in oracles:
            oracles[b.adaptive] = SC.make_oracle(c.s, len(c.states) + 8, adaptive=b.adaptive)
            oracles[b.adaptive].load_tree(c.states, c.K, c.pID)
        o = oracles[b.adaptive]
        assert np.all(b.tol >= 0)                       # (COracle.configure takes |tol|)
        o.configure(c.dt, b.FPR, b.H, b.tol, c.s.goal, np.abs(c.s.goal_buffer), c.s.sample_space, c.s.goal_bias)
        for p, xt, r in zip(b.parents, b.targets, c.expected(bi)):
            if b.adaptive:
                o.set_adaptive(1, b.H, b.H)
            _same(o, int(p), xt, r)
            assert len(r.xs) <= b.H and r.steps <= b.H + 1
            pairs += 1
    assert pairs > 300


@pytest.mark.parametrize("name", SC.NAMES)
def test_every_required_category_has_two_cases(name):
    c = SC.cases(name)
    missing = {cat: c.coverage[cat] for cat in SC.required(name) if c.coverage[cat] < 2}
    assert not missing, "categories with fewer than two cases: %r" % missing
    assert max(len(b.parents) for b in c.batches) <= 64 and max(b.H for b in c.batches) <= 6
    # placement: the mixed batches hold one case in the first, a middle and the last slot
    for b in c.batches:
        if b.tag == "mixed":
            W = len(b.parents)
            same = [t for t in range(W) if b.parents[t] == b.parents[0] and np.array_equal(b.targets[t], b.targets[0])]
            assert same[0] == 0 and same[-1] == W - 1 and any(0 < t < W - 1 for t in same)
    # a batch without a single node, and launches of one
    assert any(all(len(r.xs) == 0 for r in c.expected(bi)) and len(b.parents) > 1 for bi, b in enumerate(c.batches))
    assert any(len(b.parents) == 1 for b in c.batches)
    a, b5 = (c.batches[i] for i in c.four)
    assert len(a.parents) == 4 and len(b5.parents) == 5 and np.array_equal(a.parents, b5.parents[:4])
    # ... a horizon, a growth, a cut that leaves a node behind (a second horizon where nothing is infeasible) and a convergence
    got = [(r.reason[0], len(r.xs)) for r in c.expected(c.four[0])]
    cut = ("horizon", 6) if name in SC.NO_OBSTACLES else ("infeasible", 4)
    assert got == [("horizon", 6), ("grew", 0), cut, ("conv", 2)]
    # the goal box is probed on the first and the last state component, and on others
    assert {0, c.n - 1} <= c.goal_dims and len(c.goal_dims) >= 3


def test_case_list_is_deterministic():
    a, b = SC.SystemCases("boat_novice"), SC.cases("boat_novice")
    assert len(a.batches) == len(b.batches)
    np.testing.assert_array_equal(a.states, b.states)
    for x, y in zip(a.batches, b.batches):
        np.testing.assert_array_equal(x.parents, y.parents)
        np.testing.assert_array_equal(x.targets, y.targets)
        np.testing.assert_array_equal(x.tol, y.tol)


# ---- forced mode against the NumPy oracle ----------------------------------------------------------------------------------

def _numpy_forced(name, x0, K0, xt, **overrides):
    from lqrrt_oracle import RefTree
    from systems_np import SYSTEMS, make_oracle_planner
    s = SYSTEMS[name](0) if name != "double_integrator" else SYSTEMS[name]()
    p = make_oracle_planner(s, 16, **overrides)          # (its clock stands still: force_arrive never times out)
    p.tree = RefTree(np.array(x0), (None, np.array(K0)))
    return p._steer(0, np.copy(xt), force_arrive=True)


@pytest.mark.parametrize("name", ["boat_advanced", "boat_intermediate", "boat_novice"])
def test_forced_reference_vs_numpy_oracle_infeasible(name):
    """Unchanged demo worlds (the NumPy systems build their own obstacle field): rollouts whose sixth step is infeasible, five
    recorded steps cut by FPR = 0.5, 0.9 and 1.0 to 2, 4 and 5 rows -- a cut that ends inside the edge, one that drops the last
    row only, and none.  Every kept row is compared, so the comparison cannot be empty."""
    c = SC.cases(name)
    k = 6
    assert k in SC.FORCED_INFEASIBLE
    picked = [f for f in c.forced if f.cat == "forced:infeasible@%d/FPR0.5" % k]
    assert len(picked) >= 2
    for f in picked:
        for FPR, rows in ((0.5, 2), (0.9, 4), (1.0, 5)):
            r = R.steer_force(c.ops, c.states[f.parent], c.K[f.parent], f.target, c.dt, FPR, 1e-4, 1e-4, 64)
            assert r.reason == ("infeasible", k) and len(r.xs) == rows == int(FPR * (k - 1))
            xs, us = _numpy_forced(name, c.states[f.parent], c.K[f.parent], f.target, FPR=FPR)
            assert len(xs) == len(us) == rows > 0
            assert np.abs(np.array(xs) - r.xs).max() < 1e-9 and np.abs(np.array(us) - r.us).max() < 1e-6


def test_forced_reference_vs_numpy_oracle_arrival():
    """The double integrator arrives: np.allclose(x, xtar, 1e-4, 1e-4) ends the rollout, the arriving step is not recorded."""
    import lqrrt_amd
    s = lqrrt_amd.systems.SYSTEMS["double_integrator"]()
    o = SC.make_oracle(s, 16)
    ops = R.coracle_ops(o, s.plan_kwargs["dt"])
    x0 = np.concatenate((np.full(6, 50.0), [0.3, -0.2, 0.1, 0.0, 0.25, -0.1]))
    K0 = o.gain(x0, np.zeros(6))
    xt = np.concatenate((np.full(6, 50.0) + [0.4, -0.3, 0.2, 0.1, -0.2, 0.3], np.zeros(6)))
    r = R.steer_force(ops, x0, K0, xt, s.plan_kwargs["dt"], 0.5, 1e-4, 1e-4, 2000)
    assert r.reason[0] == "close" and 20 < len(r.xs) == r.reason[1] - 1
    xs, us = _numpy_forced("double_integrator", x0, K0, xt)
    assert len(xs) == len(r.xs)
    assert np.abs(np.array(xs) - r.xs).max() < 1e-9 and np.abs(np.array(us) - r.us).max() < 1e-6
    assert not np.allclose(xs[-1], xt, rtol=1e-4, atol=1e-4) and np.allclose(r.xall[-1], xt, rtol=1e-4, atol=1e-4)
