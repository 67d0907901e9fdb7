"""
CPU: the directed case list of tests/chain_step_cases.py reaches what tests/test_chain_step_gpu.py is there for, as the
reference alone classifies it -- no GPU, no code under test.

  * Every required category of every world holds at least two cases: the arm of the heading torque per step (v_x < 0, signed
    zeros, |v|^2 on vmin^2 and one ulp above, |v_y| / |v_x| on tan(pi/8) and one ulp above, |v_y| > |v_x|, a change of arm
    inside a rollout), each thruster saturating alone at either limit, every sign of every velocity, the car-like rule's three
    arms and its clamp, rollouts ending on step H + 1 for H = 1, 2, 3 (feasible, infeasible under three FPRs, adaptive), and in
    the sweep 0, 1, 2, 3 and six obstacles inside the cull box, a near obstacle that hits nothing, the squared distance of a
    hull point on the threshold and one ulp either side, hulls of 28, 33 and 65 points, tables of 36 and 65 obstacles.
  * The classification's restated sweep agrees with the C oracle's is_feasible on every state it labels (asserted while the
    cases are built), and the reference rollouts equal the C oracle's orc_steer_from bit for bit.
"""
import numpy as np
import pytest

import chain_step_cases as CC
import steer_cases as SC


@pytest.mark.parametrize("kind,V,O", CC.KINDS)
def test_every_required_category_has_two_cases(kind, V, O):
    w = CC.world(kind, V, O)
    missing = {c: w.coverage[c] for c in w.required if w.coverage[c] < 2}
    assert not missing, "%s: categories with fewer than two cases: %r" % (w.name, missing)
    assert len(set(w.required)) == len(w.required) >= 4
    assert max(len(b.parents) for b in w.batches) <= 64 and max(b.H for b in w.batches) <= 3
    assert sum(len(b.parents) for b in w.batches) == len(w.cases) <= 96
    assert w.geo.V == V and w.geo.O == O


@pytest.mark.parametrize("kind,V,O", CC.KINDS)
def test_reference_equals_c_oracle_on_every_case(kind, V, O):
    w = CC.world(kind, V, O)
    for bi, b in enumerate(w.batches):
        o = SC.make_oracle(w.s, len(w.states) + 8, H=b.H, FPR=b.FPR, tol=b.tol, adaptive=b.adaptive)
        o.load_tree(w.states, w.K, w.pID)
        for c in w.batch_cases[bi]:
            if b.adaptive:
                o.set_adaptive(1, b.H, b.H)
            ln, xs, us, Ke = o.steer_from(c.pid, c.target)
            r = c.rollout
            assert ln == len(r.xs)
            np.testing.assert_array_equal(xs, r.xs)
            np.testing.assert_array_equal(us, r.us)
            if ln:
                np.testing.assert_array_equal(Ke, r.K_end)
