"""
CPU: the directed case list of tests/packed_step_cases.py reaches what tests/test_packed_step_gpu.py is there for, as the
reference alone classifies it -- no GPU, no code under test.

  * Every required category of every world holds at least two cases, none of them a kept-regardless one: RosBoat's three heading
    modes (a yaw effort K e used, or recorded and replaced; the focus ahead, abeam, dead astern either side of the +-pi cut, on
    the boat with every pair of signed zeros, 1e6 m away; every arm of the velocity torque), its even down-scaling (no ratio
    below 1, a thrust on its limit, one ulp above, one thruster alone, all four, a tie, the 1e-6 floor, zero thrust, the floor
    alone switching the remap on), its per-thruster clip, its no-reverse rule (from a forward boat, from one that backs up, from
    +0 and -0, idle, and a negative surge kept where the rule is off); BoatIntermediate's torque arms, |u| on u_max and one ulp
    beyond per axis and sign, its car-like rule; every velocity sign; rollouts ending on step H + 1 for H = 1, 2, 3 (feasible,
    adaptive, infeasible under FPR 0, 0.5, 0.9, 1); an empty obstacle table.
  * The reference rollouts equal the C oracle's orc_steer_from bit for bit.
  * The C oracle's step means what the reference's behaviours mean: on every labelled step its `dynamics` agrees with the NumPy
    port of the reference (oracle/systems_np.py) to the project's 1e-9.
"""
import collections

import numpy as np
import pytest

import chain_step_cases as CC
import packed_step_cases as PC
import steer_cases as SC


@pytest.mark.parametrize("key", PC.KEYS)
def test_every_required_category_has_two_cases(key):
    w = PC.world(key)
    missing = {c: w.coverage[c] for c in w.required if w.coverage[c] < 2}
    assert not missing, "%s: categories with fewer than two cases: %r" % (w.name, missing)
    assert len(set(w.required)) == len(w.required) >= 2
    assert max(len(b.parents) for b in w.batches) <= 64 and max(b.H for b in w.batches) <= 3
    assert sum(len(b.parents) for b in w.batches) == len(w.cases) <= PC.MAX_CASES
    P = w.s.params()
    assert np.array_equal(P, w.m.P)
    if key != "intermediate":                                  # the world runs the rules its name says
        want = {"boat": (0, 0, 0), "stare": (1, 0, 0), "stare-far": (1, 0, 0), "car": (2, 1, 1), "escape": (0, 0, 0),
                "stare-clip": (1, 1, 1), "velocity-scale": (2, 0, 0), "empty": (0, 0, 0), "floor": (0, 0, 0)}[key]
        assert (int(P[38]), int(P[41]), int(P[42])) == want
        assert (len(w.s.obs) == 0) == (key == "empty") and w.s.vps.shape[1] == 1512
        assert (P[37] == 0.0) == (key == "escape")


def test_required_lists_name_what_the_worlds_are_for():
    """The lists are fixed text: every behaviour the parameter words select is required somewhere."""
    everything = set(c for key in PC.KEYS for c in PC.required(key))
    for c in (["heading:Ke-used", "heading:Ke-replaced", "focus:ahead", "focus:abeam", "focus:far", "sat0:remap", "sat0:floor-binds",
               "sat1:clipped", "thrusters:none-saturated", "norev-off:negative-kept", "empty:through-obstacle"]
              + PC.ASTERN + PC.ON_BOAT + PC.SAT0_EXACT + PC.ALONE + PC.NOREV + PC.DRAG + PC.ENDS + PC.SWEEP + CC.TORQUE_ARMS):
        assert c in everything, c
    for key in ("car", "intermediate"):
        assert set(CC.TORQUE_ARMS) <= set(PC.required(key))
    assert len(PC.ENDS) == 3 * 6 and set(PC.ENDS) <= set(PC.required("boat")) and set(PC.ENDS) <= set(PC.required("intermediate"))


@pytest.mark.parametrize("key", PC.KEYS)
def test_reference_equals_c_oracle_on_every_case(key):
    w = PC.world(key)
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


@pytest.mark.parametrize("key", PC.KEYS)
def test_c_oracle_step_means_the_reference_behaviour(key):
    """One step of the NumPy port of the reference's behaviour against the C oracle's, on every labelled step.  Left out: steps
    whose surge before the no-reverse rule lies within 1e-9 of zero, where another libm may take the
    other side -- at most a tenth of the world's labelled steps, and no category may lose a case to it."""
    w = PC.world(key)
    ref = PC.make_np_system(key)
    labelled = checked = 0
    kept = collections.Counter()
    for c in w.cases:
        seen = set()
        for k, (x, u, labels) in enumerate(c.steps):
            if not labels:
                continue
            labelled += 1
            if any(t in labels for t in PC.LIBM_THRESHOLD):
                continue
            checked += 1
            seen |= labels
            xc = w.o.dynamics(x, u)
            np.testing.assert_array_equal(xc, c.rollout.xall[k])                     # (the step the rollout took)
            xn = ref.dynamics(np.copy(x), np.copy(u), PC.DT)
            np.testing.assert_allclose(xn, xc, rtol=0, atol=PC.ATOL, err_msg="%s: x = %r u = %r (%s)" % (key, x, u, sorted(labels)))
        kept.update(seen)
    assert labelled and labelled - checked <= 0.1 * labelled, (labelled, checked)
    step_cats = set(c for case in w.cases for _, _, labels in case.steps for c in labels) - set(PC.LIBM_THRESHOLD)
    lost = {c: (w.coverage[c], kept[c]) for c in step_cats if kept[c] != w.coverage[c]}
    assert not lost, lost
