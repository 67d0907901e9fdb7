"""
GPU: the rollout step of RosBoat and BoatIntermediate, every spelling of it that a one-tree launch runs, against the plain
reference (tests/steer_reference.py over the C oracle), BIT FOR BIT, on the directed case list of tests/packed_step_cases.py --
RosBoat's heading modes, saturation rules and no-reverse rule (the three shipped behaviours, two crossings of them, an empty
obstacle table, a thrust limit below the ratio's floor), the intermediate boat's per-axis saturation on |u| == u_max and its
car-like rule, and rollouts that end on step H + 1 for H = 1, 2, 3.  tests/test_packed_step_cpu.py proves, without a GPU, that
the reference puts two cases into every category.

  * lqrrt_steer_batch in process: W <= 64, the chain of three wavefronts (trio_effort / quad_effort, duo_chain, duo_finish).
  * The same cases in one subprocess with LQRRT_STEER_WAVEFRONTS=2: the two-wavefront form (duo_effort, duo_chain, duo_finish).
  * lqrrt_dynamics_batch on every evaluated step (x_k-1, u_k) of every reference rollout, the last, unrecorded one included:
    the plain S::step at exactly the labelled states.
  * lqrrt_steer_force (k_steer_force, S::step in a loop) from the parents of up to eight cases per world.

step_packed is not run here: no launch instantiates k_steer<S, *, 1> for a PACKED system (steer_wavefronts gives them 2 or 3);
only the fleet launch's k_steer_multi<S, *, 1> (engine_multi.hpp) reaches it.

Outputs are handed over pre-filled with NaN; there is no tolerance anywhere in this file.
"""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import packed_step_cases as PC
import steer_reference as R
from test_chain_step_gpu import _compare
from test_steer_gpu import FIELDS, _engine, force_raw, run_batches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _run(p):
    return run_batches(PC.make_system(p["key"]), p["dt"], p["states"], p["K"], p["pID"], p["batches"])


@pytest.mark.parametrize("key", PC.KEYS)
def test_chain_rollout(key):
    w = PC.world(key)
    _compare(w, _run(w.plain()), "chain")


# ---- the control: the two-wavefront form, one process for all worlds (the switch is read once) -----------------------------

CHILD = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import test_packed_step_gpu
test_packed_step_gpu.child(sys.argv[1], sys.argv[2])
""" % (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"))


def child(path_in, path_out):
    with open(path_in, "rb") as f:
        work = pickle.load(f)
    outs = [_run(p) for p in work]
    with open(path_out, "wb") as f:
        pickle.dump(outs, f)
    print("DONE", len(outs))


def test_two_wavefront_control(tmp_path):
    worlds = [PC.world(k) for k in PC.KEYS]
    path_in, path_out = str(tmp_path / "cases.pkl"), str(tmp_path / "outs.pkl")
    with open(path_in, "wb") as f:
        pickle.dump([w.plain() for w in worlds], f)
    env = dict(os.environ)
    for k in ("LQRRT_STEER_WAVEFRONTS", "LQRRT_STEER_TRIO_MAX", "LQRRT_DARE_WAVEFRONTS", "LQRRT_FUSED_ROUNDS"):
        env.pop(k, None)
    env["LQRRT_STEER_WAVEFRONTS"] = "2"
    run = subprocess.run([sys.executable, "-c", CHILD, path_in, path_out], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    assert "DONE %d" % len(worlds) in run.stdout
    with open(path_out, "rb") as f:
        outs = pickle.load(f)
    for w, o in zip(worlds, outs):
        assert sorted(o[0]) == sorted(FIELDS)
        _compare(w, o, "LQRRT_STEER_WAVEFRONTS=2")


# ---- the plain step ---------------------------------------------------------------------------------------------------------

def dynamics_raw(eng, x, u):
    """lqrrt_dynamics_batch with a NaN-filled output."""
    import torch
    from lqrrt_amd import _native as nat
    B = len(x)
    dx, du = eng._dev(x, (B, eng.n)), eng._dev(u, (B, eng.m))
    out = torch.full((B, eng.n), float("nan"), dtype=torch.float64, device=dx.device)
    nat.check(nat.lib().lqrrt_dynamics_batch(eng.h, dx.data_ptr(), du.data_ptr(), B, out.data_ptr(), eng._stream()))
    return out.cpu().numpy()


@pytest.mark.parametrize("key", PC.KEYS)
def test_plain_step(key):
    w = PC.world(key)
    rows = [(x, u, c.rollout.xall[k], ci) for ci, c in enumerate(w.cases) for k, (x, u, _) in enumerate(c.steps)]
    assert all(len(c.steps) == len(c.rollout.xall) >= 1 for c in w.cases)
    eng = _engine(w.s, 1)
    eng.set_resolution(PC.DT, 0.0, 1, np.zeros(w.n), None, None)
    got = dynamics_raw(eng, np.array([r[0] for r in rows]), np.array([r[1] for r in rows]))
    eng.close()
    want = np.array([r[2] for r in rows])
    bad = sorted({rows[i][3] for i in np.nonzero((got != want).any(axis=1))[0]})
    np.testing.assert_array_equal(got, want, err_msg="%s: cases %r" % (key, [(i, sorted(w.cases[i].labels)) for i in bad[:4]]))


# ---- lqrrt_steer_force ------------------------------------------------------------------------------------------------------

FORCED_PREFIXES = ("heading:", "focus:", "sat0:", "sat1:", "thruster", "norev", "axis", "carlike:")
FORCED_STEPS = 4


def forced_picks(w):
    """The first case of each heading, saturation and no-reverse category, eight at the most."""
    picks, seen = [], set()
    for c in w.cases:
        new = {l for l in c.labels if l.startswith(FORCED_PREFIXES)} - seen
        if new and c.steps[0][2]:                              # (its first step is a labelled one)
            picks.append(c)
            seen |= new
        if len(picks) == 8:
            break
    return picks


@pytest.mark.parametrize("key", PC.KEYS)
def test_steer_force(key):
    w = PC.world(key)
    picks = forced_picks(w)
    assert picks
    eng = _engine(w.s, len(w.states))
    eng.set_resolution(PC.DT, 0.9, 6, np.zeros(w.n), None, None)
    eng.tree_load(w.states, w.K, w.pID)
    for c in picks:
        r = R.steer_force(w.ops, w.states[c.pid], w.K[c.pid], c.target, PC.DT, 0.9, 0.0, 0.0, FORCED_STEPS)
        rc, ln, xs, us = force_raw(eng, c.pid, c.target, FORCED_STEPS, 0.0, 0.0, FORCED_STEPS + 2)
        where = "%s parent %d (%s) %r" % (key, c.pid, r.reason, sorted(c.labels))
        assert rc == 0 and ln == len(r.xs), where
        np.testing.assert_array_equal(xs[:ln], r.xs, err_msg=where)
        np.testing.assert_array_equal(us[:ln], r.us, err_msg=where)
        assert np.isnan(xs[FORCED_STEPS:]).all() and np.isnan(us[FORCED_STEPS:]).all(), where
        if ln:                                                 # the gain the next edge would start with
            np.testing.assert_array_equal(eng.gain_batch(xs[ln - 1:ln], us[ln - 1:ln])[0], r.K_end, err_msg=where)
    eng.close()
