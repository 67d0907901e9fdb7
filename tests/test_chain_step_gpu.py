"""
GPU: lqrrt_steer_batch on BoatAdvanced against the plain reference (tests/steer_reference.py), BIT FOR BIT, on the directed case
list of tests/chain_step_cases.py -- the choices inside one step of the chain rollout (arm of the heading torque, saturating
thruster, sign of each velocity, car-like rule), rollouts that end on step H + 1 for H = 1, 2, 3, and the feasibility sweep with
0 .. 6 obstacles inside the cull box, a hull point on the threshold of the squared distance and one ulp either side, hulls of
28 / 33 / 65 points and tables of 36 / 65 obstacles.  tests/test_chain_step_cpu.py proves, without a GPU, that the reference
puts two cases into every category.

In process the launches (W <= 64) run the chain of three wavefronts; one subprocess runs the same cases with
LQRRT_STEER_WAVEFRONTS=2, the two-wavefront form, as the control.  Outputs are handed over pre-filled with NaN; there is no
tolerance anywhere in this file.
"""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import chain_step_cases as CC
from test_steer_gpu import FIELDS, run_batches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _compare(w, outs, what):
    missing = {c: w.coverage[c] for c in w.required if w.coverage[c] < 2}
    assert not missing, "%s: categories with fewer than two cases: %r" % (w.name, missing)
    for bi, (b, got) in enumerate(zip(w.batches, outs)):
        want = w.expected_arrays(bi)
        where = "%s batch %d (%s, W=%d)" % (what, bi, b.tag, len(b.parents))
        for k in ("len", "goal", "grew", "steps", "xseq", "useq", "xend", "Kend"):
            np.testing.assert_array_equal(got[k], want[k], err_msg="%s: %s" % (where, k))
        np.testing.assert_array_equal(got["rec_len"], want["len"], err_msg="%s: record len" % where)


def _run(p):
    w = CC.world(p["kind"], p["V"], p["O"])                    # (the system with this world's hull and table; cached per process)
    return run_batches(w.s, p["dt"], p["states"], p["K"], p["pID"], p["batches"])


@pytest.mark.parametrize("kind,V,O", CC.KINDS)
def test_chain_rollout(kind, V, O):
    w = CC.world(kind, V, O)
    _compare(w, _run(w.plain()), "chain")


# ---- the control: the two-wavefront form, one process for all worlds (the switch is read once) -----------------------------

CHILD = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import test_chain_step_gpu
test_chain_step_gpu.child(sys.argv[1], sys.argv[2])
""" % (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"))


def child(path_in, path_out):
    with open(path_in, "rb") as f:
        work = pickle.load(f)
    outs = [_run(p) for p in work]
    with open(path_out, "wb") as f:
        pickle.dump(outs, f)
    print("DONE", len(outs))


def test_two_wavefront_control(tmp_path):
    worlds = [CC.world(*k) for k in CC.KINDS]
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
