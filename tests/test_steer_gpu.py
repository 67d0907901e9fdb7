"""
GPU: every hand-written form of the rollout against the plain reference (tests/steer_reference.py), BIT FOR BIT, on the directed
case list of tests/steer_cases.py -- the stop rules (infeasible step and its FPR cut, error growth, horizon, convergence) at
their first / last steps and on their <= boundaries, the hand-over of a truncated edge (node, cos/sin and gain from the history),
the strict goal flag one ulp either side of the box, every batch slot, launches of one and launches without a single node.

Forms: in process with the defaults (one wavefront: pendulum; plain two: car, boat_novice, double_integrator; the chain of three:
the torque boats at W <= 512; four sharing the Riccati gain), and one subprocess per environment switch (they are read once) for
the two-wavefront boat form, the chain / duo choice by launch size and the one-wavefront Riccati form.  lqrrt_steer_force, a
sixth copy of the loop, gets its arrival boundary, its step cap, the FPR cuts and its argument errors.

Outputs are handed over pre-filled with NaN, so "rows at or beyond len are zero" is what the launch wrote, not what the
allocator left.  There is no tolerance anywhere in this file.
"""
import hashlib
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import steer_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

FIELDS = ("len", "xseq", "useq", "xend", "Kend", "goal", "grew", "steps", "rec_len")


def _engine(s, nodes):
    from lqrrt_amd.engine import Engine
    return Engine(s, capacity=nodes + 64 + 8, max_wave=64)


def steer_raw(eng, rec, lay, parents, xtar):
    """Engine.steer_batch with NaN-filled outputs, plus len / flags of the wave records."""
    import torch
    from lqrrt_amd import _native as nat
    W, H, n, m = len(xtar), eng.horizon_iters, eng.n, eng.m
    dev = "cuda:%d" % eng.device
    dp = torch.from_numpy(np.ascontiguousarray(parents, dtype=np.int32)).to(dev)
    dx = eng._dev(xtar, (W, n))
    ln = torch.full((W,), -7, dtype=torch.int32, device=dev)
    xs, us = (torch.full((W, H, k), float("nan"), dtype=torch.float64, device=dev) for k in (n, m))
    xe = torch.full((W, n), float("nan"), dtype=torch.float64, device=dev)
    Ke = torch.full((W, m, n), float("nan"), dtype=torch.float64, device=dev)
    nat.check(nat.lib().lqrrt_steer_batch(eng.h, dp.data_ptr(), dx.data_ptr(), W, ln.data_ptr(), xs.data_ptr(), us.data_ptr(),
                                          xe.data_ptr(), Ke.data_ptr(), eng._stream()))
    r = rec[:W].cpu().numpy()
    flags = r[:, lay[4]].astype(np.int64)
    return dict(len=ln.cpu().numpy(), xseq=xs.cpu().numpy(), useq=us.cpu().numpy(), xend=xe.cpu().numpy(), Kend=Ke.cpu().numpy(),
                goal=flags & 1, grew=(flags >> 1) & 1, steps=flags >> 8, rec_len=r[:, lay[3]].astype(np.int64))


def run_batches(s, dt, states, K, pID, batches):
    """Every batch through tree_load / set_resolution / steer_batch on one engine; a list of output dicts."""
    from lqrrt_amd.parallel import records_tensor
    eng = _engine(s, len(states))
    out = [None] * len(batches)
    loaded = None
    rec = lay = None
    for bi in sorted(range(len(batches)), key=lambda i: batches[i]["H"]):
        b = batches[bi]
        eng.set_resolution(dt, b["FPR"], b["H"], b["tol"], b["goal"], b["buf"], adaptive=b["adaptive"], hspan_min=1,
                           horizon_iters_state=b["H"])
        if loaded != b["H"]:                                       # (a new horizon re-lays the edge pools out and empties the tree)
            eng.tree_load(states, K, pID)
            loaded = b["H"]
            rec, lay = records_tensor(eng), eng.record_layout()
        assert int(b["parents"].max()) < len(states) and int(b["parents"].min()) >= 0
        out[bi] = steer_raw(eng, rec, lay, b["parents"], b["targets"])
    eng.close()
    return out


def _plain(c):
    return dict(dt=c.dt, states=c.states, K=c.K, pID=c.pID,
                batches=[dict(H=b.H, FPR=b.FPR, adaptive=b.adaptive, tol=b.tol, goal=b.goal, buf=b.buf, parents=b.parents,
                              targets=b.targets) for b in c.batches])


def _compare(c, outs, what):
    for bi, (b, got) in enumerate(zip(c.batches, outs)):
        want = c.expected_arrays(bi)
        where = "%s %s batch %d (%s: H=%d FPR=%g adaptive=%d W=%d)" % (what, c.name, bi, b.tag, b.H, b.FPR, b.adaptive, len(b.parents))
        for k in ("len", "goal", "grew", "steps", "xseq", "useq", "xend", "Kend"):
            np.testing.assert_array_equal(got[k], want[k], err_msg="%s: %s" % (where, k))
        np.testing.assert_array_equal(got["rec_len"], want["len"], err_msg="%s: record len" % where)
    # the same four cases alone and inside a launch of five
    a, b5 = (outs[i] for i in c.four)
    for k in FIELDS:
        np.testing.assert_array_equal(a[k], b5[k][:4], err_msg="%s %s: W = 4 against W = 5, %s" % (what, c.name, k))


@pytest.mark.parametrize("name", SC.NAMES)
def test_rollout_forms_by_default(name):
    c = SC.cases(name)
    p = _plain(c)
    _compare(c, run_batches(c.s, p["dt"], p["states"], p["K"], p["pID"], p["batches"]), "defaults")


# ---- the forms behind the environment switches: one process per setting ---------------------------------------------------

CHILD = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import test_steer_gpu
test_steer_gpu.child(sys.argv[1], sys.argv[2])
""" % (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"))


def _digest(outs):
    h = hashlib.sha256()
    for name in sorted(outs):
        for o in outs[name]:
            for k in FIELDS:
                h.update(np.ascontiguousarray(o[k]).tobytes())
    return h.hexdigest()


def child(path_in, path_out):
    with open(path_in, "rb") as f:
        work = pickle.load(f)
    outs = {}
    for name in sorted(work):
        p = work[name]
        outs[name] = run_batches(SC.make_system(name), p["dt"], p["states"], p["K"], p["pID"], p["batches"])
        print("CASES", name, len(outs[name]), " ".join("%d:%s" % (bi, ",".join(str(v) for v in o["len"])) for bi, o in enumerate(outs[name])))
    with open(path_out, "wb") as f:
        pickle.dump(outs, f)
    print("DIGEST", _digest(outs))


@pytest.fixture(scope="module")
def work_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("steer") / "cases.pkl")
    with open(path, "wb") as f:
        pickle.dump({name: _plain(SC.cases(name)) for name in SC.NAMES}, f)
    return path


@pytest.mark.parametrize("switch,value", [("LQRRT_STEER_WAVEFRONTS", "2"), ("LQRRT_STEER_TRIO_MAX", "4"), ("LQRRT_DARE_WAVEFRONTS", "1")])
def test_rollout_forms_behind_switches(work_file, switch, value):
    """LQRRT_STEER_WAVEFRONTS=2: the two-wavefront boat form with duo.fin.  LQRRT_STEER_TRIO_MAX=4: launches of up to four run
    the chain, larger ones the duo -- the same four cases at W = 4 and inside W = 5 must agree.  LQRRT_DARE_WAVEFRONTS=1: the
    one-wavefront Riccati rollout.  All systems in each process: a switch must not move any other system either."""
    env = dict(os.environ)
    for k in ("LQRRT_STEER_WAVEFRONTS", "LQRRT_STEER_TRIO_MAX", "LQRRT_DARE_WAVEFRONTS", "LQRRT_FUSED_ROUNDS"):
        env.pop(k, None)
    env[switch] = value
    path_out = work_file + "." + switch + ".out"
    run = subprocess.run([sys.executable, "-c", CHILD, work_file, path_out], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    with open(path_out, "rb") as f:
        outs = pickle.load(f)
    line = [l for l in run.stdout.splitlines() if l.startswith("DIGEST")][-1]
    assert line.split()[1] == _digest(outs)
    assert sorted(outs) == sorted(SC.NAMES)
    for name in SC.NAMES:
        _compare(SC.cases(name), outs[name], "%s=%s" % (switch, value))


# ---- lqrrt_steer_force ------------------------------------------------------------------------------------------------------

def force_raw(eng, parent, xt, max_steps, rtol, atol, rows):
    import torch
    from lqrrt_amd import _native as nat
    dev = "cuda:%d" % eng.device
    dx = eng._dev(xt, (eng.n,))
    ln = torch.full((1,), -7, dtype=torch.int32, device=dev)
    xs, us = (torch.full((rows, k), float("nan"), dtype=torch.float64, device=dev) for k in (eng.n, eng.m))
    rc = nat.lib().lqrrt_steer_force(eng.h, int(parent), dx.data_ptr(), int(max_steps), float(rtol), float(atol), ln.data_ptr(),
                                     xs.data_ptr(), us.data_ptr(), eng._stream())
    torch.cuda.synchronize()
    return rc, int(ln.cpu()[0]), xs.cpu().numpy(), us.cpu().numpy()


@pytest.mark.parametrize("name", SC.NAMES)
def test_steer_force(name):
    from lqrrt_amd import _native as nat
    c = SC.cases(name)
    eng = _engine(c.s, len(c.states))
    fpr = None
    for f in sorted(c.forced, key=lambda f: f.FPR):
        if f.FPR != fpr:
            eng.set_resolution(c.dt, f.FPR, 6, np.zeros(c.n), None, None)
            if fpr is None:
                eng.tree_load(c.states, c.K, c.pID)
            fpr = f.FPR
        r = c.expected_forced(f)
        rc, ln, xs, us = force_raw(eng, f.parent, f.target, f.max_steps, f.rtol, f.atol, f.max_steps + 2)
        where = "%s %s (%s)" % (name, f.cat, r.reason,)
        assert rc == 0 and ln == len(r.xs), where
        np.testing.assert_array_equal(xs[:ln], r.xs, err_msg=where)
        np.testing.assert_array_equal(us[:ln], r.us, err_msg=where)
        # Never past the cap.  Rows in [len, max_steps) are left unconstrained on purpose: the kernel writes each step where it
        # is recorded, so after an FPR cut they hold the dropped steps -- steer_force has no "rows beyond len are zero" rule.
        assert np.isnan(xs[f.max_steps:]).all() and np.isnan(us[f.max_steps:]).all(), where
    # argument errors: a parent outside the tree, no steps; nothing is written
    f = c.forced[0]
    for parent, max_steps in ((len(c.states), 4), (-1, 4), (f.parent, 0)):
        rc, ln, xs, us = force_raw(eng, parent, f.target, max_steps, 0.0, 0.0, 4)
        assert rc == nat.E_ARG and ln == -7 and np.isnan(xs).all() and np.isnan(us).all(), (parent, max_steps)
    with pytest.raises(Exception):
        eng.steer_force(len(c.states), f.target, 4)
    eng.close()
