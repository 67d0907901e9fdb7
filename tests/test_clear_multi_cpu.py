"""
The clearance queries for several trees per launch (lqrrt_tree_clear_multi / lqrrt_tree_clear_wait_multi, Engine.tree_clear_multi /
tree_clear_wait_multi, lqrrt_amd.avoids, deconflict(batched=True); csrc/clear_multi.hpp) on the CPU: the round scheduler of the
batched deconflict with a synthetic `ask`, the ABI's declarations and the binding, the refusals of the public calls before any
planner is touched, and what the sources and the compiler say about the new kernels.
"""
import ctypes as C
import os
import re
import shutil
import sys

import numpy as np
import pytest

import lqrrt
import lqrrt_amd
from lqrrt_amd import _native as nat
from lqrrt_amd import planner as planner_mod
from lqrrt_amd.engine import Engine
from clear_common import FORBIDDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lqrrt_amd", "csrc")


# ------------------------------------------------------------------------------------------------ the round scheduler

def _sequential(order, entry, answer):
    """The loop deconflict() runs: position by position, each against the final candidates of those before it."""
    cand = list(entry)
    for at, k in enumerate(order):
        if at > 0:
            cand[k] = answer(k, [cand[j] for j in order[:at]])
    return cand


class Asker(object):
    """ask() of _deconflict_rounds from a per-planner rule `answer(k, candidates of those before k)`; keeps what each round asked."""

    def __init__(self, order, answer):
        self.order, self.answer, self.rounds, self.changed_at = list(order), answer, [], []

    def __call__(self, ks, cand):
        self.rounds.append(list(ks))
        out, changed = [], []
        for k in ks:
            before = self.order[:self.order.index(k)]
            c = self.answer(k, [cand[j] for j in before])
            if c != cand[k]:
                changed.append(self.order.index(k))
            out.append((c, ("answer", k, len(self.rounds))))
        self.changed_at.append(min(changed) if changed else None)
        return out


def test_a_change_cascades_down_all_positions():
    """n = 6, planner k's answer = 1 + the candidate of the planner right before it (the first holds 10, the others 0): against the
    entry candidates only position 1 changes in round 1, then position 2 in round 2, ... -- the worst case."""
    n = 6
    order = [3, 0, 5, 1, 4, 2]
    entry = [0] * n
    entry[order[0]] = 10
    answer = lambda k, before: before[-1] + 1
    want = _sequential(order, entry, answer)
    assert [want[k] for k in order] == [10, 11, 12, 13, 14, 15]
    ask = Asker(order, answer)
    cand, answers, log = planner_mod._deconflict_rounds(order, entry, ask)
    assert cand == want and log == ask.rounds
    assert len(log) == n - 1                                                      # the worst case: exactly n - 1 rounds, never more
    assert log[0] == order[1:]                                                    # round 1: everybody but the first of the order
    for r in range(1, len(log)):                                                  # round r + 1: only planners behind the earliest change of round r
        assert log[r] == order[ask.changed_at[r - 1] + 1:]
    # In round 1 every position but the first sees a neighbour that still holds its entry candidate, 0, and answers 1 -- except
    # position 1, which sees 10: all of them change, the earliest at position 1; from then on the earliest change moves down by one.
    assert ask.changed_at == [1, 2, 3, 4, 5]
    assert answers[order[0]] is None and all(answers[k][1] == k for k in order[1:])
    assert answers[order[-1]][2] == n - 1 and answers[order[1]][2] == 1           # the last answer kept is the last one given


def test_a_fleet_without_any_change_costs_one_round():
    order = [2, 0, 1, 3]
    entry = [7, 8, 9, 10]
    ask = Asker(order, lambda k, before: entry[k])
    cand, answers, log = planner_mod._deconflict_rounds(order, entry, ask)
    assert cand == entry and log == [order[1:]] and answers[2] is None and all(answers[k] is not None for k in (0, 1, 3))


def test_nothing_dirty_means_no_launch():
    def never(ks, cand):
        raise AssertionError("asked")
    assert planner_mod._deconflict_rounds([0], ["a"], never) == (["a"], [None], [])
    assert planner_mod._deconflict_rounds([], [], never) == ([], [], [])


@pytest.mark.parametrize("seed", range(8))
def test_random_rules_reach_the_sequential_answer_within_n_minus_1_rounds(seed):
    """Any rule that is a function of the candidates before a planner: the fixed point is the loop's answer."""
    rs = np.random.RandomState(seed)
    n = 7
    order = [int(k) for k in rs.permutation(n)]
    entry = [int(v) for v in rs.randint(0, 3, n)]
    salt = rs.randint(0, 1000, n)

    def answer(k, before):
        h = (sum((i + 1) * v for i, v in enumerate(before)) + int(salt[k])) % 4
        return entry[k] if h == 0 else h                                          # (h == 0: "no clear hit", the plan it came with)
    want = _sequential(order, entry, answer)
    ask = Asker(order, answer)
    cand, _, log = planner_mod._deconflict_rounds(order, entry, ask)
    assert cand == want and 1 <= len(log) <= n - 1
    for r in range(1, len(log)):
        assert log[r] == order[ask.changed_at[r - 1] + 1:] and ask.changed_at[r - 1] >= r


# ------------------------------------------------------------------------------------------------ header and binding

def test_header_declares_the_calls_and_the_binding_has_them():
    text = open(os.path.join(ROOT, "include", "lqrrt_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    plain = re.search(r"\bint lqrrt_tree_clear_multi\s*\((.*?)\);", code, re.S)
    wait = re.search(r"\bint lqrrt_tree_clear_wait_multi\s*\((.*?)\);", code, re.S)
    assert plain and wait
    assert len(plain.group(1).split(",")) == 11 and "lqrrt_clear_stats* out" in plain.group(1) and "lqrrt_engine** engines" in plain.group(1)
    assert len(wait.group(1).split(",")) == 12 and "lqrrt_clear_wait_stats* out" in wait.group(1) and "const int32_t* waits" in wait.group(1)
    for m in (plain, wait):
        assert m.group(1).count("const double* const*") == 2 and m.group(1).count("const int32_t*") >= 3
    I, P = C.c_int, C.c_void_p
    assert nat.SIGNATURES["lqrrt_tree_clear_multi"] == (I, [P, I] + [P] * 9)
    assert nat.SIGNATURES["lqrrt_tree_clear_wait_multi"] == (I, [P, I] + [P] * 10)
    assert hasattr(nat.lib(), "lqrrt_tree_clear_multi") and hasattr(nat.lib(), "lqrrt_tree_clear_wait_multi")
    assert nat.lib().lqrrt_abi_version() == 1
    assert callable(Engine.tree_clear_multi) and callable(Engine.tree_clear_wait_multi)
    assert isinstance(Engine.__dict__["tree_clear_multi"], staticmethod) and isinstance(Engine.__dict__["tree_clear_wait_multi"], staticmethod)
    assert "avoids" in lqrrt_amd.__all__ and "avoids" in lqrrt.__all__ and lqrrt.avoids is lqrrt_amd.avoids


def test_engine_methods_refuse_on_the_host():
    with pytest.raises(ValueError, match="no engines"):
        Engine.tree_clear_multi([], [], [], [])
    with pytest.raises(ValueError, match="per engine"):
        Engine.tree_clear_multi([object()], [np.zeros((2, 1, 2))], [0.5], [0, 0])
    with pytest.raises(ValueError, match="start"):
        Engine.tree_clear_multi([object()], [np.zeros((2, 1, 2))], [0.5], [-1])
    with pytest.raises(ValueError):
        Engine.tree_clear_multi([object()], [np.full((2, 1, 2), np.nan)], [0.5], [0])
    for waits in (0, 65, [1, 2], [True]):
        with pytest.raises(ValueError, match="wait"):
            Engine.tree_clear_wait_multi([object()], [np.zeros((2, 1, 2))], [0.5], [0], waits)


def _native_planner(dt=None):
    car = lqrrt_amd.systems.Car(0)
    cons = lqrrt_amd.Constraints(car.nstates, car.ncontrols, car.goal_buffer, car.is_feasible)
    kw = dict(car.plan_kwargs)
    if dt is not None:
        kw["dt"] = dt
    return lqrrt_amd.Planner(car.dynamics, car.lqr, cons, error_tol=car.error_tol, erf=car.erf, goal0=car.goal, printing=False, **kw)


def _callback_planner():
    cons = lqrrt_amd.Constraints(2, 1, [0.1, 0.1], lambda x, u: True)
    p = lqrrt_amd.Planner(lambda x, u, dt: x + dt * np.array([x[1], u[0]]), lambda x, u: (np.eye(2), np.array([[1.0, 1.0]])), cons,
                          horizon=1, dt=0.1, goal0=[1.0, 0.0], printing=False)
    assert p.callback_mode
    return p


def test_avoids_refuses_before_touching_a_planner():
    a, b = _native_planner(), _native_planner()
    good = np.zeros((3, 2, 2))
    for bad in (dict(tracks=np.zeros((0, 1, 2)), radii=0.5), dict(tracks=np.zeros((3, 2, 3)), radii=0.5), dict(tracks=[], radii=0.5),
                dict(tracks=good, radii=-0.1), dict(tracks=good, radii=[0.5, 0.5, 0.5]), dict(tracks=good, radii=0.5, start=-1),
                dict(tracks=good, radii=0.5, start=1.5), dict(tracks=np.full((3, 2, 2), np.nan), radii=0.5),
                dict(tracks=good, radii=0.5, max_wait=64), dict(tracks=good, radii=0.5, max_wait=-1), dict(tracks=good, radii=0.5, max_wait=1.0),
                dict(tracks=[good, good], radii=0.5),                             # tracks per planner, radii not
                dict(tracks=[good, good], radii=[0.5]),
                dict(tracks=[good, np.zeros((3, 0, 2))], radii=[0.5, 0.5])):
        with pytest.raises(ValueError):
            lqrrt_amd.avoids([a, b], **bad)
    with pytest.raises(ValueError, match="twice"):
        lqrrt_amd.avoids([a, a], good, 0.5)
    with pytest.raises(ValueError, match="Planner"):
        lqrrt_amd.avoids([a, "b"], good, 0.5)
    with pytest.raises(NotImplementedError, match="Python"):
        lqrrt_amd.avoids([a, _callback_planner()], good, 0.5)
    assert all(p.tree is None and not p.plan_reached_goal and not hasattr(p, "node_seq") for p in (a, b))
    # planners without a tree on the device: None each, as avoid; no device is needed for that
    assert lqrrt_amd.avoids([a, b], good, 0.5) == [None, None]
    assert lqrrt_amd.avoids([a, b], [good, [np.zeros((4, 2))]], [[0.5, 0.2], 0.3], start=2, adopt=False, max_wait=7) == [None, None]
    assert lqrrt_amd.avoids([], good, 0.5) == []
    assert all(p.tree is None and not hasattr(p, "node_seq") for p in (a, b))


def test_batched_deconflict_refuses_what_deconflict_refuses():
    a, b, c = _native_planner(), _native_planner(), _native_planner(dt=0.05)
    with pytest.raises(ValueError, match="share dt"):
        lqrrt_amd.deconflict([a, b, c], 0.5, batched=True)
    with pytest.raises(ValueError, match="twice"):
        lqrrt_amd.deconflict([a, a], 0.5, batched=True)
    with pytest.raises(ValueError, match="permutation"):
        lqrrt_amd.deconflict([a, b], 0.5, order=[0, 0], batched=True)
    for radii in (-1.0, [0.5], [0.5, 0.5, 0.5]):
        with pytest.raises(ValueError, match="radius"):
            lqrrt_amd.deconflict([a, b], radii, batched=True)
    with pytest.raises(ValueError, match="start"):
        lqrrt_amd.deconflict([a, b], 0.5, start=-1, batched=True)
    with pytest.raises(ValueError, match="max_wait"):
        lqrrt_amd.deconflict([a, b], 0.5, max_wait=64, batched=True)
    with pytest.raises(ValueError, match="no plan"):
        lqrrt_amd.deconflict([a, b], 0.5, batched=True)
    with pytest.raises(NotImplementedError, match="Python"):
        lqrrt_amd.deconflict([_callback_planner()], 0.5, batched=True)
    assert all(p.tree is None and not hasattr(p, "node_seq") for p in (a, b, c))
    doc = lqrrt_amd.deconflict.__doc__
    assert "batched=True" in doc and "induction" in doc and "n - 1" in doc and "worst case" in doc


# ------------------------------------------------------------------------------------------------ sources

def test_the_new_files_stay_plain_launches_and_transient():
    kern = open(os.path.join(CSRC, "clear_multi.hpp")).read()
    host = open(os.path.join(CSRC, "engine_clear_multi.hpp")).read()
    for name, text in (("clear_multi.hpp", kern), ("engine_clear_multi.hpp", host)):
        for word in FORBIDDEN:
            assert word not in text, (name, word)
    # the bodies, links and joins are the solo files'; the step sums are the retain's batched kernels
    for body in ("clear_check_body<S>(", "clear_wait_check_body<S>(", "clear_select_body(", "clear_wait_select_body(", "Link::join(", "Link::FIELD"):
        assert body in kern, body
    assert "__device__" not in kern                                                # (kernels only: no per-node body of its own)
    assert "idempotent" in kern and "identity" in kern and "INCLUSIVE" in kern     # why the extra rounds are harmless
    assert "k_retain_init_multi" in host and "k_retain_double_multi" in host and "r.root = 0" in host and "r.revalidate = 0" in host
    # refusals: the solo calls' checker, reused; the engine list as the other multi calls check it; the engine is named
    assert "clear_check<typename M::Solo>(" in host and "multi_engines_check(" in host and "engine_suffix(k)" in host
    assert "static int clear_check(" not in host
    assert "multi_chunks(" in host and "multi_grid(" in host and "multi_sync_proto(" in host
    # memory: transient only, behind a StreamDrain that is armed before the first copy; one synchronise
    assert "dalloc(" not in host and "hipMalloc" not in host and host.count("dalloc_transient(") == 1
    run = host[host.index("static int clear_multi_run("):host.index("static int clear_multi_call(")]
    assert run.index("ClearMultiScratch sc;") < run.index("StreamDrain drain(st);") < run.index("drain.arm();") < run.index("dalloc_transient(") \
        < run.index("hipMemcpyAsync(")
    assert run.count("hipStreamSynchronize(") == 1 and run.index("hipStreamSynchronize(st)") < run.index("drain.disarm();")
    assert "fail(" not in run                                                      # the run refuses nothing
    call = host[host.index("static int clear_multi_call("):]
    assert call.index("TRY(clear_multi_check<M>(") < call.index("clear_multi_run<M>(")
    check = host[host.index("static int clear_multi_check("):host.index("static int clear_multi_run(")]
    for work in ("dalloc", "hipMemcpy", "hipLaunchKernelGGL"):
        assert work not in check and work not in call
    # where the fragments stand
    kernels = open(os.path.join(CSRC, "kernels.hpp")).read()
    assert kernels.index('#include "clear_wait.hpp"') < kernels.index('#include "clear_multi.hpp"')
    engine = open(os.path.join(CSRC, "engine.hip")).read()
    assert engine.index('#include "engine_clear.hpp"') < engine.index('#include "engine_clear_multi.hpp"')
    # the traits are extended from the new file only
    assert "struct ClearPlainMulti : ClearPlain" in host and "struct ClearWaitMulti : ClearWait" in host
    solo = open(os.path.join(CSRC, "engine_clear.hpp")).read()
    assert "multi" not in solo.lower()


def test_check_kernels_stay_in_the_class_of_the_retain_check():
    """For every model with a circle path k_clear_check_multi<S> and k_clear_wait_check_multi<S> exist, and for no other model; no
    private segment, at least the occupancy of k_retain_check<S>, and the wait check's static LDS within its 64 bytes."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    assert shutil.which(kr.HIPCC) or os.path.exists(kr.HIPCC), "hipcc is what builds the package: it cannot be missing here"
    user = os.path.join(ROOT, "examples", "user_system", "unicycle.hpp")
    rows = kr.parse(kr.remarks(["-DLQRRT_USER_SYSTEM=\"%s\"" % user]))

    def by_model(kernel):
        out = {}
        for r in rows:
            m = re.match(r"void lq::%s<lq::(.+?) ?>\(" % kernel, r["name"])
            if m:
                out[m.group(1)] = r
        return out
    retain, plain, wait = by_model("k_retain_check"), by_model("k_clear_check_multi"), by_model("k_clear_wait_check_multi")
    discs = ["BoatAdvanced", "BoatIntermediate", "BoatNovice", "BoatNoviceLqr", "Car", "RosBoat"]
    assert sorted(plain) == discs == sorted(wait)
    assert "UserSystem" in retain and "Pendulum" in retain
    for model in discs:
        for what, k in (("clear check multi", plain[model]), ("wait check multi", wait[model])):
            print("%-18s retain check %3d B occ %d vgpr %3d   %-17s %3d B occ %d vgpr %3d sgpr %3d lds %d" % (
                model, retain[model]["scratch"], retain[model]["occupancy"], retain[model]["vgpr"], what, k["scratch"], k["occupancy"],
                k["vgpr"], k.get("sgpr", -1), k["lds"]))
            assert k["scratch"] == 0 == retain[model]["scratch"]
            assert k["occupancy"] >= retain[model]["occupancy"]
        assert plain[model]["lds"] == 0 and wait[model]["lds"] <= 64               # (static; the hull is dynamic)
    names = [r["name"] for r in rows]
    for kernel in ("k_clear_init_multi<lq::ClearLink>", "k_clear_init_multi<lq::ClearWaitLink>", "k_clear_double_multi<lq::ClearLink>",
                   "k_clear_double_multi<lq::ClearWaitLink>", "k_clear_select_multi(", "k_clear_wait_select_multi("):
        hit = [r for r in rows if ("lq::" + kernel) in r["name"]]
        assert len(hit) == 1 and hit[0]["scratch"] == 0, (kernel, names[:3])
