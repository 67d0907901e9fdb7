"""
The rectangle clearance queries for several trees per launch (lqrrt_tree_clear_rects_multi / lqrrt_tree_clear_rects_wait_multi,
Engine.tree_clear_rects_multi / tree_clear_rects_wait_multi, lqrrt_amd.avoids_rects; csrc/clear_rects_multi.hpp) on the CPU: the
ABI's declarations and the binding, the refusals of the public calls before any planner is touched, what the sources and the
compiler say about the two new kernels, and -- with the NumPy references alone -- that no input of
tests/test_clear_rects_multi_gpu.py is degenerate.
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
from lqrrt_amd.engine import Engine
from clear_common import FORBIDDEN

import clear_reference as cl
import clear_rects_reference as cr
import clear_rects_wait_reference as rw
import clear_rects_multi_inputs as mi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lqrrt_amd", "csrc")
E = (1.0, 0.5)


# ------------------------------------------------------------------------------------------------ header and binding

def test_header_declares_the_calls_and_the_binding_has_them():
    text = open(os.path.join(ROOT, "include", "lqrrt_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    plain = re.search(r"\bint lqrrt_tree_clear_rects_multi\s*\((.*?)\);", code, re.S)
    wait = re.search(r"\bint lqrrt_tree_clear_rects_wait_multi\s*\((.*?)\);", code, re.S)
    assert plain and wait
    assert len(plain.group(1).split(",")) == 11 and "lqrrt_clear_stats* out" in plain.group(1) and "lqrrt_engine** engines" in plain.group(1)
    assert len(wait.group(1).split(",")) == 12 and "lqrrt_clear_wait_stats* out" in wait.group(1) and "const int32_t* waits" in wait.group(1)
    for m in (plain, wait):
        assert m.group(1).count("const double* const*") == 2 and m.group(1).count("const int32_t*") >= 3
        assert "extents_host" in m.group(1) and "radii" not in m.group(1)
    # the rule stands next to the declarations, by reference to the solo calls
    doc = text[text.index("/* lqrrt_tree_clear_rects and lqrrt_tree_clear_rects_wait for n engines"):text.index("int lqrrt_tree_clear_rects_multi(")]
    doc = " ".join(doc.replace("\n *", " ").split())                                # (the comment's line breaks fall where they fall)
    for word in ("exactly what the one-tree call", "lqrrt_tree_clear_multi's comment", "(engine k)", "section 23", "writes nothing into any output"):
        assert word in doc, word
    I, P = C.c_int, C.c_void_p
    assert nat.SIGNATURES["lqrrt_tree_clear_rects_multi"] == (I, [P, I] + [P] * 9)
    assert nat.SIGNATURES["lqrrt_tree_clear_rects_wait_multi"] == (I, [P, I] + [P] * 10)
    assert hasattr(nat.lib(), "lqrrt_tree_clear_rects_multi") and hasattr(nat.lib(), "lqrrt_tree_clear_rects_wait_multi")
    assert nat.lib().lqrrt_abi_version() == 1
    assert callable(Engine.tree_clear_rects_multi) and callable(Engine.tree_clear_rects_wait_multi)
    assert isinstance(Engine.__dict__["tree_clear_rects_multi"], staticmethod)
    assert isinstance(Engine.__dict__["tree_clear_rects_wait_multi"], staticmethod)
    assert "avoids_rects" in lqrrt_amd.__all__ and "avoids_rects" in lqrrt.__all__ and lqrrt.avoids_rects is lqrrt_amd.avoids_rects


# ------------------------------------------------------------------------------------------------ refusals without a device

def test_engine_methods_refuse_on_the_host():
    good = np.zeros((2, 1, 3))
    with pytest.raises(ValueError, match="no engines"):
        Engine.tree_clear_rects_multi([], [], [], [])
    with pytest.raises(ValueError, match="no engines"):
        Engine.tree_clear_rects_wait_multi([], [], [], [], 8)
    with pytest.raises(ValueError, match="per engine"):
        Engine.tree_clear_rects_multi([object()], [good], [E], [0, 0])
    with pytest.raises(ValueError, match="per engine"):
        Engine.tree_clear_rects_multi([object()], [good, good], [E], [0])
    with pytest.raises(ValueError, match="per engine"):
        Engine.tree_clear_rects_wait_multi([object()], [good], [E, E], [0], 8)
    with pytest.raises(ValueError, match="start"):
        Engine.tree_clear_rects_multi([object()], [good], [E], [-1])
    with pytest.raises(ValueError, match="start"):
        Engine.tree_clear_rects_multi([object()], [good], [E], [2 ** 31])
    with pytest.raises(ValueError, match="finite"):
        Engine.tree_clear_rects_multi([object()], [np.full((2, 1, 3), np.nan)], [E], [0])
    with pytest.raises(ValueError, match="tracks"):
        Engine.tree_clear_rects_multi([object()], [np.zeros((2, 1, 2))], [E], [0])       # a disc table is no rectangle table
    with pytest.raises(ValueError, match="[Ee]xtent"):
        Engine.tree_clear_rects_multi([object()], [good], [(1.0, -0.5)], [0])
    for waits in (0, 65, [1, 2], [True]):
        with pytest.raises(ValueError, match="wait"):
            Engine.tree_clear_rects_wait_multi([object()], [good], [E], [0], waits)
    # the discs' calls say what they said
    with pytest.raises(ValueError, match="^expected one track table, one radii array and one start per engine$"):
        Engine.tree_clear_multi([object()], [np.zeros((2, 1, 2))], [0.5], [0, 0])
    with pytest.raises(ValueError, match="^expected one track table, one extents array and one start per engine$"):
        Engine.tree_clear_rects_multi([object()], [good], [E], [0, 0])


def _native_planner():
    car = lqrrt_amd.systems.Car(0)
    cons = lqrrt_amd.Constraints(car.nstates, car.ncontrols, car.goal_buffer, car.is_feasible)
    return lqrrt_amd.Planner(car.dynamics, car.lqr, cons, error_tol=car.error_tol, erf=car.erf, goal0=car.goal, printing=False, **car.plan_kwargs)


def _callback_planner():
    cons = lqrrt_amd.Constraints(2, 1, [0.1, 0.1], lambda x, u: True)
    p = lqrrt_amd.Planner(lambda x, u, dt: x + dt * np.array([x[1], u[0]]), lambda x, u: (np.eye(2), np.array([[1.0, 1.0]])), cons,
                          horizon=1, dt=0.1, goal0=[1.0, 0.0], printing=False)
    assert p.callback_mode
    return p


def test_avoids_rects_refuses_before_touching_a_planner():
    a, b = _native_planner(), _native_planner()
    good = np.zeros((3, 2, 3))
    for bad in (dict(tracks=np.zeros((0, 1, 3)), extents=E), dict(tracks=np.zeros((3, 2, 2)), extents=E), dict(tracks=[], extents=E),
                dict(tracks=good, extents=(1.0, -0.1)), dict(tracks=good, extents=[E, E, E]), dict(tracks=good, extents=0.5),
                dict(tracks=good, extents=(np.inf, 0.5)), dict(tracks=good, extents=E, start=-1), dict(tracks=good, extents=E, start=1.5),
                dict(tracks=np.full((3, 2, 3), np.nan), extents=E),
                dict(tracks=good, extents=E, max_wait=64), dict(tracks=good, extents=E, max_wait=-1), dict(tracks=good, extents=E, max_wait=1.0),
                dict(tracks=[good, good], extents=None),                          # tracks per planner, extents not
                dict(tracks=[good, good], extents=[E]),
                dict(tracks=[good, np.zeros((3, 0, 3))], extents=[E, E])):
        with pytest.raises(ValueError):
            lqrrt_amd.avoids_rects([a, b], **bad)
    with pytest.raises(ValueError, match="extents per planner"):
        lqrrt_amd.avoids_rects([a, b], [good, good], None)
    with pytest.raises(ValueError, match="twice"):
        lqrrt_amd.avoids_rects([a, a], good, E)
    with pytest.raises(ValueError, match="Planner"):
        lqrrt_amd.avoids_rects([a, "b"], good, E)
    with pytest.raises(NotImplementedError, match="Python"):
        lqrrt_amd.avoids_rects([a, _callback_planner()], good, E)
    with pytest.raises(TypeError):
        lqrrt_amd.avoids_rects([a, b], good, E, connect=8)                         # there is no rectangle connect
    assert all(p.tree is None and not p.plan_reached_goal and not hasattr(p, "node_seq") for p in (a, b))
    # planners without a tree on the device: None each, as avoid_rects; no device is needed for that
    assert lqrrt_amd.avoids_rects([a, b], good, E) == [None, None]
    assert lqrrt_amd.avoids_rects([a, b], [good, [np.zeros((4, 3))]], [[E, (0.5, 0.2)], (0.3, 0.3)], start=2, adopt=False, max_wait=7) == [None, None]
    assert lqrrt_amd.avoids_rects([], good, E) == []
    assert all(p.tree is None and not hasattr(p, "node_seq") and p.plan_wait == 0 for p in (a, b))
    doc = lqrrt_amd.avoids_rects.__doc__
    assert "avoid_rects" in doc and "ONE" in doc and "section 23" in doc and "connect" in doc
    assert "avoids_rects" in lqrrt_amd.Planner.avoid_rects.__doc__


# ------------------------------------------------------------------------------------------------ sources

def test_the_new_files_stay_plain_launches_on_the_existing_host_path():
    kern = open(os.path.join(CSRC, "clear_rects_multi.hpp")).read()
    host = open(os.path.join(CSRC, "engine_clear_rects_multi.hpp")).read()
    for name, text in (("clear_rects_multi.hpp", kern), ("engine_clear_rects_multi.hpp", host)):
        for word in FORBIDDEN:
            assert word not in text, (name, word)
        assert "dalloc(" not in text, name
    # the kernel fragment: two kernels round the solo files' bodies as they stand, no per-node body of its own
    assert "__device__" not in kern
    assert kern.count("__global__") == 2 and "k_clear_rects_check_multi" in kern and "k_clear_rects_wait_check_multi" in kern
    for reused in ("clear_rects_check_body<S>(", "clear_rects_wait_check_body<S>(", "multi_engine_of(", "has_discs<S>::value",
                   "__launch_bounds__(64)", "__launch_bounds__(CLEAR_WAIT_BLOCK)", "d.waits", "d.hit", "extern __shared__ double hull_lds[]"):
        assert reused in kern, reused
    code = re.sub(r"//[^\n]*", "", kern)
    assert "clear_rects_hit" not in code and "__syncthreads" not in code and "atomic" not in code
    # the host fragment: the traits, the solo calls' checker reused, the existing run; nothing allocated, copied or waited for here
    assert "struct ClearRectsMulti : ClearRects" in host and "struct ClearRectsWaitMulti : ClearRectsWait" in host
    assert "clear_rects_check<typename M::Solo>(" in host and "clear_multi_run<" in host
    assert "multi_engines_check(" in host and "engine_suffix(k)" in host
    assert "static int clear_rects_check(" not in host
    for work in ("hipMemcpy", "hipMalloc", "hipStreamSynchronize", "dalloc_transient("):
        assert work not in host, work
    assert host.count("hipLaunchKernelGGL(") == 4                                  # the two checks, and the two existing selects
    for words in ("k_clear_rects_check_multi<S>), dim3(grid), dim3(64), hull_bytes, st", "k_clear_select_multi, dim3(grid), dim3(CLEAR_BLOCK)",
                  "k_clear_rects_wait_check_multi<S>), dim3(grid), dim3(CLEAR_WAIT_BLOCK), hull_bytes, st",
                  "k_clear_wait_select_multi, dim3(grid), dim3(CLEAR_WAIT_BLOCK)", "CHECK_GROUPS = 1;", "CHECK_GROUPS = CLEAR_WAIT_WAVES;",
                  'NAME_MULTI = "lqrrt_tree_clear_rects_multi"', 'NAME_MULTI = "lqrrt_tree_clear_rects_wait_multi"',
                  "typedef ClearRects Solo;", "typedef ClearRectsWait Solo;", "P.p[18]"):
        assert words in host, words
    call = host[host.index("static int clear_rects_multi_call("):]
    assert call.index("TRY(clear_rects_multi_check<M>(") < call.index("TRY(use_device(engines[0]));") < call.index("clear_multi_run<M>(")
    check = host[host.index("static int clear_rects_multi_check("):host.index("static int clear_rects_multi_call(")]
    assert "hipLaunchKernelGGL" not in check and "hipLaunchKernelGGL" not in call
    # table sharing: the same pointers, equal L and D, and for the novice boats equal inflation
    for words in ("tracks[q] == tracks[k]", "extents[q] == extents[k]", "L[q] == L[k]", "D[q] == D[k]"):
        assert words in check, words
    # where the fragments stand
    kernels = open(os.path.join(CSRC, "kernels.hpp")).read()
    assert kernels.index('#include "clear_multi.hpp"') < kernels.index('#include "clear_rects_wait.hpp"') \
        < kernels.index('#include "clear_rects_multi.hpp"')
    engine = open(os.path.join(CSRC, "engine.hip")).read()
    assert max(engine.index('#include "engine_clear_multi.hpp"'), engine.index('#include "engine_clear_rects_wait.hpp"')) \
        < engine.index('#include "engine_clear_rects_multi.hpp"')
    life = open(os.path.join(CSRC, "engine_lifecycle.hpp")).read()
    assert "clear_rects_multi" not in life and "clear_rects_wait_multi" not in life  # nothing of it enters lqrrt_engine_footprint
    # the solo fragments and the discs' fleet fragments do not know of this one
    for name in ("clear_multi.hpp", "engine_clear_multi.hpp", "clear_rects.hpp", "clear_rects_wait.hpp", "engine_clear_rects.hpp",
                 "engine_clear_rects_wait.hpp", "engine_clear.hpp"):
        assert "rects_multi" not in open(os.path.join(CSRC, name)).read(), name
    # Python: one path for both fleets
    import inspect
    from lqrrt_amd import planner as planner_mod
    src = inspect.getsource(planner_mod.avoids_rects)
    assert "_avoids_query(" in src and "Engine.tree_clear_rects_multi, Engine.tree_clear_rects_wait_multi" in src and "_fleet_avoid_runs(" in src
    assert "_fleet_groups(" in inspect.getsource(planner_mod._avoids_query)


def test_check_kernels_stay_in_the_class_of_the_retain_check():
    """For every model with a circle path k_clear_rects_check_multi<S> and k_clear_rects_wait_check_multi<S> exist, and for no other
    model; no private segment, at least the occupancy of k_retain_check<S>, static LDS 0 / within the wait check's 64 bytes."""
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
    retain, plain, wait = by_model("k_retain_check"), by_model("k_clear_rects_check_multi"), by_model("k_clear_rects_wait_check_multi")
    solo, solo_wait = by_model("k_clear_rects_check"), by_model("k_clear_rects_wait_check")
    discs = ["BoatAdvanced", "BoatIntermediate", "BoatNovice", "BoatNoviceLqr", "Car", "RosBoat"]
    assert sorted(plain) == discs == sorted(wait)
    assert "UserSystem" in retain and "Pendulum" in retain
    for model in discs:
        for what, k, s in (("rects check multi", plain[model], solo[model]), ("rects wait check multi", wait[model], solo_wait[model])):
            print("%-18s retain check occ %d vgpr %3d   solo occ %d vgpr %3d sgpr %3d   %-22s %3d B occ %d vgpr %3d sgpr %3d lds %d" % (
                model, retain[model]["occupancy"], retain[model]["vgpr"], s["occupancy"], s["vgpr"], s.get("sgpr", -1), what, k["scratch"],
                k["occupancy"], k["vgpr"], k.get("sgpr", -1), k["lds"]))
            assert k["scratch"] == 0 == retain[model]["scratch"]
            assert k["occupancy"] >= retain[model]["occupancy"]
        assert plain[model]["lds"] == 0 and wait[model]["lds"] <= 64               # (static; the hull is dynamic)


# ------------------------------------------------------------------------------------------------ the GPU file's inputs

def test_the_chunk_edge_inputs_are_not_degenerate():
    """The fork under the starts (5 k) % 23: 23 distinct first arrays over k < 33, and starts[31] != starts[32]; with the waits
    1 + (3 k) % 9, 12 distinct pairs of masks.  A member that read another's descriptor would answer for that start or that W."""
    n = max(mi.CHUNK_SIZES)
    assert n == 33 and mi.CHUNK_SIZES == (1, 32, 33)
    starts, waits = mi.starts(n), mi.waits(n)
    assert starts[31] != starts[32] and waits[31] != waits[32] and len(set(starts[:23])) == 23 and set(waits) == {1, 4, 7}
    firsts = {tuple(mi.fork_reference(s)["first"].tolist()) for s in starts}
    assert len(firsts) == 23
    assert tuple(mi.fork_reference(starts[31])["first"].tolist()) != tuple(mi.fork_reference(starts[32])["first"].tolist())
    pairs = set()
    for s, w in zip(starts, waits):
        ref = mi.fork_wait_reference(s, w)
        pairs.add((tuple(ref["clear"].tolist()), tuple(ref["dwell_ok"].tolist())))
    assert len(pairs) == 12


def test_the_one_call_inputs_span_two_chunks_and_the_tree_sizes():
    plain = mi.by_model(mi.plain_cases(), lambda c: c.tree.system)
    assert len(mi.by_model(cr.cases(), lambda c: c.tree.system)["boat_advanced"]) == 21
    assert len(plain["boat_advanced"]) == 23 and {c.tree.size for c in plain["boat_advanced"]} == {1, 11, 256, 257}
    assert sorted(plain) == ["boat_advanced", "boat_intermediate", "boat_novice", "car", "ros_boat"]
    wait = mi.by_model(mi.wait_cases(), lambda c: c.case.tree.system)
    assert len(mi.by_model(rw.cases(), lambda c: c.case.tree.system)["boat_advanced"]) == 40
    assert len(wait["boat_advanced"]) == 41 > 32 and {c.W for c in wait["boat_advanced"]} >= {1, 2, 3, 5, 8, 63, 64}      # two chunks
    assert all(c.case.tree.size <= 257 for c in mi.wait_cases()) and all(c.tree.size <= 257 for c in mi.plain_cases())
    # the one-node tree: the square on the root is a conflict at tau = 0, far away it is none; the root is no hit
    on, far = mi.one_node_cases()
    assert on.tree is cl.case("N=1, a disc on the root").tree and on.tree.size == 1
    assert on.reference()["first"].tolist() == [0] and far.reference()["first"].tolist() == [-1]
    assert on.reference()["dwell_first"].tolist() == [-2] == far.reference()["dwell_first"].tolist()
    assert on.reference()["stats"]["conflicts"] == 1 and far.reference()["stats"]["conflicts"] == 0


def test_the_hull_and_sharing_inputs_are_not_degenerate():
    big = cr.case("ros_boat on an occupied grid, 3073 hull points, D = 65")
    small = cr.case("ros_boat: the fork")
    assert big.vps().shape[1] == 3073 and small.vps().shape[1] < 64 and big.tree.system == small.tree.system == "ros_boat"
    assert big.reference()["stats"]["conflicts"] > 0 and small.reference()["stats"]["conflicts"] > 0
    # table sharing: the changed row and the start change the answer
    s = mi.SHARE_STARTS
    assert s == (0, 4, 0, 1, 0)
    assert mi.fork_reference(0)["stats"] != mi.moved_reference(0)["stats"]
    assert not np.array_equal(mi.fork_reference(0)["first"], mi.fork_reference(4)["first"])
    assert not np.array_equal(mi.fork_reference(0)["first"], mi.fork_reference(1)["first"])
    a, b = mi.fork_wait_reference(0, 8), mi.fork_wait_reference(0, 8, moved=True)
    assert not np.array_equal(a["clear"], b["clear"])
    assert not np.array_equal(a["clear"], mi.fork_wait_reference(4, 8)["clear"])
    # the novice boats: the inflation changes the answer, so two members that differ in it must not share a table
    c = cr.case("boat_novice: the fork")
    t = c.tree
    lo, hi = t.box()
    import feasibility_reference as fr
    wide = cr.clear_rects(t.state, t.pID, t.elen, t.xedge, cr.row_test("novice", half_length=fr.HALF_LENGTH), c.tracks, c.extents, 0, lo, hi)
    slim = cr.clear_rects(t.state, t.pID, t.elen, t.xedge, cr.row_test("novice", half_length=fr.HALF_LENGTH / 4), c.tracks, c.extents, 0, lo, hi)
    assert wide["stats"] == c.reference()["stats"] and not np.array_equal(wide["first"], slim["first"])
