"""
Clear goal chains for several trees per launch (lqrrt_tree_clear_connect_multi, Engine.tree_clear_connect_multi,
lqrrt_amd.avoids(connect), deconflict(connect); csrc/clear_connect_multi.hpp) on the CPU: the ABI's declaration and the binding, the
refusals of the public calls before any planner or engine is touched, and what the sources and the compiler say about the new
kernels.  The device call is compared with the one-tree call, member by member, in tests/test_clear_connect_multi_gpu.py.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lqrrt_amd", "csrc")


# ------------------------------------------------------------------------------------------------ header and binding

def test_header_declares_the_call_and_the_binding_has_it():
    text = open(os.path.join(ROOT, "include", "lqrrt_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    multi = re.search(r"\bint lqrrt_tree_clear_connect_multi\s*\((.*?)\);", code, re.S)
    assert multi
    args = [a.strip() for a in multi.group(1).split(",")]
    assert len(args) == 16 and args[0] == "lqrrt_engine** engines" and args[1] == "int n" and args[-1] == "void* stream"
    assert multi.group(1).count("const double* const*") == 2 and "const int32_t* const* nodes_host" in multi.group(1)
    for name in ("const int32_t* horizon_iters", "const int32_t* goal_tries", "const int32_t* counts", "lqrrt_clear_stats* out",
                 "lqrrt_clear_connect_stats* chain", "int32_t* const* first_host", "int32_t* const* dwell_host"):
        assert name in args, name
    I, P = C.c_int, C.c_void_p
    assert nat.SIGNATURES["lqrrt_tree_clear_connect_multi"] == (I, [P, I] + [P] * 14)
    assert hasattr(nat.lib(), "lqrrt_tree_clear_connect_multi") and nat.lib().lqrrt_abi_version() == 1
    assert isinstance(Engine.__dict__["tree_clear_connect_multi"], staticmethod)
    # the older signatures are what they were
    solo = re.search(r"\bint lqrrt_tree_clear_connect\s*\((.*?)\);", code, re.S)
    plain = re.search(r"\bint lqrrt_tree_clear_multi\s*\((.*?)\);", code, re.S)
    wait = re.search(r"\bint lqrrt_tree_clear_wait_multi\s*\((.*?)\);", code, re.S)
    assert len(solo.group(1).split(",")) == 15 and len(plain.group(1).split(",")) == 11 and len(wait.group(1).split(",")) == 12
    assert nat.SIGNATURES["lqrrt_tree_clear_multi"] == (I, [P, I] + [P] * 9)
    assert nat.SIGNATURES["lqrrt_tree_clear_wait_multi"] == (I, [P, I] + [P] * 10)
    assert nat.SIGNATURES["lqrrt_tree_clear_connect"] == (I, [P, P, P, I, I, I, I, I, P, I, C.POINTER(nat.ClearStats),
                                                              C.POINTER(nat.ClearConnectStats), P, P, P])
    assert nat.SIGNATURES["lqrrt_connect_commit_multi"] == (I, [P, I] + [P] * 7)
    assert lqrrt.avoids is lqrrt_amd.avoids and lqrrt.deconflict is lqrrt_amd.deconflict


# ------------------------------------------------------------------------------------------------ host-only refusals

def _native_planner():
    car = lqrrt_amd.systems.Car(0)
    cons = lqrrt_amd.Constraints(car.nstates, car.ncontrols, car.goal_buffer, car.is_feasible)
    return lqrrt_amd.Planner(car.dynamics, car.lqr, cons, error_tol=car.error_tol, erf=car.erf, goal0=car.goal, printing=False,
                             **dict(car.plan_kwargs))


def _callback_planner():
    cons = lqrrt_amd.Constraints(2, 1, [0.1, 0.1], lambda x, u: True)
    p = lqrrt_amd.Planner(lambda x, u, dt: x + dt * np.array([x[1], u[0]]), lambda x, u: (np.eye(2), np.array([[1.0, 1.0]])), cons,
                          horizon=1, dt=0.1, goal0=[1.0, 0.0], printing=False)
    assert p.callback_mode
    return p


def _untouched(*planners):
    return all(p.tree is None and not p.plan_reached_goal and not hasattr(p, "node_seq") for p in planners)


def test_avoids_connect_refuses_before_touching_a_planner():
    a, b = _native_planner(), _native_planner()
    good = np.zeros((3, 2, 2))
    with pytest.raises(ValueError, match="max_wait"):
        lqrrt_amd.avoids([a, b], good, 0.5, connect=8, max_wait=2)
    for bad in (-1, 1.0, True):
        with pytest.raises(ValueError, match="connect"):
            lqrrt_amd.avoids([a, b], good, 0.5, connect=bad)
    with pytest.raises(ValueError, match="twice"):
        lqrrt_amd.avoids([a, a], good, 0.5, connect=8)
    with pytest.raises(NotImplementedError, match="Python"):
        lqrrt_amd.avoids([a, _callback_planner()], good, 0.5, connect=8)
    assert _untouched(a, b)
    # planners without a tree on the device: None each, as avoid(connect); no device is needed for that
    assert lqrrt_amd.avoids([a, b], good, 0.5, connect=8) == [None, None] and a.avoid(good, 0.5, connect=8) is None
    assert lqrrt_amd.avoids([], good, 0.5, connect=8) == []
    assert _untouched(a, b)


def test_deconflict_connect_refuses_before_touching_a_planner():
    a, b = _native_planner(), _native_planner()
    with pytest.raises(ValueError, match="batched"):
        lqrrt_amd.deconflict([a, b], 0.5, batched=True, connect=8)
    with pytest.raises(ValueError, match="max_wait"):
        lqrrt_amd.deconflict([a, b], 0.5, connect=8, max_wait=3)
    with pytest.raises(ValueError, match="connect"):
        lqrrt_amd.deconflict([a, b], 0.5, connect=-1)
    with pytest.raises(ValueError, match="twice"):
        lqrrt_amd.deconflict([a, a], 0.5, connect=8)
    with pytest.raises(NotImplementedError, match="Python"):
        lqrrt_amd.deconflict([_callback_planner()], 0.5, connect=8)
    assert all(p.tree is None and not hasattr(p, "node_seq") for p in (a, b))
    doc = lqrrt_amd.deconflict.__doc__
    assert "connect" in doc and "Not covered" in doc and "until it is committed" in doc
    assert "connect" in lqrrt_amd.avoids.__doc__ and "tree_clear_connect_multi" in lqrrt_amd.avoids.__doc__
    assert "avoids(connect" in lqrrt_amd.Planner.avoid.__doc__


def test_engine_method_refuses_on_the_host():
    t, o = np.zeros((2, 1, 2)), object()
    with pytest.raises(ValueError, match="no engines"):
        Engine.tree_clear_connect_multi([], [], [], [], [])
    with pytest.raises(ValueError, match="per engine"):
        Engine.tree_clear_connect_multi([o], [t], [0.5], [0, 0], [4])
    with pytest.raises(ValueError, match="start"):
        Engine.tree_clear_connect_multi([o], [t], [0.5], [-1], [4])
    with pytest.raises(ValueError, match="horizon"):
        Engine.tree_clear_connect_multi([o, o], [t, t], [0.5, 0.5], [0, 0], [4])
    with pytest.raises(ValueError, match="goal_tries"):
        Engine.tree_clear_connect_multi([o, o], [t, t], [0.5, 0.5], [0, 0], [4, 4], tries=[8, 8, 8])
    with pytest.raises(ValueError, match="id list"):
        Engine.tree_clear_connect_multi([o, o], [t, t], [0.5, 0.5], [0, 0], [4, 4], nodes=[None])
    with pytest.raises(ValueError, match="id list"):
        Engine.tree_clear_connect_multi([o, o], [t, t], [0.5, 0.5], [0, 0], [4, 4], tries=[8, 1], nodes=[[0], None, None])


# ------------------------------------------------------------------------------------------------ sources

def test_the_new_fragments_reuse_the_body_and_the_host_path():
    kern = open(os.path.join(CSRC, "clear_connect_multi.hpp")).read()
    host = open(os.path.join(CSRC, "engine_clear_connect_multi.hpp")).read()
    shared = open(os.path.join(CSRC, "engine_clear_multi.hpp")).read()
    for name, text in (("clear_connect_multi.hpp", kern), ("engine_clear_connect_multi.hpp", host)):
        for word in FORBIDDEN:
            assert word not in text, (name, word)
    # the kernels: the solo file's body, called as it stands; no second copy of its pieces, no atomic of their own
    assert kern.count("clear_connect_search_body<S>(") == 1 and "__device__" not in kern
    for copy in ("refine_edge<S>(", "S::feasible(", "atomicMin(", "atomicAdd(", "refine_start<S>(", "stage_geo("):
        assert copy not in kern, copy
    assert kern.count("__launch_bounds__(64)") == 1 and "has_discs<S>::value" in kern
    search = kern[kern.index("void k_clear_connect_search_multi("):]
    assert "multi_engine_of(gr.block0, gr.n, (int)blockIdx.x)" in search and search.count("launch_constant(") == 2
    assert "(int)blockIdx.x - gr.block0[e]" in search and "p.P, p.g, p.r, p.tv, d.a, d.c, d.out" in search
    seed = kern[kern.index("void k_clear_connect_multi_seed("):kern.index("// Grid = the members'")]
    assert "atomic" not in seed and "tv.elen[0]" in seed and "d.out->key = incumbent << 32;" in seed and "launch_constant" not in seed
    # the host: ONE path, engine_clear_multi.hpp's -- the new fragment allocates nothing, waits for nothing and copies no checker
    for work in ("dalloc", "hipMalloc", "hipStreamSynchronize(", "hipDeviceSynchronize", "StreamDrain", "multi_chunks(", "static int clear_check(",
                 "static int connect_check("):
        assert work not in host, work
    call = host[host.index('extern "C" int lqrrt_tree_clear_connect_multi('):]
    order = [call.index(w) for w in ("clear_multi_check<M>(", "connect_check(", "multi_id_list(", "connect_candidates_check(", "connect_depths(",
                                     "> e->lds_limit", "engine_suffix(k)", "use_device(", "clear_multi_run<M>(", "chain_from")]
    assert order == sorted(order)
    for work in ("hipMemcpyAsync(", "hipLaunchKernelGGL("):
        assert work not in call, work
    assert call.index("fail(") < call.index("use_device(") and "fail(" not in call[call.index("use_device("):]
    extra = host[host.index("struct ClearConnectExtra"):host.index('extern "C" int lqrrt_tree_clear_connect_multi(')]
    assert "fail(" not in extra                                                    # what runs behind the allocation refuses nothing
    order = [extra.index(w) for w in ("k_clear_connect_multi_seed", "retain_grid(", "if (grid > 0)", "search<S>(", "hipMemcpyDeviceToHost")]
    assert order == sorted(order)
    assert "clear_connect_lds_bytes(engines[k], horizons[k])" in extra and "std::max(lds," in extra
    # ... and the shared run: transient memory only, one allocation per chunk, one synchronise, the hook behind the select
    run = shared[shared.index("static int clear_multi_run("):shared.index("static int clear_multi_call(")]
    assert run.count("hipStreamSynchronize(") == 1 and run.count("dalloc_transient(") == 1 and "dalloc(" not in shared
    assert "fail(" not in run[run.index("dalloc_transient("):]
    order = [run.index(w) for w in ("extra.groups(k)", "multi_chunks(groups)", "StreamDrain drain(st);", "extra.carve(", "dalloc_transient(",
                                    "extra.fill(", "hipMemcpyAsync(dm, c.img.data(), image", "M::select_multi(", "extra.enqueue(",
                                    "hipStreamSynchronize(st)", "drain.disarm();")]
    assert order == sorted(order)
    assert "std::max((long long)engines[k]->N * M::CHECK_GROUPS, extra.groups(k))" in run     # chunked on max(N, count)
    # where the fragments stand
    kernels = open(os.path.join(CSRC, "kernels.hpp")).read()
    assert kernels.index('#include "clear_connect.hpp"') < kernels.index('#include "clear_connect_multi.hpp"')
    engine = open(os.path.join(CSRC, "engine.hip")).read()
    assert max(engine.index('#include "engine_clear_connect.hpp"'), engine.index('#include "engine_clear_multi.hpp"')) \
        < engine.index('#include "engine_clear_connect_multi.hpp"')
    # the solo files know nothing of all this
    for name in ("clear_connect.hpp", "engine_clear_connect.hpp"):
        assert "ClearConnectDesc" not in open(os.path.join(CSRC, name)).read()


def test_avoids_connect_shares_the_planners_parts():
    src = open(os.path.join(ROOT, "lqrrt_amd", "planner.py")).read()
    solo = src[src.index("    def _avoid_connect(self"):src.index("    def _avoid_connect_end(self")]
    assert solo.count("tree_clear_connect(") == 1 and "_avoid_connect_end(" in solo and "_avoid_end(" not in solo
    fleet = src[src.index("def _avoids_connect("):src.index("def _deconflict_batched(")]
    assert fleet.count("tree_clear_connect_multi(") == 1 and fleet.count("connect_commit_multi(") == 1 and "_fleet_commit(" in fleet
    assert "_fleet_groups(" in fleet and "_avoid_connect_end(" in fleet and "tree_clear_connect(" not in fleet and "raise failed" in fleet
    end = src[src.index("    def _avoid_connect_end(self"):src.index("    def _avoid_plan_holds(self")]
    for name in ("_avoid_end(", "_connect_accept(", "plan_wait = 0", "chain_committed"):
        assert name in end, name


# ------------------------------------------------------------------------------------------------ the compiler's figures

def test_search_multi_stays_in_the_class_of_the_solo_search():
    """k_clear_connect_search_multi<S> exists for the six models with a circle path and no other; per model its occupancy is no
    lower and its private segment no larger than k_clear_connect_search<S>'s, compiled in the same build; the seed kernel has no
    private segment.  (If the occupancy drops: launch_constant is the first place to look.)"""
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
    solo, multi, connect = by_model("k_clear_connect_search"), by_model("k_clear_connect_search_multi"), by_model("k_connect_search_multi")
    discs = ["BoatAdvanced", "BoatIntermediate", "BoatNovice", "BoatNoviceLqr", "Car", "RosBoat"]
    assert sorted(multi) == discs == sorted(solo)
    assert "UserSystem" in connect and "Pendulum" in connect
    for model in discs:
        s, m = solo[model], multi[model]
        print("%-18s solo %4d B occ %d vgpr %3d sgpr %3d lds %d   multi %4d B occ %d vgpr %3d sgpr %3d lds %d" % (
            model, s["scratch"], s["occupancy"], s["vgpr"], s.get("sgpr", -1), s["lds"], m["scratch"], m["occupancy"], m["vgpr"],
            m.get("sgpr", -1), m["lds"]))
    worse = {m: (multi[m]["occupancy"], solo[m]["occupancy"], multi[m]["scratch"], solo[m]["scratch"]) for m in discs
             if multi[m]["occupancy"] < solo[m]["occupancy"] or multi[m]["scratch"] > solo[m]["scratch"]}
    assert not worse, worse
    seed = [r for r in rows if "k_clear_connect_multi_seed" in r["name"]]
    assert len(seed) == 1 and seed[0]["scratch"] == 0
