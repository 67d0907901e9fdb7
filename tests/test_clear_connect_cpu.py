"""
Clear goal chains (Engine.tree_clear_connect / Planner.avoid(connect)) on the CPU: the reference of the rule
(tests/clear_connect_reference.py, composed from clear_reference and connect_reference) on the committed fixture trees -- no case is
degenerate, and every answer is pinned --, the ABI, the host side of the public method, and what the compiler says about the search
kernel.  The device call is compared with the same reference, case by case, in tests/test_clear_connect_gpu.py.
"""
import ctypes as C
import os
import re
import shutil
import sys

import numpy as np
import pytest

import lqrrt_amd
from lqrrt_amd import _native as nat
from lqrrt_amd.engine import Engine
import clear_connect_reference as ccr
from clear_common import FORBIDDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (chain_from, chain_cost, clear_candidates, chain_arrival) of the reference, computed here on the CPU
PINS = {
    "far discs": (211, 951, 217, 951),
    "first row of the first chain edge": (-1, -1, 1, -1),
    "first row of the first chain edge, every node": (-1, -1, 212, -1),
    "first row of the first chain edge, start = 7": (-1, -1, 1, -1),
    "last row of the last edge": (213, 1051, 217, 1051),
    "second edge of the chain": (-1, -1, 1, -1),
    "second edge of the chain, the disc one edge early": (211, 951, 1, 951),
    "dwell conflict at exactly L - 1": (-1, -1, 1, -1),
    "the same track, L - 1 rows": (211, 951, 1, 951),
    "arrival after L - 1, far discs": (211, 951, 1, 951),
    "arrival after L - 1, the last table row on a late chain row": (-1, -1, 1, -1),
    "arrival exactly at L - 1": (-1, -1, 1, -1),
    "start >= L": (-1, -1, 1, -1),
    "candidate below a conflict": (-1, -1, 209, -1),
    "candidate below a conflict, listed alone": (-1, -1, 0, -1),
    "disc on the root's row": (-1, -1, 0, -1),
    "disc on the root's row one instant late": (-1, -1, 1, -1),
    "a chain strictly shorter than the best clear hit": (211, 951, 218, 951),
    "a chain that only ties with the best clear hit": (-1, -1, 1, -1),
    "tie: the smaller id wins": (331, 1551, 2, 1551),
    "last row, D = 64, the deciding disc last": (213, 1051, 217, 1051),
    "last row, D = 65, the deciding disc last": (213, 1051, 217, 1051),
    "last row, D = 65, the deciding disc first": (213, 1051, 217, 1051),
    "L = 1, far": (211, 951, 217, 951),
    "L = 1, a disc on a chain row": (-1, -1, 1, -1),
    "boat_advanced: every goal hit crossed": (-1, -1, 493, -1),
    "boat_advanced: the best hit caught while it waits": (-1, -1, 600, -1),
}


def test_every_case_is_pinned():
    assert sorted(c.name for c in ccr.cases()) == sorted(PINS)


@pytest.mark.parametrize("name", sorted(PINS))
def test_reference_answers_and_no_case_is_degenerate(name):
    c = ccr.case(name)
    ref = c.reference()
    ch = ref["chain"]
    kinds = {}
    for w in ref["verdicts"].values():
        kinds[w[0]] = kinds.get(w[0], 0) + 1
    print("%-70s %s incumbent %d %s" % (name, [ch[k] for k in ccr.CHAIN_KEYS], ref["incumbent"], kinds))
    assert c.lacks() == []
    assert (ch["chain_from"], ch["chain_cost"], ch["clear_candidates"], ch["chain_arrival"]) == PINS[name]
    if ch["chain_from"] >= 0:
        v = ch["chain_from"]
        assert ch["chain_cost"] < ref["incumbent"] and ref["first"][v] == -1 and ref["verdicts"][v][0] == "clear"
        assert ch["chain_arrival"] == ref["cum"][v] + ch["chain_rows"] and ch["chain_rows"] >= 1
        assert ch["chain_cost"] == ch["chain_arrival"] - c.tree.elen[0] + 1


def test_what_the_cases_are_there_to_show():
    free = ccr.case("far discs").reference()
    v = free["chain"]["chain_from"]
    assert (free["chain"]["chain_cost"], v) == (951, 211) and free["incumbent"] == ccr.NO_INCUMBENT      # connect_reference's winner
    # the first row: tau = start + cum[v]; on this prefix the other chains hang below v's children, which share that row
    t0 = int(free["cum"][v])
    assert ccr.case("first row of the first chain edge").reference()["verdicts"][v] == ("route", t0)
    assert ccr.case("first row of the first chain edge, every node").reference()["verdicts"][v] == ("route", t0)
    assert ccr.case("first row of the first chain edge, start = 7").reference()["verdicts"][v] == ("route", t0 + 7)
    # the last row: the winner moves to another candidate, whatever the number of discs and wherever the deciding one stands
    rows = free["chain"]["chain_rows"]
    for name in ("last row of the last edge", "last row, D = 64, the deciding disc last", "last row, D = 65, the deciding disc last",
                 "last row, D = 65, the deciding disc first"):
        ref = ccr.case(name).reference()
        assert ref["chain"]["chain_from"] not in (-1, v) and ref["verdicts"][v] == ("route", t0 + rows - 1), name
        assert ref["chain"]["chain_cost"] > 951 and ref["stats"]["conflicts"] == 0
    # the second edge: the conflict's time includes the first edge's rows; one edge earlier the same disc decides nothing
    rows_v, lens, _ = ccr.chain_times(ccr.case("far discs").tree, v, 0)
    second = ccr.case("second edge of the chain").reference()["verdicts"][v]
    assert second[0] == "route" and t0 + lens[0] <= second[1] < t0 + lens[0] + lens[1]
    assert ccr.case("second edge of the chain, the disc one edge early").reference()["chain"]["chain_from"] == v
    # the dwell: L - 1 exactly, and one row less is clear
    c = ccr.case("dwell conflict at exactly L - 1")
    assert c.reference()["verdicts"][v] == ("dwell", c.tracks.shape[0] - 1)
    assert ccr.case("the same track, L - 1 rows").reference()["chain"]["chain_from"] == v
    # arrival at or after L - 1: the conflicts are on clamped rows, the dwell range is empty
    for name, beyond in (("arrival after L - 1, the last table row on a late chain row", 0), ("start >= L", 1), ("L = 1, a disc on a chain row", 1)):
        c = ccr.case(name)
        w = c.reference()["verdicts"][v]
        assert w[0] == "route" and w[1] >= c.tracks.shape[0] - 1 + beyond, name      # (beyond the table: the row is clamped)
        assert t0 + rows - 1 > c.tracks.shape[0] - 1                                # the chain arrives after the table's last row
    c = ccr.case("arrival exactly at L - 1")
    assert c.reference()["verdicts"][v] == ("route", c.tracks.shape[0] - 1)
    # below a conflict: v's own edge is clear and so is its chain, but v is no candidate
    ref = ccr.case("candidate below a conflict").reference()
    assert ref["own_first"][v] == -1 and ref["first"][v] >= 0 and v not in ref["verdicts"] and ref["judge"](v)[0] == "clear"
    assert 0 < ref["chain"]["clear_candidates"] < free["chain"]["clear_candidates"]
    assert ccr.case("candidate below a conflict, listed alone").reference()["chain"]["clear_candidates"] == 0
    # the root
    ref = ccr.case("disc on the root's row").reference()
    assert ref["chain"]["clear_candidates"] == 0 and ref["own_first"][0] == 0 and np.all(ref["first"] == 0)
    late = ccr.case("disc on the root's row one instant late").reference()
    assert late["own_first"][0] == -1 and late["chain"]["clear_candidates"] >= 1
    # another system: the boat's chain is rejected while it waits next to the hit it left from
    c = ccr.case("boat_advanced: the best hit caught while it waits")
    ref = c.reference()
    b = ccr.plain(c.tree)["stats"]["best_end"]
    assert ref["verdicts"][b][0] == "dwell" and ref["dwell_first"][b] >= 0 and ref["first"][b] == -1 and ref["stats"]["best_end"] != b
    # the best clear hit as incumbent: strictly
    ref = ccr.case("a chain strictly shorter than the best clear hit").reference()
    assert ref["stats"]["clear_hits"] >= 1 and ref["chain"]["chain_cost"] < ref["incumbent"] < ccr.NO_INCUMBENT
    c = ccr.case("a chain that only ties with the best clear hit")
    ref = c.reference()
    assert all(ref["verdicts"][u] == ("clear", ref["incumbent"], ref["verdicts"][u][2]) for u in c.nodes) and ref["chain"]["chain_from"] == -1
    # the tie
    c = ccr.case("tie: the smaller id wins")
    ref = c.reference()
    a, b = c.nodes
    assert a > b and ref["verdicts"][a][:2] == ref["verdicts"][b][:2] and ref["chain"]["chain_from"] == b


def test_reference_does_not_depend_on_the_order_of_the_list():
    c = ccr.case("last row of the last edge")
    ids = np.random.RandomState(3).permutation(c.tree.size).tolist()
    a = ccr.clear_connect(c.tree, c.tracks, c.radii, c.start, nodes=ids)["chain"]
    b = ccr.clear_connect(c.tree, c.tracks, c.radii, c.start, nodes=sorted(ids))["chain"]
    assert a == b == c.reference()["chain"]
    assert ccr.clear_connect(c.tree, c.tracks, c.radii, c.start, nodes=[])["chain"]["chain_from"] == -1


# ------------------------------------------------------------------------------------------------ ABI and sources

def test_header_declares_the_call():
    text = open(os.path.join(ROOT, "include", "lqrrt_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint lqrrt_tree_clear_connect\s*\((.*?)\);", code, re.S)
    assert m and len(m.group(1).split(",")) == 15 and "lqrrt_clear_connect_stats* chain" in m.group(1)
    assert re.search(r"typedef struct \{[^}]*\} lqrrt_clear_connect_stats;", code, re.S)
    I, P = C.c_int, C.c_void_p
    assert nat.SIGNATURES["lqrrt_tree_clear_connect"] == (I, [P, P, P, I, I, I, I, I, P, I, C.POINTER(nat.ClearStats),
                                                              C.POINTER(nat.ClearConnectStats), P, P, P])
    assert hasattr(nat.lib(), "lqrrt_tree_clear_connect") and nat.lib().lqrrt_abi_version() == 1
    assert C.sizeof(nat.ClearConnectStats) == 4 * 4 + 2 * 8
    assert sorted(nat.ClearConnectStats().as_dict()) == sorted(ccr.CHAIN_KEYS)
    assert callable(Engine.tree_clear_connect)
    for word in ("incumbent", "candidate", "chain", "time", "winner", "strictly"):
        assert word in text[text.index("lqrrt_tree_clear and lqrrt_connect_search in one call"):text.index("} lqrrt_clear_connect_stats;")], word


def test_the_older_signatures_are_what_they_were():
    I, I64, P = C.c_int, C.c_int64, C.c_void_p
    assert nat.SIGNATURES["lqrrt_tree_clear"] == (I, [P, P, P, I, I, I, C.POINTER(nat.ClearStats), P, P, P])
    assert nat.SIGNATURES["lqrrt_connect_search"] == (I, [P, P, I, I, I, I64, C.POINTER(I64), C.POINTER(C.c_int32), P])
    assert nat.SIGNATURES["lqrrt_connect_commit"] == (I, [P, I, I, I, P, I, P])
    assert C.sizeof(nat.ClearStats) == 6 * 4 + 8


def _native_planner():
    car = lqrrt_amd.systems.Car(0)
    cons = lqrrt_amd.Constraints(car.nstates, car.ncontrols, car.goal_buffer, car.is_feasible)
    return lqrrt_amd.Planner(car.dynamics, car.lqr, cons, error_tol=car.error_tol, erf=car.erf, goal0=car.goal, printing=False,
                             **car.plan_kwargs)


def test_avoid_refusals_that_need_no_device():
    p = _native_planner()
    tracks = np.zeros((3, 1, 2))
    with pytest.raises(ValueError, match="not covered"):
        p.avoid(tracks, 0.5, max_wait=2, connect=8)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="connect"):
            p.avoid(tracks, 0.5, connect=bad)
    assert p.avoid(tracks, 0.5, connect=8) is None and p.avoid(tracks, 0.5, connect=0) is None      # no plan: nothing happens
    assert p.tree is None and not p.plan_reached_goal
    cons = lqrrt_amd.Constraints(2, 1, [0.1, 0.1], lambda x, u: True)
    cb = lqrrt_amd.Planner(lambda x, u, dt: x + dt * np.array([x[1], u[0]]), lambda x, u: (np.eye(2), np.array([[1.0, 1.0]])), cons,
                           horizon=1, dt=0.1, goal0=[1.0, 0.0], printing=False)
    with pytest.raises(NotImplementedError, match="Python"):
        cb.avoid(tracks, 0.5, connect=8)
    doc = lqrrt_amd.Planner.avoid.__doc__
    assert "MODIFIES THE TREE" in doc and "chain_committed" in doc


def test_avoid_connect_goes_through_the_connections_steps():
    src = open(os.path.join(ROOT, "lqrrt_amd", "planner.py")).read()
    body = src[src.index("    def _avoid_connect(self"):src.index("    def _avoid_plan_holds(self")]
    for name in ("tree_clear_connect(", "_commit_winner(", "connect_commit(", "_connect_accept(", "_avoid_end(", "plan_wait = 0"):
        assert name in body, name
    assert body.count("tree_clear_connect(") == 1 and "connect_search(" not in body and "tree_clear(" not in body      # ONE native query


def test_search_is_built_from_the_existing_pieces():
    """Plain launches on one stream; the chain's pieces are the refinement's and the clearance check's, not copies; the two sets of
    geometry stay apart; every refusal stands before anything is allocated or enqueued."""
    csrc = os.path.join(ROOT, "lqrrt_amd", "csrc")
    src = open(os.path.join(csrc, "clear_connect.hpp")).read()
    host = open(os.path.join(csrc, "engine_clear_connect.hpp")).read()
    for text in (src, host):
        for word in FORBIDDEN:
            assert word not in text, word
    for name in ("refine_start<S>(", "refine_edge<S>(", "refine_in_goal<S>(", "refine_best(", "stage_geo(", "GainLds<S>", "connect_key(",
                 "clear_stage_hull(", "clear_disc_world(", "clear_load_row<S>(", "S::feasible(", "has_discs<S>::value"):
        assert name in src, name
    assert src.count("__launch_bounds__(64)") == 1 and "S::step(" not in src and "trig_of<S>(" in src
    body = src[src.index("void clear_connect_search_body("):src.index("// Grid = one workgroup")]
    order = [body.index(w) for w in ("c.first[v] >= 0", "connect_key(cost, v) > refine_best(", "stage_geo(", "refine_edge<S>(",
                                     "if (key > refine_best(", "S::feasible(", "refine_in_goal<S>(", "atomicMin(")]
    assert order == sorted(order)
    assert "refine_edge<S>(P, g, gl, r," in body and body.count("S::feasible(P.p, gd, gld,") == 2 and "gl.oc" not in body
    seed = src[src.index("void k_clear_connect_seed("):src.index("// Candidate `cand`")]
    assert "atomic" not in seed and "tv.elen[0]" in seed and "out->key = incumbent << 32;" in seed
    # the host: checks, then one allocation, every launch back to back, one wait
    call = host[host.index('extern "C" int lqrrt_tree_clear_connect('):]
    run = host[host.index("static int clear_connect_run("):host.index('extern "C" int lqrrt_tree_clear_connect(')]
    order = [call.index(w) for w in ("clear_check<ClearPlain>(", "connect_check(", "connect_candidates_check(", "connect_depths(",
                                     "> e->lds_limit", "use_device(", "clear_connect_run(")]
    assert order == sorted(order)
    for work in ("dalloc", "hipMemcpyAsync(", "hipLaunchKernelGGL("):
        assert work not in call, work
    assert "fail(" not in run and run.count("dalloc_transient(") == 1 and "dalloc(" not in run
    assert run.count("hipStreamSynchronize(") == 1 and "hipDeviceSynchronize" not in host
    order = [run.index(w) for w in ("dalloc_transient(", "drain.arm();", "hipMemcpyAsync(", "retain_links(e, 0, N, nullptr", "C::template check<S>(",
                                    "k_clear_init<ClearLink>", "double_rounds(k_clear_double<ClearLink>", "C::select(", "k_clear_connect_seed",
                                    "clear_connect_search<S>(", "hipMemcpyDeviceToHost", "hipStreamSynchronize(", "drain.disarm();")]
    assert order == sorted(order)
    assert "refine_lds_bytes(e, horizon) + sizeof(double) * (size_t)2 * e->geo.V" in host
    kernels = open(os.path.join(csrc, "kernels.hpp")).read()
    assert max(kernels.index('#include "connect.hpp"'), kernels.index('#include "clear_multi.hpp"')) < kernels.index('#include "clear_connect.hpp"')
    engine = open(os.path.join(csrc, "engine.hip")).read()
    assert max(engine.index('#include "engine_connect.hpp"'), engine.index('#include "engine_clear_multi.hpp"')) \
        < engine.index('#include "engine_clear_connect.hpp"')


def test_search_kernel_stays_in_the_class_of_its_siblings():
    """k_clear_connect_search<S> exists for the six models with a circle path and no other; its occupancy is no lower than
    k_connect_search<S>'s and its private segment no larger than k_refine_search<S>'s, the larger sibling whose pieces it reuses."""
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
    refine, connect, mine = by_model("k_refine_search"), by_model("k_connect_search"), by_model("k_clear_connect_search")
    assert sorted(mine) == ["BoatAdvanced", "BoatIntermediate", "BoatNovice", "BoatNoviceLqr", "Car", "RosBoat"]
    assert "UserSystem" in connect and "Pendulum" in connect
    for model in sorted(mine):
        print("%-18s refine %4d B occ %d vgpr %3d   connect %4d B occ %d vgpr %3d   clear connect %4d B occ %d vgpr %3d sgpr %3d" % (
            model, refine[model]["scratch"], refine[model]["occupancy"], refine[model]["vgpr"], connect[model]["scratch"],
            connect[model]["occupancy"], connect[model]["vgpr"], mine[model]["scratch"], mine[model]["occupancy"], mine[model]["vgpr"],
            mine[model].get("sgpr", -1)))
    worse = {m: (mine[m]["occupancy"], connect[m]["occupancy"], mine[m]["scratch"], refine[m]["scratch"]) for m in mine
             if mine[m]["occupancy"] < connect[m]["occupancy"] or mine[m]["scratch"] > refine[m]["scratch"]}
    assert not worse, worse
    seed = [r for r in rows if "k_clear_connect_seed" in r["name"]]
    assert len(seed) == 1 and seed[0]["scratch"] == 0
