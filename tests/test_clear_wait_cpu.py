"""
The clearance query with departure delays (Planner.avoid(max_wait) / Engine.tree_clear_wait, csrc/clear_wait.hpp) on the CPU: the
reference of the rule (tests/clear_wait_reference.py) against the answers worked out by hand and against clear_reference at W = 1,
every input of tests/test_clear_wait_gpu.py shown not to be degenerate with the reference alone, the host side of the public calls
and their refusals, the ABI's declaration, and what the sources and the compiler say about the kernels.
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
import clear_reference as cl
from clear_common import FORBIDDEN, clear_host_text
import clear_wait_reference as cw
import feasibility_reference as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lqrrt_amd", "csrc")


def _direct(c):
    t = c.case.tree
    lo, hi = t.box()
    return cw.clear_wait_direct(t.state, t.pID, t.elen, t.xedge, c.case.test(), c.case.tracks, c.case.radii, c.case.start, c.W, lo, hi)


@pytest.mark.parametrize("case", cw.cases(), ids=lambda c: c.name)
def test_no_gpu_case_is_degenerate(case):
    """A condition on the INPUTS, shown with the reference alone: every case has a mask that is neither 0 nor all-ones and a goal
    hit that is clear only after a wait -- unless it exists to show that waiting changes nothing.  And the rule written out
    directly (clear_wait_direct) gives what W runs of clear_reference.clear give."""
    r = case.reference()
    print(case.name, r["stats"], bin(r["root_ok"]))
    if case.none:
        assert cw.degenerate(r, case.W), "marked as a none-case, but it is not"
        assert r["stats"]["best_wait"] <= 0
    else:
        assert cw.degenerate(r, case.W) == []
    full = cw.all_mask(case.W)
    assert all(int(m) <= full for m in r["clear"]) and all(int(m) <= full for m in r["dwell_ok"])
    assert all(int(m) & ~r["root_ok"] == 0 for m in r["clear"])                   # every mask lies within root_ok
    assert (r["root_ok"] + 1) & r["root_ok"] == 0                                # ... which is prefix-closed
    assert all(int(d) == 0 for d, h in zip(r["dwell_ok"], r["hit"]) if not h)
    d = _direct(case)
    for key in ("own_ok", "clear", "dwell_ok", "hit", "cum"):
        np.testing.assert_array_equal(d[key], r[key])
    assert d["stats"] == r["stats"] and d["root_ok"] == r["root_ok"]
    # ... also behind the cull that the reference of the fixture trees uses
    c, t = case.case, case.case.tree
    reach = fr.HALF_LENGTH if t.system == "boat_novice" else float(np.max(np.hypot(*c.vps())))
    rest = cl.row_test("advanced", np.zeros((2, 0)), speed_box=fr.PLAN_BOX) if t.system == "boat_advanced" else None
    lo, hi = t.box()
    k = cw.clear_wait_direct(t.state, t.pID, t.elen, t.xedge, cw.culled(c.test(), reach, car=t.system == "car", rest=rest), c.tracks, c.radii, c.start,
                             case.W, lo, hi)
    np.testing.assert_array_equal(k["clear"], r["clear"])
    np.testing.assert_array_equal(k["dwell_ok"], r["dwell_ok"])
    assert k["stats"] == r["stats"]


def _best(name, W=8):
    st = cw.case("%s | W = %d" % (name, W)).reference()["stats"]
    return st["best_arrival"], st["best_end"], st["best_wait"]


def test_the_results_the_issue_names():
    """Arrival, node, wait with the delays 0 .. 7.  One row of waiting brings the short branch back; the novice boat's tie on
    arrival (16) between node 2 at wait 5 and node 5 at wait 0 goes to the lower id."""
    assert _best("fork, the disc crosses the short branch") == (12, 2, 1)
    assert _best("car: the fork") == (12, 2, 1) and _best("boat_intermediate: the fork") == (12, 2, 1)
    assert _best("ros_boat on an occupied grid, 3073 hull points") == (13, 2, 2)
    assert _best("boat_novice: the inflated radius") == (16, 2, 5)
    nov = cw.case("boat_novice: the inflated radius | W = 8").reference()
    assert int(nov["clear"][5]) & int(nov["dwell_ok"][5]) & 1 and nov["cum"][5] == 16 and nov["cum"][2] == 11     # the tie
    for name in ("fork, dwell conflict at L - 1, the long branch arrives later", "fork, L = 8: the crossing is the last row (tau = L - 1)",
                 "fork, start >= L"):
        assert _best(name) == (16, 5, 0)
    for name in ("fork, the disc has passed (start = 4)", "fork, L = 7: the disc stops short, tau = L is clamped"):
        assert _best(name) == (11, 2, 0)
    for c in cw.cases():                                                         # without a wait: the best of the plain query
        r = c.reference()
        if r["stats"]["best_wait"] == 0:
            plain = r["runs"][0]["stats"]
            assert (r["stats"]["best_end"], r["stats"]["best_steps"]) == (plain["best_end"], plain["best_steps"])


def test_the_edge_cases_are_what_their_names_say():
    # the root fails at start + 3 only: the prefix 0b111, also where a later instant would pass again
    for name in ("fork, the root is hit at start + 3 | W = 8", "fork, start = 2, the root is hit at start + 3 | W = 8"):
        r = cw.case(name).reference()
        assert r["root_ok"] == 0b111 and [q["own_first"][0] for q in r["runs"]] == [-1, -1, -1, r["runs"][3]["own_first"][0], -1, -1, -1, -1]
        assert r["runs"][3]["own_first"][0] >= 0 and max(int(m) for m in r["clear"]) == 0b111
    # W = 64: bit 63 is set, a delay in the middle (59) is not, and W = 63 is the same without bit 63
    a, b = (cw.case("fork, L = 80, discs cross at rows 7 and 66 | W = %d" % W).reference() for W in (64, 63))
    assert int(a["clear"][2]) == (2 ** 64 - 1) & ~1 & ~(1 << 59) and int(a["clear"][2]) >> 63 == 1
    assert int(b["clear"][2]) == int(a["clear"][2]) & (2 ** 63 - 1) and int(b["dwell_ok"][2]) == 2 ** 63 - 1
    # the clamp: with start = L - 2 the root's delay 0 reads row L - 2, every later one row L - 1; on the edges all but one are clamped
    for name in ("fork, L = 8: the crossing is the last row (tau = L - 1)", "fork, L = 7: the disc stops short, tau = L is clamped"):
        c = cw.case(name + ", start = L - 2 | W = 8").case
        assert c.start == len(c.tracks) - 2
    c = cw.case("fork, L = 10, start = 0: delays on both sides of the clamp | W = 8")
    L, cum1 = len(c.case.tracks), 6                                              # node 2, row 1 (x = 7): tau = w + 7
    assert [w + cum1 + 1 >= L - 1 for w in range(8)] == [False, False] + [True] * 6 and int(c.reference()["clear"][2]) == 0xfe
    # the dwell suffix: node 2 arrives at w + 10, waits from w + 11 on, the disc comes at 13 = L - 1
    r = cw.case("fork, dwell conflict at L - 1 (suffix) | W = 8").reference()
    assert int(r["dwell_ok"][2]) == sum(1 << w for w in range(8) if w + 11 > 13) == 0xf8
    assert int(r["clear"][2]) == 0x07                                            # ... and who is still under way at 13 meets it there
    # deep chains: each of the three discs takes its bits at another ancestor
    for name, spine in [("N = %d, three spine nodes hit at one instant each | W = 8" % N, N - 4) for N in (255, 256, 257)] + \
                       [("chain of 256, three nodes hit at one instant each | W = 8", 255)]:
        r = cw.case(name).reference()
        js = cw.spine_hit_nodes(spine)
        for j, (_, w) in zip(js, cw.SPINE_HITS):
            assert not (int(r["own_ok"][j]) >> w) & 1 and (int(r["clear"][j - 1]) >> w) & 1
        assert int(r["clear"][js[0]]) == 0xff & ~0x84 and int(r["clear"][js[1] + 5]) == 0xff & ~0x84 & ~0x21
        assert int(r["clear"][spine]) == 0x18 and int(r["own_ok"][spine]) == 0xff
    r = cw.case("chain of 256, the root fails at start + 1 | W = 8").reference()
    assert r["root_ok"] == 1 and max(int(m) for m in r["clear"]) <= 1
    names = [c.name for c in cw.cases()]
    assert len(set(names)) == len(names)
    assert sorted(set(len(c.case.radii) for c in cw.cases()) & {64, 65}) == [64, 65]
    assert {c.case.tree.system for c in cw.cases()} >= {"car", "boat_novice", "boat_intermediate", "ros_boat", "boat_advanced"}


@pytest.mark.parametrize("case", cl.cases(), ids=lambda c: c.name)
def test_one_delay_is_the_plain_query(case):
    t = case.tree
    lo, hi = t.box()
    plain = case.reference()
    for fn in (cw.clear_wait, cw.clear_wait_direct):
        r = fn(t.state, t.pID, t.elen, t.xedge, case.test(), case.tracks, case.radii, case.start, 1, lo, hi)
        np.testing.assert_array_equal(r["clear"] == 1, plain["first"] == -1)
        np.testing.assert_array_equal(r["dwell_ok"] == 1, plain["dwell_first"] == -1)
        st, ps = r["stats"], plain["stats"]
        assert (st["size"], st["hits"], st["clear_hits"], st["clear_now"]) == (ps["size"], ps["hits"], ps["clear_hits"], ps["clear_hits"])
        assert (st["best_end"], st["best_steps"], st["best_arrival"]) == (ps["best_end"], ps["best_steps"], ps["best_steps"])
        assert st["best_wait"] == (0 if ps["best_end"] >= 0 else -1)


# ------------------------------------------------------------------------------------------------ the host side

def _native_planner():
    car = lqrrt_amd.systems.Car(0)
    cons = lqrrt_amd.Constraints(car.nstates, car.ncontrols, car.goal_buffer, car.is_feasible)
    return lqrrt_amd.Planner(car.dynamics, car.lqr, cons, error_tol=car.error_tol, erf=car.erf, goal0=car.goal, printing=False, **car.plan_kwargs)


@pytest.mark.parametrize("bad", [-1, 64, 100, 1.5, 2.0, "3", None, True], ids=repr)
def test_max_wait_refusals(bad):
    """On the host, before a tree or a device is looked at."""
    p, q = _native_planner(), _native_planner()
    with pytest.raises(ValueError, match="max_wait"):
        p.avoid(np.zeros((3, 1, 2)), 0.5, max_wait=bad)
    with pytest.raises(ValueError, match="max_wait"):
        lqrrt_amd.deconflict([p, q], 0.5, max_wait=bad)
    assert p.tree is None and p.plan_wait == 0
    for waits in (0, 65, -1, 1.0):
        with pytest.raises(ValueError, match="waits"):
            Engine.wait_count(waits)
    assert Engine.wait_count(1) == 1 and Engine.wait_count(np.int64(64)) == 64


def test_without_a_plan_nothing_happens_and_the_old_refusals_come_first():
    p = _native_planner()
    assert p.avoid(np.zeros((3, 1, 2)), 0.5, max_wait=7) is None and p.avoid(np.zeros((3, 1, 2)), 0.5, max_wait=0) is None
    with pytest.raises(ValueError):
        p.avoid(np.zeros((3, 2)), 0.5, max_wait=7)
    with pytest.raises(ValueError, match="no plan"):
        lqrrt_amd.deconflict([p, _native_planner()], 0.5, max_wait=8)
    assert "by nature" in lqrrt_amd.deconflict.__doc__ and "max_wait" in lqrrt_amd.deconflict.__doc__
    assert "hold station" in lqrrt_amd.Planner.avoid.__doc__


def test_callback_mode_is_refused():
    cons = lqrrt_amd.Constraints(2, 1, [0.1, 0.1], lambda x, u: True)
    p = lqrrt_amd.Planner(lambda x, u, dt: x + dt * np.array([x[1], u[0]]), lambda x, u: (np.eye(2), np.array([[1.0, 1.0]])), cons,
                          horizon=1, dt=0.1, goal0=[1.0, 0.0], printing=False)
    with pytest.raises(NotImplementedError, match="Python"):
        p.avoid(np.zeros((3, 1, 2)), 0.5, max_wait=3)
    with pytest.raises(NotImplementedError, match="Python"):
        lqrrt_amd.deconflict([p], 0.5, max_wait=3)


# ------------------------------------------------------------------------------------------------ ABI and sources

def test_header_declares_the_call():
    text = open(os.path.join(ROOT, "include", "lqrrt_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint lqrrt_tree_clear_wait\s*\((.*?)\);", code, re.S)
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 11 and args[6] == "int waits" and args[7] == "lqrrt_clear_wait_stats* out"
    assert args[8] == "uint64_t* clear_host" and args[9] == "uint64_t* dwell_host"
    s = re.search(r"typedef struct \{([^}]*)\} lqrrt_clear_wait_stats;", code, re.S)
    fields = re.findall(r"\b(?:int32_t|int64_t)\s+([a-z_, ]+);", s.group(1))
    assert [f.strip() for group in fields for f in group.split(",")] == list(cw.STAT_KEYS)
    assert len(nat.SIGNATURES["lqrrt_tree_clear_wait"][1]) == 11
    assert hasattr(nat.lib(), "lqrrt_tree_clear_wait") and nat.lib().lqrrt_abi_version() == 1
    assert C.sizeof(nat.ClearWaitStats) == 6 * 4 + 2 * 8 and [f[0] for f in nat.ClearWaitStats._fields_] == list(cw.STAT_KEYS)
    assert callable(Engine.tree_clear_wait)
    # the rule stands next to the declaration
    doc = text[text.index("lqrrt_tree_clear for `waits`"):text.index("lqrrt_clear_wait_stats;")]
    for word in ("root_ok", "own_ok", "dwell_ok", "prefix-closed", "waits outside 1 .. 64", "31 bits"):
        assert word in doc, word


def test_clear_wait_stays_plain_launches():
    for f in ("clear_wait.hpp", "engine_clear.hpp"):
        text = open(os.path.join(CSRC, f)).read()
        for word in FORBIDDEN:
            assert word not in text, (f, word)
    src = open(os.path.join(CSRC, "clear_wait.hpp")).read()
    shared = open(os.path.join(CSRC, "clear.hpp")).read()
    row = shared[shared.index("void clear_load_row("):]
    assert "S::feasible(" in src and "clear_load_row<S>(" in src and "trig_of<S>(" in row[:row.index("\n}\n")]
    assert "= stage_geo(" not in src and "has_discs<S>::value" in src
    assert "1 <<" not in src.replace("1ull <<", "") and "__builtin_ctz(" not in src and "__ffs(" not in src      # 64-bit shifts and ctz
    host, parts = clear_host_text()       # the host path of both calls: the refusals (clear_check) stand before all work (clear_run)
    retain = open(os.path.join(CSRC, "engine_retain.hpp")).read()
    links = retain[retain.index("static void retain_links("):retain.index("static int retain_run(")]
    assert "k_retain_init" in links and "k_retain_double" in links and "retain_links(" in parts["run"]
    assert "k_clear_wait_check<S>" in host and "hull_bytes, st" in host
    code = parts["wait"]
    assert "clear_call<ClearWait>(e, tracks_host, radii_host, L, D, start, waits," in code
    for refusal in ("L < 1 || D < 1", "start < 0", "std::isfinite(", "radii_host[d] >= 0.0", "waits < 1 || waits > 64", "has_discs<S>::value",
                    "!e->has_goal", "(long long)start + (waits - 1) + deepest > 0x7fffffffLL", "> e->lds_limit"):
        assert 0 <= parts["check"].index(refusal), refusal
    assert "static constexpr size_t CHECK_LDS = 64" in host and "hull_bytes + C::CHECK_LDS > e->lds_limit" in parts["check"]
    # transient, and the stream is drained before the scratch goes: the guard stands behind the scratch and is armed before the first copy
    run = parts["run"]
    assert "dalloc(" not in host and run.index("ClearScratch sc;") < run.index("dalloc_transient(&sc.mem") < run.index("StreamDrain drain(st);")
    assert run.index("StreamDrain drain(st);") < run.index("drain.arm();") < run.index("hipMemcpyAsync(")
    assert run.index("HIPCHK(hipStreamSynchronize(st));") < run.index("drain.disarm();")
    refine = open(os.path.join(CSRC, "engine_refine.hpp")).read()
    guard = refine[refine.index("struct StreamDrain {"):]
    assert "(void)hipStreamSynchronize(st)" in guard[:guard.index("\n};\n")]
    kernels = open(os.path.join(CSRC, "kernels.hpp")).read()
    assert kernels.index('#include "clear.hpp"') < kernels.index('#include "clear_wait.hpp"')
    engine = open(os.path.join(CSRC, "engine.hip")).read()
    assert engine.index('#include "engine_refine.hpp"') < engine.index('#include "engine_clear.hpp"') and "engine_clear_wait.hpp" not in engine


def test_check_kernel_stays_in_the_class_of_the_retain_check():
    """For every model with a circle path k_clear_wait_check<S> exists, and no other model has one; it has no private segment and
    keeps at least the occupancy of k_retain_check<S>."""
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
    retain, wait = by_model("k_retain_check"), by_model("k_clear_wait_check")
    assert sorted(wait) == ["BoatAdvanced", "BoatIntermediate", "BoatNovice", "BoatNoviceLqr", "Car", "RosBoat"]
    for model in sorted(wait):
        print("%-18s retain check %3d B occ %d vgpr %3d sgpr %3d   wait check %3d B occ %d vgpr %3d sgpr %3d lds %d" % (
            model, retain[model]["scratch"], retain[model]["occupancy"], retain[model]["vgpr"], retain[model].get("sgpr", -1),
            wait[model]["scratch"], wait[model]["occupancy"], wait[model]["vgpr"], wait[model].get("sgpr", -1), wait[model]["lds"]))
        assert wait[model]["scratch"] == 0
        assert wait[model]["occupancy"] >= retain[model]["occupancy"]
        assert wait[model]["lds"] <= 64                            # (static: the four partial masks and failure times; the hull is dynamic)
