"""
The clearance query against moving oriented rectangles with departure delays (Planner.avoid_rects(max_wait) /
Engine.tree_clear_rects_wait, csrc/clear_rects_wait.hpp) on the CPU: the reference of the rule
(tests/clear_rects_wait_reference.py) against answers worked out by hand on the fork, its direct form against the composed one,
every input of tests/test_clear_rects_wait_gpu.py shown not to be degenerate with the reference alone, the host side of the public
calls and their refusals, the ABI's declaration, and what the sources and the compiler say about the kernel.
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
import clear_rects_reference as cr
import clear_rects_wait_reference as rw
import clear_wait_reference as cw
from clear_common import FORBIDDEN
import feasibility_reference as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lqrrt_amd", "csrc")


def _direct(c, test=None):
    t = c.case.tree
    lo, hi = t.box()
    return rw.clear_rects_wait_direct(t.state, t.pID, t.elen, t.xedge, c.case.test() if test is None else test, c.case.tracks, c.case.extents,
                                      c.case.start, c.W, lo, hi)


@pytest.mark.parametrize("case", rw.cases(), ids=lambda c: c.name)
def test_no_gpu_case_is_degenerate(case):
    """A condition on the INPUTS, shown with the reference alone: every case has a mask that is neither 0 nor all-ones and a goal
    hit that is clear only after a wait -- unless it exists to show that waiting changes nothing.  And the rule written out
    directly (clear_rects_wait_direct), with and without the cull of the large trees, gives what W runs of
    clear_rects_reference.clear_rects give."""
    r = case.reference()
    print(case.name, r["stats"], bin(r["root_ok"]))
    if case.none:
        assert rw.degenerate(r, case.W), "marked as a none-case, but it is not"
        assert r["stats"]["best_wait"] <= 0
    else:
        assert rw.degenerate(r, case.W) == []
    full = rw.all_mask(case.W)
    assert all(int(m) <= full for m in r["clear"]) and all(int(m) <= full for m in r["dwell_ok"])
    assert all(int(m) & ~r["root_ok"] == 0 for m in r["clear"])                   # every mask lies within root_ok
    assert (r["root_ok"] + 1) & r["root_ok"] == 0                                # ... which is prefix-closed
    assert all(int(d) == 0 for d, h in zip(r["dwell_ok"], r["hit"]) if not h)
    c, t = case.case, case.case.tree
    if t.system == "boat_novice":
        cull = rw.culled(c.test(), 0.0, grow=fr.HALF_LENGTH)
    else:
        cull = rw.culled(c.test(), float(np.max(np.hypot(*c.vps()))))
    for d in (_direct(case), _direct(case, cull)):
        for key in ("own_ok", "clear", "dwell_ok", "hit", "cum"):
            np.testing.assert_array_equal(d[key], r[key])
        assert d["stats"] == r["stats"] and d["root_ok"] == r["root_ok"]


def test_unchanged_is_the_cap():
    """Of clear_rects_reference.cases() at W = 8, exactly the named ones lack something; of the 27 under 60 nodes, nine."""
    lacking = {c.case.name for c in rw.cases()[:len(cr.cases())] if rw.degenerate(c.reference(), 8)}
    assert [c.case.name for c in rw.cases()[:len(cr.cases())]] == [c.name for c in cr.cases()]
    assert lacking == set(rw.UNCHANGED) and len(set(rw.UNCHANGED)) == len(rw.UNCHANGED)
    small = [c for c in cr.cases() if c.tree.size < 60]
    assert len(small) == 27 and sum(c.name in lacking for c in small) == 9
    for c in rw.cases():
        assert c.none == bool(rw.degenerate(c.reference(), c.W)), c.name
    # the wait-specific cases that change nothing by waiting, and why: the clamp with start = L - 2 (every delay but the root's
    # first reads the last row: one answer for all), the dwell suffix (the conflict is at the goal at L - 1: who is under way then
    # meets it too), the chain whose root fails at start + 1 (root_ok = 0b1: there is no waiting)
    own_none = [c.name for c in rw.cases()[len(cr.cases()):] if c.none]
    assert own_none == ["fork, L = 8: the crossing is the last row (tau = L - 1), start = L - 2 | W = 8",
                        "fork, L = 7: the rectangle stops short, tau = L is clamped, start = L - 2 | W = 8",
                        "fork, dwell conflict at L - 1 (suffix) | W = 8", "chain of 256, the root fails at start + 1 | W = 8"]


def _best(name, W=8):
    st = rw.case("%s | W = %d" % (name, W)).reference()["stats"]
    return st["best_end"], st["best_wait"], st["best_arrival"]


def test_hand_computed_answers_on_the_fork():
    """From the rule, not from the code.  The fork (clear_reference.fork_nodes): cum[0] = 1, so at delay w node 1's rows x = 1 .. 5
    on y = 0 have tau = w + 1 .. w + 5, node 2's rows x = 6 .. 10 have tau = w + 6 .. w + 10: the vehicle is at (tau - w, 0), node 2
    is a hit with cum = 11 and waits at (10, 0) from tau = w + 11 on; the long branch (node 5) arrives in 16 and is touched by
    none of the rectangles below.  The small hull is a lattice of 0.25 m: at heading 0 its points are (x + {-0.5 .. 0.5},
    {-0.25, 0, 0.25}).  The parked rectangle at (11, 0) spans x in [10.65, 11.35]: node 2's hull ends at 10.5."""
    plain = cr.case("fork, the rectangle crosses the short branch").reference()["stats"]
    assert (plain["best_end"], plain["best_steps"]) == (5, 16)
    # the square of half side 0.4 has its centre at (7, tau - 7) and spans x in [6.6, 7.4]: only the vehicle at x = 7 (hull points at
    # x = 6.75, 7, 7.25; at x = 6 the hull ends at 6.5, at x = 8 it begins at 7.5) can be in it, and it is there at tau = w + 7, when
    # the square spans y in [w - 0.4, w + 0.4]: w = 0 holds (7, 0), w >= 1 begins at 0.6 > 0.25.  Node 2: bits 1 .. 7, best (2, 1, 12)
    assert _best("fork, the rectangle crosses the short branch") == (2, 1, 12)
    assert int(rw.case("fork, the rectangle crosses the short branch | W = 8").reference()["clear"][2]) == 0xfe
    # the 6 x 0.4 rectangle at heading pi/2 has its centre at (14 - tau, 0.6) and spans x in [13.8 - tau, 14.2 - tau], y in
    # [-2.4, 3.6] -- all of the hull's y.  The vehicle's centre is at tau - w: the rectangle's is d = 14 + w - 2 tau from it, an
    # integer; a hull point is within 0.2 of it iff d = 0 (the lattice point nearest to d = +-1 is 0.5 away), tau = 7 + w / 2: w = 0
    # is hit at tau = 7, w = 1 has no such instant
    assert _best("fork, the same track, heading pi/2") == (2, 1, 12)
    # at heading 0 it spans y in [0.4, 0.8]: above the hull's 0.25 at every instant; no wait is needed
    assert _best("fork, a 6 x 0.4 rectangle passes beside the short branch") == (2, 0, 11)
    # ros_boat's hull of 3 073 points is a dense lattice over [-1, 1] x [-0.3, 0.3] (0.0046 m along x).  The square spans y in
    # [tau - 7.4, tau - 6.6], which meets |y| <= 0.3 at tau = 7 alone; then the vehicle of delay w spans x in [6 - w, 8 - w] and the
    # square [6.6, 7.4]: w = 0 and 1 overlap, w = 2 ends at 6.0
    assert _best("ros_boat on an occupied grid, 3073 hull points, D = 65") == (2, 2, 13)
    for c in rw.cases():                                                         # without a wait: the best of the plain query
        r = c.reference()
        if r["stats"]["best_wait"] == 0:
            p = r["runs"][0]["stats"]
            assert (r["stats"]["best_end"], r["stats"]["best_steps"]) == (p["best_end"], p["best_steps"])


def test_the_edge_cases_are_what_their_names_say():
    # the root fails at start + 3 only: the prefix 0b111, also where a later instant would pass again
    for name in ("fork, the root is hit at start + 3 | W = 8", "fork, start = 2, the root is hit at start + 3 | W = 8"):
        r = rw.case(name).reference()
        assert r["root_ok"] == 0b111 and [q["own_first"][0] for q in r["runs"]] == [-1, -1, -1, r["runs"][3]["own_first"][0], -1, -1, -1, -1]
        assert r["runs"][3]["own_first"][0] >= 0 and max(int(m) for m in r["clear"]) == 0b111
    # W = 64: bit 63 is set, a delay in the middle (59) is not, and W = 63 is the same without bit 63
    a, b = (rw.case("fork, L = 80, squares cross at rows 7 and 66 | W = %d" % W).reference() for W in (64, 63))
    assert int(a["clear"][2]) == (2 ** 64 - 1) & ~1 & ~(1 << 59) and int(a["clear"][2]) >> 63 == 1
    assert int(b["clear"][2]) == int(a["clear"][2]) & (2 ** 63 - 1) and int(b["dwell_ok"][2]) == 2 ** 63 - 1
    # W = 2, 3, 5: wavefronts 2 and 3 (then 3) own no delay; at W = 5 wavefront 0 owns two and the others one
    assert [bin(0x1111111111111111 << q & rw.all_mask(W)).count("1") for W in (2, 3, 5) for q in range(4)] == [1, 1, 0, 0, 1, 1, 1, 0, 2, 1, 1, 1]
    for W in (2, 3, 5):
        assert int(rw.case("fork, the rectangle crosses the short branch | W = %d" % W).reference()["clear"][2]) == rw.all_mask(W) & ~1
    # the clamp
    for name in ("fork, L = 8: the crossing is the last row (tau = L - 1)", "fork, L = 7: the rectangle stops short, tau = L is clamped"):
        c = rw.case(name + ", start = L - 2 | W = 8").case
        assert c.start == len(c.tracks) - 2
    c = rw.case("fork, L = 10, start = 0: delays on both sides of the clamp | W = 8")
    L, cum1 = len(c.case.tracks), 6                                              # node 2, row 1 (x = 7): tau = w + 7
    assert [w + cum1 + 1 >= L - 1 for w in range(8)] == [False, False] + [True] * 6 and int(c.reference()["clear"][2]) == 0xfe
    # the dwell suffix: node 2 arrives at w + 10, waits from w + 11 on, the rectangle comes at 13 = L - 1
    r = rw.case("fork, dwell conflict at L - 1 (suffix) | W = 8").reference()
    assert int(r["dwell_ok"][2]) == sum(1 << w for w in range(8) if w + 11 > 13) == 0xf8
    assert int(r["clear"][2]) == 0x07                                            # ... and who is still under way at 13 meets it there
    # the empty dwell range: every hit has cum >= 11 > L - 1 = 7
    c = rw.case("fork, L = 8, every hit arrives after L - 1 | W = 8")
    r = c.reference()
    assert len(c.case.tracks) == 8 and min(int(r["cum"][i]) for i in np.flatnonzero(r["hit"])) == 11
    assert all(int(d) == 0xff for d, h in zip(r["dwell_ok"], r["hit"]) if h) and int(r["clear"][1]) == 0xfe
    # deep chains: each of the three squares takes its bits at another ancestor
    for name, spine in [("N = %d, three spine nodes hit at one instant each | W = 8" % N, N - 4) for N in (255, 256, 257)] + \
                       [("chain of 256, three nodes hit at one instant each | W = 8", 255)]:
        r = rw.case(name).reference()
        js = rw.spine_hit_nodes(spine)
        for j, (_, w) in zip(js, rw.SPINE_HITS):
            assert not (int(r["own_ok"][j]) >> w) & 1 and (int(r["clear"][j - 1]) >> w) & 1
        assert int(r["clear"][js[0]]) == 0xff & ~0x84 and int(r["clear"][js[1] + 5]) == 0xff & ~0x84 & ~0x21
        assert int(r["clear"][spine]) == 0x18 and int(r["own_ok"][spine]) == 0xff
    r = rw.case("chain of 256, the root fails at start + 1 | W = 8").reference()
    assert r["root_ok"] == 1 and max(int(m) for m in r["clear"]) <= 1
    names = [c.name for c in rw.cases()]
    assert len(set(names)) == len(names)
    assert max(c.case.tree.size for c in rw.cases()) == 257


def test_the_tie_goes_to_the_smaller_id():
    """The square parks on the short branch at (7, 0) through row 11: delay w has the vehicle there at tau = w + 7, so w = 0 .. 4
    meet it and w = 5 arrives at 11 + 5 = 16 -- when node 5 of the long branch arrives at delay 0.  (16, 2) < (16, 5)."""
    r = rw.case("fork, a tie: wait 5 on the short branch arrives with the long one | W = 8").reference()
    assert int(r["clear"][2]) & int(r["dwell_ok"][2]) == 0xe0 and int(r["clear"][5]) & int(r["dwell_ok"][5]) & 1
    assert r["cum"][2] + rw.TIE_WAIT == r["cum"][5] == 16
    st = r["stats"]
    assert (st["best_end"], st["best_wait"], st["best_steps"], st["best_arrival"]) == (2, 5, 11, 16)


def test_what_a_disc_cannot_say_with_time():
    """The 6 m x 0.4 m rectangle at heading pi/2 moves up x = 7 along its own length: it spans y in [tau - 10, tau - 4] and x in
    [6.8, 7.2], and the vehicle at x = 7 at tau = w + 7 is in it for w <= 3; a wait of 4 rows clears it.  The covering disc of
    3.007 m on the same centre track needs strictly longer, or finds nothing within W."""
    c = rw.case("fork, a 6 x 0.4 rectangle at heading pi/2 crosses the short branch | W = 8")
    rect, disc = c.reference(), c.disc_reference()
    print(rect["stats"], disc["stats"])
    assert int(rect["clear"][2]) == 0xf0 and (rect["stats"]["best_end"], rect["stats"]["best_wait"]) == (2, 4)
    lowest = lambda m: (m & -m).bit_length() - 1 if m else None
    d2 = lowest(int(disc["clear"][2]) & int(disc["dwell_ok"][2]))
    assert d2 is None or d2 > 4
    assert disc["stats"]["best_end"] == -1 or disc["stats"]["best_arrival"] > rect["stats"]["best_arrival"]
    np.testing.assert_allclose(c.case.radii[-1], np.hypot(3.0, 0.2))


@pytest.mark.parametrize("case", cr.cases(), ids=lambda c: c.name)
def test_one_delay_is_the_plain_query(case):
    t = case.tree
    lo, hi = t.box()
    plain = case.reference()
    for fn in (rw.clear_rects_wait, rw.clear_rects_wait_direct):
        r = fn(t.state, t.pID, t.elen, t.xedge, case.test(), case.tracks, case.extents, case.start, 1, lo, hi)
        np.testing.assert_array_equal(r["clear"] == 1, plain["first"] == -1)
        np.testing.assert_array_equal(r["dwell_ok"] == 1, plain["dwell_first"] == -1)
        st, ps = r["stats"], plain["stats"]
        assert (st["size"], st["hits"], st["clear_hits"], st["clear_now"]) == (ps["size"], ps["hits"], ps["clear_hits"], ps["clear_hits"])
        assert (st["best_end"], st["best_steps"], st["best_arrival"]) == (ps["best_end"], ps["best_steps"], ps["best_steps"])
        assert st["best_wait"] == (0 if ps["best_end"] >= 0 else -1)


@pytest.mark.parametrize("name", ["car_2000", "boat_advanced_3000"])
def test_fixture_inputs_are_not_degenerate(name):
    r = rw.fixture_reference(name)
    print(name, r["stats"])
    # the delays differ somewhere, some hit is clear and some is not (a hit that is clear only after a wait is asked of the hand
    # cases: four rectangles on a plan of a thousand rows leave the car's one clear hit clear at once)
    assert "partial mask" not in rw.degenerate(r, rw.FIXTURE_W) and 0 < r["stats"]["clear_hits"] < r["stats"]["hits"]
    plain = cr.fixture_reference(name)
    np.testing.assert_array_equal((r["clear"] & np.uint64(1)) == 1, plain["first"] == -1)      # delay 0 is the plain query, uncut
    np.testing.assert_array_equal((r["dwell_ok"] & np.uint64(1)) == 1, plain["dwell_first"] == -1)
    assert r["stats"]["clear_now"] == plain["stats"]["clear_hits"]


# ------------------------------------------------------------------------------------------------ the host side

E = (1.0, 0.5)


def _native_planner():
    car = lqrrt_amd.systems.Car(0)
    cons = lqrrt_amd.Constraints(car.nstates, car.ncontrols, car.goal_buffer, car.is_feasible)
    return lqrrt_amd.Planner(car.dynamics, car.lqr, cons, error_tol=car.error_tol, erf=car.erf, goal0=car.goal, printing=False, **car.plan_kwargs)


@pytest.mark.parametrize("bad", [-1, 64, 1.5, True, 2.0, "3", None], ids=repr)
def test_max_wait_refusals(bad):
    """On the host, before a tree or a device is looked at."""
    p = _native_planner()
    with pytest.raises(ValueError, match="max_wait"):
        p.avoid_rects(np.zeros((3, 1, 3)), E, max_wait=bad)
    assert p.tree is None and p.plan_wait == 0


def test_waits_refusals_at_the_engine():
    """tree_clear_rects_wait checks the table, then waits, before it touches its handle: no engine is needed to be refused."""
    class NoEngine(object):
        rect_table, wait_count = staticmethod(Engine.rect_table), staticmethod(Engine.wait_count)
    for waits in (0, 65, -1, 1.0, True):
        with pytest.raises(ValueError, match="waits"):
            Engine.tree_clear_rects_wait(NoEngine(), np.zeros((3, 1, 3)), E, 0, waits)
    with pytest.raises(ValueError, match="tracks"):
        Engine.tree_clear_rects_wait(NoEngine(), np.zeros((3, 1, 2)), E, 0, 0)      # the table's refusals come first


def test_without_a_plan_nothing_happens_and_the_old_refusals_come_first():
    p = _native_planner()
    assert p.avoid_rects(np.zeros((3, 1, 3)), E, max_wait=7) is None and p.avoid_rects(np.zeros((3, 1, 3)), E, max_wait=0) is None
    assert p.avoid_rects([np.zeros((3, 3))], [E], start=2, adopt=False, max_wait=63) is None
    with pytest.raises(ValueError, match="tracks"):
        p.avoid_rects(np.zeros((3, 2)), E, max_wait=7)
    assert p.tree is None and not hasattr(p, "node_seq") and p.plan_wait == 0
    doc = lqrrt_amd.Planner.avoid_rects.__doc__
    assert "max_wait" in doc and "clear_rects_wait_reference" in doc


def test_callback_mode_is_refused():
    cons = lqrrt_amd.Constraints(2, 1, [0.1, 0.1], lambda x, u: True)
    p = lqrrt_amd.Planner(lambda x, u, dt: x + dt * np.array([x[1], u[0]]), lambda x, u: (np.eye(2), np.array([[1.0, 1.0]])), cons,
                          horizon=1, dt=0.1, goal0=[1.0, 0.0], printing=False)
    assert p.callback_mode
    with pytest.raises(NotImplementedError, match="Python"):
        p.avoid_rects(np.zeros((3, 1, 3)), E, max_wait=3)


# ------------------------------------------------------------------------------------------------ ABI and sources

def test_header_declares_the_call():
    text = open(os.path.join(ROOT, "include", "lqrrt_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint lqrrt_tree_clear_rects_wait\s*\((.*?)\);", code, re.S)
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["lqrrt_engine* e", "const double* tracks_host", "const double* extents_host", "int L", "int D", "int start", "int waits",
                    "lqrrt_clear_wait_stats* out", "uint64_t* clear_host", "uint64_t* dwell_host", "void* stream"]
    I, P = C.c_int, C.c_void_p
    assert nat.SIGNATURES["lqrrt_tree_clear_rects_wait"] == (I, [P, P, P, I, I, I, I, C.POINTER(nat.ClearWaitStats), P, P, P])
    assert hasattr(nat.lib(), "lqrrt_tree_clear_rects_wait") and nat.lib().lqrrt_abi_version() == 1
    assert C.sizeof(nat.ClearWaitStats) == 6 * 4 + 2 * 8 and [f[0] for f in nat.ClearWaitStats._fields_] == list(rw.STAT_KEYS)
    assert rw.STAT_KEYS == cw.STAT_KEYS and callable(Engine.tree_clear_rects_wait)
    # the rule stands next to the declaration, by reference to the two comments it is made of
    doc = text[text.index("/* lqrrt_tree_clear_rects for `waits`"):text.index("int lqrrt_tree_clear_rects_wait(")]
    for word in ("lqrrt_tree_clear_wait's comment", "lqrrt_tree_clear_rects's comment", "root_ok", "dwell_ok", "waits outside 1 .. 64", "31 bits",
                 "section 22"):
        assert word in doc, word


def test_the_fragments_stay_plain_launches_on_the_existing_host_path():
    kern, host = (open(os.path.join(CSRC, f)).read() for f in ("clear_rects_wait.hpp", "engine_clear_rects_wait.hpp"))
    for text in (kern, host):
        for word in FORBIDDEN:
            assert word not in text, word
        assert "dalloc(" not in text
    # the kernel: clear_wait_check_body's shape round clear_rects.hpp's row test, as it stands
    assert kern.count("__launch_bounds__(CLEAR_WAIT_BLOCK)") == 1 and "k_clear_rects_wait_check" in kern
    for reused in ("clear_stage_hull(g, hull_lds, tid, CLEAR_WAIT_BLOCK)", "clear_load_row<S>(", "clear_rects_hit<S>(", "goal_hit<S>(",
                   "link[tv.pID[i]].steps", "clear_wait_all(W)", "part[CLEAR_WAIT_WAVES]", "fail[CLEAR_WAIT_WAVES]", "lane = tid & 63",
                   "has_discs<S>::value"):
        assert reused in kern, reused
    code = re.sub(r"//[^\n]*", "", kern)
    assert "S::feasible(" not in code and "Params" not in code and "clear_disc_world(" not in code and "stage_geo(" not in code
    assert "1 <<" not in code.replace("1ull <<", "") and "__builtin_ctz(" not in code and "__ffs(" not in code      # 64-bit shifts and ctz
    rects = open(os.path.join(CSRC, "clear_rects.hpp")).read()
    assert "bool clear_rects_hit(" in rects and "bool clear_rects_hit(" not in kern
    # the host: the traits, the existing run, the refusals of clear_rects_check ahead of it; one launch, nothing allocated or copied
    assert host.count("hipLaunchKernelGGL(") == 1 and "hipMemcpy" not in host and "hipMalloc" not in host
    assert "k_clear_rects_wait_check<S>), dim3((unsigned)N), dim3(CLEAR_WAIT_BLOCK), hull_bytes, st" in host
    for words in ("typedef ClearWaitLink Link;", "typedef unsigned long long Node;", "typedef ClearWaitOut Out;", "typedef lqrrt_clear_wait_stats Stats;",
                  "CHECK_LDS = 64", "HIT_BYTES = sizeof(int)", "ClearWait::select(", "ClearWait::stats(", "NOT_GENERIC(e);"):
        assert words in host, words
    export = host[host.index('extern "C" int lqrrt_tree_clear_rects_wait('):]
    assert export.index("NOT_GENERIC(e);") < export.index("TRY(clear_rects_check<ClearRectsWait>(") < export.index("TRY(use_device(e));") \
        < export.index("clear_run<ClearRectsWait>(")
    plain = open(os.path.join(CSRC, "engine_clear_rects.hpp")).read()
    check = plain[plain.index("static int clear_rects_check("):plain.index('extern "C" int lqrrt_tree_clear_rects(')]
    order = [check.index(r) for r in ("extents_host[d] >= 0.0", "waits < 1 || waits > 64", "has_discs<S>::value", "!e->has_goal",
                                      "(long long)start + (waits - 1) + deepest > 0x7fffffffLL", "hull_bytes + C::CHECK_LDS > e->lds_limit",
                                      "table.resize(")]
    assert order == sorted(order) and "int waits = 1)" in check and "C::WAIT_TERM" in check
    assert 'WAIT_TERM = ""' in plain and "WAIT_TERM = ClearWait::WAIT_TERM" in host
    kernels = open(os.path.join(CSRC, "kernels.hpp")).read()
    assert kernels.index('#include "clear_wait.hpp"') < kernels.index('#include "clear_rects.hpp"') < kernels.index('#include "clear_rects_wait.hpp"')
    engine = open(os.path.join(CSRC, "engine.hip")).read()
    assert engine.index('#include "engine_clear.hpp"') < engine.index('#include "engine_clear_rects.hpp"') \
        < engine.index('#include "engine_clear_rects_wait.hpp"')
    life = open(os.path.join(CSRC, "engine_lifecycle.hpp")).read()
    assert "clear_rects_wait" not in life                                         # nothing of it enters lqrrt_engine_footprint


def test_check_kernel_has_no_private_segment_and_its_static_lds_is_the_joins():
    """k_clear_rects_wait_check<S> exists for exactly the six models of k_clear_check<S>; its private segment is 0 bytes and its
    static LDS (the four partial masks and failure times) is within the CHECK_LDS the host adds to the hull points."""
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
    clear, wait, rects = by_model("k_clear_check"), by_model("k_clear_wait_check"), by_model("k_clear_rects_wait_check")
    assert sorted(rects) == sorted(clear) == ["BoatAdvanced", "BoatIntermediate", "BoatNovice", "BoatNoviceLqr", "Car", "RosBoat"]
    for model in sorted(rects):
        print("%-18s disc wait check %3d B occ %d vgpr %3d sgpr %3d lds %d   rect wait check %3d B occ %d vgpr %3d sgpr %3d lds %d" % (
            model, wait[model]["scratch"], wait[model]["occupancy"], wait[model]["vgpr"], wait[model].get("sgpr", -1), wait[model]["lds"],
            rects[model]["scratch"], rects[model]["occupancy"], rects[model]["vgpr"], rects[model].get("sgpr", -1), rects[model]["lds"]))
        assert rects[model]["scratch"] == 0
        assert 0 < rects[model]["lds"] <= 64
