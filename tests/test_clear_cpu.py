"""
The clearance query (Planner.avoid / Engine.tree_clear, csrc/clear.hpp) on the CPU: the reference of the rule
(tests/clear_reference.py) on hand-built trees against hand-computed answers, the reference's row test against the plain models of
feasibility_reference.py, every input of tests/test_clear_gpu.py shown not to be degenerate with the reference alone, the host side
of the public calls and their refusals, the ABI's declaration, and what the sources and the compiler say about the kernels.
"""
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
import clear_reference as cl
from clear_common import FORBIDDEN, clear_host_text
import feasibility_reference as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The fork (clear_reference.fork_nodes): cum by hand -- the short branch 1 + 5 + 5 = 11 (node 2), 6 below it 14, 9 and 10 below that
# 15; the long branch 6, 11, 16 (node 5); the twig 8, 9.
FORK_CUM = [1, 6, 11, 6, 11, 16, 14, 8, 9, 15, 15]
# (own_first, first, dwell_first, best_end, best_steps), worked out by hand from the geometry: the hull is 1.0 x 0.5 m around the
# pose, every disc has r = 0.4.  The crossing disc is at (7, tau - 7): it meets the vehicle of the short branch in row 1 of node 2
# (x = 7) at tau = 6 + 1 = 7 and is 0.9 m from the nearest hull point one row earlier and later.  The parked disc at (11, 0) reaches
# node 6 in its second row (x = 10.2, bow at 10.7; the first, bow at 10.6, is a hair more than 0.4 away) at tau = 11 + 1 = 12, node 9
# (x = 10.35) in its only row at 14, and both while they wait: the instant after they arrive (14, 15).
PINNED = {
    "fork, the disc crosses the short branch":
        ([-1, -1, 7, -1, -1, -1, 12, -1, -1, 14, -1], [-1, -1, 7, -1, -1, -1, 7, -1, -1, 7, 7],
         [-2, -2, -1, -2, -2, -1, 14, -2, -2, 15, -2], 5, 16),
    # start = 4: every row 4 later; at tau = 11 the disc is at (7, 4), long past the short branch
    "fork, the disc has passed (start = 4)":
        ([-1, -1, -1, -1, -1, -1, 16, -1, -1, 18, -1], [-1, -1, -1, -1, -1, -1, 16, -1, -1, 16, 16],
         [-2, -2, -1, -2, -2, -1, 18, -2, -2, 19, -2], 2, 11),
    # L = 14: the third disc jumps to (10, -0.6) in the last row, 0.35 m below the hull of a vehicle parked at (10, 0) (node 2,
    # arrived at 10: dwell conflict at 13 = L - 1) and 0.55 m below one at (10, 0.2) (node 5, which arrives at 15 >= L - 1 anyway)
    "fork, dwell conflict at L - 1, the long branch arrives later":
        ([-1, -1, -1, -1, -1, -1, 12, -1, -1, 14, -1], [-1, -1, -1, -1, -1, -1, 12, -1, -1, 12, 12],
         [-2, -2, 13, -2, -2, -1, -1, -2, -2, -1, -2], 5, 16),
    "fork, L = 8: the crossing is the last row (tau = L - 1)":
        ([-1, -1, 7, -1, -1, -1, 12, -1, -1, 14, -1], [-1, -1, 7, -1, -1, -1, 7, -1, -1, 7, 7],
         [-2, -2, -1, -2, -2, -1, -1, -2, -2, -1, -2], 5, 16),
    # L = 7: the track ends at (7, -1); at tau = 7 = L the disc is still there, 0.75 m from the hull
    "fork, L = 7: the disc stops short, tau = L is clamped":
        ([-1, -1, -1, -1, -1, -1, 12, -1, -1, 14, -1], [-1, -1, -1, -1, -1, -1, 12, -1, -1, 12, 12],
         [-2, -2, -1, -2, -2, -1, -1, -2, -2, -1, -2], 2, 11),
    # start = 8 = L: every row sees the last row of the tracks, the disc parked at (7, 0)
    "fork, start >= L":
        ([-1, -1, 15, -1, -1, -1, 20, -1, -1, 22, -1], [-1, -1, 15, -1, -1, -1, 15, -1, -1, 15, 15],
         [-2, -2, -1, -2, -2, -1, -1, -2, -2, -1, -2], 5, 16),
    # the car's vertex at 2p: node 7's last row (5, -2) puts it on the disc parked at (10, -4) at tau = 6 + 1 = 7
    "car: a disc on the 2p vertex of node 7's last row":
        ([-1, -1, 7, -1, -1, -1, -1, 7, -1, -1, -1], [-1, -1, 7, -1, -1, -1, 7, 7, 7, 7, 7],
         [-2, -2, -1, -2, -2, -1, -1, -2, -2, -1, -2], 5, 16),
    "boat_advanced: a disc on what would be a car's 2p vertex":
        ([-1, -1, 7, -1, -1, -1, -1, -1, -1, -1, -1], [-1, -1, 7, -1, -1, -1, 7, -1, -1, 7, 7],
         [-2, -2, -1, -2, -2, -1, -1, -2, -2, -1, -2], 5, 16),
    # the novice boat: radius 0.4 + half a boat length 2.667 = 3.067 m from the CENTRE: at tau = 5 the disc at (7, -2) is
    # sqrt(8) = 2.83 m from (5, 0) (node 1's last row), at tau = 4 it is sqrt(18) m from (4, 0)
    "boat_novice: the inflated radius":
        ([-1, 5, 6, -1, -1, -1, -1, 6, -1, -1, -1], [-1, 5, 5, -1, -1, -1, 5, 5, 5, 5, 5],
         [-2, -2, -1, -2, -2, -1, -1, -2, -2, -1, -2], 5, 16),
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_reference_gives_the_hand_computed_answers(name):
    own, first, dwell, best_end, best_steps = PINNED[name]
    r = cl.case(name).reference()
    print(name, r["stats"])
    assert r["cum"].tolist() == FORK_CUM
    assert r["own_first"].tolist() == own and r["first"].tolist() == first and r["dwell_first"].tolist() == dwell
    hits = [2, 5, 6, 9]
    assert np.flatnonzero(r["hit"]).tolist() == hits
    clear_hits = [i for i in hits if first[i] == -1 and dwell[i] == -1]
    assert r["stats"] == dict(size=11, conflicts=sum(v >= 0 for v in own), blocked=sum(o == -1 and f >= 0 for o, f in zip(own, first)),
                              hits=4, clear_hits=len(clear_hits), best_end=best_end, best_steps=best_steps)
    assert best_end in clear_hits and best_steps == FORK_CUM[best_end]


def test_reference_ties_go_to_the_lower_id_and_a_conflict_outweighs_fewer_steps():
    r = cl.case("L = 1, D = 1, two clear hits with equal steps").reference()
    assert r["cum"].tolist() == [1, 6, 6, 4, 5]
    assert r["own_first"].tolist() == [-1, -1, -1, 2, -1] and r["first"].tolist() == [-1, -1, -1, 2, 2]
    assert r["dwell_first"].tolist() == [-2, -1, -1, -1, -1]                     # L = 1: nobody waits against anything
    assert r["stats"] == dict(size=5, conflicts=1, blocked=1, hits=4, clear_hits=2, best_end=1, best_steps=6)


def test_reference_on_a_tree_of_one_node():
    hit, miss = cl.case("N=1, a disc on the root").reference(), cl.case("N=1, nothing near").reference()
    assert hit["first"].tolist() == [0] and miss["first"].tolist() == [-1] and hit["dwell_first"].tolist() == [-2]
    assert hit["stats"] == dict(size=1, conflicts=1, blocked=0, hits=0, clear_hits=0, best_end=-1, best_steps=-1)
    assert miss["stats"] == dict(size=1, conflicts=0, blocked=0, hits=0, clear_hits=0, best_end=-1, best_steps=-1)


def test_reference_chains():
    r = cl.case("chain of 33, conflict at node 1").reference()
    assert r["own_first"].tolist() == [-1, 2] + [-1] * 31 and r["first"].tolist() == [-1] + [2] * 32
    assert r["stats"] == dict(size=33, conflicts=1, blocked=31, hits=2, clear_hits=0, best_end=-1, best_steps=-1)
    r = cl.case("chain of 256, conflict on the root").reference()
    assert r["own_first"].tolist() == [0] + [-1] * 255 and r["first"].tolist() == [0] * 256
    assert r["stats"]["blocked"] == 255 and r["stats"]["hits"] > 0 and r["stats"]["clear_hits"] == 0
    for N in (255, 256, 257):
        r = cl.case("N = %d, the spine blocked at node 1" % N).reference()
        assert r["own_first"].tolist() == [-1, 1] + [-1] * (N - 2)
        assert r["first"].tolist() == [-1] + [1] * (N - 4) + [-1] * 3
        assert r["stats"]["best_end"] == N - 1 and r["stats"]["best_steps"] == 8 and r["stats"]["blocked"] == N - 5


def test_row_test_is_the_plain_models_row_by_row():
    """clear_reference.row_test takes the rows of an edge at once; per row it is circles_feasible / novice_feasible."""
    rs = np.random.RandomState(3)
    vps = fr.lattice_hull(1.0, 0.5, 0.25)
    R, D = 200, 5
    X = np.zeros((R, 6))
    X[:, :2] = rs.uniform(-3, 3, (R, 2))
    X[:, 2] = rs.uniform(-np.pi, np.pi, R)
    X[:, 3:] = rs.uniform(-0.7, 1.2, (R, 3)) * [1.0, 0.4, 0.2]
    discs = np.concatenate((rs.uniform(-3, 3, (R, D, 2)), rs.uniform(0.0, 0.8, (R, D, 1))), axis=2)
    discs[:, 0, 2] = 0.0
    c, s = fr.portable_sincos(X[:, 2])
    hull = cl.row_test("hull", vps)(X, c, s, discs)
    car = cl.row_test("car", vps)(X[:, [0, 1, 2, 3, 5]], c, s, discs)
    adv = cl.row_test("advanced", vps, speed_box=fr.PLAN_BOX)(X, c, s, discs)
    nov = cl.row_test("novice", half_length=fr.HALF_LENGTH)(X, c, s, discs)
    box = np.array([not (np.any(x[3:] > fr.PLAN_BOX[0]) or np.any(x[3:] < fr.PLAN_BOX[1])) for x in X])
    for k in range(R):
        plain = fr.circles_feasible(vps, discs[k], X[k], c[k], s[k])
        assert hull[k] == plain and adv[k] == (plain and box[k])
        assert car[k] == fr.circles_feasible(vps, discs[k], X[k], c[k], s[k], extra2p=True)
        assert nov[k] == fr.novice_feasible(discs[k], fr.HALF_LENGTH, X[k])
    assert 0 < hull.sum() < R and 0 < nov.sum() < R and (hull != car).any() and (hull != adv).any()


@pytest.mark.parametrize("case", cl.cases(), ids=lambda c: c.name)
def test_no_gpu_case_is_degenerate(case):
    """A condition on the INPUTS, shown with the reference alone: every case has a conflicting node, a blocked node, a clear hit and
    a hit that is not clear -- unless it exists to show 'none'."""
    r = case.reference()
    print(case.name, r["stats"])
    if case.none:
        assert cl.degenerate(r), "marked as a none-case, but it is not"
        assert r["stats"]["clear_hits"] == 0
    else:
        assert cl.degenerate(r) == []
    L = len(case.tracks)
    assert case.tracks.shape == (L, len(case.radii), 2)


def test_the_edge_cases_are_what_their_names_say():
    """Of the inputs again: the sizes, rows and instants the GPU cases are named after are really met."""
    by = {c.name: c for c in cl.cases()}
    assert sorted(set(len(c.radii) for c in by.values()) & {1, 2, 64, 65}) == [1, 2, 64, 65]
    assert sorted(c.tree.size for c in by.values() if c.name.startswith("N = ")) == [255, 256, 257]
    assert any(len(c.tracks) == 1 for c in by.values()) and any(c.start >= len(c.tracks) for c in by.values())
    assert 0.0 in by["fork, a radius-0 disc through a hull point"].radii
    fork = by["fork, the disc crosses the short branch"].tree
    assert fork.elen.tolist() == [1, 5, 5, 5, 5, 5, 3, 2, 1, 1, 1] and cl.H_HAND == 5         # edges of length 1 and of length H
    first_row, last_row = by["fork, conflict on the first row of an edge"].reference(), by["fork, conflict on the last row of an edge"].reference()
    assert first_row["own_first"][2] == 6 == first_row["cum"][1] and last_row["own_first"][2] == 10 == last_row["cum"][2] - 1
    # ... and only that row fails: the same disc one instant earlier or later (start - 1 is impossible: shift the track) passes
    for name, tau in (("fork, conflict on the first row of an edge", 6), ("fork, conflict on the last row of an edge", 10)):
        c = by[name]
        t = c.tree
        lo, hi = t.box()
        for shift in (-1, 1):
            moved = np.roll(c.tracks, shift, axis=0)
            assert cl.clear(t.state, t.pID, t.elen, t.xedge, c.test(), moved, c.radii, 0, lo, hi)["own_first"][2] != tau
    # the crossing disc of D = 64 / 65 is the last of its table (lane 63 of the first cull tile, lane 0 of the second), or the first
    for name, where in (("fork, D = 64, the crossing disc last", 63), ("fork, D = 65, the crossing disc last", 64),
                        ("fork, D = 65, the crossing disc first", 0)):
        c = by[name]
        assert np.array_equal(c.tracks[:, where], cl.crossing(len(c.tracks)))
        others = np.delete(np.arange(len(c.radii)), where)
        t = c.tree
        lo, hi = t.box()
        assert cl.clear(t.state, t.pID, t.elen, t.xedge, c.test(), c.tracks[:, others], c.radii[others], 0, lo, hi)["own_first"][2] == -1
    # the dwell conflict is at tau' = L - 1 exactly, and the long branch arrives at or after it
    c = by["fork, dwell conflict at L - 1, the long branch arrives later"]
    r = c.reference()
    assert r["dwell_first"][2] == len(c.tracks) - 1 and r["cum"][5] - 1 + c.start >= len(c.tracks) - 1 and r["dwell_first"][5] == -1
    # the occupancy grid of the RosBoat case is occupied everywhere (whoever read it would refuse every row), and its hull does not
    # fit where stage_geo would put it
    c = by["ros_boat on an occupied grid, 3073 hull points"]
    assert c.grid and c.vps().shape == (2, 3073) and 2 * 3073 * 8 > fr.OG_LDS_BYTES


@pytest.mark.parametrize("name", ["car_2000", "boat_advanced_3000"])
def test_fixture_inputs_are_not_degenerate(name):
    r = cl.fixture_reference(name)
    f = cl.fixture(name)
    print(name, r["stats"])
    assert cl.degenerate(r) == []
    end = f.plan[-1]
    assert r["hit"][end] and r["first"][end] >= 0                                 # the discs stand on the fixture's own plan
    tracks, radii = f.tracks()
    assert tracks.shape == (len(f.plan_rows()) + 60, 4, 2) and r["stats"]["best_end"] != end


# ------------------------------------------------------------------------------------------------ the host side

def _native_planner(dt=None):
    car = lqrrt_amd.systems.Car(0)
    cons = lqrrt_amd.Constraints(car.nstates, car.ncontrols, car.goal_buffer, car.is_feasible)
    kw = dict(car.plan_kwargs)
    if dt is not None:
        kw["dt"] = dt
    return car, lqrrt_amd.Planner(car.dynamics, car.lqr, cons, error_tol=car.error_tol, erf=car.erf, goal0=car.goal, printing=False, **kw)


BAD_TRACKS = [dict(tracks=np.zeros((0, 1, 2)), radii=0.5),                       # L = 0
              dict(tracks=np.zeros((3, 0, 2)), radii=0.5),                       # D = 0
              dict(tracks=np.zeros((3, 2, 3)), radii=0.5),
              dict(tracks=np.zeros((3, 2)), radii=0.5),
              dict(tracks=[], radii=0.5),
              dict(tracks=[np.zeros((0, 2))], radii=0.5),
              dict(tracks=[np.zeros((4, 3))], radii=0.5),
              dict(tracks=np.zeros((3, 2, 2)), radii=0.5, start=-1),
              dict(tracks=np.zeros((3, 2, 2)), radii=0.5, start=1.5),
              dict(tracks=np.full((3, 2, 2), np.nan), radii=0.5),
              dict(tracks=np.array([[[0.0, np.inf]]]), radii=0.5),
              dict(tracks=np.zeros((3, 2, 2)), radii=-0.1),
              dict(tracks=np.zeros((3, 2, 2)), radii=[0.5, np.nan]),
              dict(tracks=np.zeros((3, 2, 2)), radii=[0.5, 0.5, 0.5])]


@pytest.mark.parametrize("bad", BAD_TRACKS, ids=lambda b: "%s r=%s start=%s" % (np.shape(b["tracks"]), b["radii"], b.get("start", 0)))
def test_refusals(bad):
    """Every argument is checked on the host before anything else is looked at: also without a tree, also without a device."""
    with pytest.raises(ValueError):
        Engine.track_table(**bad)
    car, p = _native_planner()
    with pytest.raises(ValueError):
        p.avoid(**bad)
    assert p.tree is None and not p.plan_reached_goal


def test_track_table_pads_by_holding_the_last_row():
    a, b = np.arange(8.0).reshape(4, 2), np.array([[9.0, 9.5]])
    table, radii, start = Engine.track_table([a, b], 0.5, 2)
    assert table.shape == (4, 2, 2) and start == 2 and radii.tolist() == [0.5, 0.5]
    assert np.array_equal(table[:, 0], a) and np.array_equal(table[:, 1], np.tile(b, (4, 1)))
    t2, r2, _ = Engine.track_table(table, [0.0, 1.0])
    assert np.array_equal(t2, table) and r2.tolist() == [0.0, 1.0] and t2.flags["C_CONTIGUOUS"]


def test_without_a_plan_nothing_happens():
    car, p = _native_planner()
    assert p.avoid(np.zeros((3, 1, 2)), 0.5) is None
    assert p.avoid([np.zeros((3, 2))], [0.5], start=2, adopt=False) is None
    assert p.tree is None and not hasattr(p, "node_seq") and not p.plan_reached_goal


def test_callback_mode_is_refused():
    cons = lqrrt_amd.Constraints(2, 1, [0.1, 0.1], lambda x, u: True)
    p = lqrrt_amd.Planner(lambda x, u, dt: x + dt * np.array([x[1], u[0]]), lambda x, u: (np.eye(2), np.array([[1.0, 1.0]])), cons,
                          horizon=1, dt=0.1, goal0=[1.0, 0.0], printing=False)
    assert p.callback_mode
    with pytest.raises(NotImplementedError, match="Python"):
        p.avoid(np.zeros((3, 1, 2)), 0.5)
    with pytest.raises(NotImplementedError, match="Python"):
        lqrrt_amd.deconflict([p], 0.5)


def test_deconflict_refusals():
    assert "deconflict" in lqrrt_amd.__all__ and "deconflict" in lqrrt.__all__ and lqrrt.deconflict is lqrrt_amd.deconflict
    (_, a), (_, b), (_, c) = _native_planner(), _native_planner(), _native_planner(dt=0.05)
    assert a.dt == b.dt != c.dt
    with pytest.raises(ValueError, match="share dt"):
        lqrrt_amd.deconflict([a, b, c], 0.5)
    with pytest.raises(ValueError, match="twice"):
        lqrrt_amd.deconflict([a, a], 0.5)
    with pytest.raises(ValueError, match="permutation"):
        lqrrt_amd.deconflict([a, b], 0.5, order=[0, 0])
    for radii in (-1.0, [0.5], [0.5, 0.5, 0.5]):
        with pytest.raises(ValueError, match="radius"):
            lqrrt_amd.deconflict([a, b], radii)
    with pytest.raises(ValueError, match="start"):
        lqrrt_amd.deconflict([a, b], 0.5, start=-1)
    with pytest.raises(ValueError, match="no plan"):
        lqrrt_amd.deconflict([a, b], 0.5)
    assert "inherent" in lqrrt_amd.deconflict.__doc__ or "by nature" in lqrrt_amd.deconflict.__doc__


# ------------------------------------------------------------------------------------------------ ABI and sources

def test_header_declares_the_call():
    text = open(os.path.join(ROOT, "include", "lqrrt_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint lqrrt_tree_clear\s*\((.*?)\);", code, re.S)
    assert m and len(m.group(1).split(",")) == 10 and "lqrrt_clear_stats* out" in m.group(1)
    assert re.search(r"typedef struct \{[^}]*\} lqrrt_clear_stats;", code, re.S)
    assert "lqrrt_tree_clear" in nat.SIGNATURES and len(nat.SIGNATURES["lqrrt_tree_clear"][1]) == 10
    assert hasattr(nat.lib(), "lqrrt_tree_clear") and nat.lib().lqrrt_abi_version() == 1
    import ctypes as C
    assert C.sizeof(nat.ClearStats) == 6 * 4 + 8 and [f[0] for f in nat.ClearStats._fields_] == list(cl.STAT_KEYS)
    assert callable(Engine.tree_clear) and callable(lqrrt_amd.Planner.avoid)


def test_clear_stays_plain_launches():
    """One stream, plain launches: no cooperative launch, no grid-wide barrier, no assembly; the step sums are the retain's bodies."""
    csrc = os.path.join(ROOT, "lqrrt_amd", "csrc")
    for f in ("clear.hpp", "engine_clear.hpp"):
        text = open(os.path.join(csrc, f)).read()
        for word in FORBIDDEN:
            assert word not in text, (f, word)
    src = open(os.path.join(csrc, "clear.hpp")).read()
    assert src.count("__launch_bounds__(64)") == 1 and "S::feasible(" in src and "trig_of<S>(" in src and "= stage_geo(" not in src
    assert "hull_lds[q] = g.vps[q]" in src and "gd.og = nullptr; gd.O = D;" in src and "has_discs" in src
    host, parts = clear_host_text()
    retain = open(os.path.join(csrc, "engine_retain.hpp")).read()
    links = retain[retain.index("static void retain_links("):retain.index("static int retain_run(")]
    rounds = retain[retain.index("static void double_rounds("):retain.index("static void retain_links(")]
    assert "k_retain_init" in links and "double_rounds(k_retain_double" in links and "hipLaunchKernelGGL(round," in rounds
    assert "retain_links(e, 0, N, nullptr" in parts["run"] and "k_clear_check<S>" in host and "hull_bytes, st" in host
    # every refusal stands before the first thing that is enqueued or allocated
    for refusal in ("L < 1 || D < 1", "start < 0", "std::isfinite(", "radii_host[d] >= 0.0", "!e->has_goal", "leave 31 bits", "has_discs<S>::value",
                    "hull_bytes + C::CHECK_LDS > e->lds_limit"):
        assert 0 <= parts["check"].index(refusal), refusal
    order = [parts["check"].index(r) for r in ("null argument", "L < 1 || D < 1", "start < 0", "track table too large", "std::isfinite(",
                                               "radii_host[d] >= 0.0", "waits < 1 || waits > 64", "has_discs<S>::value", "!e->has_res",
                                               "!e->has_goal", "the root's edge has no row", "p < 0 || p >= v", "leave 31 bits",
                                               "> e->lds_limit")]
    assert order == sorted(order)                                                  # ... in the order the calls have always refused in
    assert "static constexpr size_t CHECK_LDS = 0" in host and 'WAIT_TERM = "";' in host
    # transient: the footprint stays
    assert "dalloc_transient(&sc.mem" in parts["run"] and "dalloc(" not in host
    launch = open(os.path.join(csrc, "engine_launch.hpp")).read()
    transient = launch[launch.index("static int dalloc_transient("):]
    transient = transient[:transient.index("\n}\n")]
    assert transient.index("keep = g_dalloc_bytes") < transient.index("dalloc(p, count)") < transient.index("g_dalloc_bytes = keep;")
    systems = open(os.path.join(csrc, "systems.hpp")).read()
    assert systems.count("static constexpr bool DISCS = true;") == 2               # BoatCommon (the boats) and Car
    kernels = open(os.path.join(csrc, "kernels.hpp")).read()
    assert kernels.index('#include "retain.hpp"') < kernels.index('#include "clear.hpp"')
    engine = open(os.path.join(csrc, "engine.hip")).read()
    assert engine.index('#include "engine_retain.hpp"') < engine.index('#include "engine_refine.hpp"') < engine.index('#include "engine_clear.hpp"')


def test_the_two_signatures_are_what_they_were():
    import ctypes as C
    I, P = C.c_int, C.c_void_p
    assert nat.SIGNATURES["lqrrt_tree_clear"] == (I, [P, P, P, I, I, I, C.POINTER(nat.ClearStats), P, P, P])
    assert nat.SIGNATURES["lqrrt_tree_clear_wait"] == (I, [P, P, P, I, I, I, I, C.POINTER(nat.ClearWaitStats), P, P, P])


def test_check_kernel_stays_in_the_class_of_the_retain_check():
    """For every model with a circle path k_clear_check<S> exists, and no other model has one; its private segment is that of
    k_retain_check<S> (none) and it keeps at least that kernel's occupancy."""
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
    retain, clear = by_model("k_retain_check"), by_model("k_clear_check")
    assert sorted(clear) == ["BoatAdvanced", "BoatIntermediate", "BoatNovice", "BoatNoviceLqr", "Car", "RosBoat"]
    assert "UserSystem" in retain and "Pendulum" in retain
    for model in sorted(clear):
        print("%-18s retain check %3d B occ %d vgpr %3d sgpr %3d   clear check %3d B occ %d vgpr %3d sgpr %3d" % (
            model, retain[model]["scratch"], retain[model]["occupancy"], retain[model]["vgpr"], retain[model].get("sgpr", -1),
            clear[model]["scratch"], clear[model]["occupancy"], clear[model]["vgpr"], clear[model].get("sgpr", -1)))
        assert clear[model]["scratch"] == 0 == retain[model]["scratch"]
        assert clear[model]["occupancy"] >= retain[model]["occupancy"] and clear[model]["lds"] == 0      # (dynamic LDS only: the hull)
