"""
Clear goal chains on the device (csrc/clear_connect.hpp through lqrrt_tree_clear_connect, Engine.tree_clear_connect,
Planner.avoid(connect)) against the reference of the rule (tests/clear_connect_reference.py).  Everything compared is an integer and
must be EQUAL: the seven counters, first, dwell_first, and the five chain fields.  The winner is then committed with the unchanged
connect_commit and the unchanged tree_clear must find the new node clear at the arrival the call reported.
tests/test_clear_connect_cpu.py shows with the reference alone that no case is degenerate.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import clear_connect_reference as ccr
import clear_reference as cl
import connect_reference as cr
import feasibility_reference as fr
import retain_reference as rr
from clear_common import WAVE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _engine(tree, extra=64):
    """`tree` (a clear_connect_reference.Tree) on an engine with its system's own resolution: the chains are real steers."""
    from lqrrt_amd.engine import Engine
    s = tree.system
    kw = s.plan_kwargs
    eng = Engine(s, capacity=tree.size + extra, max_wave=64)
    eng.set_resolution(kw["dt"], kw["FPR"], max(int(tree.elen.max()), tree.H), np.abs(np.asarray(s.error_tol, dtype=np.float64)), s.goal,
                       np.abs(np.asarray(s.goal_buffer, dtype=np.float64)))
    xe, ue = tree.packed()
    eng.tree_load(tree.state, tree.K, tree.pID, tree.elen, xe, ue)
    return eng


def _compare(eng, tree, ref, tracks, radii, start, tries=8, nodes=None):
    st, ch, first, dwell = eng.tree_clear_connect(tracks, radii, start, tree.H, tries, nodes, per_node=True)
    print(st, ch)
    np.testing.assert_array_equal(first, ref["first"])
    np.testing.assert_array_equal(dwell, ref["dwell_first"])
    assert first.dtype == np.int32 and dwell.dtype == np.int32
    assert st == ref["stats"] and ch == ref["chain"]
    assert eng.tree_clear_connect(tracks, radii, start, tree.H, tries, nodes) == (st, ch)       # the same call without the arrays
    assert eng.tree_clear(tracks, radii, start) == st                                          # ... and the unchanged query's counters
    return st, ch


def _commit_is_consistent(eng, tree, ch, tracks, radii, start, tries=8):
    """The winner committed by the unchanged connect_commit; the unchanged tree_clear on the same tracks then finds the chain's last
    node clear, waiting unharmed, the best clear hit, at the arrival the search reported."""
    size = eng.size
    ids = eng.connect_commit(ch["chain_from"], tree.H, tries)
    assert ids == list(range(size, size + len(ids))) and eng.climb(ids[-1])[-len(ids) - 1] == ch["chain_from"]
    assert int(np.sum(eng.edge_lengths(ids[0], len(ids)))) == ch["chain_rows"]
    st, first, dwell = eng.tree_clear(tracks, radii, start, per_node=True)
    assert first[ids[-1]] == -1 and dwell[ids[-1]] == -1
    assert st["best_end"] == ids[-1] and st["best_steps"] == ch["chain_arrival"]
    eng.tree_truncate(size)


@pytest.mark.parametrize("case", ccr.cases(), ids=lambda c: c.name)
def test_cases_against_the_reference(case):
    eng = _engine(case.tree)
    fp = eng.footprint()
    st, ch = _compare(eng, case.tree, case.reference(), case.tracks, case.radii, case.start, case.tries, case.nodes)
    assert eng.footprint() == fp
    if ch["chain_from"] >= 0:
        _commit_is_consistent(eng, case.tree, ch, case.tracks, case.radii, case.start, case.tries)
    eng.close()


def test_far_discs_give_the_unchanged_connection_search():
    for name in ("far discs", "a chain strictly shorter than the best clear hit", "a chain that only ties with the best clear hit"):
        c = ccr.case(name)
        eng = _engine(c.tree)
        ref = c.reference()
        st, ch = eng.tree_clear_connect(c.tracks, c.radii, c.start, c.tree.H, c.tries, c.nodes)
        want = eng.connect_search(c.tree.H, ref["incumbent"], c.tries, c.nodes)
        assert want == (None if ch["chain_from"] < 0 else (ch["chain_cost"], ch["chain_from"])), name
        if st["best_end"] >= 0:
            assert ref["incumbent"] == st["best_steps"] - int(c.tree.elen[0]) + 1
        eng.close()


def test_id_lists():
    c = ccr.case("last row of the last edge")
    eng = _engine(c.tree)
    want = c.reference()["chain"]
    ids = np.random.RandomState(5).permutation(c.tree.size)
    for nodes in (ids, np.sort(ids), ids[::-1]):
        assert eng.tree_clear_connect(c.tracks, c.radii, c.start, c.tree.H, nodes=nodes)[1] == want
    twice = np.concatenate((ids, ids))
    got = eng.tree_clear_connect(c.tracks, c.radii, c.start, c.tree.H, nodes=twice)[1]
    assert got == dict(want, clear_candidates=2 * want["clear_candidates"])       # (entries of the list are counted, not nodes)
    rest = [int(v) for v in ids if v != want["chain_from"]]
    ref = ccr.clear_connect(c.tree, c.tracks, c.radii, c.start, nodes=rest)
    assert eng.tree_clear_connect(c.tracks, c.radii, c.start, c.tree.H, nodes=rest)[1] == ref["chain"] != want
    st, ch = eng.tree_clear_connect(c.tracks, c.radii, c.start, c.tree.H, nodes=[])
    assert st == c.reference()["stats"] and ch == dict(clear_candidates=0, chain_from=-1, chain_cost=-1, chain_rows=-1, chain_arrival=-1)
    for bad in ([0, c.tree.size], [-1]):
        with pytest.raises(ValueError):
            eng.tree_clear_connect(c.tracks, c.radii, c.start, c.tree.H, nodes=bad)
    eng.close()


def test_refusals_in_their_order_write_nothing():
    import ctypes as C
    from lqrrt_amd import _native as nat
    c = ccr.case("far discs")
    eng = _engine(c.tree)
    H, N = c.tree.H, c.tree.size
    good = eng.tree_clear_connect(c.tracks, c.radii, 0, H)
    fp = eng.footprint()
    tr, ra = np.ascontiguousarray(c.tracks), np.ascontiguousarray(c.radii)
    L, D = tr.shape[:2]
    nanpos = tr.copy()
    nanpos[-1, -1, 1] = np.inf
    negr = ra.copy()
    negr[-1] = -1.0
    outside = np.array([0, N], dtype=np.int32)
    inside = np.array([0, 1], dtype=np.int32)

    def call(tracks=tr, radii=ra, L=L, D=D, start=0, H=H, tries=8, ids=None, count=0, chain=True):
        st, ch = nat.ClearStats(), nat.ClearConnectStats()
        first, dwell = np.full(N, 77, dtype=np.int32), np.full(N, 77, dtype=np.int32)
        C.memset(C.byref(st), 0x55, C.sizeof(st))
        C.memset(C.byref(ch), 0x55, C.sizeof(ch))
        rc = nat.lib().lqrrt_tree_clear_connect(eng.h, nat.ptr(tracks), nat.ptr(radii), L, D, start, H, tries, None if ids is None else nat.ptr(ids),
                                                count, C.byref(st), C.byref(ch) if chain else None, nat.ptr(first), nat.ptr(dwell), eng._stream())
        msg = nat.lib().lqrrt_last_error().decode() if rc else ""
        untouched = bytes(st) == b"\x55" * C.sizeof(st) and bytes(ch) == b"\x55" * C.sizeof(ch) and np.all(first == 77) and np.all(dwell == 77)
        return rc, msg, untouched
    # every refusal alone: the clearance's, then the connection's
    alone = [(dict(L=0), "L >= 1"), (dict(D=0), "L >= 1"), (dict(start=-1), "start"), (dict(tracks=nanpos), "finite"), (dict(radii=negr), "radius"),
             (dict(start=2 ** 31 - 2), "31 bits"), (dict(chain=False), "null"), (dict(tries=0), "goal_tries"), (dict(H=0), "horizon"),
             (dict(H=10 ** 6), "horizon"), (dict(ids=inside, count=-1), "negative"), (dict(ids=outside, count=2), "outside the tree")]
    for kw, word in alone:
        rc, msg, untouched = call(**kw)
        assert rc == nat.E_ARG and word in msg and untouched, (kw, msg)
    # two faults at once: the earlier refusal answers
    for kw, word in ((dict(start=-1, tries=0), "start"), (dict(radii=negr, H=0), "radius"), (dict(tries=0, H=0), "goal_tries"),
                     (dict(H=0, ids=outside, count=2), "horizon"), (dict(L=0, start=-1), "L >= 1"), (dict(tracks=nanpos, ids=outside, count=2), "finite")):
        rc, msg, untouched = call(**kw)
        assert rc == nat.E_ARG and word in msg and untouched, (kw, msg)
    rc, msg, untouched = call()
    assert rc == 0 and not untouched
    assert eng.tree_clear_connect(c.tracks, c.radii, 0, H) == good and eng.footprint() == fp
    # no goal: the clearance's refusal
    s = c.tree.system
    eng.set_resolution(s.plan_kwargs["dt"], 0.0, H, np.ones(s.nstates), None, None)
    xe, ue = c.tree.packed()
    eng.tree_load(c.tree.state, c.tree.K, c.tree.pID, c.tree.elen, xe, ue)
    rc, msg, untouched = call()
    assert rc == nat.E_STATE and "goal" in msg and untouched
    eng.close()


def test_the_lds_limit_is_refused_last():
    import lqrrt_amd
    c = cl.case("fork, the disc crosses the short branch")
    s = lqrrt_amd.systems.BoatIntermediate(0)
    import torch
    limit = int(torch.cuda.get_device_properties(0).shared_memory_per_block)
    s.vps = np.random.RandomState(0).uniform(-1, 1, (2, limit // 16 - 1))       # 16 V fits the clearance check alone, not the search
    s.set_obstacles(np.zeros((0, 3)))
    from clear_common import _load
    eng = _load(s, c.tree, cl.H_HAND, goal=c.tree.goal, goal_buffer=c.tree.goal_buffer)
    assert eng.tree_clear(c.tracks, c.radii, 0)["size"] == c.tree.size
    with pytest.raises(ValueError, match="LDS"):
        eng.tree_clear_connect(c.tracks, c.radii, 0, cl.H_HAND)
    with pytest.raises(ValueError, match="goal_tries"):
        eng.tree_clear_connect(c.tracks, c.radii, 0, cl.H_HAND, tries=0)        # (an earlier refusal answers first)
    eng.close()


def test_wrong_kind_of_engine():
    import lqrrt_amd
    from lqrrt_amd import _native as nat
    from lqrrt_amd.engine import Engine
    s = lqrrt_amd.systems.DoublePendulum()
    e = Engine(s, capacity=64, max_wave=64)
    e.set_resolution(0.1, 0.0, 4, np.ones(s.nstates), s.goal, np.abs(np.asarray(s.goal_buffer, dtype=np.float64)))
    e.tree_reset(s.x0)
    with pytest.raises(nat.NativeError) as ex:
        e.tree_clear_connect(np.zeros((2, 1, 2)), 0.5, 0, 4)
    assert ex.value.code == nat.E_STATE and "circle" in str(ex.value)
    e.close()
    # a generic engine (no plugins compiled in): the raw call, every argument in order
    import ctypes as C
    from lqrrt_amd.engine import NodeTable
    table = NodeTable(3, 1, capacity=64)
    tracks, radii = np.zeros((2, 1, 2)), np.array([0.5])
    st, ch = nat.ClearStats(), nat.ClearConnectStats()
    rc = nat.lib().lqrrt_tree_clear_connect(table.h, nat.ptr(tracks), nat.ptr(radii), 2, 1, 0, 4, 8, None, 0, C.byref(st), C.byref(ch), None, None,
                                            C.c_void_p(0))
    assert rc == nat.E_STATE and b"GENERIC" in nat.lib().lqrrt_last_error()
    table.close()


def _grow(s, H, size, seed=1):
    """A tree grown on the device by an engine set up as Planner does it (clear_common._grown, for any system)."""
    from lqrrt_amd.engine import Engine
    kw = s.plan_kwargs
    eng = Engine(s, capacity=2 * size + 2 * WAVE + 8, max_wave=WAVE)
    eng.set_resolution(kw["dt"], kw["FPR"], H, np.abs(s.error_tol), s.goal, np.abs(s.goal_buffer))
    space = np.array(s.sample_space, dtype=np.float64)
    eng.set_sampler(np.mean(space, axis=1), np.diff(space).flatten(), np.array(s.goal_bias, dtype=np.float64), 10)
    st = np.random.RandomState(seed).get_state()
    eng.set_mt19937(st[1], st[2])
    eng.tree_reset(s.x0)
    eng.extend(WAVE, node_limit=size)
    return eng


def _tree_of(s, eng, H):
    state, K, pID, elen, xedge, uedge = rr.engine_arrays(eng)
    return ccr.Tree(s, state, K, pID, elen, xedge, uedge, H)


def _system(name):
    import lqrrt_amd
    S = lqrrt_amd.systems
    if name == "ros_boat":                                          # its occupancy grid, a hull too large for stage_geo's LDS copy
        s, g = cr.case("ros_boat")
        s.set_occupancy_grid(g["grid"], g["origin"], cpm=float(g["cpm"]), threshold=float(g["threshold"]), vps=fr.big_lattice_hull())
        return s, 30, 150                                           # (3073 hull points make the reference's row tests slow: a small tree)
    s = S.SYSTEMS[name](0)
    return s, int(s.plan_kwargs["horizon"] / s.plan_kwargs["dt"]), 600 if name == "boat_advanced" else 300


@pytest.mark.parametrize("name", ["boat_advanced", "boat_novice", "ros_boat"])
def test_grown_trees_of_other_systems(name):
    """A tree grown on the device and read back; every goal hit crossed by a disc of its own, then a further disc on the winner's
    chain.  boat_advanced: the speed box comes before the hull; boat_novice: the inflated radius; ros_boat: the static steer reads
    the occupancy grid and the hull from HBM (og_lds == 0) while the disc test reads neither."""
    s, H, size = _system(name)
    eng = _grow(s, H, size)
    tree = _tree_of(s, eng, H)
    assert size <= tree.size <= size + 1
    if name == "ros_boat":
        assert 2 * 8 * np.asarray(s.vps).size // 2 > 48 * 1024
    winners = 0
    for c in ccr.generic_cases(tree, name) + [ccr.Case("%s: far discs" % name, tree, ccr.far(40, 2), winner=None)]:
        ref = c.reference()
        kinds = sorted(set(w[0] for w in ref["verdicts"].values()))
        print(c.name, tree.size, c.tracks.shape, ref["incumbent"], kinds)
        st, ch = _compare(eng, tree, ref, c.tracks, c.radii, c.start)
        if ch["chain_from"] >= 0:
            winners += 1
            _commit_is_consistent(eng, tree, ch, c.tracks, c.radii, c.start)
    print(name, "cases with a winner:", winners)
    eng.close()


def test_nothing_is_written_and_the_tree_grows_on_as_its_twin():
    s, H, size = _system("boat_advanced")
    eng, twin = _grow(s, H, size), _grow(s, H, size)
    before = rr.engine_arrays(eng)
    ign, best, fp, counters, mt = eng.ignored(), eng.plan_best(), eng.footprint(), eng.counters().as_dict(), eng.get_mt19937()
    tree = _tree_of(s, eng, H)
    tracks = ccr.cross_hits(tree, extra=9 * H)
    st, ch = eng.tree_clear_connect(tracks, 0.3, 0, H)
    assert st["size"] == eng.size
    after = rr.engine_arrays(eng)
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(eng.ignored(), ign)
    assert eng.plan_best() == best and eng.footprint() == fp and eng.counters().as_dict() == counters
    key, pos = eng.get_mt19937()
    assert pos == mt[1] and np.array_equal(key, mt[0])
    for e in (eng, twin):
        e.extend(WAVE, node_limit=size + 300)
    assert eng.size == twin.size >= size + 300
    (sa, Ka, pa, la, xa, ua), (sb, Kb, pb, lb, xb, ub) = rr.engine_arrays(eng), rr.engine_arrays(twin)
    for a, b in ((sa, sb), (Ka, Kb), (pa, pb), (la, lb)):
        np.testing.assert_array_equal(a, b)
    live = np.arange(xa.shape[1])[None, :] < la[:, None]
    np.testing.assert_array_equal(xa[live], xb[live])
    np.testing.assert_array_equal(ua[live], ub[live])
    assert eng.plan_best() == twin.plan_best()
    eng.close()
    twin.close()


# ------------------------------------------------------------------------------------------------ planner level

def _car_planner(max_nodes, seed=1, **kw):
    """tests/test_connect_gpu.py _car_planner: the fixture's recipe."""
    import lqrrt_amd
    s = lqrrt_amd.systems.Car(0)
    cons = lqrrt_amd.Constraints(s.nstates, s.ncontrols, s.goal_buffer, s.is_feasible)
    p = lqrrt_amd.Planner(s.dynamics, s.lqr, cons, error_tol=s.error_tol, erf=s.erf, goal0=s.goal, printing=False,
                          max_nodes=max_nodes, wave_size=256, **dict(s.plan_kwargs, **kw))
    np.random.seed(seed)
    p.update_plan(s.x0, s.sample_space, goal_bias=s.goal_bias, xrand_gen=10, finish_on_goal=False)
    return s, p


def _planner_with_crossed_hits(max_nodes=300):
    s, p = _car_planner(max_nodes, min_time=2, max_time=3, sys_time=lambda: 0.0)
    assert p.plan_reached_goal
    tree = _tree_of(s, p._engine, p.horizon_iters)
    tracks = ccr.cross_hits(tree, extra=9 * p.horizon_iters)
    return s, p, tree, tracks


def test_avoid_connect_adopts_a_chain_when_every_hit_is_crossed():
    s, p, tree, tracks = _planner_with_crossed_hits()
    ref = ccr.clear_connect(tree, tracks, 0.3, 0)
    assert ref["stats"]["hits"] >= 1 and ref["stats"]["clear_hits"] == 0 and ref["chain"]["chain_from"] >= 0
    seq, size = list(p.node_seq), p._engine.size
    plain = p.avoid(tracks, 0.3, adopt=True)
    assert plain["clear_hits"] == 0 and plain["best_end"] == -1 and plain["plan_first"] is not None and p.node_seq == seq
    # adopt=False: the answer, and nothing changes
    out = p.avoid(tracks, 0.3, adopt=False, connect=8)
    assert {k: out[k] for k in ccr.CHAIN_KEYS} == ref["chain"] and out["chain_committed"] is False
    assert {k: out[k] for k in cl.STAT_KEYS} == ref["stats"] and out["plan_first"] == plain["plan_first"]
    assert p._engine.size == size and p.node_seq == seq
    # adopt: the chain is committed and becomes the plan
    out = p.avoid(tracks, 0.3, connect=8)
    ch = ref["chain"]
    assert out["chain_committed"] is True and {k: out[k] for k in ccr.CHAIN_KEYS} == ch and out["plan_first"] == plain["plan_first"]
    ids = list(range(size, p._engine.size))
    assert len(ids) >= 1 and p.node_seq == p._engine.climb(ch["chain_from"]) + ids and p.tree.size == p._engine.size
    assert p.plan_reached_goal and p.plan_wait == 0 and p._in_goal(p.x_seq[-1])
    assert len(p.x_seq) == ch["chain_cost"] and p.T == ch["chain_cost"] * p.dt and p.tree._host_nodes() == 0
    # the unchanged query: the plan is clear now, and the best the tree holds
    again = p.avoid(tracks, 0.3, adopt=False)
    assert again["plan_first"] is None and again["best_end"] == p.node_seq[-1] and again["best_steps"] == ch["chain_arrival"]
    assert again["clear_hits"] == 1
    # nothing shorter is left: a second call finds no chain that beats the adopted one
    more = p.avoid(tracks, 0.3, connect=8)
    assert more["chain_from"] == -1 and more["chain_committed"] is False and more["best_end"] == p.node_seq[-1]


def test_avoid_connect_at_capacity_adopts_the_best_clear_hit():
    from test_connect_gpu import _fill
    s, p = _car_planner(300, min_time=2, max_time=3, sys_time=lambda: 0.0)
    eng = p._engine
    tree = _tree_of(s, eng, p.horizon_iters)
    res = ccr.plain(tree)
    hits = np.flatnonzero(res["hit"])
    assert len(hits) >= 2
    # every hit crossed but the one that arrives last: it is the best clear hit, and a chain beats it
    keep = int(hits[np.argmax(res["cum"][hits])])
    L = int(res["cum"].max()) + 9 * p.horizon_iters
    cols = [ccr.instant(L, int(res["cum"][h]) - 1, tree.touch(tree.xedge[h, tree.elen[h] - 1])) for h in hits if h != keep]
    tracks = np.stack(cols, axis=1)
    ref = ccr.clear_connect(tree, tracks, 0.3, 0)
    print(ref["stats"], ref["chain"])
    if ref["chain"]["chain_from"] < 0 or ref["stats"]["best_end"] < 0:
        pytest.fail("the tree offers no chain that beats its last clear hit: %s %s" % (ref["stats"], ref["chain"]))
    size = _fill(eng, s.x0, eng.gains(0, 1)[0])
    nodes = list(range(tree.size))
    ref = ccr.clear_connect(tree, tracks, 0.3, 0, nodes=nodes)
    # (the root's copies that fill the tree are no part of the reference's tree: through the engine with an id list)
    st, ch = eng.tree_clear_connect(tracks, 0.3, 0, p.horizon_iters, nodes=nodes)
    assert ch == ref["chain"] and ch["chain_from"] >= 0
    out = p.avoid(tracks, 0.3, connect=8)
    assert out["chain_committed"] is False and eng.size == size
    assert out["best_end"] == st["best_end"] >= 0 and p.node_seq == eng.climb(out["best_end"]) and p.plan_reached_goal


def test_avoid_connect_0_is_todays_avoid():
    (s, p, tree, tracks), (_, twin, _, _) = _planner_with_crossed_hits(), _planner_with_crossed_hits()
    far = ccr.far(len(tracks), 2)
    for tr in (tracks, far):
        a, b = p.avoid(tr, 0.3, connect=0), twin.avoid(tr, 0.3)
        assert a == b and list(a) == list(b) and "chain_from" not in a
        assert p.node_seq == twin.node_seq and p.T == twin.T and p._engine.size == twin._engine.size
        assert np.array_equal(np.asarray(p.x_seq), np.asarray(twin.x_seq))


def test_example_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "clear_connect_gpu.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    assert "avoid alone: clear_hits 0" in out.stdout and "chain committed: True" in out.stdout and "plan_first None" in out.stdout
