"""
Clear goal chains for several trees per launch on the device (csrc/clear_connect_multi.hpp through lqrrt_tree_clear_connect_multi,
Engine.tree_clear_connect_multi, lqrrt_amd.avoids(connect), deconflict(connect)).  The rule: member k of a call answers EXACTLY as
the one-tree call (Engine.tree_clear_connect) on its engine with its own arguments -- and that call is compared with the reference
of the rule in tests/test_clear_connect_gpu.py.  Everything compared is an integer, a mask or a dict and must be EQUAL.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import clear_connect_reference as ccr
import clear_reference as cl
import connect_reference as cr
import retain_reference as rr
from clear_common import WAVE, _load
from test_clear_connect_gpu import _car_planner, _engine, _grow, _planner_with_crossed_hits, _system, _tree_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_CHAIN = dict(chain_from=-1, chain_cost=-1, chain_rows=-1, chain_arrival=-1)


def _multi(engines, members, per_node=True):
    """One call for `members` = [(tracks, radii, start, H, tries, nodes)], one per engine."""
    from lqrrt_amd.engine import Engine
    cols = list(zip(*members))
    return Engine.tree_clear_connect_multi(engines, cols[0], cols[1], cols[2], cols[3], list(cols[4]), list(cols[5]), per_node=per_node)


def _solo(eng, member):
    tracks, radii, start, H, tries, nodes = member
    return eng.tree_clear_connect(tracks, radii, start, H, tries, nodes, per_node=True)


def _same(got, want):
    """One member's answer (stats, chain, first, dwell_first) against another's: equal, and int32."""
    assert got[0] == want[0] and got[1] == want[1], (got[:2], want[:2])
    np.testing.assert_array_equal(got[2], want[2])
    np.testing.assert_array_equal(got[3], want[3])
    assert got[2].dtype == np.int32 and got[3].dtype == np.int32 and len(got[2]) == len(got[3]) == got[0]["size"]


# ------------------------------------------------------------------------------------------------ 1: every hand-built case in one call

def _by_system():
    groups = {}
    for c in ccr.cases():
        groups.setdefault(type(c.tree.system).__name__, []).append(c)
    return groups


def test_the_car_group_holds_every_kind_of_member():
    """From the references alone (no device): what a call over the car cases mixes."""
    car = _by_system()["Car"]
    refs = [c.reference() for c in car]
    assert any(r["chain"]["chain_from"] >= 0 for r in refs) and any(r["chain"]["chain_from"] < 0 for r in refs)
    assert any(c.nodes is not None for c in car) and any(c.nodes is None for c in car)
    assert {0, 7, 9} <= set(c.start for c in car)
    assert {1, 64, 65} <= set(c.tracks.shape[1] for c in car) and 1 in set(c.tracks.shape[0] for c in car)
    assert len(_by_system()) >= 2


@pytest.mark.parametrize("system", sorted(_by_system()))
def test_every_case_of_a_system_in_one_call(system):
    cases = _by_system()[system]
    engines = [_engine(c.tree) for c in cases]
    fps = [e.footprint() for e in engines]
    members = [(c.tracks, c.radii, c.start, c.tree.H, c.tries, c.nodes) for c in cases]
    solo = [_solo(e, m) for e, m in zip(engines, members)]
    for order in (list(range(len(cases))), list(range(len(cases)))[::-1]):
        got = _multi([engines[k] for k in order], [members[k] for k in order])
        for k, g in zip(order, got):
            ref = cases[k].reference()
            _same(g, solo[k])
            _same(g, (ref["stats"], ref["chain"], ref["first"], ref["dwell_first"]))
        short = _multi([engines[k] for k in order], [members[k] for k in order], per_node=False)
        assert short == [(g[0], g[1]) for g in got]
    assert [e.footprint() for e in engines] == fps
    for e in engines:
        e.close()


# ------------------------------------------------------------------------------------------------ 2: chunk edges

def _edge_tracks(c):
    """The track of "last row of the last edge" -- it touches rows of chains only, so every `first` is all -1 whatever the start --
    and three discs more, each on the last row of a leaf of the tree at the instant that row is reached with start = 0, 5 and 10:
    members with those starts get conflicts of their own, so that the per-node answers differ among the members of a call."""
    car = c.tree
    cum = ccr.plain(car)["cum"]
    kids = np.bincount(car.pID[1:], minlength=car.size)
    leaves = [v for v in range(1, 200) if kids[v] == 0][3:12:3]
    cols = [c.tracks[:, 0]]
    for v, s in zip(leaves, (0, 5, 10)):
        cols.append(ccr.instant(len(c.tracks), int(cum[v]) - 1 + s, car.touch(car.xedge[v, car.elen[v] - 1])))
    return np.ascontiguousarray(np.stack(cols, axis=1))


def _edge_member(c, tracks, k):
    """Member k of the chunk-edge calls: its own start, tries and id list (None, a list, the empty list)."""
    N = c.tree.size
    nodes = (None, list(range(k % 7, N, 3)), [])[k % 3]
    return (tracks, 0.3, (5 * k) % 23, c.tree.H, (8, 2, 1, 8, 8)[k % 5], nodes)


@pytest.fixture(scope="module")
def edge_fleet():
    c = ccr.case("last row of the last edge")
    engines = [_engine(c.tree) for _ in range(33)]
    tracks = _edge_tracks(c)
    members = [_edge_member(c, tracks, k) for k in range(33)]
    solo = [_solo(e, m) for e, m in zip(engines, members)]
    yield engines, members, solo
    for e in engines:
        e.close()


def test_the_solo_answers_of_the_chunk_edge_members_differ(edge_fleet):
    _, members, solo = edge_fleet
    assert len(set(s[2].tobytes() for s in solo)) > 2
    assert any(s[1]["chain_from"] >= 0 for s in solo) and any(s[1]["chain_from"] < 0 for s in solo)
    assert any(m[5] == [] for m in members[1:31]) and any(m[5] is None for m in members) and any(m[5] for m in members)
    assert members[31][2:] != members[32][2:] and solo[31][:2] != solo[32][:2]
    for m, s in zip(members, solo):
        if m[5] == []:
            assert s[1] == dict(NO_CHAIN, clear_candidates=0) and s[0]["size"] == len(s[2])     # the full clearance answer, no chain


@pytest.mark.parametrize("n", [1, 32, 33])
def test_chunk_edges(edge_fleet, n):
    engines, members, solo = edge_fleet
    assert members[1][5] is not None and members[2][5] == []                      # (n = 32, 33: an empty list strictly inside the call)
    got = _multi(engines[:n], members[:n])
    for g, s in zip(got, solo[:n]):
        _same(g, s)
    if n == 33:                                                                   # ... and with an empty list first and last in a chunk
        order = [2] + [k for k in range(33) if k not in (2, 29, 32)] + [32, 29]    # (... the second chunk: one member without candidates)
        assert len(order) == 33 and members[order[0]][5] == [] and members[order[31]][5] == [] and members[order[32]][5] == []
        got = _multi([engines[k] for k in order], [members[k] for k in order])
        for k, g in zip(order, got):
            _same(g, solo[k])


# ------------------------------------------------------------------------------------------------ 3: the largest LDS sizes the launch

def test_the_largest_lds_of_the_members_sizes_the_launch():
    big_s, H, size = _system("ros_boat")                                          # 3 073 hull points: og_lds == 0
    small_s, _ = cr.case("ros_boat")
    assert 2 * 8 * np.asarray(big_s.vps).size // 2 > 48 * 1024 > 2 * 8 * np.asarray(small_s.vps).size // 2
    big, small = _grow(big_s, H, size), _grow(small_s, H, size, seed=2)
    assert size <= big.size <= size + 1 and size <= small.size <= size + 1
    members = []
    for eng in (big, small):
        state, _, pID, elen, xedge, _ = rr.engine_arrays(eng)
        cum = np.zeros(len(pID), dtype=np.int64)
        cum[0] = elen[0]
        for u in range(1, len(pID)):
            cum[u] = cum[pID[u]] + elen[u]
        v = len(pID) // 2
        L = int(cum.max()) + 9 * H
        disc = ccr.instant(L, int(cum[v]) - 1, xedge[v, elen[v] - 1, :2])        # on node v's last row when the vehicle is there
        members.append((np.stack((disc, ccr.far(L, 1)[:, 0]), axis=1), 1.0, 0, H, 8, None))
    solo = [_solo(big, members[0]), _solo(small, members[1])]
    print([s[:2] for s in solo])
    assert all(s[0]["conflicts"] >= 1 and s[1]["clear_candidates"] >= 1 for s in solo)
    for order in ((0, 1), (1, 0)):
        got = _multi([(big, small)[k] for k in order], [members[k] for k in order])
        for k, g in zip(order, got):
            _same(g, solo[k])
    big.close()
    small.close()


# ------------------------------------------------------------------------------------------------ 4, 5: shared tables, repeated ids

def test_members_that_share_a_table():
    c = ccr.case("last row of the last edge")
    engines = [_engine(c.tree) for _ in range(5)]
    tracks = _edge_tracks(c)
    radii = np.full(tracks.shape[1], 0.3)
    other = tracks.copy()
    other[:, 0] = np.roll(other[:, 0], 3, axis=0)                                 # the disc on the chain arrives three instants later
    starts = [0, 5, 0, 10, 2]
    tabs = [tracks, tracks, other, tracks, tracks]
    members = [(tabs[k], radii, starts[k], c.tree.H, 8, None) for k in range(5)]
    solo = [_solo(e, m) for e, m in zip(engines, members)]
    assert len(set(s[2].tobytes() for s in solo)) >= 3                            # the starts and the changed copy make different answers
    got = _multi(engines, members)
    for g, s in zip(got, solo):
        _same(g, s)
    for e in engines:
        e.close()


def test_an_id_list_with_every_id_twice():
    c = ccr.case("last row of the last edge")
    engines = [_engine(c.tree) for _ in range(3)]
    ids = [int(v) for v in np.random.RandomState(5).permutation(c.tree.size)]
    want = c.reference()["chain"]
    members = [(c.tracks, c.radii, c.start, c.tree.H, 8, nodes) for nodes in (ids, ids + ids, None)]
    got = _multi(engines, members)
    assert got[0][1] == want == got[2][1] and got[1][1] == dict(want, clear_candidates=2 * want["clear_candidates"])
    for e, m, g in zip(engines, members, got):
        _same(g, _solo(e, m))
    for e in engines:
        e.close()


# ------------------------------------------------------------------------------------------------ 6: refusals

def _raw(handles, tracks, radii, L, D, start, H, tries, ids=None, counts=None, sizes=None, chain=True):
    """The native call with sentinel-filled outputs: (rc, message, every output untouched)."""
    from lqrrt_amd import _native as nat
    n = len(handles)
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)
    L, D, start, H, tries = i32(L), i32(D), i32(start), i32(H), i32(tries)
    st, ch = (nat.ClearStats * n)(), (nat.ClearConnectStats * n)()
    C.memset(st, 0x55, C.sizeof(st))
    C.memset(ch, 0x55, C.sizeof(ch))
    sizes = [1] * n if sizes is None else sizes
    first, dwell = [np.full(s, 77, dtype=np.int32) for s in sizes], [np.full(s, 77, dtype=np.int32) for s in sizes]
    ptrs = lambda arrays: (C.c_void_p * n)(*[None if a is None else a.ctypes.data for a in arrays])
    id_ptrs = None if ids is None else ptrs(ids)
    cnt = None if counts is None else i32(counts)
    rc = nat.lib().lqrrt_tree_clear_connect_multi((C.c_void_p * n)(*handles), n, ptrs(tracks), ptrs(radii), nat.ptr(L), nat.ptr(D), nat.ptr(start),
                                                  nat.ptr(H), nat.ptr(tries), id_ptrs, None if cnt is None else nat.ptr(cnt), st,
                                                  ch if chain else None, ptrs(first), ptrs(dwell), C.c_void_p(0))
    msg = nat.lib().lqrrt_last_error().decode() if rc else ""
    untouched = bytes(st) == b"\x55" * C.sizeof(st) and bytes(ch) == b"\x55" * C.sizeof(ch) and all(np.all(a == 77) for a in first + dwell)
    return rc, msg, untouched


def test_refusals_in_their_order_name_the_engine_and_write_nothing():
    from lqrrt_amd import _native as nat
    c = ccr.case("far discs")
    engines = [_engine(c.tree) for _ in range(3)]
    H, N = c.tree.H, c.tree.size
    tr, ra = np.ascontiguousarray(c.tracks), np.ascontiguousarray(c.radii)
    L, D = tr.shape[:2]
    outside, inside = np.array([0, N], dtype=np.int32), np.array([0, 1], dtype=np.int32)

    def call(n=3, **kw):
        """Every member as "far discs" takes it, but for kw: name=(member, value)."""
        a = dict(tracks=[tr] * n, radii=[ra] * n, L=[L] * n, D=[D] * n, start=[0] * n, H=[H] * n, tries=[8] * n, ids=[None] * n, counts=[0] * n)
        for name, (k, value) in kw.items():
            a[name] = list(a[name])
            a[name][k] = value
        return _raw([e.h for e in engines[:n]], a["tracks"], a["radii"], a["L"], a["D"], a["start"], a["H"], a["tries"], a["ids"], a["counts"], [N] * n)
    rc, msg, untouched = call()
    assert rc == 0 and not untouched
    alone = [(dict(start=(1, -1)), "start"), (dict(L=(1, 0)), "L >= 1"), (dict(tries=(1, 0)), "goal_tries"), (dict(H=(1, 0)), "horizon"),
             (dict(H=(1, 10 ** 6)), "horizon"), (dict(ids=(1, inside), counts=(1, -1)), "negative"),
             (dict(ids=(1, outside), counts=(1, 2)), "outside the tree")]
    for kw, word in alone:
        rc, msg, untouched = call(**kw)
        assert rc == nat.E_ARG and word in msg and "(engine 1)" in msg and msg.count("(engine") == 1 and untouched, (kw, msg)
    # two faults: within a member the solo call's order, and across members the earlier engine
    for kw, word, who in ((dict(start=(1, -1), tries=(1, 0)), "start", 1), (dict(tries=(1, 0), H=(1, 0)), "goal_tries", 1),
                          (dict(H=(1, 0), ids=(1, outside), counts=(1, 2)), "horizon", 1), (dict(tries=(2, 0), start=(1, -1)), "start", 1),
                          (dict(start=(2, -1), ids=(1, outside), counts=(1, 2)), "outside the tree", 1), (dict(tries=(0, 0), start=(1, -1)), "goal_tries", 0)):
        rc, msg, untouched = call(**kw)
        assert rc == nat.E_ARG and word in msg and "(engine %d)" % who in msg and untouched, (kw, msg)
    # an id list without the counts; a null chain; no engines
    rc, msg, untouched = _raw([e.h for e in engines], [tr] * 3, [ra] * 3, [L] * 3, [D] * 3, [0] * 3, [H] * 3, [8] * 3, [None, inside, None], None, [N] * 3)
    assert rc == nat.E_ARG and "without its count" in msg and "(engine 1)" in msg and untouched
    rc, msg, untouched = _raw([e.h for e in engines], [tr] * 3, [ra] * 3, [L] * 3, [D] * 3, [0] * 3, [H] * 3, [8] * 3, sizes=[N] * 3, chain=False)
    assert rc == nat.E_ARG and "null" in msg and untouched
    assert nat.lib().lqrrt_tree_clear_connect_multi(None, 0, *([None] * 13), C.c_void_p(0)) == nat.E_ARG
    # the engine list: an engine twice, 129 engines
    rc, msg, untouched = _raw([engines[0].h, engines[1].h, engines[0].h], [tr] * 3, [ra] * 3, [L] * 3, [D] * 3, [0] * 3, [H] * 3, [8] * 3, sizes=[N] * 3)
    assert rc == nat.E_ARG and "engine 2 appears twice" in msg and untouched
    rc, msg, untouched = _raw([engines[0].h] * 129, [tr] * 129, [ra] * 129, [L] * 129, [D] * 129, [0] * 129, [H] * 129, [8] * 129)
    assert rc == nat.E_ARG and "at most 128" in msg and untouched
    rc, msg, untouched = call()
    assert rc == 0 and not untouched
    for e in engines:
        e.close()


def test_the_lds_limit_of_one_member_is_refused_last_and_names_it():
    import lqrrt_amd
    import torch
    from lqrrt_amd.engine import Engine
    c = cl.case("fork, the disc crosses the short branch")
    limit = int(torch.cuda.get_device_properties(0).shared_memory_per_block)
    engines = []
    for k in range(3):
        s = lqrrt_amd.systems.BoatIntermediate(0)
        if k == 1:
            s.vps = np.random.RandomState(0).uniform(-1, 1, (2, limit // 16 - 1))   # 16 V fits the clearance check alone, not the search
        s.set_obstacles(np.zeros((0, 3)))
        engines.append(_load(s, c.tree, cl.H_HAND, goal=c.tree.goal, goal_buffer=c.tree.goal_buffer))
    n = [3] * 3
    args = ([c.tracks] * 3, [c.radii] * 3, [0] * 3, [cl.H_HAND] * 3)
    assert [g["size"] for g in Engine.tree_clear_multi(engines, *args[:3])] == [c.tree.size] * 3
    with pytest.raises(ValueError, match=r"LDS.*\(engine 1\)"):
        Engine.tree_clear_connect_multi(engines, *args)
    with pytest.raises(ValueError, match=r"goal_tries.*\(engine 1\)"):
        Engine.tree_clear_connect_multi(engines, *args, tries=[8, 0, 8])         # (an earlier refusal of the member answers first)
    with pytest.raises(ValueError, match=r"start.*\(engine 0\)"):
        Engine.tree_clear_connect_multi(engines, args[0], args[1], [2 ** 31 - 2, 0, 0], args[3])     # (... and an earlier member's)
    got = Engine.tree_clear_connect_multi([engines[0], engines[2]], *[a[:2] for a in args])
    assert got == [engines[0].tree_clear_connect(c.tracks, c.radii, 0, cl.H_HAND)] * 2
    for e in engines:
        e.close()


def test_wrong_kinds_of_engine():
    import lqrrt_amd
    from lqrrt_amd import _native as nat
    from lqrrt_amd.engine import Engine, NodeTable
    s = lqrrt_amd.systems.DoublePendulum()
    e = Engine(s, capacity=64, max_wave=64)
    e.set_resolution(0.1, 0.0, 4, np.ones(s.nstates), s.goal, np.abs(np.asarray(s.goal_buffer, dtype=np.float64)))
    e.tree_reset(s.x0)
    tracks, radii = np.zeros((2, 1, 2)), np.array([0.5])
    with pytest.raises(nat.NativeError) as ex:
        Engine.tree_clear_connect_multi([e], [tracks], [radii], [0], [4])
    assert ex.value.code == nat.E_STATE and "circle" in str(ex.value) and "(engine 0)" in str(ex.value)
    # mixed models: a car next to it
    c = ccr.case("far discs")
    car = _engine(c.tree)
    with pytest.raises(ValueError, match="share the device and the model"):
        Engine.tree_clear_connect_multi([car, e], [c.tracks, tracks], [c.radii, radii], [0, 0], [c.tree.H, 4])
    e.close()
    car.close()
    table = NodeTable(3, 1, capacity=64)
    rc, msg, untouched = _raw([table.h], [tracks], [radii], [2], [1], [0], [4], [8])
    assert rc == nat.E_STATE and "GENERIC" in msg and untouched
    table.close()


# ------------------------------------------------------------------------------------------------ 7: nothing is written

def test_nothing_of_any_tree_is_written_and_the_trees_grow_on_as_their_twins():
    s, H, _ = _system("boat_advanced")
    size = 300
    engines, twins = [_grow(s, H, size, seed=k + 1) for k in range(2)], [_grow(s, H, size, seed=k + 1) for k in range(2)]
    before = [rr.engine_arrays(e) for e in engines]
    kept = [(e.ignored(), e.plan_best(), e.footprint(), e.counters().as_dict(), e.get_mt19937()) for e in engines]
    members = [(ccr.cross_hits(_tree_of(s, e, H), extra=9 * H), 0.3, 0, H, 8, None) for e in engines]
    got = _multi(engines, members, per_node=False)
    assert [g[0]["size"] for g in got] == [e.size for e in engines]
    for e, b, (ign, best, fp, counters, mt) in zip(engines, before, kept):
        for x, y in zip(b, rr.engine_arrays(e)):
            np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(e.ignored(), ign)
        assert e.plan_best() == best and e.footprint() == fp and e.counters().as_dict() == counters
        key, pos = e.get_mt19937()
        assert pos == mt[1] and np.array_equal(key, mt[0])
    for e, twin in zip(engines, twins):
        for x in (e, twin):
            x.extend(WAVE, node_limit=size + 300)
        assert e.size == twin.size >= size + 300
        (sa, Ka, pa, la, xa, ua), (sb, Kb, pb, lb, xb, ub) = rr.engine_arrays(e), rr.engine_arrays(twin)
        for x, y in ((sa, sb), (Ka, Kb), (pa, pb), (la, lb)):
            np.testing.assert_array_equal(x, y)
        live = np.arange(xa.shape[1])[None, :] < la[:, None]
        np.testing.assert_array_equal(xa[live], xb[live])
        np.testing.assert_array_equal(ua[live], ub[live])
        assert e.plan_best() == twin.plan_best()
    for e in engines + twins:
        e.close()


# ------------------------------------------------------------------------------------------------ 8, 9: the planners

def _no_tree_planner():
    import lqrrt_amd
    s = lqrrt_amd.systems.Car(0)
    cons = lqrrt_amd.Constraints(s.nstates, s.ncontrols, s.goal_buffer, s.is_feasible)
    return lqrrt_amd.Planner(s.dynamics, s.lqr, cons, error_tol=s.error_tol, erf=s.erf, goal0=s.goal, printing=False, **dict(s.plan_kwargs))


def _fleet():
    """Car planners and their tracks: two with every hit crossed, one with far traffic, one without a tree on the device, one at
    capacity whose hits are crossed but the one that arrives last."""
    from test_connect_gpu import _fill
    planners, tracks = [], []
    for seed in (1, 2):
        s, p = _car_planner(300, seed=seed, min_time=2, max_time=3, sys_time=lambda: 0.0)
        assert p.plan_reached_goal
        planners.append(p)
        tracks.append(ccr.cross_hits(_tree_of(s, p._engine, p.horizon_iters), extra=9 * p.horizon_iters))
    s, p = _car_planner(300, seed=3, min_time=2, max_time=3, sys_time=lambda: 0.0)
    planners.append(p)
    tracks.append(ccr.far(len(tracks[0]), 2))
    planners.append(_no_tree_planner())
    tracks.append(ccr.far(4, 1))
    s, p = _car_planner(300, min_time=2, max_time=3, sys_time=lambda: 0.0)
    tree = _tree_of(s, p._engine, p.horizon_iters)
    res = ccr.plain(tree)
    hits = np.flatnonzero(res["hit"])
    keep = int(hits[np.argmax(res["cum"][hits])])
    L = int(res["cum"].max()) + 9 * p.horizon_iters
    tracks.append(np.stack([ccr.instant(L, int(res["cum"][h]) - 1, tree.touch(tree.xedge[h, tree.elen[h] - 1])) for h in hits if h != keep], axis=1))
    _fill(p._engine, s.x0, p._engine.gains(0, 1)[0])
    planners.append(p)
    return planners, tracks


def _state(p):
    if getattr(p, "node_seq", None) is None:
        return None
    return (list(p.node_seq), np.asarray(p.x_seq).tobytes(), np.asarray(p.u_seq).tobytes(), p.plan_wait, p.plan_reached_goal, p.T,
            p._engine.size, p.tree.size)


def test_avoids_connect_is_the_loop_of_avoid_connect(monkeypatch):
    import lqrrt_amd
    from lqrrt_amd.engine import Engine
    (fleet, tracks), (twins, _) = _fleet(), _fleet()
    n = len(fleet)
    radii = [0.3] * n
    assert [_state(p) for p in fleet] == [_state(p) for p in twins]
    calls = dict(query=0, commit=0, solo=0)

    def counted(name, key):
        real = getattr(Engine, name)

        def wrapper(*a, **kw):
            calls[key] += 1
            return real(*a, **kw)
        monkeypatch.setattr(Engine, name, staticmethod(wrapper))
    counted("tree_clear_connect_multi", "query")
    counted("connect_commit_multi", "commit")
    sizes = [p._engine.size if p._engine is not None and p.tree is not None else None for p in fleet]
    # adopt=False: the answers, nothing committed
    got = lqrrt_amd.avoids(fleet, tracks, radii, adopt=False, connect=8)
    want = [p.avoid(t, 0.3, adopt=False, connect=8) for p, t in zip(twins, tracks)]
    assert got == want and calls == dict(query=1, commit=0, solo=0)
    assert [_state(p) for p in fleet] == [_state(p) for p in twins]
    assert [p._engine.size if s is not None else None for p, s in zip(fleet, sizes)] == sizes
    assert got[3] is None and got[0]["chain_from"] >= 0 and got[1]["chain_from"] >= 0 and not any(g["chain_committed"] for g in got if g)
    # connect = 0: today's avoids, its calls and its dicts
    got = lqrrt_amd.avoids(fleet, tracks, radii, connect=0)
    want = lqrrt_amd.avoids(twins, tracks, radii)
    assert got == want and all("chain_from" not in g for g in got if g) and calls == dict(query=1, commit=0, solo=0)
    assert [_state(p) for p in fleet] == [_state(p) for p in twins]
    # connect = 8 with per-planner tracks: one query and one commit for the group
    got = lqrrt_amd.avoids(fleet, tracks, radii, connect=8)
    assert calls == dict(query=2, commit=1, solo=0)
    want = [p.avoid(t, 0.3, connect=8) for p, t in zip(twins, tracks)]
    print(got)
    assert got == want and [list(g) for g in got if g] == [list(w) for w in want if w]
    assert [_state(p) for p in fleet] == [_state(p) for p in twins]
    assert got[0]["chain_committed"] and got[1]["chain_committed"] and got[0]["clear_hits"] == 0       # every hit crossed: a chain wins
    # far traffic: every hit is clear -- and on this tree a chain still arrives strictly earlier than the best of them
    assert got[2]["clear_hits"] == got[2]["hits"] >= 1 and got[2]["best_end"] >= 0 and got[2]["plan_first"] is None
    assert got[2]["chain_committed"] == (got[2]["chain_from"] >= 0) and fleet[2].plan_reached_goal
    assert got[3] is None
    assert got[4]["chain_from"] >= 0 and got[4]["chain_committed"] is False and got[4]["best_end"] >= 0     # at capacity
    assert fleet[4].node_seq == fleet[4]._engine.climb(got[4]["best_end"]) and fleet[4]._engine.size == sizes[4]
    for k in (0, 1):
        assert fleet[k]._engine.size > sizes[k] and fleet[k].plan_wait == 0 and fleet[k].plan_reached_goal
        assert fleet[k].node_seq[-1] == fleet[k]._engine.size - 1
    # shared tracks, on the trees as they are now
    got = lqrrt_amd.avoids(fleet, tracks[0], 0.3, connect=8)
    want = [p.avoid(tracks[0], 0.3, connect=8) for p in twins]
    assert got == want and calls["query"] == 3 and calls["commit"] <= 2
    assert [_state(p) for p in fleet] == [_state(p) for p in twins]
    # vehicle 0 again against its crossing traffic: the chain it committed is now its best clear hit, and no chain beats it
    assert got[0]["chain_from"] == -1 and not got[0]["chain_committed"] and got[0]["clear_hits"] == 1
    assert got[0]["best_end"] == fleet[0].node_seq[-1] and got[0]["plan_first"] is None


def test_deconflict_connect_is_the_loop_of_avoid_connect():
    import lqrrt_amd

    def trio():
        s, p1, tree, tracks = _planner_with_crossed_hits()
        _, p0 = _car_planner(300, seed=2, min_time=2, max_time=3, sys_time=lambda: 0.0)
        _, p2 = _car_planner(300, seed=3, min_time=2, max_time=3, sys_time=lambda: 0.0)
        # the first of the order as ONE disc that is on each of p1's goal hits when that hit arrives, and far away otherwise
        rows = np.tile(np.array([ccr.FAR[0], ccr.FAR[1], 0.0, 0.0, 0.0]), (len(tracks), 1))
        for d in range(tracks.shape[1]):
            at = np.flatnonzero(tracks[:, d, 0] != ccr.FAR[0])
            rows[at, :2] = tracks[at, d]
        p0.x_seq = [r for r in rows]
        return [p0, p1, p2]
    fleet, twins = trio(), trio()
    got = lqrrt_amd.deconflict(fleet, 0.3, connect=8)
    want = [None]
    for at in (1, 2):
        before = [np.asarray(twins[j].x_seq, dtype=np.float64)[:, :2] for j in range(at)]
        want.append(twins[at].avoid(before, np.full(at, 0.3), 0, connect=8))
    print(got)
    assert got == want and got[0] is None
    assert [_state(p) for p in fleet[1:]] == [_state(p) for p in twins[1:]]
    # p1 adopted a chain, and its rows are the track p2 was asked against
    assert got[1]["chain_committed"] and fleet[1].node_seq[-1] == fleet[1]._engine.size - 1 and got[2] is not None
    assert np.array_equal(np.asarray(fleet[1].x_seq), np.asarray(twins[1].x_seq)) and len(fleet[1].x_seq) == got[1]["chain_cost"]
    with pytest.raises(ValueError, match="batched"):
        lqrrt_amd.deconflict(fleet, 0.3, connect=8, batched=True)


# ------------------------------------------------------------------------------------------------ 10: the example

def test_example_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "fleet_clear_connect_gpu.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    assert "adopted a chain" in out.stdout and "kept its best clear hit" in out.stdout and "one query, one commit" in out.stdout
