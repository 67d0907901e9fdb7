"""
Plan refinement for several engines per call (csrc/refine.hpp k_refine_search_multi / k_refine_commit_multi through
lqrrt_refine_search_multi / lqrrt_refine_commit_multi) against the reference of the rule (tests/refine_reference.py), BIT FOR BIT
and per engine: the winner (cost, i, j) of every round and every appended node's state, gain, parent, edge length and edge rows --
for engines that leave the call at different rounds -- then against engines that run the one-engine calls, at capacity, with bad
arguments and with more engines than one launch takes.
"""
import numpy as np
import pytest

import refine_reference as rr
from test_refine_gpu import _case, _engine, _fill

pytestmark = pytest.mark.gpu


class _Item(object):
    """One engine of a call: the fixture's tree on the device, its Refiner and the plan as it stands."""

    def __init__(self, name, factor=1.0, extra=64, reference=True):
        self.name = name
        self.s, self.g = _case(name)
        self.buf = factor * np.abs(np.asarray(self.s.goal_buffer, dtype=np.float64))
        ref, self.plan = rr.from_fixture(self.s, self.g, goal_buffer=self.buf)
        self.H = ref.H
        self.ref = ref if reference else None
        self.eng = _engine(self.s, self.g, self.buf, extra=extra)
        self.size0 = self.eng.size
        self.log = []

    def cost(self):
        lens = self.eng.edge_lengths()
        return 1 + int(sum(int(lens[p]) for p in self.plan[1:]))


def _check_against_reference(it, ids, ids_ref):
    eng, ref = it.eng, it.ref
    assert ids == ids_ref, it.name
    first, k = ids[0], len(ids)
    assert np.array_equal(eng.states(first, k), np.array([ref.states[v] for v in ids]))
    assert np.array_equal(eng.gains(first, k), np.array([ref.K[v] for v in ids]))
    assert eng.parents(first, k).tolist() == [ref.pID[v] for v in ids]
    assert eng.edge_lengths(first, k).tolist() == [ref.elen[v] for v in ids]
    for v in ids:
        x, u = eng.edge(v)
        assert np.array_equal(x, ref.edges[v][0]) and np.array_equal(u, ref.edges[v][1]), (it.name, v)
    assert eng.climb(it.plan[-1]) == it.plan


def _drive_against_reference(items, max_rounds=8):
    """Batched rounds to the fix-point of every engine; after every round each engine is compared with its Refiner."""
    from lqrrt_amd.engine import Engine
    active = list(items)
    calls = 0
    while active and calls < max_rounds:
        wants = [it.ref.round(it.plan) for it in active]
        got = Engine.refine_round_multi([it.eng for it in active], [it.plan for it in active], [it.H for it in active],
                                        [it.ref.cost(it.plan) for it in active])
        calls += 1
        assert got == [None if w is None else tuple(w[:3]) for w in wants], ([it.name for it in active], calls)
        winners = [(it, w) for it, w in zip(active, wants) if w is not None]
        if not winners:
            break
        new = Engine.refine_commit_multi([it.eng for it, _ in winners], [it.plan for it, _ in winners], [it.H for it, _ in winners],
                                         [(w[1], w[2]) for _, w in winners])
        for (it, w), ids in zip(winners, new):
            it.plan, ids_ref = it.ref.commit(it.plan, w)
            _check_against_reference(it, ids, ids_ref)
            it.log.append(tuple(w[:3]))
        active = [it for it, _ in winners]
    return [it.log for it in items]


# the per-engine sequences are the ones tests/test_refine_gpu.py::test_device_rounds_match_reference pins for the one-engine calls
MIXES = [
    ([("car_500", 1.0), ("car_2000", 1.0)], 8, [[(551, 2, 12), (501, 0, 1), (496, 0, 1)], [(601, 2, 5)]]),
    ([("boat_novice_300", 1.0), ("boat_novice_firstgoal", 1.0)], 8, [[(679, 23, 43), (678, 29, 33)], [(741, 23, 29)]]),
    # 113 plan nodes, 6 328 candidates each: none reaches the narrow goal box, one the wide one (then none)
    ([("boat_advanced_10k", 1.0), ("boat_advanced_10k", 2.0)], 2, [[], [(501, 41, 46)]]),
    # Riccati gains (GainLds in the workgroup); the searched chains hold FPR-cut edges
    ([("boat_novice_lqr_400", 1.0), ("boat_novice_lqr_400", 2.0)], 8, [[(450, 0, 14)], [(390, 0, 14), (387, 18, 19)]]),
    ([("double_integrator_600", 1.0)], 8, [[(41, 0, 18), (38, 0, 1), (36, 0, 1), (21, 0, 1)]]),
    ([("ros_boat", 1.0), ("ros_boat", 1.0)], 8, [[(481, 5, 38), (465, 0, 3), (464, 9, 15)]] * 2),
]


@pytest.mark.parametrize("mix,max_rounds,expect", MIXES, ids=[m[0][0][0] for m in MIXES])
def test_batched_rounds_match_reference(mix, max_rounds, expect):
    items = [_Item(name, factor) for name, factor in mix]
    try:
        assert _drive_against_reference(items, max_rounds) == expect
    finally:
        for it in items:
            it.eng.close()


def _whole_tree(eng, size0):
    new = list(range(size0, eng.size))
    return dict(size=eng.size, states=eng.states(), gains=eng.gains(), parents=eng.parents(), lens=eng.edge_lengths(),
                edges=[eng.edge(v) for v in new])


def _assert_same_tree(a, b, where):
    assert a["size"] == b["size"], where
    for key in ("states", "gains", "parents", "lens"):
        assert np.array_equal(a[key], b[key]), (where, key)
    for (xa, ua), (xb, ub) in zip(a["edges"], b["edges"]):
        assert np.array_equal(xa, xb) and np.array_equal(ua, ub), where


def _solo_to_fix_point(it, max_rounds=8):
    for _ in range(max_rounds):
        win = it.eng.refine_round(it.plan, it.H, it.cost())
        if win is None:
            break
        ids = it.eng.refine_commit(it.plan, it.H, win[1], win[2])
        it.plan = it.plan[:win[1] + 1] + ids
        it.log.append(win)


def _batched_to_fix_point(items, max_rounds=8):
    from lqrrt_amd.engine import Engine
    active = list(items)
    for _ in range(max_rounds):
        if not active:
            break
        wins = Engine.refine_round_multi([it.eng for it in active], [it.plan for it in active], [it.H for it in active],
                                         [it.cost() for it in active])
        winners = [(it, w) for it, w in zip(active, wins) if w is not None]
        if not winners:
            break
        new = Engine.refine_commit_multi([it.eng for it, _ in winners], [it.plan for it, _ in winners], [it.H for it, _ in winners],
                                         [(w[1], w[2]) for _, w in winners])
        for (it, w), ids in zip(winners, new):
            it.plan = it.plan[:w[1] + 1] + ids
            it.log.append(w)
        active = [it for it, _ in winners]


@pytest.mark.parametrize("mix", [[("car_500", 1.0), ("car_2000", 1.0), ("car_500", 2.0)],
                                 [("boat_novice_lqr_400", 1.0), ("boat_novice_lqr_400", 2.0)],
                                 [("ros_boat", 1.0), ("ros_boat", 2.0)]], ids=["car", "boat_novice_lqr", "ros_boat"])
def test_batched_rounds_match_one_engine_calls(mix):
    """Twins: the same fixtures in two sets of engines, one refined through the batched calls, the other engine by engine."""
    fleet = [_Item(name, factor, reference=False) for name, factor in mix]
    twins = [_Item(name, factor, reference=False) for name, factor in mix]
    try:
        _batched_to_fix_point(fleet)
        for t in twins:
            _solo_to_fix_point(t)
        assert any(t.log for t in twins)
        for a, b in zip(fleet, twins):
            assert a.log == b.log and a.plan == b.plan, a.name
            _assert_same_tree(_whole_tree(a.eng, a.size0), _whole_tree(b.eng, b.size0), a.name)
            assert a.eng.climb(a.plan[-1]) == a.plan
    finally:
        for it in fleet + twins:
            it.eng.close()


def test_batched_commit_capacity_stop():
    """A full tree among the engines of a call: its count reports LQRRT_E_CAPACITY and it stays as it was; the others commit."""
    from lqrrt_amd import _native as nat
    from lqrrt_amd.engine import Engine
    import ctypes as C
    full_one, other = _Item("car_500", extra=5), _Item("car_2000")
    try:
        full = _fill(full_one.eng, full_one.g["state"][0], full_one.g["K"][0])
        items = [full_one, other]
        wants = [it.ref.round(it.plan) for it in items]
        args = ([it.eng for it in items], [it.plan for it in items], [it.H for it in items])
        assert Engine.refine_round_multi(*args, [it.ref.cost(it.plan) for it in items]) == [tuple(w[:3]) for w in wants]
        # the raw call: counts_out
        n = 2
        plans = [np.ascontiguousarray(it.plan, dtype=np.int32) for it in items]
        handles = (C.c_void_p * n)(*[it.eng.h for it in items])
        plan_ptrs = (C.c_void_p * n)(*[p.ctypes.data for p in plans])
        lens = np.array([len(p) for p in plans], dtype=np.int32)
        tries, hz = np.array([8, 8], dtype=np.int32), np.array([it.H for it in items], dtype=np.int32)
        ci, cj = np.array([w[1] for w in wants], dtype=np.int32), np.array([w[2] for w in wants], dtype=np.int32)
        outs = [np.empty(len(p) + 8, dtype=np.int32) for p in plans]
        out_ptrs = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        caps, counts = np.array([len(o) for o in outs], dtype=np.int32), np.zeros(n, dtype=np.int32)
        rc = nat.lib().lqrrt_refine_commit_multi(handles, n, plan_ptrs, nat.ptr(lens), nat.ptr(tries), nat.ptr(hz), nat.ptr(ci), nat.ptr(cj),
                                                 out_ptrs, nat.ptr(caps), nat.ptr(counts), full_one.eng._stream())
        assert rc == 0
        assert counts[0] == nat.E_CAPACITY and full_one.eng.size == full
        assert full_one.eng.climb(full_one.plan[-1]) == full_one.plan
        ids = outs[1][:counts[1]].tolist()
        other.plan, ids_ref = other.ref.commit(other.plan, wants[1])
        _check_against_reference(other, ids, ids_ref)
        # the full tree still answers the same search, and the Python call reports the stop as None
        assert Engine.refine_round_multi([full_one.eng], [full_one.plan], [full_one.H], [full_one.ref.cost(full_one.plan)]) == [tuple(wants[0][:3])]
        assert Engine.refine_commit_multi([full_one.eng], [full_one.plan], [full_one.H], [(wants[0][1], wants[0][2])]) == [None]
        assert full_one.eng.size == full
    finally:
        full_one.eng.close()
        other.eng.close()


def test_batched_calls_check_every_argument_first():
    from lqrrt_amd.engine import Engine
    a, b, c = _Item("car_500"), _Item("car_2000"), _Item("boat_novice_300")
    items = [a, b, c]
    try:
        sizes = [it.eng.size for it in items]
        prints = [it.eng.footprint() for it in items]
        costs = {it: it.ref.cost(it.plan) for it in items}
        wa = a.ref.round(a.plan)

        def refused(engs, plans, ijs=None):
            hz, inc = [it.H for it in engs], [costs[it] for it in engs]
            with pytest.raises(ValueError):
                Engine.refine_round_multi([it.eng for it in engs], plans, hz, inc)
            with pytest.raises(ValueError):
                Engine.refine_commit_multi([it.eng for it in engs], plans, hz, ijs or [(wa[1], wa[2])] * len(engs))
            assert [it.eng.size for it in items] == sizes and [it.eng.footprint() for it in items] == prints

        refused([a, c], [a.plan, c.plan])                                        # mixed models
        refused([a, b, a], [a.plan, b.plan, a.plan])                             # an engine twice
        refused([a, b], [a.plan, b.plan[1:]])                                    # a plan that does not start at node 0
        refused([a, b], [a.plan, b.plan[:1] + b.plan[2:]])                       # a link that is not parent -> child
        for bad in [(5, len(b.plan)), (3, 3), (-2, 4)]:                          # i / j out of range for one engine
            with pytest.raises(ValueError):
                Engine.refine_commit_multi([a.eng, b.eng], [a.plan, b.plan], [a.H, b.H], [(wa[1], wa[2]), bad])
            assert [it.eng.size for it in items] == sizes and [it.eng.footprint() for it in items] == prints
        with pytest.raises(ValueError):
            Engine.refine_round_multi([a.eng, b.eng], [a.plan, b.plan], [a.H, b.H], [costs[a], 0])      # an incumbent of 0 steps
        assert [it.eng.size for it in items] == sizes and [it.eng.footprint() for it in items] == prints
        # ... and a call that goes through leaves the footprints where they were
        assert _drive_against_reference([a, b])[0][0] == tuple(wa[:3])
        assert a.eng.size > sizes[0] and [it.eng.footprint() for it in items] == prints
    finally:
        for it in items:
            it.eng.close()


def test_more_engines_than_one_launch_takes():
    """40 engines: two chunks (32 + 8).  Every engine gets what one engine alone gets."""
    solo = _Item("car_500", reference=False)
    fleet = [_Item("car_500", reference=False) for _ in range(40)]
    try:
        _solo_to_fix_point(solo)
        assert [tuple(w) for w in solo.log] == [(551, 2, 12), (501, 0, 1), (496, 0, 1)]
        _batched_to_fix_point(fleet)
        want = _whole_tree(solo.eng, solo.size0)
        for k, it in enumerate(fleet):
            assert it.log == solo.log and it.plan == solo.plan, k
            _assert_same_tree(_whole_tree(it.eng, it.size0), want, k)
    finally:
        for it in fleet + [solo]:
            it.eng.close()
