"""
The batched tree retention (csrc/retain.hpp k_retain_*_multi through lqrrt_tree_retain_multi, Engine.tree_retain_multi): several
trees re-rooted, re-validated and compacted by ONE native call.  Per tree the result is the rule's (tests/retain_reference.py,
NumPy + the C oracle's feasibility test) and the solo call's (Engine.tree_retain on an identically grown twin), BIT FOR BIT:
stats, id map, states, gains, parents, edge lengths, every live edge row, ignore flags, goal bookkeeping -- and so is what the
trees grow into afterwards.  Recipe and helpers: tests/test_retain_gpu.py.
"""
import numpy as np
import pytest

import retain_reference as rr
from test_retain_gpu import WAVE, _engine, _oracle, _other_world, _seed

pytestmark = pytest.mark.gpu


def _grow(s, nodes, seed, extra=0, wave=WAVE, horizon=None):
    eng = _engine(s, nodes + extra + 2 * wave + 8, wave=wave, horizon=horizon, seed=seed)
    eng.tree_reset(s.x0)
    eng.extend(wave, max_attempts=60 * nodes, node_limit=nodes)
    return eng


def _path(eng):
    """The best plan, or without one the path to the last node."""
    end = eng.plan_best()[0]
    return eng.climb(end if end >= 0 else eng.size - 1)


def _same_tree(a, b):
    """Two engines hold the same tree, bit for bit."""
    assert a.size == b.size
    np.testing.assert_array_equal(a.states(), b.states())
    np.testing.assert_array_equal(a.gains(), b.gains())
    np.testing.assert_array_equal(a.parents(), b.parents())
    xa, ua, la = a.edges()
    xb, ub, lb = b.edges()
    np.testing.assert_array_equal(la, lb)
    live = np.arange(xa.shape[1])[None, :] < la[:, None]
    np.testing.assert_array_equal(xa[live], xb[live])
    np.testing.assert_array_equal(ua[live], ub[live])
    np.testing.assert_array_equal(a.ignored(), b.ignored())
    assert a.plan_best() == b.plan_best()


def _snapshot(eng):
    return rr.engine_arrays(eng) + (eng.ignored(), eng.plan_best())


def _unchanged(eng, snap):
    now = _snapshot(eng)
    for a, b in zip(now[:6], snap[:6]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(now[6], snap[6])
    assert now[7] == snap[7]


def _check_against_reference(eng, ref, stats, old_to_new):
    """What tests/test_retain_gpu.py _retain_and_compare checks after the device call."""
    assert stats == ref["stats"]
    np.testing.assert_array_equal(old_to_new, ref["old_to_new"])
    assert eng.size == ref["stats"]["kept"]
    np.testing.assert_array_equal(eng.states(), ref["state"])
    np.testing.assert_array_equal(eng.gains(), ref["K"])
    np.testing.assert_array_equal(eng.parents(), ref["pID"])
    xe, ue, ln = eng.edges()
    np.testing.assert_array_equal(ln, ref["elen"])
    live = np.arange(xe.shape[1])[None, :] < ln[:, None]
    np.testing.assert_array_equal(xe[live], ref["xedge"][live])
    np.testing.assert_array_equal(ue[live], ref["uedge"][live])
    np.testing.assert_array_equal(eng.ignored(), ref["ignored"])
    assert eng.plan_best() == (ref["stats"]["best_end"], ref["stats"]["best_steps"], ref["stats"]["goal_hits"])
    assert eng.climb(max(ref["stats"]["best_end"], 0))[0] == 0                   # the host mirror of the parents follows
    x, u = eng.edge(0)
    assert len(x) == 1 and np.array_equal(x[0], ref["state"][0]) and not u.any()


def _retain_multi_and_compare(engines, systems, roots, flags, oracles=None):
    """References from every engine's pre-call arrays, ONE batched call, everything compared.  Returns the references."""
    from lqrrt_amd.engine import Engine
    refs = []
    for k, (eng, s, root, flag) in enumerate(zip(engines, systems, roots, np.broadcast_to(flags, (len(engines),)))):
        o = oracles[k] if oracles is not None else _oracle(s, 16, 1)
        lo, hi = rr.goal_box(s)
        refs.append(rr.retain(*rr.engine_arrays(eng), root, o.feasible if flag else None, lo, hi))
    generations = [eng.generation for eng in engines]
    done = Engine.tree_retain_multi(engines, roots, flags)
    assert len(done) == len(engines)
    for eng, ref, (stats, old_to_new), gen in zip(engines, refs, done, generations):
        print("retain_multi: %s" % stats)
        _check_against_reference(eng, ref, stats, old_to_new)
        assert eng.generation == gen + 1
    return refs


def _add_circle(s, eng, at, dx, radius):
    p = eng.states(int(at), 1)[0]
    s.set_obstacles(np.vstack((np.asarray(s.obs, dtype=np.float64).reshape(-1, 3), [p[0] + dx, p[1], radius])))


def test_batched_retain_is_the_reference_and_the_solo_call_then_growth():
    """Six boat_advanced trees of different seeds and sizes, each with its own root, its own new obstacle and its own
    revalidate flag, through one call; twins through tree_retain one by one; then everybody grows on (extend_multi / extend)."""
    import lqrrt_amd
    from lqrrt_amd.engine import Engine
    specs = [(1, 3000, True), (2, 1700, False), (3, 2400, True), (4, 900, True), (5, 3300, False), (6, 1300, True)]
    more = 1200
    fleet, twins = [], []
    for seed, nodes, _ in specs:
        for group in (fleet, twins):
            s = lqrrt_amd.systems.BoatAdvanced(0)
            group.append((s, _grow(s, nodes, seed, extra=more)))
    roots, flags = [], []
    for k, ((s, eng), (s2, twin), (seed, nodes, flag)) in enumerate(zip(fleet, twins, specs)):
        assert eng.size == twin.size == nodes + 1
        path = _path(eng)
        roots.append(int(path[max(1, len(path) // 5)]) if k != 3 else 0)        # (one engine keeps its root: only revalidation cuts)
        flags.append(flag)
        for sys_, e in ((s, eng), (s2, twin)):                                   # every boat's map changes in its own way
            _add_circle(sys_, e, path[len(path) // 2], 3.0 + 0.5 * k, 0.8 + 0.2 * k)
            assert e.sync_geometry()
    engines, systems = [e for _, e in fleet], [s for s, _ in fleet]
    footprints = [e.footprint() for e in engines]
    refs = _retain_multi_and_compare(engines, systems, roots, flags)
    assert [e.footprint() for e in engines] == footprints                        # all scratch is transient
    kept = [r["stats"]["kept"] for r in refs]
    assert all(1 < k_ <= n + 1 for k_, (_, n, _) in zip(kept, specs)), kept
    assert any(r["stats"]["infeasible"] > 0 for r, f in zip(refs, flags) if f)
    assert all(r["stats"]["infeasible"] == 0 and r["stats"]["orphaned"] == 0 for r, f in zip(refs, flags) if not f)
    # the solo call on the twins
    for (_, eng), (_, twin), root, flag, ref in zip(fleet, twins, roots, flags, refs):
        stats, old_to_new = twin.tree_retain(root, revalidate=flag)
        assert stats == ref["stats"]
        np.testing.assert_array_equal(old_to_new, ref["old_to_new"])
        _same_tree(eng, twin)
    # growth from the kept trees: shared launches against one engine at a time
    for k, ((_, eng), (_, twin)) in enumerate(zip(fleet, twins)):
        _seed(eng, 40 + k)
        _seed(twin, 40 + k)
    sts = Engine.extend_multi(engines, WAVE, max_attempts=more)
    for (_, eng), (_, twin), st, k0 in zip(fleet, twins, sts, kept):
        st2 = twin.extend(WAVE, max_attempts=more)
        assert (st.attempts, st.accepted, st.goal_hits) == (st2.attempts, st2.accepted, st2.goal_hits) and st.attempts == more
        assert eng.size == k0 + st.accepted
        _same_tree(eng, twin)
    # ... and a second batched retain of the grown trees, every engine from the middle of its path, all flags swapped
    roots2 = [int(_path(e)[len(_path(e)) // 2]) for e in engines]
    refs2 = _retain_multi_and_compare(engines, systems, roots2, [not f for f in flags])
    for (_, twin), root, flag, ref in zip(twins, roots2, flags, refs2):
        assert twin.tree_retain(root, revalidate=not flag)[0] == ref["stats"]
    for (_, eng), (_, twin) in zip(fleet, twins):
        _same_tree(eng, twin)
    for _, e in fleet + twins:
        e.close()


def test_special_cases_keep_their_solo_meaning_in_one_call():
    """A one-node tree, a leaf as root (one node kept), an identity retain (root 0, no revalidation: nothing moves), a tree that
    fills its engine's capacity, and an ordinary one -- one call.  Footprints are unchanged: every buffer is transient."""
    import lqrrt_amd
    from lqrrt_amd import _native as nat
    S = lqrrt_amd.systems.BoatAdvanced
    s_one, s_leaf, s_same, s_full, s_plain = S(0), S(0), S(0), S(0), S(0)
    one = _engine(s_one, 600, seed=1)
    one.tree_reset(s_one.x0)
    leaf = _grow(s_leaf, 700, 2)
    same = _grow(s_same, 1100, 3)
    plain = _grow(s_plain, 1500, 4)
    full = _engine(s_full, 900, wave=64, seed=5)
    full.tree_reset(s_full.x0)
    full.extend(64, node_limit=700)
    x0, K0 = np.ascontiguousarray(s_full.x0, dtype=np.float64), np.ascontiguousarray(full.gains(0, 1)[0])
    while True:
        rc = nat.lib().lqrrt_tree_append(full.h, 0, nat.ptr(x0), nat.ptr(K0), 1, None, None, full._stream())
        if rc == nat.E_CAPACITY:
            break
        nat.check(rc)
    assert full.size >= 900 and one.size == 1
    leaf_id = int(np.setdiff1d(np.arange(leaf.size), leaf.parents())[-1])
    pid = full.parents()
    engines = [one, leaf, same, full, plain]
    systems = [s_one, s_leaf, s_same, s_full, s_plain]
    path = _path(plain)
    _add_circle(s_plain, plain, path[len(path) // 2], 3.0, 1.0)
    assert plain.sync_geometry()
    before_same = _snapshot(same)
    footprints = [e.footprint() for e in engines]
    roots = [0, leaf_id, 0, 0, int(path[max(1, len(path) // 5)])]
    refs = _retain_multi_and_compare(engines, systems, roots, [True, True, False, True, True])
    assert [r["stats"]["kept"] for r in refs[:4]] == [1, 1, same.size, full.size]
    assert one.size == 1 and leaf.size == 1 and 1 < plain.size < 1501
    _unchanged(same, before_same)                                                # the identity retain moved nothing
    assert [e.footprint() for e in engines] == footprints
    # the full tree again, cut this time; the one-node trees once more (the smallest call there is)
    refs = _retain_multi_and_compare([full, one, leaf], [s_full, s_one, s_leaf], [int(pid[pid[600]]) or 1, 0, 0], [True, False, True])
    assert 1 <= refs[0]["stats"]["kept"] < 900 and refs[1]["stats"]["kept"] == refs[2]["stats"]["kept"] == 1
    assert [e.footprint() for e in engines] == footprints
    # every engine still plans: grow them all on together
    from lqrrt_amd.engine import Engine
    for k, e in enumerate(engines):
        _seed(e, 70 + k)
    sizes = [e.size for e in engines]
    Engine.extend_multi([one, same, plain], WAVE, max_attempts=300)
    assert one.size > 1 and same.size > sizes[2] and plain.size > sizes[4]
    for e in engines:
        e.close()


def test_more_engines_than_one_launch_holds():
    """40 small trees in one call: two chunks (32 + 8), every tree against the reference."""
    import lqrrt_amd
    n = 40
    systems = [lqrrt_amd.systems.BoatAdvanced(0) for _ in range(n)]
    engines = [_grow(s, 150 + 9 * k, 100 + k, wave=64) for k, s in enumerate(systems)]
    roots, flags = [], []
    for k, (s, eng) in enumerate(zip(systems, engines)):
        path = _path(eng)
        roots.append(int(path[min(1 + k % 3, len(path) - 1)]) if k % 5 else 0)
        flags.append(k % 4 != 1)
        if k % 2:
            _add_circle(s, eng, path[len(path) // 2], 2.0, 1.0)
            assert eng.sync_geometry()
    refs = _retain_multi_and_compare(engines, systems, roots, flags)
    assert len(set(r["stats"]["kept"] for r in refs)) > 10                        # forty different trees, not forty times one
    for e in engines:
        e.close()


@pytest.mark.parametrize("name", ["double_integrator", "ros_boat"])
def test_other_geometry_kinds(name):
    """Boxes through the CSR grid (double integrator) and an occupancy grid (ROS boat): three trees of the model, two of them in
    a world that changed, one call (the check launch reserves the largest LDS image of the three)."""
    trio = []
    for k in range(3):
        s, nodes, horizon, change = _other_world(name)
        eng = _grow(s, nodes - 250 * k, 3 + k, horizon=horizon)
        assert eng.size > (nodes - 250 * k) // 2, eng.size
        if k != 1:
            change(s, eng)
            assert eng.sync_geometry()
        trio.append((s, eng, horizon))
    engines, systems = [e for _, e, _ in trio], [s for s, _, _ in trio]
    oracles = [_oracle(s, 16, 3, horizon=h) for s, _, h in trio]
    pid = engines[2].parents()
    mid = engines[2].size // 2
    roots = [0, 0, int(pid[pid[mid]]) if pid[mid] > 0 else mid]
    refs = _retain_multi_and_compare(engines, systems, roots, [True, True, True], oracles=oracles)
    assert refs[0]["stats"]["infeasible"] > 0 and refs[1]["stats"]["infeasible"] == 0 and refs[1]["stats"]["kept"] == refs[1]["stats"]["old_size"]
    for e in engines:
        e.close()


def test_bad_arguments_leave_every_tree_as_it_was():
    """A root that does not exist in the LAST engine, an engine listed twice, engines of two models: each is refused with the
    solo call's kind of error before anything is written."""
    import lqrrt_amd
    from lqrrt_amd.engine import Engine
    systems = [lqrrt_amd.systems.BoatAdvanced(0) for _ in range(3)]
    engines = [_grow(s, 400 + 100 * k, 20 + k, wave=64) for k, s in enumerate(systems)]
    car = lqrrt_amd.systems.Car(0)
    other = _grow(car, 300, 30, wave=64)
    snaps = [_snapshot(e) for e in engines + [other]]
    generations = [e.generation for e in engines + [other]]
    with pytest.raises(ValueError, match="doesn't exist"):
        Engine.tree_retain_multi(engines, [5, 7, engines[2].size])
    with pytest.raises(ValueError, match="doesn't exist"):
        Engine.tree_retain_multi(engines, [5, 7, -1])
    with pytest.raises(ValueError, match="twice"):
        Engine.tree_retain_multi([engines[0], engines[1], engines[0]], [5, 7, 9])
    with pytest.raises(ValueError, match="share"):
        Engine.tree_retain_multi(engines + [other], [5, 7, 9, 11])
    with pytest.raises(ValueError):
        Engine.tree_retain_multi(engines, [5, 7])                                 # a root per engine
    for e, snap, gen in zip(engines + [other], snaps, generations):
        _unchanged(e, snap)
        assert e.generation == gen                                               # bound Tree views stay valid
    # the same arguments put right go through
    _retain_multi_and_compare(engines, systems, [5, 7, 9], True)
    for e in engines + [other]:
        e.close()
