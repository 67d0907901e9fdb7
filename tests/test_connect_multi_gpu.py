"""
Goal connection for several trees per call on the device (csrc/connect.hpp k_connect_search_multi through lqrrt_connect_search_multi /
lqrrt_connect_commit_multi) against the reference of the rule (tests/connect_reference.py, the C oracle's primitives), BIT FOR BIT,
and against the one-tree calls on identically loaded twins.  Every call holds engines of one model, loaded from fixture prefixes.
"""
import functools

import numpy as np
import pytest

import connect_reference as cr
from test_connect_gpu import _engine, _fill, _plan_cost

pytestmark = pytest.mark.gpu

# per call: (fixture, nodes loaded -- None: the whole tree, under its plan's cost --, goal_tries, the winner computed with the reference)
CALLS = {
    "car": [("car_2000", 150, 8, None), ("car_2000", 217, 8, (951, 211)), ("car_2000", 217, 1, None),
            ("car_2000", 400, 1, (1151, 217)), ("car_2000", 1000, 2, (951, 211))],
    "boat_novice": [("boat_novice_300", 60, 8, None), ("boat_novice_300", 107, 8, (781, 77)), ("boat_novice_300", 107, 2, (821, 102)),
                    ("boat_novice_300", 200, 1, (821, 106))],
    # the box grid; the one-node prefix is a one-candidate engine, the smallest slice of the prefix table
    "double_integrator": [("double_integrator_600", 1, 8, (41, 0)), ("double_integrator_600", 1, 1, None),
                          ("double_integrator_600", 5, 1, (81, 3)), ("double_integrator_600", 50, 2, (41, 0))],
    "riccati": [("boat_novice_lqr_400", 60, 8, None), ("boat_novice_lqr_400", 144, 8, (481, 73)), ("boat_novice_lqr_400", 144, 2, (529, 142))],
    # the solo test's cases in one launch
    "boat_advanced": [("boat_advanced_10k", 3308, 8, (1707, 3305)), ("boat_advanced_200", None, 8, None),
                      ("boat_advanced_3000", None, 8, None), ("boat_advanced_10k", None, 8, (1256, 5993))],
}


@functools.lru_cache(maxsize=None)
def _case(name):
    return cr.case(name)


def _incumbent(name, size):
    s, g = _case(name)
    return cr.NO_INCUMBENT if size is not None else _plan_cost(cr.from_fixture(s, g), g)


@functools.lru_cache(maxsize=None)
def _ref_win(name, size, tries, incumbent, nodes=None):
    """The reference's winner (cost, node, edges) or None; computed once per case and left unchanged."""
    s, g = _case(name)
    return cr.from_fixture(s, g, size).search(goal_tries=tries, incumbent=incumbent, nodes=None if nodes is None else list(nodes))


def _load(name, size, extra=64):
    s, g = _case(name)
    return _engine(s, g, size, extra)


def _horizon(name):
    s, g = _case(name)
    return cr.horizon_of(s, g)


def _tree(eng):
    return eng.states(), eng.gains(), eng.parents(), eng.edge_lengths()


def _same_tree(a, b, where=None):
    assert a.size == b.size, where
    for x, y in zip(_tree(a), _tree(b)):
        assert np.array_equal(x, y), where


def _check_commit(eng, name, size, win, ids, where=None):
    """A batched commit against the reference's commit (the assertions of tests/test_connect_gpu.py _compare_commit)."""
    s, g = _case(name)
    ref = cr.from_fixture(s, g, size)
    plan, ids_ref = ref.commit_chain(win)
    assert ids == ids_ref, where
    first, k = ids[0], len(ids)
    assert np.array_equal(eng.states(first, k), np.array([ref.states[v] for v in ids])), where
    assert np.array_equal(eng.gains(first, k), np.array([ref.K[v] for v in ids])), where
    assert eng.parents(first, k).tolist() == [ref.pID[v] for v in ids], where
    assert eng.edge_lengths(first, k).tolist() == [ref.elen[v] for v in ids], where
    for v in ids:
        x, u = eng.edge(v)
        assert np.array_equal(x, ref.edges[v][0]) and np.array_equal(u, ref.edges[v][1]), (where, v)
    assert eng.climb(ids[-1]) == plan and eng.size == ref.size, where


@pytest.mark.parametrize("call", sorted(CALLS))
def test_batched_search_and_commit_match_reference(call):
    from lqrrt_amd.engine import Engine
    rows = CALLS[call]
    incs = [_incumbent(name, size) for name, size, _, _ in rows]
    wants = [_ref_win(name, size, tries, inc) for (name, size, tries, _), inc in zip(rows, incs)]
    print(call, [None if w is None else w[:2] for w in wants])
    assert [None if w is None else (w[0], w[1]) for w in wants] == [row[3] for row in rows]      # the table is the reference's
    engines = [_load(name, size) for name, size, _, _ in rows]
    H = [_horizon(name) for name, _, _, _ in rows]
    tries = [row[2] for row in rows]
    sizes = [e.size for e in engines]
    fp0 = [e.footprint() for e in engines]
    got = Engine.connect_search_multi(engines, H, incs, tries)
    assert got == [row[3] for row in rows]
    new = Engine.connect_commit_multi(engines, [None if w is None else w[1] for w in got], H, tries)
    for k, ((name, size, _, _), w, ids) in enumerate(zip(rows, wants, new)):
        if w is None:
            assert ids == [] and engines[k].size == sizes[k], k
        else:
            _check_commit(engines[k], name, size, w, ids, k)
    # the trees with their new chains: nothing below each winner's cost
    again = Engine.connect_search_multi(engines, H, [inc if w is None else w[0] for inc, w in zip(incs, wants)], tries)
    assert again == [None] * len(rows)
    assert [e.footprint() for e in engines] == fp0                  # the images are scratch, not footprint
    for e in engines:
        e.close()


def test_every_engine_has_its_own_key():
    from lqrrt_amd.engine import Engine
    engines = [_load("car_2000", 217) for _ in range(3)]
    H = [_horizon("car_2000")] * 3
    got = Engine.connect_search_multi(engines, H, [cr.NO_INCUMBENT, 951, 952])
    assert got == [(951, 211), None, (951, 211)]
    for e in engines:
        e.close()


def test_id_lists_per_engine():
    from lqrrt_amd.engine import Engine
    perm = np.random.RandomState(5).permutation(217)
    rest = tuple(int(v) for v in perm if v != 211)
    want = _ref_win("car_2000", 217, 8, cr.NO_INCUMBENT, rest)
    assert want is not None and (want[0], want[1]) != (951, 211)
    engines = [_load("car_2000", 217) for _ in range(4)]
    H = [_horizon("car_2000")] * 4
    got = Engine.connect_search_multi(engines, H, [cr.NO_INCUMBENT] * 4, nodes=[perm, list(rest), [], None])
    assert got == [(951, 211), (want[0], want[1]), None, (951, 211)]
    assert Engine.connect_search_multi(engines, H, [cr.NO_INCUMBENT] * 4, nodes=None) == [(951, 211)] * 4
    assert Engine.connect_search_multi(engines[:2], H[:2], [cr.NO_INCUMBENT] * 2, nodes=[[], []]) == [None, None]
    for e in engines:
        e.close()


def test_batched_calls_equal_the_solo_calls_on_twins():
    """Each engine's result is that of connect_search / connect_commit on an identically loaded twin: the whole tree agrees."""
    from lqrrt_amd.engine import Engine
    rows = CALLS["car"]
    fleet = [_load(name, size) for name, size, _, _ in rows]
    twins = [_load(name, size) for name, size, _, _ in rows]
    H = _horizon("car_2000")
    tries = [row[2] for row in rows]
    got = Engine.connect_search_multi(fleet, [H] * len(rows), [cr.NO_INCUMBENT] * len(rows), tries)
    new = Engine.connect_commit_multi(fleet, [None if w is None else w[1] for w in got], [H] * len(rows), tries)
    for k, (p, q) in enumerate(zip(fleet, twins)):
        solo = q.connect_search(H, cr.NO_INCUMBENT, tries[k])
        assert got[k] == solo, k
        ids = [] if solo is None else q.connect_commit(solo[1], H, tries[k])
        assert new[k] == ids, k
        _same_tree(p, q, k)
        for v in ids:
            (x, u), (y, w) = p.edge(v), q.edge(v)
            assert np.array_equal(x, y) and np.array_equal(u, w), (k, v)
    for e in fleet + twins:
        e.close()


def test_more_engines_than_one_launch_holds():
    """34 engines: two launches (32 + 2).  Every engine's result is its solo result."""
    from lqrrt_amd.engine import Engine
    name = "double_integrator_600"
    H = _horizon(name)
    combos = [(1, 8), (5, 1), (1, 1), (5, 8)]                       # prefixes alternate, and so do the goal tries within each
    table = {(1, 8): (41, 0), (1, 1): None, (5, 1): (81, 3), (5, 8): (41, 0)}
    plan = [combos[k % 4] for k in range(34)]
    engines = [_load(name, size, extra=16) for size, _ in plan]
    twins = {c: _load(name, c[0], extra=16) for c in combos}
    solo = {c: twins[c].connect_search(H, cr.NO_INCUMBENT, c[1]) for c in combos}
    assert solo == table
    for c in combos:
        if solo[c] is not None:
            twins[c].connect_commit(solo[c][1], H, c[1])
    tries = [t for _, t in plan]
    got = Engine.connect_search_multi(engines, [H] * 34, [cr.NO_INCUMBENT] * 34, tries)
    assert got == [solo[c] for c in plan]
    new = Engine.connect_commit_multi(engines, [None if w is None else w[1] for w in got], [H] * 34, tries)
    for k, c in enumerate(plan):
        assert (new[k] == []) == (solo[c] is None), k
        _same_tree(engines[k], twins[c], k)
        for v in new[k]:
            (x, u), (y, w) = engines[k].edge(v), twins[c].edge(v)
            assert np.array_equal(x, y) and np.array_equal(u, w), (k, v)
    for e in engines + list(twins.values()):
        e.close()


def test_a_full_tree_keeps_its_own_while_the_others_commit():
    from lqrrt_amd.engine import Engine
    s, g = _case("car_2000")
    H = [_horizon("car_2000")] * 3
    engines = [_load("car_2000", 217), _load("car_2000", 217, extra=1), _load("car_2000", 217)]     # (the winner's chain has two nodes)
    full = _fill(engines[1], g["state"][0], g["K"][0])
    parents, lens = engines[1].parents(), engines[1].edge_lengths()
    nodes = [None, list(range(217)), None]                          # (the copies of the root that fill the tree are not candidates)
    assert Engine.connect_search_multi(engines, H, [cr.NO_INCUMBENT] * 3, nodes=nodes) == [(951, 211)] * 3
    new = Engine.connect_commit_multi(engines, [211, 211, 211], H)
    assert new[1] is None and engines[1].size == full
    assert np.array_equal(engines[1].parents(), parents) and np.array_equal(engines[1].edge_lengths(), lens)
    win = _ref_win("car_2000", 217, 8, cr.NO_INCUMBENT)
    for k in (0, 2):
        _check_commit(engines[k], "car_2000", 217, win, new[k], k)
    assert Engine.connect_search_multi(engines, H, [cr.NO_INCUMBENT] * 3, nodes=nodes) == [(951, 211)] * 3
    for e in engines:
        e.close()


def test_a_chain_that_misses_the_goal_fails_alone():
    from lqrrt_amd import _native as nat
    from lqrrt_amd.engine import Engine
    s, g = _case("car_2000")
    assert cr.from_fixture(s, g, 217).chain(0) is None              # eight steers from the root do not reach the goal box
    engines = [_load("car_2000", 217) for _ in range(3)]
    H = [_horizon("car_2000")] * 3
    with pytest.raises(nat.NativeError) as ex:
        Engine.connect_commit_multi(engines, [211, 0, None], H)
    assert ex.value.code == nat.E_STATE and ex.value.failed == [1]
    assert ex.value.results[1] is None and ex.value.results[2] == [] and engines[1].size == engines[2].size == 217
    _check_commit(engines[0], "car_2000", 217, _ref_win("car_2000", 217, 8, cr.NO_INCUMBENT), ex.value.results[0])
    assert Engine.connect_search_multi(engines[1:], H[1:], [cr.NO_INCUMBENT] * 2) == [(951, 211)] * 2
    for e in engines:
        e.close()


def test_refused_with_nothing_launched():
    from lqrrt_amd.engine import Engine
    cars = [_load("car_2000", 217) for _ in range(3)]
    boat = _load("boat_novice_300", 107)
    H, Hb = _horizon("car_2000"), _horizon("boat_novice_300")
    NO = cr.NO_INCUMBENT
    before = [_tree(e) for e in cars + [boat]]
    fp0 = [e.footprint() for e in cars + [boat]]
    with pytest.raises(ValueError, match="twice"):
        Engine.connect_search_multi([cars[0], cars[1], cars[0]], [H] * 3, [NO] * 3)
    with pytest.raises(ValueError, match="twice"):
        Engine.connect_commit_multi([cars[0], cars[1], cars[0]], [211] * 3, [H] * 3)
    with pytest.raises(ValueError, match="model"):
        Engine.connect_search_multi([cars[0], boat], [H, Hb], [NO] * 2)
    with pytest.raises(ValueError, match="model"):
        Engine.connect_commit_multi([cars[0], boat], [211, 77], [H, Hb])
    with pytest.raises(ValueError, match="outside the tree"):
        Engine.connect_search_multi(cars, [H] * 3, [NO] * 3, nodes=[None, None, [0, 217]])
    with pytest.raises(ValueError, match="outside the tree"):
        Engine.connect_commit_multi(cars, [211, 211, 217], [H] * 3)
    with pytest.raises(ValueError, match="incumbent"):
        Engine.connect_search_multi(cars, [H] * 3, [NO, NO, 0])
    with pytest.raises(ValueError, match="horizon"):
        Engine.connect_search_multi(cars, [H, H, H + 10 ** 6], [NO] * 3)
    with pytest.raises(ValueError, match="horizon"):
        Engine.connect_commit_multi(cars, [211] * 3, [H, H, H + 10 ** 6])
    with pytest.raises(ValueError, match="goal_tries"):
        Engine.connect_search_multi(cars, [H] * 3, [NO] * 3, goal_tries=[8, 8, 0])
    with pytest.raises(ValueError):
        Engine.connect_search_multi(cars, [H] * 3, [NO] * 3, nodes=[None])
    with pytest.raises(ValueError):
        Engine.connect_search_multi([], [], [])
    crowd = [_load("double_integrator_600", 1, extra=2) for _ in range(129)]
    Hd = _horizon("double_integrator_600")
    with pytest.raises(ValueError, match="128"):
        Engine.connect_search_multi(crowd, [Hd] * 129, [NO] * 129)
    with pytest.raises(ValueError, match="128"):
        Engine.connect_commit_multi(crowd, [0] * 129, [Hd] * 129)
    assert all(e.size == 1 for e in crowd)
    assert Engine.connect_search_multi(crowd[:128], [Hd] * 128, [NO] * 128) == [(41, 0)] * 128     # 128 engines are a call
    for e, old in zip(cars + [boat], before):
        for x, y in zip(_tree(e), old):
            assert np.array_equal(x, y)
    assert [e.footprint() for e in cars + [boat]] == fp0
    for e in cars + [boat] + crowd:
        e.close()
