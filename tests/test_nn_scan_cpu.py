"""
tests/nn_scan_reference.py checked on the host: the model against the reference planner's cost and selection (bit for bit), the
table builders' planted answers against the model for every (N, s) that tests/test_nn_scan_gpu.py uses, and the restated launch
plan against hand-computed values.
"""
import numpy as np
import pytest

import nn_scan_reference as R
from systems_np import SYSTEMS, make_oracle_planner


def _oracle_system(name):
    if name == "double_integrator":
        return SYSTEMS[name]()
    if name == "ros_boat":
        return SYSTEMS[name]("car")                  # the behaviour with S = diag(1,1,1,0,0,0)
    return SYSTEMS[name](0)


@pytest.mark.parametrize("name", sorted(SYSTEMS))
def test_model_is_the_reference(name):
    """costs == RefPlanner._costs_to_go and select == the reference's selection (oracle/lqrrt_oracle.py extend_once), exactly, on a
    random 300-node table with and without an ignore set -- and with every node ignored."""
    from lqrrt_oracle import RefTree
    s = _oracle_system(name)
    rs = np.random.RandomState(len(name))
    N = 300
    nodes = R.self_table(s, N, rs)
    ref = make_oracle_planner(s, N)
    ref.tree = RefTree(nodes[0], s.lqr(nodes[0], np.zeros(s.ncontrols)))
    ref.tree.state = nodes.copy()
    ref.tree.size = N
    m = R.ScanModel(nodes, s.wrap_dims)
    lo, hi = R.widened_space(s)
    queries = list(lo + (hi - lo) * rs.random_sample((6, s.nstates))) + [nodes[17].copy(), nodes[N - 1].copy()]
    for flags in (np.zeros(N, dtype=bool), rs.random_sample(N) < 0.5, np.ones(N, dtype=bool)):
        m.ign = flags
        for x in queries:
            want = ref._costs_to_go(np.copy(x))
            S = s.lqr(np.copy(x), np.zeros(s.ncontrols))[0]
            got = m.costs(x, S)
            np.testing.assert_array_equal(got, want)
            if not np.any(np.asarray(S) - np.diag(np.diag(S))) and np.all(np.diag(S) == 1):
                np.testing.assert_array_equal(m.costs(x, None), want)         # S = None is the identity
            order = np.argsort(want, kind="stable")                          # lqrrt_oracle.py:234-238
            nearest = order[0]
            live = order[~flags[order]]
            if len(live):
                nearest = live[0]
            assert m.select(got) == int(nearest) == int(m.answers(got[None, :])[0])
            assert m.answers(got[None, :], use_ignore=False)[0] == int(np.argmin(want))
            assert m.select(got, use_ignore=False) == int(np.argmin(want))
    np.testing.assert_array_equal(m.cost_rows(queries[:3], None), [m.costs(x) for x in queries[:3]])
    Ss = rs.random_sample((3, s.nstates, s.nstates))
    np.testing.assert_array_equal(m.cost_rows(queries[:3], Ss), [m.costs(x, Ss[t]) for t, x in enumerate(queries[:3])])


def _tie_cases():
    return [(N, s) for N in R.TIE_SIZES for s in sorted(set(R.PERIODS))] + [(R.BIG_N, s) for s in R.BIG_PERIODS]


@pytest.mark.parametrize("N,s", _tie_cases())
def test_periodic_table_plants_what_the_model_selects(N, s):
    """The query base[r] of a period-s table: the model selects the lowest eligible id congruent to r; it moves up as the lower
    copies are ignored; with every node ignored it is r itself, the overall first."""
    sysm = _oracle_system("pendulum")                               # two wrapped states
    rs = np.random.RandomState(N + s)
    base = R.self_table(sysm, s, rs)
    if s <= 1024:                                                   # (beyond: the zero count per row below says the same)
        R.ScanModel(base, sysm.wrap_dims).assert_distinct()
    nodes = R.periodic_table(base, N)
    assert nodes.shape == (N, 4) and np.array_equal(nodes[N - 1], base[(N - 1) % s])
    m = R.ScanModel(nodes, sysm.wrap_dims)
    res = R.tie_residues(s)
    assert set(range(min(8, s))) <= set(res) and len(res) >= min(64, s)
    rows = m.cost_rows(base[res])
    for name, flags in R.tie_ignore_sets(N, s):
        m.ign = flags
        for r, c in zip(res, rows):
            planted = R.lowest_congruent(N, s, r, flags)
            copies = np.arange(r, N, s)
            assert np.all(c[copies] == 0.0) and np.count_nonzero(c == 0.0) == len(copies)
            got = m.select(c)
            assert got == m.answers(c[None, :])[0]
            if name == "all":
                assert planted is None and got == r
            elif planted is not None:
                assert got == planted and not flags[planted]
                assert name != "none" or planted == r
                assert name != "all but the highest copy" or planted == copies[-1]
            else:
                assert flags[copies].all() and c[got] > 0.0 and not flags[got]


@pytest.mark.parametrize("s", R.DIAG_PERIODS)
def test_velocity_table_ties_under_a_diagonal_S_with_zeros(s):
    """ros_boat 'car' (S = diag(1,1,1,0,0,0)): nodes that share position and heading but not velocity cost the same, bit for bit,
    for a query on the position and for one next to it; under the identity they do not tie."""
    N = 1025
    sysm = _oracle_system("ros_boat")
    S = sysm.lqr(np.zeros(6), np.zeros(3))[0]
    assert np.array_equal(np.diag(S), [1, 1, 1, 0, 0, 0])
    rs = np.random.RandomState(s)
    base = R.self_table(sysm, s, rs)
    nodes = R.velocity_table(sysm, base, N, (3, 4, 5), rs)
    assert len(np.unique(nodes, axis=0)) == N
    m = R.ScanModel(nodes, sysm.wrap_dims)
    res = R.tie_residues(s)
    xs = R.velocity_queries(sysm, base, res, rs)
    assert len(xs) == 2 * len(res)
    rows = m.cost_rows(xs, S)
    for t, c in enumerate(rows):
        r = res[t % len(res)]
        copies = np.arange(r, N, s)
        assert np.all(c[copies] == c[r]) and (c[r] == 0.0) == (t < len(res))
        for name, flags in R.tie_ignore_sets(N, s):
            m.ign = flags
            got = m.select(c)
            assert got == m.answers(c[None, :])[0]
            planted = R.lowest_congruent(N, s, r, flags)
            if name == "all":
                assert got == r
            elif planted is not None:
                assert got == planted
        if len(copies) > 1:
            assert len(set(m.costs(xs[t], None)[copies])) == len(copies)    # the identity tells the copies apart


@pytest.mark.parametrize("N", R.SELF_SIZES)
def test_self_table_plants_what_the_model_selects(N):
    for name in ("boat_advanced", "pendulum", "ros_boat"):
        sysm = _oracle_system(name)
        nodes = R.self_table(sysm, N, np.random.RandomState(N))
        m = R.ScanModel(nodes, sysm.wrap_dims)
        S = sysm.lqr(nodes[0], np.zeros(sysm.ncontrols))[0]
        m.assert_distinct(S)
        rows = m.cost_rows(nodes, S)
        for sname, flags in R.self_ignore_sets(N):
            m.ign = flags
            got = m.answers(rows)
            for k in range(N):
                if flags.all() or not flags[k]:            # (every node ignored: the overall first, planner.py:245)
                    assert got[k] == k
                else:
                    assert got[k] != k and not flags[got[k]]


def test_launch_plan_hand_values():
    """engine_launch.hpp pick_chunks / launch_nn by hand: want = min(2048 / groups, 1024) wavefronts (4096 from 8 groups on), chunk =
    ceil(count / want) rounded up to 8, at least 16 (LQRRT_NN_MIN_CHUNK)."""
    pc = R.pick_chunks
    assert pc(1, 1) == (16, 1) and pc(16, 64) == (16, 1) and pc(17, 64) == (16, 2)
    assert pc(128, 64) == (16, 8) and pc(144, 64) == (16, 9) and pc(1024, 64) == (16, 64) and pc(1025, 64) == (16, 65)
    assert pc(1024, 1024) == (16, 64) and pc(1025, 65) == (16, 65) and pc(1025, 129) == (16, 65)
    assert pc(16407, 64) == (24, 684)                              # ceil(16407 / 1024) = 17 -> 24
    assert pc(16407, 65) == (24, 684)                              # two groups: want = 1024 still
    assert pc(32805, 64) == (40, 821)                              # ceil(32805 / 1024) = 33 -> 40
    assert pc(32805, 1024) == (136, 242)                           # 16 groups: want = 256, ceil(32805 / 256) = 129 -> 136
    assert pc(1025, 64, min_chunk=8) == (8, 129) and pc(1025, 1024, min_chunk=8) == (8, 129)
    assert pc(1025, 64, nn_waves=64) == (24, 43)                   # want = 64: ceil(1025 / 64) = 17 -> 24
    assert pc(1025, 129, nn_waves=64) == (56, 19)                  # three groups: want = 21, ceil(1025 / 21) = 49 -> 56
    assert pc(5, 64, nn_waves=64, min_chunk=8) == (8, 1)

    p = R.launch_plan(128, 64)
    assert (p["wg4"], p["parts"], p["xcd"], p["reduce_stride"]) == (False, 8, True, False)
    p = R.launch_plan(144, 64)
    assert (p["wg4"], p["parts"], p["xcd"]) == (False, 9, False)
    p = R.launch_plan(1025, 64)
    assert (p["wg4"], p["parts"], p["xcd"], p["reduce_stride"]) == (False, 65, False, True)
    p = R.launch_plan(1024, 1024)
    assert (p["gx"], p["gy"], p["xcd"]) == (16, 64, True)
    p = R.launch_plan(16407, 64)
    assert (p["wg4"], p["parts"], p["reduce_stride"]) == (False, 684, True) and 684 > 10 * 64      # every reduce lane strides
    # the natural WPB = 4 table: 821 chunks of 40 -> 206 workgroups, the last one with a single real chunk
    p = R.launch_plan(R.BIG_N, 64)
    assert (p["chunk"], p["n_sub"], p["wg4"], p["parts"], p["last_group"]) == (40, 821, True, 206, 1)
    assert p["reduce_stride"] and not p["xcd"]
    for form, wg4 in (("ident", True), ("dense", True), ("band2", True), ("diag", False), ("persample", False)):
        assert R.launch_plan(R.BIG_N, 64, form)["wg4"] is wg4
    assert R.launch_plan(32767, 64)["wg4"] is False and R.launch_plan(32768, 64)["wg4"] is True
    # forced forms
    p = R.launch_plan(1025, 64, wg4_env=1, min_chunk=8)
    assert (p["n_sub"], p["wg4"], p["parts"], p["last_group"], p["xcd"]) == (129, True, 33, 1, False)
    p = R.launch_plan(1024, 64, wg4_env=1, min_chunk=8)
    assert (p["n_sub"], p["wg4"], p["parts"], p["last_group"], p["xcd"]) == (128, True, 32, 4, True)
    p = R.launch_plan(63, 63, wg4_env=1, min_chunk=8)
    assert (p["n_sub"], p["wg4"], p["parts"], p["last_group"]) == (8, True, 2, 4)
    p = R.launch_plan(65, 64, wg4_env=1, min_chunk=8)
    assert (p["n_sub"], p["wg4"], p["parts"], p["last_group"]) == (9, True, 3, 1)
    assert R.launch_plan(5, 5, wg4_env=1, min_chunk=8)["wg4"] is False                # fewer than 8 chunks: never
    assert R.launch_plan(1025, 64, "persample", wg4_env=1, min_chunk=8)["wg4"] is False
    p = R.launch_plan(1025, 64, wg4_env=0, nn_waves=64)
    assert (p["wg4"], p["parts"], p["reduce_stride"]) == (False, 43, False)
    assert R.launch_plan(R.BIG_N, 64, wg4_env=0)["wg4"] is False


def test_angle_mode_restated():
    xs = np.zeros((130, 4))
    xs[:, 0], xs[:, 1] = 0.5, -0.25
    xs[64:, 0] = 0.75
    xs[129, 1] = 1.0
    assert R.angle_mode(xs, (0, 1), fixed=(0.5, -0.25)) == [2, 1, 0]
    assert R.angle_mode(xs, (0, 1), fixed=None) == [1, 1, 0]
    assert R.angle_mode(xs[:129], (0, 1), fixed=(0.75, -0.25)) == [1, 2, 2]
    assert R.angle_mode(xs, ()) == [0, 0, 0]
