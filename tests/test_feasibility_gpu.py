"""
S::feasible of the hull-sweeping vehicles (csrc/systems.hpp hull_hits, grid_hits, BoatNovice::feasible) at its cull and map edges,
through Engine.feasible_batch -- one wavefront per pose -- against the sequential C oracle, flag for flag, and the plain NumPy model
of tests/feasibility_reference.py.  Booleans: the comparison is exact.

Every pose set is built in tests/feasibility_reference.py and shared with tests/test_feasibility_cpu.py, which holds model, NumPy twin
and C oracle together on all of them; every case that is named after a path asserts through the restated culls (grid_cull,
circle_near) that it reaches it, before anything is launched.

  a  index rules       truncation, one wrap of a negative index, IndexError = infeasible; one ulp either side of every rule
  b  threshold         value < thr for int8 extremes and thr in {90, 89.5, 128, -128, NaN}
  c  sweep masks       V in {1 .. 1025}: only the last vertex / the first of the last group of 512 hits; all free
  d  og_lds = 0        3073 hull points read from HBM
  e  coarse cull       block edges (mod 8 in {0, 7}), the partial last block of 61 x 75, the border condition
  f  fine cull         alongside a wall, the sparse hull, > 1024 cells, the disc at the border (where the fine cull used to read off the map)
  g  every model that calls grid_hits, one pose set
  h  a map swap to a smaller grid and hull on a live engine, then e again
  i  non-finite poses: infeasible
  j  tangency          distance exactly 5k against r = 5k and its neighbours; BoatNovice's inflated radius
  k  radii             0, inf, negative, NaN
  l  ballot rounds     O in {0 .. 129} x V in {1 .. 187}, the last obstacle and the last vertex
  m  cull edge         diagonal from a corner, the farthest corner, just outside / inside the grown box, rounding alone
  n  car               2p inside an obstacle nowhere near the hull, in the second ballot round; empty hull
  o  a NaN pose        feasible
  p  one tree through the rollout kernel, disc hull on the 61 x 75 map, bit for bit against the C oracle
  and the refusal of a circle table whose LDS stage exceeds the device's limit per workgroup.
Each test prints its wall time (nothing is asserted about it).
"""
import time

import numpy as np
import pytest

import feasibility_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _wall_time(request):
    t0 = time.time()
    yield
    print("[wall time] %s: %.2f s" % (request.node.name, time.time() - t0))


class Rig(object):
    """One native system per model with the engine behind its plugin handles: a case replaces the geometry (Case.native(into=...)),
    the engine picks it up on its next use (sync_geometry)."""

    def __init__(self):
        self.systems = {}

    def flags(self, case):
        s = case.native(into=self.systems.get(case.system))
        self.systems[case.system] = s
        eng = s._engine(0.1)
        return eng.feasible_batch(case.X)

    def close(self):
        for s in self.systems.values():
            if s._ops is not None:
                s._ops.close()
                s._ops = None


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()


def _judge(case, got, want_oracle=None):
    """Device flags against the C oracle's and the model's; the case's path and planted answers first."""
    if case.stages is not None:
        assert case.stage_names() == list(case.stages), (case.name, "does not reach the path it names")
    model = case.model()
    oracle = case.oracle_answers() if want_oracle is None else want_oracle
    np.testing.assert_array_equal(model, oracle, err_msg="%s: model and C oracle disagree" % case.name)
    if case.expect is not None:
        np.testing.assert_array_equal(model, case.expect, err_msg="%s: the model does not give the planted answers" % case.name)
    bad = np.flatnonzero(got != oracle)
    assert len(bad) == 0, (case.name, "poses", bad[:8], "device", got[bad][:8], "oracle", oracle[bad][:8], case.X[bad][:4, :3])
    return model


def _run(rig, cases):
    assert cases
    for case in cases:
        assert len(case.X) <= 4096
        _judge(case, rig.flags(case))


# ------------------------------------------------------------------------------------------------ occupancy grid

def test_a_index_rules(rig):
    cases = R.cases_a()
    assert len(cases) == 8 and {(c.grid.shape) for c in cases} == {(64, 64), (61, 75)}
    _run(rig, cases)
    for case in cases:                                             # both answers occur: the cell that is read decides
        assert case.expect.any() and not case.expect.all()


def test_b_threshold(rig):
    cases = R.cases_b()
    assert len(cases) == len(R.B_THRESHOLDS)
    _run(rig, cases)
    assert any(c.expect.all() for c in cases) and any(not c.expect.any() for c in cases)      # thr = 128 / thr = -128, NaN


def test_c_sweep_masks(rig):
    cases = R.cases_c()
    assert sorted(set(c.vps.shape[1] for c in cases)) == list(R.SWEEP_V)
    assert all(c.geo().og_lds for c in cases)
    _run(rig, cases)


def test_d_hull_points_in_hbm(rig):
    cases = R.cases_d()
    assert all(c.vps.shape[1] == 3073 and not c.geo().og_lds for c in cases)
    _run(rig, cases)
    wall = cases[-1].model()
    assert wall.any() and not wall.all()


def _check_e(cases):
    assert any(c.name == "e cell (58, 73)" and "fine" in c.stages for c in cases)             # the partial last block is read
    for c in cases:
        assert c.grid.shape == (61, 75)
        assert "coarse" in c.stages and ("fine" in c.stages or "sweep:border" in c.stages)


def test_e_coarse_cull(rig):
    cases = R.cases_e()
    _check_e(cases)
    _run(rig, cases)


def test_f_fine_cull(rig):
    cases = R.cases_f()
    for c in cases:
        if "wall" in c.name:
            st = c.stage_names()
            assert {"coarse", "fine", "sweep:occupied"} <= set(st), (c.name, sorted(set(st)))
    disc = [c for c in cases if c.name == "f disc at the border"][0]
    old = disc.culls(bounded=False)
    assert old[0]["fine"][0] == -3 and old[1]["fine"][3] == 67 and all(d["fine_read"] for d in old)    # what the previous rule read
    assert all(d["stage"] == "sweep" and d["why"] == "bounds" and not d["fine_read"] for d in disc.culls())
    _run(rig, cases)


def test_g_every_model_that_calls_grid_hits(rig):
    cases = R.cases_g()
    assert [(c.system, c.parked) for c in cases] == list(R.G_MODELS)
    answers = {}
    for case in cases:
        answers[case.name] = _judge(case, rig.flags(case))
        assert 0.1 < answers[case.name].mean() < 0.9
    parked, boxed = answers["g boat_advanced"], answers["g boat_advanced with its speed box"]
    assert np.all(parked[boxed]) and np.count_nonzero(parked & ~boxed) > 20                    # the speed box turns poses away by itself
    np.testing.assert_array_equal(parked, answers["g boat_intermediate"])
    np.testing.assert_array_equal(parked, answers["g ros_boat"])
    np.testing.assert_array_equal(parked, answers["g car"])


def test_h_map_swap_to_a_smaller_grid_and_hull_on_a_live_engine():
    from lqrrt_amd.engine import Engine
    rs = np.random.RandomState(8)
    big = R.Case("h before the swap", "boat_intermediate", R.poses([(rs.uniform(1, 11), rs.uniform(1, 11), rs.uniform(-3, 3)) for _ in range(64)]),
                 R.cluster_hull(1025, 1024), R._blob_map(128, 128, 5, blobs=30), (0.0, 0.0), 10.0)
    s = big.native()
    eng = Engine(s, capacity=64, max_wave=64)
    try:
        first = eng.feasible_batch(big.X)
        _judge(big, first)
        assert first.any() and not first.all()
        cases = R.cases_e()
        _check_e(cases)
        for case in cases:
            assert case.grid.size < big.grid.size and case.vps.shape[1] < big.vps.shape[1]
            case.native(into=s)
            assert eng.sync_geometry() and not eng.sync_geometry()
            _judge(case, eng.feasible_batch(case.X))
    finally:
        eng.close()


def test_i_non_finite_poses_are_infeasible(rig):
    cases = R.cases_i()
    _run(rig, cases)
    for case in cases:
        assert case.grid[0, 0] == R.FREE and not case.expect[:-2].any() and case.expect[-2:].all()
        st = case.stage_names()
        k = [i for i, x in enumerate(case.X) if np.isfinite(x[0]) and x[0] > 1 and np.isfinite(x[1]) and not np.isfinite(x[2])]
        assert len(k) == 3 and all(st[i] == "sweep:bounds" for i in k), (case.name, [st[i] for i in k])    # past the first cull, stopped at the second


# ------------------------------------------------------------------------------------------------ circles

def test_j_tangency(rig):
    cases = R.cases_j()
    assert {c.system for c in cases} == {"boat_intermediate", "car", "boat_novice"}
    _run(rig, cases)


def test_k_radii(rig):
    _run(rig, R.cases_k())


def test_l_ballot_rounds(rig):
    cases = R.cases_l()
    assert len(cases) == len(R.BALLOT_O) * len(R.BALLOT_V)
    for case in cases:
        if case.geo().O:
            near = case.nears()
            assert near[0].sum() == 1 and near[0][-1]              # only the last slot passes the cull
    _run(rig, cases)


def test_m_cull_edge(rig):
    cases = R.cases_m()
    for case in cases:
        near = case.nears()
        if case.name.startswith("m diagonal"):
            assert near.any()
        if "just outside" in case.name:
            assert not near.any(), case.name
        if "just inside" in case.name or "touching" in case.name:
            assert near.any(), case.name
        if "rounding" in case.name:
            assert near[0][1] and not case.nears(padded=False)[0][1], case.name
    assert sum("rounding" in c.name for c in cases) >= 4
    _run(rig, cases)


def test_n_car_stray_vertex_at_2p(rig):
    cases = R.cases_n()
    for case in cases:
        assert not case.nears().any() and case.geo().O == 70
    assert any(c.vps.shape[1] == 0 for c in cases)
    _run(rig, cases)


def test_o_a_nan_pose_is_feasible(rig):
    _run(rig, R.cases_o())


# ------------------------------------------------------------------------------------------------ end to end

def test_p_tree_through_the_rollout_kernel_bit_exact_vs_coracle():
    """boat_intermediate with the 96-point disc on the 61 x 75 map: k_steer stages the hull beside its edge history and calls the same
    grid_hits per rollout step.  Parents, states and edge lengths agree with the sequential C oracle bit for bit."""
    import coracle
    import lqrrt_amd
    from lqrrt_amd.engine import Engine
    t = R.tree_case()
    s = lqrrt_amd.systems.BoatIntermediate(0)
    s.set_occupancy_grid(t["grid"], t["origin"], cpm=t["cpm"], threshold=t["thr"], vps=t["vps"])
    nodes, wave, budget = 400, 128, 6000
    eng = Engine(s, capacity=nodes + wave + 8, max_wave=wave)
    try:
        kw = s.plan_kwargs
        eng.set_resolution(kw["dt"], kw["FPR"], int(kw["horizon"] / kw["dt"]), np.abs(s.error_tol), s.goal, np.abs(s.goal_buffer))
        space = np.array(s.sample_space, dtype=np.float64)
        eng.set_sampler(np.mean(space, axis=1), np.diff(space).flatten(), np.array(s.goal_bias, dtype=np.float64), 10)
        st = np.random.RandomState(4).get_state()
        eng.set_mt19937(st[1], st[2])
        eng.tree_reset(s.x0)
        stats = eng.extend(wave, max_attempts=budget, node_limit=nodes)
        o = coracle.make(s, nodes + wave + 8, seed=4)
        o.extend(max_iters=budget, max_nodes=nodes)
        assert eng.size == o.size and eng.size > 200
        assert stats.attempts == o.iterations and stats.candidates == o.candidates
        np.testing.assert_array_equal(eng.parents(), o.parents())
        np.testing.assert_array_equal(eng.states(), o.states())
        np.testing.assert_array_equal(eng.edge_lengths(), o.edge_lengths())
        assert (eng.edge_lengths() < 20).mean() > 0.05             # the map cut some edges
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ an oversized circle table

def test_oversized_circle_table_is_refused_before_any_launch():
    """8 (2V + 4O) bytes of LDS per workgroup, and nothing bounds O: a table just over the device's limit is refused with a ValueError
    (LQRRT_E_ARG) naming the limit by feasible_batch, the steer launch, the retain check and the sample refill; a small table on the
    same engine then passes case l."""
    import torch
    import lqrrt_amd
    from lqrrt_amd.engine import Engine
    limit = int(torch.cuda.get_device_properties(0).shared_memory_per_block)          # hipDeviceProp_t::sharedMemPerBlock
    assert limit >= 32768
    V = 1
    O = (limit // 8 - 2 * V) // 4 + 1
    assert 8 * (2 * V + 4 * O) > limit >= 8 * (2 * V + 4 * (O - 1))
    s = lqrrt_amd.systems.BoatIntermediate(0)
    s.vps = R.point_hull()
    s.set_obstacles(R.planted_table(O, {}))
    eng = Engine(s, capacity=256, max_wave=64)
    try:
        kw = s.plan_kwargs
        eng.set_resolution(kw["dt"], kw["FPR"], int(kw["horizon"] / kw["dt"]), np.abs(s.error_tol), s.goal, np.abs(s.goal_buffer))
        space = np.array(s.sample_space, dtype=np.float64)
        eng.set_sampler(np.mean(space, axis=1), np.diff(space).flatten(), np.array(s.goal_bias, dtype=np.float64), 10)
        st = np.random.RandomState(1).get_state()
        eng.set_mt19937(st[1], st[2])
        eng.tree_reset(s.x0)
        x = np.zeros((4, 6))
        calls = {"feasible_batch": lambda: eng.feasible_batch(x),
                 "steer launch": lambda: eng.steer_batch(np.zeros(4, dtype=np.int32), x + 1.0),
                 "retain check": lambda: eng.tree_retain(0, revalidate=True),
                 "refill": lambda: eng.extend(64, max_attempts=64, node_limit=32)}
        for name, call in calls.items():
            with pytest.raises(ValueError) as err:
                call()
            assert "limit" in str(err.value) and str(limit) in str(err.value), (name, str(err.value))
            assert eng.size == 1, name
        for case in R.cases_l():                                   # a small table on the same engine: the ballot-round cases
            case.native(into=s)
            assert eng.sync_geometry()
            _judge(case, eng.feasible_batch(case.X))
    finally:
        eng.close()
