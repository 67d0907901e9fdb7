"""
tests/feasibility_reference.py checked on the host, and with it everything about the collision tests that needs no GPU:

  * on EVERY pose set of tests/test_feasibility_gpu.py the model, the NumPy twin (oracle/systems_np.py) and the sequential C oracle
    (oracle/lqrrt_oracle.c) give the same flags, pose for pose, none left out -- and where a case plants its answers, those.  The
    planted edge cases use the one-point hull or heading 0, where np.sin and the portable sine cannot differ in effect; the
    general-heading sets (wall approaches, the shared set of case g) agree as drawn: no pose had to be replaced.
  * the restated culls are conservative: over some thousands of random (hull, map, pose) and (hull, circle table, pose) triples --
    disc, diamond and sparse hulls, maps whose sizes are no multiple of 8 -- the grid cull only answers "free" where the plain model
    does, and an obstacle that is not `near` holds no hull point.
  * every index the restated grid cull reads lies inside the coarse map or the map, over that sweep and at the two border poses of
    the disc; the rule before the fine stage got its bounds condition reads rows -3 and columns 67 of a 64 x 64 map
    there, and this test says so.
  * exact_sq_threshold restated: `d2 <= thr` is `sqrt(d2) <= r` at the threshold, either side of it and at r * r, for radii over many
    binades and for 0, a denormal, inf, negative and NaN.
"""
import numpy as np
import pytest

import feasibility_reference as R


@pytest.fixture(scope="module")
def grid_cases():
    return R.grid_cases()


@pytest.fixture(scope="module")
def circle_cases():
    return R.circle_cases()


def _hold_together(case):
    m = case.model()
    t = case.twin_answers()
    o = case.oracle_answers()
    bad = np.flatnonzero((m != t) | (m != o))
    assert len(bad) == 0, (case.name, "poses", bad[:8], "model", m[bad][:8], "twin", t[bad][:8], "C oracle", o[bad][:8], case.X[bad][:4])
    if case.expect is not None:
        np.testing.assert_array_equal(m, case.expect, err_msg="%s: the model does not give the planted answers" % case.name)
    return m


def test_grid_cases_model_twin_and_oracle_agree(grid_cases):
    names = [c.name for c in grid_cases]
    assert len(set(names)) == len(names)
    seen = set()
    for case in grid_cases:
        m = _hold_together(case)
        seen.add(case.name[0])
        if case.name[0] in "fg" and case.expect is None:
            assert m.any() and not m.all(), case.name             # a wall approach / the shared set sees both answers
    assert seen == set("abcdefgi")


def test_circle_cases_model_twin_and_oracle_agree(circle_cases):
    names = [c.name for c in circle_cases]
    assert len(set(names)) == len(names)
    for case in circle_cases:
        _hold_together(case)
    assert set(c.name[0] for c in circle_cases) == set("jklmno")


def test_model_with_numpy_trig_is_the_twin(grid_cases):
    """The model fed np.cos / np.sin is the reference's own arithmetic up to the BLAS order of the 2 x 2 rotation: on the general-
    heading sets it gives the twin's flags too."""
    for case in grid_cases:
        if case.name[0] in "fg":
            np.testing.assert_array_equal(case.model(R.numpy_sincos), case.twin_answers(), err_msg=case.name)


def test_cases_reach_the_paths_they_name(grid_cases, circle_cases):
    """What tests/test_feasibility_gpu.py asserts before it launches anything, on the host."""
    for case in grid_cases:
        if case.stages is not None:
            assert case.stage_names() == list(case.stages), (case.name, case.stage_names(), case.stages)
    by = lambda letter: [c for c in grid_cases if c.name.startswith(letter + " ")]
    # e: the include / exclude pairs differ in exactly the block they are about
    for case in by("e"):
        if "cell" not in case.name:
            continue
        r, c = [int(v) for v in case.name[case.name.index("(") + 1:case.name.index(")")].split(",")]
        for d, st in zip(case.culls(), case.stages):
            cy0, cy1, cx0, cx1 = d["coarse"]
            inside = cy0 <= (r >> 3) <= cy1 and cx0 <= (c >> 3) <= cx1
            assert inside == (st == "fine"), (case.name, d, st)
        assert case.stages.count("fine") == case.stages.count("coarse") >= 2, case.name
    assert any(c.name == "e cell (58, 73)" and "fine" in c.stages for c in by("e"))           # the partial last block is read
    # f: a wall approach passes through every stage
    for case in by("f"):
        if "wall" in case.name:
            st = case.stage_names()
            assert {"coarse", "fine", "sweep:occupied"} <= set(st), (case.name, sorted(set(st)))
            m = case.model()
            assert m[[i for i, v in enumerate(st) if v == "sweep:occupied"]].any()            # next to the wall and clear of it
    # d: the hull is read from HBM
    for case in by("d"):
        assert not case.geo().og_lds
    for case in by("c"):
        assert case.geo().og_lds
    # i: a non-finite heading next to the blob passes the first cull and is turned to the sweep by the bounds condition
    for case in by("i"):
        st = case.stage_names()
        bad_heading = [k for k, x in enumerate(case.X) if np.isfinite(x[0]) and np.isfinite(x[1]) and not np.isfinite(x[2]) and x[0] > 1]
        assert bad_heading and all(st[k] in ("sweep:bounds", "sweep:occupied") for k in bad_heading), (case.name, [st[k] for k in bad_heading])
    # l / n / m through the near predicate
    for case in circle_cases:
        near = case.nears() if case.kind == "circle" else None
        if case.name.startswith("l ") and case.geo().O:
            assert near[0].sum() == 1 and near[0][-1], case.name                              # only the last slot is near ...
            assert case.geo().O - 1 >= 0 and near.shape[1] == case.geo().O
        if case.name.startswith("n "):
            assert not near.any(), case.name                                                  # the obstacle around 2p is nowhere near the hull
            assert int(np.flatnonzero(case.obs[:, 0] == 2 * case.X[0, 0])[0]) >= 64
        if case.name.startswith("m diagonal"):
            assert near[0].any() and case.model()[0]                                          # near, no hit
        if case.name.startswith("m centre just outside"):
            assert not near.any(), case.name
        if case.name.startswith("m centre just inside"):
            assert near.any(), case.name
        if case.name.startswith("m rounding"):
            assert near[0][1] and not case.nears(padded=False)[0][1] and not case.model()[0], case.name


# ------------------------------------------------------------------------------------------------ the culls are conservative

def _random_hull(rs):
    k = rs.randint(0, 6)
    if k == 0:
        return R.disc_hull(int(rs.choice([12, 96])), rs.uniform(0.3, 1.6))
    if k == 1:
        return R.diamond_hull(rs.uniform(0.5, 2.0), rs.uniform(0.2, 0.9), int(rs.randint(2, 9)))
    if k == 2:
        return R.sparse_hull(rs.uniform(0.4, 2.5), rs.uniform(0.2, 1.2))
    if k == 3:
        return R.lattice_hull(rs.choice([0.5, 1.0, 2.0]), rs.choice([0.25, 0.5, 1.0]), 0.25)
    if k == 4:
        return R.point_hull()
    return rs.uniform(-1.0, 1.0, (2, int(rs.randint(1, 30)))) + rs.uniform(-0.5, 0.5, (2, 1))      # off-centre cloud


def _assert_reads_inside(geo, d):
    if d["coarse"] is not None:
        cy0, cy1, cx0, cx1 = d["coarse"]
        assert 0 <= cy0 <= cy1 < geo.crows and 0 <= cx0 <= cx1 < geo.ccols, d
    if d["fine_read"]:
        fy0, fy1, fx0, fx1 = d["fine"]
        assert 0 <= fy0 <= fy1 < geo.rows and 0 <= fx0 <= fx1 < geo.cols, d


def test_grid_cull_is_conservative_and_reads_inside_the_map():
    rs = np.random.RandomState(2024)
    stages, outside_before = {}, 0
    for trial in range(160):
        rows, cols = int(rs.randint(20, 90)), int(rs.randint(20, 90))
        cpm = float(rs.choice([2.0, 5.0, 10.0, 7.3]))
        origin = (rs.uniform(-3, 3), rs.uniform(-3, 3))
        grid = np.where(rs.random_sample((rows, cols)) < rs.choice([0.002, 0.01, 0.05]), R.OCC, R.FREE).astype(np.int8)
        vps = _random_hull(rs)
        geo = R.GridGeo(vps, grid, R.THR)
        for _ in range(25):
            x = np.array([origin[0] + rs.uniform(-0.5, cols / cpm + 0.5), origin[1] + rs.uniform(-0.5, rows / cpm + 0.5), rs.uniform(-4, 4)])
            if rs.random_sample() < 0.3:                          # hug the border: where the rotated box leaves the reach box
                x[0] = origin[0] + (2.0 + rs.uniform(0, 0.3)) / cpm + geo.reach if rs.random_sample() < 0.5 else origin[0] + (cols - 2 - rs.uniform(0, 0.3)) / cpm - geo.reach
                x[1] = origin[1] + (2.0 + rs.uniform(0, 0.3)) / cpm + geo.reach if rs.random_sample() < 0.5 else origin[1] + (rows - 2 - rs.uniform(0, 0.3)) / cpm - geo.reach
            c, s = R.portable_sincos(float(x[2]))
            d = R.grid_cull(geo, origin, cpm, x, c, s)
            _assert_reads_inside(geo, d)
            stages[d["stage"] + ":" + str(d["why"])] = stages.get(d["stage"] + ":" + str(d["why"]), 0) + 1
            if d["stage"] != "sweep":
                assert R.grid_feasible(vps, grid, origin, cpm, R.THR, x, c, s), (trial, d, x)
            old = R.grid_cull(geo, origin, cpm, x, c, s, bounded=False)
            outside_before += old["why"] == "outside"
            if d["why"] != "bounds":
                assert old == d
    assert stages.get("coarse:None", 0) > 200 and stages.get("fine:None", 0) > 50 and stages.get("sweep:border", 0) > 200, stages
    assert stages.get("sweep:bounds", 0) > 5 and stages.get("sweep:occupied", 0) > 20, stages
    assert outside_before == stages["sweep:bounds"] > 0           # what the previous rule read outside the map, the new one does not read


def test_the_finding_border_poses_of_the_disc():
    """The disc at heading pi/4 with its reach box just inside the 64 x 64 map: the fine box of the previous rule spans cells
    [-3, 27] at the low corner and [36, 67] at the high one -- rows and columns that do not exist; the bounds condition sends both
    poses to the exact sweep, which reads only cells that hull points lie in."""
    case = R.border_disc_case()
    geo = case.geo()
    assert (geo.rows, geo.cols) == (64, 64)
    old = case.culls(bounded=False)
    assert old[0]["fine"] == (-3, 27, -3, 27) and old[0]["fine_read"] and old[0]["why"] == "outside"
    assert old[1]["fine"] == (36, 67, 36, 67) and old[1]["fine_read"] and old[1]["why"] == "outside"
    assert old[0]["fine"][0] == -3 and old[1]["fine"][3] == 67
    assert (27 + 3 + 1) ** 2 == 961 <= R.FINE_CELLS_MAX and (67 - 36 + 1) ** 2 <= R.FINE_CELLS_MAX      # few enough cells to be read
    new = case.culls()
    for d in new:
        assert d["stage"] == "sweep" and d["why"] == "bounds" and not d["fine_read"]
        _assert_reads_inside(geo, d)
    with pytest.raises(AssertionError):
        for d in old:
            _assert_reads_inside(geo, d)
    np.testing.assert_array_equal(case.model(), [True, True])


def test_circle_cull_is_conservative():
    rs = np.random.RandomState(77)
    far = 0
    for trial in range(250):
        vps = _random_hull(rs)
        O = int(rs.choice([1, 5, 20]))
        obs = np.column_stack((rs.uniform(-6, 6, O), rs.uniform(-6, 6, O), rs.choice([0.0, 0.05, 0.5, 1.5, -1.0], O)))
        geo = R.CircleGeo(vps, obs)
        for _ in range(12):
            x = np.array([rs.uniform(-6, 6), rs.uniform(-6, 6), rs.uniform(-4, 4)])
            c, s = R.portable_sincos(float(x[2]))
            near = R.circle_near(geo, x, c, s)
            verts = R.vertices(vps, x, c, s)
            for o in np.flatnonzero(~near):
                far += 1
                assert not np.any(np.linalg.norm(verts - obs[o, :2], axis=1) <= obs[o, 2]), (trial, o, x)
            assert R.circles_feasible(vps, obs[near], x, c, s) == R.circles_feasible(vps, obs, x, c, s)
    assert far > 10000


# ------------------------------------------------------------------------------------------------ the squared threshold

def test_exact_sq_threshold_restated():
    nan, inf = float("nan"), float("inf")
    rs = np.random.RandomState(9)
    radii = [0.0, 5e-324, 2.2250738585072014e-308, 1e-200, 1.0, 1.25, 0.1, 3.0, 5.0, 1e154, 1.3407807929942596e154, 1e200, 1.7976931348623157e308]
    radii += list(np.exp2(rs.uniform(-600, 600, 300))) + [float(np.nextafter(1.0, 2.0)), float(np.nextafter(1.0, 0.0))]
    with np.errstate(over="ignore", invalid="ignore"):
        for r in radii:
            r = np.float64(r)
            thr = R.exact_sq_threshold(r)
            assert thr >= 0.0
            cand = [thr, np.nextafter(thr, np.inf), np.nextafter(thr, -np.inf), r * r, np.float64(0.0), np.float64(inf)]
            for d2 in cand:
                if d2 >= 0.0:
                    assert bool(d2 <= thr) == bool(np.sqrt(d2) <= r), (r, thr, d2)
            assert np.sqrt(thr) <= r and (np.isinf(np.nextafter(thr, np.inf)) or np.sqrt(np.nextafter(thr, np.inf)) > r), (r, thr)
        assert R.exact_sq_threshold(inf) == inf
        # thr == r * r exactly where the mantissa of r is at least sqrt 2, above it otherwise: case j's k = 3 (r = 15, d2 = 225 = thr) and
        # case k's r = 0 (d2 = 0 = thr) are the poses that tell `d2 <= thr` from `d2 < thr`
        assert R.exact_sq_threshold(15.0) == 225.0 and R.exact_sq_threshold(5.0) > 25.0 and R.exact_sq_threshold(0.0) == 0.0
        assert 3.0 in R.TANGENT_K
        for r in (-1.0, -5e-324, -inf, nan, -9999.0):
            thr = R.exact_sq_threshold(r)
            assert thr == -1.0
            for d2 in (0.0, 5e-324, 1.0, inf):
                assert bool(d2 <= thr) == bool(np.sqrt(np.float64(d2)) <= r) == False  # noqa: E712
        assert R.exact_sq_threshold(-0.0) == 0.0                  # -0.0 >= 0: a vertex on the centre hits, as norm 0 <= -0.0 does
    # and the derived table of a case: thresholds, padded radii, the never-near mark of a placeholder
    g = R.CircleGeo(R.lattice_hull(), [[1.0, 2.0, 0.5], [0.0, 0.0, -9999.0], [0.0, 0.0, nan]])
    assert g.oc[0, 2] == R.exact_sq_threshold(0.5) and g.oc[0, 3] == 0.5 * (1.0 + 1e-9) + 1e-9
    assert g.oc[1, 2] == -1.0 and g.oc[1, 3] == -1e300 and g.oc[2, 2] == -1.0 and g.oc[2, 3] == -1e300
    assert g.lds_bytes == 8 * (2 * 45 + 4 * 3)


def test_index_rules_restated():
    """cell_indices by hand: truncation towards zero, one wrap, IndexError beyond; undefined casts are outside."""
    f = np.array([0.0, 0.99, -0.0, -0.5, -0.999, -1.0, -1.5, -10.0, -10.5, -11.0, 9.0, 9.99, 10.0, float("nan"), float("inf"), -float("inf"), 2.0 ** 63, -2.0 ** 63,
                  9.2e18])
    i, ok = R.cell_indices(f, 10)
    assert list(i[ok]) == [0, 0, 0, 0, 0, 9, 9, 0, 0, 9, 9]
    assert list(ok) == [True] * 9 + [False] + [True, True] + [False] * 7
