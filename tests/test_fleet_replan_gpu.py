"""
Fleet replanning: lqrrt_amd.update_plans jobs with a `root` (one batched tree retain per group, Engine.tree_retain_multi) against
the same planners replanning one by one (Planner.replan, Engine.tree_retain), BIT FOR BIT.  Recipe of tests/test_retain_gpu.py:
the clock stands still, so every plan ends when its tree exceeds max_nodes and everything is deterministic.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_retain_gpu import _check_plan, _planner

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _change_map(s, p, k):
    """Planner k's own new obstacle: a circle beside the middle of its plan (replan / update_plans synchronise it)."""
    plan = [int(v) for v in p.node_seq]
    mid = p._engine.states(plan[len(plan) // 2], 1)[0]
    s.set_obstacles(np.vstack((np.asarray(s.obs, dtype=np.float64).reshape(-1, 3), [mid[0] + 3.0 + 0.5 * k, mid[1], 0.8 + 0.2 * k])))
    return plan


def test_fleet_replan_is_every_planners_own_replan():
    import lqrrt_amd
    n, max_nodes = 5, 2500
    seeds, seeds2 = [11, 12, 13, 14, 15], [21, 22, 23, 24, 25]
    revalidate = [True, True, False, True, True]
    fresh = 3                                                                    # this planner starts over from a new x0 in the second call
    fleet = [(s, _planner(s, max_nodes=max_nodes)) for s in (lqrrt_amd.systems.BoatAdvanced(0) for _ in range(n))]
    twins = [(s, _planner(s, max_nodes=max_nodes)) for s in (lqrrt_amd.systems.BoatAdvanced(0) for _ in range(n))]
    job = lambda s, p, **kw: dict(planner=p, sample_space=s.sample_space, goal_bias=s.goal_bias, **kw)

    # ---- first plan: together / one by one
    res = lqrrt_amd.update_plans([job(s, p, x0=s.x0, seed=sd) for (s, p), sd in zip(fleet, seeds)])
    assert res == [False] * n                                                    # ended by max_nodes
    for (s, q), sd in zip(twins, seeds):
        np.random.seed(sd)
        assert q.update_plan(s.x0, s.sample_space, goal_bias=s.goal_bias) is False
    held = [p.tree for _, p in fleet]                                            # held: must stay what they were
    held_state = [t.state.copy() for t in held]
    held_pid = [list(t.pID) for t in held]
    roots = []
    for k, ((s, p), (s2, q)) in enumerate(zip(fleet, twins)):
        assert p.tree.size == q.tree.size == max_nodes + 1
        plan = _change_map(s, p, k)
        assert _change_map(s2, q, k) == plan and len(plan) > 4
        kk, node, _ = p.plan_node_after(0.2 * p.T)
        assert node == plan[kk] and 0 < kk < len(plan) - 1
        roots.append(node)
    x_new = np.array(fleet[fresh][0].x0, dtype=np.float64) + np.array([1.0, 0.5, 0.0, 0.0, 0.0, 0.0])

    # ---- second plan: ONE update_plans call (four roots, one of them without revalidation, and a fresh start in the same group) ...
    jobs = []
    for k, ((s, p), sd) in enumerate(zip(fleet, seeds2)):
        if k == fresh:
            jobs.append(job(s, p, x0=x_new, seed=sd))
        elif revalidate[k]:
            jobs.append(job(s, p, root=roots[k], seed=sd))
        else:
            jobs.append(job(s, p, root=roots[k], seed=sd, revalidate=False))
    before = np.random.get_state()[1].copy()
    res = lqrrt_amd.update_plans(jobs)
    assert np.array_equal(np.random.get_state()[1], before)                      # per-planner streams: np.random untouched
    # ... against replan / update_plan one by one
    res2 = []
    for k, ((s, q), sd) in enumerate(zip(twins, seeds2)):
        np.random.seed(sd)
        if k == fresh:
            res2.append(q.update_plan(x_new, s.sample_space, goal_bias=s.goal_bias))
        else:
            res2.append(q.replan(roots[k], s.sample_space, goal_bias=s.goal_bias, revalidate=revalidate[k]))
    assert res == res2 == [False] * n
    for k, ((s, p), (_, q)) in enumerate(zip(fleet, twins)):
        print("planner %d: retained %s, tree %d, attempts %d" % (k, p.retained, p.tree.size, p.stats["attempts"]))
        assert p.retained == q.retained and (p.retained is None) == (k == fresh)
        if k != fresh:
            assert 1 < p.retained["kept"] < max_nodes + 1 and p.retained["old_size"] == max_nodes + 1
            if not revalidate[k]:
                assert p.retained["infeasible"] == 0 and p.retained["orphaned"] == 0
        a, b = p._engine, q._engine
        assert p.tree.size == q.tree.size == a.size == b.size == max_nodes + 1 and p.tree.on_device
        np.testing.assert_array_equal(a.states(), b.states())
        np.testing.assert_array_equal(a.parents(), b.parents())
        np.testing.assert_array_equal(a.gains(), b.gains())
        np.testing.assert_array_equal(a.ignored(), b.ignored())
        np.testing.assert_array_equal(p.tree.state, q.tree.state)
        assert list(p.tree.pID) == list(q.tree.pID)
        assert p.plan_reached_goal == q.plan_reached_goal and list(p.node_seq) == list(q.node_seq) and p.T == q.T
        np.testing.assert_array_equal(np.array(p.x_seq), np.array(q.x_seq))
        np.testing.assert_array_equal(np.array(p.u_seq), np.array(q.u_seq))
        assert p.stats["attempts"] == q.stats["attempts"]
        for key in ("accepted", "candidates", "goal_hits", "tree_size"):
            assert p.stats[key] == q.stats[key], key
        if revalidate[k]:
            _check_plan(p)                                                       # (unchecked edges may cross the new obstacle)
        if k != fresh:
            np.testing.assert_array_equal(p.x_seq[0], held_state[k][roots[k]])  # the plan starts at the root's state
        else:
            np.testing.assert_array_equal(p.x_seq[0], x_new)
    # the Tree objects of the first plan were detached, not overwritten
    for t, st, pid, (_, p) in zip(held, held_state, held_pid, fleet):
        assert t is not p.tree and not t.on_device and t.size == max_nodes + 1
        np.testing.assert_array_equal(t.state, st)
        assert list(t.pID) == pid

    # ---- what replan refuses is refused for every job before any planner is touched
    trees = [p.tree for _, p in fleet]
    sizes = [p._engine.size for _, p in fleet]
    with pytest.raises(ValueError, match="doesn't exist"):
        lqrrt_amd.update_plans([job(s, p, root=(0 if k < n - 1 else max_nodes + 1), seed=1) for k, (s, p) in enumerate(fleet)])
    _, p_last = fleet[-1]
    own_group = lambda: [job(s, p, root=0, seed=1, group=k) for k, (s, p) in enumerate(fleet)]   # (a group shares dt, horizon and max_nodes)
    p_last.set_resolution(dt=2 * p_last.dt)
    with pytest.raises(RuntimeError, match="dt or horizon"):
        lqrrt_amd.update_plans(own_group())
    p_last.set_resolution(dt=p_last.dt / 2)
    p_last.set_runtime(max_nodes=max_nodes - 500)
    with pytest.raises(RuntimeError, match="no tree to keep"):
        lqrrt_amd.update_plans(own_group())
    p_last.set_runtime(max_nodes=max_nodes)
    for (_, p), t, size in zip(fleet, trees, sizes):
        assert p.tree is t and t.on_device and p._engine.size == size
    # ... and a third tick still works: everybody from a node of the plan it holds now
    res = lqrrt_amd.update_plans([job(s, p, root=p.plan_node_after(0.1 * p.T)[1], seed=31 + k) for k, (s, p) in enumerate(fleet)])
    assert res == [False] * n
    for _, p in fleet:
        assert p.retained["kept"] > 1 and p.tree.size == max_nodes + 1
        _check_plan(p)


def test_fleet_replan_example_runs():
    """examples/fleet_replan_gpu.py: real clock, four boats, three plan-drive-plan ticks through update_plans."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "fleet_replan_gpu.py"), "4", "3"], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    ticks = [l for l in out.stdout.splitlines() if l.startswith("tick ")]
    assert len(ticks) == 3, out.stdout[-2000:]
    kept = [int(tok) for tok in ticks[-1].split("kept [")[1].split("]")[0].split(",")]
    assert len(kept) == 4 and all(v >= 1 for v in kept), ticks[-1]
