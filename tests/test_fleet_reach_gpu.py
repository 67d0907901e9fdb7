"""
Fleet goal costs and retargets: lqrrt_amd.fleet_goal_costs (one batched search call per group, Engine.reach_search_multi) and
lqrrt_amd.retargets (one batched search call and one batched commit call per group, Engine.reach_commit_multi; the grown goal through
connect_goals) against the same planners asked one by one (Planner.goal_costs / Planner.retarget), BIT FOR BIT.  The planners are
grown by the recipe of tests/test_connect_gpu.py::_car_planner (seed 1, a clock that stands still, ended by the node limit below the
first goal hit), so a fleet and its twins hold identical trees.
"""
import numpy as np
import pytest

import connect_reference as cr
from test_connect_gpu import _car_planner
from test_fleet_connect_gpu import STILL, _make
from test_fleet_refine_gpu import _same_planner
from test_reach_gpu import _off_plan_targets, _reach_of

pytestmark = pytest.mark.gpu

NEVER = 4


def _fleet():
    """Four cars stopped before their first goal hit (fallback plans on trees of different sizes) and one that never planned."""
    return [_car_planner(215, **STILL), _car_planner(213, **STILL), _car_planner(216, **STILL), _car_planner(214, **STILL), _make("car")]


def _snapshot(p):
    if getattr(p, "node_seq", None) is None:
        return None, np.array(p.goal).tobytes()
    return list(p.node_seq), p.T, p.tree.size, p._engine.size, bool(p.plan_reached_goal), np.array(p.x_seq).tobytes(), \
        np.array(p.goal).tobytes(), p._engine.footprint()


def _compare(fleet, twins, where):
    for k, ((_, p), (_, q)) in enumerate(zip(fleet, twins)):
        assert bool(p.plan_reached_goal) == bool(q.plan_reached_goal) and np.array_equal(p.goal, q.goal), (where, k)
        assert np.array_equal(np.array(p.goal_region), np.array(q.goal_region)), (where, k)
        if k == NEVER:
            assert p.tree is None and q.tree is None and not hasattr(p, "node_seq"), (where, k)
            continue
        _same_planner(p, q, (where, k))
        assert np.array_equal(p._grown_goal, q._grown_goal) and p.tree._host_nodes() == q.tree._host_nodes(), (where, k)
        # the engine's own goal and box are the twin's: the tree-wide question has the twin's answer
        assert p._engine.connect_search(p.horizon_iters, cr.NO_INCUMBENT) == q._engine.connect_search(q.horizon_iters, cr.NO_INCUMBENT), (where, k)


def test_fleet_goal_costs_and_retargets_are_every_planners_own(monkeypatch):
    import lqrrt_amd
    from lqrrt_amd.engine import Engine
    fleet, twins = _fleet(), _fleet()
    planners = [p for _, p in fleet]
    n = len(fleet)
    s0, q0 = twins[0]
    assert all(not q.plan_reached_goal for _, q in twins) and [q._engine.size for _, q in twins[:NEVER]] == [216, 214, 217, 215]
    _compare(fleet, twins, "grown")                                 # the twins are twins

    # the berths: states of nodes of tree 0 off its plan (the first ones with a winner there), the cars' own goal, a far place
    ref0 = _reach_of(s0, q0)
    picks = _off_plan_targets(s0, q0, ref0, want=3)
    own = np.array(s0.goal, dtype=np.float64)
    far = own.copy()
    far[0] += 1e4
    goals = np.array([ref0.states[k] for k in picks] + [own, far])
    T = len(goals)

    solo = []

    def never(self, *a, **kw):
        solo.append(1)
        raise AssertionError("a solo reach call ran")
    calls = {"search": 0, "commit": 0}
    search, commit = Engine.reach_search_multi, Engine.reach_commit_multi

    def counted_search(*a, **kw):
        calls["search"] += 1
        return search(*a, **kw)

    def counted_commit(*a, **kw):
        calls["commit"] += 1
        return commit(*a, **kw)

    # ---- the matrix
    before = [_snapshot(p) for p in planners]
    monkeypatch.setattr(Engine, "reach_search", never)
    monkeypatch.setattr(Engine, "reach_search_multi", staticmethod(counted_search))
    steps, start = lqrrt_amd.fleet_goal_costs(planners, goals)
    bufs = np.abs(np.asarray(s0.goal_buffer, dtype=np.float64))[None, :] * np.array([1.0, 0.5, 1.0, 0.25, 1.0])[:T, None]
    lists = [list(range(0, 216, 2)), None, [], list(range(215))[::-1], [0]]
    steps2, start2 = lqrrt_amd.fleet_goal_costs(planners, goals, bufs, goal_tries=4, nodes=lists)
    monkeypatch.undo()
    assert not solo and calls["search"] == 2                        # one batched search call per matrix: the cars are one group
    print("steps:\n%s\nnodes:\n%s" % (steps, start))
    assert [_snapshot(p) for p in planners] == before               # reads only
    for m in (steps, start, steps2, start2):
        assert m.shape == (n, T) and m.dtype == np.int64
    for k, (_, q) in enumerate(twins):
        want, want2 = q.goal_costs(goals), q.goal_costs(goals, bufs, 4, lists[k])
        if k == NEVER:
            assert want is None and want2 is None
            assert np.all(steps[k] == -1) and np.all(start[k] == -1) and np.all(steps2[k] == -1) and np.all(start2[k] == -1)
            continue
        assert np.array_equal(steps[k], want[0]) and np.array_equal(start[k], want[1]), k
        assert np.array_equal(steps2[k], want2[0]) and np.array_equal(start2[k], want2[1]), k
    assert np.all(steps2[2] == -1)                                  # an empty id list
    assert (steps[0, :3] >= 0).any() and np.all(steps[:NEVER, T - 1] == -1)      # row 0 has winners; nobody reaches the far place
    row0 = ref0.search(goals)                                       # and row 0 is the reference's
    assert steps[0].tolist() == [-1 if w is None else w[0] for w in row0] and start[0].tolist() == [-1 if w is None else w[1] for w in row0]

    # ---- the retargets: 0 to its cheapest berth, 1 to the goal its tree was grown for (connect_goals' route), 2 to the far place
    # (False, nothing changes), 3 sits out, 4 never planned
    best = min((t for t in range(3) if steps[0, t] >= 0), key=lambda t: (steps[0, t], t))
    new = [goals[best], own, far, None, goals[best]]
    before = [_snapshot(p) for p in planners]
    monkeypatch.setattr(Engine, "reach_search", never)
    monkeypatch.setattr(Engine, "reach_commit", never)
    monkeypatch.setattr(Engine, "connect_search", never)
    monkeypatch.setattr(Engine, "reach_search_multi", staticmethod(counted_search))
    monkeypatch.setattr(Engine, "reach_commit_multi", staticmethod(counted_commit))
    got = lqrrt_amd.retargets(planners, new)
    monkeypatch.undo()
    assert not solo and calls == {"search": 3, "commit": 1}         # one search and one commit call for the group
    want = [False if g is None else q.retarget(g) for (_, q), g in zip(twins, new)]
    print("retargeted:", got)
    assert got == want and got[0] is True and got[2:] == [False, False, False]
    _compare(fleet, twins, "retargeted")
    after = [_snapshot(p) for p in planners]
    assert after[2:] == before[2:] and after[0] != before[0]        # False: everything unchanged, planner.goal included
    p0 = planners[0]
    assert np.array_equal(p0.goal, goals[best]) and p0.plan_reached_goal and p0.T == steps[0, best] * p0.dt
    assert p0._in_goal(p0.x_seq[-1]) and p0.node_seq[-1] >= 216

    # ---- the calls that follow run against the new goals
    assert lqrrt_amd.connect_goals(planners) == [q.connect_goal() for _, q in twins]
    _compare(fleet, twins, "connected")
    assert lqrrt_amd.refine_plans(planners) == [q.refine_plan() for _, q in twins]
    _compare(fleet, twins, "refined")
    again, _ = lqrrt_amd.fleet_goal_costs(planners, goals[best:best + 1])
    assert 0 <= again[0, 0] <= steps[0, best]                       # the berth is now planner 0's goal, and no farther than it was

    # ---- what is refused is refused for every planner before any is touched
    before = [_snapshot(p) for p in planners]
    with pytest.raises(ValueError, match="twice"):
        lqrrt_amd.retargets([p0, planners[1], p0], [own] * 3)
    with pytest.raises(ValueError, match="per planner"):
        lqrrt_amd.retargets(planners, [own] * (n - 1))
    with pytest.raises(ValueError, match="dimensionality"):
        lqrrt_amd.retargets(planners, [own] * (n - 1) + [own[:-1]])
    with pytest.raises(ValueError, match="negative"):
        lqrrt_amd.fleet_goal_costs(planners, goals, -bufs - 1.0)
    hand = planners[2]
    hand.tree.add_node(0, hand.tree.state[0], None, [hand.tree.state[0]], [np.zeros(hand.ncontrols)])
    with pytest.raises(ValueError, match="add_node"):
        lqrrt_amd.retargets(planners, [own] * n)
    with pytest.raises(ValueError, match="add_node"):
        lqrrt_amd.fleet_goal_costs(planners, goals)
    hand.tree._drop_host_tail()
    assert [_snapshot(p) for p in planners] == before


def test_retargets_finish_on_goal_id_lists_and_capacity():
    """finish_on_goal=True and per-planner id lists against the twins' own calls; a full tree gets False while the other commits."""
    import lqrrt_amd
    from test_connect_gpu import _fill

    def small():
        return [_car_planner(215, **STILL), _car_planner(215, **STILL), _car_planner(213, **STILL)]
    fleet, twins = small(), small()
    planners = [p for _, p in fleet]
    s0, q0 = twins[0]
    ref0 = _reach_of(s0, q0)
    pick = _off_plan_targets(s0, q0, ref0, want=1)[0]
    goal = ref0.states[pick].copy()
    win = ref0.search(goal[None, :])[0]
    assert win is not None
    rest = [v for v in range(216) if v != win[1]]
    for (s, p) in (fleet[1], twins[1]):                             # planner 1's tree is full (the copies of the root are not candidates)
        _fill(p._engine, s.x0, p._engine.gains(0, 1)[0])
    nodes = [rest, list(range(216)), None]
    size1, seq1 = planners[1]._engine.size, list(planners[1].node_seq)
    got = lqrrt_amd.retargets(planners, [goal] * 3, goal_tries=6, nodes=nodes, finish_on_goal=True)
    want = [q.retarget(goal, 6, nodes[k], True) for k, (_, q) in enumerate(twins)]
    print("retargeted:", got)
    assert got == want and got[1] is False
    assert planners[1]._engine.size == size1 and planners[1].node_seq == seq1 and not np.array_equal(planners[1].goal, goal)
    for k, ((_, p), (_, q)) in enumerate(zip(fleet, twins)):
        _same_planner(p, q, k)
        assert np.array_equal(p.goal, q.goal) and bool(p.plan_reached_goal) == bool(q.plan_reached_goal), k
        assert p.tree._host_nodes() == q.tree._host_nodes(), k


def test_fleet_assign_example_runs():
    """examples/fleet_assign_gpu.py: update_plans, one fleet_goal_costs matrix, a greedy assignment, one retargets call."""
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "fleet_assign_gpu.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert re.search(r"fleet_goal_costs, 4 cars x 5 berths in [0-9.]+ ms", out.stdout), out.stdout[-2000:]
    pairs = re.findall(r"(\d+) -> (\d+)", out.stdout[out.stdout.index("assignment"):].splitlines()[0])
    assert pairs and len(set(b for _, b in pairs)) == len(pairs)    # every berth at most once
    moved = re.findall(r"car (\d+): berth (\d+), reached goal: True, T = ([0-9.]+) s \(the matrix said ([0-9.]+) s\)", out.stdout)
    assert moved and all((c, b) in pairs and T == said for c, b, T, said in moved), out.stdout[-2000:]
    assert re.search(r"^refine_plans toward the new goals", out.stdout, flags=re.M)
