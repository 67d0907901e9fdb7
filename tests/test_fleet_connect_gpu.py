"""
Fleet goal connection: lqrrt_amd.connect_goals (one batched search call and one batched commit call per group,
Engine.connect_search_multi / connect_commit_multi) against the same planners connecting one by one (Planner.connect_goal), BIT FOR
BIT.  The planners are grown by the recipe of tests/test_connect_gpu.py::_car_planner (seed 1, a clock that stands still, ended by the
node limit), so a fleet and its twins hold identical trees.
"""
import numpy as np
import pytest

import connect_reference as cr
from test_connect_gpu import _car_planner, _reference_of
from test_fleet_refine_gpu import _same_planner

pytestmark = pytest.mark.gpu


def _make(name, **kw):
    import lqrrt_amd
    s = lqrrt_amd.systems.SYSTEMS[name](0)
    cons = lqrrt_amd.Constraints(s.nstates, s.ncontrols, s.goal_buffer, s.is_feasible)
    return s, lqrrt_amd.Planner(s.dynamics, s.lqr, cons, error_tol=s.error_tol, erf=s.erf, goal0=s.goal, printing=False,
                                **dict(s.plan_kwargs, **kw))


def _grown(name, max_nodes, finish=False, seed=1, **kw):
    """_car_planner's recipe for any native system."""
    s, p = _make(name, max_nodes=max_nodes, wave_size=256, **kw)
    np.random.seed(seed)
    p.update_plan(s.x0, s.sample_space, goal_bias=s.goal_bias, xrand_gen=10, finish_on_goal=finish)
    return s, p


STILL = dict(min_time=2, max_time=3, sys_time=lambda: 0.0)          # the budget is the node limit
FIRST = dict(min_time=0.0, max_time=10, sys_time=lambda: 0.0)       # the plan ends at its first goal hit


_FINISH_SEED = []


def _finish_seed():
    """The first seed whose car plan ends in a finish_on_goal node on the host (the force-arrive steer may produce nothing)."""
    if not _FINISH_SEED:
        for seed in range(1, 9):
            _, p = _car_planner(3000, finish=True, seed=seed, **FIRST)
            if p.plan_reached_goal and p.node_seq[-1] >= p._engine.size:
                _FINISH_SEED.append(seed)
                break
        else:
            pytest.fail("no finish_on_goal plan of the car in 8 seeds")
    return _FINISH_SEED[0]


def _fleet():
    """Cars: three fallback plans just below the fixture's first goal node (217) and one far below, a plan that reached the goal, two
    grown with finish_on_goal (one of them ends in a finish node), one that never planned.  Boats: two fallback plans below the
    fixture's first goal node (107)."""
    fleet = [_car_planner(215, **STILL), _car_planner(213, **STILL), _car_planner(216, **STILL), _car_planner(149, **STILL),
             _car_planner(3000, seed=1, **FIRST), _car_planner(3000, finish=True, seed=_finish_seed(), **FIRST),
             _car_planner(3000, finish=True, seed=_finish_seed() % 8 + 1, **FIRST), _make("car"),
             _grown("boat_novice", 106, **STILL), _grown("boat_novice", 104, **STILL)]
    return fleet


NEVER = 7


def _snapshot(p):
    if getattr(p, "node_seq", None) is None:
        return None
    return list(p.node_seq), p.T, p.tree.size, bool(p.plan_reached_goal), np.array(p.x_seq).tobytes()


def _reference_winner(s, p):
    """What the rule gives on the planner's own tree (connect_goal's arguments: the plan without its finish node as incumbent)."""
    eng = p._engine
    ref = _reference_of(s, p)
    core = [v for v in p.node_seq if v < eng.size]
    return ref.search(incumbent=ref.cost(core) if p.plan_reached_goal else cr.NO_INCUMBENT)


def _compare(fleet, twins, where):
    for k, ((_, p), (_, q)) in enumerate(zip(fleet, twins)):
        assert bool(p.plan_reached_goal) == bool(q.plan_reached_goal), (where, k)
        if k == NEVER:
            assert p.tree is None and q.tree is None and not hasattr(p, "node_seq"), (where, k)
            continue
        _same_planner(p, q, (where, k))
        assert p.tree._host_nodes() == q.tree._host_nodes(), (where, k)


def test_connect_goals_is_every_planners_own_connect_goal(monkeypatch):
    import lqrrt_amd
    from lqrrt_amd.engine import Engine
    fleet, twins = _fleet(), _fleet()
    n = len(fleet)
    _compare(fleet, twins, "grown")                                 # the twins are twins

    # conditions on the inputs, from the reference of the rule on the twins' trees
    wins = [None if k == NEVER else _reference_winner(s, q) for k, (s, q) in enumerate(twins)]
    print("reference winners:", [None if w is None else w[:2] for w in wins])
    fallback = [k for k, (_, q) in enumerate(twins) if k != NEVER and not q.plan_reached_goal]
    cars, boats = [k for k in fallback if k < NEVER], [k for k in fallback if k > NEVER]
    assert 0 in cars and sum(1 for k in cars if wins[k] is not None) >= 2      # fallback plans with a winner (215: the pinned one)
    assert 3 in cars and wins[3] is None                                       # a fallback plan without one
    assert twins[4][1].plan_reached_goal and twins[4][1].node_seq[-1] < twins[4][1]._engine.size
    finishers = [k for k in (5, 6) if twins[k][1].plan_reached_goal and twins[k][1].node_seq[-1] >= twins[k][1]._engine.size]
    assert finishers                                                           # a goal node that lives on the host
    assert boats and any(wins[k] is not None for k in boats)                   # the second group has a winner

    calls, solo = [], []
    search = Engine.connect_search_multi

    def counted(engines, *a, **kw):
        engines = list(engines)
        calls.append(type(engines[0].system).__name__)
        return search(engines, *a, **kw)

    def never(self, *a, **kw):
        solo.append(1)
        raise AssertionError("a solo search ran")
    monkeypatch.setattr(Engine, "connect_search_multi", staticmethod(counted))
    monkeypatch.setattr(Engine, "connect_search", never)
    got = lqrrt_amd.connect_goals([p for _, p in fleet])
    monkeypatch.undo()
    assert not solo                                                 # nobody's own search ran
    assert len(calls) == 2 and len(set(calls)) == 2                 # one search call per group
    want = [q.connect_goal() for _, q in twins]
    print("connected:", got)
    assert got == want == [w is not None for w in wins]
    _compare(fleet, twins, "connected")
    for k, (s, p) in enumerate(fleet):
        if got[k]:
            assert p.plan_reached_goal
            core = [v for v in p.node_seq if v < p._engine.size]
            assert len(p.tree.trajectory(core)[0]) == wins[k][0], k

    # a second call finds nothing below the plans it has just made
    before = [_snapshot(p) for _, p in fleet]
    assert lqrrt_amd.connect_goals([p for _, p in fleet]) == [False] * n
    assert [_snapshot(p) for _, p in fleet] == before

    # refine_plans works on the new plans as every twin's refine_plan does
    assert lqrrt_amd.refine_plans([p for _, p in fleet]) == [q.refine_plan() for _, q in twins]
    _compare(fleet, twins, "refined")

    # what is refused is refused for every planner before any is touched
    before = [_snapshot(p) for _, p in fleet]
    p0 = fleet[0][1]
    with pytest.raises(ValueError, match="twice"):
        lqrrt_amd.connect_goals([p0, fleet[2][1], p0])
    with pytest.raises(ValueError, match="per planner"):
        lqrrt_amd.connect_goals([p for _, p in fleet], nodes=[None] * (n - 1))
    s1, moved = fleet[1]
    goal = np.array(s1.goal, dtype=np.float64)
    moved.set_goal(goal + 1.0)
    with pytest.raises(ValueError, match="goal changed"):
        lqrrt_amd.connect_goals([p for _, p in fleet])
    moved.set_goal(goal)
    moved.plan_reached_goal = before[1][3]                          # (set_goal clears it: back to what the snapshot holds)
    hand = fleet[2][1]
    hand.tree.add_node(0, hand.tree.state[0], None, [hand.tree.state[0]], [np.zeros(hand.ncontrols)])
    with pytest.raises(ValueError, match="add_node"):
        lqrrt_amd.connect_goals([p for _, p in fleet])
    hand.tree._drop_host_tail()
    assert [_snapshot(p) for _, p in fleet] == before


def test_connect_goals_finish_on_goal_and_id_lists():
    """finish_on_goal=True and a per-planner `nodes` list, each against the twins' own calls."""
    import lqrrt_amd

    def small():
        return [_car_planner(215, **STILL), _car_planner(216, **STILL), _make("car"), _grown("boat_novice", 106, **STILL)]
    fleet, twins = small(), small()
    nodes = [[v for v in range(216) if v != 211], None, [0], list(range(107))[::-1]]
    win = _reference_of(*twins[0]).search(nodes=nodes[0])           # a condition on the inputs: the list without 211 has another winner
    assert win is not None and win[1] != 211
    got = lqrrt_amd.connect_goals([p for _, p in fleet], nodes=nodes, finish_on_goal=True)
    want = [q.connect_goal(nodes=nodes[k], finish_on_goal=True) for k, (_, q) in enumerate(twins)]
    print("connected:", got)
    assert got == want and got[2] is False and sum(got) >= 2
    assert got[0] and win[1] in fleet[0][1].node_seq
    for k, ((_, p), (_, q)) in enumerate(zip(fleet, twins)):
        if k == 2:
            assert p.tree is None
            continue
        _same_planner(p, q, k)
        assert p.tree._host_nodes() == q.tree._host_nodes(), k


def test_connect_goals_capacity():
    """A planner whose tree is full gets False and is unchanged; the others connect."""
    import lqrrt_amd
    from test_connect_gpu import _fill
    fleet = [_car_planner(215, **STILL), _car_planner(215, **STILL), _car_planner(216, **STILL)]
    s, full = fleet[1]
    _fill(full._engine, s.x0, full._engine.gains(0, 1)[0])
    seq, T, size = list(full.node_seq), full.T, full._engine.size
    got = lqrrt_amd.connect_goals([p for _, p in fleet], nodes=[None, list(range(216)), None])
    assert got == [True, False, True]
    assert full.node_seq == seq and full.T == T and full._engine.size == size and not full.plan_reached_goal
    assert fleet[0][1].plan_reached_goal and fleet[2][1].plan_reached_goal


def test_fleet_connect_example_runs():
    """examples/fleet_connect_gpu.py: budgets too small for a goal hit; update_plans, connect_goals, refine_plans."""
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "fleet_connect_gpu.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    reach = {m.group(1): int(m.group(2)) for m in re.finditer(r"^(update_plans|connect_goals|refine_plans)\b.*?: (\d+) of \d+ plans reach the goal",
                                                              out.stdout, flags=re.M)}
    assert set(reach) == {"update_plans", "connect_goals", "refine_plans"}, out.stdout[-2000:]
    assert reach["update_plans"] < reach["connect_goals"] == reach["refine_plans"], out.stdout[-2000:]
