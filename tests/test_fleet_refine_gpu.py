"""
Fleet refinement: lqrrt_amd.refine_plans (one batched search launch and one batched commit launch per round and group,
Engine.refine_round_multi / refine_commit_multi) against the same planners refining one by one (Planner.refine_plan), BIT FOR BIT.
The planners are grown as tests/test_refine_gpu.py::_planner grows them (min_time 0: the plan ends at its first goal hit), but with the
clock standing still, so nothing depends on the host's speed and a fleet and its twins hold identical trees.
"""
import numpy as np
import pytest

from test_refine_gpu import _check_plan, _fill, _reference_of

pytestmark = pytest.mark.gpu

SEEDS = range(1, 7)


def _grow(name, seed, finish=False, max_nodes=3000):
    import lqrrt_amd
    s = lqrrt_amd.systems.SYSTEMS[name](0)
    cons = lqrrt_amd.Constraints(s.nstates, s.ncontrols, s.goal_buffer, s.is_feasible)
    p = lqrrt_amd.Planner(s.dynamics, s.lqr, cons, error_tol=s.error_tol, erf=s.erf, goal0=s.goal, printing=False,
                          min_time=0.0, max_time=10, max_nodes=max_nodes, wave_size=256, sys_time=lambda: 0.0, **s.plan_kwargs)
    np.random.seed(seed)
    p.update_plan(s.x0, s.sample_space, goal_bias=s.goal_bias, finish_on_goal=finish)
    return s, p


def _fleet():
    """Cars and boats, seeds 1-6 each; two cars finish on the goal; a seventh car's tree is too small to reach the goal."""
    fleet = [_grow("car", seed, finish=(seed in (2, 5))) for seed in SEEDS]
    fleet.append(_grow("car", 1, max_nodes=40))
    fleet += [_grow("boat_novice", seed) for seed in SEEDS]
    return fleet


def _same_planner(p, q, where):
    assert list(p.node_seq) == list(q.node_seq), where
    assert np.array_equal(np.array(p.x_seq), np.array(q.x_seq)) and np.array_equal(np.array(p.u_seq), np.array(q.u_seq)), where
    assert p.T == q.T and p.tree.size == q.tree.size and p._engine.size == q._engine.size, where
    assert np.array_equal(p.t_seq, q.t_seq), where
    beyond = len(p.x_seq) * p.dt + 1.0
    assert np.array_equal(p.get_state(beyond), q.get_state(beyond)) and np.array_equal(p.get_state(beyond), p.x_seq[-1]), where
    assert np.array_equal(p.get_effort(0.5 * p.T), q.get_effort(0.5 * q.T)), where
    assert np.array_equal(p._engine.states(), q._engine.states()) and np.array_equal(p._engine.parents(), q._engine.parents()), where
    assert np.array_equal(p._engine.gains(), q._engine.gains()), where
    assert np.array_equal(p._engine.edge_lengths(), q._engine.edge_lengths()), where


def test_refine_plans_is_every_planners_own_refine_plan(monkeypatch):
    import lqrrt_amd
    from lqrrt_amd.engine import Engine
    fleet, twins = _fleet(), _fleet()
    n = len(fleet)
    for k, ((_, p), (_, q)) in enumerate(zip(fleet, twins)):                     # the twins are twins
        assert p.plan_reached_goal == q.plan_reached_goal
        if p.plan_reached_goal:
            _same_planner(p, q, k)
    stuck = len(SEEDS)
    assert not fleet[stuck][1].plan_reached_goal                                 # nothing to refine: never part of a launch
    reached = [bool(p.plan_reached_goal) for _, p in fleet]
    assert sum(reached[:stuck]) >= 2 and sum(reached[stuck + 1:]) >= 2
    finishers = [k for k, (_, p) in enumerate(fleet) if reached[k] and p.node_seq[-1] >= p._engine.size]
    assert finishers and set(finishers) <= {1, 4}                                # a goal node that lives on the host

    # conditions on the inputs, from the reference of the rule: somebody accepts a round, and planners stop at different rounds
    expected = [len(_reference_of(s, p)[1][1]) if p.plan_reached_goal else 0 for s, p in twins]
    print("reference rounds per planner:", expected)
    assert max(expected) >= 1 and len(set(expected)) >= 2

    calls, solo = [], []
    search = Engine.refine_round_multi

    def counted(engines, *a, **kw):
        engines = list(engines)
        calls.append(type(engines[0].system).__name__)
        return search(engines, *a, **kw)
    monkeypatch.setattr(Engine, "refine_round_multi", staticmethod(counted))
    monkeypatch.setattr(Engine, "refine_round", lambda self, *a, **kw: solo.append(1))
    got = lqrrt_amd.refine_plans([p for _, p in fleet])
    monkeypatch.undo()
    assert not solo                                                              # nobody's own search ran
    want = [q.refine_plan() for _, q in twins]
    print("accepted rounds:", got)
    assert got == want == expected
    for k, ((s, p), (_, q)) in enumerate(zip(fleet, twins)):
        if p.plan_reached_goal:
            _same_planner(p, q, k)
            _check_plan(s, p, finish=(k in finishers))
        assert p.plan_reached_goal == q.plan_reached_goal
    # one search launch per round and group: the slowest planner's accepted rounds + the round that finds nothing (max_rounds at most)
    groups = {}
    for k, (s, p) in enumerate(fleet):
        if p.plan_reached_goal:
            groups.setdefault(type(s).__name__, []).append(min(got[k] + 1, 8))
    assert len(calls) == sum(max(v) for v in groups.values()), (calls, groups)
    assert len(set(calls)) == len(groups) == 2

    # at the fix-point: a second call changes nothing
    before = [(list(p.node_seq), p.T, p.tree.size) for _, p in fleet]
    assert lqrrt_amd.refine_plans([p for _, p in fleet]) == [0] * n
    assert [(list(p.node_seq), p.T, p.tree.size) for _, p in fleet] == before

    # what is refused is refused for every planner before any is touched
    p0 = fleet[0][1]
    with pytest.raises(ValueError, match="twice"):
        lqrrt_amd.refine_plans([p0, fleet[2][1], p0])
    hand = fleet[2][1]
    hand.tree.add_node(0, hand.tree.state[0], None, [hand.tree.state[0]], [np.zeros(hand.ncontrols)])
    with pytest.raises(ValueError, match="add_node"):
        lqrrt_amd.refine_plans([p for _, p in fleet])
    assert [(list(p.node_seq), p.T) for _, p in fleet] == [(b[0], b[1]) for b in before]


def test_refine_plans_max_rounds_and_capacity():
    """max_rounds caps every planner; a planner whose tree is full stops with what it has while the others go on."""
    import lqrrt_amd
    seeds = (1, 2, 3, 4)
    fleet = [_grow("car", seed) for seed in seeds]
    twins = [_grow("car", seed) for seed in seeds]
    would = [len(_reference_of(s, q)[1][1]) for s, q in twins]
    assert sum(1 for v in would if v >= 1) >= 2, would              # (a condition on the inputs)
    full = max(k for k, v in enumerate(would) if v >= 1)             # this one would accept a round, had its tree the room
    for group in (fleet, twins):
        s, p = group[full]
        _fill(p._engine, s.x0, p._engine.gains(0, 1)[0])
    plan0, T0 = list(fleet[full][1].node_seq), fleet[full][1].T
    got = lqrrt_amd.refine_plans([p for _, p in fleet], max_rounds=1)
    assert got == [q.refine_plan(max_rounds=1) for _, q in twins]
    assert got == [0 if k == full else min(v, 1) for k, v in enumerate(would)]
    assert list(fleet[full][1].node_seq) == plan0 and fleet[full][1].T == T0
    for k, ((_, p), (_, q)) in enumerate(zip(fleet, twins)):
        _same_planner(p, q, k)


def test_fleet_tick_replan_refine_replan():
    """update_plans with roots -> refine_plans -> update_plans with roots, against replan / refine_plan / replan per planner."""
    import lqrrt_amd
    from test_retain_gpu import _planner
    n, max_nodes = 4, 2500
    fleet = [(s, _planner(s, max_nodes=max_nodes)) for s in (lqrrt_amd.systems.BoatAdvanced(0) for _ in range(n))]
    twins = [(s, _planner(s, max_nodes=max_nodes)) for s in (lqrrt_amd.systems.BoatAdvanced(0) for _ in range(n))]
    job = lambda s, p, **kw: dict(planner=p, sample_space=s.sample_space, goal_bias=s.goal_bias, **kw)
    lqrrt_amd.update_plans([job(s, p, x0=s.x0, seed=11 + k) for k, (s, p) in enumerate(fleet)])
    for k, (s, q) in enumerate(twins):
        np.random.seed(11 + k)
        q.update_plan(s.x0, s.sample_space, goal_bias=s.goal_bias)
    rounds = []
    for tick in range(2):
        roots = [p.plan_node_after(0.2 * p.T)[1] for _, p in fleet]
        res = lqrrt_amd.update_plans([job(s, p, root=r, seed=21 + 10 * tick + k) for k, ((s, p), r) in enumerate(zip(fleet, roots))])
        res2 = []
        for k, ((s, q), r) in enumerate(zip(twins, roots)):
            np.random.seed(21 + 10 * tick + k)
            res2.append(q.replan(r, s.sample_space, goal_bias=s.goal_bias))
        assert res == res2
        if tick == 0:
            rounds = lqrrt_amd.refine_plans([p for _, p in fleet])
            assert rounds == [q.refine_plan() for _, q in twins]
            print("accepted rounds:", rounds)
        for k, ((_, p), (_, q)) in enumerate(zip(fleet, twins)):
            assert p.plan_reached_goal == q.plan_reached_goal and p.retained == q.retained
            if p.plan_reached_goal:
                _same_planner(p, q, (tick, k))
    assert any(p.plan_reached_goal for _, p in fleet)


def test_fleet_refine_example_runs():
    """examples/fleet_refine_gpu.py: real clock, four boats, two ticks of update_plans with roots followed by refine_plans."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "fleet_refine_gpu.py"), "4", "2"], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("tick ") and "refined in" in l]
    assert len(lines) == 2, out.stdout[-2000:]
