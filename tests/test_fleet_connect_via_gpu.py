"""
Fleet goal chains through waypoints: lqrrt_amd.connect_vias (one batched search call and one batched commit call per group,
Engine.connect_via_search_multi / connect_via_commit_multi) against the same planners connecting one by one (Planner.connect_via),
BIT FOR BIT.  The planners are grown by the recipe of tests/test_connect_gpu.py::_car_planner (seed 1, a clock that stands still,
ended by the node limit), so a fleet and its twins hold identical trees; the waypoints are the plan of a planner grown with the same
seed to its first goal hit, from the first node that the smaller tree does not hold.
"""
import functools

import numpy as np
import pytest

import connect_via_reference as cvr
from test_connect_gpu import _car_planner
from test_fleet_connect_gpu import _make, _grown, _snapshot, STILL, FIRST
from test_fleet_refine_gpu import _same_planner

pytestmark = pytest.mark.gpu

NEVER = 5
SIZES = [215, 216, 107, 149]                                        # the cars' node budgets, all below seed 1's first goal hit (node 217)
BOATS = [106, 104]                                                  # below the fixture's first goal node (107)


@functools.lru_cache(maxsize=None)
def _long_plans():
    """(node ids, states) of the plans that reach the goal first, car and boat, seed 1; read-only."""
    out = {}
    for name, (s, p) in (("car", _car_planner(3000, seed=1, **FIRST)), ("boat_novice", _grown("boat_novice", 3000, **FIRST))):
        assert p.plan_reached_goal
        way = p.plan_waypoints()
        assert len(way) == len(p.node_seq) and np.array_equal(way[-1], np.asarray(p.tree.state)[p.node_seq[-1]])
        way.setflags(write=False)
        out[name] = ([int(v) for v in p.node_seq], way)
    return out


def _waypoints(name, size):
    """The long plan's states from its first node that a tree of `size` nodes does not hold."""
    ids, way = _long_plans()[name]
    start = next(k for k, v in enumerate(ids) if v >= size)
    assert len(ids) - start >= 1
    return way[start:]


def _fleet():
    """Cars: four fallback plans below the first goal hit (one of them, 107, so far below that no goal chain reaches), a plan that
    reached the goal, one that never planned.  Boats: two fallback plans."""
    return ([_car_planner(n, **STILL) for n in SIZES] + [_car_planner(3000, seed=1, **FIRST), _make("car")]
            + [_grown("boat_novice", n, **STILL) for n in BOATS])


def _tables(fleet):
    """One waypoint table per planner: what its tree lacks of the long plan; the planner that reached the goal gets the whole plan
    (every state of it is a node of its own tree), the one that never planned gets one too (it takes part in nothing)."""
    ways = []
    for k, (s, p) in enumerate(fleet):
        name = "car" if k <= NEVER else "boat_novice"
        if k == NEVER or p.plan_reached_goal:
            ways.append(_long_plans()[name][1])
        else:
            ways.append(_waypoints(name, p._engine.size))
    return ways


def _reference(s, p):
    eng = p._engine
    return cvr.ViaConnector(s, eng.states(), eng.gains(), eng.parents(), eng.edge_lengths(), p.horizon_iters)


def _reference_winner(s, p, way):
    """What the rule gives on the planner's own tree (connect_via's arguments: the plan without its finish node as incumbent)."""
    ref = _reference(s, p)
    core = [v for v in p.node_seq if v < p._engine.size]
    return ref.search_via(way, incumbent=ref.cost(core) if p.plan_reached_goal else cvr.NO_INCUMBENT)


def _compare(fleet, twins, where):
    for k, ((_, p), (_, q)) in enumerate(zip(fleet, twins)):
        assert bool(p.plan_reached_goal) == bool(q.plan_reached_goal), (where, k)
        if k == NEVER:
            assert p.tree is None and q.tree is None and not hasattr(p, "node_seq"), (where, k)
            continue
        _same_planner(p, q, (where, k))
        assert p.tree._host_nodes() == q.tree._host_nodes(), (where, k)


def test_connect_vias_is_every_planners_own_connect_via(monkeypatch):
    import lqrrt_amd
    from lqrrt_amd.engine import Engine
    fleet, twins = _fleet(), _fleet()
    n = len(fleet)
    _compare(fleet, twins, "grown")                                 # the twins are twins
    ways = _tables(twins)
    sizes = [None if k == NEVER else q._engine.size for k, (_, q) in enumerate(twins)]

    # conditions on the inputs, from the reference of the rule on the twins' trees
    wins = [None if k == NEVER else _reference_winner(s, q, ways[k]) for k, (s, q) in enumerate(twins)]
    print("reference winners:", [None if w is None else w[:3] for w in wins], "Q:", [len(w) for w in ways])
    fallback = [k for k, (_, q) in enumerate(twins) if k != NEVER and not q.plan_reached_goal]
    cars, boats = [k for k in fallback if k < NEVER], [k for k in fallback if k > NEVER]
    assert cars == [0, 1, 2, 3] and boats == [6, 7] and twins[4][1].plan_reached_goal
    assert sum(1 for k in cars if wins[k] is not None) >= 2                    # fallback plans with a winner
    rescued = [k for k in fallback if wins[k] is not None and _reference(*twins[k]).search() is None]
    print("found through waypoints only:", rescued)
    assert rescued                                                             # the waypoint rule finds a plan, the Q = 0 rule none
    assert any(wins[k] is not None for k in boats)                             # the second group has a winner

    calls, solo = [], []
    search = Engine.connect_via_search_multi

    def counted(engines, *a, **kw):
        engines = list(engines)
        calls.append(type(engines[0].system).__name__)
        return search(engines, *a, **kw)

    def never(self, *a, **kw):
        solo.append(1)
        raise AssertionError("a solo search ran")
    monkeypatch.setattr(Engine, "connect_via_search_multi", staticmethod(counted))
    monkeypatch.setattr(Engine, "connect_via_search", never)
    got = lqrrt_amd.connect_vias([p for _, p in fleet], ways)
    monkeypatch.undo()
    assert not solo                                                 # nobody's own search ran
    assert len(calls) == 2 and len(set(calls)) == 2                 # one search call per group
    want = [q.connect_via(w) for (_, q), w in zip(twins, ways)]
    print("connected:", got)
    assert got == want == [w is not None for w in wins]
    _compare(fleet, twins, "connected")
    for k, (s, p) in enumerate(fleet):
        if got[k]:
            assert p.plan_reached_goal
            core = [v for v in p.node_seq if v < p._engine.size]
            assert len(p.tree.trajectory(core)[0]) == wins[k][0], k

    # a second call over the nodes first searched finds nothing below the plans it has just made (the appended nodes are new
    # candidates, which may do better: they are left out)
    before = [_snapshot(p) for _, p in fleet]
    first = [None if m is None else list(range(m)) for m in sizes]
    assert lqrrt_amd.connect_vias([p for _, p in fleet], ways, nodes=first) == [False] * n
    assert [_snapshot(p) for _, p in fleet] == before

    # refine_plans works on the new plans as every twin's refine_plan does
    assert lqrrt_amd.refine_plans([p for _, p in fleet]) == [q.refine_plan() for _, q in twins]
    _compare(fleet, twins, "refined")

    # what is refused is refused for every planner before any is touched
    before = [_snapshot(p) for _, p in fleet]
    everybody = [p for _, p in fleet]
    p0 = fleet[0][1]
    with pytest.raises(ValueError, match="twice"):
        lqrrt_amd.connect_vias([p0, fleet[2][1], p0], ways[:3])
    with pytest.raises(ValueError, match="per planner"):
        lqrrt_amd.connect_vias(everybody, ways[:-1])
    with pytest.raises(ValueError, match="per planner"):
        lqrrt_amd.connect_vias(everybody, ways, nodes=[None] * (n - 1))
    with pytest.raises(ValueError, match="shape"):
        lqrrt_amd.connect_vias(everybody, ways[:-1] + [np.zeros((2, 1))])
    with pytest.raises(ValueError, match="goal_tries"):
        lqrrt_amd.connect_vias(everybody, ways, goal_tries=0)
    s1, moved = fleet[1]
    goal = np.array(s1.goal, dtype=np.float64)
    moved.set_goal(goal + 1.0)
    with pytest.raises(ValueError, match="goal changed"):
        lqrrt_amd.connect_vias(everybody, ways)
    moved.set_goal(goal)
    moved.plan_reached_goal = before[1][3]                          # (set_goal clears it: back to what the snapshot holds)
    hand = fleet[2][1]
    hand.tree.add_node(0, hand.tree.state[0], None, [hand.tree.state[0]], [np.zeros(hand.ncontrols)])
    with pytest.raises(ValueError, match="add_node"):
        lqrrt_amd.connect_vias(everybody, ways)
    hand.tree._drop_host_tail()
    assert [_snapshot(p) for _, p in fleet] == before


def test_fleet_connect_via_example_runs():
    """examples/fleet_connect_via_gpu.py: a tick that finds plans, a second on a tenth of the budget that mostly does not,
    connect_vias over the saved plans, refine_plans."""
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "fleet_connect_via_gpu.py")], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    reach = {m.group(1): int(m.group(2)) for m in re.finditer(
        r"^(tick one: update_plans|tick two: update_plans|connect_vias|refine_plans)\b.*?: (\d+) of \d+ plans reach the goal",
        out.stdout, flags=re.M)}
    assert set(reach) == {"tick one: update_plans", "tick two: update_plans", "connect_vias", "refine_plans"}, out.stdout[-2000:]
    assert reach["tick two: update_plans"] < reach["tick one: update_plans"], out.stdout[-2000:]
    assert reach["tick two: update_plans"] < reach["connect_vias"] == reach["refine_plans"], out.stdout[-2000:]
