"""
Fleet replanning (lqrrt_amd.update_plans jobs with a `root`) on the CPU: which jobs are refused, and that a refused call
leaves every planner of the call as it was.  The trees themselves are compared on the device, bit for bit, in
tests/test_retain_multi_gpu.py and tests/test_fleet_replan_gpu.py.
"""
import pytest

import lqrrt_amd
from lqrrt_amd import _native as nat


def _fleet(n=3):
    boat = lqrrt_amd.systems.BoatAdvanced(0)
    cons = lqrrt_amd.Constraints(6, 3, boat.goal_buffer, boat.is_feasible)
    kw = dict(error_tol=boat.error_tol, erf=boat.erf, goal0=boat.goal, printing=False, wave_size=256, **boat.plan_kwargs)
    return boat, [lqrrt_amd.Planner(boat.dynamics, boat.lqr, cons, **kw) for _ in range(n)]


def _snapshot(p):
    return (p.tree, p._engine, p._engine_key, getattr(p, "retained", "unset"), getattr(p, "node_seq", "unset"),
            getattr(p, "_grown_with", "unset"), getattr(p, "xguide", "unset"), p.stats, p.killed)


def _refused(planners, jobs, error, match=None):
    before = [_snapshot(p) for p in planners]
    with pytest.raises(error, match=match):
        lqrrt_amd.update_plans(jobs)
    for p, was in zip(planners, before):
        now = _snapshot(p)
        assert all(a is b or a == b for a, b in zip(now, was))


def test_a_job_gives_exactly_one_of_x0_and_root():
    boat, (a, b, c) = _fleet()
    ok = lambda p: dict(planner=p, x0=boat.x0, sample_space=boat.sample_space, goal_bias=boat.goal_bias, seed=1)
    both = dict(planner=b, x0=boat.x0, root=0, sample_space=boat.sample_space, goal_bias=boat.goal_bias, seed=2)
    neither = dict(planner=b, sample_space=boat.sample_space, goal_bias=boat.goal_bias, seed=2)
    _refused([a, b, c], [ok(a), both, ok(c)], ValueError, "exactly one of x0 and root")
    _refused([a, b, c], [ok(a), neither, ok(c)], ValueError, "exactly one of x0 and root")
    # `revalidate` says how a kept tree is treated: it has no meaning for a job that starts from x0
    _refused([a, b], [ok(a), dict(ok(b), revalidate=False)], ValueError, "revalidate")
    # ... and an unknown key is still an unknown key
    _refused([a, b], [ok(a), dict(ok(b), roots=0)], ValueError, "unknown job key")


def test_root_without_a_previous_plan_is_replans_refusal():
    boat, (a, b, c) = _fleet()
    rooted = lambda p, **kw: dict(planner=p, root=0, sample_space=boat.sample_space, goal_bias=boat.goal_bias, **kw)
    fresh = dict(planner=a, x0=boat.x0, sample_space=boat.sample_space, goal_bias=boat.goal_bias, seed=1)
    _refused([a, b, c], [fresh, rooted(b, seed=2), rooted(c, seed=3, revalidate=False)], RuntimeError, "no tree to keep")
    _refused([b], [rooted(b)], RuntimeError, "no tree to keep")
    # the message is replan's own
    with pytest.raises(RuntimeError) as solo:
        b.replan(0, boat.sample_space, goal_bias=boat.goal_bias)
    with pytest.raises(RuntimeError) as fleet:
        lqrrt_amd.update_plans([rooted(b)])
    assert str(solo.value) == str(fleet.value)
    # the other rules of a call come first or later, but they still hold for jobs with a root
    _refused([a, b], [fresh, rooted(b), rooted(b)], ValueError, "appears twice")
    _refused([b], [rooted(b, xrand_gen="nonsense")], ValueError, "xrand_gen")


def test_binding_and_wrapper_exist():
    assert "lqrrt_tree_retain_multi" in nat.SIGNATURES
    assert hasattr(nat.lib(), "lqrrt_tree_retain_multi")
    assert hasattr(lqrrt_amd.engine.Engine, "tree_retain_multi")
    with pytest.raises(ValueError):
        lqrrt_amd.engine.Engine.tree_retain_multi([], [])
