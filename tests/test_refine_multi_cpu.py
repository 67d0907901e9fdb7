"""
Fleet refinement (lqrrt_amd.refine_plans, the *_multi refine kernels) on the CPU: the host side of the public function, and what
the compiler says about the two kernels whose grid spans several engines.  The device side is compared bit for bit in
tests/test_refine_multi_gpu.py and tests/test_fleet_refine_gpu.py.
"""
import os
import re
import shutil
import sys

import numpy as np
import pytest

import lqrrt_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _native_planner():
    car = lqrrt_amd.systems.Car(0)
    cons = lqrrt_amd.Constraints(car.nstates, car.ncontrols, car.goal_buffer, car.is_feasible)
    return lqrrt_amd.Planner(car.dynamics, car.lqr, cons, error_tol=car.error_tol, erf=car.erf, goal0=car.goal, printing=False,
                             **car.plan_kwargs)


def _callback_planner():
    cons = lqrrt_amd.Constraints(2, 1, [0.1, 0.1], lambda x, u: True)
    return lqrrt_amd.Planner(lambda x, u, dt: x + dt * np.array([x[1], u[0]]), lambda x, u: (np.eye(2), np.array([[1.0, 1.0]])), cons,
                             horizon=1, dt=0.1, goal0=[1.0, 0.0], printing=False)


def test_refine_plans_of_nobody():
    assert lqrrt_amd.refine_plans([]) == []
    import lqrrt
    assert lqrrt.refine_plans is lqrrt_amd.refine_plans


def test_refine_plans_without_plans_changes_nothing():
    a, b = _native_planner(), _native_planner()
    assert lqrrt_amd.refine_plans([a, b]) == [0, 0]                 # nothing to refine: no native call, no engine
    assert lqrrt_amd.refine_plans([a], max_rounds=3, goal_tries=2) == [0]
    assert a.tree is None and not hasattr(a, "node_seq")
    with pytest.raises(ValueError):
        lqrrt_amd.refine_plans([a, b], goal_tries=0)


def test_refine_plans_refuses_before_touching_anybody():
    a, b = _native_planner(), _native_planner()
    with pytest.raises(ValueError, match="twice"):
        lqrrt_amd.refine_plans([a, b, a])
    cb = _callback_planner()
    assert cb.callback_mode
    with pytest.raises(ValueError, match="Python"):
        lqrrt_amd.refine_plans([a, cb])
    with pytest.raises(ValueError):
        lqrrt_amd.refine_plans([a, object()])


def test_refine_plan_and_refine_plans_share_their_steps():
    """refine_plan calls the instance's own refine_round / refine_commit; the helpers both paths use exist on the planner."""
    for name in ("_refine_begin", "_refine_incumbent", "_refine_accept", "_refine_end"):
        assert callable(getattr(lqrrt_amd.Planner, name))
    src = open(os.path.join(ROOT, "lqrrt_amd", "planner.py")).read()
    body = src[src.index("    def refine_plan(self"):src.index("    def _refine_begin(self")]
    assert "eng.refine_round(" in body and "eng.refine_commit(" in body


def test_multi_kernels_keep_their_solo_twins_frame():
    """For every model S: k_refine_search_multi<S> / k_refine_commit_multi<S> exist and their private segment is no larger than
    that of k_refine_search<S> / k_refine_commit<S> -- the indirection through EngineProto and RefineDesc must not spill."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    if not shutil.which(kr.HIPCC) and not os.path.exists(kr.HIPCC):
        pytest.skip("hipcc not available")
    user = os.path.join(ROOT, "examples", "user_system", "unicycle.hpp")
    rows = kr.parse(kr.remarks(["-DLQRRT_USER_SYSTEM=\"%s\"" % user]))

    def by_model(kernel):
        out = {}
        for r in rows:
            m = re.match(r"void lq::%s<lq::(.+?) ?>\(" % kernel, r["name"])
            if m:
                out[m.group(1)] = r
        return out
    for stage in ("search", "commit"):
        solo, multi = by_model("k_refine_%s" % stage), by_model("k_refine_%s_multi" % stage)
        assert len(solo) >= 10 and "UserSystem" in solo, sorted(solo)
        assert sorted(multi) == sorted(solo)
        for model in solo:
            print("%-7s %-18s solo %4d B  multi %4d B  vgpr %3d / %3d" % (stage, model, solo[model]["scratch"], multi[model]["scratch"],
                                                                           solo[model]["vgpr"], multi[model]["vgpr"]))
        worse = {m: (solo[m]["scratch"], multi[m]["scratch"]) for m in solo if multi[m]["scratch"] > solo[m]["scratch"]}
        assert not worse, (stage, worse)


def test_refinement_stays_plain_launches():
    """One stream, plain launches: no cooperative launch, no grid-wide barrier in the refinement's kernels or its host code."""
    for f in ("refine.hpp", "engine_refine.hpp"):
        text = open(os.path.join(ROOT, "lqrrt_amd", "csrc", f)).read()
        for word in ("hipLaunchCooperativeKernel", "hipModuleLaunchCooperativeKernel", "cooperative_groups", "grid.sync", "this_grid"):
            assert word not in text, (f, word)
    src = open(os.path.join(ROOT, "lqrrt_amd", "csrc", "refine.hpp")).read()
    assert "k_refine_search_multi" in src and "k_refine_commit_multi" in src and "multi_engine_of" in src
