"""
Fleet goal connection (lqrrt_amd.connect_goals, k_connect_search_multi) on the CPU: the host side of the public function, and what
the compiler says about the kernel whose grid spans several engines.  The device side is compared bit for bit in
tests/test_connect_multi_gpu.py and tests/test_fleet_connect_gpu.py.
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


def test_connect_goals_of_nobody():
    assert lqrrt_amd.connect_goals([]) == []
    import lqrrt
    assert lqrrt.connect_goals is lqrrt_amd.connect_goals
    assert "connect_goals" in lqrrt_amd.__all__ and "connect_goals" in lqrrt.__all__


def test_connect_goals_without_plans_changes_nothing():
    a, b = _native_planner(), _native_planner()
    assert lqrrt_amd.connect_goals([a, b]) == [False, False]        # no tree on the device: no native call, no engine
    assert lqrrt_amd.connect_goals([a], goal_tries=2, nodes=[[0]], finish_on_goal=True) == [False]
    assert lqrrt_amd.connect_goals([a, b], nodes=[None, [0, 1]]) == [False, False]
    for p in (a, b):
        assert p.tree is None and not hasattr(p, "node_seq") and not p.plan_reached_goal
        assert getattr(p, "_engine", None) is None


def test_connect_goals_refuses_before_touching_anybody():
    a, b = _native_planner(), _native_planner()
    with pytest.raises(ValueError, match="twice"):
        lqrrt_amd.connect_goals([a, b, a])
    cb = _callback_planner()
    assert cb.callback_mode
    with pytest.raises(ValueError, match="Python"):
        lqrrt_amd.connect_goals([a, cb])
    with pytest.raises(ValueError, match="Planner"):
        lqrrt_amd.connect_goals([a, object()])
    with pytest.raises(ValueError, match="goal_tries"):
        lqrrt_amd.connect_goals([a, b], goal_tries=0)
    with pytest.raises(ValueError, match="per planner"):
        lqrrt_amd.connect_goals([a, b], nodes=[None])
    with pytest.raises(ValueError, match="per planner"):
        lqrrt_amd.connect_goals([], nodes=[None])
    for p in (a, b):
        assert p.tree is None and not hasattr(p, "node_seq")


def test_connect_goal_and_connect_goals_share_their_steps():
    """connect_goal calls the instance's own connect_search / connect_commit; connect_goals the batched ones; both go through the
    same three steps, which live on the planner."""
    for name in ("_connect_begin", "_connect_incumbent", "_connect_accept"):
        assert callable(getattr(lqrrt_amd.Planner, name))
    src = open(os.path.join(ROOT, "lqrrt_amd", "planner.py")).read()
    solo = src[src.index("    def connect_goal(self"):src.index("    def _connect_begin(self")]
    fleet = src[src.index("def connect_goals("):]
    assert "eng.connect_search(" in solo and "eng.connect_commit(" in solo
    assert "Engine.connect_search_multi(" in fleet and "Engine.connect_commit_multi(" in fleet
    assert ".connect_search(" not in fleet and ".connect_commit(" not in fleet
    for name in ("_connect_begin(", "_connect_incumbent(", "_connect_accept("):
        assert name in solo and name in fleet, name


# The one model the issue allowed to be pinned as an exception (the wrapper as first written: 256 VGPRs + 2 AGPRs, one wavefront per
# SIMD against the solo kernel's 247 VGPRs and two) needs none: the prototype and the descriptor are read through the constant
# address space (connect.hpp launch_constant) and every model keeps the solo kernel's occupancy.
OCCUPANCY_EXCEPTIONS = {}


def test_multi_search_keeps_its_solo_twins_frame_and_occupancy():
    """For every model S, UserSystem included: k_connect_search_multi<S> exists, its private segment is no larger than that of
    k_connect_search<S> and its occupancy no lower -- the indirection through EngineProto and ConnectDesc costs neither."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    assert shutil.which(kr.HIPCC) or os.path.exists(kr.HIPCC), "hipcc is what builds the package: it cannot be missing here"
    user = os.path.join(ROOT, "examples", "user_system", "unicycle.hpp")
    rows = kr.parse(kr.remarks(["-DLQRRT_USER_SYSTEM=\"%s\"" % user]))

    def by_model(kernel):
        out = {}
        for r in rows:
            m = re.match(r"void lq::%s<lq::(.+?) ?>\(" % kernel, r["name"])
            if m:
                out[m.group(1)] = r
        return out
    solo, multi = by_model("k_connect_search"), by_model("k_connect_search_multi")
    assert len(solo) >= 10 and "UserSystem" in solo, sorted(solo)
    assert sorted(multi) == sorted(solo)
    for model in solo:
        print("%-18s solo %4d B occ %d vgpr %3d agpr %d   multi %4d B occ %d vgpr %3d agpr %d" % (
            model, solo[model]["scratch"], solo[model]["occupancy"], solo[model]["vgpr"], solo[model]["agpr"],
            multi[model]["scratch"], multi[model]["occupancy"], multi[model]["vgpr"], multi[model]["agpr"]))
    assert not set(OCCUPANCY_EXCEPTIONS) - set(solo)
    worse = {}
    for m in solo:
        floor = OCCUPANCY_EXCEPTIONS.get(m, solo[m]["occupancy"])
        if multi[m]["scratch"] > solo[m]["scratch"] or multi[m]["occupancy"] < floor:
            worse[m] = (solo[m]["scratch"], multi[m]["scratch"], solo[m]["occupancy"], multi[m]["occupancy"])
    assert not worse, worse


def test_fleet_connection_stays_plain_launches():
    """One stream, plain launches: no cooperative launch, no grid-wide barrier; the multi kernel wraps the shared body, it holds no
    copy of the chain."""
    csrc = os.path.join(ROOT, "lqrrt_amd", "csrc")
    for f in ("connect.hpp", "engine_connect.hpp", "engine_refine.hpp"):        # (engine_refine.hpp: the multi path the calls run on)
        text = open(os.path.join(csrc, f)).read()
        for word in ("hipLaunchCooperativeKernel", "hipModuleLaunchCooperativeKernel", "cooperative_groups", "grid.sync", "this_grid"):
            assert word not in text, (f, word)
    src = open(os.path.join(csrc, "connect.hpp")).read()
    assert "k_connect_search_multi" in src and "multi_engine_of" in src and "struct ConnectDesc" in src
    assert "S::step(" not in src and src.count("refine_edge<S>(") == 1 and src.count("connect_search_body<S>(") == 2
    # the depth pass: defined once in all of csrc, and every tree-wide search reaches it -- connect's and reach's solo search, via's,
    # and the two searches for several trees
    texts = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".hpp"))}
    assert sum(t.count("static int connect_depths(") for t in texts.values()) == 1
    host = texts["engine_connect.hpp"]
    assert host.count("connect_depths(") == 3                       # the depth pass: one definition, the solo and the multi search
    assert "static int connect_depths(" in host and host.count("TRY(connect_depths(") == 2
    for f in ("engine_reach.hpp", "engine_connect_via.hpp", "engine_connect_via_multi.hpp"):
        assert texts[f].count("TRY(connect_depths(") == 1, f
    # the batched commit has no kernel and no hooks of its own: it is the shared commit runner with the refinement's hooks
    refine = texts["engine_refine.hpp"]
    search = refine[refine.index("static int multi_search_run("):refine.index("static int multi_commit_run(")]
    commit = refine[refine.index("static int multi_commit_run("):refine.index("static int refine_multi_check(")]
    assert "refine_multi_scratch(" in search and "refine_multi_scratch(" in commit
    assert "multi_search_run(" in host and "multi_commit_run(" in host and "RefineCommitMulti{" in host and "k_refine_commit_multi" not in host
    # the solo search and the multi search; the solo commit, like the batched one, is the refinement's (RefineCommitSolo's launch)
    assert host.count("hipLaunchKernelGGL(") == 2 and "RefineCommitSolo{" in host and "k_refine_commit<S>" in refine
    # the chunk loop of the fleet calls is written out in the two runners and in the clearance run, nowhere else
    clear = texts["engine_clear_multi.hpp"]
    clear_run = clear[clear.index("static int clear_multi_run("):clear.index("static int clear_multi_call(")]
    assert search.count("multi_chunks(") == 1 and commit.count("multi_chunks(") == 1 and clear_run.count("multi_chunks(") == 1
    assert sum(t.count("multi_chunks(") for t in texts.values()) == 4          # its definition and the three calls
    assert sorted(set(re.findall(r"static int (\w*_multi_run)\(", "".join(texts.values())))) == ["clear_multi_run"]
