"""
What the tests of the two clearance queries share (tests/test_clear_*.py).  For the device tests: an engine with a tree loaded from
the host, and one with a tree grown on the device; the engine is imported only when one is asked for.  For the tests that read the
sources: the host fragment of both calls, cut into its parts.
"""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WAVE = 256


def _load(system, tree, H, capacity=None, goal=None, goal_buffer=None, dt=0.1):
    """An engine with `tree` (state, K, pID, elen and packed edges) loaded and the goal box set."""
    from lqrrt_amd.engine import Engine
    eng = Engine(system, capacity=(len(tree.pID) + 64) if capacity is None else capacity, max_wave=64)
    goal = system.goal if goal is None else goal
    buf = system.goal_buffer if goal_buffer is None else goal_buffer
    eng.set_resolution(dt, 0.0, H, np.ones(system.nstates), goal, np.abs(np.asarray(buf, dtype=np.float64)))
    xe, ue = tree.packed()
    eng.tree_load(tree.state, tree.K, tree.pID, tree.elen, xe, ue)
    return eng


def _grown(seed=1, size=600):
    """A boat_advanced tree grown on the device by an engine set up like Planner does it: resolution, default sampler, MT19937."""
    import lqrrt_amd
    from lqrrt_amd.engine import Engine
    s = lqrrt_amd.systems.BoatAdvanced(0)
    kw = s.plan_kwargs
    eng = Engine(s, capacity=1200 + 2 * WAVE + 8, max_wave=WAVE)
    eng.set_resolution(kw["dt"], kw["FPR"], int(kw["horizon"] / kw["dt"]), np.abs(s.error_tol), s.goal, np.abs(s.goal_buffer))
    space = np.array(s.sample_space, dtype=np.float64)
    eng.set_sampler(np.mean(space, axis=1), np.diff(space).flatten(), np.array(s.goal_bias, dtype=np.float64), 10)
    st = np.random.RandomState(seed).get_state()
    eng.set_mt19937(st[1], st[2])
    eng.tree_reset(s.x0)
    eng.extend(WAVE, node_limit=size)
    return s, eng


FORBIDDEN = ("hipLaunchCooperativeKernel", "hipModuleLaunchCooperativeKernel", "cooperative_groups", "grid.sync", "this_grid", "asm(",
             "asm volatile", "__threadfence")
WORK = ("dalloc(", "dalloc_transient(", "hipMemcpyAsync(", "hipLaunchKernelGGL(")


def clear_host_text():
    """engine_clear.hpp (both calls) cut into what an export reaches, in the order it reaches it: the body of clear_check (every
    refusal), of clear_run (everything allocated and enqueued), of clear_call (check, then run) and of the two exports."""
    csrc = os.path.join(ROOT, "lqrrt_amd", "csrc")
    host = open(os.path.join(csrc, "engine_clear.hpp")).read()
    marks = ["static int clear_check(", "static int clear_run(", "static int clear_call(", 'extern "C" int lqrrt_tree_clear(',
             'extern "C" int lqrrt_tree_clear_wait(']
    at = [host.index(m) for m in marks]
    assert at == sorted(at) and all(host.count(m) == 1 for m in marks)
    parts = dict(zip(("check", "run", "call", "plain", "wait"), (host[p:q] for p, q in zip(at, at[1:] + [len(host)]))))
    # nothing is allocated or enqueued ahead of clear_run in the text but the launches the traits hand to it; an export does
    # nothing but clear_call, and clear_call checks before it runs
    assert not any(w in parts["check"] for w in WORK) and not any(w in parts["call"] + parts["plain"] + parts["wait"] for w in WORK)
    assert 0 <= parts["call"].index("TRY(clear_check<C>(") < parts["call"].index("clear_run<C>(") and parts["call"].count("fail(") == 0
    assert "clear_call<ClearPlain>(" in parts["plain"] and "clear_call<ClearWait>(" in parts["wait"]
    assert "fail(" not in parts["run"]                                             # the run refuses nothing
    return host, parts
