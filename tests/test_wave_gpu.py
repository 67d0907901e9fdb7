"""
GPU: exact-mode waves ONE AT A TIME against the sequential reference, BIT FOR BIT, at their size, cut, tie and repair-path edges.

The long runs of test_hip_vs_coracle.py compare a final tree; here lqrrt_wave_speculate / lqrrt_wave_commit are driven directly and
after EVERY wave the whole tree (parents, edge lengths, states, gains, ignore flags, best plan, every new edge row by row) is
compared with the reference, and the wave's own lqrrt_extend_stats with the census of tests/wave_reference.py: attempts == the
committed prefix C, accepted, goal_hits, tree_size, chain_slots == deepest chain of in-wave parents + 1, and fix_rounds >=
chain_slots - 1 (a link cannot be steered before its parent's final record exists: a bound that is derived, not measured).  A
failure names the case, the repair path, the engine's max_wave and the wave.

Repair paths, as the entry points reach them (csrc/engine_wave.hpp):
  fused   one whole-wave wave_speculate(W, 0, W), W <= 256: the rounds run inside k_steer;
  sliced  the same wave speculated as (0, a) then (a, W): k_par_from_records + k_wave_rows rebuild the bookkeeping and the in-wave
          matrix, then k_decide over the matrix, listed re-steers and k_append;
  empty   (0, 0) then (0, W): the empty slice must leave nothing behind, the whole slice runs fused;
  tri     W > 256 (and Riccati systems at any W through this entry point): k_decide over the k_nn_scan<TRI> partials.
The crafted waves are tests/wave_cases.py's (their conditions are checked on the CPU by tests/test_wave_cpu.py); the observed
fix_rounds / resteers per case and path are printed (pytest -s) and recorded in LABNOTES.md, not asserted.
"""
import numpy as np
import pytest

import wave_cases as wc
from wave_reference import census

pytestmark = pytest.mark.gpu


def make_engine(s, capacity, max_wave, root=None, horizon=None, sampler_seed=None):
    from lqrrt_amd.engine import Engine
    eng = Engine(s, capacity=capacity, max_wave=max_wave)
    kw = s.plan_kwargs
    if horizon is None:
        eng.set_resolution(kw["dt"], kw["FPR"], int(kw["horizon"] / kw["dt"]), np.abs(s.error_tol), s.goal, np.abs(s.goal_buffer))
    else:
        hspan = np.divide(horizon, kw["dt"]).astype(np.int64)
        eng.set_resolution(kw["dt"], kw["FPR"], int(hspan[1]), np.abs(s.error_tol), s.goal, np.abs(s.goal_buffer),
                           adaptive=True, hspan_min=int(hspan[0]), horizon_iters_state=1)
    if sampler_seed is not None:
        space = np.array(s.sample_space, dtype=np.float64)
        eng.set_sampler(np.mean(space, axis=1), np.diff(space).flatten(), np.array(s.goal_bias, dtype=np.float64), 10)
        st = np.random.RandomState(sampler_seed).get_state()
        eng.set_mt19937(st[1], st[2])
    eng.tree_reset(np.array(s.x0 if root is None else root, dtype=np.float64))
    return eng


class ReplayView(object):
    """tests/wave_reference.py Replay with the accessors of a COracle."""

    def __init__(self, rp):
        self.rp = rp

    size = property(lambda self: self.rp.size)
    hits = property(lambda self: self.rp.hits)
    parents = lambda self: self.rp.parents()
    edge_lengths = lambda self: self.rp.edge_lengths()
    ignored = lambda self: self.rp.ignored()
    states = lambda self: self.rp.node_states()
    gains = lambda self: self.rp.gains()
    best = lambda self: self.rp.best()
    edge = lambda self, ID: self.rp.edges[ID]


def assert_same_tree(eng, ref, first, ctx):
    """The engine's whole tree against the reference's; the edges of the nodes from `first` on row by row."""
    assert eng.size == ref.size, ctx
    np.testing.assert_array_equal(eng.parents(), ref.parents(), err_msg=ctx)
    np.testing.assert_array_equal(eng.edge_lengths(), ref.edge_lengths(), err_msg=ctx)
    np.testing.assert_array_equal(eng.states(), ref.states(), err_msg=ctx)
    np.testing.assert_array_equal(eng.gains(), ref.gains(), err_msg=ctx)
    np.testing.assert_array_equal(eng.ignored(), ref.ignored(), err_msg=ctx)
    end, steps, hits = eng.plan_best()
    assert hits == ref.hits and (end, steps) == tuple(ref.best()), ctx
    if eng.size > first:
        xe, ue, ln = eng.edges(first, eng.size - first)
        for k in range(eng.size - first):
            ox, ou = ref.edge(first + k)
            assert int(ln[k]) == len(ox), (ctx, first + k)
            np.testing.assert_array_equal(xe[k, :len(ox)], ox, err_msg="%s edge %d" % (ctx, first + k))
            np.testing.assert_array_equal(ue[k, :len(ou)], ou, err_msg="%s edge %d" % (ctx, first + k))


def slices_of(path, W):
    """The wave_speculate calls of a path for a wave of W samples; None where the path does not apply to this W."""
    if path == "fused" or path == "tri":
        return [(0, W)]
    if path == "empty":
        return [(0, 0), (0, W)]
    a = {"slice1": 1, "slice64": 64, "sliceW-1": W - 1}[path]
    return [(0, a), (a, W)] if 0 < a < W else None


def one_wave(eng, rp, xs, W, slices, mc, nl, ctx):
    """One engine wave over xs[:W] against census + replay; returns (C, stats)."""
    cs = census(rp, xs[:W], max_commit=mc, node_limit=nl)
    q0, c0, n0 = eng.queued_samples(), eng.counters(), eng.size
    for lo, hi in slices:
        eng.wave_speculate(W, lo, hi)
    st = eng.wave_commit(W, mc, nl, rp.pruning)
    got = dict(attempts=st.attempts, accepted=st.accepted, goal_hits=st.goal_hits, tree_size=st.tree_size, chain_slots=st.chain_slots)
    want = dict(attempts=cs.C, accepted=cs.accepted, goal_hits=cs.goal_hits, tree_size=cs.tree_size, chain_slots=cs.chain_slots)
    assert got == want, (ctx, cs)
    assert st.fix_rounds >= st.chain_slots - 1, (ctx, st.fix_rounds, st.chain_slots)
    assert eng.queued_samples() == q0 - cs.C, ctx
    if cs.C == 0:                                             # nothing committed: tree, cursor and counters stand
        c1 = eng.counters()
        assert (c1.attempts, c1.accepted, c1.goal_hits, c1.tree_size, c1.candidates) == \
               (c0.attempts, c0.accepted, c0.goal_hits, c0.tree_size, c0.candidates), ctx
        assert eng.size == n0
    rp.run(xs[:cs.C])
    assert_same_tree(eng, ReplayView(rp), n0, ctx)
    return cs.C, st


def run_case(case, path, max_wave, first=None):
    """The case's wave (cut by `first` = (max_commit, node_limit) if given), then waves without limits until every sample is
    consumed, all on `path`; the engine against the replay after every wave.  Returns the first wave's stats."""
    total = case.W
    rp = case.replay()
    eng = make_engine(case.system, rp.size + 2 * total + 16, max_wave, root=case.root)
    try:
        for p in case.pre:
            p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1, rp.n)
            n0 = eng.size
            eng.push_samples(p)
            eng.wave_speculate(len(p), 0, len(p))
            st = eng.wave_commit(len(p), len(p), -1, rp.pruning)
            assert st.attempts == len(p)
            assert_same_tree(eng, ReplayView(rp), n0, "%s pre-wave" % case.name)
        eng.push_samples(case.samples)
        assert eng.queued_samples() == total
        k, wave, first_stats = 0, 0, None
        while k < total:
            W = total - k
            mc, nl = (W, -1) if (first is None or wave > 0) else first
            slices = slices_of(path, W) or [(0, W)]
            ctx = "%s path=%s max_wave=%d wave %d (W=%d max_commit=%d node_limit=%d)" % (case.name, path, max_wave, wave, W, mc, nl)
            C, st = one_wave(eng, rp, case.samples[k:], W, slices, mc, nl, ctx)
            first_stats = first_stats or st
            if C == 0:
                assert wave == 0 and first is not None, ctx   # only a limit of the first wave may commit nothing
            k += C
            wave += 1
            assert wave <= total + 2, ctx
        assert rp.iterations - sum(len(p) for p in case.pre) == total and eng.queued_samples() == 0
        return first_stats
    finally:
        eng.close()


def configs(W):
    """(path, max_wave) pairs a crafted wave of W <= 256 samples runs on: every path its W allows; the engine's max_wave is W
    itself, 251 (no multiple of 8; W <= 251 only) or 1024 -- the round block's offsets follow from it."""
    odd = 251 if W <= 251 else 1024
    out = [("fused", W), ("fused", odd), ("fused", 1024), ("empty", odd)]
    for path, mw in (("slice1", 1024), ("slice64", odd), ("sliceW-1", W)):
        if slices_of(path, W) and (path, W) != ("sliceW-1", 2):      # (W = 2: slice1 is sliceW-1)
            out.append((path, mw))
    return list(dict.fromkeys(out))


@pytest.mark.parametrize("case", wc.small_cases(), ids=repr)
def test_crafted_wave_on_every_path(case):
    rounds = {}
    for path, mw in configs(case.W):
        st = run_case(case, path, mw)
        rounds.setdefault(path, set()).add((int(st.fix_rounds), int(st.resteers)))
    print("[rounds] %s W=%d %s" % (case.name, case.W, " ".join("%s=%s" % (p, sorted(v)) for p, v in sorted(rounds.items()))))


@pytest.mark.parametrize("case", wc.tri_cases(), ids=repr)
def test_crafted_wave_tri_scan(case):
    """W in {257, 288, 289, 511, 1000} on an engine whose max_wave is W: the records end where the wave ends, W % 4 != 0 included."""
    st = run_case(case, "tri", case.W)
    print("[rounds] %s W=%d tri=(%d, %d)" % (case.name, case.W, st.fix_rounds, st.resteers))
    if case.W <= 511:
        run_case(case, "tri", 1024)


@pytest.mark.parametrize("case,max_commit,node_limit", wc.limit_cases(), ids=repr)
def test_wave_cut_by_limits(case, max_commit, node_limit):
    first = wc.limit_of(case, max_commit, node_limit)
    for path, mw in (("fused", case.W), ("slice64", 1024)):
        run_case(case, path, mw, first=first)


def test_tri_wave_cut_by_limits():
    """The cuts again where the commit reads the legacy summary of a W > 256 wave: hit and node limit on one sample, the sample
    before it, max_commit inside the wave, and nothing committed."""
    h = wc.hit_case(289, 256)
    for mc, nl in ((None, "hit"), (None, "before"), (257, -1), (0, -1), (None, 0)):
        run_case(h, "tri", 289, first=wc.limit_of(h, mc, nl))


# ---------------------------------------------------------------------------------------------- sampler-driven lockstep
def lockstep(name, part, sliced):
    s, o, seed, waves = wc.lockstep_oracle(name, part)
    horizon = wc.lockstep_horizon(name)
    max_wave = max(waves)
    eng = make_engine(s, 2600, max_wave, horizon=horizon, sampler_seed=seed)
    try:
        if part == 2:                                         # a tree to search first, through the native loop
            o.extend(max_iters=wc.LOCKSTEP_GROWN)
            st = eng.extend(256, max_attempts=wc.LOCKSTEP_GROWN)
            assert st.attempts == o.iterations and st.candidates == o.candidates
            assert_same_tree(eng, o, 0, "%s part 2 grown" % name)
        for i, W in enumerate(waves):
            mc, nl = wc.lockstep_limits(i, W, o.size)
            n0, it0, hits0 = o.size, o.iterations, o.hits
            o.extend(max_iters=min(W, mc), max_nodes=nl, stop_on_goal=True)
            C = o.iterations - it0
            a = W // 2
            slices = [(0, a), (a, W)] if (sliced and 0 < a) else [(0, W)]
            for lo, hi in slices:
                eng.wave_speculate(W, lo, hi)
            st = eng.wave_commit(W, mc, nl, True)
            ctx = "%s part %d wave %d (W=%d max_commit=%d node_limit=%d sliced=%s)" % (name, part, i, W, mc, nl, sliced)
            assert (st.attempts, st.accepted, st.goal_hits, st.tree_size, st.candidates) == \
                   (C, o.size - n0, o.hits - hits0, o.size, o.candidates), ctx
            assert st.fix_rounds >= st.chain_slots - 1 >= 0, ctx
            assert_same_tree(eng, o, n0, ctx)
            if horizon is not None:
                assert eng.horizon_iters_state() == o.horizon_iters, ctx
    finally:
        eng.close()


@pytest.mark.parametrize("sliced", [False, True], ids=["whole", "sliced"])
@pytest.mark.parametrize("part", [1, 2])
@pytest.mark.parametrize("name", wc.LOCKSTEP)
def test_lockstep_with_the_oracle(name, part, sliced):
    """Sampler-driven waves of the fixed schedule, near the goal: the oracle runs extend(min(W, max_commit), node_limit,
    stop_on_goal) first -- its iterations are the expected C -- then the engine runs the wave; everything is compared, the
    sampler rows consumed (`candidates`) included.  tests/test_wave_cpu.py shows that the runs hold >= 3 goal-cut waves and a
    wave ended by the node limit."""
    lockstep(name, part, sliced)


def test_riccati_through_extend_with_explicit_samples():
    """pendulum_lqr through Engine.extend (the native loop keeps the in-wave matrix for Riccati systems) on pushed samples,
    against the replay."""
    import coracle
    from wave_reference import Replay
    s = wc.lockstep_system("pendulum_lqr")
    total = 300
    o = coracle.make(s, total + 8, seed=3)
    o.enable_trace(total)
    o.extend(max_iters=total)
    xs = o.trace_samples()
    rp = Replay(s, total + 8)
    eng = make_engine(s, total + 256 + 16, 256)
    try:
        eng.push_samples(xs)
        k = 0
        for attempts in (1, 70, total):                       # three calls: the loop picks its own waves inside each
            st = eng.extend(256, max_attempts=attempts - k)
            assert st.attempts == attempts - k
            n0 = rp.size
            rp.run(xs[k:attempts])
            k = attempts
            assert_same_tree(eng, ReplayView(rp), n0, "pendulum_lqr extend to %d" % attempts)
        assert rp.hits == o.hits and eng.queued_samples() == 0
    finally:
        eng.close()
