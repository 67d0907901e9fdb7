"""
CPU: the sequential reference of the per-wave suite and the crafted waves, checked against the C oracle alone.

  * tests/wave_reference.py Replay -- the loop restated over the oracle's single-decision primitives -- equals orc_extend on the
    oracle's own traced samples BIT FOR BIT: parents, edge lengths, states, gains, ignore sets, hit counts and best plan.
  * Every crafted wave of tests/wave_cases.py satisfies the condition it carries, according to the census alone: a case that no
    longer builds the chain, tie, vanishing hit or hit position it is named after fails here.
  * The census's rule for the committed prefix C (max_commit, node limit, first goal hit) equals the iterations that
    orc_extend(max_iters, max_nodes, stop_on_goal=True) runs, wave after wave, on sampler-driven waves.
"""
import numpy as np
import pytest

import coracle
import wave_cases as wc
from wave_reference import Replay, census


def traced_samples(s, iters, seed=1):
    """(oracle after `iters` iterations, their samples)"""
    o = coracle.make(s, iters + 8, seed=seed)
    o.enable_trace(iters)
    o.extend(max_iters=iters)
    return o, o.trace_samples()


@pytest.mark.parametrize("name,iters", [("car", 600), ("double_integrator", 400), ("boat_advanced", 400), ("pendulum", 300),
                                        ("pendulum_lqr", 60)])
def test_replay_equals_orc_extend(name, iters):
    s = wc.system(name)
    o, xs = traced_samples(s, iters)
    assert o.iterations == iters
    rp = Replay(s, iters + 8)
    rp.run(xs)
    near, ln = o.trace()
    np.testing.assert_array_equal(rp.near, near)
    np.testing.assert_array_equal(rp.lens, ln)
    np.testing.assert_array_equal(rp.parents(), o.parents())
    np.testing.assert_array_equal(rp.edge_lengths(), o.edge_lengths())
    np.testing.assert_array_equal(rp.node_states(), o.states())
    np.testing.assert_array_equal(rp.gains(), o.gains())
    np.testing.assert_array_equal(rp.ignored(), o.ignored())
    assert rp.hits == o.hits and rp.best() == o.best()
    for ID in range(0, rp.size, 17):
        ox, ou = o.edge(ID)
        np.testing.assert_array_equal(rp.edges[ID][0], ox)
        np.testing.assert_array_equal(rp.edges[ID][1], ou)
    if name in ("car", "double_integrator"):
        assert o.hits >= 3                                    # the goal bookkeeping was exercised


@pytest.mark.parametrize("case", wc.small_cases() + wc.tri_cases(), ids=repr)
def test_crafted_wave_keeps_its_condition(case):
    c = case.census()
    assert c.W == case.W and c.N0 == 1 + sum(len(p) for p in case.pre)
    case.check(c)


@pytest.mark.parametrize("case,max_commit,node_limit", wc.limit_cases(), ids=repr)
def test_limit_cases_cut_where_they_say(case, max_commit, node_limit):
    full = case.census()
    tag = node_limit
    mc, nl = wc.limit_of(case, max_commit, node_limit)
    c = case.census(max_commit=mc, node_limit=nl)
    acc = np.cumsum(full.length > 0)
    if tag == -1:
        assert c.C == min(mc, full.C)
    elif tag == "hit":
        assert c.C == full.first_hit + 1 and c.goal_hits == 1 and c.tree_size == nl + 1      # hit and limit on one sample
    elif tag == "before":
        last = int(np.flatnonzero(full.length[:full.first_hit] > 0)[-1])
        assert c.C == last + 1 and c.goal_hits == 0 and c.tree_size == nl + 1
    elif tag == 0:
        assert c.C == 0 and c.accepted == 0
    else:
        assert c.accepted == min(tag, full.accepted) and (c.C == full.C or acc[c.C - 1] == tag)


WAVES = [1, 2, 3, 5, 63, 64, 65, 127, 129, 255, 256, 257, 289]


@pytest.mark.parametrize("name", ["car", "double_integrator"])
def test_census_prefix_rule_equals_orc_extend(name):
    """Sampler-driven waves near the goal: the oracle runs extend(min(W, max_commit), node_limit, stop_on_goal); the iterations it
    ran are the C the census names for the same wave of samples."""
    s = wc.system(name)
    total = 1600
    _, xs = traced_samples(s, total)                          # the sampler's stream does not depend on the tree
    o = coracle.make(s, total + 8, seed=1)
    rp = Replay(s, total + 8)
    k = goal_cuts = limit_cuts = 0
    for i, W in enumerate(WAVES * 2):
        if k + W > total:
            break
        mc = W if i % 2 == 0 else max(1, (2 * W) // 3)
        nl = -1 if i % 3 else rp.size + W // 4                # every third wave has room for W // 4 + 1 nodes
        c = census(rp, xs[k:k + W], max_commit=mc, node_limit=nl)
        before = o.iterations
        reason = o.extend(max_iters=min(W, mc), max_nodes=nl, stop_on_goal=True)
        assert o.iterations - before == c.C, (i, W, mc, nl, c)
        goal_cuts += reason == 4
        limit_cuts += reason == 2
        rp.run(xs[k:k + c.C])
        k += c.C
        assert rp.size == o.size == c.tree_size
        np.testing.assert_array_equal(rp.parents(), o.parents())
        np.testing.assert_array_equal(rp.ignored(), o.ignored())
    np.testing.assert_array_equal(rp.node_states(), o.states())
    assert limit_cuts >= 1
    if name == "double_integrator":
        assert goal_cuts >= 3


@pytest.mark.parametrize("name", wc.LOCKSTEP)
def test_lockstep_runs_contain_goal_cuts_and_limit_cuts(name):
    """The sampler-driven lockstep runs of tests/test_wave_gpu.py, by the oracle alone: at least 3 waves are cut by a goal hit and
    at least one is ended by the node limit."""
    cuts = lims = 0
    for part in (1, 2):
        s, o, _, waves = wc.lockstep_oracle(name, part)
        if part == 2:
            o.extend(max_iters=wc.LOCKSTEP_GROWN)
        for i, W in enumerate(waves):
            mc, nl = wc.lockstep_limits(i, W, o.size)
            reason = o.extend(max_iters=min(W, mc), max_nodes=nl, stop_on_goal=True)
            cuts += reason == 4
            lims += reason == 2
        assert o.size < 1500
    assert cuts >= 3 and lims >= 1, (cuts, lims)
