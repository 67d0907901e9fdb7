"""
GPU: the entry of k_steer -- the hot argument header, the round block and the three entry modes (speculative launch with the
reduce prologue, fused repair round, plain list) -- against the sequential C oracle, BIT FOR BIT: parents, edge lengths, states,
gains, edges, ignore set, counters.  Only where a launch's arguments come from changed, so equality is the bar; the shapes are the
smallest at which an entry mode or the layout of the round block can go wrong:

  * boat_advanced (the chain rollout, three wavefronts) to 400 nodes at wave caps 1, 2, 64, 65 and 256: the lane-group edges of
    the round prologue's four-by-64 prefetch, a fused round with one workgroup, a round block laid out for maxW that is no
    multiple of 8;
  * car (the plain two-wavefront form) and pendulum (one wavefront) to 200 nodes at wave caps 8 and 65;
  * boat_novice_lqr to 60 nodes at wave cap 8: four cooperating wavefronts, one ticket per workgroup;
  * lqrrt_steer_batch with 1 and 65 problems: plain list mode, no fuse, no round;
  * a sample-sharded world of one (the loopback communicator, no process group) at wave cap 65: round 0 of a gathered wave.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _make(name, nodes, wave, seed=1):
    import lqrrt_amd
    from lqrrt_amd.engine import Engine
    s = lqrrt_amd.systems.SYSTEMS[name](0)
    eng = Engine(s, capacity=nodes + wave + 8, max_wave=wave)
    kw = s.plan_kwargs
    eng.set_resolution(kw["dt"], kw["FPR"], int(kw["horizon"] / kw["dt"]), np.abs(s.error_tol), s.goal, np.abs(s.goal_buffer))
    space = np.array(s.sample_space, dtype=np.float64)
    eng.set_sampler(np.mean(space, axis=1), np.diff(space).flatten(), np.array(s.goal_bias, dtype=np.float64), 10)
    st = np.random.RandomState(seed).get_state()
    eng.set_mt19937(st[1], st[2])
    eng.tree_reset(s.x0)
    return s, eng


_ORACLES = {}


def _oracle(s, name, nodes):
    """One sequential tree per (system, size), shared by the wave caps that are compared against it; never changed afterwards."""
    import coracle
    if (name, nodes) not in _ORACLES:
        o = coracle.make(s, nodes + 256 + 8, seed=1)
        assert o.extend(max_nodes=nodes) == 2
        _ORACLES[(name, nodes)] = o
    return _ORACLES[(name, nodes)]


def _compare(eng, stats, o):
    assert eng.size == o.size
    assert stats.attempts == o.iterations
    assert stats.candidates == o.candidates
    np.testing.assert_array_equal(eng.parents(), o.parents())
    np.testing.assert_array_equal(eng.edge_lengths(), o.edge_lengths())
    np.testing.assert_array_equal(eng.ignored(), o.ignored())
    np.testing.assert_array_equal(eng.states(), o.states())
    np.testing.assert_array_equal(eng.gains(), o.gains())
    for ID in range(eng.size):
        ex, eu = eng.edge(ID)
        ox, ou = o.edge(ID)
        np.testing.assert_array_equal(ex, ox)
        np.testing.assert_array_equal(eu, ou)
    end, steps, hits = eng.plan_best()
    assert hits == o.hits
    assert (end, steps) == o.best()


CASES = ([("boat_advanced", 400, w) for w in (1, 2, 64, 65, 256)] +
         [(name, 200, w) for name in ("car", "pendulum") for w in (8, 65)] +
         [("boat_novice_lqr", 60, 8)])


@pytest.mark.parametrize("name,nodes,wave", CASES)
def test_tree_bit_exact_at_the_entry_edges(name, nodes, wave):
    s, eng, = _make(name, nodes, wave)
    stats = eng.extend(wave, node_limit=nodes)
    _compare(eng, stats, _oracle(s, name, nodes))
    if wave > 1:
        assert stats.waves < stats.attempts                      # (waves of more than one sample were run: rounds, not a sequential loop)
    eng.close()


@pytest.mark.parametrize("W", [1, 65])
def test_steer_batch_plain_list_mode(W):
    """lqrrt_steer_batch: parents from a list, no reduce prologue, no round -- every problem against the oracle's own rollout from
    the same node of the same tree."""
    nodes = 100
    s, eng = _make("boat_advanced", nodes, 65)
    stats = eng.extend(65, node_limit=nodes)
    o = _oracle(s, "boat_advanced", nodes)
    _compare(eng, stats, o)
    rng = np.random.RandomState(7)
    space = np.array(s.sample_space, dtype=np.float64)
    parents = rng.randint(0, eng.size, size=W)
    xtar = space[:, 0] + rng.rand(W, eng.n) * (space[:, 1] - space[:, 0])
    ln, xs, us, xe, Ke = eng.steer_batch(parents, xtar)
    for i in range(W):
        oln, oxs, ous, oK = o.steer_from(int(parents[i]), xtar[i])
        assert int(ln[i]) == oln, i
        np.testing.assert_array_equal(xs[i, :oln], oxs)
        np.testing.assert_array_equal(us[i, :oln], ous)
        if oln > 0:
            np.testing.assert_array_equal(xe[i], oxs[-1])
            np.testing.assert_array_equal(Ke[i], oK)
    eng.close()


def test_gathered_wave_round_zero_in_a_world_of_one():
    """The sample-sharded loop with the loopback communicator as rank 0 of 1: every wave goes through the all-gather blocks, and
    round 0 of the fused rounds takes the samples out of them (RoundArgs::gblk)."""
    from lqrrt_amd.parallel import NativeComm
    nodes, wave = 400, 65
    s, eng = _make("boat_advanced", nodes, wave)
    comm = NativeComm(0, 1)
    stats = eng.extend_sharded(comm, "sample", wave, node_limit=nodes)
    _compare(eng, stats, _oracle(s, "boat_advanced", nodes))
    eng.close()
