"""
Tree retention on the device (csrc/retain.hpp, csrc/engine_retain.hpp) on the directed cases of tests/retain_cases.py: small
hand-built trees put on the device with Engine.tree_load, retained by Engine.tree_retain / Engine.tree_retain_multi and compared
BIT FOR BIT (tests/retain_compare.py) with the reference of the rule (tests/retain_reference.py).  What every case is there for
is asserted from the reference alone in tests/test_retain_edges_cpu.py: a chain that needs every doubling round, the scan's
block edges and its second tile of block sums, a steps tie, both strict sides of the goal box, nested root paths over four
ignore words, edge copies of one row beside more than 64 doubles, zero-count members in the middle of every batched grid.
These are moves, integer scans and strict comparisons: there is no tolerance.
"""
import numpy as np
import pytest

import retain_cases as RC
import retain_reference as rr
from retain_compare import check_retained

pytestmark = pytest.mark.gpu

WAVE = 64
SOLO = [n for n in RC.REGISTRY if not n.startswith("multi-")]
TWICE = ("chain_tight", "block_edges", "goal_nested")          # retained a second time, from a root in the middle


def _engine(c, capacity=None):
    """(system, engine) of a case: capacity = N, so the tree fills the pools, unless the test goes on growing it."""
    from lqrrt_amd.engine import Engine
    s = RC.make_system(c)
    kw = s.plan_kwargs
    eng = Engine(s, capacity=max(capacity or len(c.pID), 2), max_wave=WAVE)
    eng.set_resolution(kw["dt"], kw["FPR"], c.H, np.abs(s.error_tol), c.goal, c.buf)
    return s, eng


def _load(eng, c):
    eng.tree_load(c.state, c.K, c.pID, edge_len=c.elen, xedge=c.xedge, uedge=c.uedge)
    assert eng.size == len(c.pID) and eng.plan_best() == (-1, -1, 0)


def _retain(eng, name):
    c, ref = RC.case(name), RC.reference(name)
    stats, old_to_new = eng.tree_retain(c.root, revalidate=c.revalidate)
    check_retained(eng, ref, stats, old_to_new)
    return ref


def _retain_again(eng, c, ref):
    """The retained tree once more, from the node in its middle: the reference starts from the FIRST reference's result, so the
    host mirrors the first retain left (parents, edge lengths, ignore words) have to be right.  Returns the new reference."""
    root = ref["stats"]["kept"] // 2
    lo, hi = RC.goal_box(c)
    again = rr.retain(ref["state"], ref["K"], ref["pID"], ref["elen"], ref["xedge"], ref["uedge"], root, RC.feasible_of(c), lo, hi)
    stats, old_to_new = eng.tree_retain(root, revalidate=c.revalidate)
    check_retained(eng, again, stats, old_to_new)
    return again


@pytest.mark.parametrize("name", SOLO)
def test_solo_retain_is_the_reference(name):
    c = RC.case(name)
    s, eng = _engine(c)
    _load(eng, c)
    fp = eng.footprint()
    ref = _retain(eng, name)
    if name.startswith(TWICE):
        ref = _retain_again(eng, c, ref)
        if ref["stats"]["kept"] > 3:
            _retain_again(eng, c, ref)
    assert eng.footprint() == fp                                                 # every buffer of a retain is transient
    if name == "move_widths-identity":
        # nothing moved: the loaded arrays as they were, but for the root's edge
        np.testing.assert_array_equal(eng.states(), c.state)
        np.testing.assert_array_equal(eng.edge_lengths()[1:], c.elen[1:])
    eng.close()


def test_identity_retain_after_a_load_with_a_long_root_edge():
    """Root 0, nothing dropped, and the loaded root carries an edge of several rows: only elen[0] and the seed's edge change,
    on the device and in the host mirror, and a retain of THAT tree moves every edge from the right place."""
    c = RC.case("move_widths-identity")
    s, eng = _engine(c)
    _load(eng, c)
    x, _ = eng.edge(0)
    assert len(x) == c.elen[0] > 1
    ref = _retain(eng, c.name)
    assert eng.edge_lengths()[0] == 1 and len(eng.edge(0)[0]) == 1
    lo, hi = RC.goal_box(c)
    again = rr.retain(ref["state"], ref["K"], ref["pID"], ref["elen"], ref["xedge"], ref["uedge"], 1, None, lo, hi)
    stats, old_to_new = eng.tree_retain(1, revalidate=False)
    check_retained(eng, again, stats, old_to_new)
    assert again["stats"]["kept"] == RC.reference("move_widths-moves")["stats"]["kept"]
    eng.close()


@pytest.mark.parametrize("mode", ["exact", "synchronous"])
@pytest.mark.parametrize("name", ["goal_nested", "block_edges-heap-N512-r1"])
def test_growth_from_the_retained_tree(name, mode):
    """A few dozen nodes more, with a fixed seed: the flushed ignore bitmap (256 kept nodes: four full words and a cleared
    fifth) and the cleared words of the dropped nodes are what the NN scan reads, so the tree grows exactly as the sequential C
    oracle's does from the reference's kept tree, and the kept part stays what it was."""
    import coracle
    c = RC.case(name)
    more = 40
    kept = RC.reference(name)["stats"]["kept"]
    assert kept == 256
    s, eng = _engine(c, capacity=len(c.pID) + more + 2 * WAVE + 8)
    _load(eng, c)
    ref = _retain(eng, name)
    hits = ref["stats"]["goal_hits"]
    kw = s.plan_kwargs
    space = np.array(s.sample_space, dtype=np.float64)
    eng.set_sampler(np.mean(space, axis=1), np.diff(space).flatten(), np.array(s.goal_bias, dtype=np.float64), 10)
    st = np.random.RandomState(9).get_state()
    eng.set_mt19937(st[1], st[2])
    o = coracle.COracle(s, kept + more + 2 * WAVE + 16)
    o.configure(kw["dt"], kw["FPR"], c.H, s.error_tol, c.goal, c.buf, s.sample_space, s.goal_bias, 10)
    o.seed(9)
    o.reset(ref["state"][0])
    o.load_tree(ref["state"], ref["K"], ref["pID"], ref["ignored"])
    if mode == "synchronous":
        eng.set_wave_mode("synchronous")
        eng.extend(WAVE, max_attempts=40 * more, node_limit=kept + more - 1)
        o.extend_sync(WAVE, max_iters=40 * more, max_nodes=kept + more - 1)
    else:
        eng.extend(WAVE, max_attempts=40 * more, node_limit=kept + more - 1)
        o.extend(max_iters=40 * more, max_nodes=kept + more - 1)
    print("%s %s: %d -> %d nodes, %d goal hits" % (name, mode, kept, eng.size, eng.plan_best()[2]))
    assert eng.size == o.size >= kept + more
    np.testing.assert_array_equal(eng.parents(), o.parents())
    np.testing.assert_array_equal(eng.states(), o.states())
    np.testing.assert_array_equal(eng.gains(), o.gains())
    np.testing.assert_array_equal(eng.ignored(), o.ignored())
    assert eng.plan_best()[2] == hits                                            # no new hit: no new root path to ignore
    np.testing.assert_array_equal(eng.ignored()[:kept], ref["ignored"])
    assert not eng.ignored()[kept:].any()
    np.testing.assert_array_equal(eng.states()[:kept], ref["state"])
    eng.close()


# ---------------------------------------------------------------------------------------------- Engine.tree_retain_multi

def _fleet(names):
    return [_engine(RC.case(n))[1] for n in names]


def _retain_multi(engines, names):
    """Every tree loaded afresh, ONE batched call, every member against its own reference (and so against the solo call, which
    test_solo_retain_is_the_reference holds to the same references)."""
    from lqrrt_amd.engine import Engine
    cases = [RC.case(n) for n in names]
    for eng, c in zip(engines, cases):
        _load(eng, c)
    done = Engine.tree_retain_multi(engines, [c.root for c in cases], [c.revalidate for c in cases])
    assert len(done) == len(engines)
    for eng, n, (stats, old_to_new) in zip(engines, names, done):
        check_retained(eng, RC.reference(n), stats, old_to_new)


def test_multi_mixed_sizes_and_both_round_parities():
    """Trees of 1, 2, 257, 1024 (a tight chain) and 65837 nodes in one call: 17 rounds for everybody, the final links in buffer
    1; then the same call without the largest: 10 rounds, the final links in buffer 0."""
    names = list(RC.MULTI_MIXED)
    engines = _fleet(names)
    footprints = [e.footprint() for e in engines]
    _retain_multi(engines, names)
    _retain_multi(engines[:-1], names[:-1])
    _retain_multi(engines[::-1], names[::-1])
    assert [e.footprint() for e in engines] == footprints
    for e in engines:
        e.close()


@pytest.mark.parametrize("key", sorted(RC.MULTI_ZERO))
def test_multi_zero_count_members_in_the_middle(key):
    """A member that does not revalidate between two that do (no check workgroups), one that keeps everything between two that
    move, one that keeps a single node between two with goal hits (no goal workgroups) -- and all of it in one call of five;
    each ordering forwards and reversed."""
    names = list(RC.MULTI_ZERO[key])
    engines = _fleet(names)
    _retain_multi(engines, names)
    _retain_multi(engines[::-1], names[::-1])
    for e in engines:
        e.close()


def test_multi_same_tree_two_roots():
    """Two members load the same tree and take different roots: different answers, each its own reference's."""
    names = list(RC.MULTI_SHARED)
    engines = _fleet(names)
    _retain_multi(engines, names)
    assert engines[0].size != engines[1].size
    assert not np.array_equal(engines[0].states(0, 2), engines[1].states(0, 2))
    _retain_multi(engines[::-1], names[::-1])
    for e in engines:
        e.close()
