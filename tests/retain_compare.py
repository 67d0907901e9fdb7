"""
What a device tree must be after a retain, given the reference's result (tests/retain_reference.py retain()): BIT FOR BIT the
stats, the id map, the size, states, gains, parents, edge lengths, every live edge row, the ignore flags, the goal bookkeeping,
the host mirror of the parents (climb) and the new root's one-row zero-effort edge.  Shared by tests/test_retain_gpu.py and
tests/test_retain_edges_gpu.py (test infrastructure).
"""
import numpy as np


def check_retained(eng, ref, stats, old_to_new):
    """`stats`, `old_to_new`: what Engine.tree_retain (or this engine's entry of tree_retain_multi) returned."""
    assert stats == ref["stats"]
    np.testing.assert_array_equal(old_to_new, ref["old_to_new"])
    M = ref["stats"]["kept"]
    assert eng.size == M
    np.testing.assert_array_equal(eng.states(), ref["state"])
    np.testing.assert_array_equal(eng.gains(), ref["K"])
    np.testing.assert_array_equal(eng.parents(), ref["pID"])
    xe, ue, ln = eng.edges()
    np.testing.assert_array_equal(ln, ref["elen"])
    live = np.arange(xe.shape[1])[None, :] < ln[:, None]
    np.testing.assert_array_equal(xe[live], ref["xedge"][live])
    np.testing.assert_array_equal(ue[live], ref["uedge"][live])
    np.testing.assert_array_equal(eng.ignored(), ref["ignored"])
    assert eng.plan_best() == (ref["stats"]["best_end"], ref["stats"]["best_steps"], ref["stats"]["goal_hits"])
    best = ref["stats"]["best_end"]
    assert eng.climb(max(best, 0))[0] == 0                                       # the host mirror of the parents follows
    x, u = eng.edge(0)
    assert len(x) == 1 and np.array_equal(x[0], ref["state"][0]) and not u.any()
