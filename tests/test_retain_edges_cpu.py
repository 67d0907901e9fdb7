"""
The directed retain cases (tests/retain_cases.py) through the reference of the rule alone (tests/retain_reference.py, plain
NumPy + the C oracle's feasibility test): every case HAS the property it is named for, so that a later edit of a builder cannot
silently empty the device test that runs it (tests/test_retain_edges_gpu.py).  These are conditions on the inputs.
"""
import numpy as np
import pytest

import retain_cases as RC

BLOCK = 256                                                    # csrc/retain.hpp RETAIN_BLOCK


def depths(pID):
    d = np.zeros(len(pID), dtype=np.int64)
    for k in range(1, len(pID)):
        d[k] = d[pID[k]] + 1
    return d


def test_values_differ_from_node_to_node():
    """A state, gain or edge row moved to the wrong slot cannot compare equal."""
    for name in ("block_edges-heap-N513-r0", "scan_carry", "move_widths-moves", "revalidate_small", "goal_ties-tie"):
        c = RC.case(name)
        N = len(c.pID)
        assert len(np.unique(c.state, axis=0)) == N and len(np.unique(c.K.reshape(N, -1), axis=0)) == N
        assert len(np.unique(c.xedge, axis=0)) == len(c.xedge) == int(c.elen.sum())
        assert len(np.unique(c.uedge, axis=0)) == len(c.uedge)
        xe, ue = RC.dense(c)
        assert np.array_equal(xe[0, :c.elen[0]], c.xedge[:c.elen[0]]) and np.array_equal(ue[-1, :c.elen[-1]], c.uedge[-c.elen[-1]:])


@pytest.mark.parametrize("name", RC.names("chain_tight"))
def test_chain_tight(name):
    c, r = RC.case(name), RC.reference(name)
    N = len(c.pID)
    depth = N - 1 - c.root
    assert c.props["depth"] == depth and int(depths(r["pID"]).max()) == depth and r["stats"]["kept"] == depth + 1
    assert set(c.elen.tolist()) == set(range(1, c.H + 1)) or N < 5
    if depth >= 1:
        # the box holds the last node only: the best plan is the whole chain
        assert (r["stats"]["goal_hits"], r["stats"]["best_end"]) == (1, depth)
        assert r["stats"]["best_steps"] == c.props["best_steps"] == 1 + int(c.elen[c.root + 1:].sum())
        if depth >= 4:
            assert (r["stats"]["best_steps"] - 1) % depth != 0                  # not a multiple of the depth
    else:
        assert r["stats"]["goal_hits"] == 0


def test_chain_tight_needs_every_round():
    """N = 2^k with root 0: depth N - 1 > 2^(k - 1), so k - 1 doubling rounds do not reach the root from the last node; N + 1
    nodes are the first size with one round more."""
    have = [len(RC.case(n).pID) for n in RC.names("chain_tight") if RC.case(n).root == 0]
    for N in (4, 256, 1024):
        assert N in have and N + 1 in have and N - 1 > N // 2
    assert set(RC.case(n).root for n in RC.names("chain_tight-N1024")) == {0, 1, 1022}


@pytest.mark.parametrize("name", RC.names("block_edges"))
def test_block_edges(name):
    c, r = RC.case(name), RC.reference(name)
    st = r["stats"]
    if "kept" in c.props:
        assert st["kept"] == c.props["kept"]
    assert st["kept"] + st["outside"] == st["old_size"] and st["infeasible"] == st["orphaned"] == 0
    if c.root > 0:
        assert st["outside"] >= c.root                                           # a fixed rule drops what the root excludes


def test_block_edges_cover_the_stated_edges():
    cases = [RC.case(n) for n in RC.names("block_edges")]
    assert set(len(c.pID) for c in cases) == {1, 2, 255, 256, 257, 511, 512, 513}
    roots = set((len(c.pID), c.root) for c in cases)
    for N in (257, 511, 512, 513):
        assert {(N, 0), (N, 255), (N, 256), (N, N - 1)} <= roots
    kept = [RC.reference(c.name)["stats"]["kept"] for c in cases]
    assert 256 in kept and (64 in kept or 128 in kept) and 1 in kept
    ones = [c for c in cases if RC.reference(c.name)["stats"]["kept"] == 1]
    assert any(len(c.pID) == 1 for c in ones) and any(len(c.pID) > 1 and c.root == len(c.pID) - 1 for c in ones)
    # kept nodes that end exactly at a block boundary, a root on the last slot of a block and on the first of the next, with
    # kept nodes on both sides of the boundary
    for c in cases:
        if c.root in (255, 256) and len(c.pID) >= 511 and "comb" in c.name:
            old = RC.reference(c.name)["old_ids"]
            assert old[0] == c.root and old[-1] >= len(c.pID) - 2 and len(old) > 100


def test_scan_carry():
    c, r = RC.case("scan_carry"), RC.reference("scan_carry")
    N = len(c.pID)
    assert N == 65537 + 300 and c.H == 2 and c.root == 1 and not c.revalidate
    nblocks = (N + BLOCK - 1) // BLOCK
    assert nblocks >= 257                                                        # a second tile of block sums
    keep = r["old_to_new"] >= 0
    tile = np.arange(N) // (BLOCK * BLOCK)
    assert keep[65536:].any() and (~keep[65536:]).any()
    assert keep[:65536].any() and (~keep[:65536]).any() and not keep[0]
    par = np.maximum(c.pID, 0)
    assert np.any(keep & keep[par] & (tile[par] < tile))                         # a kept parent in an earlier scan tile
    assert int(depths(r["pID"]).max()) <= 4                                      # shallow: this one is about the scan
    assert r["stats"]["goal_hits"] > 10 and r["stats"]["outside"] > 9000


@pytest.mark.parametrize("variant", ["tie", "fewer_high"])
def test_goal_ties(variant):
    c, r = RC.case("goal_ties-" + variant), RC.reference("goal_ties-" + variant)
    a, b = c.props["pair"]
    assert r["ignored"][a] and r["ignored"][b] and a // BLOCK != b // BLOCK and (a - 1) // BLOCK != (b - 1) // BLOCK
    assert (int(r["steps"][a]), int(r["steps"][b])) == c.props["pair_steps"]
    assert r["stats"]["best_end"] == c.props["best_end"] == (a if variant == "tie" else b)
    assert r["stats"]["best_steps"] == min(c.props["pair_steps"])
    lo, hi = RC.goal_box(c)
    on_lo, on_hi = c.props["on_box"]
    in_lo, in_hi = c.props["inside"]
    assert np.sum(r["state"][on_lo] == lo) == 1 and np.sum(r["state"][on_hi] == hi) == 1
    assert np.sum(r["state"][in_lo] == np.nextafter(lo, np.inf)) == 1 and np.sum(r["state"][in_hi] == np.nextafter(hi, -np.inf)) == 1
    hits = set(k for k in range(1, r["stats"]["kept"]) if np.all((lo < r["state"][k]) & (r["state"][k] < hi)))
    assert hits == {a, b, in_lo, in_hi} and r["stats"]["goal_hits"] == 4
    assert not r["ignored"][on_lo] and not r["ignored"][on_hi] and r["ignored"][in_lo] and r["ignored"][in_hi]
    assert min(int(r["steps"][k]) for k in (in_lo, in_hi)) > max(c.props["pair_steps"])


def test_goal_nested():
    c, r = RC.case("goal_nested"), RC.reference("goal_nested")
    st = r["stats"]
    assert st["kept"] == c.props["kept"] == 256 and st["kept"] % 64 == 0 and st["goal_hits"] == 5
    lo, hi = RC.goal_box(c)
    hits = [k for k in range(1, st["kept"]) if np.all((lo < r["state"][k]) & (r["state"][k] < hi))]
    union = set()
    for k in hits:
        while k != -1:
            union.add(k)
            k = int(r["pID"][k])
    assert int(r["ignored"].sum()) == len(union) == c.props["union"] and set(np.flatnonzero(r["ignored"]).tolist()) == union
    assert len(set(k >> 6 for k in union)) >= 4                                  # four or more ignore words
    d = depths(r["pID"])
    assert sorted(int(d[k]) for k in hits) == [10, 70, 70, 135, 199]             # spine 10 / 70 / 199, branches 65 + 5 / 130 + 5
    assert int(d.max()) >= 200 and len(union) < st["kept"]                       # and kept nodes that nothing ignores


@pytest.mark.parametrize("variant", ["moves", "identity"])
def test_move_widths(variant):
    c, r = RC.case("move_widths-" + variant), RC.reference("move_widths-" + variant)
    n = RC.DIMS[c.system][0]
    st = r["stats"]
    assert c.system == "boat_advanced" and c.H >= 11 and st["kept"] == c.props["kept"]
    if variant == "moves":
        ln = c.elen[r["old_ids"]][1:]                                            # (the root's edge is replaced)
        assert int(ln.max()) * n > 64 and int(ln.max()) == c.H and int(ln.min()) == 1 and 1 < sorted(ln)[len(ln) // 2] < c.H
        assert np.all(r["old_to_new"][r["old_ids"]] < r["old_ids"])              # every kept node moves
        assert np.any(np.diff(r["old_ids"]) > 1)                                 # a dropped node between kept ones
    else:
        assert c.root == 0 and st["kept"] == st["old_size"] and c.elen[0] > 1 and r["elen"][0] == 1
        np.testing.assert_array_equal(r["elen"][1:], c.elen[1:])


def test_revalidate_small():
    c, r = RC.case("revalidate_small"), RC.reference("revalidate_small")
    st = r["stats"]
    N = len(c.pID)
    assert N <= 600 and c.revalidate and c.obstacles is not None
    assert st["outside"] > 0 and st["infeasible"] > 0 and st["orphaned"] > 0 and st["root_feasible"] == 0
    assert st["kept"] > 1 and r["old_ids"][0] == c.root                          # the root is kept whatever its own edge says
    feasible = RC.feasible_of(c)
    xe, ue = RC.dense(c)
    rows = [[bool(feasible(xe[i, k], ue[i, k])) for k in range(c.elen[i])] for i in range(N)]
    fail = c.props["fail"]
    for i in range(N):
        want = [True] * int(c.elen[i])
        if fail[i] in ("last", "only"):
            want[-1] = False
        elif fail[i] == "first":
            want[0] = False
        assert rows[i] == want, i
    assert any(f == "last" for f in fail[5:]) and any(f == "first" for f in fail[5:]) and fail[c.root] == "last"
    # one failing edge above a subtree that is otherwise clean: it alone orphans those nodes
    below = c.props["below_clean"]
    assert len(below) > 0 and all(fail[i] is None for i in below) and fail[c.props["clean"]] is not None
    assert r["old_to_new"][c.props["clean"]] == -1 and all(r["old_to_new"][i] == -1 for i in below)
    # a node whose parent lies below the root fails under the new world: outside, not infeasible
    assert c.pID[4] < c.root and not all(rows[4])
    n_fail_inside = sum(1 for i in range(N) if i > c.root and fail[i] is not None and i != 4)
    assert st["infeasible"] == n_fail_inside


def test_batched_members():
    """What tests/test_retain_edges_gpu.py puts into one call: sizes from 1 to 65837 with both parities of the round count,
    and a member with no workgroups between two with some in the check, move and goal grids."""
    sizes = [len(RC.case(n).pID) for n in RC.MULTI_MIXED]
    assert sizes == [1, 2, 257, 1024, 65537 + 300]
    rounds = lambda N: int(np.ceil(np.log2(N)))
    assert rounds(max(sizes)) % 2 == 1 and rounds(max(sizes[:-1])) == 10         # fin = rounds & 1 flips without the largest
    assert len(set((RC.case(n).system, RC.case(n).H) for n in RC.MULTI_MIXED)) == 1
    assert any(RC.case(n).goal is None for n in RC.MULTI_MIXED)
    for grid in ("check", "move", "goal"):
        for key in (grid, "all"):
            members = RC.MULTI_ZERO[key]
            assert 3 <= len(members) <= 5 and len(set((RC.case(n).system, RC.case(n).H) for n in members)) == 1
            counts = [RC.grid_counts(n)[grid] for n in members]
            assert any(counts[k] == 0 and any(counts[:k]) and any(counts[k + 1:]) for k in range(1, len(counts) - 1)), (grid, counts)
    assert RC.grid_counts("multi-leaf")["goal"] == 0 and RC.reference("multi-leaf")["stats"]["kept"] == 1
    assert RC.reference("multi-reval-a")["stats"]["goal_hits"] > 0 and RC.reference("multi-noreval-moves")["stats"]["goal_hits"] > 0
    a, b = (RC.case(n) for n in RC.MULTI_SHARED)
    assert np.array_equal(a.state, b.state) and np.array_equal(a.pID, b.pID) and a.root != b.root
    ra, rb = (RC.reference(n) for n in RC.MULTI_SHARED)
    assert ra["stats"] != rb["stats"] and not np.array_equal(ra["old_to_new"], rb["old_to_new"])
