"""
Reference of the tree retention (Engine.tree_retain / Planner.replan, csrc/retain.hpp) in plain NumPy: one sequential pass.

The rule, exactly as the engine implements it.  A tree of N nodes (pID[i] < i) with edges xedge / uedge / elen is re-rooted
at node `new_root`, optionally re-validated against the CURRENT world, and compacted:

  1. ok[i]: with `revalidate`, every recorded row k < elen[i] of node i's edge passes feasible(xedge[i][k], uedge[i][k]);
     without, ok[i] = True.
  2. keep[new_root] = True; keep[i] = False for i < new_root; keep[i] = ok[i] and keep[pID[i]] for i > new_root.  The new
     root is kept whatever its own edge says (that edge is not part of the new tree); `root_feasible` reports the test of
     its last edge row (1 without revalidation: nothing is tested).
  3. Kept nodes are renumbered in ascending old-id order.  Parents are remapped; the root gets pID -1, elen 1 and an edge of
     one row: its state with zero effort (tree.py:69-70).  State, K and edge rows of every other kept node move unchanged;
     the root keeps the gain it had as a node.
  4. Goal bookkeeping against the CURRENT goal box: a hit is a kept non-root node whose state lies strictly inside it
     (planner.py:442-447); steps(i) = sum of elen from the new root (its 1 included) down to i; best = the hit with the
     fewest steps, lowest new id on ties (planner.py:276, strict <); ignore set = union of the root paths of all hits
     (planner.py:270).
  5. Reported: old_size, kept, outside (not in the subtree of new_root), infeasible (in the subtree, own edge fails),
     orphaned (in the subtree, own edge passes, an ancestor was dropped), root_feasible, goal_hits, best_end, best_steps
     (-1 / -1 without a hit) and the old-id -> new-id map (-1 = dropped).
"""
import numpy as np

STAT_KEYS = ("old_size", "kept", "outside", "infeasible", "orphaned", "root_feasible", "goal_hits", "best_end", "best_steps")


def retain(state, K, pID, elen, xedge, uedge, new_root, feasible=None, goal_lo=None, goal_hi=None):
    """state (N, n), K (N, m, n), pID (N,), elen (N,), xedge (N, H, n), uedge (N, H, m) -- rows beyond elen[i] are not
    read.  feasible: callable (x, u) -> bool, or None = no revalidation.  goal_lo / goal_hi: the goal box, or None = no goal.
    Returns a dict: the arrays of the kept tree (same layout, rows beyond an edge's length zero), `ignored` (bool),
    `old_to_new` (int32), `steps` (per kept node) and `stats`."""
    state, K = np.asarray(state, dtype=np.float64), np.asarray(K, dtype=np.float64)
    pID, elen = np.asarray(pID, dtype=np.int64), np.asarray(elen, dtype=np.int64)
    xedge, uedge = np.asarray(xedge, dtype=np.float64), np.asarray(uedge, dtype=np.float64)
    N = len(state)
    r = int(new_root)
    if not 0 <= r < N:
        raise ValueError("The given ID, {}, doesn't exist.".format(new_root))

    def edge_ok(i):
        return all(feasible(xedge[i, k], uedge[i, k]) for k in range(int(elen[i])))

    insub = np.zeros(N, dtype=bool)
    keep = np.zeros(N, dtype=bool)
    insub[r] = keep[r] = True
    outside = infeasible = orphaned = 0
    for i in range(N):
        if i == r:
            continue
        insub[i] = i > r and insub[pID[i]]
        if not insub[i]:
            outside += 1
            continue
        ok = True if feasible is None else edge_ok(i)
        keep[i] = ok and keep[pID[i]]
        if not ok:
            infeasible += 1
        elif not keep[i]:
            orphaned += 1
    root_feasible = 1
    if feasible is not None:
        root_feasible = int(bool(feasible(xedge[r, elen[r] - 1], uedge[r, elen[r] - 1])))

    old = np.flatnonzero(keep)
    old_to_new = np.full(N, -1, dtype=np.int32)
    old_to_new[old] = np.arange(len(old), dtype=np.int32)
    M = len(old)
    out = dict(state=state[old].copy(), K=K[old].copy(), old_ids=old)
    npid = old_to_new[pID[old]].astype(np.int32)
    npid[0] = -1
    nlen = elen[old].astype(np.int32)
    nlen[0] = 1
    nx, nu = np.zeros((M,) + xedge.shape[1:]), np.zeros((M,) + uedge.shape[1:])
    for k, i in enumerate(old):
        nx[k, :nlen[k]] = xedge[i, :nlen[k]]
        nu[k, :nlen[k]] = uedge[i, :nlen[k]]
    nx[0, 0], nu[0, 0] = state[r], 0.0
    out.update(pID=npid, elen=nlen, xedge=nx, uedge=nu)

    steps = np.zeros(M, dtype=np.int64)
    steps[0] = 1
    ignored = np.zeros(M, dtype=bool)
    hits, best_end, best_steps = 0, -1, -1
    for k in range(1, M):
        steps[k] = steps[npid[k]] + nlen[k]
        if goal_lo is None or not np.all((goal_lo < out["state"][k]) & (out["state"][k] < goal_hi)):
            continue
        hits += 1
        if best_end < 0 or steps[k] < best_steps:
            best_end, best_steps = k, int(steps[k])
        v = k
        while v != -1:
            ignored[v] = True
            v = npid[v]
    out.update(ignored=ignored, old_to_new=old_to_new, steps=steps)
    out["stats"] = dict(old_size=N, kept=M, outside=outside, infeasible=infeasible, orphaned=orphaned, root_feasible=root_feasible,
                        goal_hits=hits, best_end=best_end, best_steps=best_steps)
    return out


def packed_edges(res):
    """(xedge, uedge) of a retain() result back to back in node order: the form Engine.tree_load takes."""
    live = np.arange(res["xedge"].shape[1])[None, :] < res["elen"][:, None]
    return res["xedge"][live], res["uedge"][live]


def oracle_arrays(o):
    """(state, K, pID, elen, xedge, uedge) of a C oracle's tree in retain()'s layout."""
    N, H = o.size, o.H
    xe, ue = np.zeros((N, H, o.n)), np.zeros((N, H, o.m))
    ln = o.edge_lengths()
    for i in range(N):
        x, u = o.edge(i)
        assert len(x) == ln[i]
        xe[i, :len(x)], ue[i, :len(u)] = x, u
    return o.states(), o.gains(), o.parents(), ln, xe, ue


def engine_arrays(eng):
    """The same of a device tree (Engine)."""
    xe, ue, ln = eng.edges()
    return eng.states(), eng.gains(), eng.parents(), ln, xe, ue


def goal_box(system, goal=None):
    g = np.asarray(system.goal if goal is None else goal, dtype=np.float64)
    b = np.abs(np.asarray(system.goal_buffer, dtype=np.float64))
    return g - b, g + b
