"""
Thin object wrapper over the C ABI (include/lqrrt_hip.h).  Device memory for the operator
inputs/outputs is owned by PyTorch-ROCm tensors whose data_ptr() is handed to the HIP
library; launches go onto torch's current HIP stream.
"""
import ctypes as C

import numpy as np

from . import _native as nat


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise nat.NativeError(nat.E_NODEVICE, "torch sees no HIP device: lqrrt_amd needs an MI355X (no CPU fallback)")
    return torch


class Engine(object):
    """One native engine handle = one problem on one GPU."""

    def __init__(self, system, capacity, max_wave=1024, device=0):
        nat.require_device()
        self.system = system
        self.n, self.m = system.nstates, system.ncontrols
        self.device = device
        self.capacity = int(capacity)
        self.max_wave = int(max_wave)
        desc, keep = system.desc()
        self._keep = keep
        h = C.c_void_p()
        nat.check(nat.lib().lqrrt_engine_create(C.byref(desc), device, self.capacity, self.max_wave, C.byref(h)))
        self.h = h
        self._geometry_revision = getattr(system, "revision", 0)
        if system.S is not None:
            S = nat.as_f64(system.S, (self.n, self.n))
            nat.check(nat.lib().lqrrt_engine_set_dense_S(self.h, nat.ptr(S)))
        self.horizon_iters = None
        self.generation = 0           # bumped whenever the tree is replaced (reset / load): Tree views check it
        self.epoch = 0                # bumped whenever nodes can change behind a view's back (truncate / rewind / re-layout)

    def _stream(self):
        """torch's current HIP stream on THIS engine's device."""
        return nat.current_stream(self.device)

    def set_wave_mode(self, mode):
        """'exact' (default: the reference's sequential result) or 'synchronous' (all samples of a wave see the
        wave-start snapshot; fixed wave size; parity target oracle/lqrrt_oracle.c orc_extend_sync)."""
        modes = {"exact": 0, "synchronous": 1}
        if mode not in modes:
            raise ValueError("wave mode must be 'exact' or 'synchronous'")
        nat.check(nat.lib().lqrrt_engine_set_wave_mode(self.h, modes[mode]))
        self.wave_mode = mode

    def set_cu_mask(self, xcds=None, mask=None, n_cus=256):
        """Runs this engine's native loops on a stream restricted to some of the GPU's compute units (include/lqrrt_hip.h
        lqrrt_engine_set_cu_mask).  `xcds`: iterable of XCD numbers 0..7 (all CUs of those XCDs), or `mask`: the raw words;
        neither = the whole chip again.  Speed only."""
        if mask is None and xcds is not None:
            want = set(int(x) & 7 for x in xcds)
            words = np.zeros((n_cus + 31) // 32, dtype=np.uint32)
            for b in range(n_cus):
                if (b & 7) in want:
                    words[b >> 5] |= np.uint32(1 << (b & 31))
            mask = words
        if mask is None:
            nat.check(nat.lib().lqrrt_engine_set_cu_mask(self.h, None, 0))
            return
        mask = np.ascontiguousarray(mask, dtype=np.uint32)
        nat.check(nat.lib().lqrrt_engine_set_cu_mask(self.h, nat.ptr(mask), int(mask.size)))

    def footprint(self):
        """dict(device_bytes, pinned_bytes): what this engine holds in HBM and in page-locked host memory (lqrrt_engine_footprint)."""
        d, h = C.c_int64(), C.c_int64()
        nat.check(nat.lib().lqrrt_engine_footprint(self.h, C.byref(d), C.byref(h)))
        return dict(device_bytes=d.value, pinned_bytes=h.value)

    def sync_geometry(self):
        """Re-uploads parameters, hull points, obstacles and occupancy grid if the system object changed since
        this engine last saw it (system.revision; e.g. set_occupancy_grid between two plans)."""
        rev = getattr(self.system, "revision", 0)
        if rev != self._geometry_revision:
            desc, keep = self.system.desc()
            nat.check(nat.lib().lqrrt_engine_set_geometry(self.h, C.byref(desc), self._stream()))
            self._keep = keep
            self._geometry_revision = rev
            return True
        return False

    def close(self):
        if getattr(self, "h", None):
            nat.lib().lqrrt_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- configuration -------------------------------------------------------------------------
    def set_resolution(self, dt, FPR, horizon_iters, error_tol, goal, goal_buffer, adaptive=False, hspan_min=1,
                       horizon_iters_state=1):
        r = nat.Resolution()
        r.dt, r.FPR, r.horizon_iters = float(dt), float(FPR), int(horizon_iters)
        r.adaptive, r.hspan_min, r.horizon_iters_state = (1 if adaptive else 0), int(hspan_min), int(horizon_iters_state)
        tol = np.broadcast_to(np.asarray(error_tol, dtype=np.float64), (self.n,))
        for i in range(nat.MAX_STATES):
            r.error_tol[i] = tol[i] if i < self.n else np.inf
            r.goal[i] = 0.0
            r.goal_lo[i], r.goal_hi[i] = -np.inf, np.inf
        r.has_goal = 0
        if goal is not None:
            g, lo, hi = self._goal_box(goal, goal_buffer)
            r.has_goal = 1
            for i in range(self.n):
                r.goal[i] = g[i]
                r.goal_lo[i] = lo[i]
                r.goal_hi[i] = hi[i]
        nat.check(nat.lib().lqrrt_engine_set_resolution(self.h, C.byref(r)))
        if self.horizon_iters is not None and int(horizon_iters) != self.horizon_iters:
            self.generation += 1      # the edge pools were re-laid out and the tree emptied: bound Tree views are dead
        self.horizon_iters = int(horizon_iters)
        self.epoch += 1

    def _goal_box(self, goal, goal_buffer):
        """(goal, lo, hi) of a goal state and its buffer, one Python float per state: the ONE statement of the goal box, for the
        engine's own goal (set_resolution) and for the targets of reach_search / reach_commit."""
        g = np.asarray(goal, dtype=np.float64)
        b = np.asarray(goal_buffer, dtype=np.float64)
        lo, hi = [], []
        for i in range(self.n):
            lo.append(g[i] - b[i])                # planner.py:482-484
            hi.append(g[i] + b[i])
        return [g[i] for i in range(self.n)], lo, hi

    def horizon_iters_state(self):
        return nat.check(nat.lib().lqrrt_engine_horizon_iters(self.h))

    def set_sampler(self, centers, spans, goal_bias, tries_limit):
        s = nat.SamplerDesc()
        for i in range(self.n):
            s.centers[i], s.spans[i], s.goal_bias[i] = centers[i], spans[i], goal_bias[i]
        s.tries_limit = int(tries_limit)
        nat.check(nat.lib().lqrrt_engine_set_sampler(self.h, C.byref(s)))

    def set_mt19937(self, key, pos):
        key = np.ascontiguousarray(key, dtype=np.uint32)
        nat.check(nat.lib().lqrrt_engine_set_mt19937(self.h, nat.ptr(key), int(pos)))

    def get_mt19937(self):
        key = np.zeros(624, dtype=np.uint32)
        pos = C.c_int()
        nat.check(nat.lib().lqrrt_engine_get_mt19937(self.h, nat.ptr(key), C.byref(pos)))
        return key, pos.value

    def seed_from_numpy_global(self):
        st = np.random.get_state()
        self.set_mt19937(st[1], st[2])

    def sync_numpy_global(self):
        """Leaves np.random exactly where the reference's sampler would have left it."""
        key, pos = self.get_mt19937()
        st = np.random.get_state()
        np.random.set_state((st[0], key, pos, 0, 0.0))

    # -- tree -----------------------------------------------------------------------------------
    def tree_reset(self, x0):
        x0 = nat.as_f64(x0, (self.n,))
        nat.check(nat.lib().lqrrt_tree_reset(self.h, nat.ptr(x0), self._stream()))
        self.generation += 1

    def tree_load(self, states, K, pID, edge_len=None, xedge=None, uedge=None, ignored=None):
        """Puts an existing tree on the device (lqrrt_tree_load): states (N, n), K (N, m, n), pID (N,), optionally the
        edge lengths (N,) with the packed edges (sum(len), n) / (sum(len), m) and the ignore flags (N,)."""
        states = nat.as_f64(states)
        N = len(states)
        states = nat.as_f64(states, (N, self.n))
        K = nat.as_f64(K, (N, self.m, self.n))
        pID = np.ascontiguousarray(pID, dtype=np.int32)
        if pID.shape != (N,):
            raise ValueError("expected %d parent IDs" % N)
        keep = [states, K, pID]

        def opt(a, dtype, shape=None):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dtype)
            if shape is not None and a.shape != shape:
                raise ValueError("expected array of shape %r, got %r" % (shape, a.shape))
            keep.append(a)
            return nat.ptr(a)
        el = opt(edge_len, np.int32, (N,))
        rows = int(np.sum(edge_len)) if edge_len is not None else N
        nat.check(nat.lib().lqrrt_tree_load(self.h, N, nat.ptr(states), nat.ptr(K), nat.ptr(pID), el,
                                            opt(xedge, np.float64, (rows, self.n)), opt(uedge, np.float64, (rows, self.m)),
                                            opt(ignored, np.uint8, (N,)), self._stream()))
        self.generation += 1

    def tree_retain(self, root, revalidate=True):
        """Keeps the subtree below node `root` as the tree of the next plan, in place (lqrrt_tree_retain; the rule:
        tests/retain_reference.py): with `revalidate` every kept edge is tested again against the engine's current geometry and
        what hangs below a failing edge is dropped; kept nodes are renumbered in ascending order, goal bookkeeping and ignore set
        are rebuilt against the current goal.  Returns (stats dict, old_to_new int32 array, -1 = dropped)."""
        st = nat.RetainStats()
        old_to_new = np.empty(max(self.size, 1), dtype=np.int32)
        nat.check(nat.lib().lqrrt_tree_retain(self.h, int(root), 1 if revalidate else 0, C.byref(st), nat.ptr(old_to_new),
                                              self._stream()))
        self.generation += 1          # bound Tree views of the old numbering are dead
        return st.as_dict(), old_to_new[:st.old_size]

    @staticmethod
    def tree_retain_multi(engines, roots, revalidate=True):
        """lqrrt_tree_retain_multi: tree_retain for n engines in one native call -- every stage one kernel launch that spans the
        engines, allocations and waits per call instead of per engine.  `roots`: one node id per engine; `revalidate`: one flag for
        all or one per engine.  Returns [(stats dict, old_to_new)] in the engines' order, each exactly what that engine's own
        tree_retain(root, revalidate) returns.  The engines share device, model, horizon and form of S.  Every argument is checked
        before any tree is touched (ValueError / NativeError as tree_retain); after a failure past that point the trees of all
        engines of the call are undefined."""
        engines = list(engines)
        n = len(engines)
        if n < 1:
            raise ValueError("no engines")
        roots = np.ascontiguousarray([int(r) for r in roots], dtype=np.int32)
        if roots.shape != (n,):
            raise ValueError("expected one root per engine")
        flags = np.ascontiguousarray(np.broadcast_to(np.asarray(revalidate, dtype=bool), (n,)), dtype=np.int32)
        handles = (C.c_void_p * n)(*[e.h for e in engines])
        stats = (nat.RetainStats * n)()
        maps = [np.empty(max(e.size, 1), dtype=np.int32) for e in engines]
        map_ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in maps])
        try:
            nat.check(nat.lib().lqrrt_tree_retain_multi(handles, n, nat.ptr(roots), nat.ptr(flags), stats, map_ptrs,
                                                        engines[0]._stream()))
        except ValueError:
            raise                         # (bad arguments are refused before anything is written: trees and views stand)
        except Exception:
            for e in engines:
                e.generation += 1         # (whatever the trees are now, views of the old ones are dead)
            raise
        for e in engines:
            e.generation += 1             # bound Tree views of the old numbering are dead
        return [(stats[i].as_dict(), maps[i][:stats[i].old_size]) for i in range(n)]

    @staticmethod
    def track_table(tracks, radii, start=0):
        """(tracks [L][D][2], radii [D], start) as lqrrt_tree_clear takes them, or ValueError.  `tracks` is an array (L, D, 2) -- D
        discs at L consecutive instants -- or a list of D arrays (L_d, 2), each padded to the longest by holding its last row;
        `radii` is one radius for all or one per disc.  Host only."""
        if isinstance(tracks, (list, tuple)):
            rows = [np.asarray(t, dtype=np.float64) for t in tracks]
            if len(rows) < 1 or any(t.ndim != 2 or t.shape[1] != 2 or len(t) < 1 for t in rows):
                raise ValueError("Expected tracks as an array (L, D, 2) or a list of D >= 1 arrays (L_d >= 1, 2).")
            L = max(len(t) for t in rows)
            table = np.empty((L, len(rows), 2))
            for d, t in enumerate(rows):
                table[:len(t), d] = t
                table[len(t):, d] = t[-1]                         # a track that has ended stays where it ended
        else:
            table = np.ascontiguousarray(tracks, dtype=np.float64)
        if table.ndim != 3 or table.shape[2] != 2 or table.shape[0] < 1 or table.shape[1] < 1:
            raise ValueError("Expected tracks as an array (L, D, 2) with L >= 1 and D >= 1, or a list of D arrays (L_d, 2).")
        if not np.all(np.isfinite(table)):
            raise ValueError("A track position is not finite.")
        D = table.shape[1]
        r = np.asarray(radii, dtype=np.float64)
        if r.shape not in [(), (D,)]:
            raise ValueError("Expected radii to be one radius or one per disc (%d)." % D)
        r = np.ascontiguousarray(np.broadcast_to(r, (D,)))
        if not np.all(r >= 0):
            raise ValueError("A radius must be >= 0.")
        if int(start) != start or int(start) < 0:
            raise ValueError("start must be an integer >= 0.")
        return np.ascontiguousarray(table), r, int(start)

    def tree_clear(self, tracks, radii, start=0, per_node=False):
        """Which plans of the tree stay clear of moving discs (lqrrt_tree_clear; the rule: tests/clear_reference.py).  `tracks`,
        `radii`: what track_table takes -- the discs' centres at consecutive instants spaced by the engine's dt; row `start` of
        the table coincides with the root's row.  Returns the counters (dict: size, conflicts, blocked, hits, clear_hits, best_end,
        best_steps), and with `per_node` also first [N] and dwell_first [N] (int32: the time index of the first conflict on a
        node's root path, -1 = clear; for a goal hit the first conflict while it waits at the goal, -1 = none, -2 = not a hit).
        Reads only: tree, goal bookkeeping and footprint stay as they are."""
        return self._clear("lqrrt_tree_clear", nat.ClearStats, np.int32, tracks, radii, start, None, per_node)

    @staticmethod
    def rect_table(tracks, extents, start=0):
        """(tracks [L][D][3], extents [D][2], start) as lqrrt_tree_clear_rects takes them, or ValueError.  `tracks` is an array
        (L, D, 3) -- world x, y and heading of D rectangles at L consecutive instants -- or a list of D arrays (L_d, 3), each padded
        to the longest by holding its last row; `extents` is one (half length, half width) for all, or one pair per rectangle.
        Host only."""
        if isinstance(tracks, (list, tuple)):
            rows = [np.asarray(t, dtype=np.float64) for t in tracks]
            if len(rows) < 1 or any(t.ndim != 2 or t.shape[1] != 3 or len(t) < 1 for t in rows):
                raise ValueError("Expected tracks as an array (L, D, 3) or a list of D >= 1 arrays (L_d >= 1, 3).")
            L = max(len(t) for t in rows)
            table = np.empty((L, len(rows), 3))
            for d, t in enumerate(rows):
                table[:len(t), d] = t
                table[len(t):, d] = t[-1]                         # a track that has ended stays where it ended
        else:
            table = np.ascontiguousarray(tracks, dtype=np.float64)
        if table.ndim != 3 or table.shape[2] != 3 or table.shape[0] < 1 or table.shape[1] < 1:
            raise ValueError("Expected tracks as an array (L, D, 3) with L >= 1 and D >= 1, or a list of D arrays (L_d, 3).")
        if not np.all(np.isfinite(table)):
            raise ValueError("A track position or heading is not finite.")
        D = table.shape[1]
        ext = np.asarray(extents, dtype=np.float64)
        if ext.shape not in [(2,), (D, 2)]:
            raise ValueError("Expected extents to be one (half length, half width), or one pair per rectangle (%d)." % D)
        ext = np.ascontiguousarray(np.broadcast_to(ext, (D, 2)))
        if not (np.all(ext >= 0) and np.all(np.isfinite(ext))):
            raise ValueError("An extent must be >= 0 and finite.")
        if int(start) != start or int(start) < 0:
            raise ValueError("start must be an integer >= 0.")
        return np.ascontiguousarray(table), ext, int(start)

    def tree_clear_rects(self, tracks, extents, start=0, per_node=False):
        """tree_clear against moving oriented rectangles (lqrrt_tree_clear_rects; the rule: tests/clear_rects_reference.py).
        `tracks`, `extents`: what rect_table takes -- the rectangles' x, y and heading at consecutive instants spaced by the
        engine's dt, and their half length (along the heading) and half width; row `start` of the table coincides with the root's
        row.  Returns what tree_clear returns: the counters, and with `per_node` also first [N] and dwell_first [N] (int32).
        Reads only: tree, goal bookkeeping and footprint stay as they are."""
        table, ext, start = self.rect_table(tracks, extents, start)
        st = nat.ClearStats()
        a = b = None
        if per_node:
            n = max(self.size, 1)
            a, b = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        nat.check(nat.lib().lqrrt_tree_clear_rects(self.h, nat.ptr(table), nat.ptr(ext), table.shape[0], table.shape[1], start, C.byref(st),
                                                   None if a is None else nat.ptr(a), None if b is None else nat.ptr(b), self._stream()))
        if per_node:
            return st.as_dict(), a[:st.size], b[:st.size]
        return st.as_dict()

    def tree_clear_connect(self, tracks, radii, start, horizon_iters, tries=8, nodes=None, per_node=False):
        """tree_clear and connect_search in one native call (lqrrt_tree_clear_connect; the rule: tests/clear_connect_reference.py):
        besides tree_clear's answer, the node whose root path is clear of the discs and whose goal chain -- up to `tries` steers at
        the goal with the fixed horizon `horizon_iters`, as connect_search makes them -- stays clear of them at its own times, waits
        at the goal unharmed and gives a plan strictly shorter than the best clear hit.  `nodes`: None (every node) or an id list.
        Returns (stats, chain) and with `per_node` also first [N] and dwell_first [N]: `stats` is tree_clear's dict, `chain` holds
        clear_candidates (candidates whose root path is clear), chain_from (the winner, -1: none), chain_cost (steps from the root,
        the root's included), chain_rows and chain_arrival (best_steps after connect_commit(chain_from, horizon_iters, tries)).
        Reads only: tree, goal bookkeeping and footprint stay as they are."""
        table, r, start = self.track_table(tracks, radii, start)
        ids, ids_ptr, count = self._id_list(nodes)
        if ids is not None and count == 0:
            ids = np.zeros(1, dtype=np.int32)                     # (an empty list still has an address)
            ids_ptr = nat.ptr(ids)
        st, ch = nat.ClearStats(), nat.ClearConnectStats()
        a = b = None
        if per_node:
            n = max(self.size, 1)
            a, b = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        nat.check(nat.lib().lqrrt_tree_clear_connect(self.h, nat.ptr(table), nat.ptr(r), table.shape[0], table.shape[1], start,
                                                     int(horizon_iters), int(tries), ids_ptr, count, C.byref(st), C.byref(ch),
                                                     None if a is None else nat.ptr(a), None if b is None else nat.ptr(b), self._stream()))
        if per_node:
            return st.as_dict(), ch.as_dict(), a[:st.size], b[:st.size]
        return st.as_dict(), ch.as_dict()

    @staticmethod
    def wait_count(waits, what="waits", lo=1, hi=64):
        """`waits` as an integer in lo .. hi, or ValueError.  Host only."""
        if isinstance(waits, (bool, np.bool_)) or not isinstance(waits, (int, np.integer)) or not lo <= int(waits) <= hi:
            raise ValueError("%s must be an integer in %d .. %d." % (what, lo, hi))
        return int(waits)

    def tree_clear_wait(self, tracks, radii, start=0, waits=1, per_node=False):
        """tree_clear for the departure delays w = 0 .. waits - 1 at once, 1 <= waits <= 64 (lqrrt_tree_clear_wait; the rule:
        tests/clear_wait_reference.py): the vehicle holds the root's row for w rows of dt, tested there at every instant of the
        wait, and then follows the tree w rows later.  `tracks`, `radii`, `start`: what track_table takes.  Returns the counters
        (dict: size, hits, clear_hits -- hits that are clear at some delay --, clear_now -- at delay 0: tree_clear's clear_hits --,
        best_end, best_wait, best_steps -- without the wait --, best_arrival = best_wait + best_steps; -1 without a best), and with
        `per_node` also clear [N] and dwell_ok [N] (uint64: bit w of clear = the node's root path and the wait before it are clear
        at delay w; bit w of dwell_ok = a goal hit can wait at the goal from its arrival at delay w on, 0 for a node that is no
        hit).  Reads only: tree, goal bookkeeping and footprint stay as they are."""
        return self._clear("lqrrt_tree_clear_wait", nat.ClearWaitStats, np.uint64, tracks, radii, start, waits, per_node)

    def tree_clear_rects_wait(self, tracks, extents, start=0, waits=1, per_node=False):
        """tree_clear_wait against moving oriented rectangles (lqrrt_tree_clear_rects_wait; the rule:
        tests/clear_rects_wait_reference.py): tree_clear_rects for the departure delays w = 0 .. waits - 1 at once, 1 <= waits <= 64,
        the root's row tested at every instant of the wait.  `tracks`, `extents`, `start`: what rect_table takes.  Returns what
        tree_clear_wait returns: its counters, and with `per_node` also clear [N] and dwell_ok [N] (uint64 masks over the delays).
        Reads only: tree, goal bookkeeping and footprint stay as they are."""
        table, ext, start = self.rect_table(tracks, extents, start)
        waits = self.wait_count(waits)
        st = nat.ClearWaitStats()
        a = b = None
        if per_node:
            n = max(self.size, 1)
            a, b = np.empty(n, dtype=np.uint64), np.empty(n, dtype=np.uint64)
        nat.check(nat.lib().lqrrt_tree_clear_rects_wait(self.h, nat.ptr(table), nat.ptr(ext), table.shape[0], table.shape[1], start, waits,
                                                        C.byref(st), None if a is None else nat.ptr(a), None if b is None else nat.ptr(b),
                                                        self._stream()))
        if per_node:
            return st.as_dict(), a[:st.size], b[:st.size]
        return st.as_dict()

    def _clear(self, call, stats, dtype, tracks, radii, start, waits, per_node):
        """tree_clear (`waits` None) and tree_clear_wait: the arguments checked in their order, the counters, and with `per_node`
        the call's two arrays [N] of `dtype`."""
        table, r, start = self.track_table(tracks, radii, start)
        extra = () if waits is None else (self.wait_count(waits),)
        st = stats()
        a = b = None
        if per_node:
            n = max(self.size, 1)
            a, b = np.empty(n, dtype=dtype), np.empty(n, dtype=dtype)
        nat.check(getattr(nat.lib(), call)(self.h, nat.ptr(table), nat.ptr(r), table.shape[0], table.shape[1], start, *extra, C.byref(st),
                                           None if a is None else nat.ptr(a), None if b is None else nat.ptr(b), self._stream()))
        if per_node:
            return st.as_dict(), a[:st.size], b[:st.size]
        return st.as_dict()

    @staticmethod
    def tree_clear_multi(engines, tables, radii, starts, per_node=False):
        """tree_clear for n engines in one native call (lqrrt_tree_clear_multi): every stage one kernel launch that spans the
        engines, one allocation per chunk of 32 and one wait per call.  `tables`, `radii`, `starts`: one entry per engine, each
        what track_table takes; engines that are handed the SAME table and radii objects (arrays, as track_table returns them)
        share one upload.  Returns, per engine, exactly what its own tree_clear(tables[k], radii[k], starts[k], per_node) returns.
        The engines share device and model.  Every argument of every engine is checked before anything is launched (ValueError /
        NativeError as tree_clear, the message naming the engine); nothing of any tree is written."""
        return Engine._clear_multi("lqrrt_tree_clear_multi", nat.ClearStats, np.int32, engines, tables, radii, starts, None, per_node)

    @staticmethod
    def tree_clear_wait_multi(engines, tables, radii, starts, waits, per_node=False):
        """tree_clear_wait for n engines in one native call (lqrrt_tree_clear_wait_multi), as tree_clear_multi; `waits`: one count
        for all or one per engine, each 1 .. 64.  Returns, per engine, exactly what its own tree_clear_wait returns."""
        return Engine._clear_multi("lqrrt_tree_clear_wait_multi", nat.ClearWaitStats, np.uint64, engines, tables, radii, starts, waits,
                                   per_node)

    @staticmethod
    def tree_clear_rects_multi(engines, tables, extents, starts, per_node=False):
        """tree_clear_rects for n engines in one native call (lqrrt_tree_clear_rects_multi; csrc/clear_rects_multi.hpp), as
        tree_clear_multi: every stage one kernel launch that spans the engines, one allocation per chunk of 32 and one wait per
        call.  `tables`, `extents`, `starts`: one entry per engine, each what rect_table takes; engines that are handed the SAME
        table and extents objects (arrays, as rect_table returns them) share one upload.  Returns, per engine, exactly what its own
        tree_clear_rects(tables[k], extents[k], starts[k], per_node) returns.  The engines share device and model.  Every argument
        of every engine is checked before anything is launched (ValueError / NativeError as tree_clear_rects, the message naming
        the engine); nothing of any tree is written."""
        return Engine._clear_multi("lqrrt_tree_clear_rects_multi", nat.ClearStats, np.int32, engines, tables, extents, starts, None,
                                   per_node, rects=True)

    @staticmethod
    def tree_clear_rects_wait_multi(engines, tables, extents, starts, waits, per_node=False):
        """tree_clear_rects_wait for n engines in one native call (lqrrt_tree_clear_rects_wait_multi), as tree_clear_rects_multi;
        `waits`: one count for all or one per engine, each 1 .. 64.  Returns, per engine, exactly what its own
        tree_clear_rects_wait returns."""
        return Engine._clear_multi("lqrrt_tree_clear_rects_wait_multi", nat.ClearWaitStats, np.uint64, engines, tables, extents, starts,
                                   waits, per_node, rects=True)

    @staticmethod
    def tree_clear_connect_multi(engines, tables, radii, starts, horizons, tries=8, nodes=None, per_node=False):
        """tree_clear_connect for n engines in one native call (lqrrt_tree_clear_connect_multi; csrc/clear_connect_multi.hpp):
        tree_clear_multi's stages, then ONE launch that seeds every tree's key and ONE search launch over the candidates of all
        trees, every tree with a key of its own; one allocation per chunk of 32 and one wait per call.  `tables`, `radii`, `starts`:
        as tree_clear_multi takes them (the same table and radii objects share one upload); `horizons`: one per engine; `tries`:
        one for all or one per engine; `nodes`: None, or one entry per engine, each None (every node) or an id list (it may repeat
        ids; an empty one: the clearance answer and no chain).  Returns, per engine, exactly what its own tree_clear_connect(
        tables[k], radii[k], starts[k], horizons[k], tries[k], nodes[k], per_node) returns.  The engines share device and model.
        Every argument of every engine is checked before anything is launched (ValueError / NativeError as tree_clear_connect, the
        message naming the engine); nothing of any tree is written."""
        return Engine._clear_multi("lqrrt_tree_clear_connect_multi", nat.ClearStats, np.int32, engines, tables, radii, starts, None,
                                   per_node, connect=(horizons, tries, nodes))

    @staticmethod
    def _clear_multi(call, stats, dtype, engines, tables, radii, starts, waits, per_node, connect=None, rects=False):
        """tree_clear_multi (`waits` None), tree_clear_wait_multi and tree_clear_connect_multi (`connect`: horizons, tries, nodes):
        every engine's arguments checked in the solo calls' order, one native call, and per engine what _clear / tree_clear_connect
        returns.  `rects`: the tables are rect_table's and `radii` holds the extents (tree_clear_rects_multi,
        tree_clear_rects_wait_multi); the rest is the same."""
        build, second = (Engine.rect_table, "extents") if rects else (Engine.track_table, "radii")
        engines = list(engines)
        n = len(engines)
        if n < 1:
            raise ValueError("no engines")
        tables, radii, starts = list(tables), list(radii), list(starts)
        if not len(tables) == len(radii) == len(starts) == n:
            raise ValueError("expected one track table, one %s array and one start per engine" % second)
        if waits is not None:
            waits = [waits] * n if isinstance(waits, (int, np.integer)) else list(waits)
            if len(waits) != n:
                raise ValueError("expected one wait count, or one per engine")
            waits = np.array([Engine.wait_count(w) for w in waits], dtype=np.int32)
        # (track_table hands a contiguous float64 table back as it is: engines given one object keep one pointer)
        seen, tabs = {}, []
        for k in range(n):
            key = (id(tables[k]), id(radii[k]))
            if key not in seen:
                seen[key] = build(tables[k], radii[k], 0)[:2]
            tabs.append(seen[key])
            if int(starts[k]) != starts[k] or int(starts[k]) < 0:
                raise ValueError("start must be an integer >= 0.")
        Ls = np.array([t.shape[0] for t, _ in tabs], dtype=np.int32)
        Ds = np.array([t.shape[1] for t, _ in tabs], dtype=np.int32)
        st0 = np.array([int(s) for s in starts], dtype=np.int64)
        if np.any(st0 > 2 ** 31 - 1):
            raise ValueError("start leaves 31 bits.")
        st0 = st0.astype(np.int32)
        chain, keep = None, None
        if connect is not None:
            horizons, tries, nodes = connect
            horizons = np.ascontiguousarray([int(h) for h in horizons], dtype=np.int32)
            if horizons.shape != (n,):
                raise ValueError("expected one horizon per engine")
            tries = [tries] * n if isinstance(tries, (int, np.integer)) else list(tries)
            if len(tries) != n:
                raise ValueError("expected one goal_tries, or one per engine")
            tries = np.ascontiguousarray([int(t) for t in tries], dtype=np.int32)
            keep, node_ptrs, counts_ptr = Engine._id_lists(nodes, n)
            chain = (nat.ClearConnectStats * n)()
        handles = (C.c_void_p * n)(*[e.h for e in engines])
        t_ptrs = (C.c_void_p * n)(*[t.ctypes.data for t, _ in tabs])
        r_ptrs = (C.c_void_p * n)(*[r.ctypes.data for _, r in tabs])
        out = (stats * n)()
        a = b = a_ptrs = b_ptrs = None
        if per_node:
            a = [np.empty(max(e.size, 1), dtype=dtype) for e in engines]
            b = [np.empty(max(e.size, 1), dtype=dtype) for e in engines]
            a_ptrs = (C.c_void_p * n)(*[x.ctypes.data for x in a])
            b_ptrs = (C.c_void_p * n)(*[x.ctypes.data for x in b])
        extra = () if waits is None else (nat.ptr(waits),)
        if connect is not None:
            nat.check(getattr(nat.lib(), call)(handles, n, t_ptrs, r_ptrs, nat.ptr(Ls), nat.ptr(Ds), nat.ptr(st0), nat.ptr(horizons),
                                               nat.ptr(tries), node_ptrs, counts_ptr, out, chain, a_ptrs, b_ptrs, engines[0]._stream()))
            del keep                                              # (the id lists lived until here)
            if per_node:
                return [(out[k].as_dict(), chain[k].as_dict(), a[k][:out[k].size], b[k][:out[k].size]) for k in range(n)]
            return [(out[k].as_dict(), chain[k].as_dict()) for k in range(n)]
        nat.check(getattr(nat.lib(), call)(handles, n, t_ptrs, r_ptrs, nat.ptr(Ls), nat.ptr(Ds), nat.ptr(st0), *extra, out, a_ptrs, b_ptrs,
                                           engines[0]._stream()))
        if per_node:
            return [(out[k].as_dict(), a[k][:out[k].size], b[k][:out[k].size]) for k in range(n)]
        return [out[k].as_dict() for k in range(n)]

    def tree_truncate(self, size):
        nat.check(nat.lib().lqrrt_tree_truncate(self.h, int(size)))
        self.epoch += 1

    def set_ignored(self, flags, first=0):
        flags = np.ascontiguousarray(flags, dtype=np.uint8)
        nat.check(nat.lib().lqrrt_tree_set_ignored(self.h, int(first), len(flags), nat.ptr(flags)))

    def edges(self, first=0, count=None, pinned=False):
        """(x [count][H][n], u [count][H][m], len [count]) in three copies instead of one per node.  pinned: the two big arrays
        are views of page-locked host memory (torch's caching host allocator) -- a copy out of HBM at PCIe speed instead of the
        ~0.7 GB/s a pageable destination gets; for snapshots of whole trees (Tree._detach: 18 MB per 12k nodes)."""
        count = self.size - first if count is None else count
        H = max(self.horizon_iters or 1, 1)
        if pinned:
            torch = _torch()
            x = torch.empty((count, H, self.n), dtype=torch.float64, pin_memory=True).numpy()
            u = torch.empty((count, H, self.m), dtype=torch.float64, pin_memory=True).numpy()
        else:
            x = np.empty((count, H, self.n))
            u = np.empty((count, H, self.m))
        nat.check(nat.lib().lqrrt_tree_get_edges(self.h, int(first), int(count), nat.ptr(x), nat.ptr(u)))
        return x, u, self.edge_lengths(first, count)

    def tree_mark(self):
        nat.check(nat.lib().lqrrt_tree_mark(self.h))

    def set_rewind_above(self, size):
        """Measurement aid: extend_multi rewinds this engine to its mark whenever a wave would begin above `size` nodes (0: off)."""
        nat.check(nat.lib().lqrrt_tree_set_rewind_above(self.h, int(size)))

    def tree_rewind(self):
        nat.check(nat.lib().lqrrt_tree_rewind(self.h))
        self.epoch += 1

    @property
    def size(self):
        return nat.check(nat.lib().lqrrt_tree_size(self.h))

    def states(self, first=0, count=None):
        count = self.size - first if count is None else count
        out = np.empty((count, self.n))
        nat.check(nat.lib().lqrrt_tree_get_states(self.h, first, count, nat.ptr(out)))
        return out

    def gains(self, first=0, count=None):
        count = self.size - first if count is None else count
        out = np.empty((count, self.m, self.n))
        nat.check(nat.lib().lqrrt_tree_get_gains(self.h, first, count, nat.ptr(out)))
        return out

    def parents(self, first=0, count=None):
        count = self.size - first if count is None else count
        out = np.empty(count, dtype=np.int32)
        nat.check(nat.lib().lqrrt_tree_get_parents(self.h, first, count, nat.ptr(out)))
        return out

    def edge_lengths(self, first=0, count=None):
        count = self.size - first if count is None else count
        out = np.empty(count, dtype=np.int32)
        nat.check(nat.lib().lqrrt_tree_get_edge_lengths(self.h, first, count, nat.ptr(out)))
        return out

    def edge(self, ID):
        H = max(self.horizon_iters or 1, 1)
        x = np.empty((H, self.n))
        u = np.empty((H, self.m))
        ln = nat.check(nat.lib().lqrrt_tree_get_edge(self.h, int(ID), nat.ptr(x), nat.ptr(u)))
        return x[:ln].copy(), u[:ln].copy()

    def ignored(self, first=0, count=None):
        count = self.size - first if count is None else count
        out = np.empty(count, dtype=np.uint8)
        nat.check(nat.lib().lqrrt_tree_get_ignored(self.h, first, count, nat.ptr(out)))
        return out.astype(bool)

    def climb(self, ID):
        """Node ids from the seed down to ID (tree.py:100-117), from the engine's host mirror of the parents: no device access."""
        cap = 4096
        while True:
            out = np.empty(cap, dtype=np.int32)
            rc = nat.lib().lqrrt_tree_climb(self.h, int(ID), nat.ptr(out), cap)
            if rc == nat.E_CAPACITY and cap < self.size + 1:
                cap = min(4 * cap, self.size + 1)
                continue
            return out[:nat.check(rc)].tolist()

    def edges_of(self, ids):
        """[(x [len][n], u [len][m])] of the listed nodes: one gather on the device, two copies out (lqrrt_tree_get_edges_of)."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        H = max(self.horizon_iters or 1, 1)
        x = np.empty((len(ids), H, self.n))
        u = np.empty((len(ids), H, self.m))
        ln = np.empty(len(ids), dtype=np.int32)
        nat.check(nat.lib().lqrrt_tree_get_edges_of(self.h, nat.ptr(ids), len(ids), nat.ptr(x), nat.ptr(u), nat.ptr(ln)))
        return [(x[k, :ln[k]].copy(), u[k, :ln[k]].copy()) for k in range(len(ids))]

    # -- batched operators (host arrays in, host arrays out; device memory via torch) ----------
    def _dev(self, a, shape):
        torch = _torch()
        a = nat.as_f64(a, shape)
        return torch.from_numpy(a).to("cuda:%d" % self.device)

    def feasible_batch(self, x, u=None):
        torch = _torch()
        B = len(x)
        dx = self._dev(x, (B, self.n))
        du = self._dev(u, (B, self.m)) if u is not None else None
        ok = torch.empty(B, dtype=torch.uint8, device=dx.device)
        nat.check(nat.lib().lqrrt_feasible_batch(self.h, dx.data_ptr(), du.data_ptr() if du is not None else None,
                                                 B, ok.data_ptr(), self._stream()))
        return ok.cpu().numpy().astype(bool)

    def dynamics_batch(self, x, u):
        torch = _torch()
        B = len(x)
        dx, du = self._dev(x, (B, self.n)), self._dev(u, (B, self.m))
        out = torch.empty_like(dx)
        nat.check(nat.lib().lqrrt_dynamics_batch(self.h, dx.data_ptr(), du.data_ptr(), B, out.data_ptr(), self._stream()))
        return out.cpu().numpy()

    def gain_batch(self, x, u=None):
        torch = _torch()
        B = len(x)
        dx = self._dev(x, (B, self.n))
        du = self._dev(u, (B, self.m)) if u is not None else None
        K = torch.empty((B, self.m, self.n), dtype=torch.float64, device=dx.device)
        nat.check(nat.lib().lqrrt_gain_batch(self.h, dx.data_ptr(), du.data_ptr() if du is not None else None,
                                             B, K.data_ptr(), self._stream()))
        return K.cpu().numpy()

    def erf_batch(self, xg, x):
        torch = _torch()
        B = len(x)
        dg, dx = self._dev(xg, (B, self.n)), self._dev(x, (B, self.n))
        e = torch.empty_like(dx)
        nat.check(nat.lib().lqrrt_erf_batch(self.h, dg.data_ptr(), dx.data_ptr(), B, e.data_ptr(), self._stream()))
        return e.cpu().numpy()

    def lqr_dare_batch(self, x, u, Q, R, eps=1e-6, outputs=("S", "K", "A", "B", "it")):
        """(S, K, A, B, iterations) of the finite-difference-linearised DARE at every (x[i], u[i]).  u = None: zero efforts (the
        native call's NULL).  outputs: A, B and "it" left out of it are not computed into memory (NULL) and come back as None."""
        torch = _torch()
        Bn = len(x)
        dev = "cuda:%d" % self.device
        if not {"S", "K"} <= set(outputs) <= {"S", "K", "A", "B", "it"}:
            raise ValueError("outputs: S and K, optionally A, B, it")
        dx = self._dev(x, (Bn, self.n))
        du = self._dev(u, (Bn, self.m)) if u is not None else None
        dQ, dR = self._dev(Q, (self.n, self.n)), self._dev(R, (self.m, self.m))
        S = torch.empty((Bn, self.n, self.n), dtype=torch.float64, device=dev)
        K = torch.empty((Bn, self.m, self.n), dtype=torch.float64, device=dev)
        A = torch.empty((Bn, self.n, self.n), dtype=torch.float64, device=dev) if "A" in outputs else None
        Bm = torch.empty((Bn, self.n, self.m), dtype=torch.float64, device=dev) if "B" in outputs else None
        it = torch.empty(Bn, dtype=torch.int32, device=dev) if "it" in outputs else None
        pu, pA, pB, pit = (t.data_ptr() if t is not None else None for t in (du, A, Bm, it))
        nat.check(nat.lib().lqrrt_lqr_dare_batch(self.h, dx.data_ptr(), pu, Bn, dQ.data_ptr(), dR.data_ptr(),
                                                 float(eps), S.data_ptr(), K.data_ptr(), pA, pB, pit, self._stream()))
        return tuple(t.cpu().numpy() if t is not None else None for t in (S, K, A, Bm, it))

    def nn_argmin(self, xs, S=None, use_ignore=True):
        torch = _torch()
        W = len(xs)
        dxs = self._dev(xs, (W, self.n))
        dS = self._dev(S, (self.n, self.n)) if S is not None else None
        ids = torch.empty(W, dtype=torch.int32, device=dxs.device)
        cost = torch.empty(W, dtype=torch.float64, device=dxs.device)
        nat.check(nat.lib().lqrrt_nn_argmin(self.h, dxs.data_ptr(), W, dS.data_ptr() if dS is not None else None,
                                            1 if use_ignore else 0, ids.data_ptr(), cost.data_ptr(), self._stream()))
        return ids.cpu().numpy(), cost.cpu().numpy()

    def costs_to_go(self, x, S=None):
        torch = _torch()
        dx = self._dev(x, (self.n,))
        dS = self._dev(S, (self.n, self.n)) if S is not None else None
        cost = torch.empty(self.size, dtype=torch.float64, device=dx.device)
        nat.check(nat.lib().lqrrt_costs_to_go(self.h, dx.data_ptr(), dS.data_ptr() if dS is not None else None,
                                              cost.data_ptr(), self._stream()))
        return cost.cpu().numpy()

    def steer_batch(self, parents, xtar):
        torch = _torch()
        W = len(xtar)
        H = self.horizon_iters
        dev = "cuda:%d" % self.device
        dp = torch.from_numpy(np.ascontiguousarray(parents, dtype=np.int32)).to(dev)
        dx = self._dev(xtar, (W, self.n))
        ln = torch.empty(W, dtype=torch.int32, device=dev)
        xs = torch.empty((W, H, self.n), dtype=torch.float64, device=dev)
        us = torch.empty((W, H, self.m), dtype=torch.float64, device=dev)
        xe = torch.empty((W, self.n), dtype=torch.float64, device=dev)
        Ke = torch.empty((W, self.m, self.n), dtype=torch.float64, device=dev)
        nat.check(nat.lib().lqrrt_steer_batch(self.h, dp.data_ptr(), dx.data_ptr(), W, ln.data_ptr(), xs.data_ptr(),
                                              us.data_ptr(), xe.data_ptr(), Ke.data_ptr(), self._stream()))
        return ln.cpu().numpy(), xs.cpu().numpy(), us.cpu().numpy(), xe.cpu().numpy(), Ke.cpu().numpy()

    def steer_force(self, parent, xtar, max_steps, rtol=1e-4, atol=1e-4):
        torch = _torch()
        dev = "cuda:%d" % self.device
        dx = self._dev(xtar, (self.n,))
        ln = torch.zeros(1, dtype=torch.int32, device=dev)
        xs = torch.empty((max_steps, self.n), dtype=torch.float64, device=dev)
        us = torch.empty((max_steps, self.m), dtype=torch.float64, device=dev)
        nat.check(nat.lib().lqrrt_steer_force(self.h, int(parent), dx.data_ptr(), int(max_steps), float(rtol), float(atol),
                                              ln.data_ptr(), xs.data_ptr(), us.data_ptr(), self._stream()))
        k = int(ln.cpu()[0])
        return xs[:k].cpu().numpy(), us[:k].cpu().numpy()

    # -- plan refinement (csrc/engine_refine.hpp; the rule: tests/refine_reference.py) ---------
    def refine_round(self, plan, horizon_iters, incumbent, goal_tries=8):
        """One shortcut search over `plan` (node ids from the root): (cost, i, j) of the cheapest candidate whose chain reaches the
        goal in fewer than `incumbent` steps, or None (lqrrt_refine_search)."""
        ids = np.ascontiguousarray(plan, dtype=np.int32)
        cost, i, j = C.c_int64(), C.c_int32(), C.c_int32()
        nat.check(nat.lib().lqrrt_refine_search(self.h, nat.ptr(ids), len(ids), int(goal_tries), int(horizon_iters), int(incumbent),
                                                C.byref(cost), C.byref(i), C.byref(j), self._stream()))
        return None if i.value < 0 else (cost.value, i.value, j.value)

    def refine_commit(self, plan, horizon_iters, i, j, goal_tries=8):
        """Appends the chain of candidate (i, j) below plan[i] (lqrrt_refine_commit); returns the new node ids.  NativeError with
        code E_CAPACITY when the tree cannot hold it (the tree is then unchanged)."""
        ids = np.ascontiguousarray(plan, dtype=np.int32)
        out = np.empty(max(len(ids) - 1 - int(j) + int(goal_tries), 1), dtype=np.int32)
        k = nat.check(nat.lib().lqrrt_refine_commit(self.h, nat.ptr(ids), len(ids), int(goal_tries), int(horizon_iters), int(i), int(j),
                                                    nat.ptr(out), len(out), self._stream()))
        return out[:k].tolist()

    # What the wrappers of the refine, connect, via and reach calls share: how an argument of theirs becomes what the native call
    # takes.  The arrays they return are what the pointers point into: the caller holds them until the native call has returned.
    @staticmethod
    def _id_list(nodes, unique=False):
        """(ids, pointer, count) of a candidate id list: (None, None, 0) for None (every node), else a flat int32 array -- `unique`:
        sorted and freed of duplicates."""
        if nodes is None:
            return None, None, 0
        ids = np.ascontiguousarray(nodes, dtype=np.int32).reshape(-1)
        if unique:
            ids = np.unique(ids)
        return ids, nat.ptr(ids), len(ids)

    @staticmethod
    def _per_engine(values, n, what):
        values = list(values)
        if len(values) != n:
            raise ValueError("expected one %s per engine" % what)
        return values

    @staticmethod
    def _id_lists(nodes, n, unique=False):
        """(arrays, pointers, pointer to the counts) of one id list (or None) per engine, each as _id_list makes it; (None, None,
        None) for None."""
        if nodes is None:
            return None, None, None
        ids = [Engine._id_list(v, unique)[0] for v in Engine._per_engine(nodes, n, "id list (or None)")]
        counts = np.ascontiguousarray([0 if a is None else len(a) for a in ids], dtype=np.int32)
        ids = [a if a is None or len(a) else np.zeros(1, dtype=np.int32) for a in ids]    # (an empty list still has an address)
        return (ids, counts), (C.c_void_p * n)(*[None if a is None else a.ctypes.data for a in ids]), nat.ptr(counts)

    @staticmethod
    def _incumbents(incumbents, n, what="engine"):
        inc = np.ascontiguousarray([int(c) for c in incumbents], dtype=np.int64)
        if inc.shape != (n,):
            raise ValueError("expected one incumbent per %s" % what)
        return inc

    @staticmethod
    def _commit_outputs(rooms):
        """(outs, pointers, capacities, counts) of a commit for several engines: room for rooms[k] new ids of engine k."""
        outs = [np.empty(max(int(r), 1), dtype=np.int32) for r in rooms]
        out_ptrs = (C.c_void_p * len(outs))(*[a.ctypes.data for a in outs])
        return outs, out_ptrs, np.ascontiguousarray([len(a) for a in outs], dtype=np.int32), np.zeros(len(outs), dtype=np.int32)

    @staticmethod
    def _commit_results(outs, counts, message):
        """What a commit for several engines returns: per engine the new ids, None where the tree is full.  An engine whose chain
        fell short raises NativeError -- message(k) for the first such k -- that carries what the others committed."""
        results = [None if counts[k] < 0 else outs[k][:counts[k]].tolist() for k in range(len(outs))]
        bad = [k for k in range(len(outs)) if counts[k] < 0 and counts[k] != nat.E_CAPACITY]
        if bad:
            err = nat.NativeError(int(counts[bad[0]]), message(bad[0]))
            err.results, err.failed = results, bad                  # what the other engines of the call committed
            raise err
        return results

    @staticmethod
    def _refine_multi_args(engines, plans, horizons, goal_tries):
        engines, n, handles, horizons, tries = Engine._connect_multi_args(engines, horizons, goal_tries)
        plans = [np.ascontiguousarray(p, dtype=np.int32).reshape(-1) for p in Engine._per_engine(plans, n, "plan")]
        plan_ptrs = (C.c_void_p * n)(*[p.ctypes.data for p in plans])
        plan_lens = np.ascontiguousarray([len(p) for p in plans], dtype=np.int32)
        return engines, n, handles, plans, plan_ptrs, plan_lens, horizons, tries

    @staticmethod
    def refine_round_multi(engines, plans, horizons, incumbents, goal_tries=8):
        """refine_round for n engines in one native call (lqrrt_refine_search_multi): the searches of all plans share one kernel
        launch, every engine with a best key of its own.  `plans`, `horizons`, `incumbents`: one per engine; `goal_tries`: one for
        all or one per engine.  Returns [(cost, i, j) or None] in the engines' order, each what that engine's own refine_round
        returns.  The engines share device and model; every argument is checked before anything is launched."""
        engines, n, handles, plans, plan_ptrs, plan_lens, horizons, tries = Engine._refine_multi_args(engines, plans, horizons, goal_tries)
        inc = Engine._incumbents(incumbents, n)
        cost, i, j = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        nat.check(nat.lib().lqrrt_refine_search_multi(handles, n, plan_ptrs, nat.ptr(plan_lens), nat.ptr(tries), nat.ptr(horizons),
                                                      nat.ptr(inc), nat.ptr(cost), nat.ptr(i), nat.ptr(j), engines[0]._stream()))
        return [None if i[k] < 0 else (int(cost[k]), int(i[k]), int(j[k])) for k in range(n)]

    @staticmethod
    def refine_commit_multi(engines, plans, horizons, ijs, goal_tries=8):
        """refine_commit for n engines in one native call (lqrrt_refine_commit_multi): one workgroup per engine replays its
        candidate ijs[k] = (i, j) below its own tree size (None: the engine is left out and gets []).  Returns a list of new-id
        lists, None where the tree cannot hold the chain (that tree is unchanged; the others commit).  A candidate whose chain
        does not reach the goal raises NativeError(E_STATE) after the other engines have committed; the error carries what they
        appended (`results`: this list, `failed`: the indices of the engines that appended nothing for that reason)."""
        engines, n, handles, plans, plan_ptrs, plan_lens, horizons, tries = Engine._refine_multi_args(engines, plans, horizons, goal_tries)
        ijs = Engine._per_engine(ijs, n, "candidate")
        ci = np.ascontiguousarray([-1 if c is None else int(c[0]) for c in ijs], dtype=np.int32)
        cj = np.ascontiguousarray([-1 if c is None else int(c[1]) for c in ijs], dtype=np.int32)
        outs, out_ptrs, caps, counts = Engine._commit_outputs(len(plans[k]) - 1 - max(int(cj[k]), 0) + int(tries[k]) for k in range(n))
        nat.check(nat.lib().lqrrt_refine_commit_multi(handles, n, plan_ptrs, nat.ptr(plan_lens), nat.ptr(tries), nat.ptr(horizons),
                                                      nat.ptr(ci), nat.ptr(cj), out_ptrs, nat.ptr(caps), nat.ptr(counts),
                                                      engines[0]._stream()))
        return Engine._commit_results(outs, counts, lambda k: "candidate (%d, %d) of engine %d does not reach the goal: nothing appended"
                                      % (ci[k], cj[k], k))

    # -- tree-wide goal connection (csrc/engine_connect.hpp; the rule: tests/connect_reference.py) ---------
    def connect_search(self, horizon_iters, incumbent, goal_tries=8, nodes=None):
        """(cost, node) of the tree node -- any node, or one of `nodes` -- whose chain of up to `goal_tries` steers toward the goal
        reaches it in the fewest steps from the root, fewer than `incumbent`; None when there is none (lqrrt_connect_search)."""
        ids, ids_ptr, count = self._id_list(nodes)
        cost, node = C.c_int64(), C.c_int32()
        nat.check(nat.lib().lqrrt_connect_search(self.h, ids_ptr, count, int(goal_tries), int(horizon_iters), int(incumbent),
                                                 C.byref(cost), C.byref(node), self._stream()))
        return None if node.value < 0 else (cost.value, node.value)

    def connect_commit(self, node, horizon_iters, goal_tries=8):
        """Appends the goal chain of candidate `node` below it (lqrrt_connect_commit); returns the new node ids.  NativeError with
        code E_CAPACITY when the tree cannot hold it, E_STATE when the chain does not reach the goal (the tree is then unchanged)."""
        out = np.empty(max(int(goal_tries), 1), dtype=np.int32)
        k = nat.check(nat.lib().lqrrt_connect_commit(self.h, int(node), int(goal_tries), int(horizon_iters), nat.ptr(out), len(out),
                                                     self._stream()))
        return out[:k].tolist()

    # -- one tree asked about many goals (csrc/engine_reach.hpp; the rule: tests/reach_reference.py) ---------
    def _targets(self, goals, buffers):
        """The target table of a reach call: goals [T][n] and their boxes lo / hi [T][n] (`buffers`: one for all, or one per
        goal), each box what set_resolution computes for the engine's own goal."""
        goals = np.ascontiguousarray(goals, dtype=np.float64)
        if goals.ndim != 2 or goals.shape[1] != self.n:
            raise ValueError("expected goals of shape (T, %d)" % self.n)
        T = len(goals)
        try:
            buffers = np.broadcast_to(np.asarray(buffers, dtype=np.float64), (T, self.n))
        except ValueError:
            raise ValueError("expected one goal buffer of %d entries, or one per goal" % self.n)
        lo, hi = np.empty((T, self.n)), np.empty((T, self.n))
        for t in range(T):
            _, lo[t], hi[t] = self._goal_box(goals[t], buffers[t])
        return goals, lo, hi

    def reach_search(self, goals, buffers, horizon_iters, incumbents=None, goal_tries=8, nodes=None):
        """connect_search for T targets in one launch (lqrrt_reach_search): target t is the goal state goals[t] with the box
        goals[t] -/+ buffers[t] (`buffers`: one for all, or one per goal).  Returns [(cost, node) or None] * T, entry t what
        connect_search returns on an engine whose goal and goal buffer are target t's, with incumbents[t] (None: nothing to
        beat).  The engine's own goal is not involved, and nothing of the engine changes."""
        goals, lo, hi = self._targets(goals, buffers)
        T = len(goals)
        ids, ids_ptr, count = self._id_list(nodes)
        inc = None if incumbents is None else self._incumbents(incumbents, T, "goal")
        cost, node = np.empty(max(T, 1), dtype=np.int64), np.empty(max(T, 1), dtype=np.int32)
        nat.check(nat.lib().lqrrt_reach_search(self.h, nat.ptr(goals), nat.ptr(lo), nat.ptr(hi), T, ids_ptr, count, int(goal_tries),
                                               int(horizon_iters), None if inc is None else nat.ptr(inc), nat.ptr(cost), nat.ptr(node),
                                               self._stream()))
        return [None if node[t] < 0 else (int(cost[t]), int(node[t])) for t in range(T)]

    def reach_commit(self, goal, buffer, node, horizon_iters, goal_tries=8):
        """connect_commit toward the target `goal` with the box goal -/+ buffer (lqrrt_reach_commit): appends the chain of
        candidate `node` below it and returns the new node ids.  NativeError with code E_CAPACITY when the tree cannot hold it,
        E_STATE when the chain does not reach the target (the tree is then unchanged).  The engine's own goal is not touched."""
        goals, lo, hi = self._targets(np.asarray(goal, dtype=np.float64).reshape(1, -1), buffer)
        out = np.empty(max(int(goal_tries), 1), dtype=np.int32)
        k = nat.check(nat.lib().lqrrt_reach_commit(self.h, nat.ptr(goals), nat.ptr(lo), nat.ptr(hi), int(node), int(goal_tries),
                                                   int(horizon_iters), nat.ptr(out), len(out), self._stream()))
        return out[:k].tolist()

    # -- goal chains through waypoints (csrc/engine_connect_via.hpp; the rule: tests/connect_via_reference.py) ---------
    def _waypoints(self, waypoints):
        way = np.ascontiguousarray(waypoints, dtype=np.float64)
        if way.size == 0 and way.ndim <= 2:
            way = way.reshape(0, self.n)                            # (no waypoints, however the caller spells it)
        if way.ndim != 2 or way.shape[1] != self.n:
            raise ValueError("expected waypoints of shape (Q, %d)" % self.n)
        return way

    def connect_via_search(self, waypoints, horizon_iters, incumbent, goal_tries=8, nodes=None):
        """(cost, node, j) of the cheapest chain that starts at a tree node -- any node, or one of `nodes` --, steers toward
        waypoints[j], waypoints[j + 1], ... and then up to `goal_tries` times toward the goal, and reaches the goal box in fewer than
        `incumbent` steps from the root; ties to the smaller node id, then the smaller j; None when there is none
        (lqrrt_connect_via_search).  j = len(waypoints) is connect_search's candidate.  An id list is sorted and its duplicates are
        removed: the winner does not depend on its order."""
        way = self._waypoints(waypoints)
        ids, ids_ptr, count = self._id_list(nodes, unique=True)
        cost, node, j = C.c_int64(), C.c_int32(), C.c_int32()
        nat.check(nat.lib().lqrrt_connect_via_search(self.h, ids_ptr, count, nat.ptr(way) if len(way) else None, len(way),
                                                     int(goal_tries), int(horizon_iters), int(incumbent), C.byref(cost),
                                                     C.byref(node), C.byref(j), self._stream()))
        return None if node.value < 0 else (cost.value, node.value, j.value)

    def connect_via_commit(self, node, j, waypoints, horizon_iters, goal_tries=8):
        """Appends the chain of candidate (node, j) over `waypoints` below `node` (lqrrt_connect_via_commit); returns the new node
        ids.  NativeError with code E_CAPACITY when the tree cannot hold it, E_STATE when the chain does not reach the goal (the tree
        is then unchanged)."""
        way = self._waypoints(waypoints)
        out = np.empty(max(len(way) + int(goal_tries), 1), dtype=np.int32)
        k = nat.check(nat.lib().lqrrt_connect_via_commit(self.h, int(node), int(j), nat.ptr(way) if len(way) else None, len(way),
                                                         int(goal_tries), int(horizon_iters), nat.ptr(out), len(out), self._stream()))
        return out[:k].tolist()

    @staticmethod
    def _connect_multi_args(engines, horizons, goal_tries):
        engines = list(engines)
        n = len(engines)
        if n < 1:
            raise ValueError("no engines")
        horizons = np.ascontiguousarray([int(h) for h in horizons], dtype=np.int32)
        tries = np.ascontiguousarray(np.broadcast_to(np.asarray(goal_tries, dtype=np.int64), (n,)), dtype=np.int32)
        if horizons.shape != (n,):
            raise ValueError("expected one horizon per engine")
        handles = (C.c_void_p * n)(*[e.h for e in engines])
        return engines, n, handles, horizons, tries

    @staticmethod
    def connect_search_multi(engines, horizons, incumbents, goal_tries=8, nodes=None):
        """connect_search for n engines in one native call (lqrrt_connect_search_multi): the searches of all trees share one kernel
        launch, every engine with a best key of its own.  `horizons`, `incumbents`: one per engine; `goal_tries`: one for all or one
        per engine; `nodes`: None, or one entry per engine, each None (every node) or an id list (an empty one: no candidates).
        Returns [(cost, node) or None] in the engines' order, each what that engine's own connect_search returns.  The engines share
        device and model; every argument is checked before anything is launched."""
        engines, n, handles, horizons, tries = Engine._connect_multi_args(engines, horizons, goal_tries)
        inc = Engine._incumbents(incumbents, n)
        ids, node_ptrs, counts_ptr = Engine._id_lists(nodes, n)
        cost, node = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int32)
        nat.check(nat.lib().lqrrt_connect_search_multi(handles, n, node_ptrs, counts_ptr, nat.ptr(tries), nat.ptr(horizons), nat.ptr(inc),
                                                       nat.ptr(cost), nat.ptr(node), engines[0]._stream()))
        return [None if node[k] < 0 else (int(cost[k]), int(node[k])) for k in range(n)]

    @staticmethod
    def connect_commit_multi(engines, nodes, horizons, goal_tries=8):
        """connect_commit for n engines in one native call (lqrrt_connect_commit_multi): one workgroup per engine replays the goal
        chain of its candidate nodes[k] below its own tree size (None: the engine is left out and gets []).  Returns a list of
        new-id lists, None where the tree cannot hold the chain (that tree is unchanged; the others commit).  A chain that does not
        reach the goal raises NativeError(E_STATE) after the other engines have committed; the error carries what they appended
        (`results`: this list, `failed`: the indices of the engines that appended nothing for that reason)."""
        engines, n, handles, horizons, tries = Engine._connect_multi_args(engines, horizons, goal_tries)
        nodes = Engine._per_engine(nodes, n, "candidate")
        if any(v is not None and int(v) < 0 for v in nodes):
            raise ValueError("a candidate is a node id >= 0, or None")
        cn = np.ascontiguousarray([-1 if v is None else int(v) for v in nodes], dtype=np.int32)
        outs, out_ptrs, caps, counts = Engine._commit_outputs(tries)
        nat.check(nat.lib().lqrrt_connect_commit_multi(handles, n, nat.ptr(cn), nat.ptr(tries), nat.ptr(horizons), out_ptrs, nat.ptr(caps),
                                                       nat.ptr(counts), engines[0]._stream()))
        return Engine._commit_results(outs, counts, lambda k: "the chain below node %d of engine %d does not reach the goal: nothing appended"
                                      % (cn[k], k))

    # -- goal chains through waypoints for several trees per call (csrc/engine_connect_via_multi.hpp) ---------
    @staticmethod
    def _waypoints_multi(engines, waypoints):
        """One table [Q][n] per engine (None or empty: Q = 0), the array of their addresses and their lengths."""
        waypoints = Engine._per_engine(waypoints, len(engines), "waypoint table (or None)")
        ways = [e._waypoints(() if w is None else w) for e, w in zip(engines, waypoints)]
        ptrs = (C.c_void_p * len(ways))(*[w.ctypes.data if len(w) else None for w in ways])
        return ways, ptrs, np.ascontiguousarray([len(w) for w in ways], dtype=np.int32)

    @staticmethod
    def connect_via_search_multi(engines, waypoints, horizons, incumbents, goal_tries=8, nodes=None):
        """connect_via_search for n engines in one native call (lqrrt_connect_via_search_multi): the searches of all trees share one
        kernel launch, every engine with its own waypoint table and a best key of its own.  `waypoints`: one entry per engine, an
        array [Q_k][n] or None / empty (Q_k = 0: connect_search's candidates); `horizons`, `incumbents`: one per engine;
        `goal_tries`: one for all or one per engine; `nodes`: None, or one entry per engine, each None (every node) or an id list
        (sorted and freed of duplicates as connect_via_search does; an empty one: no candidates).  Returns [(cost, node, j) or None]
        in the engines' order, each what that engine's own connect_via_search returns.  The engines share device and model; every
        argument is checked before anything is launched."""
        engines, n, handles, horizons, tries = Engine._connect_multi_args(engines, horizons, goal_tries)
        ways, way_ptrs, Q = Engine._waypoints_multi(engines, waypoints)
        inc = Engine._incumbents(incumbents, n)
        ids, node_ptrs, counts_ptr = Engine._id_lists(nodes, n, unique=True)
        cost, node, j = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        nat.check(nat.lib().lqrrt_connect_via_search_multi(handles, n, node_ptrs, counts_ptr, way_ptrs, nat.ptr(Q), nat.ptr(tries),
                                                           nat.ptr(horizons), nat.ptr(inc), nat.ptr(cost), nat.ptr(node), nat.ptr(j),
                                                           engines[0]._stream()))
        return [None if node[k] < 0 else (int(cost[k]), int(node[k]), int(j[k])) for k in range(n)]

    @staticmethod
    def connect_via_commit_multi(engines, candidates, waypoints, horizons, goal_tries=8):
        """connect_via_commit for n engines in one native call (lqrrt_connect_via_commit_multi): one workgroup per engine replays the
        chain of its candidate candidates[k] = (node, j) over its own waypoints below its own tree size (None: the engine is left
        out and gets []).  Returns a list of new-id lists, None where the tree cannot hold the chain (that tree is unchanged; the
        others commit).  A chain that does not reach the goal raises NativeError(E_STATE) after the other engines have committed; the
        error carries what they appended (`results`: this list, `failed`: the indices of the engines that appended nothing for that
        reason)."""
        engines, n, handles, horizons, tries = Engine._connect_multi_args(engines, horizons, goal_tries)
        ways, way_ptrs, Q = Engine._waypoints_multi(engines, waypoints)
        candidates = Engine._per_engine(candidates, n, "candidate")
        if any(c is not None and (int(c[0]) < 0 or int(c[1]) < 0) for c in candidates):
            raise ValueError("a candidate is a pair (node id >= 0, first waypoint >= 0), or None")
        cn = np.ascontiguousarray([-1 if c is None else int(c[0]) for c in candidates], dtype=np.int32)
        cj = np.ascontiguousarray([-1 if c is None else int(c[1]) for c in candidates], dtype=np.int32)
        outs, out_ptrs, caps, counts = Engine._commit_outputs(int(Q[k]) + int(tries[k]) for k in range(n))
        nat.check(nat.lib().lqrrt_connect_via_commit_multi(handles, n, nat.ptr(cn), nat.ptr(cj), way_ptrs, nat.ptr(Q), nat.ptr(tries),
                                                           nat.ptr(horizons), out_ptrs, nat.ptr(caps), nat.ptr(counts),
                                                           engines[0]._stream()))
        return Engine._commit_results(outs, counts, lambda k: "the chain of candidate (%d, %d) of engine %d does not reach the goal: "
                                      "nothing appended" % (cn[k], cj[k], k))

    # -- several trees asked about many goals per call (csrc/engine_reach_multi.hpp) ---------
    @staticmethod
    def _targets_multi(engines, goals, buffers):
        """One target table per engine as _targets makes it: (tables, pointers to the goals, the los, the his, the T_k)."""
        n = len(engines)
        goals, buffers = Engine._per_engine(goals, n, "goal table"), Engine._per_engine(buffers, n, "goal buffer (or one per goal)")
        tabs = [e._targets(g, b) for e, g, b in zip(engines, goals, buffers)]
        ptrs = [(C.c_void_p * n)(*[t[i].ctypes.data if len(t[i]) else None for t in tabs]) for i in range(3)]
        return tabs, ptrs[0], ptrs[1], ptrs[2], np.ascontiguousarray([len(t[0]) for t in tabs], dtype=np.int32)

    @staticmethod
    def reach_search_multi(engines, goals, buffers, horizons, incumbents=None, goal_tries=8, nodes=None):
        """reach_search for n engines in one native call (lqrrt_reach_search_multi): the searches of all trees for all their
        targets share one kernel launch, every (engine, target) pair with a best key of its own.  `goals`: one table [T_k][n] per
        engine; `buffers`: per engine one buffer, or one per goal; `horizons`: one per engine; `incumbents`: None, or one entry per
        engine, each None (nothing to beat) or [T_k]; `goal_tries`: one for all or one per engine; `nodes`: None, or one entry per
        engine, each None (every node) or an id list (an empty one: no candidates).  Returns a list, per engine, of
        [(cost, node) or None] * T_k, each what that engine's own reach_search returns.  The engines share device and model; every
        argument is checked before anything is launched, and nothing of any engine changes."""
        engines, n, handles, horizons, tries = Engine._connect_multi_args(engines, horizons, goal_tries)
        tabs, goal_ptrs, lo_ptrs, hi_ptrs, T = Engine._targets_multi(engines, goals, buffers)
        incs, inc_ptrs = None, None
        if incumbents is not None:
            incs = [None if c is None else Engine._incumbents(c, int(T[k]), "goal")
                    for k, c in enumerate(Engine._per_engine(incumbents, n, "incumbent list (or None)"))]
            inc_ptrs = (C.c_void_p * n)(*[None if a is None or not len(a) else a.ctypes.data for a in incs])
        ids, node_ptrs, counts_ptr = Engine._id_lists(nodes, n)
        cost = [np.empty(max(int(t), 1), dtype=np.int64) for t in T]
        node = [np.empty(max(int(t), 1), dtype=np.int32) for t in T]
        cost_ptrs, out_ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in cost]), (C.c_void_p * n)(*[a.ctypes.data for a in node])
        nat.check(nat.lib().lqrrt_reach_search_multi(handles, n, goal_ptrs, lo_ptrs, hi_ptrs, nat.ptr(T), node_ptrs, counts_ptr,
                                                     nat.ptr(tries), nat.ptr(horizons), inc_ptrs, cost_ptrs, out_ptrs,
                                                     engines[0]._stream()))
        return [[None if node[k][t] < 0 else (int(cost[k][t]), int(node[k][t])) for t in range(int(T[k]))] for k in range(n)]

    @staticmethod
    def reach_commit_multi(engines, goals, buffers, nodes, horizons, goal_tries=8):
        """reach_commit for n engines in one native call (lqrrt_reach_commit_multi): one workgroup per engine replays the chain of
        its candidate nodes[k] toward its ONE target goals[k] with the box goals[k] -/+ buffers[k], below its own tree size (None:
        the engine is left out and gets []).  Returns a list of new-id lists, None where the tree cannot hold the chain (that tree
        is unchanged; the others commit).  A chain that does not reach its target raises NativeError(E_STATE) after the other
        engines have committed; the error carries what they appended (`results`: this list, `failed`: the indices of the engines
        that appended nothing for that reason).  The engines' own goals are not touched."""
        engines, n, handles, horizons, tries = Engine._connect_multi_args(engines, horizons, goal_tries)
        goals = [np.asarray(g, dtype=np.float64).reshape(1, -1) for g in Engine._per_engine(goals, n, "goal")]
        tabs, goal_ptrs, lo_ptrs, hi_ptrs, T = Engine._targets_multi(engines, goals, buffers)
        nodes = Engine._per_engine(nodes, n, "candidate")
        if any(v is not None and int(v) < 0 for v in nodes):
            raise ValueError("a candidate is a node id >= 0, or None")
        cn = np.ascontiguousarray([-1 if v is None else int(v) for v in nodes], dtype=np.int32)
        outs, out_ptrs, caps, counts = Engine._commit_outputs(tries)
        nat.check(nat.lib().lqrrt_reach_commit_multi(handles, n, goal_ptrs, lo_ptrs, hi_ptrs, nat.ptr(cn), nat.ptr(tries),
                                                     nat.ptr(horizons), out_ptrs, nat.ptr(caps), nat.ptr(counts), engines[0]._stream()))
        return Engine._commit_results(outs, counts, lambda k: "the chain below node %d of engine %d does not reach the target: "
                                      "nothing appended" % (cn[k], k))

    def push_samples(self, xs):
        xs = nat.as_f64(xs)
        if xs.ndim != 2 or xs.shape[1] != self.n:
            raise ValueError("expected samples of shape (count, %d)" % self.n)
        nat.check(nat.lib().lqrrt_engine_push_samples(self.h, nat.ptr(xs), len(xs)))

    def queued_samples(self):
        return nat.check(nat.lib().lqrrt_engine_queued_samples(self.h))

    # -- wave engine -----------------------------------------------------------------------------
    def record_layout(self):
        lay = np.zeros(11, dtype=np.int32)
        nat.check(nat.lib().lqrrt_record_layout(self.h, nat.ptr(lay)))
        return lay

    def wave_records_ptr(self):
        p = C.c_void_p()
        nat.check(nat.lib().lqrrt_wave_records(self.h, C.byref(p)))
        return p.value

    def wave_suggest(self, wave_cap):
        return nat.check(nat.lib().lqrrt_wave_suggest(self.h, int(wave_cap)))

    def wave_speculate(self, W, lo, hi):
        nat.check(nat.lib().lqrrt_wave_speculate(self.h, W, lo, hi, self._stream()))

    def wave_scan_nodes(self, W, node_lo, node_hi, best_ptr):
        """Tree-sharded wave, phase 1: this rank's (cost, id) candidates [W][2] over nodes [node_lo, node_hi)."""
        nat.check(nat.lib().lqrrt_wave_scan_nodes(self.h, int(W), int(node_lo), int(node_hi), best_ptr, self._stream()))

    def wave_steer_candidates(self, W, parts, best_ptr):
        """Tree-sharded wave, phase 2: nearest node per sample from the gathered candidates [parts][W][2], then the steer."""
        nat.check(nat.lib().lqrrt_wave_steer_candidates(self.h, int(W), int(parts), best_ptr, self._stream()))

    def wave_commit(self, W, max_commit, node_limit, pruning=True):
        st = nat.ExtendStats()
        nat.check(nat.lib().lqrrt_wave_commit(self.h, W, int(max_commit), int(node_limit), 1 if pruning else 0,
                                              C.byref(st), self._stream()))
        return st

    def extend(self, wave, max_attempts=-1, node_limit=-1, until_size=0, pruning=True, stop_on_goal=False):
        st = nat.ExtendStats()
        nat.check(nat.lib().lqrrt_engine_extend(self.h, int(wave), int(max_attempts), int(node_limit), int(until_size),
                                                1 if pruning else 0, 1 if stop_on_goal else 0, C.byref(st),
                                                self._stream()))
        return st

    @staticmethod
    def extend_multi(engines, wave, max_attempts=-1, node_limit=-1, until_size=0, pruning=True, stop_on_goal=False):
        """lqrrt_engine_extend_multi: n independent engines (trees) advanced in lock step by one native loop, two launches per
        step whatever n is.  Every tree is what its engine grows alone with `extend`; returns the n stats blocks."""
        engines = list(engines)
        n = len(engines)
        if n < 1:
            raise ValueError("no engines")
        handles = (C.c_void_p * n)(*[e.h for e in engines])
        stats = (nat.ExtendStats * n)()
        nat.check(nat.lib().lqrrt_engine_extend_multi(handles, n, int(wave), int(max_attempts), int(node_limit), int(until_size),
                                                       1 if pruning else 0, 1 if stop_on_goal else 0, stats, engines[0]._stream()))
        return [stats[i] for i in range(n)]

    def extend_sharded(self, comm, scheme, wave, max_attempts=-1, node_limit=-1, until_size=0, pruning=True, stop_on_goal=False):
        """lqrrt_engine_extend_sharded: the native loop with one RCCL all-gather per wave (comm: parallel.NativeComm)."""
        st = nat.ExtendStats()
        nat.check(nat.lib().lqrrt_engine_extend_sharded(self.h, comm.h, {"sample": 0, "tree": 1}[scheme], int(wave), int(max_attempts),
                                                       int(node_limit), int(until_size), 1 if pruning else 0,
                                                       1 if stop_on_goal else 0, C.byref(st), self._stream()))
        return st

    def allgather_nodes(self, comm, W):
        nat.check(nat.lib().lqrrt_allgather_nodes(self.h, comm.h, int(W), self._stream()))

    def plan_best(self):
        end, steps, hits = C.c_int32(), C.c_int64(), C.c_int64()
        nat.check(nat.lib().lqrrt_plan_best(self.h, C.byref(end), C.byref(steps), C.byref(hits)))
        return end.value, steps.value, hits.value

    def counters(self):
        st = nat.ExtendStats()
        nat.check(nat.lib().lqrrt_engine_counters(self.h, C.byref(st)))
        return st

    def profile_enable(self, on=True, steer=True, every=1):
        """HIP-event timing of the NN scan launches (every `every`-th one) and of the steer launches when `steer`."""
        nat.check(nat.lib().lqrrt_profile_enable(self.h, ((2 if steer else 1) + 16 * (max(1, int(every)) - 1)) if on else 0))

    def profile_read(self):
        a, b, c, d, f = C.c_double(), C.c_int64(), C.c_double(), C.c_double(), C.c_int64()
        nat.check(nat.lib().lqrrt_profile_read(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(f)))
        return dict(nn_ms=a.value, nn_launches=b.value, nn_bytes=c.value, steer_ms=d.value, steer_launches=f.value)


class NodeTable(object):
    """
    An LQRRT_MODEL_GENERIC engine (include/lqrrt_hip.h): the node table of a tree whose plugins are host callables -- SoA states,
    cos/sin of the angular ones, parents, ignore set -- and the nearest-neighbour stage over it (planner.py:239-247, 340-350).
    No dynamics, lqr or feasibility is compiled in; gains and edges stay with the caller (lqrrt_amd/callback.py).

    angle_dims: the indices of the angular states, in ascending order, distinct and below nstates.  Anything else raises ValueError
    before an engine is created (the indices are not sorted or de-duplicated here).
    """

    def __init__(self, nstates, ncontrols, angle_dims=(), capacity=100008, device=0, max_wave=64):
        nat.require_device()
        self.n, self.m, self.device = int(nstates), int(ncontrols), device
        if not 1 <= self.n <= 64:
            raise ValueError("the device node table holds 1 to 64 states per node, got %d" % self.n)
        self.angle_dims = tuple(int(d) for d in angle_dims)
        # refused here, before an engine exists: the native table takes the indices as they come (ascending, distinct, < nstates)
        if any(not 0 <= d < self.n for d in self.angle_dims) or any(a >= b for a, b in zip(self.angle_dims, self.angle_dims[1:])):
            raise ValueError("angle_dims must be distinct state indices below %d in ascending order, got %r" % (self.n, self.angle_dims))
        d = nat.SystemDesc()
        d.model, d.nstates, d.ncontrols = nat.MODEL_GENERIC, self.n, self.m
        d.n_params = 1 + len(self.angle_dims)
        d.params[0] = float(len(self.angle_dims))
        for k, dim in enumerate(self.angle_dims):
            d.params[1 + k] = float(dim)
        h = C.c_void_p()
        nat.check(nat.lib().lqrrt_engine_create(C.byref(d), device, int(capacity), int(max_wave), C.byref(h)))
        self.h = h
        self.capacity, self.max_wave = int(capacity), int(max_wave)
        self._id, self._cost = C.c_int32(), C.c_double()
        self._lib = nat.lib()
        self._stream = nat.current_stream(device)

    def close(self):
        if getattr(self, "h", None):
            nat.lib().lqrrt_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def size(self):
        return nat.check(self._lib.lqrrt_tree_size(self.h))

    def reset(self, x0):
        """Tree(seed_state, ...) (tree.py:50): the table holds the seed only, the ignore set is empty."""
        x0 = nat.as_f64(x0, (self.n,))
        self._stream = nat.current_stream(self.device)
        nat.check(self._lib.lqrrt_tree_reset(self.h, nat.ptr(x0), self._stream))

    def load(self, states, pID, ignored=None):
        states = nat.as_f64(states)
        N = len(states)
        states = nat.as_f64(states, (N, self.n))
        pID = np.ascontiguousarray(pID, dtype=np.int32)
        ign = None if ignored is None else np.ascontiguousarray(ignored, dtype=np.uint8)
        self._stream = nat.current_stream(self.device)
        nat.check(self._lib.lqrrt_tree_load(self.h, N, nat.ptr(states), None, nat.ptr(pID), None, None, None,
                                            nat.ptr(ign) if ign is not None else None, self._stream))

    def append(self, parent, state):
        """Tree.add_node's device half (tree.py:77-96): asynchronous, ordered before the next query."""
        state = nat.as_f64(state, (self.n,))
        nat.check(self._lib.lqrrt_tree_append(self.h, int(parent), nat.ptr(state), None, 1, None, None, self._stream))

    def ignore(self, ids):
        """planner.py:270: the nodes of a finished path join the ignore set."""
        one = np.ones(1, dtype=np.uint8)
        for i in ids:
            nat.check(self._lib.lqrrt_tree_set_ignored(self.h, int(i), 1, nat.ptr(one)))

    def ignored(self):
        out = np.empty(self.size, dtype=np.uint8)
        nat.check(self._lib.lqrrt_tree_get_ignored(self.h, 0, len(out), nat.ptr(out)))
        return out.astype(bool)

    def truncate(self, size):
        nat.check(self._lib.lqrrt_tree_truncate(self.h, int(size)))

    def states(self):
        out = np.empty((self.size, self.n))
        nat.check(self._lib.lqrrt_tree_get_states(self.h, 0, len(out), nat.ptr(out)))
        return out

    def parents(self):
        out = np.empty(self.size, dtype=np.int32)
        nat.check(self._lib.lqrrt_tree_get_parents(self.h, 0, len(out), nat.ptr(out)))
        return out

    def nearest(self, x, S=None, use_ignore=True):
        """(id, cost) of the nearest eligible node to x under S (None = identity): one synchronous call, no copies."""
        x = nat.as_f64(x, (self.n,))
        Sp = None
        if S is not None:
            S = nat.as_f64(S, (self.n, self.n))
            Sp = nat.ptr(S)
        nat.check(self._lib.lqrrt_nn_argmin_host(self.h, nat.ptr(x), Sp, 1 if use_ignore else 0, C.byref(self._id), C.byref(self._cost),
                                                 self._stream))
        return self._id.value, self._cost.value

    def nearest_from_errors(self, errors, S=None, use_ignore=True):
        """The same selection for error rows erf(x, node i) the caller evaluated itself ([size][n])."""
        errors = nat.as_f64(errors, (self.size, self.n))
        Sp = None
        if S is not None:
            S = nat.as_f64(S, (self.n, self.n))
            Sp = nat.ptr(S)
        nat.check(self._lib.lqrrt_nn_argmin_errors(self.h, nat.ptr(errors), Sp, 1 if use_ignore else 0, C.byref(self._id),
                                                   C.byref(self._cost), self._stream))
        return self._id.value, self._cost.value

    def nn_argmin(self, xs, S=None, use_ignore=True):
        """Batched device form (lqrrt_nn_argmin): xs [W][n] -> ids [W], costs [W]."""
        torch = _torch()
        W = len(xs)
        dev = "cuda:%d" % self.device
        dxs = torch.from_numpy(nat.as_f64(xs, (W, self.n))).to(dev)
        dS = torch.from_numpy(nat.as_f64(S, (self.n, self.n))).to(dev) if S is not None else None
        ids = torch.empty(W, dtype=torch.int32, device=dev)
        cost = torch.empty(W, dtype=torch.float64, device=dev)
        nat.check(self._lib.lqrrt_nn_argmin(self.h, dxs.data_ptr(), W, dS.data_ptr() if dS is not None else None,
                                            1 if use_ignore else 0, ids.data_ptr(), cost.data_ptr(), nat.current_stream(self.device)))
        return ids.cpu().numpy(), cost.cpu().numpy()

    def costs_to_go(self, x, S=None):
        torch = _torch()
        dev = "cuda:%d" % self.device
        dx = torch.from_numpy(nat.as_f64(x, (self.n,))).to(dev)
        dS = torch.from_numpy(nat.as_f64(S, (self.n, self.n))).to(dev) if S is not None else None
        cost = torch.empty(self.size, dtype=torch.float64, device=dev)
        nat.check(self._lib.lqrrt_costs_to_go(self.h, dx.data_ptr(), dS.data_ptr() if dS is not None else None, cost.data_ptr(),
                                              nat.current_stream(self.device)))
        return cost.cpu().numpy()
