// ABI: the rectangle clearance calls for several trees -- lqrrt_tree_clear_rects_multi and lqrrt_tree_clear_rects_wait_multi
// (lqrrt_amd.avoids_rects; the check kernels in clear_rects_multi.hpp).  Member k answers exactly as lqrrt_tree_clear_rects /
// lqrrt_tree_clear_rects_wait on engines[k] with its own tracks, extents, L, D, start (and waits); nothing of any tree is written.
// The host path is engine_clear_multi.hpp's, unchanged: clear_multi_run<M> takes the members' finished step sums and tables and a
// traits struct, and its steps, propagate rounds, select, image, chunks and read-back do not know what the obstacle is.  This
// file adds the two traits (engine_clear_rects.hpp's and engine_clear_rects_wait.hpp's, extended by the two launches that span
// several engines) and the per-member argument check.  Fragment of engine.hip, behind engine_clear_multi.hpp (clear_multi_run,
// ClearMember), engine_clear_rects.hpp and engine_clear_rects_wait.hpp (clear_rects_check, ClearRects, ClearRectsWait).
//
// Every argument of every member is checked -- the engine list by multi_engines_check, the member's own arguments by the solo
// calls' clear_rects_check, in list order -- before anything is allocated or enqueued; a refusal keeps the solo call's code and
// message and names the engine.  The table of a member is the solo call's: 32 L D bytes of poses (x, y, cos, sin of the heading)
// and the 32 D bytes of extents behind them; members that pass the same tracks and extents arrays with equal L, D (and, the novice
// boats, equal inflation, which is part of the extents tail) share one table.  Per chunk of up to MULTI_MAX members the run makes
// one transient allocation and every stage ONE launch; the chunks are enqueued one after another and waited for once.  Nothing of
// this is part of any engine's footprint.
// --------------------------------------------------------------------------------------------

struct ClearRectsMulti : ClearRects {
    typedef ClearRects Solo;
    typedef ClearDesc<ClearLink> Desc;
    static constexpr const char* NAME_MULTI = "lqrrt_tree_clear_rects_multi";
    static constexpr long long CHECK_GROUPS = 1;                // 64-thread groups of the check per node (multi_chunks counts in those)
    template <class S>
    static void check_multi(unsigned grid, size_t hull_bytes, hipStream_t st, const ProtoTable& pt, const Desc* ds, const RetainGrid& gr) {
        hipLaunchKernelGGL((k_clear_rects_check_multi<S>), dim3(grid), dim3(64), hull_bytes, st, pt, ds, gr);
    }
    static void select_multi(unsigned grid, hipStream_t st, const ProtoTable& pt, const Desc* ds, const RetainGrid& gr) {
        hipLaunchKernelGGL(k_clear_select_multi, dim3(grid), dim3(CLEAR_BLOCK), 0, st, pt, ds, gr);
    }
};

struct ClearRectsWaitMulti : ClearRectsWait {
    typedef ClearRectsWait Solo;
    typedef ClearDesc<ClearWaitLink> Desc;
    static constexpr const char* NAME_MULTI = "lqrrt_tree_clear_rects_wait_multi";
    static constexpr long long CHECK_GROUPS = CLEAR_WAIT_WAVES;  // (so a chunk of the wait call holds fewer than 2^24 nodes)
    template <class S>
    static void check_multi(unsigned grid, size_t hull_bytes, hipStream_t st, const ProtoTable& pt, const Desc* ds, const RetainGrid& gr) {
        hipLaunchKernelGGL((k_clear_rects_wait_check_multi<S>), dim3(grid), dim3(CLEAR_WAIT_BLOCK), hull_bytes, st, pt, ds, gr);
    }
    static void select_multi(unsigned grid, hipStream_t st, const ProtoTable& pt, const Desc* ds, const RetainGrid& gr) {
        hipLaunchKernelGGL(k_clear_wait_select_multi, dim3(grid), dim3(CLEAR_WAIT_BLOCK), 0, st, pt, ds, gr);
    }
};

// Every argument of every member, before anything is allocated or enqueued.  waits == nullptr: lqrrt_tree_clear_rects_multi.
template <class M>
static int clear_rects_multi_check(lqrrt_engine** engines, int n, const double* const* tracks, const double* const* extents, const int32_t* L,
                                   const int32_t* D, const int32_t* start, const int32_t* waits, const typename M::Stats* out,
                                   std::vector<ClearMember>& mem) {
    mem.resize(n > 0 ? (size_t)n : 0);
    return multi_engines_check(engines, n, tracks && extents && L && D && start && out && (waits || !M::HIT_BYTES), [&](int k) {
        ClearMember& me = mem[(size_t)k];
        const int rc = clear_rects_check<typename M::Solo>(engines[k], out + k, tracks[k], extents[k], L[k], D[k], start[k], me.cum, me.table,
                                                           waits ? waits[k] : 1);
        if (rc) { g_err += engine_suffix(k); return rc; }
        // the shared-traffic case: the same arrays, read the same way, make the same table (the extents tail included) -- keep one
        const bool novice = model_novice(engines[k]->model);
        for (int q = 0; q < k && me.shares < 0; ++q)
            if (mem[(size_t)q].shares < 0 && tracks[q] == tracks[k] && extents[q] == extents[k] && L[q] == L[k] && D[q] == D[k] &&
                (!novice || engines[q]->P.p[18] == engines[k]->P.p[18]))
                me.shares = q;
        if (me.shares >= 0) std::vector<double>().swap(me.table);
        return 0;
    });
}

template <class M>
static int clear_rects_multi_call(lqrrt_engine** engines, int n, const double* const* tracks, const double* const* extents, const int32_t* L,
                                  const int32_t* D, const int32_t* start, const int32_t* waits, typename M::Stats* out,
                                  typename M::Node* const* ans_host, typename M::Node* const* dwell_host, void* stream) {
    std::vector<ClearMember> mem;
    TRY(clear_rects_multi_check<M>(engines, n, tracks, extents, L, D, start, waits, out, mem));
    TRY(use_device(engines[0]));
    return clear_multi_run<M>(engines, n, mem, L, D, start, waits, out, ans_host, dwell_host, (hipStream_t)stream);
}

extern "C" int lqrrt_tree_clear_rects_multi(lqrrt_engine** engines, int n, const double* const* tracks_host,
                                            const double* const* extents_host, const int32_t* L, const int32_t* D, const int32_t* start,
                                            lqrrt_clear_stats* out, int32_t* const* first_host, int32_t* const* dwell_host, void* stream) {
    return clear_rects_multi_call<ClearRectsMulti>(engines, n, tracks_host, extents_host, L, D, start, nullptr, out, first_host, dwell_host,
                                                   stream);
}

extern "C" int lqrrt_tree_clear_rects_wait_multi(lqrrt_engine** engines, int n, const double* const* tracks_host,
                                                 const double* const* extents_host, const int32_t* L, const int32_t* D, const int32_t* start,
                                                 const int32_t* waits, lqrrt_clear_wait_stats* out, uint64_t* const* clear_host,
                                                 uint64_t* const* dwell_host, void* stream) {
    return clear_rects_multi_call<ClearRectsWaitMulti>(engines, n, tracks_host, extents_host, L, D, start, waits, out,
                                                       (unsigned long long* const*)clear_host, (unsigned long long* const*)dwell_host, stream);
}
