// ABI: clearance of the tree against moving oriented rectangles for `waits` departure delays at once --
// lqrrt_tree_clear_rects_wait (Planner.avoid_rects with max_wait; the check kernel in clear_rects_wait.hpp, the rule restated in
// NumPy in tests/clear_rects_wait_reference.py).  Reads the tree and writes nothing of it.  The host path is engine_clear.hpp's:
// engine_clear_rects.hpp's refusals with the delays' three (clear_rects_check<ClearRectsWait>), then clear_run<ClearRectsWait> --
// the step sums, the propagate rounds on mask links, the select, the counters and the stats are lqrrt_tree_clear_wait's.
// Fragment of engine.hip, behind engine_clear_rects.hpp.
// --------------------------------------------------------------------------------------------

// Scratch of one call (transient, not part of the footprint): lqrrt_tree_clear_wait's 92 bytes per node, and
// lqrrt_tree_clear_rects's table, 32 L D + 32 D bytes.

// What lqrrt_tree_clear_rects_wait is made of: lqrrt_tree_clear_wait's link, answers, counters, select and stats, and a check of
// its own.
struct ClearRectsWait {
    typedef ClearWaitLink Link;
    typedef unsigned long long Node;
    typedef ClearWaitOut Out;
    typedef lqrrt_clear_wait_stats Stats;
    static constexpr const char* NAME = "lqrrt_tree_clear_rects_wait";
    static constexpr const char* WAIT_TERM = ClearWait::WAIT_TERM;
    static constexpr size_t CHECK_LDS = 64, HIT_BYTES = sizeof(int);
    template <class S>
    static void check(const lqrrt_engine* e, const ClearBufs<ClearRectsWait>& d, int N, int L, int D, int start, int waits, size_t hull_bytes,
                      hipStream_t st) {
        hipLaunchKernelGGL((k_clear_rects_wait_check<S>), dim3((unsigned)N), dim3(CLEAR_WAIT_BLOCK), hull_bytes, st, e->geo, e->tv, e->res, N,
                           (const RetainLink*)d.a, (const double*)d.table, L, D, start, waits, d.own, d.dwell, d.hit);
    }
    static void select(const lqrrt_engine* e, const ClearBufs<ClearRectsWait>& d, int N, hipStream_t st) {
        const ClearBufs<ClearWait> p = {d.a, d.b, d.ca, d.cb, d.own, d.dwell, d.ans, d.hit, d.table, d.out};
        ClearWait::select(e, p, N, st);
    }
    static void stats(const ClearWaitOut& h, const std::vector<long long>& cum, int N, lqrrt_clear_wait_stats* out) {
        ClearWait::stats(h, cum, N, out);
    }
};

extern "C" int lqrrt_tree_clear_rects_wait(lqrrt_engine* e, const double* tracks_host, const double* extents_host, int L, int D, int start,
                                           int waits, lqrrt_clear_wait_stats* out, uint64_t* clear_host, uint64_t* dwell_host, void* stream) {
    NOT_GENERIC(e);
    std::vector<long long> cum;
    std::vector<double> table;
    TRY(clear_rects_check<ClearRectsWait>(e, out, tracks_host, extents_host, L, D, start, cum, table, waits));
    TRY(use_device(e));
    return clear_run<ClearRectsWait>(e, cum, table, L, D, start, waits, out, (unsigned long long*)clear_host, (unsigned long long*)dwell_host,
                                     (hipStream_t)stream);
}
