// ABI: clearance of the tree against moving oriented rectangles -- lqrrt_tree_clear_rects (Planner.avoid_rects; the check kernel in
// clear_rects.hpp, the rule restated in NumPy in tests/clear_rects_reference.py).  Reads the tree and writes nothing of it.
// The host path is engine_clear.hpp's: the refusals here (clear_rects_check: a rectangle's arguments, then the tree-side checks
// of clear_check restated in their order), then clear_run<ClearRects> -- the step sums, the propagate rounds, the select, the
// counters and the stats do not depend on the obstacle's shape.  Fragment of engine.hip, behind engine_clear.hpp.
// --------------------------------------------------------------------------------------------

// Scratch of one call (transient, not part of the footprint): lqrrt_tree_clear's 60 bytes per node, and the table:
//   32 L D bytes   per instant and rectangle x, y, cos, sin of the heading (lq_sincos, as the vehicle's own heading)
//   32 D bytes     per rectangle a', b' (the novice boats: grown by half the boat length), the padded half diagonal of the cull, 0

// What lqrrt_tree_clear_rects is made of: lqrrt_tree_clear's link, answers, counters, select and stats, and a check of its own.
struct ClearRects {
    typedef ClearLink Link;
    typedef int Node;
    typedef ClearOut Out;
    typedef lqrrt_clear_stats Stats;
    static constexpr const char* NAME = "lqrrt_tree_clear_rects";
    static constexpr const char* WAIT_TERM = "";
    static constexpr size_t CHECK_LDS = 0, HIT_BYTES = 0;
    template <class S>
    static void check(const lqrrt_engine* e, const ClearBufs<ClearRects>& d, int N, int L, int D, int start, int, size_t hull_bytes, hipStream_t st) {
        hipLaunchKernelGGL((k_clear_rects_check<S>), dim3((unsigned)N), dim3(64), hull_bytes, st, e->geo, e->tv, e->res, N,
                           (const RetainLink*)d.a, (const double*)d.table, L, D, start, d.own, d.dwell);
    }
    static void select(const lqrrt_engine* e, const ClearBufs<ClearRects>& d, int N, hipStream_t st) {
        const ClearBufs<ClearPlain> p = {d.a, d.b, d.ca, d.cb, d.own, d.dwell, d.ans, d.hit, d.table, d.out};
        ClearPlain::select(e, p, N, st);
    }
    static void stats(const ClearOut& h, const std::vector<long long>& cum, int N, lqrrt_clear_stats* out) { ClearPlain::stats(h, cum, N, out); }
};

// Every argument of the call, before anything is allocated or enqueued.  Fills cum (as clear_check) and the table.  `C`: the
// call's traits (engine_clear_rects_wait.hpp has the other one); `waits`: 1 for lqrrt_tree_clear_rects.
template <class C = ClearRects>
static int clear_rects_check(lqrrt_engine* e, const void* out, const double* tracks_host, const double* extents_host, int L, int D, int start,
                             std::vector<long long>& cum, std::vector<double>& table, int waits = 1) {
    if (!e || !out || !tracks_host || !extents_host) return fail(LQRRT_E_ARG, "null argument");
    if (L < 1 || D < 1) return fail(LQRRT_E_ARG, "the track table needs L >= 1 instants and D >= 1 rectangles (L = %d, D = %d)", L, D);
    if (start < 0) return fail(LQRRT_E_ARG, "start must be >= 0 (%d)", start);
    if ((long long)L * D > 0x7fffffffLL / 4) return fail(LQRRT_E_ARG, "track table too large (L = %d, D = %d)", L, D);
    for (size_t q = 0; q < (size_t)L * D * 3; ++q)
        if (!std::isfinite(tracks_host[q]))
            return fail(LQRRT_E_ARG, "track %s %zu of rectangle %zu is not finite", q % 3 == 2 ? "heading" : "position", q / 3 / D, q / 3 % D);
    for (int d = 0; d < 2 * D; ++d)
        if (!(extents_host[d] >= 0.0) || !std::isfinite(extents_host[d]))
            return fail(LQRRT_E_ARG, "half %s %d is not >= 0 and finite", d % 2 ? "width" : "length", d / 2);
    if (waits < 1 || waits > 64) return fail(LQRRT_E_ARG, "waits must be 1 .. 64 delays (%d): the answers are 64-bit masks", waits);
    bool discs = false;
    DISPATCH(e, discs = has_discs<S>::value);
    if (!discs) return fail(LQRRT_E_STATE, "%s: the feasibility test of model %d has no circle path", C::NAME, e->model);
    if (!e->has_res || e->N < 1) return fail(LQRRT_E_STATE, "no tree to check: set_resolution and tree_reset / tree_load first");
    if (!e->has_goal) return fail(LQRRT_E_STATE, "no goal: lqrrt_engine_set_resolution with has_goal first");
    // start + the longest wait + the deepest cum fits 31 bits
    const int N = e->N;
    cum.resize((size_t)N);
    if (e->h_elen[0] < 1) return fail(LQRRT_E_STATE, "the root's edge has no row");
    cum[0] = e->h_elen[0];
    long long deepest = cum[0];
    for (int v = 1; v < N; ++v) {
        const int p = e->h_pid[(size_t)v];
        if (p < 0 || p >= v) return fail(LQRRT_E_STATE, "node %d has parent %d: the step sums need pID[v] < v", v, p);
        if (e->h_elen[(size_t)v] < 1) return fail(LQRRT_E_STATE, "node %d has an edge without rows", v);
        cum[(size_t)v] = cum[(size_t)p] + e->h_elen[(size_t)v];
        deepest = std::max(deepest, cum[(size_t)v]);
    }
    if ((long long)start + (waits - 1) + deepest > 0x7fffffffLL)
        return fail(LQRRT_E_ARG, "start%s + the deepest node's steps leave 31 bits", C::WAIT_TERM);
    const size_t hull_bytes = sizeof(double) * (size_t)2 * e->geo.V;
    if (e->lds_limit && hull_bytes + C::CHECK_LDS > e->lds_limit)
        return fail(LQRRT_E_ARG, "the clearance check stages the hull points in LDS: 16 V = %zu bytes (V = %d), the device's limit is %zu",
                    hull_bytes, e->geo.V, e->lds_limit);
    const double inflate = model_novice(e->model) ? e->P.p[18] : 0.0;
    const size_t poses = (size_t)L * D;
    table.resize(4 * poses + 4 * (size_t)D);
    // (lq_sincos costs ~20 ns a pose on the host, 0.8 ms for L D = 37 800: more than the kernels of the call.  A rectangle that
    //  stands, runs straight or has arrived keeps its heading from one instant to the next, and then its cos / sin.)
    for (size_t q = 0; q < poses; ++q) {
        double so, co;
        const double h = tracks_host[3 * q + 2];
        if (q >= (size_t)D && h == tracks_host[3 * (q - D) + 2] && std::signbit(h) == std::signbit(tracks_host[3 * (q - D) + 2])) {
            co = table[4 * (q - D) + 2]; so = table[4 * (q - D) + 3];
        } else lq_sincos(h, &so, &co);
        table[4 * q] = tracks_host[3 * q]; table[4 * q + 1] = tracks_host[3 * q + 1];
        table[4 * q + 2] = co; table[4 * q + 3] = so;
    }
    for (int d = 0; d < D; ++d) {
        const double a = model_novice(e->model) ? extents_host[2 * d] + inflate : extents_host[2 * d];
        const double b = model_novice(e->model) ? extents_host[2 * d + 1] + inflate : extents_host[2 * d + 1];
        double* x = &table[4 * poses + 4 * (size_t)d];
        x[0] = a; x[1] = b;
        x[2] = std::sqrt(a * a + b * b) * (1.0 + 1e-9) + 1e-9;       // (padded half diagonal: the cull's reach)
        x[3] = 0.0;
    }
    return 0;
}

extern "C" int lqrrt_tree_clear_rects(lqrrt_engine* e, const double* tracks_host, const double* extents_host, int L, int D, int start,
                                      lqrrt_clear_stats* out, int32_t* first_host, int32_t* dwell_host, void* stream) {
    NOT_GENERIC(e);
    std::vector<long long> cum;
    std::vector<double> table;
    TRY(clear_rects_check(e, out, tracks_host, extents_host, L, D, start, cum, table));
    TRY(use_device(e));
    return clear_run<ClearRects>(e, cum, table, L, D, start, 1, out, first_host, dwell_host, (hipStream_t)stream);
}
