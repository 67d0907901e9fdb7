// ABI: clearance of the tree against moving discs -- lqrrt_tree_clear (Planner.avoid; kernels in clear.hpp, the rule restated in
// NumPy in tests/clear_reference.py) and lqrrt_tree_clear_wait, the same for `waits` departure delays at once (Planner.avoid with
// max_wait; clear_wait.hpp, tests/clear_wait_reference.py).  Both read the tree and write nothing of it.  One host path: the
// refusals (clear_check), then the launches (clear_run); what differs between the calls is in a traits struct each.
// Fragment of engine.hip, behind engine_retain.hpp (retain_links, double_rounds) and engine_refine.hpp (Carve, StreamDrain).
// --------------------------------------------------------------------------------------------

// Scratch of one call: everything is transient (freed before the call returns, not part of the footprint).
//   per node  16 + 16 (step links, two parities), then
//             lqrrt_tree_clear       8 + 8 (first links, two parities) + 3 * 4 (own, dwell, first) = 60 bytes
//             lqrrt_tree_clear_wait  16 + 16 (mask links, two parities) + 3 * 8 (own_ok, dwell_ok, clear) + 4 (hit) = 92 bytes
//   table     32 L D bytes: per instant and disc x, y, the exact threshold, the padded radius
struct ClearScratch {
    char* mem = nullptr;
    ~ClearScratch() {
        if (mem) (void)hipFree(mem);
    }
};

// the device arrays of a call, in the scratch's order
template <class C>
struct ClearBufs {
    RetainLink *a, *b;
    typename C::Link *ca, *cb;
    typename C::Node *own, *dwell, *ans;
    int* hit;                             // (lqrrt_tree_clear_wait only)
    double* table;
    typename C::Out* out;
};

// What lqrrt_tree_clear is made of: the link of its propagate rounds, its per-node answers, its counters, the launches of its
// check and its select, and its stats from the counters.
struct ClearPlain {
    typedef ClearLink Link;
    typedef int Node;
    typedef ClearOut Out;
    typedef lqrrt_clear_stats Stats;
    static constexpr const char* NAME = "lqrrt_tree_clear";
    static constexpr const char* WAIT_TERM = "";
    static constexpr size_t CHECK_LDS = 0, HIT_BYTES = 0;
    template <class S>
    static void check(const lqrrt_engine* e, const ClearBufs<ClearPlain>& d, int N, int L, int D, int start, int, size_t hull_bytes, hipStream_t st) {
        hipLaunchKernelGGL((k_clear_check<S>), dim3((unsigned)N), dim3(64), hull_bytes, st, e->P, e->geo, e->tv, e->res, N,
                           (const RetainLink*)d.a, (const double*)d.table, L, D, start, d.own, d.dwell);
    }
    static void select(const lqrrt_engine* e, const ClearBufs<ClearPlain>& d, int N, hipStream_t st) {
        hipLaunchKernelGGL(k_clear_select, dim3((unsigned)((N + CLEAR_BLOCK - 1) / CLEAR_BLOCK)), dim3(CLEAR_BLOCK), 0, st, e->tv, N,
                           (const int*)d.own, (const int*)d.dwell, (const ClearLink*)d.ca, (const RetainLink*)d.a, d.ans, d.out);
    }
    static void stats(const ClearOut& h, const std::vector<long long>&, int N, lqrrt_clear_stats* out) {
        out->size = N; out->conflicts = h.conflicts; out->blocked = h.blocked; out->hits = h.hits; out->clear_hits = h.clear_hits;
        if (h.best != ~0ull) { out->best_end = (int)(h.best & 0xffffffffull); out->best_steps = (int64_t)(h.best >> 32); }
        else { out->best_end = -1; out->best_steps = -1; }
    }
};

// ... and lqrrt_tree_clear_wait; the host takes best_wait from cum
struct ClearWait {
    typedef ClearWaitLink Link;
    typedef unsigned long long Node;
    typedef ClearWaitOut Out;
    typedef lqrrt_clear_wait_stats Stats;
    static constexpr const char* NAME = "lqrrt_tree_clear_wait";
    static constexpr const char* WAIT_TERM = " + the longest wait";
    static constexpr size_t CHECK_LDS = 64, HIT_BYTES = sizeof(int);
    template <class S>
    static void check(const lqrrt_engine* e, const ClearBufs<ClearWait>& d, int N, int L, int D, int start, int waits, size_t hull_bytes,
                      hipStream_t st) {
        hipLaunchKernelGGL((k_clear_wait_check<S>), dim3((unsigned)N), dim3(CLEAR_WAIT_BLOCK), hull_bytes, st, e->P, e->geo, e->tv, e->res,
                           N, (const RetainLink*)d.a, (const double*)d.table, L, D, start, waits, d.own, d.dwell, d.hit);
    }
    static void select(const lqrrt_engine* e, const ClearBufs<ClearWait>& d, int N, hipStream_t st) {
        hipLaunchKernelGGL(k_clear_wait_select, dim3((unsigned)((N + CLEAR_WAIT_BLOCK - 1) / CLEAR_WAIT_BLOCK)), dim3(CLEAR_WAIT_BLOCK), 0,
                           st, e->tv, N, (const unsigned long long*)d.dwell, (const int*)d.hit, (const ClearWaitLink*)d.ca,
                           (const RetainLink*)d.a, d.ans, d.out);
    }
    static void stats(const ClearWaitOut& h, const std::vector<long long>& cum, int N, lqrrt_clear_wait_stats* out) {
        out->size = N; out->hits = h.hits; out->clear_hits = h.clear_hits; out->clear_now = h.clear_now;
        if (h.best != ~0ull) {
            out->best_end = (int)(h.best & 0xffffffffull);
            out->best_arrival = (int64_t)(h.best >> 32);
            out->best_steps = (int64_t)cum[(size_t)out->best_end];
            out->best_wait = (int)(out->best_arrival - out->best_steps);
        } else { out->best_end = -1; out->best_wait = -1; out->best_steps = -1; out->best_arrival = -1; }
    }
};

// Every argument of a call, before anything is allocated or enqueued; `waits`: 1 for lqrrt_tree_clear.  Fills cum (one ascending
// pass over the host mirrors, as connect_depths) and the disc table [L][D][4], as upload_geometry derives a static circle.
template <class C>
static int clear_check(lqrrt_engine* e, const void* out, const double* tracks_host, const double* radii_host, int L, int D, int start,
                       int waits, std::vector<long long>& cum, std::vector<double>& table) {
    if (!e || !out || !tracks_host || !radii_host) return fail(LQRRT_E_ARG, "null argument");
    if (L < 1 || D < 1) return fail(LQRRT_E_ARG, "the track table needs L >= 1 instants and D >= 1 discs (L = %d, D = %d)", L, D);
    if (start < 0) return fail(LQRRT_E_ARG, "start must be >= 0 (%d)", start);
    if ((long long)L * D > 0x7fffffffLL / 4) return fail(LQRRT_E_ARG, "track table too large (L = %d, D = %d)", L, D);
    for (size_t q = 0; q < (size_t)L * D * 2; ++q)
        if (!std::isfinite(tracks_host[q])) return fail(LQRRT_E_ARG, "track position %zu of disc %zu is not finite", q / 2 / D, q / 2 % D);
    for (int d = 0; d < D; ++d)
        if (!(radii_host[d] >= 0.0)) return fail(LQRRT_E_ARG, "radius %d is not >= 0", d);
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
    std::vector<double> thr((size_t)D), pad((size_t)D);
    for (int d = 0; d < D; ++d) {
        const double r = model_novice(e->model) ? inflate + radii_host[d] : radii_host[d];
        thr[(size_t)d] = exact_sq_threshold(r);
        pad[(size_t)d] = (r >= 0.0) ? r * (1.0 + 1e-9) + 1e-9 : -1e300;
    }
    table.resize((size_t)L * D * 4);
    for (size_t q = 0; q < (size_t)L * D; ++q) {
        table[4 * q] = tracks_host[2 * q]; table[4 * q + 1] = tracks_host[2 * q + 1];
        table[4 * q + 2] = thr[q % D]; table[4 * q + 3] = pad[q % D];
    }
    return 0;
}

// The launches of a checked call: the step sums, the check, the propagate rounds, the select, and the call's one synchronise.
template <class C>
static int clear_run(lqrrt_engine* e, const std::vector<long long>& cum, const std::vector<double>& table, int L, int D, int start, int waits,
                     typename C::Stats* out, typename C::Node* ans_host, typename C::Node* dwell_host, hipStream_t st) {
    typedef typename C::Link Link;
    typedef typename C::Node Node;
    const int N = e->N;
    const size_t hull_bytes = sizeof(double) * (size_t)2 * e->geo.V;
    // ---- scratch, carved out of one allocation
    Carve carve{0, 256};
    const size_t o_a = carve(sizeof(RetainLink) * N), o_b = carve(sizeof(RetainLink) * N);
    const size_t o_ca = carve(sizeof(Link) * N), o_cb = carve(sizeof(Link) * N);
    const size_t o_own = carve(sizeof(Node) * N), o_dwell = carve(sizeof(Node) * N), o_ans = carve(sizeof(Node) * N);
    const size_t o_hit = carve(C::HIT_BYTES * N);
    const size_t o_table = carve(sizeof(double) * table.size()), o_out = carve(sizeof(typename C::Out));
    ClearScratch sc;
    TRY(dalloc_transient(&sc.mem, carve.off));                  // (transient: not part of the engine's footprint)
    ClearBufs<C> d = {(RetainLink*)(sc.mem + o_a), (RetainLink*)(sc.mem + o_b), (Link*)(sc.mem + o_ca), (Link*)(sc.mem + o_cb),
                      (Node*)(sc.mem + o_own), (Node*)(sc.mem + o_dwell), (Node*)(sc.mem + o_ans), (int*)(sc.mem + o_hit),
                      (double*)(sc.mem + o_table), (typename C::Out*)(sc.mem + o_out)};
    typename C::Out h{};
    h.best = ~0ull;
    StreamDrain drain(st);                                      // (the scratch is in use by the stream, h a source and a target of copies)
    drain.arm();
    HIPCHK(hipMemcpyAsync(d.out, &h, sizeof h, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d.table, table.data(), sizeof(double) * table.size(), hipMemcpyHostToDevice, st));
    // ---- steps: cum - elen[0] in RetainLink::steps (root 0, every edge passes)
    retain_links(e, 0, N, nullptr, d.a, d.b, st);
    HIPCHK(hipGetLastError());
    // ---- check
    DISPATCH(e, if constexpr (has_discs<S>::value) C::template check<S>(e, d, N, L, D, start, waits, hull_bytes, st));
    HIPCHK(hipGetLastError());
    // ---- propagate
    hipLaunchKernelGGL((k_clear_init<Link>), dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, e->tv, N, (const Node*)d.own, d.ca);
    double_rounds(k_clear_double<Link>, N, d.ca, d.cb, st);
    // ---- select
    C::select(e, d, N, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&h, d.out, sizeof h, hipMemcpyDeviceToHost, st));
    if (ans_host) HIPCHK(hipMemcpyAsync(ans_host, d.ans, sizeof(Node) * N, hipMemcpyDeviceToHost, st));
    if (dwell_host) HIPCHK(hipMemcpyAsync(dwell_host, d.dwell, sizeof(Node) * N, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    drain.disarm();
    C::stats(h, cum, N, out);
    return 0;
}

template <class C>
static int clear_call(lqrrt_engine* e, const double* tracks_host, const double* radii_host, int L, int D, int start, int waits,
                      typename C::Stats* out, typename C::Node* ans_host, typename C::Node* dwell_host, void* stream) {
    std::vector<long long> cum;
    std::vector<double> table;
    TRY(clear_check<C>(e, out, tracks_host, radii_host, L, D, start, waits, cum, table));
    TRY(use_device(e));
    return clear_run<C>(e, cum, table, L, D, start, waits, out, ans_host, dwell_host, (hipStream_t)stream);
}

extern "C" int lqrrt_tree_clear(lqrrt_engine* e, const double* tracks_host, const double* radii_host, int L, int D, int start,
                                lqrrt_clear_stats* out, int32_t* first_host, int32_t* dwell_host, void* stream) {
    NOT_GENERIC(e);
    return clear_call<ClearPlain>(e, tracks_host, radii_host, L, D, start, 1, out, first_host, dwell_host, stream);
}

extern "C" int lqrrt_tree_clear_wait(lqrrt_engine* e, const double* tracks_host, const double* radii_host, int L, int D, int start,
                                     int waits, lqrrt_clear_wait_stats* out, uint64_t* clear_host, uint64_t* dwell_host, void* stream) {
    NOT_GENERIC(e);
    return clear_call<ClearWait>(e, tracks_host, radii_host, L, D, start, waits, out, (unsigned long long*)clear_host,
                                 (unsigned long long*)dwell_host, stream);
}
