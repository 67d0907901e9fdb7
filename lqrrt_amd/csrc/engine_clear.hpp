// ABI: clearance of the tree against moving discs -- lqrrt_tree_clear (Planner.avoid; kernels in clear.hpp, the rule restated in
// NumPy in tests/clear_reference.py).  Reads the tree, writes nothing of it.  Fragment of engine.hip.
// --------------------------------------------------------------------------------------------

// Scratch of one call: everything is transient (freed before lqrrt_tree_clear returns, not part of the footprint).
//   per node  16 + 16 (step links, two parities) + 8 + 8 (first links, two parities) + 3 * 4 (own, dwell, first) = 60 bytes
//   table     32 L D bytes: per instant and disc x, y, the exact threshold, the padded radius
struct ClearScratch {
    char* mem = nullptr;
    ~ClearScratch() {
        if (mem) (void)hipFree(mem);
    }
};

extern "C" int lqrrt_tree_clear(lqrrt_engine* e, const double* tracks_host, const double* radii_host, int L, int D, int start,
                                lqrrt_clear_stats* out, int32_t* first_host, int32_t* dwell_host, void* stream) {
    NOT_GENERIC(e);
    if (!e || !out || !tracks_host || !radii_host) return fail(LQRRT_E_ARG, "null argument");
    // ---- every argument, before anything is enqueued
    if (L < 1 || D < 1) return fail(LQRRT_E_ARG, "the track table needs L >= 1 instants and D >= 1 discs (L = %d, D = %d)", L, D);
    if (start < 0) return fail(LQRRT_E_ARG, "start must be >= 0 (%d)", start);
    if ((long long)L * D > 0x7fffffffLL / 4) return fail(LQRRT_E_ARG, "track table too large (L = %d, D = %d)", L, D);
    for (size_t q = 0; q < (size_t)L * D * 2; ++q)
        if (!std::isfinite(tracks_host[q])) return fail(LQRRT_E_ARG, "track position %zu of disc %zu is not finite", q / 2 / D, q / 2 % D);
    for (int d = 0; d < D; ++d)
        if (!(radii_host[d] >= 0.0)) return fail(LQRRT_E_ARG, "radius %d is not >= 0", d);
    bool discs = false;
    DISPATCH(e, discs = has_discs<S>::value);
    if (!discs) return fail(LQRRT_E_STATE, "lqrrt_tree_clear: the feasibility test of model %d has no circle path", e->model);
    if (!e->has_res || e->N < 1) return fail(LQRRT_E_STATE, "no tree to check: set_resolution and tree_reset / tree_load first");
    if (!e->has_goal) return fail(LQRRT_E_STATE, "no goal: lqrrt_engine_set_resolution with has_goal first");
    const int N = e->N;
    {   // start + the deepest cum fits 31 bits (one ascending pass over the host mirrors, as connect_depths)
        std::vector<long long> cum((size_t)N);
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
        if ((long long)start + deepest > 0x7fffffffLL) return fail(LQRRT_E_ARG, "start + the deepest node's steps leave 31 bits");
    }
    const size_t hull_bytes = sizeof(double) * (size_t)2 * e->geo.V;
    if (e->lds_limit && hull_bytes > e->lds_limit)
        return fail(LQRRT_E_ARG, "the clearance check stages the hull points in LDS: 16 V = %zu bytes (V = %d), the device's limit is %zu",
                    hull_bytes, e->geo.V, e->lds_limit);
    TRY(use_device(e));
    hipStream_t st = (hipStream_t)stream;

    // ---- the disc table, as upload_geometry derives a static circle
    const double inflate = model_novice(e->model) ? e->P.p[18] : 0.0;
    std::vector<double> thr((size_t)D), pad((size_t)D);
    for (int d = 0; d < D; ++d) {
        const double r = model_novice(e->model) ? inflate + radii_host[d] : radii_host[d];
        thr[(size_t)d] = exact_sq_threshold(r);
        pad[(size_t)d] = (r >= 0.0) ? r * (1.0 + 1e-9) + 1e-9 : -1e300;
    }
    std::vector<double> table((size_t)L * D * 4);
    for (size_t q = 0; q < (size_t)L * D; ++q) {
        table[4 * q] = tracks_host[2 * q]; table[4 * q + 1] = tracks_host[2 * q + 1];
        table[4 * q + 2] = thr[q % D]; table[4 * q + 3] = pad[q % D];
    }

    // ---- scratch, carved out of one allocation
    size_t off = 0;
    auto carve = [&](size_t bytes) { const size_t at = off; off += (bytes + 255) / 256 * 256; return at; };
    const size_t o_a = carve(sizeof(RetainLink) * N), o_b = carve(sizeof(RetainLink) * N);
    const size_t o_ca = carve(sizeof(ClearLink) * N), o_cb = carve(sizeof(ClearLink) * N);
    const size_t o_own = carve(sizeof(int) * N), o_dwell = carve(sizeof(int) * N), o_first = carve(sizeof(int) * N);
    const size_t o_table = carve(sizeof(double) * table.size()), o_out = carve(sizeof(ClearOut));
    ClearScratch sc;
    const size_t keep_bytes = g_dalloc_bytes;
    const int rc = dalloc(&sc.mem, off);
    g_dalloc_bytes = keep_bytes;                                // (transient: not part of the engine's footprint)
    if (rc) return rc;
    RetainLink* d_a = (RetainLink*)(sc.mem + o_a);
    RetainLink* d_b = (RetainLink*)(sc.mem + o_b);
    ClearLink* d_ca = (ClearLink*)(sc.mem + o_ca);
    ClearLink* d_cb = (ClearLink*)(sc.mem + o_cb);
    int* d_own = (int*)(sc.mem + o_own);
    int* d_dwell = (int*)(sc.mem + o_dwell);
    int* d_first = (int*)(sc.mem + o_first);
    double* d_table = (double*)(sc.mem + o_table);
    ClearOut* d_out = (ClearOut*)(sc.mem + o_out);

    // From here on the scratch is in use by the stream: wait for it before the scratch goes, whatever happens.
    auto run = [&]() -> int {
        ClearOut h{};
        h.best = ~0ull;
        HIPCHK(hipMemcpyAsync(d_out, &h, sizeof h, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_table, table.data(), sizeof(double) * table.size(), hipMemcpyHostToDevice, st));
        const dim3 per_node((unsigned)((N + 255) / 256)), t256(256);
        int rounds = 0;
        while ((1ll << rounds) < (long long)N) ++rounds;
        // ---- steps: cum - elen[0] in RetainLink::steps (root 0, every edge passes)
        hipLaunchKernelGGL(k_retain_init, per_node, t256, 0, st, e->tv, 0, N, (const unsigned char*)nullptr, d_a);
        for (int r = 0; r < rounds; ++r) {
            hipLaunchKernelGGL(k_retain_double, per_node, t256, 0, st, N, (const RetainLink*)d_a, d_b);
            std::swap(d_a, d_b);
        }
        HIPCHK(hipGetLastError());
        // ---- check
        DISPATCH(e, if constexpr (has_discs<S>::value)
                        hipLaunchKernelGGL((k_clear_check<S>), dim3((unsigned)N), dim3(64), hull_bytes, st, e->P, e->geo, e->tv, e->res, N,
                                           (const RetainLink*)d_a, (const double*)d_table, L, D, start, d_own, d_dwell));
        HIPCHK(hipGetLastError());
        // ---- propagate: 2^rounds >= N covers every parent chain
        hipLaunchKernelGGL(k_clear_init, per_node, t256, 0, st, e->tv, N, (const int*)d_own, d_ca);
        for (int r = 0; r < rounds; ++r) {
            hipLaunchKernelGGL(k_clear_double, per_node, t256, 0, st, N, (const ClearLink*)d_ca, d_cb);
            std::swap(d_ca, d_cb);
        }
        // ---- select
        hipLaunchKernelGGL(k_clear_select, dim3((unsigned)((N + CLEAR_BLOCK - 1) / CLEAR_BLOCK)), dim3(CLEAR_BLOCK), 0, st, e->tv, N,
                           (const int*)d_own, (const int*)d_dwell, (const ClearLink*)d_ca, (const RetainLink*)d_a, d_first, d_out);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&h, d_out, sizeof h, hipMemcpyDeviceToHost, st));
        if (first_host) HIPCHK(hipMemcpyAsync(first_host, d_first, sizeof(int) * N, hipMemcpyDeviceToHost, st));
        if (dwell_host) HIPCHK(hipMemcpyAsync(dwell_host, d_dwell, sizeof(int) * N, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        out->size = N; out->conflicts = h.conflicts; out->blocked = h.blocked; out->hits = h.hits; out->clear_hits = h.clear_hits;
        if (h.best != ~0ull) { out->best_end = (int)(h.best & 0xffffffffull); out->best_steps = (int64_t)(h.best >> 32); }
        else { out->best_end = -1; out->best_steps = -1; }
        return 0;
    };
    const int rrc = run();
    if (rrc) {
        const std::string keep = g_err;
        (void)hipStreamSynchronize(st);                         // nothing in flight when the scratch goes
        g_err = keep;
    }
    return rrc;
}
