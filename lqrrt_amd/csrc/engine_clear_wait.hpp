// ABI: clearance of the tree against moving discs for `waits` departure delays at once -- lqrrt_tree_clear_wait (Planner.avoid with
// max_wait; kernels in clear_wait.hpp, the rule restated in NumPy in tests/clear_wait_reference.py).  Reads the tree, writes nothing
// of it.  Fragment of engine.hip.
// --------------------------------------------------------------------------------------------

// Scratch of one call: everything is transient (freed before lqrrt_tree_clear_wait returns, not part of the footprint).
//   per node  16 + 16 (step links, two parities) + 16 + 16 (mask links, two parities) + 3 * 8 (own_ok, dwell_ok, clear) + 4 (hit)
//             = 92 bytes
//   table     32 L D bytes: per instant and disc x, y, the exact threshold, the padded radius
// (ClearScratch of engine_clear.hpp owns the allocation.)

// The disc table [L][D][4] as upload_geometry derives a static circle: lqrrt_tree_clear builds the same rows.
static std::vector<double> clear_wait_disc_table(const lqrrt_engine* e, const double* tracks_host, const double* radii_host, int L, int D) {
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
    return table;
}

extern "C" int lqrrt_tree_clear_wait(lqrrt_engine* e, const double* tracks_host, const double* radii_host, int L, int D, int start,
                                     int waits, lqrrt_clear_wait_stats* out, uint64_t* clear_host, uint64_t* dwell_host, void* stream) {
    NOT_GENERIC(e);
    if (!e || !out || !tracks_host || !radii_host) return fail(LQRRT_E_ARG, "null argument");
    // ---- every argument, before anything is enqueued (lqrrt_tree_clear's refusals in its order, then the two of the delays)
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
    if (!discs) return fail(LQRRT_E_STATE, "lqrrt_tree_clear_wait: the feasibility test of model %d has no circle path", e->model);
    if (!e->has_res || e->N < 1) return fail(LQRRT_E_STATE, "no tree to check: set_resolution and tree_reset / tree_load first");
    if (!e->has_goal) return fail(LQRRT_E_STATE, "no goal: lqrrt_engine_set_resolution with has_goal first");
    const int N = e->N;
    std::vector<long long> cum((size_t)N);                      // (kept: the host takes best_wait from it)
    {   // start + the longest wait + the deepest cum fits 31 bits (one ascending pass over the host mirrors, as lqrrt_tree_clear)
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
            return fail(LQRRT_E_ARG, "start + the longest wait + the deepest node's steps leave 31 bits");
    }
    const size_t hull_bytes = sizeof(double) * (size_t)2 * e->geo.V;
    if (e->lds_limit && hull_bytes + 64 > e->lds_limit)
        return fail(LQRRT_E_ARG, "the clearance check stages the hull points in LDS: 16 V = %zu bytes (V = %d), the device's limit is %zu",
                    hull_bytes, e->geo.V, e->lds_limit);
    TRY(use_device(e));
    hipStream_t st = (hipStream_t)stream;

    const std::vector<double> table = clear_wait_disc_table(e, tracks_host, radii_host, L, D);

    // ---- scratch, carved out of one allocation
    size_t off = 0;
    auto carve = [&](size_t bytes) { const size_t at = off; off += (bytes + 255) / 256 * 256; return at; };
    const size_t o_a = carve(sizeof(RetainLink) * N), o_b = carve(sizeof(RetainLink) * N);
    const size_t o_ca = carve(sizeof(ClearWaitLink) * N), o_cb = carve(sizeof(ClearWaitLink) * N);
    const size_t o_own = carve(sizeof(uint64_t) * N), o_dwell = carve(sizeof(uint64_t) * N), o_clear = carve(sizeof(uint64_t) * N);
    const size_t o_hit = carve(sizeof(int) * N);
    const size_t o_table = carve(sizeof(double) * table.size()), o_out = carve(sizeof(ClearWaitOut));
    ClearScratch sc;
    const size_t keep_bytes = g_dalloc_bytes;
    const int rc = dalloc(&sc.mem, off);
    g_dalloc_bytes = keep_bytes;                                // (transient: not part of the engine's footprint)
    if (rc) return rc;
    RetainLink* d_a = (RetainLink*)(sc.mem + o_a);
    RetainLink* d_b = (RetainLink*)(sc.mem + o_b);
    ClearWaitLink* d_ca = (ClearWaitLink*)(sc.mem + o_ca);
    ClearWaitLink* d_cb = (ClearWaitLink*)(sc.mem + o_cb);
    unsigned long long* d_own = (unsigned long long*)(sc.mem + o_own);
    unsigned long long* d_dwell = (unsigned long long*)(sc.mem + o_dwell);
    unsigned long long* d_clear = (unsigned long long*)(sc.mem + o_clear);
    int* d_hit = (int*)(sc.mem + o_hit);
    double* d_table = (double*)(sc.mem + o_table);
    ClearWaitOut* d_out = (ClearWaitOut*)(sc.mem + o_out);

    // From here on the scratch is in use by the stream: wait for it before the scratch goes, whatever happens.
    auto run = [&]() -> int {
        ClearWaitOut h{};
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
                        hipLaunchKernelGGL((k_clear_wait_check<S>), dim3((unsigned)N), dim3(CLEAR_WAIT_BLOCK), hull_bytes, st, e->P, e->geo,
                                           e->tv, e->res, N, (const RetainLink*)d_a, (const double*)d_table, L, D, start, waits, d_own,
                                           d_dwell, d_hit));
        HIPCHK(hipGetLastError());
        // ---- propagate: 2^rounds >= N covers every parent chain
        hipLaunchKernelGGL(k_clear_wait_init, per_node, t256, 0, st, e->tv, N, (const unsigned long long*)d_own, d_ca);
        for (int r = 0; r < rounds; ++r) {
            hipLaunchKernelGGL(k_clear_wait_double, per_node, t256, 0, st, N, (const ClearWaitLink*)d_ca, d_cb);
            std::swap(d_ca, d_cb);
        }
        // ---- select
        hipLaunchKernelGGL(k_clear_wait_select, dim3((unsigned)((N + CLEAR_WAIT_BLOCK - 1) / CLEAR_WAIT_BLOCK)), dim3(CLEAR_WAIT_BLOCK), 0,
                           st, e->tv, N, (const unsigned long long*)d_dwell, (const int*)d_hit, (const ClearWaitLink*)d_ca,
                           (const RetainLink*)d_a, d_clear, d_out);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&h, d_out, sizeof h, hipMemcpyDeviceToHost, st));
        if (clear_host) HIPCHK(hipMemcpyAsync(clear_host, d_clear, sizeof(uint64_t) * N, hipMemcpyDeviceToHost, st));
        if (dwell_host) HIPCHK(hipMemcpyAsync(dwell_host, d_dwell, sizeof(uint64_t) * N, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        out->size = N; out->hits = h.hits; out->clear_hits = h.clear_hits; out->clear_now = h.clear_now;
        if (h.best != ~0ull) {
            out->best_end = (int)(h.best & 0xffffffffull);
            out->best_arrival = (int64_t)(h.best >> 32);
            out->best_steps = (int64_t)cum[(size_t)out->best_end];
            out->best_wait = (int)(out->best_arrival - out->best_steps);
        } else { out->best_end = -1; out->best_wait = -1; out->best_steps = -1; out->best_arrival = -1; }
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
