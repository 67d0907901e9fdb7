// ABI: tree retention -- re-root, re-validate and compact the device-resident tree in place (Planner.replan; kernels in
// retain.hpp, the rule restated in NumPy in tests/retain_reference.py).  Fragment of engine.hip.
// --------------------------------------------------------------------------------------------

// Scratch of one retain: everything is transient (freed before lqrrt_tree_retain returns, not part of the footprint).
//   small  per old node 16 + 16 (links, two parities) + 1 + 1 (ok, keep) + 5 * 4 (local scan, new id, new parent, new edge
//          length, steps) bytes, + the block sums, a bitmap of the new ignore set and the counters: ~54 bytes per node
//   big    the kept nodes' rows of ONE pool at a time: kept * 8 * max(H n, H m, m n) bytes (the x-edge pool is the largest)
struct RetainScratch {
    char* small = nullptr;
    double* big = nullptr;
    ~RetainScratch() {
        if (small) (void)hipFree(small);
        if (big) (void)hipFree(big);
    }
};

static int retain_run(lqrrt_engine* e, int root, int revalidate, lqrrt_retain_stats* out, int32_t* old_to_new, hipStream_t st,
                      RetainScratch& sc) {
    const int N = e->N, n = e->n, m = e->m, H = e->H;
    const int nblocks = (N + RETAIN_BLOCK - 1) / RETAIN_BLOCK;
    const size_t words = (size_t)e->cap / 64 + 1;
    // ---- small scratch, carved out of one allocation
    size_t off = 0;
    auto carve = [&](size_t bytes) { const size_t at = off; off += (bytes + 255) / 256 * 256; return at; };
    const size_t o_a = carve(sizeof(RetainLink) * N), o_b = carve(sizeof(RetainLink) * N), o_ok = carve(N), o_keep = carve(N);
    const size_t o_local = carve(sizeof(int) * N), o_sums = carve(sizeof(int) * nblocks), o_newid = carve(sizeof(int) * N);
    const size_t o_nelen = carve(sizeof(int) * N), o_npid = carve(sizeof(int) * N), o_nsteps = carve(sizeof(int) * N);
    const size_t o_ign = carve(sizeof(unsigned long long) * words), o_out = carve(sizeof(RetainOut));
    const size_t keep_bytes = g_dalloc_bytes;
    int rc = dalloc(&sc.small, off);
    g_dalloc_bytes = keep_bytes;                                // (transient: not part of the engine's footprint)
    if (rc) return rc;
    RetainLink* d_a = (RetainLink*)(sc.small + o_a);
    RetainLink* d_b = (RetainLink*)(sc.small + o_b);
    unsigned char* d_ok = (unsigned char*)(sc.small + o_ok);
    unsigned char* d_keep = (unsigned char*)(sc.small + o_keep);
    int* d_local = (int*)(sc.small + o_local);
    int* d_sums = (int*)(sc.small + o_sums);
    int* d_newid = (int*)(sc.small + o_newid);
    int* d_nelen = (int*)(sc.small + o_nelen);
    int* d_npid = (int*)(sc.small + o_npid);
    int* d_nsteps = (int*)(sc.small + o_nsteps);
    unsigned long long* d_ign = (unsigned long long*)(sc.small + o_ign);
    RetainOut* d_out = (RetainOut*)(sc.small + o_out);

    RetainOut h{};
    h.best = ~0ull;
    h.root_feasible = 1;
    HIPCHK(hipMemcpyAsync(d_out, &h, sizeof h, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_ign, 0, sizeof(unsigned long long) * words, st));
    const dim3 per_node((unsigned)((N + 255) / 256)), t256(256);

    // ---- check
    if (revalidate) {
        DISPATCH(e, hipLaunchKernelGGL((k_retain_check<S>), dim3((unsigned)(N - root)), dim3(64), geo_lds_bytes(e), st, e->P, e->geo, e->tv,
                                       root, N, d_ok, d_out));
        HIPCHK(hipGetLastError());
    }
    // ---- propagate: 2^rounds >= N covers every parent chain
    hipLaunchKernelGGL(k_retain_init, per_node, t256, 0, st, e->tv, root, N, revalidate ? d_ok : (const unsigned char*)nullptr, d_a);
    int rounds = 0;
    while ((1ll << rounds) < (long long)N) ++rounds;
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(k_retain_double, per_node, t256, 0, st, N, (const RetainLink*)d_a, d_b);
        std::swap(d_a, d_b);
    }
    // ---- scan
    hipLaunchKernelGGL(k_retain_flags, dim3((unsigned)nblocks), dim3(RETAIN_BLOCK), 0, st, root, N, (const RetainLink*)d_a,
                       revalidate ? d_ok : (const unsigned char*)nullptr, d_keep, d_local, d_sums, d_out);
    hipLaunchKernelGGL(k_retain_scan_sums, dim3(1), dim3(RETAIN_BLOCK), 0, st, nblocks, d_sums, d_out);
    hipLaunchKernelGGL(k_retain_ids, dim3((unsigned)nblocks), dim3(RETAIN_BLOCK), 0, st, e->tv, root, N, (const unsigned char*)d_keep,
                       (const int*)d_local, (const int*)d_sums, (const RetainLink*)d_a, d_newid, d_nelen, d_nsteps);
    hipLaunchKernelGGL(k_retain_parents, per_node, t256, 0, st, e->tv, root, N, (const int*)d_newid, d_npid);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&h, d_out, sizeof h, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const int kept = h.kept;
    if (kept < 1 || kept > N) return fail(LQRRT_E_HIP, "retain: the scan counted %d kept nodes of %d", kept, N);

    // ---- move (nothing of the tree has been written so far).  kept == N: the root is node 0 and nothing was dropped --
    // every node keeps its place.
    std::vector<int> h_npid, h_nelen;
    if (kept < N) {
        const size_t widest = std::max((size_t)H * std::max(n, m), (size_t)m * n);
        rc = dalloc(&sc.big, (size_t)kept * widest);
        g_dalloc_bytes = keep_bytes;
        if (rc) return rc;
        h_npid.resize((size_t)kept); h_nelen.resize((size_t)kept);
        HIPCHK(hipMemcpyAsync(h_npid.data(), d_npid, sizeof(int) * kept, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(h_nelen.data(), d_nelen, sizeof(int) * kept, hipMemcpyDeviceToHost, st));
        // SoA tables: one component at a time through the scratch
        auto move_rows = [&](double* table, int rows) -> int {
            for (int d = 0; d < rows; ++d) {
                double* row = table + (size_t)d * e->cap;
                hipLaunchKernelGGL(k_retain_gather1, per_node, t256, 0, st, (const double*)row, sc.big, (const int*)d_newid, N);
                HIPCHK(hipMemcpyAsync(row, sc.big, sizeof(double) * kept, hipMemcpyDeviceToDevice, st));
            }
            return 0;
        };
        TRY(move_rows(e->tv.state, n));
        TRY(move_rows(e->tv.trig, 2 * e->nw));
        // AoS pools: K whole, the edges row by recorded row
        auto move_pool = [&](double* pool, int w, int per) -> int {
            hipLaunchKernelGGL(k_retain_gather, dim3((unsigned)N), dim3(64), 0, st, (const double*)pool, sc.big, (const int*)d_newid,
                               (const int*)e->tv.elen, N, w, per);
            hipLaunchKernelGGL(k_retain_scatter, dim3((unsigned)kept), dim3(64), 0, st, (const double*)sc.big, pool, (const int*)d_nelen,
                               kept, w, per);
            HIPCHK(hipGetLastError());
            return 0;
        };
        TRY(move_pool(e->tv.K, m * n, 0));
        TRY(move_pool(e->tv.xedge, H * n, n));                  // (reads the OLD edge lengths: tv.elen is replaced last)
        TRY(move_pool(e->tv.uedge, H * m, m));
        HIPCHK(hipMemcpyAsync(e->tv.pID, d_npid, sizeof(int) * kept, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(e->tv.elen, d_nelen, sizeof(int) * kept, hipMemcpyDeviceToDevice, st));
    } else {                                                    // (a loaded tree's root may carry a longer edge: a seed's from now on)
        HIPCHK(hipMemcpyAsync(e->tv.elen, d_nelen, sizeof(int), hipMemcpyDeviceToDevice, st));
    }
    hipLaunchKernelGGL(k_retain_root_edge, dim3(1), dim3(64), 0, st, e->tv, n, m);
    HIPCHK(hipGetLastError());
    // ---- goal (on the new tree)
    if (e->has_goal && kept > 1) {
        DISPATCH(e, hipLaunchKernelGGL((k_retain_goal<S>), dim3((unsigned)((kept - 1 + 255) / 256)), t256, 0, st, e->tv, e->res, kept,
                                       (const int*)d_npid, (const int*)d_nsteps, d_ign, d_out));
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(&h, d_out, sizeof h, hipMemcpyDeviceToHost, st));
    const size_t new_words = (size_t)kept / 64 + 1;
    std::vector<unsigned long long> ign(new_words);
    HIPCHK(hipMemcpyAsync(ign.data(), d_ign, sizeof(unsigned long long) * new_words, hipMemcpyDeviceToHost, st));
    if (old_to_new) HIPCHK(hipMemcpyAsync(old_to_new, d_newid, sizeof(int) * N, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));

    // ---- host state, as lqrrt_tree_load / lqrrt_tree_truncate leave it
    if (kept < N) { e->h_pid.swap(h_npid); e->h_elen.swap(h_nelen); }
    else e->h_elen[0] = 1;
    std::fill(e->h_ign.begin(), e->h_ign.end(), 0ull);
    std::copy(ign.begin(), ign.end(), e->h_ign.begin());
    e->ign_hi = std::max(e->ign_hi, N);                         // the device words of the dropped nodes are cleared by the next upload
    e->ign_dirty = true; e->ign_patch_valid = false;
    e->N = kept;
    e->werr_valid = false;
    e->goal_hits = h.hits;
    if (h.best != ~0ull) { e->best_end = (int)(h.best & 0xffffffffull); e->best_steps = (int64_t)(h.best >> 32); }
    else { e->best_end = -1; e->best_steps = -1; }
    e->mark_N = 0;
    e->tot.tree_size = kept;
    e->ctl_w = 0.0;
    e->proto_cache.clear();                                      // (multi-engine path: the prototype is uploaded again)
    TRY(flush_ignore(e, st, false));
    HIPCHK(hipStreamSynchronize(st));

    out->old_size = N; out->kept = kept; out->outside = h.outside; out->infeasible = h.infeasible; out->orphaned = h.orphaned;
    out->root_feasible = h.root_feasible; out->goal_hits = h.hits; out->best_end = e->best_end; out->best_steps = e->best_steps;
    return 0;
}

extern "C" int lqrrt_tree_retain(lqrrt_engine* e, int new_root, int revalidate, lqrrt_retain_stats* out, int32_t* old_to_new_host,
                                 void* stream) {
    NOT_GENERIC(e);
    if (!e || !out) return fail(LQRRT_E_ARG, "null argument");
    if (!e->has_res || e->N < 1) return fail(LQRRT_E_STATE, "no tree to retain: set_resolution and tree_reset / tree_load first");
    if (new_root < 0 || new_root >= e->N) return fail(LQRRT_E_ARG, "The given parent ID, %d, doesn't exist.", new_root);   // tree.py:83-84
    if ((long long)e->N * e->H > 0x7fffffffLL) return fail(LQRRT_E_ARG, "tree too large for 32-bit step counts");
    TRY(use_device(e));
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipStreamSynchronize(st));                           // nothing of the old tree may still be in flight
    RetainScratch sc;
    return retain_run(e, new_root, revalidate ? 1 : 0, out, old_to_new_host, st, sc);
}
