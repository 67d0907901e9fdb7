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

// Host state of an engine after a retain of its N-node tree, as lqrrt_tree_load / lqrrt_tree_truncate leave it, and the stats.
// h: the counters; ign: the new ignore bitmap (kept / 64 + 1 words); h_npid / h_nelen: the new parents and edge lengths (kept
// entries; not read when every node was kept).  The ignore words still have to be flushed.
static void retain_adopt(lqrrt_engine* e, int N, const RetainOut& h, const std::vector<unsigned long long>& ign, std::vector<int>& h_npid,
                         std::vector<int>& h_nelen, lqrrt_retain_stats* out) {
    const int kept = h.kept;
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
    out->old_size = N; out->kept = kept; out->outside = h.outside; out->infeasible = h.infeasible; out->orphaned = h.orphaned;
    out->root_feasible = h.root_feasible; out->goal_hits = h.hits; out->best_end = e->best_end; out->best_steps = e->best_steps;
}

// ceil(log2 N) double-buffered rounds of a pointer-doubling kernel: 2^rounds >= N covers every parent chain.  `a` ends up as the
// finished links, `b` as the spare.
template <class Link>
static void double_rounds(void (*round)(int, const Link*, Link*), int N, Link*& a, Link*& b, hipStream_t st) {
    for (int r = 0; (1ll << r) < (long long)N; ++r) {
        hipLaunchKernelGGL(round, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, N, (const Link*)a, b);
        std::swap(a, b);
    }
}

// The RetainLink of every node against `root` in d_a (ok == nullptr: every edge passes).  With root 0 and no ok table
// RetainLink::steps is cum - elen[0]: the step sums of the clearance calls (engine_clear.hpp).
static void retain_links(const lqrrt_engine* e, int root, int N, const unsigned char* ok, RetainLink*& d_a, RetainLink*& d_b, hipStream_t st) {
    hipLaunchKernelGGL(k_retain_init, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, e->tv, root, N, ok, d_a);
    double_rounds(k_retain_double, N, d_a, d_b, st);
}

static int retain_run(lqrrt_engine* e, int root, int revalidate, lqrrt_retain_stats* out, int32_t* old_to_new, hipStream_t st,
                      RetainScratch& sc) {
    const int N = e->N, n = e->n, m = e->m, H = e->H;
    const int nblocks = (N + RETAIN_BLOCK - 1) / RETAIN_BLOCK;
    const size_t words = (size_t)e->cap / 64 + 1;
    if (revalidate) TRY(lds_fits(e, geo_lds_bytes(e), "the retain check"));
    // ---- small scratch, carved out of one allocation
    size_t off = 0;
    auto carve = [&](size_t bytes) { const size_t at = off; off += (bytes + 255) / 256 * 256; return at; };
    const size_t o_a = carve(sizeof(RetainLink) * N), o_b = carve(sizeof(RetainLink) * N), o_ok = carve(N), o_keep = carve(N);
    const size_t o_local = carve(sizeof(int) * N), o_sums = carve(sizeof(int) * nblocks), o_newid = carve(sizeof(int) * N);
    const size_t o_nelen = carve(sizeof(int) * N), o_npid = carve(sizeof(int) * N), o_nsteps = carve(sizeof(int) * N);
    const size_t o_ign = carve(sizeof(unsigned long long) * words), o_out = carve(sizeof(RetainOut));
    TRY(dalloc_transient(&sc.small, off));                      // (transient: not part of the engine's footprint)
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
    // ---- propagate
    retain_links(e, root, N, revalidate ? d_ok : (const unsigned char*)nullptr, d_a, d_b, st);
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
        TRY(dalloc_transient(&sc.big, (size_t)kept * widest));
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

    retain_adopt(e, N, h, ign, h_npid, h_nelen, out);
    TRY(flush_ignore(e, st, false));
    HIPCHK(hipStreamSynchronize(st));
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

// --------------------------------------------------------------------------------------------
// Several trees per call: lqrrt_tree_retain_multi (update_plans jobs with a `root`).  The stages of retain_run, each as ONE launch
// whose grid spans the engines of a chunk (retain.hpp k_retain_*_multi), and per CHUNK -- not per engine -- two allocations, two
// waits for the stream before the final one, and a handful of copies: the per-engine arrays of one kind lie back to back in one
// small scratch, so the counters, the ignore bitmaps, the id maps and the new parents / edge lengths each come back in one copy.
//   small  as retain_run's, summed over the chunk's engines (~54 bytes per old node) + a RetainDesc per engine
//   big    the kept rows of ONE pool at a time for every engine of the chunk that moves anything: 8 * widest * (sum of their kept)
//          bytes, widest = max(H n, H m, m n) doubles per node -- for 16 boat_advanced trees that keep 5000 nodes each 77 MB
// Both are freed before the call returns and are not part of any engine's footprint.
struct RetainMultiScratch {
    char* small = nullptr;
    double* big = nullptr;
    ~RetainMultiScratch() {
        if (small) (void)hipFree(small);
        if (big) (void)hipFree(big);
    }
};

// prefix table of a launch from the workgroups every engine takes; returns the grid size
static unsigned retain_grid(const std::vector<long long>& counts, RetainGrid& gr) {
    memset(&gr, 0, sizeof gr);
    const int n = (int)counts.size();
    long long at = 0;
    gr.n = n;
    for (int i = 0; i < n; ++i) { gr.block0[i] = (int)at; at += counts[i]; }
    gr.block0[n] = gr.block0[n + 1] = (int)at;
    return (unsigned)at;
}

constexpr long long RETAIN_MULTI_NODES = 1ll << 25;             // old nodes per chunk: a wavefront per node stays below 2^32 threads per launch

static int retain_multi_chunk(lqrrt_engine** eng, int n, const int32_t* roots, const int32_t* reval, lqrrt_retain_stats* out,
                              int32_t** old_to_new, hipStream_t st) {
    lqrrt_engine* e0 = eng[0];
    const int ns = e0->n, m = e0->m, H = e0->H, nw = e0->nw;
    ProtoTable pt;
    memset(&pt, 0, sizeof pt);
    size_t lds = 0;
    std::vector<size_t> offN((size_t)n + 1, 0), offB((size_t)n + 1, 0), offW((size_t)n + 1, 0);
    int maxN = 1;
    for (int i = 0; i < n; ++i) {
        lqrrt_engine* e = eng[i];
        TRY(multi_sync_proto(e, st));                           // (P, g, r, tv as they are now: a new map has been set before the call)
        pt.p[i] = e->d_proto;
        lds = std::max(lds, geo_lds_bytes(e));
        offN[i + 1] = offN[i] + (size_t)e->N;
        offB[i + 1] = offB[i] + (size_t)((e->N + RETAIN_BLOCK - 1) / RETAIN_BLOCK);
        offW[i + 1] = offW[i] + ((size_t)e->cap / 64 + 1);
        maxN = std::max(maxN, e->N);
    }
    const size_t sumN = offN[n], sumB = offB[n], sumW = offW[n];
    // ---- small scratch: one allocation, one array per kind, the engines' slices back to back in it
    size_t off = 0;
    auto carve = [&](size_t bytes) { const size_t at = off; off += (bytes + 255) / 256 * 256; return at; };
    const size_t o_a = carve(sizeof(RetainLink) * sumN), o_b = carve(sizeof(RetainLink) * sumN), o_ok = carve(sumN), o_keep = carve(sumN);
    const size_t o_local = carve(sizeof(int) * sumN), o_sums = carve(sizeof(int) * sumB), o_newid = carve(sizeof(int) * sumN);
    const size_t o_nelen = carve(sizeof(int) * sumN), o_npid = carve(sizeof(int) * sumN), o_nsteps = carve(sizeof(int) * sumN);
    const size_t o_ign = carve(sizeof(unsigned long long) * sumW), o_out = carve(sizeof(RetainOut) * n), o_desc = carve(sizeof(RetainDesc) * n);
    RetainMultiScratch sc;
    TRY(dalloc_transient(&sc.small, off));                      // (transient: not part of any engine's footprint)
    RetainOut* d_out = (RetainOut*)(sc.small + o_out);
    RetainDesc* d_desc = (RetainDesc*)(sc.small + o_desc);
    int* d_newid = (int*)(sc.small + o_newid);
    int* d_npid = (int*)(sc.small + o_npid);
    int* d_nelen = (int*)(sc.small + o_nelen);
    unsigned long long* d_ign = (unsigned long long*)(sc.small + o_ign);

    std::vector<RetainDesc> hd((size_t)n);
    std::vector<RetainOut> ho((size_t)n);
    std::vector<long long> c_check((size_t)n), c_node((size_t)n), c_one((size_t)n, 1);
    for (int i = 0; i < n; ++i) {
        lqrrt_engine* e = eng[i];
        RetainDesc& d = hd[i];
        memset(&d, 0, sizeof d);
        d.link[0] = (RetainLink*)(sc.small + o_a) + offN[i];
        d.link[1] = (RetainLink*)(sc.small + o_b) + offN[i];
        d.ok = (unsigned char*)(sc.small + o_ok) + offN[i];
        d.keep = (unsigned char*)(sc.small + o_keep) + offN[i];
        d.local = (int*)(sc.small + o_local) + offN[i];
        d.sums = (int*)(sc.small + o_sums) + offB[i];
        d.newid = d_newid + offN[i];
        d.nelen = d_nelen + offN[i];
        d.npid = d_npid + offN[i];
        d.nsteps = (int*)(sc.small + o_nsteps) + offN[i];
        d.ign = d_ign + offW[i];
        d.out = d_out + i;
        d.root = roots[i]; d.N = e->N; d.revalidate = reval && reval[i] ? 1 : 0;
        d.nblocks = (int)(offB[i + 1] - offB[i]);
        memset(&ho[i], 0, sizeof(RetainOut));
        ho[i].best = ~0ull;
        ho[i].root_feasible = 1;
        c_check[i] = d.revalidate ? (long long)(e->N - roots[i]) : 0;
        c_node[i] = d.nblocks;
    }
    HIPCHK(hipMemcpyAsync(d_out, ho.data(), sizeof(RetainOut) * n, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_desc, hd.data(), sizeof(RetainDesc) * n, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_ign, 0, sizeof(unsigned long long) * sumW, st));
    const dim3 t256(RETAIN_BLOCK), t64(64);
    RetainGrid g_check, g_node, g_one;
    const unsigned n_check = retain_grid(c_check, g_check), n_node = retain_grid(c_node, g_node);
    (void)retain_grid(c_one, g_one);

    // ---- check (the engines that revalidate), with the largest LDS image of the call's geometries
    if (n_check > 0) {
        DISPATCH(e0, hipLaunchKernelGGL((k_retain_check_multi<S>), dim3(n_check), t64, lds, st, pt, (const RetainDesc*)d_desc, g_check));
        HIPCHK(hipGetLastError());
    }
    // ---- propagate: 2^rounds >= the LARGEST tree of the chunk (retain.hpp: the extra rounds are the identity on a smaller one)
    hipLaunchKernelGGL(k_retain_init_multi, dim3(n_node), t256, 0, st, pt, (const RetainDesc*)d_desc, g_node);
    int rounds = 0;
    while ((1ll << rounds) < (long long)maxN) ++rounds;
    for (int r = 0; r < rounds; ++r)
        hipLaunchKernelGGL(k_retain_double_multi, dim3(n_node), t256, 0, st, pt, (const RetainDesc*)d_desc, g_node, r & 1);
    const int fin = rounds & 1;
    // ---- scan
    hipLaunchKernelGGL(k_retain_flags_multi, dim3(n_node), t256, 0, st, pt, (const RetainDesc*)d_desc, g_node, fin);
    hipLaunchKernelGGL(k_retain_scan_sums_multi, dim3((unsigned)n), t256, 0, st, (const RetainDesc*)d_desc, n);
    hipLaunchKernelGGL(k_retain_ids_multi, dim3(n_node), t256, 0, st, pt, (const RetainDesc*)d_desc, g_node, fin);
    hipLaunchKernelGGL(k_retain_parents_multi, dim3(n_node), t256, 0, st, pt, (const RetainDesc*)d_desc, g_node);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(ho.data(), d_out, sizeof(RetainOut) * n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    size_t sum_kept = 0;
    bool any_moves = false;
    for (int i = 0; i < n; ++i) {
        const int kept = ho[i].kept;
        if (kept < 1 || kept > eng[i]->N) return fail(LQRRT_E_HIP, "retain: the scan counted %d kept nodes of %d (engine %d)", kept, eng[i]->N, i);
        if (kept < eng[i]->N) { sum_kept += (size_t)kept; any_moves = true; }
    }

    // ---- move (nothing of any tree has been written so far).  An engine that keeps every node moves nothing.
    const size_t widest = std::max(std::max((size_t)H * std::max(ns, m), (size_t)m * ns), (size_t)std::max(ns, 2 * nw));
    if (any_moves) TRY(dalloc_transient(&sc.big, sum_kept * widest));
    std::vector<RetainDesc> hd2(hd);                           // (a second staging copy: the first upload may still read `hd`)
    std::vector<long long> c_old((size_t)n), c_oldb((size_t)n), c_new((size_t)n), c_newb((size_t)n), c_small((size_t)n), c_goal((size_t)n);
    {
        size_t at = 0;
        for (int i = 0; i < n; ++i) {
            lqrrt_engine* e = eng[i];
            const int kept = ho[i].kept;
            const bool mv = kept < e->N;
            hd2[i].moves = mv ? 1 : 0;
            hd2[i].big = mv ? sc.big + at * widest : nullptr;
            hd2[i].has_goal = (e->has_goal && kept > 1) ? 1 : 0;
            if (mv) at += (size_t)kept;
            c_old[i] = mv ? e->N : 0;
            c_oldb[i] = mv ? hd2[i].nblocks : 0;
            c_new[i] = mv ? kept : 0;
            c_newb[i] = mv ? (kept + RETAIN_BLOCK - 1) / RETAIN_BLOCK : 0;
            c_small[i] = mv ? c_newb[i] : 1;
            c_goal[i] = hd2[i].has_goal ? (kept - 1 + RETAIN_BLOCK - 1) / RETAIN_BLOCK : 0;
        }
    }
    HIPCHK(hipMemcpyAsync(d_desc, hd2.data(), sizeof(RetainDesc) * n, hipMemcpyHostToDevice, st));
    RetainGrid g_old, g_oldb, g_new, g_newb, g_small, g_goal;
    const unsigned n_old = retain_grid(c_old, g_old), n_oldb = retain_grid(c_oldb, g_oldb), n_new = retain_grid(c_new, g_new);
    const unsigned n_newb = retain_grid(c_newb, g_newb), n_small = retain_grid(c_small, g_small), n_goal = retain_grid(c_goal, g_goal);
    if (any_moves) {
        // SoA tables: all components of a table through the scratch at once
        for (int which = 0; which < 2; ++which) {
            const int rows = which == 0 ? ns : 2 * nw;
            if (rows < 1) continue;
            hipLaunchKernelGGL(k_retain_gather1_multi, dim3(n_oldb, (unsigned)rows), t256, 0, st, pt, (const RetainDesc*)d_desc, g_oldb, which);
            hipLaunchKernelGGL(k_retain_scatter1_multi, dim3(n_newb, (unsigned)rows), t256, 0, st, pt, (const RetainDesc*)d_desc, g_newb, which);
        }
        // AoS pools: K whole, the edges row by recorded row (the gathers read the OLD edge lengths: tv.elen is replaced last)
        const int pw[3] = {m * ns, H * ns, H * m}, pper[3] = {0, ns, m};
        for (int which = 0; which < 3; ++which) {
            hipLaunchKernelGGL(k_retain_gather_multi, dim3(n_old), t64, 0, st, pt, (const RetainDesc*)d_desc, g_old, which, pw[which], pper[which]);
            hipLaunchKernelGGL(k_retain_scatter_multi, dim3(n_new), t64, 0, st, pt, (const RetainDesc*)d_desc, g_new, which, pw[which], pper[which]);
        }
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_retain_small_multi, dim3(n_small), t256, 0, st, pt, (const RetainDesc*)d_desc, g_small);
    hipLaunchKernelGGL(k_retain_root_edge_multi, dim3((unsigned)n), t64, 0, st, pt, n, ns, m);
    HIPCHK(hipGetLastError());
    // ---- goal (on the new trees)
    if (n_goal > 0) {
        DISPATCH(e0, hipLaunchKernelGGL((k_retain_goal_multi<S>), dim3(n_goal), t256, 0, st, pt, (const RetainDesc*)d_desc, g_goal));
        HIPCHK(hipGetLastError());
    }
    // ---- back to the host: one copy per kind for the whole chunk
    std::vector<unsigned long long> h_ign(sumW);
    std::vector<int> h_newid, h_npid_all, h_nelen_all;
    bool want_map = false;
    if (old_to_new)
        for (int i = 0; i < n; ++i) want_map = want_map || old_to_new[i] != nullptr;
    HIPCHK(hipMemcpyAsync(ho.data(), d_out, sizeof(RetainOut) * n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h_ign.data(), d_ign, sizeof(unsigned long long) * sumW, hipMemcpyDeviceToHost, st));
    if (want_map) {
        h_newid.resize(sumN);
        HIPCHK(hipMemcpyAsync(h_newid.data(), d_newid, sizeof(int) * sumN, hipMemcpyDeviceToHost, st));
    }
    if (any_moves) {
        h_npid_all.resize(sumN); h_nelen_all.resize(sumN);
        HIPCHK(hipMemcpyAsync(h_npid_all.data(), d_npid, sizeof(int) * sumN, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(h_nelen_all.data(), d_nelen, sizeof(int) * sumN, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));

    // ---- host state of every engine, as retain_run leaves it
    for (int i = 0; i < n; ++i) {
        lqrrt_engine* e = eng[i];
        const int N = e->N, kept = ho[i].kept;
        std::vector<int> h_npid, h_nelen;
        if (kept < N) {
            h_npid.assign(h_npid_all.begin() + (ptrdiff_t)offN[i], h_npid_all.begin() + (ptrdiff_t)offN[i] + kept);
            h_nelen.assign(h_nelen_all.begin() + (ptrdiff_t)offN[i], h_nelen_all.begin() + (ptrdiff_t)offN[i] + kept);
        }
        const std::vector<unsigned long long> ign(h_ign.begin() + (ptrdiff_t)offW[i], h_ign.begin() + (ptrdiff_t)offW[i] + (kept / 64 + 1));
        if (old_to_new && old_to_new[i]) memcpy(old_to_new[i], h_newid.data() + offN[i], sizeof(int) * (size_t)N);
        retain_adopt(e, N, ho[i], ign, h_npid, h_nelen, &out[i]);
        TRY(flush_ignore(e, st, false));
    }
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

extern "C" int lqrrt_tree_retain_multi(lqrrt_engine** engines, int n, const int32_t* new_roots, const int32_t* revalidate,
                                       lqrrt_retain_stats* out, int32_t** old_to_new_host, void* stream) {
    if (!engines || n < 1) return fail(LQRRT_E_ARG, "no engines");
    if (!new_roots || !out) return fail(LQRRT_E_ARG, "null argument");
    if (n > 4 * MULTI_MAX) return fail(LQRRT_E_ARG, "at most %d engines per call", 4 * (int)MULTI_MAX);
    lqrrt_engine* e0 = engines[0];
    // every argument of every engine, before anything is written
    for (int i = 0; i < n; ++i) {
        lqrrt_engine* e = engines[i];
        if (!e) return fail(LQRRT_E_ARG, "null engine");
        NOT_GENERIC(e);
        for (int j = 0; j < i; ++j)
            if (engines[j] == e) return fail(LQRRT_E_ARG, "engine %d appears twice", i);
        if (e->device != e0->device || e->model != e0->model || e->H != e0->H || (e->d_S != nullptr) != (e0->d_S != nullptr))
            return fail(LQRRT_E_ARG, "engines of one call share the device, the model, the horizon and the form of S");
        if (!e->has_res || e->N < 1) return fail(LQRRT_E_STATE, "no tree to retain: set_resolution and tree_reset / tree_load first");
        if (new_roots[i] < 0 || new_roots[i] >= e->N) return fail(LQRRT_E_ARG, "The given parent ID, %d, doesn't exist.", new_roots[i]);   // tree.py:83-84
        if ((long long)e->N * e->H > 0x7fffffffLL) return fail(LQRRT_E_ARG, "tree too large for 32-bit step counts");
    }
    TRY(use_device(e0));
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipStreamSynchronize(st));                           // nothing of the old trees may still be in flight
    // chunks of up to MULTI_MAX engines (the pointer table of a launch), one after the other on the same stream
    for (int first = 0; first < n;) {
        int count = 0;
        long long nodes = 0;
        while (first + count < n && count < MULTI_MAX && (count == 0 || nodes + engines[first + count]->N <= RETAIN_MULTI_NODES)) {
            nodes += engines[first + count]->N;
            ++count;
        }
        const int rc = retain_multi_chunk(engines + first, count, new_roots + first, revalidate ? revalidate + first : nullptr, out + first,
                                          old_to_new_host ? old_to_new_host + first : nullptr, st);
        if (rc) {
            const std::string keep = g_err;
            (void)hipStreamSynchronize(st);                     // nothing in flight when the scratch goes
            g_err = keep;
            return rc;
        }
        first += count;
    }
    return 0;
}
