// ABI: goal chains clear of moving discs -- lqrrt_tree_clear_connect (Planner.avoid(connect); kernels in clear_connect.hpp, the rule
// restated in tests/clear_connect_reference.py).  lqrrt_tree_clear's query and lqrrt_connect_search's in one call: the clearance of
// the tree as engine_clear.hpp runs it, then a search over the nodes whose root paths are clear for the goal chain that stays clear
// at its own times and beats the best clear hit.  Reads the tree and writes nothing of it; the winner is replayed by the unchanged
// lqrrt_connect_commit.  Fragment of engine.hip, behind engine_clear.hpp (clear_check, ClearPlain, ClearBufs, ClearScratch) and
// engine_connect.hpp (connect_check, connect_candidates_check, connect_depths, connect_fill_args).
// --------------------------------------------------------------------------------------------

// Scratch of one call, all of it transient (one allocation, freed before the call returns, not part of the footprint): per node the
// 60 bytes of lqrrt_tree_clear and 4 of the depth table, 4 per listed id, the table's 32 L D bytes, the two counter blocks.

// dynamic LDS of the search: the refinement's layout, then the hull points of the disc test (clear_connect.hpp)
static size_t clear_connect_lds_bytes(const lqrrt_engine* e, int horizon) {
    return refine_lds_bytes(e, horizon) + sizeof(double) * (size_t)2 * e->geo.V;
}

// one 64-thread workgroup per candidate (a model without a circle path has no such kernel: clear_check refused it)
template <class S>
static void clear_connect_search(const lqrrt_engine* e, const ConnectArgs& a, const ClearConnectArgs& c, ClearConnectOut* d_win, hipStream_t st) {
    hipLaunchKernelGGL((k_clear_connect_search<S>), dim3((unsigned)a.count), dim3(64), clear_connect_lds_bytes(e, a.H), st, e->P, e->geo,
                       e->res, e->tv, a, c, d_win);
}

// The launches of a checked call: lqrrt_tree_clear's stages, the seed, the search, and the call's one synchronise.  `depth`: the
// table of connect_depths; `ids` (null: every node) of `count` entries.
static int clear_connect_run(lqrrt_engine* e, const std::vector<long long>& cum, const std::vector<double>& table,
                             const std::vector<int>& depth, const int32_t* ids, int count, int L, int D, int start, int horizon, int tries,
                             lqrrt_clear_stats* out, lqrrt_clear_connect_stats* chain, int32_t* first_host, int32_t* dwell_host,
                             hipStream_t st) {
    typedef ClearPlain C;
    const int N = e->N;
    const size_t hull_bytes = sizeof(double) * (size_t)2 * e->geo.V;
    // ---- scratch, carved out of one allocation
    Carve carve{0, 256};
    const size_t o_a = carve(sizeof(RetainLink) * N), o_b = carve(sizeof(RetainLink) * N);
    const size_t o_ca = carve(sizeof(ClearLink) * N), o_cb = carve(sizeof(ClearLink) * N);
    const size_t o_own = carve(sizeof(int) * N), o_dwell = carve(sizeof(int) * N), o_ans = carve(sizeof(int) * N);
    const size_t o_table = carve(sizeof(double) * table.size()), o_out = carve(sizeof(ClearOut));
    const size_t o_depth = carve(sizeof(int) * N), o_ids = carve(ids ? sizeof(int) * (size_t)count : 0), o_win = carve(sizeof(ClearConnectOut));
    ClearScratch sc;
    TRY(dalloc_transient(&sc.mem, carve.off));                  // (transient: not part of the engine's footprint)
    ClearBufs<C> d = {(RetainLink*)(sc.mem + o_a), (RetainLink*)(sc.mem + o_b), (ClearLink*)(sc.mem + o_ca), (ClearLink*)(sc.mem + o_cb),
                      (int*)(sc.mem + o_own), (int*)(sc.mem + o_dwell), (int*)(sc.mem + o_ans), nullptr, (double*)(sc.mem + o_table),
                      (ClearOut*)(sc.mem + o_out)};
    int* d_depth = (int*)(sc.mem + o_depth);
    int* d_ids = ids && count ? (int*)(sc.mem + o_ids) : nullptr;
    ClearConnectOut* d_win = (ClearConnectOut*)(sc.mem + o_win);
    ClearOut h{};
    h.best = ~0ull;
    ClearConnectOut w{};                                        // (the key is the seed kernel's to write)
    StreamDrain drain(st);                                      // (the scratch is in use by the stream, h and w sources and targets of copies)
    drain.arm();
    HIPCHK(hipMemcpyAsync(d.out, &h, sizeof h, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_win, &w, sizeof w, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d.table, table.data(), sizeof(double) * table.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_depth, depth.data(), sizeof(int) * (size_t)N, hipMemcpyHostToDevice, st));
    if (d_ids) HIPCHK(hipMemcpyAsync(d_ids, ids, sizeof(int) * (size_t)count, hipMemcpyHostToDevice, st));
    // ---- lqrrt_tree_clear's stages: steps, check, propagate, select
    retain_links(e, 0, N, nullptr, d.a, d.b, st);
    HIPCHK(hipGetLastError());
    DISPATCH(e, if constexpr (has_discs<S>::value) C::template check<S>(e, d, N, L, D, start, 1, hull_bytes, st));
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL((k_clear_init<ClearLink>), dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, e->tv, N, (const int*)d.own, d.ca);
    double_rounds(k_clear_double<ClearLink>, N, d.ca, d.cb, st);
    C::select(e, d, N, st);
    HIPCHK(hipGetLastError());
    // ---- the search: seeded with the best clear hit's depth, over the candidates whose root paths are clear
    hipLaunchKernelGGL(k_clear_connect_seed, dim3(1), dim3(1), 0, st, e->tv, (const ClearOut*)d.out, d_win);
    HIPCHK(hipGetLastError());
    if (count > 0) {
        ConnectArgs a;
        connect_fill_args(e, d_depth, d_ids, count, tries, horizon, &a);
        const ClearConnectArgs c = {d.table, d.ans, d.a, L, D, start, 0};
        DISPATCH(e, if constexpr (has_discs<S>::value) clear_connect_search<S>(e, a, c, d_win, st));
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(&h, d.out, sizeof h, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&w, d_win, sizeof w, hipMemcpyDeviceToHost, st));
    if (first_host) HIPCHK(hipMemcpyAsync(first_host, d.ans, sizeof(int) * N, hipMemcpyDeviceToHost, st));
    if (dwell_host) HIPCHK(hipMemcpyAsync(dwell_host, d.dwell, sizeof(int) * N, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    drain.disarm();
    C::stats(h, cum, N, out);
    // every node with first == -1 is neither a conflict nor blocked; of an id list the search counted its entries
    chain->clear_candidates = ids ? w.listed_clear : N - h.conflicts - h.blocked;
    chain->reserved = 0;
    const long long incumbent = out->best_end >= 0 ? out->best_steps - e->h_elen[0] + 1 : 0x7fffffffLL;
    if (w.key != ((unsigned long long)incumbent << 32)) {
        const int v = (int)(w.key & 0xffffffffull);
        chain->chain_from = v;
        chain->chain_cost = (int64_t)(w.key >> 32);
        chain->chain_rows = (int32_t)(chain->chain_cost - depth[(size_t)v]);
        chain->chain_arrival = (int64_t)(cum[(size_t)v] + chain->chain_rows);
    } else { chain->chain_from = -1; chain->chain_rows = -1; chain->chain_cost = -1; chain->chain_arrival = -1; }
    return 0;
}

extern "C" int lqrrt_tree_clear_connect(lqrrt_engine* e, const double* tracks_host, const double* radii_host, int L, int D, int start,
                                        int horizon_iters, int goal_tries, const int32_t* nodes_host, int count, lqrrt_clear_stats* out,
                                        lqrrt_clear_connect_stats* chain, int32_t* first_host, int32_t* dwell_host, void* stream) {
    NOT_GENERIC(e);
    std::vector<long long> cum;
    std::vector<double> table;
    // lqrrt_tree_clear's refusals, in its order; then lqrrt_connect_search's; then the LDS of the search
    TRY(clear_check<ClearPlain>(e, out, tracks_host, radii_host, L, D, start, 1, cum, table));
    if (!chain) return fail(LQRRT_E_ARG, "null argument");
    TRY(connect_check(e, goal_tries, horizon_iters));
    TRY(connect_candidates_check(e, nodes_host, &count, -1));
    std::vector<int> depth((size_t)e->N, 0);
    TRY(connect_depths(e, goal_tries, horizon_iters, depth.data()));
    const size_t lds = clear_connect_lds_bytes(e, horizon_iters);
    if (e->lds_limit && lds > e->lds_limit)
        return fail(LQRRT_E_ARG, "the search stages the static geometry, an edge of %d rows and the hull points of the disc test in LDS: %zu bytes "
                    "(V = %d, O = %d), the device's limit is %zu", horizon_iters, lds, e->geo.V, e->geo.O, e->lds_limit);
    TRY(use_device(e));
    return clear_connect_run(e, cum, table, depth, nodes_host, count, L, D, start, horizon_iters, goal_tries, out, chain, first_host,
                             dwell_host, (hipStream_t)stream);
}
