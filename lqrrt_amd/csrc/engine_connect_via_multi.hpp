// ABI: goal chains through waypoints for several trees per call -- lqrrt_connect_via_search_multi / lqrrt_connect_via_commit_multi
// (connect_vias; kernels in connect_via_multi.hpp).  Fragment of engine.hip, behind engine_connect_via.hpp.  Every argument of every
// engine is checked, with the one-engine calls' own checkers, before anything is written or launched.  The calls run on
// engine_refine.hpp's multi path: its chunks, scratch (d_refm: not part of the footprint), prototypes, keys, commit head and guard.
// A search's image per chunk: the keys, then a ConnectViaDesc per engine, then every engine's waypoints (8-byte aligned: Carve
// rounds to 16), depth table and id list.  A commit's image per chunk of up to MULTI_MAX winners: every engine's out[3] and edge
// lengths (what comes back), then a ConnectViaCommitDesc per engine and the waypoints; one workgroup per winner.
// --------------------------------------------------------------------------------------------

// what the two calls check alike, for every engine, behind connect_multi_check
static int connect_via_multi_check(lqrrt_engine** engines, int n, const double* const* waypoints, const int32_t* Q, const int32_t* tries,
                                   const int32_t* horizons) {
    TRY(connect_multi_check(engines, n, tries, horizons));
    if (!Q) return fail(LQRRT_E_ARG, "null argument");
    for (int k = 0; k < n; ++k)
        TRY(connect_via_check(engines[k], waypoints ? waypoints[k] : nullptr, Q[k], tries[k], horizons[k]));
    return 0;
}

// member k's waypoints into the image at o_way, and the argument block of its chains over them
static void connect_via_stage_way(const lqrrt_engine* e, const double* way, int Q, int tries, int horizon, MultiChunk& c, char* d_img,
                                  size_t o_way, ConnectViaArgs* a) {
    if (Q) memcpy(c.img.data() + o_way, way, sizeof(double) * (size_t)Q * e->n);
    connect_via_fill_args(e, (const double*)(d_img + o_way), Q, tries, horizon, a);
}

static int connect_via_search_multi_run(lqrrt_engine** engines, int n, const int32_t* const* nodes, const std::vector<int>& counts,
                                        const std::vector<std::vector<int>>& depths, const double* const* waypoints, const int32_t* Q,
                                        const int32_t* tries, const int32_t* horizons, const int64_t* incumbents, int64_t* cost,
                                        int32_t* node_out, int32_t* j_out, hipStream_t st) {
    std::vector<long long> cands((size_t)n);                    // (an empty id list: no launch, no winner)
    for (int k = 0; k < n; ++k) cands[k] = (long long)counts[k] * ((long long)Q[k] + 1);
    std::vector<MultiChunk> chunks = multi_chunks(cands);
    StreamDrain drain(st);
    for (MultiChunk& c : chunks) {
        const int m = (int)c.members.size();
        Carve carve;
        carve(sizeof(unsigned long long) * m);                  // the keys
        const size_t o_desc = carve(sizeof(ConnectViaDesc) * m);
        std::vector<size_t> o_way((size_t)m), o_depth((size_t)m), o_ids((size_t)m);
        for (int q = 0; q < m; ++q) {
            const int k = c.members[q];
            o_way[q] = carve(sizeof(double) * (size_t)Q[k] * engines[k]->n);
            o_depth[q] = carve(sizeof(int) * depths[k].size());
            o_ids[q] = carve(nodes && nodes[k] ? sizeof(int) * (size_t)counts[k] : 0);
        }
        c.img.assign(carve.off, 0);
        char* d_img = nullptr;
        TRY(refine_multi_scratch(engines[c.first], carve.off, &d_img));
        ConnectViaDesc* hd = (ConnectViaDesc*)(c.img.data() + o_desc);
        for (int q = 0; q < m; ++q) {
            const int k = c.members[q];
            const bool listed = nodes && nodes[k];
            ((unsigned long long*)c.img.data())[q] = incumbent_key(incumbents[k]);   // (incumbent, candidate 0)
            memcpy(c.img.data() + o_depth[q], depths[k].data(), sizeof(int) * depths[k].size());
            if (listed) memcpy(c.img.data() + o_ids[q], nodes[k], sizeof(int) * (size_t)counts[k]);
            ConnectViaArgs& a = hd[q].a;
            connect_via_stage_way(engines[k], waypoints ? waypoints[k] : nullptr, Q[k], tries[k], horizons[k], c, d_img, o_way[q], &a);
            a.depth = (const int*)(d_img + o_depth[q]);
            a.nodes = listed ? (const int*)(d_img + o_ids[q]) : nullptr;
            a.count = counts[k];
            hd[q].best = (unsigned long long*)d_img + q;
        }
        ProtoTable pt;
        size_t lds = 0;
        TRY(refine_multi_protos(engines, c, horizons, st, pt, lds));
        RetainGrid gr;
        const unsigned grid = multi_grid(c, cands, gr);
        drain.arm();
        HIPCHK(hipMemcpyAsync(d_img, c.img.data(), c.img.size(), hipMemcpyHostToDevice, st));
        DISPATCH(engines[0], hipLaunchKernelGGL((k_connect_via_search_multi<S>), dim3(grid), dim3(64), lds, st, pt,
                                                (const ConnectViaDesc*)(d_img + o_desc), gr));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(c.img.data(), d_img, sizeof(unsigned long long) * m, hipMemcpyDeviceToHost, st));
    }
    std::vector<unsigned long long> keys;
    TRY(multi_search_keys(chunks, n, incumbents, st, drain, keys));
    for (int k = 0; k < n; ++k)
        if (keys[k] != incumbent_key(incumbents[k])) connect_via_decode(keys[k], nodes ? nodes[k] : nullptr, Q[k], &cost[k], &node_out[k], &j_out[k]);
    return 0;
}

extern "C" int lqrrt_connect_via_search_multi(lqrrt_engine** engines, int n, const int32_t* const* nodes, const int32_t* counts,
                                              const double* const* waypoints, const int32_t* Q, const int32_t* goal_tries,
                                              const int32_t* horizon_iters, const int64_t* incumbents, int64_t* cost_out,
                                              int32_t* node_out, int32_t* j_out, void* stream) {
    TRY(connect_via_multi_check(engines, n, waypoints, Q, goal_tries, horizon_iters));
    if (!incumbents || !cost_out || !node_out || !j_out) return fail(LQRRT_E_ARG, "null argument");
    std::vector<int> cnt((size_t)n);
    std::vector<std::vector<int>> depths((size_t)n);
    for (int k = 0; k < n; ++k) {
        lqrrt_engine* e = engines[k];
        const int32_t* ids = nullptr;
        TRY(incumbent_check(incumbents[k], k));
        TRY(multi_id_list(nodes, counts, k, &ids, &cnt[k]));
        TRY(connect_via_candidates_check(e, ids, &cnt[k], Q[k], k));
        depths[k].assign((size_t)e->N, 0);
        TRY(connect_depths(e, 0, horizon_iters[k], depths[k].data()));
        TRY(connect_via_deepest_check(depths[k].data(), e->N, ids, cnt[k], Q[k], goal_tries[k], horizon_iters[k], k));
    }
    TRY(use_device(engines[0]));
    for (int k = 0; k < n; ++k) { cost_out[k] = incumbents[k]; node_out[k] = -1; j_out[k] = -1; }
    return connect_via_search_multi_run(engines, n, nodes, cnt, depths, waypoints, Q, goal_tries, horizon_iters, incumbents, cost_out,
                                        node_out, j_out, (hipStream_t)stream);
}

static int connect_via_commit_multi_run(lqrrt_engine** engines, int n, const int32_t* nodes, const int32_t* cj,
                                        const std::vector<long long>& depth, const std::vector<int>& room, const double* const* waypoints,
                                        const int32_t* Q, const int32_t* tries, const int32_t* horizons, int32_t* const* ids_out,
                                        int32_t* counts_out, hipStream_t st) {
    std::vector<long long> winner((size_t)n);
    for (int k = 0; k < n; ++k) { counts_out[k] = 0; winner[k] = nodes[k] >= 0; }   // (no winner: not part of the launch)
    std::vector<MultiChunk> chunks = multi_chunks(winner);
    StreamDrain drain(st);
    for (MultiChunk& c : chunks) {
        const int m = (int)c.members.size();
        Carve carve;
        multi_commit_head(c, room, carve);
        const size_t o_desc = carve(sizeof(ConnectViaCommitDesc) * m);
        std::vector<size_t> o_way((size_t)m);
        for (int q = 0; q < m; ++q) o_way[q] = carve(sizeof(double) * (size_t)Q[c.members[q]] * engines[c.members[q]]->n);
        c.img.assign(carve.off, 0);
        char* d_img = nullptr;
        TRY(refine_multi_scratch(engines[c.first], carve.off, &d_img));
        ConnectViaCommitDesc* hd = (ConnectViaCommitDesc*)(c.img.data() + o_desc);
        for (int q = 0; q < m; ++q) {
            const int k = c.members[q];
            connect_via_stage_way(engines[k], waypoints ? waypoints[k] : nullptr, Q[k], tries[k], horizons[k], c, d_img, o_way[q], &hd[q].a);
            hd[q].out = c.out_of(d_img, q);
            hd[q].lens = c.lens_of(d_img, q);
            hd[q].v = nodes[k]; hd[q].j = cj[k]; hd[q].depth = (int)depth[k]; hd[q].base = engines[k]->N;
        }
        ProtoTable pt;
        size_t lds = 0;
        TRY(refine_multi_protos(engines, c, horizons, st, pt, lds));
        drain.arm();
        HIPCHK(hipMemcpyAsync(d_img, c.img.data(), c.img.size(), hipMemcpyHostToDevice, st));
        DISPATCH(engines[0], hipLaunchKernelGGL((k_connect_via_commit_multi<S>), dim3((unsigned)m), dim3(64), lds, st, pt,
                                                (const ConnectViaCommitDesc*)(d_img + o_desc), m));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(c.img.data(), d_img, c.back, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    drain.disarm();
    multi_commit_adopt(engines, chunks, std::vector<int>(nodes, nodes + n), ids_out, counts_out);
    return 0;
}

extern "C" int lqrrt_connect_via_commit_multi(lqrrt_engine** engines, int n, const int32_t* nodes, const int32_t* j,
                                              const double* const* waypoints, const int32_t* Q, const int32_t* goal_tries,
                                              const int32_t* horizon_iters, int32_t* const* ids_out, const int32_t* cap_ids,
                                              int32_t* counts_out, void* stream) {
    TRY(connect_via_multi_check(engines, n, waypoints, Q, goal_tries, horizon_iters));
    if (!nodes || !j || !ids_out || !cap_ids || !counts_out) return fail(LQRRT_E_ARG, "null argument");
    std::vector<long long> depth((size_t)n, 0);
    std::vector<int> room((size_t)n, 0);
    for (int k = 0; k < n; ++k) {
        if (nodes[k] == -1) continue;                           // an engine without a winner
        TRY(connect_via_winner_check(engines[k], nodes[k], j[k], Q[k], goal_tries[k], horizon_iters[k], ids_out[k], cap_ids[k], k, &depth[k],
                                     &room[k]));
    }
    TRY(use_device(engines[0]));
    return connect_via_commit_multi_run(engines, n, nodes, j, depth, room, waypoints, Q, goal_tries, horizon_iters, ids_out, counts_out,
                                        (hipStream_t)stream);
}
