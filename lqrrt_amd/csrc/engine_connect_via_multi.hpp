// ABI: goal chains through waypoints for several trees per call -- lqrrt_connect_via_search_multi / lqrrt_connect_via_commit_multi
// (connect_vias; kernels in connect_via_multi.hpp).  Fragment of engine.hip, behind engine_connect_via.hpp, in the structure of
// engine_connect.hpp's multi path, whose helpers it uses.  Every argument of every engine is checked, with the rules of the
// one-engine calls, before anything is written or launched.  A search call is cut into CHUNKS of up to MULTI_MAX engines with
// candidates (fewer than 2^32 threads per launch); per chunk one image in device memory -- the keys, then a ConnectViaDesc per
// engine, then every engine's waypoints (8-byte aligned: carve rounds to 16), depth table and id list -- staged on the host and
// uploaded in one copy; one launch; the keys back in one copy.  The chunks of a call are enqueued one after another and waited for
// once.  The image lives in the scratch of the chunk's first engine that refine_plans' and connect_goals' calls use too
// (refine_multi_scratch, d_refm: not part of the footprint); the calls are synchronous, so nothing reads it after they return.
// The commit: per chunk of up to MULTI_MAX winners one image -- every engine's out[3] and edge lengths (what comes back), then a
// ConnectViaCommitDesc per engine and the waypoints --, one launch (one workgroup per winner), one read-back.
// --------------------------------------------------------------------------------------------
struct ConnectViaChunk {
    int first = 0;                        // the engine (index into the call) whose scratch holds the image
    std::vector<int> members;             // indices (into the call) of the engines that take part in the launch
    std::vector<char> img;                // host image of the scratch
    size_t o_out = 0, o_lens = 0;         // commit: where the outputs and the edge lengths lie in the image
    std::vector<size_t> lens_at;          // commit, per member: its first edge length (ints from o_lens)
};

// what the two calls check alike, for every engine, behind connect_multi_check
static int connect_via_multi_check(lqrrt_engine** engines, int n, const double* const* waypoints, const int32_t* Q, const int32_t* tries,
                                   const int32_t* horizons) {
    TRY(connect_multi_check(engines, n, tries, horizons));
    if (!Q) return fail(LQRRT_E_ARG, "null argument");
    for (int k = 0; k < n; ++k)
        TRY(connect_via_check(engines[k], waypoints ? waypoints[k] : nullptr, Q[k], tries[k], horizons[k]));
    return 0;
}

static void connect_via_multi_args(const lqrrt_engine* e, const double* way_dev, int Q, int tries, int horizon, ConnectViaArgs* a) {
    a->way = way_dev;
    a->nodes = nullptr; a->depth = nullptr;
    a->count = 0; a->Q = Q; a->tries = tries; a->H = horizon;
    for (int d = 0; d < MAXN; ++d) a->goal[d] = d < e->n ? e->goal[d] : 0.0;
}

static int connect_via_search_multi_run(lqrrt_engine** engines, int n, const int32_t* const* nodes, const std::vector<int>& counts,
                                        const std::vector<std::vector<int>>& depths, const double* const* waypoints, const int32_t* Q,
                                        const int32_t* tries, const int32_t* horizons, const int64_t* incumbents, int64_t* cost,
                                        int32_t* node_out, int32_t* j_out, hipStream_t st, std::vector<ConnectViaChunk>& chunks) {
    // chunks: up to MULTI_MAX engines with candidates, one 64-thread workgroup per candidate and fewer than 2^32 threads per launch
    long long cands = 0;
    for (int k = 0; k < n; ++k) {
        if (counts[k] == 0) continue;                           // (an empty id list: no launch, no winner)
        const long long mine = (long long)counts[k] * ((long long)Q[k] + 1);
        if (chunks.empty() || (int)chunks.back().members.size() == MULTI_MAX || (cands + mine) * 64 > 0xffffffffLL) {
            chunks.emplace_back();
            chunks.back().first = k;
            cands = 0;
        }
        chunks.back().members.push_back(k);
        cands += mine;
    }
    for (ConnectViaChunk& c : chunks) {
        const int m = (int)c.members.size();
        size_t off = 0;
        auto carve = [&](size_t bytes) { const size_t at = off; off += (bytes + 15) / 16 * 16; return at; };
        const size_t o_keys = carve(sizeof(unsigned long long) * m);
        const size_t o_desc = carve(sizeof(ConnectViaDesc) * m);
        std::vector<size_t> o_way((size_t)m), o_depth((size_t)m), o_ids((size_t)m);
        for (int q = 0; q < m; ++q) {
            const int k = c.members[q];
            o_way[q] = carve(sizeof(double) * (size_t)Q[k] * engines[k]->n);
            o_depth[q] = carve(sizeof(int) * depths[k].size());
            o_ids[q] = carve(nodes && nodes[k] ? sizeof(int) * (size_t)counts[k] : 0);
        }
        c.img.assign(off, 0);
        char* d_img = nullptr;
        TRY(refine_multi_scratch(engines[c.first], off, &d_img));
        unsigned long long* keys = (unsigned long long*)(c.img.data() + o_keys);
        ConnectViaDesc* hd = (ConnectViaDesc*)(c.img.data() + o_desc);
        ProtoTable pt;
        memset(&pt, 0, sizeof pt);
        size_t lds = 0;
        std::vector<long long> grid_counts((size_t)m);
        for (int q = 0; q < m; ++q) {
            const int k = c.members[q];
            lqrrt_engine* e = engines[k];
            const bool listed = nodes && nodes[k];
            const size_t way_bytes = sizeof(double) * (size_t)Q[k] * e->n;
            keys[q] = (unsigned long long)incumbents[k] << 32;  // (incumbent, candidate 0): every candidate at its cost loses
            if (way_bytes) memcpy(c.img.data() + o_way[q], waypoints[k], way_bytes);
            memcpy(c.img.data() + o_depth[q], depths[k].data(), sizeof(int) * depths[k].size());
            if (listed) memcpy(c.img.data() + o_ids[q], nodes[k], sizeof(int) * (size_t)counts[k]);
            ConnectViaArgs& a = hd[q].a;
            connect_via_multi_args(e, (const double*)(d_img + o_way[q]), Q[k], tries[k], horizons[k], &a);
            a.depth = (const int*)(d_img + o_depth[q]);
            a.nodes = listed ? (const int*)(d_img + o_ids[q]) : nullptr;
            a.count = counts[k];
            hd[q].best = (unsigned long long*)(d_img + o_keys) + q;
            TRY(multi_sync_proto(e, st));
            pt.p[q] = e->d_proto;
            lds = std::max(lds, refine_lds_bytes(e, horizons[k]));
            grid_counts[q] = (long long)counts[k] * ((long long)Q[k] + 1);
        }
        RetainGrid gr;
        const unsigned grid = retain_grid(grid_counts, gr);
        HIPCHK(hipMemcpyAsync(d_img, c.img.data(), c.img.size(), hipMemcpyHostToDevice, st));
        DISPATCH(engines[0], hipLaunchKernelGGL((k_connect_via_search_multi<S>), dim3(grid), dim3(64), lds, st, pt,
                                                (const ConnectViaDesc*)(d_img + o_desc), gr));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(c.img.data(), d_img, sizeof(unsigned long long) * m, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    for (const ConnectViaChunk& c : chunks) {
        const unsigned long long* keys = (const unsigned long long*)c.img.data();
        for (size_t q = 0; q < c.members.size(); ++q) {
            const int k = c.members[q];
            if (keys[q] == (unsigned long long)incumbents[k] << 32) continue;
            const long long cand = (long long)(keys[q] & 0xffffffffull), pos = cand / ((long long)Q[k] + 1);
            cost[k] = (int64_t)(keys[q] >> 32);
            node_out[k] = nodes && nodes[k] ? nodes[k][pos] : (int32_t)pos;
            j_out[k] = (int32_t)(cand - pos * ((long long)Q[k] + 1));
        }
    }
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
        if (incumbents[k] < 1 || incumbents[k] > 0x7fffffffLL)
            return fail(LQRRT_E_ARG, "incumbent cost %lld out of range (engine %d)", (long long)incumbents[k], k);
        const bool listed = nodes && nodes[k];
        if (listed && !counts) return fail(LQRRT_E_ARG, "an id list without its count (engine %d)", k);
        cnt[k] = listed ? counts[k] : e->N;
        if (cnt[k] < 0) return fail(LQRRT_E_ARG, "negative candidate count (engine %d)", k);
        if ((long long)cnt[k] * ((long long)Q[k] + 1) > 0xffffffffLL / 64)
            return fail(LQRRT_E_ARG, "%d nodes with %d waypoints: %lld candidates exceed one launch (engine %d)", cnt[k], Q[k],
                        (long long)cnt[k] * ((long long)Q[k] + 1), k);
        if (listed)
            for (int c = 0; c < cnt[k]; ++c) {
                TRY(range_ok(e, nodes[k][c], 1));
                if (c > 0 && nodes[k][c] <= nodes[k][c - 1])
                    return fail(LQRRT_E_ARG, "the id list of engine %d is not strictly ascending at position %d", k, c);
            }
        depths[k].assign((size_t)e->N, 0);
        TRY(connect_depths(e, 0, horizon_iters[k], depths[k].data()));
        long long deepest = 0;                                  // the deepest candidate, with every target's edge at full length
        if (listed)
            for (int c = 0; c < cnt[k]; ++c) deepest = std::max(deepest, (long long)depths[k][(size_t)nodes[k][c]]);
        else
            for (int v = 0; v < e->N; ++v) deepest = std::max(deepest, (long long)depths[k][(size_t)v]);
        if (cnt[k] && deepest + ((long long)Q[k] + goal_tries[k]) * horizon_iters[k] > 0x7fffffffLL)
            return fail(LQRRT_E_ARG, "tree too deep for 32-bit step counts (engine %d)", k);
    }
    TRY(use_device(engines[0]));
    hipStream_t st = (hipStream_t)stream;
    for (int k = 0; k < n; ++k) { cost_out[k] = incumbents[k]; node_out[k] = -1; j_out[k] = -1; }
    std::vector<ConnectViaChunk> chunks;                        // (outlives every copy of the call, also when the call fails)
    const int rc = connect_via_search_multi_run(engines, n, nodes, cnt, depths, waypoints, Q, goal_tries, horizon_iters, incumbents, cost_out,
                                                node_out, j_out, st, chunks);
    return rc ? refine_multi_fail(rc, st) : 0;
}

static int connect_via_commit_multi_run(lqrrt_engine** engines, int n, const int32_t* nodes, const int32_t* cj,
                                        const std::vector<long long>& depth, const std::vector<int>& room, const double* const* waypoints,
                                        const int32_t* Q, const int32_t* tries, const int32_t* horizons, int32_t* const* ids_out,
                                        int32_t* counts_out, hipStream_t st, std::vector<ConnectViaChunk>& chunks) {
    for (int k = 0; k < n; ++k) {
        counts_out[k] = 0;
        if (nodes[k] < 0) continue;                             // (no winner: not part of the launch)
        if (chunks.empty() || (int)chunks.back().members.size() == MULTI_MAX) {
            chunks.emplace_back();
            chunks.back().first = k;
        }
        chunks.back().members.push_back(k);
    }
    for (ConnectViaChunk& c : chunks) {
        const int m = (int)c.members.size();
        size_t off = 0;
        auto carve = [&](size_t bytes) { const size_t at = off; off += (bytes + 15) / 16 * 16; return at; };
        c.o_out = carve(sizeof(int) * 4 * m);
        size_t sum_ids = 0;
        c.lens_at.assign((size_t)m, 0);
        for (int q = 0; q < m; ++q) { c.lens_at[q] = sum_ids; sum_ids += (size_t)room[c.members[q]]; }
        c.o_lens = carve(sizeof(int) * sum_ids);
        const size_t back = off;                                // what comes back: the outputs and the edge lengths
        const size_t o_desc = carve(sizeof(ConnectViaCommitDesc) * m);
        std::vector<size_t> o_way((size_t)m);
        for (int q = 0; q < m; ++q) o_way[q] = carve(sizeof(double) * (size_t)Q[c.members[q]] * engines[c.members[q]]->n);
        c.img.assign(off, 0);
        char* d_img = nullptr;
        TRY(refine_multi_scratch(engines[c.first], off, &d_img));
        ConnectViaCommitDesc* hd = (ConnectViaCommitDesc*)(c.img.data() + o_desc);
        ProtoTable pt;
        memset(&pt, 0, sizeof pt);
        size_t lds = 0;
        for (int q = 0; q < m; ++q) {
            const int k = c.members[q];
            lqrrt_engine* e = engines[k];
            const size_t way_bytes = sizeof(double) * (size_t)Q[k] * e->n;
            if (way_bytes) memcpy(c.img.data() + o_way[q], waypoints[k], way_bytes);
            connect_via_multi_args(e, (const double*)(d_img + o_way[q]), Q[k], tries[k], horizons[k], &hd[q].a);
            hd[q].out = (int*)(d_img + c.o_out) + 4 * q;
            hd[q].lens = (int*)(d_img + c.o_lens) + c.lens_at[q];
            hd[q].v = nodes[k]; hd[q].j = cj[k]; hd[q].depth = (int)depth[k]; hd[q].base = e->N;
            TRY(multi_sync_proto(e, st));
            pt.p[q] = e->d_proto;
            lds = std::max(lds, refine_lds_bytes(e, horizons[k]));
        }
        HIPCHK(hipMemcpyAsync(d_img, c.img.data(), c.img.size(), hipMemcpyHostToDevice, st));
        DISPATCH(engines[0], hipLaunchKernelGGL((k_connect_via_commit_multi<S>), dim3((unsigned)m), dim3(64), lds, st, pt,
                                                (const ConnectViaCommitDesc*)(d_img + o_desc), m));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(c.img.data(), d_img, back, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    for (const ConnectViaChunk& c : chunks) {
        const int* outs = (const int*)(c.img.data() + c.o_out);
        const int* lens = (const int*)(c.img.data() + c.o_lens);
        for (size_t q = 0; q < c.members.size(); ++q) {
            const int k = c.members[q];
            const int* out = outs + 4 * q;
            if (out[0] < 0) { counts_out[k] = LQRRT_E_CAPACITY; continue; }
            if (!out[2]) { counts_out[k] = LQRRT_E_STATE; continue; }      // (the chain does not reach the goal: nothing appended)
            refine_adopt(engines[k], nodes[k], out[0], lens + c.lens_at[q], ids_out[k]);
            counts_out[k] = out[0];
        }
    }
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
        lqrrt_engine* e = engines[k];
        TRY(range_ok(e, nodes[k], 1));
        if (j[k] < 0 || j[k] > Q[k]) return fail(LQRRT_E_ARG, "first waypoint %d outside [0, %d] (engine %d)", j[k], Q[k], k);
        const long long want = (long long)Q[k] - j[k] + goal_tries[k];
        if (!ids_out[k] || cap_ids[k] < want) return fail(LQRRT_E_ARG, "ids_out of engine %d must hold %lld ids", k, want);
        depth[k] = connect_depth_of(e, nodes[k]);
        if (depth[k] + want * horizon_iters[k] > 0x7fffffffLL)
            return fail(LQRRT_E_ARG, "tree too deep for 32-bit step counts (engine %d)", k);
        room[k] = (int)want;
    }
    TRY(use_device(engines[0]));
    hipStream_t st = (hipStream_t)stream;
    std::vector<ConnectViaChunk> chunks;                        // (outlives every copy of the call, also when the call fails)
    const int rc = connect_via_commit_multi_run(engines, n, nodes, j, depth, room, waypoints, Q, goal_tries, horizon_iters, ids_out, counts_out,
                                                st, chunks);
    return rc ? refine_multi_fail(rc, st) : 0;
}
