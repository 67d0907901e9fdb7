// ABI: several trees asked about many goals per call -- lqrrt_reach_search_multi / lqrrt_reach_commit_multi (fleet_goal_costs /
// retargets; kernels in reach_multi.hpp).  Fragment of engine.hip, behind engine_reach.hpp whose target checks and fill it uses.
// Every argument of every engine and of every target is checked, with the one-engine calls' own checkers, before anything is
// written or launched.  The calls run on engine_refine.hpp's multi path: its engine-list check, chunks, scratch (d_refm: not part
// of the footprint), prototypes, grid, commit head and guard.
// A search's image per chunk: ALL keys first -- T_k per member, member by member; only they come back --, then a ReachDesc per
// member, then per member its ReachTarget table [T_k], its depth table and its id list.  Member k occupies T_k * count_k
// workgroups of the chunk's one launch.  A commit's image per chunk of up to MULTI_MAX winners: every engine's out[3] and edge
// lengths (what comes back), then a ReachCommitDesc per engine and its one-node plan [v | depth[v]]; one workgroup per winner.
// --------------------------------------------------------------------------------------------

// what the two calls check alike, for every engine, behind the engine-list check
static int reach_multi_check(lqrrt_engine** engines, int n, bool args, const int32_t* tries, const int32_t* horizons) {
    return multi_engines_check(engines, n, args && tries && horizons, [&](int k) { return connect_check(engines[k], tries[k], horizons[k]); });
}

static int reach_search_multi_run(lqrrt_engine** engines, int n, const double* const* goals, const double* const* lo,
                                  const double* const* hi, const int32_t* T, const int32_t* const* nodes, const std::vector<int>& counts,
                                  const std::vector<std::vector<int>>& depths, const int32_t* tries, const int32_t* horizons,
                                  int64_t* const* cost, int32_t* const* node_out, hipStream_t st) {
    // cost[k][t] holds target t's incumbent on entry (node_out -1) and its winner's cost on exit
    std::vector<long long> groups((size_t)n);                   // (an empty id list: no launch, no winner)
    for (int k = 0; k < n; ++k) groups[k] = (long long)T[k] * counts[k];
    std::vector<MultiChunk> chunks = multi_chunks(groups);
    std::vector<std::vector<size_t>> key_at(chunks.size());     // per chunk and member: its first key
    StreamDrain drain(st);
    for (size_t ci = 0; ci < chunks.size(); ++ci) {
        MultiChunk& c = chunks[ci];
        const int m = (int)c.members.size();
        size_t n_keys = 0;
        key_at[ci].assign((size_t)m, 0);
        for (int q = 0; q < m; ++q) { key_at[ci][q] = n_keys; n_keys += (size_t)T[c.members[q]]; }
        Carve carve;
        carve(sizeof(unsigned long long) * n_keys);             // the keys
        const size_t o_desc = carve(sizeof(ReachDesc) * m);
        std::vector<size_t> o_tab((size_t)m), o_depth((size_t)m), o_ids((size_t)m);
        for (int q = 0; q < m; ++q) {
            const int k = c.members[q];
            o_tab[q] = carve(sizeof(ReachTarget) * (size_t)T[k]);
            o_depth[q] = carve(sizeof(int) * depths[k].size());
            o_ids[q] = carve(nodes && nodes[k] ? sizeof(int) * (size_t)counts[k] : 0);
        }
        c.img.assign(carve.off, 0);
        char* d_img = nullptr;
        TRY(refine_multi_scratch(engines[c.first], carve.off, &d_img));
        ReachDesc* hd = (ReachDesc*)(c.img.data() + o_desc);
        for (int q = 0; q < m; ++q) {
            const int k = c.members[q];
            const lqrrt_engine* e = engines[k];
            const bool listed = nodes && nodes[k];
            const size_t ns = (size_t)e->n;
            unsigned long long* keys = (unsigned long long*)c.img.data() + key_at[ci][q];
            ReachTarget* tab = (ReachTarget*)(c.img.data() + o_tab[q]);
            for (int t = 0; t < T[k]; ++t) {
                keys[t] = incumbent_key(cost[k][t]);            // (incumbent, node 0)
                reach_target_fill(e, goals[k] + t * ns, lo[k] + t * ns, hi[k] + t * ns, tab[t].goal, tab[t].lo, tab[t].hi);
            }
            memcpy(c.img.data() + o_depth[q], depths[k].data(), sizeof(int) * depths[k].size());
            if (listed) memcpy(c.img.data() + o_ids[q], nodes[k], sizeof(int) * (size_t)counts[k]);
            ReachArgs& a = hd[q].a;
            a.targets = (const ReachTarget*)(d_img + o_tab[q]);
            a.depth = (const int*)(d_img + o_depth[q]);
            a.nodes = listed ? (const int*)(d_img + o_ids[q]) : nullptr;
            a.T = T[k]; a.count = counts[k]; a.tries = tries[k]; a.H = horizons[k];
            hd[q].keys = (unsigned long long*)d_img + key_at[ci][q];
        }
        ProtoTable pt;
        size_t lds = 0;
        TRY(refine_multi_protos(engines, c, horizons, st, pt, lds));
        RetainGrid gr;
        const unsigned grid = multi_grid(c, groups, gr);
        drain.arm();
        HIPCHK(hipMemcpyAsync(d_img, c.img.data(), c.img.size(), hipMemcpyHostToDevice, st));
        DISPATCH(engines[0], hipLaunchKernelGGL((k_reach_search_multi<S>), dim3(grid), dim3(64), lds, st, pt,
                                                (const ReachDesc*)(d_img + o_desc), gr));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(c.img.data(), d_img, sizeof(unsigned long long) * n_keys, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));                           // the call's one synchronise
    drain.disarm();
    for (size_t ci = 0; ci < chunks.size(); ++ci) {
        const MultiChunk& c = chunks[ci];
        for (size_t q = 0; q < c.members.size(); ++q) {
            const int k = c.members[q];
            const unsigned long long* keys = (const unsigned long long*)c.img.data() + key_at[ci][q];
            for (int t = 0; t < T[k]; ++t) {
                if (keys[t] == incumbent_key(cost[k][t])) continue;   // (cost holds the incumbent until a winner replaces it)
                cost[k][t] = (int64_t)(keys[t] >> 32);
                node_out[k][t] = (int32_t)(keys[t] & 0xffffffffull);
            }
        }
    }
    return 0;
}

extern "C" int lqrrt_reach_search_multi(lqrrt_engine** engines, int n, const double* const* goals, const double* const* lo,
                                        const double* const* hi, const int32_t* T, const int32_t* const* nodes, const int32_t* counts,
                                        const int32_t* goal_tries, const int32_t* horizon_iters, const int64_t* const* incumbents,
                                        int64_t* const* cost_out, int32_t* const* node_out, void* stream) {
    TRY(reach_multi_check(engines, n, goals && lo && hi && T && cost_out && node_out, goal_tries, horizon_iters));
    std::vector<int> cnt((size_t)n);
    std::vector<std::vector<int>> depths((size_t)n);
    for (int k = 0; k < n; ++k) {
        lqrrt_engine* e = engines[k];
        const int32_t* ids = nullptr;
        if (T[k] < 1 || T[k] > 1024) return fail(LQRRT_E_ARG, "%d targets (1 to 1024 per engine) (engine %d)", T[k], k);
        if (!goals[k] || !lo[k] || !hi[k] || !cost_out[k] || !node_out[k]) return fail(LQRRT_E_ARG, "null argument (engine %d)", k);
        TRY(multi_id_list(nodes, counts, k, &ids, &cnt[k]));
        TRY(candidates_check(e, ids, &cnt[k], T[k], k, [&](int c) {
            return fail(LQRRT_E_ARG, "%d targets of %d candidates: %lld workgroups exceed one launch (engine %d)", T[k], c,
                        (long long)T[k] * c, k);
        }));
        const size_t ns = (size_t)e->n;
        for (int t = 0; t < T[k]; ++t) {
            const long long inc = incumbents && incumbents[k] ? (long long)incumbents[k][t] : 0x7fffffffLL;
            if (inc < 1 || inc > 0x7fffffffLL)
                return fail(LQRRT_E_ARG, "incumbent cost %lld of target %d out of range (engine %d)", inc, t, k);
            TRY(reach_target_check(e, goals[k] + t * ns, lo[k] + t * ns, hi[k] + t * ns, t));
        }
        depths[k].assign((size_t)e->N, 0);
        TRY(connect_depths(e, goal_tries[k], horizon_iters[k], depths[k].data()));
    }
    TRY(use_device(engines[0]));
    for (int k = 0; k < n; ++k)
        for (int t = 0; t < T[k]; ++t) {
            cost_out[k][t] = incumbents && incumbents[k] ? incumbents[k][t] : 0x7fffffffLL;
            node_out[k][t] = -1;
        }
    return reach_search_multi_run(engines, n, goals, lo, hi, T, nodes, cnt, depths, goal_tries, horizon_iters, cost_out, node_out,
                                  (hipStream_t)stream);
}

static int reach_commit_multi_run(lqrrt_engine** engines, int n, const double* const* goal, const double* const* lo,
                                  const double* const* hi, const int32_t* nodes, const std::vector<long long>& depth, const int32_t* tries,
                                  const int32_t* horizons, int32_t* const* ids_out, int32_t* counts_out, hipStream_t st) {
    std::vector<int> room((size_t)n, 0);
    std::vector<long long> winner((size_t)n, 0);
    for (int k = 0; k < n; ++k) {
        counts_out[k] = 0;
        if (nodes[k] < 0) continue;                             // (no winner: not part of the launch)
        room[k] = tries[k];
        winner[k] = 1;
    }
    std::vector<MultiChunk> chunks = multi_chunks(winner);
    StreamDrain drain(st);
    for (MultiChunk& c : chunks) {
        const int m = (int)c.members.size();
        Carve carve;
        multi_commit_head(c, room, carve);
        const size_t o_desc = carve(sizeof(ReachCommitDesc) * m);
        const size_t o_plan = carve(sizeof(int) * 2 * m);       // per member the one-node plan [v] and its cost prefix [depth[v]]
        c.img.assign(carve.off, 0);
        char* d_img = nullptr;
        TRY(refine_multi_scratch(engines[c.first], carve.off, &d_img));
        ReachCommitDesc* hd = (ReachCommitDesc*)(c.img.data() + o_desc);
        for (int q = 0; q < m; ++q) {
            const int k = c.members[q];
            const lqrrt_engine* e = engines[k];
            int* plan = (int*)(c.img.data() + o_plan) + 2 * q;
            plan[0] = nodes[k]; plan[1] = (int)depth[k];
            refine_fill_args(e, (const int*)(d_img + o_plan) + 2 * q, 1, tries[k], horizons[k], &hd[q].a);
            hd[q].r = e->res;                                   // as lqrrt_reach_commit: the engine's block, the target's box
            reach_target_fill(e, goal[k], lo[k], hi[k], hd[q].a.goal, hd[q].r.goal_lo, hd[q].r.goal_hi);
            hd[q].out = c.out_of(d_img, q);
            hd[q].lens = c.lens_of(d_img, q);
            hd[q].i = hd[q].j = 0; hd[q].base = e->N; hd[q].pad = 0;
        }
        ProtoTable pt;
        size_t lds = 0;
        TRY(refine_multi_protos(engines, c, horizons, st, pt, lds));
        drain.arm();
        HIPCHK(hipMemcpyAsync(d_img, c.img.data(), c.img.size(), hipMemcpyHostToDevice, st));
        DISPATCH(engines[0], hipLaunchKernelGGL((k_reach_commit_multi<S>), dim3((unsigned)m), dim3(64), lds, st, pt,
                                                (const ReachCommitDesc*)(d_img + o_desc), m));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(c.img.data(), d_img, c.back, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    drain.disarm();
    multi_commit_adopt(engines, chunks, std::vector<int>(nodes, nodes + n), ids_out, counts_out);
    return 0;
}

extern "C" int lqrrt_reach_commit_multi(lqrrt_engine** engines, int n, const double* const* goal, const double* const* lo,
                                        const double* const* hi, const int32_t* nodes, const int32_t* goal_tries,
                                        const int32_t* horizon_iters, int32_t* const* ids_out, const int32_t* cap_ids, int32_t* counts_out,
                                        void* stream) {
    TRY(reach_multi_check(engines, n, goal && lo && hi && nodes && ids_out && cap_ids && counts_out, goal_tries, horizon_iters));
    std::vector<long long> depth((size_t)n, 0);
    for (int k = 0; k < n; ++k) {
        if (nodes[k] == -1) continue;                           // an engine without a winner
        if (!goal[k] || !lo[k] || !hi[k]) return fail(LQRRT_E_ARG, "null argument (engine %d)", k);
        TRY(range_ok(engines[k], nodes[k], 1));
        TRY(connect_winner_check(engines[k], nodes[k], goal_tries[k], horizon_iters[k], ids_out[k], cap_ids[k], k, &depth[k]));
        TRY(reach_target_check(engines[k], goal[k], lo[k], hi[k], 0));
    }
    TRY(use_device(engines[0]));
    return reach_commit_multi_run(engines, n, goal, lo, hi, nodes, depth, goal_tries, horizon_iters, ids_out, counts_out,
                                  (hipStream_t)stream);
}
