// ABI: goal chains through waypoints for several trees per call -- lqrrt_connect_via_search_multi / lqrrt_connect_via_commit_multi
// (connect_vias; kernels in connect_via_multi.hpp).  Fragment of engine.hip, behind engine_connect_via.hpp.  Every argument of every
// engine is checked, with the one-engine calls' own checkers, before anything is written or launched.  The calls run on
// engine_refine.hpp's two runners (multi_search_run, multi_commit_run: the chunks, the scratch d_refm, the prototypes, the keys, the
// commit head, the guard and the one synchronise are theirs) and state their hooks here.  A search's tables behind its
// ConnectViaDescs: every engine's waypoints (8-byte aligned: Carve rounds to 16), depth table and id list (engine_connect.hpp:
// MultiCands).  A commit's behind its ConnectViaCommitDescs: the waypoints; one workgroup per winner.
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

// what the hooks of the two calls share: a member's waypoints in the image, and the argument block of its chains over them
struct ConnectViaMulti {
    lqrrt_engine** engines;
    const double* const* waypoints;
    const int32_t* Q; const int32_t* tries; const int32_t* horizons;
    size_t carve_way(int k, Carve& carve) const { return carve(sizeof(double) * (size_t)Q[k] * engines[k]->n); }
    void stage_way(int k, size_t o_way, MultiChunk& c, ConnectViaArgs* a) const {
        if (Q[k]) memcpy(c.img.data() + o_way, waypoints[k], sizeof(double) * (size_t)Q[k] * engines[k]->n);
        connect_via_fill_args(engines[k], (const double*)(c.dev + o_way), Q[k], tries[k], horizons[k], a);
    }
};

struct ConnectViaSearchMulti : ConnectViaMulti {
    typedef ConnectViaDesc Desc;
    struct Part { size_t way; MultiCands::At cands; };
    const MultiCands& x;
    const int64_t* incumbents; int64_t* cost; int32_t* node_out; int32_t* j_out;
    long long groups(int k) const { return (long long)x.counts[k] * ((long long)Q[k] + 1); }
    int keys(int) const { return 1; }
    int64_t incumbent(int k, int) const { return incumbents[k]; }   // (incumbent, candidate 0)
    Part carve(const MultiChunk& c, size_t q, Carve& carve) const {
        const size_t o_way = carve_way(c.members[q], carve);
        return {o_way, x.carve(c.members[q], carve)};
    }
    void fill(MultiChunk& c, size_t q, const std::vector<Part>& at, ConnectViaDesc* d) const {
        stage_way(c.members[q], at[q].way, c, &d->a);
        x.stage(c.members[q], at[q].cands, c, &d->a);
        d->best = c.keys_of(c.dev, q);
    }
    template <class S>
    static void launch(unsigned grid, size_t lds, hipStream_t st, const ProtoTable& pt, const ConnectViaDesc* ds, const RetainGrid& gr) {
        hipLaunchKernelGGL((k_connect_via_search_multi<S>), dim3(grid), dim3(64), lds, st, pt, ds, gr);
    }
    void won(int k, int, unsigned long long key) const { connect_via_decode(key, x.ids[k], Q[k], &cost[k], &node_out[k], &j_out[k]); }
};

extern "C" int lqrrt_connect_via_search_multi(lqrrt_engine** engines, int n, const int32_t* const* nodes, const int32_t* counts,
                                              const double* const* waypoints, const int32_t* Q, const int32_t* goal_tries,
                                              const int32_t* horizon_iters, const int64_t* incumbents, int64_t* cost_out,
                                              int32_t* node_out, int32_t* j_out, void* stream) {
    TRY(connect_via_multi_check(engines, n, waypoints, Q, goal_tries, horizon_iters));
    if (!incumbents || !cost_out || !node_out || !j_out) return fail(LQRRT_E_ARG, "null argument");
    MultiCands x(n);
    for (int k = 0; k < n; ++k) {
        lqrrt_engine* e = engines[k];
        TRY(incumbent_check(incumbents[k], k));
        TRY(multi_id_list(nodes, counts, k, &x.ids[k], &x.counts[k]));
        TRY(connect_via_candidates_check(e, x.ids[k], &x.counts[k], Q[k], k));
        x.depths[k].assign((size_t)e->N, 0);
        TRY(connect_depths(e, 0, horizon_iters[k], x.depths[k].data()));
        TRY(connect_via_deepest_check(x.depths[k].data(), e->N, x.ids[k], x.counts[k], Q[k], goal_tries[k], horizon_iters[k], k));
    }
    TRY(use_device(engines[0]));
    for (int k = 0; k < n; ++k) { cost_out[k] = incumbents[k]; node_out[k] = -1; j_out[k] = -1; }
    return multi_search_run(engines, n, horizon_iters, (hipStream_t)stream,
                            ConnectViaSearchMulti{{engines, waypoints, Q, goal_tries, horizon_iters}, x, incumbents, cost_out, node_out, j_out});
}

struct ConnectViaCommitMulti : ConnectViaMulti {
    typedef ConnectViaCommitDesc Desc;
    typedef size_t Part;                                        // where the member's waypoints lie
    const int32_t* nodes; const int32_t* cj;
    const std::vector<long long>& depth;
    const std::vector<int>& rooms;
    bool winner(int k) const { return nodes[k] >= 0; }
    int room(int k) const { return rooms[k]; }
    int parent(int k) const { return nodes[k]; }
    size_t carve(const MultiChunk& c, size_t q, Carve& carve) const { return carve_way(c.members[q], carve); }
    void fill(MultiChunk& c, size_t q, const std::vector<size_t>& at, ConnectViaCommitDesc* d) const {
        const int k = c.members[q];
        stage_way(k, at[q], c, &d->a);
        d->v = nodes[k]; d->j = cj[k]; d->depth = (int)depth[k];
    }
    template <class S>
    static void launch(unsigned m, size_t lds, hipStream_t st, const ProtoTable& pt, const ConnectViaCommitDesc* ds) {
        hipLaunchKernelGGL((k_connect_via_commit_multi<S>), dim3(m), dim3(64), lds, st, pt, ds, (int)m);
    }
};

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
    return multi_commit_run(engines, n, horizon_iters, ids_out, counts_out, (hipStream_t)stream,
                            ConnectViaCommitMulti{{engines, waypoints, Q, goal_tries, horizon_iters}, nodes, j, depth, room});
}
