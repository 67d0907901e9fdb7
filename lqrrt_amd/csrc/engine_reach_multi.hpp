// ABI: several trees asked about many goals per call -- lqrrt_reach_search_multi / lqrrt_reach_commit_multi (fleet_goal_costs /
// retargets; kernels in reach_multi.hpp).  Fragment of engine.hip, behind engine_reach.hpp whose target checks and fill it uses.
// Every argument of every engine and of every target is checked, with the one-engine calls' own checkers, before anything is
// written or launched.  The calls run on engine_refine.hpp's engine-list check and its two runners (multi_search_run,
// multi_commit_run: the chunks, the scratch d_refm, the prototypes, the grid, the commit head, the guard and the one synchronise
// are theirs) and state their hooks here.
// A search asks for T_k keys per member (ALL keys lie first in a chunk's image, member by member; only they come back) and
// T_k * count_k workgroups of the chunk's one launch; behind its ReachDescs lie per member its ReachTarget table [T_k], its depth
// table and its id list (engine_connect.hpp: MultiCands).  A commit's tables behind its ReachCommitDescs: per winner its one-node
// plan [v | depth[v]]; one workgroup per winner.
// --------------------------------------------------------------------------------------------

// what the two calls check alike, for every engine, behind the engine-list check
static int reach_multi_check(lqrrt_engine** engines, int n, bool args, const int32_t* tries, const int32_t* horizons) {
    return multi_engines_check(engines, n, args && tries && horizons, [&](int k) { return connect_check(engines[k], tries[k], horizons[k]); });
}

struct ReachSearchMulti {
    typedef ReachDesc Desc;
    struct Part { size_t tab; MultiCands::At cands; };
    const MultiCands& x;
    lqrrt_engine** engines;
    const double* const* goals; const double* const* lo; const double* const* hi;
    const int32_t* T; const int32_t* tries; const int32_t* horizons;
    int64_t* const* cost; int32_t* const* node_out;             // cost[k][t]: target t's incumbent on entry, its winner's cost on exit
    long long groups(int k) const { return (long long)T[k] * x.counts[k]; }
    int keys(int k) const { return T[k]; }
    int64_t incumbent(int k, int t) const { return cost[k][t]; }    // (incumbent, node 0; cost holds it until a winner replaces it)
    Part carve(const MultiChunk& c, size_t q, Carve& carve) const {
        const size_t o_tab = carve(sizeof(ReachTarget) * (size_t)T[c.members[q]]);
        return {o_tab, x.carve(c.members[q], carve)};
    }
    void fill(MultiChunk& c, size_t q, const std::vector<Part>& at, ReachDesc* d) const {
        const int k = c.members[q];
        const lqrrt_engine* e = engines[k];
        const size_t ns = (size_t)e->n;
        ReachTarget* tab = (ReachTarget*)(c.img.data() + at[q].tab);
        for (int t = 0; t < T[k]; ++t) reach_target_fill(e, goals[k] + t * ns, lo[k] + t * ns, hi[k] + t * ns, tab[t].goal, tab[t].lo, tab[t].hi);
        ReachArgs& a = d->a;
        a.targets = (const ReachTarget*)(c.dev + at[q].tab);
        x.stage(k, at[q].cands, c, &a);
        a.T = T[k]; a.tries = tries[k]; a.H = horizons[k];
        d->keys = c.keys_of(c.dev, q);
    }
    template <class S>
    static void launch(unsigned grid, size_t lds, hipStream_t st, const ProtoTable& pt, const ReachDesc* ds, const RetainGrid& gr) {
        hipLaunchKernelGGL((k_reach_search_multi<S>), dim3(grid), dim3(64), lds, st, pt, ds, gr);
    }
    void won(int k, int t, unsigned long long key) const {
        cost[k][t] = (int64_t)(key >> 32);
        node_out[k][t] = (int32_t)(key & 0xffffffffull);
    }
};

extern "C" int lqrrt_reach_search_multi(lqrrt_engine** engines, int n, const double* const* goals, const double* const* lo,
                                        const double* const* hi, const int32_t* T, const int32_t* const* nodes, const int32_t* counts,
                                        const int32_t* goal_tries, const int32_t* horizon_iters, const int64_t* const* incumbents,
                                        int64_t* const* cost_out, int32_t* const* node_out, void* stream) {
    TRY(reach_multi_check(engines, n, goals && lo && hi && T && cost_out && node_out, goal_tries, horizon_iters));
    MultiCands x(n);
    for (int k = 0; k < n; ++k) {
        lqrrt_engine* e = engines[k];
        if (T[k] < 1 || T[k] > 1024) return fail(LQRRT_E_ARG, "%d targets (1 to 1024 per engine) (engine %d)", T[k], k);
        if (!goals[k] || !lo[k] || !hi[k] || !cost_out[k] || !node_out[k]) return fail(LQRRT_E_ARG, "null argument (engine %d)", k);
        TRY(multi_id_list(nodes, counts, k, &x.ids[k], &x.counts[k]));
        TRY(candidates_check(e, x.ids[k], &x.counts[k], T[k], k, [&](int c) {
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
        x.depths[k].assign((size_t)e->N, 0);
        TRY(connect_depths(e, goal_tries[k], horizon_iters[k], x.depths[k].data()));
    }
    TRY(use_device(engines[0]));
    for (int k = 0; k < n; ++k)
        for (int t = 0; t < T[k]; ++t) {
            cost_out[k][t] = incumbents && incumbents[k] ? incumbents[k][t] : 0x7fffffffLL;
            node_out[k][t] = -1;
        }
    return multi_search_run(engines, n, horizon_iters, (hipStream_t)stream,
                            ReachSearchMulti{x, engines, goals, lo, hi, T, goal_tries, horizon_iters, cost_out, node_out});
}

struct ReachCommitMulti {
    typedef ReachCommitDesc Desc;
    typedef size_t Part;
    lqrrt_engine** engines;
    const double* const* goal; const double* const* lo; const double* const* hi;
    const int32_t* nodes;
    const std::vector<long long>& depth;
    const int32_t* tries; const int32_t* horizons;
    bool winner(int k) const { return nodes[k] >= 0; }
    int room(int k) const { return tries[k]; }
    int parent(int k) const { return nodes[k]; }
    // per member the one-node plan [v] and its cost prefix [depth[v]]: one part for the chunk, carved with its first member
    size_t carve(const MultiChunk& c, size_t q, Carve& carve) const { return q ? 0 : carve(sizeof(int) * 2 * c.members.size()); }
    void fill(MultiChunk& c, size_t q, const std::vector<size_t>& at, ReachCommitDesc* d) const {
        const int k = c.members[q];
        const lqrrt_engine* e = engines[k];
        const size_t o_plan = at[0] + sizeof(int) * 2 * q;
        int* plan = (int*)(c.img.data() + o_plan);
        plan[0] = nodes[k]; plan[1] = (int)depth[k];
        refine_fill_args(e, (const int*)(c.dev + o_plan), 1, tries[k], horizons[k], &d->a);
        d->r = e->res;                                          // as lqrrt_reach_commit: the engine's block, the target's box
        reach_target_fill(e, goal[k], lo[k], hi[k], d->a.goal, d->r.goal_lo, d->r.goal_hi);
        d->i = d->j = 0;
    }
    template <class S>
    static void launch(unsigned m, size_t lds, hipStream_t st, const ProtoTable& pt, const ReachCommitDesc* ds) {
        hipLaunchKernelGGL((k_reach_commit_multi<S>), dim3(m), dim3(64), lds, st, pt, ds, (int)m);
    }
};

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
    return multi_commit_run(engines, n, horizon_iters, ids_out, counts_out, (hipStream_t)stream,
                            ReachCommitMulti{engines, goal, lo, hi, nodes, depth, goal_tries, horizon_iters});
}
