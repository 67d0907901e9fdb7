// ABI: one tree asked about many goals -- the search for T targets in one launch and the commit of one target's winner
// (Planner.goal_costs / Planner.retarget; kernel in reach.hpp, the rule restated from the C oracle's primitives in
// tests/reach_reference.py).  Fragment of engine.hip, behind engine_connect.hpp whose checks, depth table and candidates it uses.
//
// The rule: engine_connect.hpp's, with a target's goal state g_t and box lo_t < x < hi_t in place of the engine's own, for every
// target independently.  The engine's goal and box are read by neither call and written by neither.
//
// One image per search (engine_refine.hpp: the solo runner and its scratch), the 8-byte parts first: the head (the keys [T], 64
// bit), the target table [T] (ReachTarget: goal, lo, hi), the depth table [N], the id list [count].  The commit's image is the
// connect commit's.
// --------------------------------------------------------------------------------------------

// a target as the caller gave it: finite goal, lo <= hi in the model's dimensions
static int reach_target_check(const lqrrt_engine* e, const double* goal, const double* lo, const double* hi, int t) {
    for (int d = 0; d < e->n; ++d) {
        if (!std::isfinite(goal[d])) return fail(LQRRT_E_ARG, "goal %d is not finite", t);
        if (!(lo[d] <= hi[d])) return fail(LQRRT_E_ARG, "goal box %d is empty in dimension %d (lo > hi, or not a number)", t, d);
    }
    return 0;
}

// what the kernels read of a target; the dimensions beyond the model's are those of an engine without a goal
static void reach_target_fill(const lqrrt_engine* e, const double* goal, const double* lo, const double* hi, double* g_out,
                              double* lo_out, double* hi_out) {
    for (int d = 0; d < MAXN; ++d) {
        g_out[d] = d < e->n ? goal[d] : 0.0;
        lo_out[d] = d < e->n ? lo[d] : -INFINITY;
        hi_out[d] = d < e->n ? hi[d] : INFINITY;
    }
}

// the incumbent of target t: the caller's, or none (every reaching chain wins)
static long long reach_incumbent(const int64_t* incumbents, int t) { return incumbents ? (long long)incumbents[t] : 0x7fffffffLL; }

// the search's hooks (engine_refine.hpp: solo_search_run): a key per target
struct ReachSearchSolo : SoloCands {
    typedef ReachArgs Args;
    const double* goals; const double* lo; const double* hi;
    int T, tries, horizon; const int64_t* incumbents; int64_t* cost; int32_t* node_out;
    size_t bytes() const { return sizeof(ReachTarget) * (size_t)T + SoloCands::bytes(); }
    long long groups() const { return (long long)T * count; }
    int keys() const { return T; }
    int64_t incumbent(int t) const { return reach_incumbent(incumbents, t); }   // (incumbent, node 0)
    void fill(const lqrrt_engine* e, char* host, const char* dev, ReachArgs* a) const {
        ReachTarget* tab = (ReachTarget*)host;
        const size_t n = (size_t)e->n, o_cands = sizeof(ReachTarget) * (size_t)T;
        for (int t = 0; t < T; ++t) reach_target_fill(e, goals + t * n, lo + t * n, hi + t * n, tab[t].goal, tab[t].lo, tab[t].hi);
        a->targets = (const ReachTarget*)dev;
        a->T = T; a->tries = tries; a->H = horizon;
        stage(host + o_cands, dev + o_cands, a);
    }
    template <class S>
    static void launch(const lqrrt_engine* e, unsigned grid, size_t lds, hipStream_t st, const ReachArgs& a, unsigned long long* keys) {
        hipLaunchKernelGGL((k_reach_search<S>), dim3(grid), dim3(64), lds, st, e->P, e->geo, e->res, e->tv, a, keys);
    }
    void won(int t, unsigned long long key) const { connect_decode(key, &cost[t], &node_out[t]); }
};

extern "C" int lqrrt_reach_search(lqrrt_engine* e, const double* goals, const double* lo, const double* hi, int T,
                                  const int32_t* nodes_host, int count, int goal_tries, int horizon_iters, const int64_t* incumbents,
                                  int64_t* cost_out, int32_t* node_out, void* stream) {
    NOT_GENERIC(e);
    if (!e || !goals || !lo || !hi || !cost_out || !node_out) return fail(LQRRT_E_ARG, "null argument");
    if (T < 1 || T > 1024) return fail(LQRRT_E_ARG, "%d targets (1 to 1024 per call)", T);
    TRY(connect_check(e, goal_tries, horizon_iters));
    TRY(candidates_check(e, nodes_host, &count, T, -1, [&](int c) {
        return fail(LQRRT_E_ARG, "%d targets of %d candidates: %lld workgroups exceed one launch", T, c, (long long)T * c);
    }));
    const size_t n = (size_t)e->n;
    for (int t = 0; t < T; ++t) {
        const long long inc = reach_incumbent(incumbents, t);
        if (inc < 1 || inc > 0x7fffffffLL) return fail(LQRRT_E_ARG, "incumbent cost %lld of target %d out of range", inc, t);
        TRY(reach_target_check(e, goals + t * n, lo + t * n, hi + t * n, t));
    }
    ReachSearchSolo h{{std::vector<int>((size_t)e->N), nodes_host, count}, goals, lo, hi, T, goal_tries, horizon_iters, incumbents,
                      cost_out, node_out};
    TRY(connect_depths(e, goal_tries, horizon_iters, h.depth.data()));
    for (int t = 0; t < T; ++t) { cost_out[t] = reach_incumbent(incumbents, t); node_out[t] = -1; }
    return solo_search_run(e, horizon_iters, (hipStream_t)stream, h);
}

// lqrrt_connect_commit's replay (connect_commit_run) with the target as the chain's goal and a copy of the resolution block whose
// goal box is the target's
extern "C" int lqrrt_reach_commit(lqrrt_engine* e, const double* goal, const double* lo, const double* hi, int node, int goal_tries,
                                  int horizon_iters, int32_t* ids_out, int cap_ids, void* stream) {
    NOT_GENERIC(e);
    if (!e || !goal || !lo || !hi) return fail(LQRRT_E_ARG, "null argument");
    TRY(connect_check(e, goal_tries, horizon_iters));
    TRY(range_ok(e, node, 1));
    TRY(reach_target_check(e, goal, lo, hi, 0));
    double g[MAXN];
    Res res = e->res;
    reach_target_fill(e, goal, lo, hi, g, res.goal_lo, res.goal_hi);
    return connect_commit_run(e, node, goal_tries, horizon_iters, g, res, "target", ids_out, cap_ids, stream);
}
