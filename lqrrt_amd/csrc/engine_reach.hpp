// ABI: one tree asked about many goals -- the search for T targets in one launch and the commit of one target's winner
// (Planner.goal_costs / Planner.retarget; kernel in reach.hpp, the rule restated from the C oracle's primitives in
// tests/reach_reference.py).  Fragment of engine.hip, behind engine_connect.hpp whose checks, depth table and scratch it uses.
//
// The rule: engine_connect.hpp's, with a target's goal state g_t and box lo_t < x < hi_t in place of the engine's own, for every
// target independently.  The engine's goal and box are read by neither call and written by neither.
//
// One image per search in d_con, the 8-byte parts first: the keys [T] (64 bit), the target table [T] (ReachTarget: goal, lo, hi),
// the depth table [N], the id list [count].  One copy up, one launch, the T keys back in one copy.
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
    const int N = e->N, n = e->n;
    for (int t = 0; t < T; ++t) {
        const long long inc = incumbents ? (long long)incumbents[t] : 0x7fffffffLL;
        if (inc < 1 || inc > 0x7fffffffLL) return fail(LQRRT_E_ARG, "incumbent cost %lld of target %d out of range", inc, t);
        TRY(reach_target_check(e, goals + (size_t)t * n, lo + (size_t)t * n, hi + (size_t)t * n, t));
    }
    // the image of the call: keys [T], targets [T], depth [N], candidate ids [count]
    const size_t o_tab = sizeof(unsigned long long) * (size_t)T, o_depth = o_tab + sizeof(ReachTarget) * (size_t)T;
    const size_t o_ids = o_depth + sizeof(int) * (size_t)N;
    std::vector<unsigned long long> img((o_ids + sizeof(int) * (size_t)(nodes_host ? count : 0) + 7) / 8, 0);
    char* base = (char*)img.data();
    TRY(connect_depths(e, goal_tries, horizon_iters, (int*)(base + o_depth)));
    if (nodes_host && count) memcpy(base + o_ids, nodes_host, sizeof(int) * (size_t)count);
    ReachTarget* tab = (ReachTarget*)(base + o_tab);
    for (int t = 0; t < T; ++t) {
        cost_out[t] = incumbents ? incumbents[t] : 0x7fffffffLL;
        node_out[t] = -1;
        img[(size_t)t] = incumbent_key(cost_out[t]);             // (incumbent, node 0)
        reach_target_fill(e, goals + (size_t)t * n, lo + (size_t)t * n, hi + (size_t)t * n, tab[t].goal, tab[t].lo, tab[t].hi);
    }
    if (count == 0) return 0;
    TRY(use_device(e));
    hipStream_t st = (hipStream_t)stream;
    TRY(connect_scratch(e, img.size() * 2));                    // (the scratch counts ints behind its head of 8; the image starts at the head)
    std::vector<unsigned long long> keys((size_t)T);
    StreamDrain drain(st);                                      // (img is the source of a copy, keys the target of one)
    char* d_img = (char*)e->d_con;
    drain.arm();
    HIPCHK(hipMemcpyAsync(d_img, base, sizeof(unsigned long long) * img.size(), hipMemcpyHostToDevice, st));
    ReachArgs a;
    a.targets = (const ReachTarget*)(d_img + o_tab);
    a.depth = (const int*)(d_img + o_depth);
    a.nodes = nodes_host ? (const int*)(d_img + o_ids) : nullptr;
    a.T = T; a.count = count; a.tries = goal_tries; a.H = horizon_iters;
    unsigned long long* d_keys = (unsigned long long*)d_img;
    const unsigned grid = (unsigned)((long long)T * count);
    DISPATCH(e, hipLaunchKernelGGL((k_reach_search<S>), dim3(grid), dim3(64), refine_lds_bytes(e, horizon_iters), st, e->P, e->geo, e->res,
                                   e->tv, a, d_keys));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(keys.data(), d_keys, sizeof(unsigned long long) * (size_t)T, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    drain.disarm();
    for (int t = 0; t < T; ++t) {
        if (keys[(size_t)t] == img[(size_t)t]) continue;
        cost_out[t] = (int64_t)(keys[(size_t)t] >> 32);
        node_out[t] = (int32_t)(keys[(size_t)t] & 0xffffffffull);
    }
    return 0;
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
