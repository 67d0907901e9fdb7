// ABI: plan refinement -- the shortcut search over a found plan and the commit of its winner (Planner.refine_plan; kernels in
// refine.hpp, the rule restated from the C oracle's primitives in tests/refine_reference.py).  Fragment of engine.hip.
// --------------------------------------------------------------------------------------------

// Checks a plan (a parent chain from the root) and uploads its ids and cost prefix; `buf` holds the host copy until the caller
// has synchronised the stream.
static int refine_prepare(lqrrt_engine* e, const int32_t* plan, int P, int tries, int horizon, std::vector<int>& buf, RefineArgs* a,
                          hipStream_t st) {
    if (!plan || P < 1) return fail(LQRRT_E_ARG, "empty plan");
    if (P > 65535) return fail(LQRRT_E_ARG, "plan of %d nodes (at most 65535)", P);
    if (tries < 0) return fail(LQRRT_E_ARG, "goal_tries must be >= 0");
    if (!e->has_res || !e->has_goal) return fail(LQRRT_E_STATE, "set_resolution with a goal first");
    if (horizon < 1 || horizon > e->H) return fail(LQRRT_E_ARG, "horizon of %d steps (the edge pools hold %d)", horizon, e->H);
    if (plan[0] != 0) return fail(LQRRT_E_ARG, "a plan starts at the root (node 0), not at node %d", plan[0]);
    buf.assign((size_t)2 * P, 0);
    long long cost = 0;
    for (int k = 0; k < P; ++k) {
        TRY(range_ok(e, plan[k], 1));
        if (k > 0 && e->h_pid[(size_t)plan[k]] != plan[k - 1])
            return fail(LQRRT_E_ARG, "node %d of the plan is not a child of node %d", plan[k], plan[k - 1]);
        cost += k > 0 ? e->h_elen[(size_t)plan[k]] : 1;
        buf[k] = plan[k];
        buf[(size_t)P + k] = (int)cost;
    }
    if (cost + (long long)(P + tries) * horizon > 0x7fffffffLL) return fail(LQRRT_E_ARG, "plan too long for 32-bit step counts");
    if (P > e->ref_cap) {
        const size_t keep = g_dalloc_bytes;
        if (e->d_ref) (void)hipFree(e->d_ref);
        e->ref_cap = 0;
        int rc = dalloc(&e->d_ref, (size_t)2 * P);
        if (!rc && !e->d_ref_key) rc = dalloc(&e->d_ref_key, (size_t)4);
        g_dalloc_bytes = keep;                                  // (a few kB, allocated on first use: not part of the footprint)
        if (rc) return rc;
        e->ref_cap = P;
    }
    HIPCHK(hipMemcpyAsync(e->d_ref, buf.data(), sizeof(int) * buf.size(), hipMemcpyHostToDevice, st));
    a->plan = e->d_ref;
    a->prefix = e->d_ref + P;
    a->P = P; a->tries = tries; a->H = horizon; a->pad = 0;
    for (int d = 0; d < MAXN; ++d) a->goal[d] = d < e->n ? e->goal[d] : 0.0;
    return 0;
}

static size_t refine_lds_bytes(const lqrrt_engine* e, int horizon) {
    return geo_lds_bytes(e) + ((size_t)horizon * (e->n + e->m) + e->n + 2 * e->nw + (size_t)e->m * e->n) * sizeof(double);
}

extern "C" int lqrrt_refine_search(lqrrt_engine* e, const int32_t* plan_host, int P, int goal_tries, int horizon_iters,
                                   int64_t incumbent, int64_t* cost, int32_t* i_out, int32_t* j_out, void* stream) {
    NOT_GENERIC(e);
    if (!e || !cost || !i_out || !j_out) return fail(LQRRT_E_ARG, "null argument");
    if (incumbent < 1 || incumbent > 0x7fffffffLL) return fail(LQRRT_E_ARG, "incumbent cost %lld out of range", (long long)incumbent);
    TRY(use_device(e));
    hipStream_t st = (hipStream_t)stream;
    std::vector<int> buf;
    RefineArgs a;
    TRY(refine_prepare(e, plan_host, P, goal_tries, horizon_iters, buf, &a, st));
    *cost = incumbent; *i_out = -1; *j_out = -1;
    const unsigned long long init = (unsigned long long)incumbent << 32;   // (incumbent, 0, 0): every candidate at its cost loses
    unsigned long long key = init;
    if (P >= 2) {
        // one 64-thread workgroup per candidate: the grid's thread count must stay below 2^32
        if ((long long)P * (P - 1) / 2 * 64 > 0xffffffffLL)
            return fail(LQRRT_E_ARG, "plan of %d nodes: %lld candidates exceed one launch (at most 11586 nodes)", P, (long long)P * (P - 1) / 2);
        HIPCHK(hipMemcpyAsync(e->d_ref_key, &init, sizeof init, hipMemcpyHostToDevice, st));
        const unsigned ncand = (unsigned)((long long)P * (P - 1) / 2);
        DISPATCH(e, hipLaunchKernelGGL((k_refine_search<S>), dim3(ncand), dim3(64), refine_lds_bytes(e, horizon_iters), st, e->P, e->geo,
                                       e->res, e->tv, a, e->d_ref_key));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&key, e->d_ref_key, sizeof key, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    if (key != init) {
        *cost = (int64_t)(key >> 32);
        *i_out = (int32_t)((key >> 16) & 0xffff);
        *j_out = (int32_t)(key & 0xffff);
    }
    return 0;
}

extern "C" int lqrrt_refine_commit(lqrrt_engine* e, const int32_t* plan_host, int P, int goal_tries, int horizon_iters, int i, int j,
                                   int32_t* ids_out, int cap_ids, void* stream) {
    NOT_GENERIC(e);
    if (!e) return fail(LQRRT_E_ARG, "null engine");
    if (i < 0 || j <= i || j >= P) return fail(LQRRT_E_ARG, "candidate (%d, %d) outside a plan of %d nodes", i, j, P);
    if (!ids_out || cap_ids < P - 1 - j + goal_tries) return fail(LQRRT_E_ARG, "ids_out must hold %d ids", P - 1 - j + goal_tries);
    TRY(use_device(e));
    hipStream_t st = (hipStream_t)stream;
    std::vector<int> buf;
    RefineArgs a;
    TRY(refine_prepare(e, plan_host, P, goal_tries, horizon_iters, buf, &a, st));
    const int base = e->N;
    int* d_out = (int*)(e->d_ref_key + 1);
    DISPATCH(e, hipLaunchKernelGGL((k_refine_commit<S>), dim3(1), dim3(64), refine_lds_bytes(e, horizon_iters), st, e->P, e->geo, e->res,
                                   e->tv, a, i, j, base, e->fix, d_out));
    HIPCHK(hipGetLastError());
    int out[3] = {0, 0, 0};
    HIPCHK(hipMemcpyAsync(out, d_out, sizeof out, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (out[0] < 0) return fail(LQRRT_E_CAPACITY, "tree capacity %d cannot hold the refined chain", e->cap);
    if (!out[2]) return fail(LQRRT_E_STATE, "candidate (%d, %d) does not reach the goal: nothing appended", i, j);
    const int count = out[0];
    // host mirrors, as lqrrt_tree_append keeps them: parents, edge lengths, the ignore set (new nodes are not ignored)
    std::vector<int> lens((size_t)count);
    HIPCHK(hipMemcpy(lens.data(), e->tv.elen + base, sizeof(int) * count, hipMemcpyDeviceToHost));
    for (int k = 0; k < count; ++k) {
        const int id = base + k;
        e->h_pid.push_back(k == 0 ? plan_host[i] : id - 1);
        e->h_elen.push_back(lens[k]);
        if ((e->h_ign[id >> 6] >> (id & 63)) & 1ull) {
            e->h_ign[id >> 6] &= ~(1ull << (id & 63));
            e->ign_dirty = true; e->ign_patch_valid = false;
        }
        ids_out[k] = id;
    }
    e->N = base + count;
    e->ign_hi = std::max(e->ign_hi, e->N);
    e->tot.tree_size = e->N;
    return count;
}
