// ABI: tree-wide goal connection -- the search over the nodes of the tree and the commit of its winner (Planner.connect_goal; kernel
// in connect.hpp, the rule restated from the C oracle's primitives in tests/connect_reference.py).  Fragment of engine.hip.
//
// The rule: for a tree of N nodes with pID[v] < v, depth[0] = 1 and depth[v] = depth[pID[v]] + L_v (L_v the edge length).  A candidate
// is a node v (every node, or those of the caller's id list); it starts at v's state and gain at cost depth[v] and steers toward the
// goal, one edge per try (refine_edge: _steer(force_arrive=False), fixed horizon, FPR cut, no hfactor heuristic; an empty edge adds
// nothing, a non-empty one moves the chain to its end with lqr(x_end, u_last)[1]), up to goal_tries times.  It is valid when an edge
// ends strictly inside the goal box, and ends there; a candidate that already lies in the box needs a non-empty edge like any other.
// Winner: the valid candidate of smallest (cost, v) with cost < incumbent.  Its non-empty edges become a parent chain of new nodes
// below v.
//
// The depth table is computed HERE, from the host mirrors of the parents and edge lengths in one ascending pass, and uploaded with
// the call (4 B per node: 0.4 MB and well under a millisecond at 10^5 nodes).  It lives with the candidate ids and the results in
// one scratch (d_con) that grows on demand and is, like d_ref, not part of lqrrt_engine_footprint.
// --------------------------------------------------------------------------------------------

static int connect_check(lqrrt_engine* e, int tries, int horizon) {
    if (tries < 1) return fail(LQRRT_E_ARG, "goal_tries must be >= 1");
    if (!e->has_res || !e->has_goal) return fail(LQRRT_E_STATE, "set_resolution with a goal first");
    if (horizon < 1 || horizon > e->H) return fail(LQRRT_E_ARG, "horizon of %d steps (the edge pools hold %d)", horizon, e->H);
    if (e->N < 1) return fail(LQRRT_E_STATE, "the tree is empty");
    return 0;
}

// room for `ints` ints behind the head of 8
static int connect_scratch(lqrrt_engine* e, size_t ints) {
    if (e->d_con && ints <= e->con_cap) return 0;
    const size_t keep = g_dalloc_bytes;
    if (e->d_con) (void)hipFree(e->d_con);
    e->d_con = nullptr; e->con_cap = 0;
    const size_t want = (ints + 1023) / 1024 * 1024;
    const int rc = dalloc(&e->d_con, want + 8);
    g_dalloc_bytes = keep;                                      // (allocated on first use: not part of the footprint)
    if (rc) return rc;
    e->con_cap = want;
    return 0;
}

extern "C" int lqrrt_connect_search(lqrrt_engine* e, const int32_t* nodes_host, int count, int goal_tries, int horizon_iters,
                                    int64_t incumbent, int64_t* cost, int32_t* node_out, void* stream) {
    NOT_GENERIC(e);
    if (!e || !cost || !node_out) return fail(LQRRT_E_ARG, "null argument");
    if (incumbent < 1 || incumbent > 0x7fffffffLL) return fail(LQRRT_E_ARG, "incumbent cost %lld out of range", (long long)incumbent);
    TRY(connect_check(e, goal_tries, horizon_iters));
    const int N = e->N;
    if (!nodes_host) count = N;
    if (count < 0) return fail(LQRRT_E_ARG, "negative candidate count");
    if ((long long)count * 64 > 0xffffffffLL) return fail(LQRRT_E_ARG, "%d candidates exceed one launch", count);
    if (nodes_host)
        for (int k = 0; k < count; ++k) TRY(range_ok(e, nodes_host[k], 1));
    // the image of the call: head (the key), depth [N], candidate ids [count]
    std::vector<int> img((size_t)8 + N + (nodes_host ? count : 0), 0);
    int* depth = img.data() + 8;
    long long deepest = 1;
    depth[0] = 1;
    for (int v = 1; v < N; ++v) {
        const int p = e->h_pid[(size_t)v];
        if (p < 0 || p >= v) return fail(LQRRT_E_STATE, "node %d has parent %d: the depth table needs pID[v] < v", v, p);
        const long long d = (long long)depth[p] + e->h_elen[(size_t)v];
        if (d + (long long)goal_tries * horizon_iters > 0x7fffffffLL) return fail(LQRRT_E_ARG, "tree too deep for 32-bit step counts");
        depth[v] = (int)d;
        deepest = std::max(deepest, d);
    }
    if (deepest + (long long)goal_tries * horizon_iters > 0x7fffffffLL) return fail(LQRRT_E_ARG, "tree too deep for 32-bit step counts");
    if (nodes_host && count) memcpy(depth + N, nodes_host, sizeof(int) * (size_t)count);
    const unsigned long long init = (unsigned long long)incumbent << 32;   // (incumbent, node 0): every candidate at its cost loses
    memcpy(img.data(), &init, sizeof init);
    *cost = incumbent; *node_out = -1;
    if (count == 0) return 0;
    TRY(use_device(e));
    hipStream_t st = (hipStream_t)stream;
    TRY(connect_scratch(e, img.size() - 8));
    HIPCHK(hipMemcpyAsync(e->d_con, img.data(), sizeof(int) * img.size(), hipMemcpyHostToDevice, st));
    ConnectArgs a;
    a.depth = e->d_con + 8;
    a.nodes = nodes_host ? e->d_con + 8 + N : nullptr;
    a.count = count; a.tries = goal_tries; a.H = horizon_iters; a.pad = 0;
    for (int d = 0; d < MAXN; ++d) a.goal[d] = d < e->n ? e->goal[d] : 0.0;
    unsigned long long* d_key = (unsigned long long*)e->d_con;
    DISPATCH(e, hipLaunchKernelGGL((k_connect_search<S>), dim3((unsigned)count), dim3(64), refine_lds_bytes(e, horizon_iters), st, e->P,
                                   e->geo, e->res, e->tv, a, d_key));
    HIPCHK(hipGetLastError());
    unsigned long long key = init;
    HIPCHK(hipMemcpyAsync(&key, d_key, sizeof key, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));                           // (img is the source of a copy until here)
    if (key != init) {
        *cost = (int64_t)(key >> 32);
        *node_out = (int32_t)(key & 0xffffffffull);
    }
    return 0;
}

extern "C" int lqrrt_connect_commit(lqrrt_engine* e, int node, int goal_tries, int horizon_iters, int32_t* ids_out, int cap_ids,
                                    void* stream) {
    NOT_GENERIC(e);
    if (!e) return fail(LQRRT_E_ARG, "null engine");
    TRY(connect_check(e, goal_tries, horizon_iters));
    TRY(range_ok(e, node, 1));
    if (!ids_out || cap_ids < goal_tries) return fail(LQRRT_E_ARG, "ids_out must hold %d ids", goal_tries);
    long long depth = 1;
    for (int v = node; v > 0; v = e->h_pid[(size_t)v]) depth += e->h_elen[(size_t)v];
    if (depth + (long long)goal_tries * horizon_iters > 0x7fffffffLL) return fail(LQRRT_E_ARG, "tree too deep for 32-bit step counts");
    TRY(use_device(e));
    hipStream_t st = (hipStream_t)stream;
    // the winner's replay is k_refine_commit on the one-node "plan" [node] with the cost prefix [depth]: i = j = 0 steers goal_tries
    // times at the goal and appends the non-empty edges below `node`
    TRY(connect_scratch(e, 2));
    const int img[10] = {0, 0, 0, 0, 0, 0, 0, 0, node, (int)depth};
    HIPCHK(hipMemcpyAsync(e->d_con, img, sizeof img, hipMemcpyHostToDevice, st));
    RefineArgs a;
    refine_fill_args(e, e->d_con + 8, 1, goal_tries, horizon_iters, &a);
    const int base = e->N;
    int* d_out = e->d_con + 2;
    DISPATCH(e, hipLaunchKernelGGL((k_refine_commit<S>), dim3(1), dim3(64), refine_lds_bytes(e, horizon_iters), st, e->P, e->geo, e->res,
                                   e->tv, a, 0, 0, base, e->fix, d_out));
    HIPCHK(hipGetLastError());
    int out[3] = {0, 0, 0};
    HIPCHK(hipMemcpyAsync(out, d_out, sizeof out, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (out[0] < 0) return fail(LQRRT_E_CAPACITY, "tree capacity %d cannot hold the chain to the goal", e->cap);
    if (!out[2]) return fail(LQRRT_E_STATE, "the chain below node %d does not reach the goal: nothing appended", node);
    const int count = out[0];
    std::vector<int> lens((size_t)count);
    HIPCHK(hipMemcpy(lens.data(), e->tv.elen + base, sizeof(int) * count, hipMemcpyDeviceToHost));
    refine_adopt(e, node, count, lens.data(), ids_out);
    return count;
}
