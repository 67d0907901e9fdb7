// ABI: tree-wide goal chains through waypoints -- the search over (node, first waypoint) pairs and the commit of its winner
// (Planner.connect_via; kernels in connect_via.hpp, the rule restated from the C oracle's primitives in
// tests/connect_via_reference.py).  Fragment of engine.hip, behind engine_connect.hpp whose checks, depth table and scratch it uses.
//
// The rule: engine_connect.hpp's tree and depth table; waypoints w_0 .. w_{Q-1}, Q >= 0, states of n doubles that need be neither
// tree nodes nor feasible.  A candidate is a pair (v, j), 0 <= j <= Q, v every node or those of the caller's strictly ascending id
// list; it starts at v's state and gain at cost depth[v] and steers, one refine_edge per target, toward w_j .. w_{Q-1} and then
// toward the goal up to goal_tries times.  An empty edge adds nothing and the chain goes on to its next target.  After every
// non-empty edge the chain ends valid if its end lies strictly inside the goal box; when the targets run out it is invalid.
// Winner: the valid candidate of smallest (cost, v, j) with cost < incumbent.  With Q = 0 this is lqrrt_connect_search's rule.
//
// One image per call in d_con: the head of 8 ints (the key; a commit's out[3] behind it), the waypoints [Q][n] (8-byte aligned
// behind the head), the depth table [N], the id list [count].  One copy up, one launch, one read-back.
// --------------------------------------------------------------------------------------------

// what the two calls check alike, before anything is written; Q waypoints of e->n doubles
static int connect_via_check(lqrrt_engine* e, const double* way, int Q, int tries, int horizon) {
    TRY(connect_check(e, tries, horizon));
    if (Q < 0 || (Q > 0 && !way)) return fail(LQRRT_E_ARG, "%d waypoints without a table", Q);
    if ((long long)Q + tries > 0x7fffffffLL) return fail(LQRRT_E_ARG, "%d waypoints and %d goal tries: too many targets", Q, tries);
    for (size_t k = 0; k < (size_t)Q * e->n; ++k)
        if (!std::isfinite(way[k])) return fail(LQRRT_E_ARG, "waypoint %d is not finite", (int)(k / e->n));
    return 0;
}

static void connect_via_fill_args(const lqrrt_engine* e, int Q, int tries, int horizon, ConnectViaArgs* a) {
    a->way = (const double*)(e->d_con + 8);
    a->nodes = nullptr; a->depth = nullptr;
    a->count = 0; a->Q = Q; a->tries = tries; a->H = horizon;
    for (int d = 0; d < MAXN; ++d) a->goal[d] = d < e->n ? e->goal[d] : 0.0;
}

extern "C" int lqrrt_connect_via_search(lqrrt_engine* e, const int32_t* nodes_host, int count, const double* waypoints_host, int Q,
                                        int goal_tries, int horizon_iters, int64_t incumbent, int64_t* cost, int32_t* node_out,
                                        int32_t* j_out, void* stream) {
    NOT_GENERIC(e);
    if (!e || !cost || !node_out || !j_out) return fail(LQRRT_E_ARG, "null argument");
    if (incumbent < 1 || incumbent > 0x7fffffffLL) return fail(LQRRT_E_ARG, "incumbent cost %lld out of range", (long long)incumbent);
    TRY(connect_via_check(e, waypoints_host, Q, goal_tries, horizon_iters));
    const int N = e->N;
    if (!nodes_host) count = N;
    if (count < 0) return fail(LQRRT_E_ARG, "negative candidate count");
    if ((long long)count * ((long long)Q + 1) * 64 > 0xffffffffLL)
        return fail(LQRRT_E_ARG, "%d nodes with %d waypoints: %lld candidates exceed one launch", count, Q, (long long)count * ((long long)Q + 1));
    if (nodes_host)
        for (int k = 0; k < count; ++k) {
            TRY(range_ok(e, nodes_host[k], 1));
            if (k > 0 && nodes_host[k] <= nodes_host[k - 1]) return fail(LQRRT_E_ARG, "the id list is not strictly ascending at position %d", k);
        }
    // the image of the call: head (the key), waypoints [Q][n], depth [N], candidate ids [count]
    const size_t way_ints = (size_t)2 * Q * e->n;
    std::vector<int> img((size_t)8 + way_ints + N + (nodes_host ? count : 0), 0);
    int* depth = img.data() + 8 + way_ints;
    TRY(connect_depths(e, 0, horizon_iters, depth));
    long long deepest = 0;                                      // the deepest candidate, with every target's edge at full length
    if (nodes_host)
        for (int k = 0; k < count; ++k) deepest = std::max(deepest, (long long)depth[nodes_host[k]]);
    else
        for (int v = 0; v < N; ++v) deepest = std::max(deepest, (long long)depth[v]);
    if (count && deepest + ((long long)Q + goal_tries) * horizon_iters > 0x7fffffffLL)
        return fail(LQRRT_E_ARG, "tree too deep for 32-bit step counts");
    if (way_ints) memcpy(img.data() + 8, waypoints_host, sizeof(int) * way_ints);
    if (nodes_host && count) memcpy(depth + N, nodes_host, sizeof(int) * (size_t)count);
    const unsigned long long init = (unsigned long long)incumbent << 32;   // (incumbent, candidate 0): every candidate at its cost loses
    memcpy(img.data(), &init, sizeof init);
    *cost = incumbent; *node_out = -1; *j_out = -1;
    if (count == 0) return 0;
    TRY(use_device(e));
    hipStream_t st = (hipStream_t)stream;
    TRY(connect_scratch(e, img.size() - 8));
    HIPCHK(hipMemcpyAsync(e->d_con, img.data(), sizeof(int) * img.size(), hipMemcpyHostToDevice, st));
    ConnectViaArgs a;
    connect_via_fill_args(e, Q, goal_tries, horizon_iters, &a);
    a.depth = e->d_con + 8 + way_ints;
    a.nodes = nodes_host ? a.depth + N : nullptr;
    a.count = count;
    unsigned long long* d_key = (unsigned long long*)e->d_con;
    const unsigned grid = (unsigned)((long long)count * (Q + 1));
    DISPATCH(e, hipLaunchKernelGGL((k_connect_via_search<S>), dim3(grid), dim3(64), refine_lds_bytes(e, horizon_iters), st, e->P, e->geo,
                                   e->res, e->tv, a, d_key));
    HIPCHK(hipGetLastError());
    unsigned long long key = init;
    HIPCHK(hipMemcpyAsync(&key, d_key, sizeof key, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));                           // (img is the source of a copy until here)
    if (key != init) {
        const long long c = (long long)(key & 0xffffffffull), pos = c / (Q + 1);
        *cost = (int64_t)(key >> 32);
        *node_out = nodes_host ? nodes_host[pos] : (int32_t)pos;
        *j_out = (int32_t)(c - pos * (Q + 1));
    }
    return 0;
}

extern "C" int lqrrt_connect_via_commit(lqrrt_engine* e, int node, int j, const double* waypoints_host, int Q, int goal_tries,
                                        int horizon_iters, int32_t* ids_out, int cap_ids, void* stream) {
    NOT_GENERIC(e);
    if (!e) return fail(LQRRT_E_ARG, "null engine");
    TRY(connect_via_check(e, waypoints_host, Q, goal_tries, horizon_iters));
    TRY(range_ok(e, node, 1));
    if (j < 0 || j > Q) return fail(LQRRT_E_ARG, "first waypoint %d outside [0, %d]", j, Q);
    const long long room = (long long)Q - j + goal_tries;
    if (!ids_out || cap_ids < room) return fail(LQRRT_E_ARG, "ids_out must hold %lld ids", room);
    const long long depth = connect_depth_of(e, node);
    if (depth + room * horizon_iters > 0x7fffffffLL) return fail(LQRRT_E_ARG, "tree too deep for 32-bit step counts");
    TRY(use_device(e));
    hipStream_t st = (hipStream_t)stream;
    const size_t way_ints = (size_t)2 * Q * e->n;
    TRY(connect_scratch(e, way_ints));
    std::vector<int> img((size_t)8 + way_ints, 0);
    if (way_ints) memcpy(img.data() + 8, waypoints_host, sizeof(int) * way_ints);
    HIPCHK(hipMemcpyAsync(e->d_con, img.data(), sizeof(int) * img.size(), hipMemcpyHostToDevice, st));
    ConnectViaArgs a;
    connect_via_fill_args(e, Q, goal_tries, horizon_iters, &a);
    const int base = e->N;
    int* d_out = e->d_con + 2;
    DISPATCH(e, hipLaunchKernelGGL((k_connect_via_commit<S>), dim3(1), dim3(64), refine_lds_bytes(e, horizon_iters), st, e->P, e->geo,
                                   e->res, e->tv, a, node, j, (int)depth, base, e->fix, d_out));
    HIPCHK(hipGetLastError());
    int out[3] = {0, 0, 0};
    HIPCHK(hipMemcpyAsync(out, d_out, sizeof out, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));                           // (img is the source of a copy until here)
    if (out[0] < 0) return fail(LQRRT_E_CAPACITY, "tree capacity %d cannot hold the chain to the goal", e->cap);
    if (!out[2]) return fail(LQRRT_E_STATE, "the chain of candidate (%d, %d) does not reach the goal: nothing appended", node, j);
    const int count = out[0];
    std::vector<int> lens((size_t)count);
    HIPCHK(hipMemcpy(lens.data(), e->tv.elen + base, sizeof(int) * count, hipMemcpyDeviceToHost));
    refine_adopt(e, node, count, lens.data(), ids_out);
    return count;
}
