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
// one scratch (d_con) that grows on demand and is, like d_ref, not part of lqrrt_engine_footprint.  The calls for several trees
// (lqrrt_connect_*_multi, connect_goals) follow the one-tree calls below.
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

// The depth table of the tree as it stands, depth[0 .. N): one ascending pass over the host mirrors of the parents and edge lengths
// (the rule above: depth[0] = 1, depth[v] = depth[pID[v]] + L_v, which needs pID[v] < v).  No chain of `tries` edges of up to
// `horizon` steps below any node may leave 32-bit step counts.  The one statement of the rule: the solo search and the searches of
// a multi-engine call both fill their images here.
static int connect_depths(const lqrrt_engine* e, int tries, int horizon, int* depth) {
    const int N = e->N;
    long long deepest = 1;
    depth[0] = 1;
    for (int v = 1; v < N; ++v) {
        const int p = e->h_pid[(size_t)v];
        if (p < 0 || p >= v) return fail(LQRRT_E_STATE, "node %d has parent %d: the depth table needs pID[v] < v", v, p);
        const long long d = (long long)depth[p] + e->h_elen[(size_t)v];
        if (d + (long long)tries * horizon > 0x7fffffffLL) return fail(LQRRT_E_ARG, "tree too deep for 32-bit step counts");
        depth[v] = (int)d;
        deepest = std::max(deepest, d);
    }
    if (deepest + (long long)tries * horizon > 0x7fffffffLL) return fail(LQRRT_E_ARG, "tree too deep for 32-bit step counts");
    return 0;
}

// steps from the root to `node`, the root's own included, by climbing: what a commit needs of the table
static long long connect_depth_of(const lqrrt_engine* e, int node) {
    long long depth = 1;
    for (int v = node; v > 0; v = e->h_pid[(size_t)v]) depth += e->h_elen[(size_t)v];
    return depth;
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
    TRY(connect_depths(e, goal_tries, horizon_iters, depth));
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
    const long long depth = connect_depth_of(e, node);
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

// --------------------------------------------------------------------------------------------
// Several trees per call: lqrrt_connect_search_multi / lqrrt_connect_commit_multi (connect_goals), in the structure of
// engine_refine.hpp's multi path.  Every argument of every engine is checked before anything is written or launched.  A search call
// is cut into CHUNKS of up to MULTI_MAX engines with candidates (fewer than 2^32 threads per launch); per chunk one image in device
// memory -- the keys, then a ConnectDesc per engine, then every engine's depth table and id list -- staged on the host, uploaded
// in one copy; one launch (connect.hpp k_connect_search_multi); the keys back in one copy.  The chunks of a call are enqueued one
// after another and waited for once.  The image lives in the scratch of the chunk's first engine that refine_plans' calls use too
// (refine_multi_scratch, d_refm: not part of the footprint); the calls are synchronous, so nothing reads it after they return.
// The commit IS refine_commit_multi_run: per winner the one-node plan [v] with the cost prefix [depth[v]], i = j = 0.
struct ConnectChunk {
    int first = 0;                        // the engine (index into the call) whose scratch holds the image
    std::vector<int> members;             // indices (into the call) of the engines that take part in the launch
    std::vector<char> img;                // host image of the scratch
};

// what the two calls check alike, for every engine
static int connect_multi_check(lqrrt_engine** engines, int n, const int32_t* tries, const int32_t* horizons) {
    if (!engines || n < 1) return fail(LQRRT_E_ARG, "no engines");
    if (!tries || !horizons) return fail(LQRRT_E_ARG, "null argument");
    if (n > 4 * MULTI_MAX) return fail(LQRRT_E_ARG, "at most %d engines per call", 4 * (int)MULTI_MAX);
    lqrrt_engine* e0 = engines[0];
    for (int k = 0; k < n; ++k) {
        lqrrt_engine* e = engines[k];
        if (!e) return fail(LQRRT_E_ARG, "null engine");
        NOT_GENERIC(e);
        for (int q = 0; q < k; ++q)
            if (engines[q] == e) return fail(LQRRT_E_ARG, "engine %d appears twice", k);
        if (e->device != e0->device || e->model != e0->model) return fail(LQRRT_E_ARG, "engines of one call share the device and the model");
        TRY(connect_check(e, tries[k], horizons[k]));
    }
    return 0;
}

static int connect_search_multi_run(lqrrt_engine** engines, int n, const int32_t* const* nodes, const std::vector<int>& counts,
                                    const std::vector<std::vector<int>>& depths, const int32_t* tries, const int32_t* horizons,
                                    const int64_t* incumbents, int64_t* cost, int32_t* node_out, hipStream_t st,
                                    std::vector<ConnectChunk>& chunks) {
    // chunks: up to MULTI_MAX engines with candidates, one 64-thread workgroup per candidate and fewer than 2^32 threads per launch
    long long cands = 0;
    for (int k = 0; k < n; ++k) {
        if (counts[k] == 0) continue;                           // (an empty id list: no launch, no winner)
        if (chunks.empty() || (int)chunks.back().members.size() == MULTI_MAX || (cands + counts[k]) * 64 > 0xffffffffLL) {
            chunks.emplace_back();
            chunks.back().first = k;
            cands = 0;
        }
        chunks.back().members.push_back(k);
        cands += counts[k];
    }
    for (ConnectChunk& c : chunks) {
        const int m = (int)c.members.size();
        size_t off = 0;
        auto carve = [&](size_t bytes) { const size_t at = off; off += (bytes + 15) / 16 * 16; return at; };
        const size_t o_keys = carve(sizeof(unsigned long long) * m);
        const size_t o_desc = carve(sizeof(ConnectDesc) * m);
        std::vector<size_t> o_depth((size_t)m), o_ids((size_t)m);
        for (int q = 0; q < m; ++q) {
            const int k = c.members[q];
            o_depth[q] = carve(sizeof(int) * depths[k].size());
            o_ids[q] = carve(nodes && nodes[k] ? sizeof(int) * (size_t)counts[k] : 0);
        }
        c.img.assign(off, 0);
        char* d_img = nullptr;
        TRY(refine_multi_scratch(engines[c.first], off, &d_img));
        unsigned long long* keys = (unsigned long long*)(c.img.data() + o_keys);
        ConnectDesc* hd = (ConnectDesc*)(c.img.data() + o_desc);
        ProtoTable pt;
        memset(&pt, 0, sizeof pt);
        size_t lds = 0;
        std::vector<long long> grid_counts((size_t)m);
        for (int q = 0; q < m; ++q) {
            const int k = c.members[q];
            lqrrt_engine* e = engines[k];
            const bool listed = nodes && nodes[k];
            keys[q] = (unsigned long long)incumbents[k] << 32;  // (incumbent, node 0): every candidate at its cost loses
            memcpy(c.img.data() + o_depth[q], depths[k].data(), sizeof(int) * depths[k].size());
            if (listed) memcpy(c.img.data() + o_ids[q], nodes[k], sizeof(int) * (size_t)counts[k]);
            ConnectArgs& a = hd[q].a;
            a.depth = (const int*)(d_img + o_depth[q]);
            a.nodes = listed ? (const int*)(d_img + o_ids[q]) : nullptr;
            a.count = counts[k]; a.tries = tries[k]; a.H = horizons[k]; a.pad = 0;
            for (int d = 0; d < MAXN; ++d) a.goal[d] = d < e->n ? e->goal[d] : 0.0;
            hd[q].best = (unsigned long long*)(d_img + o_keys) + q;
            TRY(multi_sync_proto(e, st));
            pt.p[q] = e->d_proto;
            lds = std::max(lds, refine_lds_bytes(e, horizons[k]));
            grid_counts[q] = counts[k];
        }
        RetainGrid gr;
        const unsigned grid = retain_grid(grid_counts, gr);
        HIPCHK(hipMemcpyAsync(d_img, c.img.data(), c.img.size(), hipMemcpyHostToDevice, st));
        DISPATCH(engines[0], hipLaunchKernelGGL((k_connect_search_multi<S>), dim3(grid), dim3(64), lds, st, pt,
                                                (const ConnectDesc*)(d_img + o_desc), gr));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(c.img.data(), d_img, sizeof(unsigned long long) * m, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    for (const ConnectChunk& c : chunks) {
        const unsigned long long* keys = (const unsigned long long*)c.img.data();
        for (size_t q = 0; q < c.members.size(); ++q) {
            const int k = c.members[q];
            if (keys[q] == (unsigned long long)incumbents[k] << 32) continue;
            cost[k] = (int64_t)(keys[q] >> 32);
            node_out[k] = (int32_t)(keys[q] & 0xffffffffull);
        }
    }
    return 0;
}

extern "C" int lqrrt_connect_search_multi(lqrrt_engine** engines, int n, const int32_t* const* nodes, const int32_t* counts,
                                          const int32_t* goal_tries, const int32_t* horizon_iters, const int64_t* incumbents,
                                          int64_t* cost_out, int32_t* node_out, void* stream) {
    TRY(connect_multi_check(engines, n, goal_tries, horizon_iters));
    if (!incumbents || !cost_out || !node_out) return fail(LQRRT_E_ARG, "null argument");
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
        if ((long long)cnt[k] * 64 > 0xffffffffLL) return fail(LQRRT_E_ARG, "%d candidates exceed one launch (engine %d)", cnt[k], k);
        if (listed)
            for (int c = 0; c < cnt[k]; ++c) TRY(range_ok(e, nodes[k][c], 1));
        depths[k].assign((size_t)e->N, 0);
        TRY(connect_depths(e, goal_tries[k], horizon_iters[k], depths[k].data()));
    }
    TRY(use_device(engines[0]));
    hipStream_t st = (hipStream_t)stream;
    for (int k = 0; k < n; ++k) { cost_out[k] = incumbents[k]; node_out[k] = -1; }
    std::vector<ConnectChunk> chunks;                           // (outlives every copy of the call, also when the call fails)
    const int rc = connect_search_multi_run(engines, n, nodes, cnt, depths, goal_tries, horizon_iters, incumbents, cost_out, node_out, st, chunks);
    return rc ? refine_multi_fail(rc, st) : 0;
}

extern "C" int lqrrt_connect_commit_multi(lqrrt_engine** engines, int n, const int32_t* nodes, const int32_t* goal_tries,
                                          const int32_t* horizon_iters, int32_t* const* ids_out, const int32_t* cap_ids,
                                          int32_t* counts_out, void* stream) {
    TRY(connect_multi_check(engines, n, goal_tries, horizon_iters));
    if (!nodes || !ids_out || !cap_ids || !counts_out) return fail(LQRRT_E_ARG, "null argument");
    // per winner the one-node "plan" [node] with the cost prefix [depth], candidate i = j = 0: goal_tries steers at the goal, the
    // non-empty edges appended below `node` (as lqrrt_connect_commit replays its winner with k_refine_commit)
    std::vector<std::vector<int>> bufs((size_t)n);
    std::vector<int32_t> ones((size_t)n, 1), ij((size_t)n, -1);
    for (int k = 0; k < n; ++k) {
        if (nodes[k] == -1) continue;                           // an engine without a winner
        lqrrt_engine* e = engines[k];
        TRY(range_ok(e, nodes[k], 1));
        if (!ids_out[k] || cap_ids[k] < goal_tries[k]) return fail(LQRRT_E_ARG, "ids_out of engine %d must hold %d ids", k, goal_tries[k]);
        const long long depth = connect_depth_of(e, nodes[k]);
        if (depth + (long long)goal_tries[k] * horizon_iters[k] > 0x7fffffffLL)
            return fail(LQRRT_E_ARG, "tree too deep for 32-bit step counts (engine %d)", k);
        bufs[k] = {nodes[k], (int)depth};
        ij[k] = 0;
    }
    TRY(use_device(engines[0]));
    hipStream_t st = (hipStream_t)stream;
    std::vector<RefineChunk> chunks;                            // (outlives every copy of the call, also when the call fails)
    const int rc = refine_commit_multi_run(engines, n, bufs, ones.data(), goal_tries, horizon_iters, ij.data(), ij.data(), ids_out, counts_out,
                                           st, chunks);
    return rc ? refine_multi_fail(rc, st) : 0;
}
