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
// the call (4 B per node: 0.4 MB and well under a millisecond at 10^5 nodes).  The image of a search (engine_refine.hpp: the solo
// runners and their scratch): the head (the key), the depth table [N], the candidate ids [count]; that of a commit: the head
// (out[3]), the one-node plan [node] and its cost prefix [depth].  The calls for several trees (lqrrt_connect_*_multi,
// connect_goals) follow the one-tree calls below.
// --------------------------------------------------------------------------------------------

static int connect_check(lqrrt_engine* e, int tries, int horizon) {
    if (tries < 1) return fail(LQRRT_E_ARG, "goal_tries must be >= 1");
    if (!e->has_res || !e->has_goal) return fail(LQRRT_E_STATE, "set_resolution with a goal first");
    if (horizon < 1 || horizon > e->H) return fail(LQRRT_E_ARG, "horizon of %d steps (the edge pools hold %d)", horizon, e->H);
    if (e->N < 1) return fail(LQRRT_E_STATE, "the tree is empty");
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

// A search's candidates: the nodes `ids` (null: every node of the tree, and *count becomes its size) of *count entries, each a
// node of the tree.  One 64-thread workgroup per candidate, `per` candidates per node: they must fit one launch (fewer than 2^32
// threads), else too_many(count) words the refusal.  k: the engine's index for the messages (< 0: a one-engine call).
template <class TooMany>
static int candidates_check(lqrrt_engine* e, const int32_t* ids, int* count, long long per, int k, TooMany too_many) {
    if (!ids) *count = e->N;
    if (*count < 0) return fail(LQRRT_E_ARG, "negative candidate count%s", engine_suffix(k).c_str());
    if (*count * per > 0xffffffffLL / 64) return too_many(*count);
    for (int c = 0; ids && c < *count; ++c) TRY(range_ok(e, ids[c], 1));
    return 0;
}

static int connect_candidates_check(lqrrt_engine* e, const int32_t* ids, int* count, int k) {
    return candidates_check(e, ids, count, 1, k, [&](int c) {
        return fail(LQRRT_E_ARG, "%d candidates exceed one launch%s", c, engine_suffix(k).c_str());
    });
}

static void connect_fill_args(const lqrrt_engine* e, const int* depth_dev, const int* ids_dev, int count, int tries, int horizon,
                              ConnectArgs* a) {
    a->depth = depth_dev;
    a->nodes = ids_dev;
    a->count = count; a->tries = tries; a->H = horizon; a->pad = 0;
    goal_fill(e, e->goal, a->goal);
}

// a winner's key: (cost, node)
static void connect_decode(unsigned long long key, int64_t* cost, int32_t* node) {
    *cost = (int64_t)(key >> 32);
    *node = (int32_t)(key & 0xffffffffull);
}

// What a search over the nodes of one tree (connect, via, reach) keeps of its candidates -- the depth table, the id list (null:
// every node), the candidate count -- and the one staging of the table and the optional list into the call's image.
struct SoloCands {
    std::vector<int> depth;
    const int32_t* ids; int count;
    size_t bytes() const { return sizeof(int) * (depth.size() + (ids ? (size_t)count : 0)); }
    // the table and the list to `host`, and depth / nodes / count of the argument block
    template <class Args>
    void stage(char* host, const char* dev, Args* a) const {
        const size_t o_ids = sizeof(int) * depth.size();
        memcpy(host, depth.data(), o_ids);
        if (ids) memcpy(host + o_ids, ids, sizeof(int) * (size_t)count);
        a->depth = (const int*)dev;
        a->nodes = ids ? (const int*)(dev + o_ids) : nullptr;
        a->count = count;
    }
};

// the search's hooks (engine_refine.hpp: solo_search_run), over its candidates
struct ConnectSearchSolo : SoloCands {
    typedef ConnectArgs Args;
    int tries, horizon; int64_t best; int64_t* cost; int32_t* node_out;
    long long groups() const { return count; }
    int keys() const { return 1; }
    int64_t incumbent(int) const { return best; }               // (incumbent, node 0)
    void fill(const lqrrt_engine* e, char* host, const char* dev, ConnectArgs* a) const {
        connect_fill_args(e, nullptr, nullptr, 0, tries, horizon, a);
        stage(host, dev, a);
    }
    template <class S>
    static void launch(const lqrrt_engine* e, unsigned grid, size_t lds, hipStream_t st, const ConnectArgs& a, unsigned long long* key) {
        hipLaunchKernelGGL((k_connect_search<S>), dim3(grid), dim3(64), lds, st, e->P, e->geo, e->res, e->tv, a, key);
    }
    void won(int, unsigned long long key) const { connect_decode(key, cost, node_out); }
};

extern "C" int lqrrt_connect_search(lqrrt_engine* e, const int32_t* nodes_host, int count, int goal_tries, int horizon_iters,
                                    int64_t incumbent, int64_t* cost, int32_t* node_out, void* stream) {
    NOT_GENERIC(e);
    if (!e || !cost || !node_out) return fail(LQRRT_E_ARG, "null argument");
    TRY(incumbent_check(incumbent, -1));
    TRY(connect_check(e, goal_tries, horizon_iters));
    TRY(connect_candidates_check(e, nodes_host, &count, -1));
    ConnectSearchSolo h{{std::vector<int>((size_t)e->N), nodes_host, count}, goal_tries, horizon_iters, incumbent, cost, node_out};
    TRY(connect_depths(e, goal_tries, horizon_iters, h.depth.data()));
    *cost = incumbent; *node_out = -1;
    return solo_search_run(e, horizon_iters, (hipStream_t)stream, h);
}

// A commit's winner `node` (a node of the tree) with a chain of up to `targets` edges below it: ids_out has room for their ids, and
// the chain's end stays within 32-bit step counts.  *depth: the steps from the root to `node`.
static int connect_winner_check(const lqrrt_engine* e, int node, long long targets, int horizon, const int32_t* ids_out, int cap_ids, int k,
                                long long* depth) {
    if (!ids_out || cap_ids < targets) return fail(LQRRT_E_ARG, "ids_out must hold %lld ids%s", targets, engine_suffix(k).c_str());
    *depth = connect_depth_of(e, node);
    if (*depth + targets * horizon > 0x7fffffffLL)
        return fail(LQRRT_E_ARG, "tree too deep for 32-bit step counts%s", engine_suffix(k).c_str());
    return 0;
}

// The replay of a search's winner, behind the caller's checks: the refinement's commit (solo_commit_run with RefineCommitSolo:
// k_refine_commit) on the one-node "plan" [node] with the cost prefix [depth], i = j = 0, steers goal_tries times at `goal` and
// appends the non-empty edges below `node`; the chain ends inside the goal box of `res`.  lqrrt_connect_commit passes the engine's
// own goal and resolution block, lqrrt_reach_commit a target's (`end`: what the messages call it).
static int connect_commit_run(lqrrt_engine* e, int node, int goal_tries, int horizon_iters, const double* goal, const Res& res,
                              const char* end, int32_t* ids_out, int cap_ids, void* stream) {
    long long depth = 0;
    TRY(connect_winner_check(e, node, goal_tries, horizon_iters, ids_out, cap_ids, -1, &depth));
    const std::vector<int> buf = {node, (int)depth};
    return solo_commit_run(e, horizon_iters, node, ids_out, (hipStream_t)stream,
                           RefineCommitSolo{{buf, 1, goal_tries, horizon_iters, goal}, 0, 0, res}, strf("the chain to the %s", end).c_str(),
                           strf("the chain below node %d does not reach the %s: nothing appended", node, end).c_str());
}

extern "C" int lqrrt_connect_commit(lqrrt_engine* e, int node, int goal_tries, int horizon_iters, int32_t* ids_out, int cap_ids,
                                    void* stream) {
    NOT_GENERIC(e);
    if (!e) return fail(LQRRT_E_ARG, "null engine");
    TRY(connect_check(e, goal_tries, horizon_iters));
    TRY(range_ok(e, node, 1));
    return connect_commit_run(e, node, goal_tries, horizon_iters, e->goal, e->res, "goal", ids_out, cap_ids, stream);
}

// --------------------------------------------------------------------------------------------
// Several trees per call: lqrrt_connect_search_multi / lqrrt_connect_commit_multi (connect_goals), on engine_refine.hpp's multi
// path: its engine-list check and its two runners, which own the chunks, the scratch (d_refm: not part of the footprint), the
// prototypes, the keys, the guard and the one synchronise.  The search states its hooks: a ConnectDesc per engine, behind it every
// engine's depth table and id list (MultiCands), one launch (connect.hpp k_connect_search_multi), a key's decoding.  The commit
// states none: it IS the refinement's, multi_commit_run with RefineCommitMulti -- per winner the one-node plan [v] with the cost
// prefix [depth[v]], i = j = 0.

// what the two calls check alike, for every engine
static int connect_multi_check(lqrrt_engine** engines, int n, const int32_t* tries, const int32_t* horizons) {
    return multi_engines_check(engines, n, tries && horizons, [&](int k) { return connect_check(engines[k], tries[k], horizons[k]); });
}

// engine k's id list in a call for several engines: none (every node of its tree), or `ids` with their count
static int multi_id_list(const int32_t* const* nodes, const int32_t* counts, int k, const int32_t** ids, int* count) {
    *ids = nodes ? nodes[k] : nullptr;
    if (*ids && !counts) return fail(LQRRT_E_ARG, "an id list without its count (engine %d)", k);
    *count = *ids ? counts[k] : 0;
    return 0;
}

// What a search over the nodes of several trees (connect, via, reach) keeps per engine of its call -- the id list (null: every
// node), the candidate count, the depth table -- and the one staging of a member's depth table and optional id list into a chunk's
// image.
struct MultiCands {
    std::vector<const int32_t*> ids;
    std::vector<int> counts;                                    // (an empty id list: no launch, no winner)
    std::vector<std::vector<int>> depths;
    explicit MultiCands(int n) : ids((size_t)n, nullptr), counts((size_t)n, 0), depths((size_t)n) {}
    struct At { size_t depth, ids; };
    At carve(int k, Carve& carve) const {
        const size_t o_depth = carve(sizeof(int) * depths[k].size());
        return {o_depth, carve(ids[k] ? sizeof(int) * (size_t)counts[k] : 0)};
    }
    // engine k's table and list into c's image, and depth / nodes / count of its argument block
    template <class Args>
    void stage(int k, const At& at, MultiChunk& c, Args* a) const {
        memcpy(c.img.data() + at.depth, depths[k].data(), sizeof(int) * depths[k].size());
        if (ids[k]) memcpy(c.img.data() + at.ids, ids[k], sizeof(int) * (size_t)counts[k]);
        a->depth = (const int*)(c.dev + at.depth);
        a->nodes = ids[k] ? (const int*)(c.dev + at.ids) : nullptr;
        a->count = counts[k];
    }
};

// the search's hooks (engine_refine.hpp: multi_search_run)
struct ConnectSearchMulti {
    typedef ConnectDesc Desc;
    typedef MultiCands::At Part;
    const MultiCands& x;
    lqrrt_engine** engines;
    const int32_t* tries; const int32_t* horizons; const int64_t* incumbents; int64_t* cost; int32_t* node_out;
    long long groups(int k) const { return x.counts[k]; }
    int keys(int) const { return 1; }
    int64_t incumbent(int k, int) const { return incumbents[k]; }   // (incumbent, node 0)
    Part carve(const MultiChunk& c, size_t q, Carve& carve) const { return x.carve(c.members[q], carve); }
    void fill(MultiChunk& c, size_t q, const std::vector<Part>& at, ConnectDesc* d) const {
        const int k = c.members[q];
        connect_fill_args(engines[k], nullptr, nullptr, 0, tries[k], horizons[k], &d->a);
        x.stage(k, at[q], c, &d->a);
        d->best = c.keys_of(c.dev, q);
    }
    template <class S>
    static void launch(unsigned grid, size_t lds, hipStream_t st, const ProtoTable& pt, const ConnectDesc* ds, const RetainGrid& gr) {
        hipLaunchKernelGGL((k_connect_search_multi<S>), dim3(grid), dim3(64), lds, st, pt, ds, gr);
    }
    void won(int k, int, unsigned long long key) const { connect_decode(key, &cost[k], &node_out[k]); }
};

extern "C" int lqrrt_connect_search_multi(lqrrt_engine** engines, int n, const int32_t* const* nodes, const int32_t* counts,
                                          const int32_t* goal_tries, const int32_t* horizon_iters, const int64_t* incumbents,
                                          int64_t* cost_out, int32_t* node_out, void* stream) {
    TRY(connect_multi_check(engines, n, goal_tries, horizon_iters));
    if (!incumbents || !cost_out || !node_out) return fail(LQRRT_E_ARG, "null argument");
    MultiCands x(n);
    for (int k = 0; k < n; ++k) {
        lqrrt_engine* e = engines[k];
        TRY(incumbent_check(incumbents[k], k));
        TRY(multi_id_list(nodes, counts, k, &x.ids[k], &x.counts[k]));
        TRY(connect_candidates_check(e, x.ids[k], &x.counts[k], k));
        x.depths[k].assign((size_t)e->N, 0);
        TRY(connect_depths(e, goal_tries[k], horizon_iters[k], x.depths[k].data()));
    }
    TRY(use_device(engines[0]));
    for (int k = 0; k < n; ++k) { cost_out[k] = incumbents[k]; node_out[k] = -1; }
    return multi_search_run(engines, n, horizon_iters, (hipStream_t)stream,
                            ConnectSearchMulti{x, engines, goal_tries, horizon_iters, incumbents, cost_out, node_out});
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
        long long depth = 0;
        TRY(range_ok(engines[k], nodes[k], 1));
        TRY(connect_winner_check(engines[k], nodes[k], goal_tries[k], horizon_iters[k], ids_out[k], cap_ids[k], k, &depth));
        bufs[k] = {nodes[k], (int)depth};
        ij[k] = 0;
    }
    TRY(use_device(engines[0]));
    return multi_commit_run(engines, n, horizon_iters, ids_out, counts_out, (hipStream_t)stream,
                            RefineCommitMulti{{engines, bufs, ones.data(), goal_tries, horizon_iters}, ij.data(), ij.data()});
}
