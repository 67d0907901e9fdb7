// ABI: tree-wide goal chains through waypoints -- the search over (node, first waypoint) pairs and the commit of its winner
// (Planner.connect_via; kernels in connect_via.hpp, the rule restated from the C oracle's primitives in
// tests/connect_via_reference.py).  Fragment of engine.hip, behind engine_connect.hpp whose checks, depth table and candidates it uses.
//
// The rule: engine_connect.hpp's tree and depth table; waypoints w_0 .. w_{Q-1}, Q >= 0, states of n doubles that need be neither
// tree nodes nor feasible.  A candidate is a pair (v, j), 0 <= j <= Q, v every node or those of the caller's strictly ascending id
// list; it starts at v's state and gain at cost depth[v] and steers, one refine_edge per target, toward w_j .. w_{Q-1} and then
// toward the goal up to goal_tries times.  An empty edge adds nothing and the chain goes on to its next target.  After every
// non-empty edge the chain ends valid if its end lies strictly inside the goal box; when the targets run out it is invalid.
// Winner: the valid candidate of smallest (cost, v, j) with cost < incumbent.  With Q = 0 this is lqrrt_connect_search's rule.
//
// One image per call (engine_refine.hpp: the solo runners and their scratch): the head (a search's key, a commit's out[3]), the
// waypoints [Q][n] (8-byte aligned behind the head) and, in a search, the depth table [N] and the id list [count].
//
// The checks, the argument block and the key's decoding below serve the calls for several trees too (engine_connect_via_multi.hpp).
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

// a candidate's position in the key is its place in the id list: the list is strictly ascending, so ties go to the smaller node
static int ids_ascending_check(const int32_t* ids, int count, int k) {
    for (int c = 1; ids && c < count; ++c)
        if (ids[c] <= ids[c - 1])
            return fail(LQRRT_E_ARG, "the id list is not strictly ascending at position %d%s", c, engine_suffix(k).c_str());
    return 0;
}

// a search's candidates: connect's list, Q + 1 candidates per node
static int connect_via_candidates_check(lqrrt_engine* e, const int32_t* ids, int* count, int Q, int k) {
    TRY(candidates_check(e, ids, count, (long long)Q + 1, k, [&](int c) {
        return fail(LQRRT_E_ARG, "%d nodes with %d waypoints: %lld candidates exceed one launch%s", c, Q, (long long)c * ((long long)Q + 1),
                    engine_suffix(k).c_str());
    }));
    return ids_ascending_check(ids, *count, k);
}

// The 32-bit bound of a search: the deepest CANDIDATE (of the id list, or of the tree) with every one of its Q + tries targets' edges
// at full length.  It is not connect's and reach's bound, which holds every node of the tree to `tries` edges while the table is
// filled (connect_depths): a chain here is Q edges longer, and only the nodes it may start from count, so the table is filled with
// no edges to come (tries = 0) and the bound is taken here, over the candidates.
static int connect_via_deepest_check(const int* depth, int N, const int32_t* ids, int count, int Q, int tries, int horizon, int k) {
    long long deepest = 0;
    for (int c = 0; c < (ids ? count : N); ++c) deepest = std::max(deepest, (long long)depth[ids ? ids[c] : c]);
    if (count && deepest + ((long long)Q + tries) * horizon > 0x7fffffffLL)
        return fail(LQRRT_E_ARG, "tree too deep for 32-bit step counts%s", engine_suffix(k).c_str());
    return 0;
}

// the argument block of a chain over the waypoints at way_dev; a search adds its depth table and candidates
static void connect_via_fill_args(const lqrrt_engine* e, const double* way_dev, int Q, int tries, int horizon, ConnectViaArgs* a) {
    a->way = way_dev;
    a->nodes = nullptr; a->depth = nullptr;
    a->count = 0; a->Q = Q; a->tries = tries; a->H = horizon;
    goal_fill(e, e->goal, a->goal);
}

// a winner's key: (cost, position in the candidate list * (Q + 1) + j)
static void connect_via_decode(unsigned long long key, const int32_t* ids, int Q, int64_t* cost, int32_t* node, int32_t* j) {
    const long long cand = (long long)(key & 0xffffffffull), pos = cand / ((long long)Q + 1);
    *cost = (int64_t)(key >> 32);
    *node = ids ? ids[pos] : (int32_t)pos;
    *j = (int32_t)(cand - pos * ((long long)Q + 1));
}

// The solo hooks.  What the search and the commit share: behind the head the waypoints (`way`: way_bytes bytes), and the argument block.
struct ConnectViaSolo {
    typedef ConnectViaArgs Args;
    const double* way; size_t way_bytes;
    int Q, tries, horizon;
    size_t bytes() const { return way_bytes; }
    void fill(const lqrrt_engine* e, char* host, const char* dev, ConnectViaArgs* a) const {
        if (way_bytes) memcpy(host, way, way_bytes);
        connect_via_fill_args(e, (const double*)dev, Q, tries, horizon, a);
    }
};

struct ConnectViaSearchSolo : ConnectViaSolo, SoloCands {
    int64_t best; int64_t* cost; int32_t* node_out; int32_t* j_out;
    size_t bytes() const { return way_bytes + SoloCands::bytes(); }
    long long groups() const { return (long long)count * (Q + 1); }
    int keys() const { return 1; }
    int64_t incumbent(int) const { return best; }               // (incumbent, candidate 0)
    void fill(const lqrrt_engine* e, char* host, const char* dev, ConnectViaArgs* a) const {
        ConnectViaSolo::fill(e, host, dev, a);
        stage(host + way_bytes, dev + way_bytes, a);
    }
    template <class S>
    static void launch(const lqrrt_engine* e, unsigned grid, size_t lds, hipStream_t st, const ConnectViaArgs& a, unsigned long long* key) {
        hipLaunchKernelGGL((k_connect_via_search<S>), dim3(grid), dim3(64), lds, st, e->P, e->geo, e->res, e->tv, a, key);
    }
    void won(int, unsigned long long key) const { connect_via_decode(key, ids, Q, cost, node_out, j_out); }
};

// the replay of candidate (node, j), `depth` steps from the root
struct ConnectViaCommitSolo : ConnectViaSolo {
    int node, j, depth;
    template <class S>
    void launch(const lqrrt_engine* e, size_t lds, hipStream_t st, const ConnectViaArgs& a, int base, int* out) const {
        hipLaunchKernelGGL((k_connect_via_commit<S>), dim3(1), dim3(64), lds, st, e->P, e->geo, e->res, e->tv, a, node, j, depth, base, e->fix, out);
    }
};

extern "C" int lqrrt_connect_via_search(lqrrt_engine* e, const int32_t* nodes_host, int count, const double* waypoints_host, int Q,
                                        int goal_tries, int horizon_iters, int64_t incumbent, int64_t* cost, int32_t* node_out,
                                        int32_t* j_out, void* stream) {
    NOT_GENERIC(e);
    if (!e || !cost || !node_out || !j_out) return fail(LQRRT_E_ARG, "null argument");
    TRY(incumbent_check(incumbent, -1));
    TRY(connect_via_check(e, waypoints_host, Q, goal_tries, horizon_iters));
    TRY(connect_via_candidates_check(e, nodes_host, &count, Q, -1));
    ConnectViaSearchSolo h{{waypoints_host, sizeof(double) * Q * e->n, Q, goal_tries, horizon_iters},
                           {std::vector<int>((size_t)e->N), nodes_host, count}, incumbent, cost, node_out, j_out};
    TRY(connect_depths(e, 0, horizon_iters, h.depth.data()));
    TRY(connect_via_deepest_check(h.depth.data(), e->N, nodes_host, count, Q, goal_tries, horizon_iters, -1));
    *cost = incumbent; *node_out = -1; *j_out = -1;
    return solo_search_run(e, horizon_iters, (hipStream_t)stream, h);
}

// a commit's winner (node, j): what connect_winner_check asks of its Q - j + tries targets; *room: their number
static int connect_via_winner_check(lqrrt_engine* e, int node, int j, int Q, int tries, int horizon, const int32_t* ids_out, int cap_ids,
                                    int k, long long* depth, int* room) {
    TRY(range_ok(e, node, 1));
    if (j < 0 || j > Q) return fail(LQRRT_E_ARG, "first waypoint %d outside [0, %d]%s", j, Q, engine_suffix(k).c_str());
    *room = (int)((long long)Q - j + tries);
    return connect_winner_check(e, node, (long long)Q - j + tries, horizon, ids_out, cap_ids, k, depth);
}

extern "C" int lqrrt_connect_via_commit(lqrrt_engine* e, int node, int j, const double* waypoints_host, int Q, int goal_tries,
                                        int horizon_iters, int32_t* ids_out, int cap_ids, void* stream) {
    NOT_GENERIC(e);
    if (!e) return fail(LQRRT_E_ARG, "null engine");
    TRY(connect_via_check(e, waypoints_host, Q, goal_tries, horizon_iters));
    long long depth = 0;
    int room = 0;
    TRY(connect_via_winner_check(e, node, j, Q, goal_tries, horizon_iters, ids_out, cap_ids, -1, &depth, &room));
    return solo_commit_run(e, horizon_iters, node, ids_out, (hipStream_t)stream,
                           ConnectViaCommitSolo{{waypoints_host, sizeof(double) * Q * e->n, Q, goal_tries, horizon_iters}, node, j, (int)depth},
                           "the chain to the goal",
                           strf("the chain of candidate (%d, %d) does not reach the goal: nothing appended", node, j).c_str());
}
