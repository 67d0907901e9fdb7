// clear_connect.hpp -- goal chains clear of moving discs (lqrrt_tree_clear_connect, Planner.avoid(connect)): clear.hpp's question and
// connect.hpp's at once.  Which node whose root path stays clear of the D moving discs reaches the goal by a short chain of
// goal-directed steers that stays clear of them too, at the times the vehicle would be on it -- and is that plan shorter than the best
// clear goal hit the tree already holds?  Reads the tree, writes nothing of it.  Fragment of kernels.hpp (included there behind
// connect.hpp and clear_multi.hpp, inside namespace lq).  The rule is restated in tests/clear_connect_reference.py from
// connect_reference.Connector and clear_reference; in short, on top of clear.hpp's cum / first / dwell / best, all unchanged:
//   incumbent  depth of the best clear hit b, depth = cum - elen[0] + 1 (connect.hpp's cost units), or 2^31 - 1 without one
//   candidate  a node v -- every node, or those of a caller's id list -- with first[v] == -1 (the propagated first: a node below a
//              conflict is no candidate)
//   chain      connect.hpp's, unchanged: up to `tries` refine_edges at the goal against the STATIC map, an empty edge ends it, valid
//              when an edge ends strictly inside the goal box.  The discs cut no edge: they accept or reject the chain, so
//              lqrrt_connect_commit(v, H, tries) replays exactly the chain that was judged
//   time       row k of the chain's j-th non-empty edge has tau = start + cum[v] + (rows of the chain's earlier edges) + k -- what
//              clear.hpp gives the same row once the chain is committed; the discs of tau stand at table row min(tau, L - 1).  A chain
//              is clear when every row of every edge passes at its tau and its last row passes at every tau' in
//              [start + cum[v] + chain rows, L - 1] (the dwell; an empty range passes)
//   winner     the valid and clear candidate of smallest (cost, v) with cost = depth[v] + chain rows < incumbent
//
// Execution: one wavefront per candidate, plain launches on one stream behind clear.hpp's (steps, check, propagate, select) -- no grid
// barrier, no flag another workgroup waits for.  k_clear_connect_seed turns the select's best (cum << 32 | id) into the search's start
// key incumbent << 32; k_clear_connect_search lowers it with connect.hpp's early stop: only valid AND clear chains lower the key, a
// chain whose running key exceeds it is abandoned (costs only grow along a chain), so the winner depends neither on scheduling nor on
// the order of an id list.  Per try the steer comes first, then the key comparison, and only then the disc test of the edge's rows,
// which still lie in the LDS edge buffers: a pruned chain pays for no disc sweep.
// Two worlds, two sets of geometry: g / gl (stage_geo: the static map, as refine_edge wants it) and gd / gld (clear_disc_world: the D
// discs of one instant and nothing else).  The disc test reads the hull through an LDS address whatever the engine's map (clear.hpp),
// so the hull is staged once more behind the layout of refine_lds_bytes: the launch reserves refine_lds_bytes + 16 V.

struct ClearConnectArgs {
    const double* table;          // [L][D][4]: clear.hpp's disc table
    const int* first;             // [tree size] the finished first of k_clear_select
    const RetainLink* steps;      // [tree size] the finished step sums (cum - elen[0])
    int L, D, start, pad;
};

// what the search leaves behind (device -> host in one copy)
struct ClearConnectOut {
    unsigned long long key;       // the seed's incumbent << 32 on entry, the winner's cost << 32 | v on exit
    int listed_clear;             // entries of an id list with first == -1 (without a list the host has the count from the counters)
    int pad;
};

// the start key of the search from the select's best: the depth of the best clear hit, node 0 (every chain at that cost loses)
__global__ void k_clear_connect_seed(TreeView tv, const ClearOut* __restrict__ sel, ClearConnectOut* __restrict__ out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const unsigned long long b = sel->best;
    const unsigned long long incumbent = b == ~0ull ? 0x7fffffffull : (b >> 32) - (unsigned long long)tv.elen[0] + 1ull;
    out->key = incumbent << 32;
}

// Candidate `cand` by one wavefront.  lds: the layout of refine_lds_bytes, then the hull points [2][V] of the disc test.  A body of its
// own so that a grid spanning several engines can share it.
template <class S>
__device__ __forceinline__ void clear_connect_search_body(const Params& P, const Geo& g, const Res& r, const TreeView& tv, const ConnectArgs& a,
                                                          const ClearConnectArgs& c, ClearConnectOut* __restrict__ out, double* lds, int cand) {
    __shared__ GainLds<S> gl_lds;
    const int lane = threadIdx.x;
    if (cand >= a.count) return;
    const int v = a.nodes ? a.nodes[cand] : cand;
    if (c.first[v] >= 0) return;                                // below a conflict, or on one: no candidate
    if (a.nodes && lane == 0) atomicAdd(&out->listed_clear, 1);
    int cost = a.depth[v];
    if (connect_key(cost, v) > refine_best(&out->key)) return;
    const GeoL gl = stage_geo(g, lds, lane, 64);
    double* hx = lds + geo_lds_doubles(g);
    double* hu = hx + (size_t)a.H * S::N;
    double* cur = hu + (size_t)a.H * S::M;
    double* hull_lds = cur + refine_cur_doubles<S>();
    clear_stage_hull(g, hull_lds, lane, 64);
    Geo gd = g;
    GeoL gld;
    clear_disc_world(g, hull_lds, c.D, gd, gld);
    refine_start<S>(tv, v, cur, lane);                          // (its barrier also covers the staged geometry and the hull)
    double xt[S::N], ttrig[2 * S::NW + 1];
#pragma unroll
    for (int d = 0; d < S::N; ++d) xt[d] = a.goal[d];
    trig_of<S>(xt, ttrig);
    // time index of row 0 of the next edge: start + cum[v] + the rows so far (64 bits: beyond L - 1 only the clamp reads it)
    long long base = (long long)c.start + c.steps[v].steps + tv.elen[0];
    for (int t = 0; t < a.tries; ++t) {
        const int len = refine_edge<S>(P, g, gl, r, a.H, cur, xt, ttrig, hx, hu, gl_lds, lane);
        if (len == 0) break;                                    // (nothing moved and the target stays: every later try repeats it)
        cost += len;
        const unsigned long long key = connect_key(cost, v);
        if (key > refine_best(&out->key)) return;
        double x[S::N], u[S::M], trig[2 * S::NW + 1];
        for (int k = 0; k < len; ++k) {
            clear_load_row<S>(hx, hu, k, x, u, trig);
            const long long tau = base + k;
            gld.oc = c.table + (size_t)(tau < c.L - 1 ? tau : c.L - 1) * c.D * 4;
            if (!S::feasible(P.p, gd, gld, x, u, trig, lane)) return;
        }
        base += len;
        if (refine_in_goal<S>(r, cur)) {
            // the chain waits at its last row (x, u, trig hold it) while the discs move on
            for (long long tau = base; tau <= c.L - 1; ++tau) {
                gld.oc = c.table + (size_t)tau * c.D * 4;
                if (!S::feasible(P.p, gd, gld, x, u, trig, lane)) return;
            }
            if (lane == 0) atomicMin(&out->key, key);
            return;
        }
    }
}

// Grid = one workgroup of one wavefront per candidate.  Dynamic LDS: refine_lds_bytes + 16 V.
template <class S>
__global__ __launch_bounds__(64) void k_clear_connect_search(Params P, Geo g, Res r, TreeView tv, ConnectArgs a, ClearConnectArgs c,
                                                             ClearConnectOut* __restrict__ out) {
    extern __shared__ double geo_lds[];
    if constexpr (has_discs<S>::value) clear_connect_search_body<S>(P, g, r, tv, a, c, out, geo_lds, (int)blockIdx.x);
}
