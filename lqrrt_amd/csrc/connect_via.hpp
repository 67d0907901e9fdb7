// connect_via.hpp -- tree-wide goal chains through waypoints (Planner.connect_via): refine.hpp starts a chain only on the plan and
// aims it at the plan's own nodes, connect.hpp starts one at every node of the tree and aims it at the goal alone; here a chain
// starts at any node of the tree and runs through a caller's list of states -- the rest of an older plan that the tree no longer
// holds, or the path of a coarser planner -- before it turns to the goal.  Fragment of kernels.hpp (included there after
// connect.hpp, inside namespace lq).  The rule is restated on the host from the C oracle's primitives in
// tests/connect_via_reference.py; in short, for a tree of N nodes with connect.hpp's depth table and waypoints w_0 .. w_{Q-1}
// (states of n doubles; they need be neither tree nodes nor feasible):
//   a candidate is a pair (v, j), 0 <= j <= Q, v any node (or one of a caller's id list); it starts at v's state and gain at cost
//   depth[v] and steers, one refine_edge per target, toward w_j .. w_{Q-1} and then up to `tries` times toward the goal.  An empty
//   edge adds nothing and the chain goes on to its next target; a non-empty one moves the chain to its end.  After every non-empty
//   edge, a waypoint's included, the chain ends valid if its end lies strictly inside the goal box; when the targets run out first
//   it is invalid.  Winner: the valid candidate of smallest (cost, v, j) with cost < incumbent.  j = Q is connect.hpp's candidate.
//
// Execution: one wavefront per candidate; candidate c = pos (Q + 1) + j, pos the position in the strictly ascending id list (or v
// itself), so that the order of c is that of (v, j) and shallow nodes come first in the grid.  The best key -- cost << 32 | c -- is
// connect.hpp's: one 64-bit word, initialised to incumbent << 32, lowered with a global atomic min, polled for the early stop.  The
// waypoint table is written by the host before the launch and by nothing during it: it is read through the constant address
// space (launch_constant), so that its wave-uniform reads stay scalar loads behind the atomic poll of the key instead of vector
// loads whose results sit in VGPRs across refine_edge.  Plain launches on one stream.

struct ConnectViaArgs {
    const int* nodes;         // [count] candidate node ids, strictly ascending, or null: position pos is node pos
    const int* depth;         // [tree size] connect.hpp's depth table
    const double* way;        // [Q][S::N] waypoints
    int count, Q, tries, H;   // candidate nodes, waypoints, goal tries, fixed steer horizon (<= TreeView::H)
    double goal[MAXN];
};

// target t of a chain: waypoint t (t < Q) or the goal; the cos / sin of a waypoint come from its state, as the goal's do
template <class S>
__device__ __forceinline__ void connect_via_target(const ConnectViaArgs& a, int t, double* xt, double* ttrig) {
    if (t < a.Q) {
#pragma unroll
        for (int d = 0; d < S::N; ++d) xt[d] = launch_constant(a.way + (size_t)t * S::N + d);
    } else {
#pragma unroll
        for (int d = 0; d < S::N; ++d) xt[d] = a.goal[d];
    }
    trig_of<S>(xt, ttrig);
}

// Candidate `cand` by one wavefront.  lds: the layout of refine_lds_bytes.  *best holds the incumbent's key on entry and the winner's
// on exit.  A body of its own so that a grid spanning several engines can share it.
template <class S>
__device__ __forceinline__ void connect_via_search_body(const Params& P, const Geo& g, const Res& r, const TreeView& tv,
                                                        const ConnectViaArgs& a, unsigned long long* __restrict__ best, double* lds,
                                                        unsigned cand) {
    __shared__ GainLds<S> gl_lds;
    const int lane = threadIdx.x;
    const unsigned per = (unsigned)a.Q + 1u;
    const unsigned pos = cand / per;
    if (pos >= (unsigned)a.count) return;
    const int j = (int)(cand - pos * per);
    const int v = a.nodes ? a.nodes[pos] : (int)pos;
    int cost = a.depth[v];
    if (connect_key(cost, (int)cand) > refine_best(best)) return;
    const GeoL gl = stage_geo(g, lds, lane, 64);
    double* hx = lds + geo_lds_doubles(g);
    double* hu = hx + (size_t)a.H * S::N;
    double* cur = hu + (size_t)a.H * S::M;
    refine_start<S>(tv, v, cur, lane);                          // (its barrier also covers the staged geometry)
    for (int t = j; t < a.Q + a.tries; ++t) {
        double xt[S::N], ttrig[2 * S::NW + 1];
        connect_via_target<S>(a, t, xt, ttrig);
        const int len = refine_edge<S>(P, g, gl, r, a.H, cur, xt, ttrig, hx, hu, gl_lds, lane);
        if (len == 0) {
            if (t >= a.Q) break;                                // (nothing moved and the goal stays: every later try repeats it)
            continue;
        }
        cost += len;
        const unsigned long long key = connect_key(cost, (int)cand);
        if (key > refine_best(best)) return;
        if (refine_in_goal<S>(r, cur)) {
            if (lane == 0) atomicMin(best, key);
            return;
        }
    }
}

// Grid = one workgroup of one wavefront per candidate, count (Q + 1) of them.  Dynamic LDS: refine_lds_bytes.
template <class S>
__global__ __launch_bounds__(64) void k_connect_via_search(Params P, Geo g, Res r, TreeView tv, ConnectViaArgs a,
                                                           unsigned long long* __restrict__ best) {
    extern __shared__ double geo_lds[];
    connect_via_search_body<S>(P, g, r, tv, a, best, geo_lds, (unsigned)blockIdx.x);
}

// Replays candidate (v, j) in one workgroup and appends its non-empty edges as nodes base, base + 1, ... (a parent chain below v)
// through refine.hpp's node writer.  depth: depth[v].  out as in refine_commit_body: out[0] = the number of nodes appended, or -1
// when the chain does not fit below tv.cap; out[1] = the chain's cost; out[2] = 1 when it ended in the goal box.  lens (may be
// null), as in refine_commit_body: the appended nodes' edge lengths once more, in order, where the host finds those of a whole
// call in one copy.
template <class S>
__device__ __forceinline__ void connect_via_commit_body(const Params& P, const Geo& g, const Res& r, const TreeView& tv,
                                                        const ConnectViaArgs& a, int v, int j, int depth, int base,
                                                        const FixedAngles& fx, int* __restrict__ out, int* __restrict__ lens,
                                                        double* lds) {
    __shared__ GainLds<S> gl_lds;
    const int lane = threadIdx.x;
    const GeoL gl = stage_geo(g, lds, lane, 64);
    double* hx = lds + geo_lds_doubles(g);
    double* hu = hx + (size_t)a.H * S::N;
    double* cur = hu + (size_t)a.H * S::M;
    int parent = v, cost = depth, added = 0, goal = 0;
    refine_start<S>(tv, parent, cur, lane);
    for (int t = j; t < a.Q + a.tries; ++t) {
        double xt[S::N], ttrig[2 * S::NW + 1];
        connect_via_target<S>(a, t, xt, ttrig);
        const int len = refine_edge<S>(P, g, gl, r, a.H, cur, xt, ttrig, hx, hu, gl_lds, lane);
        if (len == 0) continue;
        const int id = base + added;
        if (id >= tv.cap) { added = -1; break; }
        if (lens && lane == 0) lens[added] = len;
        refine_write_node<S>(tv, fx, id, parent, len, hx, hu, cur, lane);
        parent = id;
        ++added;
        cost += len;
        if (refine_in_goal<S>(r, cur)) { goal = 1; break; }
    }
    if (lane == 0) { out[0] = added; out[1] = cost; out[2] = goal; }
}

template <class S>
__global__ __launch_bounds__(64) void k_connect_via_commit(Params P, Geo g, Res r, TreeView tv, ConnectViaArgs a, int v, int j,
                                                           int depth, int base, FixedAngles fx, int* __restrict__ out) {
    extern __shared__ double geo_lds[];
    if (blockIdx.x != 0) return;
    connect_via_commit_body<S>(P, g, r, tv, a, v, j, depth, base, fx, out, nullptr, geo_lds);
}
