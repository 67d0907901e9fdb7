// reach.hpp -- one tree asked about MANY goals (Planner.goal_costs / Planner.retarget): connect.hpp's question -- from which node of
// the whole tree does a short chain of goal-directed steers reach the goal, and at what cost? -- for T targets in one launch.
// Fragment of kernels.hpp (included there after connect.hpp, inside namespace lq).  A tree rooted at the vehicle is a single-source
// reachability structure: which goal it was grown for matters to the goal bias of its samples only.  The rule is restated on the
// host from the C oracle's primitives in tests/reach_reference.py (a connect_reference.Connector per target over one tree).
//
// A target t is a goal state g_t with a box lo_t < x < hi_t.  The rule is connect.hpp's with g_t and box_t in place of the engine's
// goal and box, for every target on its own: candidates are every node (or those of an id list) starting at cost depth[v]; up to
// `tries` refine_edges are steered at g_t, an empty edge ends the chain; the chain is valid when an edge ends strictly inside
// box_t; the winner of target t is the valid candidate of smallest (cost, v) with cost < incumbent_t.  Targets never interact.
//
// Execution: T x count workgroups of one wavefront, target-major (t = block / count, c = block % count): the candidates of one
// target run in id order, shallow nodes first, and the early stop bites as it does in k_connect_search.  Every target has its OWN
// best key -- cost << 32 | v, initialised to incumbent_t << 32 and lowered with a global atomic min -- so each winner is the one
// k_connect_search finds for that goal and box, whatever the scheduling.  The targets (goal, lo, hi) are a table in device memory
// that the host writes before the launch; the body polls its key with an atomic load, so the table is read through launch_constant
// (connect.hpp): scalar loads wherever they stand.  The goal state stays in registers along the chain, as the engine's goal does in
// k_connect_search; the box goes to 2 N doubles of LDS once, so that no pointer into the table lives across refine_edge (kept as
// scalar loads at the box test, BoatNovice's private segment grows from 96 to 128 bytes; with the box in LDS every model has the
// private segment and the occupancy of its k_connect_search).
// Plain launches on one stream: no cooperative launch, no flag another workgroup waits for.  The winner of a target is replayed by
// k_refine_commit with RefineArgs::goal = g_t and a Res whose goal box is box_t (lqrrt_reach_commit): no commit kernel of its own.

struct ReachTarget {
    double goal[MAXN];
    double lo[MAXN], hi[MAXN];    // the goal box: lo < x < hi in the model's dimensions
};

struct ReachArgs {
    const ReachTarget* targets;   // [T], written by the host before the launch
    const int* nodes;             // [count] candidate node ids, or null: candidate c is node c
    const int* depth;             // [tree size] steps from the root to each node, the root's own included (depth[0] = 1)
    int T, count, tries, H;       // targets, candidates per target, goal tries, fixed steer horizon (<= TreeView::H)
};

// Workgroup `block` of the T x count grid by one wavefront.  lds: the layout of refine_lds_bytes.  keys[t] holds target t's
// incumbent key on entry and its winner's on exit.  A body of its own so that a grid spanning several engines can share it.
template <class S>
__device__ __forceinline__ void reach_search_body(const Params& P, const Geo& g, const Res& r, const TreeView& tv, const ReachArgs& a,
                                                  unsigned long long* __restrict__ keys, double* lds, unsigned block) {
    __shared__ GainLds<S> gl_lds;
    __shared__ double box[2 * S::N];                            // the target's lo | hi
    const int lane = threadIdx.x;
    const int t = (int)(block / (unsigned)a.count), cand = (int)(block % (unsigned)a.count);
    if (t >= a.T) return;
    unsigned long long* best = keys + t;
    const int v = a.nodes ? a.nodes[cand] : cand;
    int cost = a.depth[v];
    if (connect_key(cost, v) > refine_best(best)) return;
    const ReachTarget& tg = launch_constant(a.targets + t);
    if (lane < S::N) { box[lane] = tg.lo[lane]; box[S::N + lane] = tg.hi[lane]; }
    const GeoL gl = stage_geo(g, lds, lane, 64);
    double* hx = lds + geo_lds_doubles(g);
    double* hu = hx + (size_t)a.H * S::N;
    double* cur = hu + (size_t)a.H * S::M;
    refine_start<S>(tv, v, cur, lane);                          // (its barrier also covers the staged geometry)
    double xt[S::N], ttrig[2 * S::NW + 1];
#pragma unroll
    for (int d = 0; d < S::N; ++d) xt[d] = tg.goal[d];
    trig_of<S>(xt, ttrig);
    for (int k = 0; k < a.tries; ++k) {
        const int len = refine_edge<S>(P, g, gl, r, a.H, cur, xt, ttrig, hx, hu, gl_lds, lane);
        if (len == 0) break;                                    // (nothing moved and the target stays: every later try repeats it)
        cost += len;
        const unsigned long long key = connect_key(cost, v);
        if (key > refine_best(best)) return;
        if (refine_in_goal<S>(box, box + S::N, cur)) {
            if (lane == 0) atomicMin(best, key);
            return;
        }
    }
}

// Grid = T * count workgroups of one wavefront.  Dynamic LDS: refine_lds_bytes.
template <class S>
__global__ __launch_bounds__(64) void k_reach_search(Params P, Geo g, Res r, TreeView tv, ReachArgs a,
                                                     unsigned long long* __restrict__ keys) {
    extern __shared__ double geo_lds[];
    reach_search_body<S>(P, g, r, tv, a, keys, geo_lds, blockIdx.x);
}
