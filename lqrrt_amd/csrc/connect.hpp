// connect.hpp -- tree-wide goal connection (Planner.connect_goal): from which node of the WHOLE tree does a short chain of
// goal-directed steers reach the goal, and which of them gives the shortest plan?  Fragment of kernels.hpp (included there after
// refine.hpp, inside namespace lq).  The rule is restated on the host from the C oracle's primitives in tests/connect_reference.py;
// in short, for a tree of N nodes with pID[v] < v, depth[0] = 1 and depth[v] = depth[pID[v]] + L_v (L_v the edge length; RefineArgs::
// prefix extended from the plan to the tree):
//   a candidate is a node v -- every node, or those of a caller's id list; it starts at v's state and gain at cost depth[v] and
//   steers toward the goal, one edge per try, up to `tries` times.  Every edge is refine_edge: Planner._steer(force_arrive=False)
//   (planner.py:354-438) with a FIXED horizon, the FPR cut, no hfactor heuristic; an empty edge adds nothing, a non-empty one moves
//   the chain to its end state with lqr(x_end, u_last)[1].  The chain is valid when an edge ends strictly inside the goal box, and
//   ends there; when the tries run out first it is invalid.  A candidate that itself lies in the goal box is an ordinary candidate:
//   it needs a non-empty edge like any other.  Winner: the valid candidate of smallest (cost, v) with cost < incumbent.
//
// Execution: one wavefront per candidate (k_connect_search), as in k_refine_search.  The best key found so far -- cost << 32 | v --
// is one 64-bit word in global memory, initialised to incumbent << 32 and lowered with a global atomic min; a chain whose running
// key already exceeds it stops (costs only grow along a chain, so the winner depends neither on scheduling nor on the order of an
// id list), and a candidate whose depth[v] << 32 | v exceeds it returns before it stages anything.  Plain launches on one stream:
// no cooperative launch, no flag another workgroup waits for.  No trajectory leaves the search: the winner is replayed in one
// workgroup by k_refine_commit (refine_commit_body with P = 1, plan = [v], prefix = [depth[v]], i = j = 0: `tries` steers at the
// goal) and its non-empty edges become a parent chain of new nodes below v.

struct ConnectArgs {
    const int* nodes;         // [count] candidate node ids, or null: candidate c is node c
    const int* depth;         // [tree size] steps from the root to each node, the root's own included (depth[0] = 1)
    int count, tries, H;      // candidates, goal tries, fixed steer horizon (<= TreeView::H)
    int pad;
    double goal[MAXN];
};

__device__ __forceinline__ unsigned long long connect_key(int cost, int v) {
    return ((unsigned long long)(unsigned)cost << 32) | (unsigned long long)(unsigned)v;
}

// Candidate `cand` by one wavefront.  lds: the staged geometry, then the edge rows [H][N] and [H][M], then the chain's current node
// (the layout of refine_lds_bytes).  *best holds the incumbent's key on entry and the winner's on exit.  A body of its own so that a
// grid spanning several engines can share it (P / g / r / tv / a are then references into device memory).
template <class S>
__device__ __forceinline__ void connect_search_body(const Params& P, const Geo& g, const Res& r, const TreeView& tv, const ConnectArgs& a,
                                                    unsigned long long* __restrict__ best, double* lds, int cand) {
    __shared__ GainLds<S> gl_lds;
    const int lane = threadIdx.x;
    if (cand >= a.count) return;
    const int v = a.nodes ? a.nodes[cand] : cand;
    int cost = a.depth[v];
    if (connect_key(cost, v) > refine_best(best)) return;
    const GeoL gl = stage_geo(g, lds, lane, 64);
    double* hx = lds + geo_lds_doubles(g);
    double* hu = hx + (size_t)a.H * S::N;
    double* cur = hu + (size_t)a.H * S::M;
    refine_start<S>(tv, v, cur, lane);                          // (its barrier also covers the staged geometry)
    double xt[S::N], ttrig[2 * S::NW + 1];
#pragma unroll
    for (int d = 0; d < S::N; ++d) xt[d] = a.goal[d];
    trig_of<S>(xt, ttrig);
    for (int t = 0; t < a.tries; ++t) {
        const int len = refine_edge<S>(P, g, gl, r, a.H, cur, xt, ttrig, hx, hu, gl_lds, lane);
        if (len == 0) break;                                    // (nothing moved and the target stays: every later try repeats it)
        cost += len;
        const unsigned long long key = connect_key(cost, v);
        if (key > refine_best(best)) return;
        if (refine_in_goal<S>(r, cur)) {
            if (lane == 0) atomicMin(best, key);
            return;
        }
    }
}

// Grid = one workgroup of one wavefront per candidate.  Dynamic LDS: refine_lds_bytes.
template <class S>
__global__ __launch_bounds__(64) void k_connect_search(Params P, Geo g, Res r, TreeView tv, ConnectArgs a,
                                                       unsigned long long* __restrict__ best) {
    extern __shared__ double geo_lds[];
    connect_search_body<S>(P, g, r, tv, a, best, geo_lds, (int)blockIdx.x);
}

// ------------------------------------------------------------------------------------------
// The same search for SEVERAL trees per launch (lqrrt_connect_search_multi; connect_goals).  A search leaves most of the chip idle
// once its first chain has reached the goal and the early stop prunes the rest: the searches of a fleet's trees run side by side in
// ONE launch.  As in k_refine_search_multi a workgroup finds its engine from the ascending prefix table of workgroup counts in the
// arguments (multi_engine_of) and reads P / g / r / tv from that engine's device-resident EngineProto; what belongs to the call --
// the candidate ids, the depth table, count, tries, H, the goal and where the winner goes -- is a ConnectDesc per engine in device
// memory.  Every engine has its OWN best key: the early stop prunes within one tree only, so each winner is the one the engine's
// own launch finds, whatever the scheduling.  The batched commit is k_refine_commit_multi (a RefineDesc per winner: plan = [v],
// prefix = [depth[v]], P = 1, i = j = 0).
struct ConnectDesc {
    ConnectArgs a;
    unsigned long long* best;     // the engine's key
};

// *p for data that nothing writes while the kernel runs (the host wrote it before the launch), read through the CONSTANT address
// space.  connect_search_body polls the best key with an atomic load, and behind an atomic load the compiler takes every later read
// of ordinary global memory for clobbered: the body's reads of P / g / r / tv -- wave-uniform, scalar loads in the solo kernel, whose
// arguments are constant by construction -- turn into vector loads whose results sit in VGPRs (DoubleIntegratorT<6>: 256 VGPRs + 2
// AGPRs and one wavefront per SIMD instead of two).  A read of the constant address space stays a scalar load wherever it stands.
// The detour through an integer keeps the address-space inference from folding the cast back into the global pointer it came from.
template <class T>
__device__ __forceinline__ const T& launch_constant(const T* p) {
    return *(const T*)(const __attribute__((address_space(4))) T*)(unsigned long long)p;
}

// Grid = the engines' candidate counts back to back.  Dynamic LDS: the largest refine_lds_bytes of the call.
template <class S>
__global__ __launch_bounds__(64) void k_connect_search_multi(ProtoTable pt, const ConnectDesc* __restrict__ ds, RetainGrid gr) {
    extern __shared__ double geo_lds[];
    const int e = multi_engine_of(gr.block0, gr.n, (int)blockIdx.x);
    const ConnectDesc& d = launch_constant(ds + e);
    const EngineProto& p = launch_constant(pt.p[e]);
    connect_search_body<S>(p.P, p.g, p.r, p.tv, d.a, d.best, geo_lds, (int)blockIdx.x - gr.block0[e]);
}
