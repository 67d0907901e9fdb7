// refine.hpp -- plan refinement (Planner.refine_plan): the shortcut search over a found plan and the replay of its winner.
// Fragment of kernels.hpp (included there, in order, inside namespace lq).  The rule is restated on the host from the C
// oracle's primitives in tests/refine_reference.py; in short, for a plan p_0 .. p_{P-1}:
//   candidate (i, j), 0 <= i < j <= P-1, starts at p_i (state and gain) at cost sum_{k<=i} L_k and steers, one edge per
//   target, toward p_j .. p_{P-2} and then up to `tries` times toward the goal; the chain ends after the first edge whose
//   end lies strictly inside the goal box (valid) or when the targets run out (invalid).  Winner: smallest
//   (cost, i, j); accepted only below the plan's own cost.
// Every edge is Planner._steer(force_arrive=False) (planner.py:354-438) with a FIXED horizon: the same error / K / step /
// feasibility sequence as k_steer, the FPR cut of an infeasible rollout, no hfactor heuristic.
//
// Execution: one wavefront per candidate (k_refine_search), everything wave-uniform as in k_steer_force; the lanes split the
// feasibility sweep.  The best key found so far -- cost << 32 | i << 16 | j -- is one 64-bit word in global memory, lowered
// with a global atomic min; a chain whose running key already exceeds it stops (costs only grow along a chain, so this never
// changes the winner).  No trajectory leaves the search: k_refine_commit replays the winner in one workgroup and writes its
// non-empty edges into the tree as a parent chain below p_i.

struct RefineArgs {
    const int* plan;          // [P] node ids, p_0 (the root) first
    const int* prefix;        // [P] sum_{k<=i} L_k (L_0 = 1)
    int P, tries, H;          // plan length, goal tries, fixed steer horizon (<= TreeView::H)
    int pad;
    double goal[MAXN];
};

__device__ __forceinline__ unsigned long long refine_key(int cost, int i, int j) {
    return ((unsigned long long)(unsigned)cost << 32) | ((unsigned long long)(unsigned)i << 16) | (unsigned long long)(unsigned)j;
}

// The chain's current node lives in LDS (cur: state [N] | trig [2 NW] | K [M N]), not in registers: the rollout's own registers
// are what the feasibility sweep and the gain need.
template <class S> constexpr int refine_cur_doubles() { return S::N + 2 * S::NW + S::M * S::N; }

// One edge from the chain's current node toward xt.  Returns the recorded length; when it is > 0 the current node becomes the
// edge's end state with its trig and lqr(x_end, u_last)[1] (tree.add_node, planner.py:257).  The rows go to hx [H][N],
// hu [H][M] (LDS): the FPR cut of an infeasible rollout ends the edge on an earlier row, whose gain is then evaluated again.
// Ends with a barrier: the caller may read cur and the rows from any lane.
template <class S>
__device__ __forceinline__ int refine_edge(const Params& P, const Geo& g, const GeoL& gl, const Res& r, int H, double* cur,
                                           const double* xt, const double* ttrig, double* hx, double* hu, GainLds<S>& gls, int lane) {
    double xc[S::N], tc[2 * S::NW + 1], Kc[S::M * S::N];
#pragma unroll
    for (int d = 0; d < S::N; ++d) xc[d] = cur[d];
#pragma unroll
    for (int k = 0; k < 2 * S::NW; ++k) tc[k] = cur[S::N + k];
#pragma unroll
    for (int q = 0; q < S::M * S::N; ++q) Kc[q] = cur[S::N + 2 * S::NW + q];
    int cnt = 0, steps = 0;
    bool cut = false;
    for (;;) {
        double e[S::N], u[S::M], uc[S::M], xn[S::N], trn[2 * S::NW + 1];
        erf_cached<S>(xt, ttrig, xc, tc, e);
#pragma unroll
        for (int i = 0; i < S::M; ++i) {
            double a = Kc[i * S::N] * e[0];
#pragma unroll
            for (int j = 1; j < S::N; ++j) a += Kc[i * S::N + j] * e[j];
            u[i] = a; uc[i] = a;
        }
        S::step(P.p, xc, tc, uc, r.dt, xn);
        trig_of<S>(xn, trn);
        if (!S::feasible(P.p, g, gl, xn, u, trn, lane)) {         // planner.py:393-396
            const int kept = (int)(r.FPR * (double)cnt);
            cut = kept < cnt;
            cnt = kept;
            break;
        }
        ++steps;
        bool conv = true;                                        // planner.py:428-429 (hfactor off)
#pragma unroll
        for (int d = 0; d < S::N; ++d) conv = conv && (fabs(e[d]) <= r.tol[d]);
        if (steps > H || conv) break;
        store_uniform<S::N>(hx + (size_t)cnt * S::N, xn, lane);
        store_uniform<S::M>(hu + (size_t)cnt * S::M, u, lane);
        ++cnt;
#pragma unroll
        for (int d = 0; d < S::N; ++d) xc[d] = xn[d];
#pragma unroll
        for (int k = 0; k < 2 * S::NW; ++k) tc[k] = trn[k];
        system_gain<S>(P.p, xc, tc, u, r.dt, gls, lane, Kc);     // planner.py:436
    }
    __syncthreads();
    if (cnt == 0) return 0;
    if (cut) {                                                   // the edge now ends on row cnt - 1
        double ul[S::M];
#pragma unroll
        for (int d = 0; d < S::N; ++d) xc[d] = hx[(size_t)(cnt - 1) * S::N + d];
#pragma unroll
        for (int j = 0; j < S::M; ++j) ul[j] = hu[(size_t)(cnt - 1) * S::M + j];
        trig_of<S>(xc, tc);
        system_gain<S>(P.p, xc, tc, ul, r.dt, gls, lane, Kc);
    }
    if (lane == 0) {
#pragma unroll
        for (int d = 0; d < S::N; ++d) cur[d] = xc[d];
#pragma unroll
        for (int k = 0; k < 2 * S::NW; ++k) cur[S::N + k] = tc[k];
#pragma unroll
        for (int q = 0; q < S::M * S::N; ++q) cur[S::N + 2 * S::NW + q] = Kc[q];
    }
    __syncthreads();
    return cnt;
}

template <class S>
__device__ __forceinline__ bool refine_in_goal(const double* lo, const double* hi, const double* x) {   // planner.py:442-447
    bool in = true;
#pragma unroll
    for (int d = 0; d < S::N; ++d) in = in && (lo[d] < x[d]) && (x[d] < hi[d]);
    return in;
}

template <class S>
__device__ __forceinline__ bool refine_in_goal(const Res& r, const double* x) {   // (the engine's own goal box)
    return refine_in_goal<S>(r.goal_lo, r.goal_hi, x);
}

// target t of a chain: plan node t (t < P - 1) or the goal
template <class S>
__device__ __forceinline__ void refine_target(const TreeView& tv, const RefineArgs& a, int t, double* xt, double* ttrig) {
    if (t < a.P - 1) {
        const int id = a.plan[t];
#pragma unroll
        for (int d = 0; d < S::N; ++d) xt[d] = tv.state[(size_t)d * tv.cap + id];
#pragma unroll
        for (int k = 0; k < 2 * S::NW; ++k) ttrig[k] = tv.trig[(size_t)k * tv.cap + id];
    } else {
#pragma unroll
        for (int d = 0; d < S::N; ++d) xt[d] = a.goal[d];
        trig_of<S>(xt, ttrig);
    }
}

// node id of the tree -> the chain's current node (cur, LDS); ends with a barrier
template <class S>
__device__ __forceinline__ void refine_start(const TreeView& tv, int id, double* cur, int lane) {
    if (lane < S::N) cur[lane] = tv.state[(size_t)lane * tv.cap + id];
    if (lane < 2 * S::NW) cur[S::N + lane] = tv.trig[(size_t)lane * tv.cap + id];
    for (int q = lane; q < S::M * S::N; q += 64) cur[S::N + 2 * S::NW + q] = tv.K[(size_t)id * S::M * S::N + q];
    __syncthreads();
}

__device__ __forceinline__ unsigned long long refine_best(const unsigned long long* best) {
    const unsigned long long v = __hip_atomic_load(best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

// Candidate `cand` of one plan, c <-> (i, j) row by row, by one wavefront.  lds: the staged geometry, then the edge rows [H][N]
// and [H][M], then the chain's current node.  *best holds the incumbent's key on entry and the winner's on exit.  Shared by
// k_refine_search (the grid is one plan) and k_refine_search_multi (the grid spans the plans of a call; P / g / r / tv / a are
// then references into device memory, read by scalar loads).
template <class S>
__device__ __forceinline__ void refine_search_body(const Params& P, const Geo& g, const Res& r, const TreeView& tv, const RefineArgs& a,
                                                   unsigned long long* __restrict__ best, double* lds, int cand) {
    __shared__ GainLds<S> gl_lds;
    const int lane = threadIdx.x;
    int c = cand, i = 0;
    while (c >= a.P - 1 - i) { c -= a.P - 1 - i; ++i; }
    const int j = i + 1 + c;
    int cost = a.prefix[i];
    if (refine_key(cost, i, j) > refine_best(best)) return;
    const GeoL gl = stage_geo(g, lds, lane, 64);
    double* hx = lds + geo_lds_doubles(g);
    double* hu = hx + (size_t)a.H * S::N;
    double* cur = hu + (size_t)a.H * S::M;
    refine_start<S>(tv, a.plan[i], cur, lane);                  // (its barrier also covers the staged geometry)
    for (int t = j; t < a.P - 1 + a.tries; ++t) {
        double xt[S::N], ttrig[2 * S::NW + 1];
        refine_target<S>(tv, a, t, xt, ttrig);
        const int len = refine_edge<S>(P, g, gl, r, a.H, cur, xt, ttrig, hx, hu, gl_lds, lane);
        if (len == 0) continue;
        cost += len;
        const unsigned long long key = refine_key(cost, i, j);
        if (key > refine_best(best)) return;
        if (refine_in_goal<S>(r, cur)) {
            if (lane == 0) atomicMin(best, key);
            return;
        }
    }
}

// Grid = P (P - 1) / 2 workgroups of one wavefront.  Dynamic LDS: refine_lds_bytes.
template <class S>
__global__ __launch_bounds__(64) void k_refine_search(Params P, Geo g, Res r, TreeView tv, RefineArgs a,
                                                      unsigned long long* __restrict__ best) {
    extern __shared__ double geo_lds[];
    refine_search_body<S>(P, g, r, tv, a, best, geo_lds, (int)blockIdx.x);
}

// Writes the chain's current node (cur) and its edge rows (hx, hu: `len` of them) into the tree as node `id` below `parent`: state,
// trig, K, parent, edge length, edge rows and -- when the sampler has fixed angles -- the angle errors (TreeView::werr).  Ends with
// a barrier: the next edge overwrites the rows and the current node.  Shared by the commits of refine.hpp and connect_via.hpp.
template <class S>
__device__ __forceinline__ void refine_write_node(const TreeView& tv, const FixedAngles& fx, int id, int parent, int len,
                                                  const double* hx, const double* hu, const double* cur, int lane) {
    double* xe = tv.xedge + (size_t)id * tv.H * S::N;
    double* ue = tv.uedge + (size_t)id * tv.H * S::M;
    for (int q = lane; q < len * S::N; q += 64) xe[q] = hx[q];
    for (int q = lane; q < len * S::M; q += 64) ue[q] = hu[q];
    if (lane < S::N) tv.state[(size_t)lane * tv.cap + id] = cur[lane];
    if (lane < 2 * S::NW) tv.trig[(size_t)lane * tv.cap + id] = cur[S::N + lane];
    for (int q = lane; q < S::M * S::N; q += 64) tv.K[(size_t)id * S::M * S::N + q] = cur[S::N + 2 * S::NW + q];
    if constexpr (S::NW > 0) {
        if (fx.on && lane < S::NW)
            tv.werr[(size_t)lane * tv.cap + id] = wrap_err(fx.t[2 * lane], fx.t[2 * lane + 1], cur[S::N + 2 * lane],
                                                           cur[S::N + 2 * lane + 1]);
    }
    if (lane == 0) { tv.pID[id] = parent; tv.elen[id] = len; }
    __syncthreads();
}

// Replays candidate (i, j) in one workgroup and appends its non-empty edges as nodes base, base + 1, ... (parent chain below
// p_i), with state, trig, K, parent, edge length, edge rows and -- when the sampler has fixed angles -- the angle errors
// (TreeView::werr).  out[0] = the number of nodes appended, or -1 when the chain does not fit below tv.cap (then nothing
// at or above the tree size is meaningful and the caller keeps its size); out[1] = the chain's cost; out[2] = 1 when it ended
// in the goal box.  lens (may be null): the appended nodes' edge lengths once more, in order, where the host finds those of a
// whole call in one copy.
template <class S>
__device__ __forceinline__ void refine_commit_body(const Params& P, const Geo& g, const Res& r, const TreeView& tv, const RefineArgs& a,
                                                   int i, int j, int base, const FixedAngles& fx, int* __restrict__ out,
                                                   int* __restrict__ lens, double* lds) {
    __shared__ GainLds<S> gl_lds;
    const int lane = threadIdx.x;
    const GeoL gl = stage_geo(g, lds, lane, 64);
    double* hx = lds + geo_lds_doubles(g);
    double* hu = hx + (size_t)a.H * S::N;
    double* cur = hu + (size_t)a.H * S::M;
    int parent = a.plan[i], cost = a.prefix[i], added = 0, goal = 0;
    refine_start<S>(tv, parent, cur, lane);
    for (int t = j; t < a.P - 1 + a.tries; ++t) {
        double xt[S::N], ttrig[2 * S::NW + 1];
        refine_target<S>(tv, a, t, xt, ttrig);
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
__global__ __launch_bounds__(64) void k_refine_commit(Params P, Geo g, Res r, TreeView tv, RefineArgs a, int i, int j, int base,
                                                      FixedAngles fx, int* __restrict__ out) {
    extern __shared__ double geo_lds[];
    if (blockIdx.x != 0) return;
    refine_commit_body<S>(P, g, r, tv, a, i, j, base, fx, out, nullptr, geo_lds);
}

// ------------------------------------------------------------------------------------------
// The same two stages for SEVERAL plans per launch (lqrrt_refine_search_multi / lqrrt_refine_commit_multi; refine_plans).  A search
// round is bound by its longest chain, not by its width: the rounds of a fleet's plans run side by side in ONE launch.  As in
// retain.hpp a workgroup finds its engine from the ascending prefix table of workgroup counts in the arguments (multi_engine_of)
// and reads P / g / r / tv from that engine's device-resident EngineProto; what belongs to the call -- the plan, its cost prefix,
// P, tries, H, the goal, the candidate to replay and where the results go -- is a RefineDesc per engine in device memory.  Every
// engine has its OWN best key: the early stop prunes within one plan only, so each winner is the one the engine's own launch finds.
struct RefineDesc {
    RefineArgs a;
    unsigned long long* best;     // search: the engine's key
    int* out;                     // commit: the engine's out[3]
    int* lens;                    // commit: the engine's slice of the edge lengths
    int i, j, base, pad;          // commit: the candidate and the tree size
};

// Grid = the engines' P (P - 1) / 2 back to back.  Dynamic LDS: the largest refine_lds_bytes of the call.
template <class S>
__global__ __launch_bounds__(64) void k_refine_search_multi(ProtoTable pt, const RefineDesc* __restrict__ ds, RetainGrid gr) {
    extern __shared__ double geo_lds[];
    const int e = multi_engine_of(gr.block0, gr.n, (int)blockIdx.x);
    const RefineDesc& d = ds[e];
    const EngineProto& p = *pt.p[e];
    refine_search_body<S>(p.P, p.g, p.r, p.tv, d.a, d.best, geo_lds, (int)blockIdx.x - gr.block0[e]);
}

// One workgroup per engine with a winner: ds and pt hold those engines only, in the same order.
template <class S>
__global__ __launch_bounds__(64) void k_refine_commit_multi(ProtoTable pt, const RefineDesc* __restrict__ ds, int n) {
    extern __shared__ double geo_lds[];
    if ((int)blockIdx.x >= n) return;
    const RefineDesc& d = ds[blockIdx.x];
    const EngineProto& p = *pt.p[blockIdx.x];
    refine_commit_body<S>(p.P, p.g, p.r, p.tv, d.a, d.i, d.j, d.base, p.ra.fx, d.out, d.lens, geo_lds);
}
