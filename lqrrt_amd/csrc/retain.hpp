// retain.hpp -- tree retention (lqrrt_tree_retain, Planner.replan): re-root the device tree at one of its nodes, re-validate the
// kept edges against the current world, compact.  Fragment of kernels.hpp (included there, in order, inside namespace lq).
// The rule is restated in plain NumPy in tests/retain_reference.py; in short, for a tree of N nodes (pID[i] < i) and a root r:
//   ok[i]   = every recorded row of node i's edge passes S::feasible under the current geometry (or true: no revalidation)
//   keep[i] = i == r, or i > r and ok[i] and keep[pID[i]]
//   kept nodes are renumbered in ascending old-id order; the root gets pID -1 and the one-row edge of a seed (tree.py:69-70)
//   goal hits / best plan end / ignore set are rebuilt from the kept nodes against the current goal box.
//
// Execution: plain launches, one after another on one stream -- no grid-wide barrier, no flag another workgroup waits for.
//   check      one wavefront per node, rows in order, the lanes split the hull x obstacle sweep (as k_steer_force does)
//   propagate  keep / in-subtree / step counts down the parent chains by pointer doubling, ceil(log2 N) double-buffered rounds
//   scan       exclusive prefix sum of keep -> new ids: block sums, scan of the sums, add
//   move       gather into scratch by old id, copy back by new id (new ids <= old ids: an in-place parallel move is not safe)
//   goal       hit flags and count, best = 64-bit (steps << 32 | id) lowered with a global atomic min, ignore bits by climbing
//              the new parents from every hit with 64-bit atomic OR
// Every stage body is a __device__ function of (its data, the index of its workgroup or thread within ONE tree), shared by two
// kernels: k_retain_X, whose grid is that tree (lqrrt_tree_retain), and k_retain_X_multi, whose grid spans the trees of a whole
// call (lqrrt_tree_retain_multi) -- a workgroup finds its tree as in multi.hpp: from the ascending prefix table of workgroup
// counts in the arguments (multi_engine_of); it reads P / g / r / tv from that engine's device-resident EngineProto and root, old
// size, revalidate flag and the engine's slices of the scratch from a RetainDesc in device memory.  Per tree the result is the
// same bit for bit (tests/test_retain_multi_gpu.py).

// One node of the pointer-doubling rounds: `jump` is an ancestor (or the node itself once it is a terminal: the new root, or a
// node below it in id order, which no kept node descends from), `ok` = every node from this one up to, not including, `jump`
// passed its check, `steps` = their edge lengths summed.
struct alignas(16) RetainLink { int jump, ok, steps, pad; };

// counters of one retain (device -> host in one copy)
struct RetainOut {
    unsigned long long best;      // (steps << 32 | new id) of the best goal hit; ~0 = none
    int kept, outside, infeasible, orphaned, root_feasible, hits, pad0, pad1;
};

constexpr int RETAIN_BLOCK = 256;

// check: block b <-> node root + b.  Block 0 (the new root) only tests the last row of its edge (RetainOut::root_feasible);
// a node whose parent lies below the root cannot be in the subtree and is not tested.
template <class S>
__device__ __forceinline__ void retain_check_body(const Params& P, const Geo& g, const TreeView& tv, int root, int N,
                                                  unsigned char* __restrict__ ok, RetainOut* __restrict__ out, double* geo_lds, int blk) {
    const int lane = threadIdx.x;
    const int i = root + blk;
    if (i >= N) return;
    if (i > root && tv.pID[i] < root) { if (lane == 0) ok[i] = 0; return; }
    const GeoL gl = stage_geo(g, geo_lds, lane, 64);
    __syncthreads();
    const int len = tv.elen[i];
    const double* xe = tv.xedge + (size_t)i * tv.H * S::N;
    const double* ue = tv.uedge + (size_t)i * tv.H * S::M;
    bool good = true;
    for (int k = (i == root ? len - 1 : 0); k < len && good; ++k) {
        double x[S::N], u[S::M], trig[2 * S::NW + 1];
#pragma unroll
        for (int d = 0; d < S::N; ++d) x[d] = xe[(size_t)k * S::N + d];
#pragma unroll
        for (int j = 0; j < S::M; ++j) u[j] = ue[(size_t)k * S::M + j];
        trig_of<S>(x, trig);
        good = S::feasible(P.p, g, gl, x, u, trig, lane);
    }
    if (lane == 0) {
        if (i == root) { out->root_feasible = good ? 1 : 0; ok[i] = 1; }
        else ok[i] = good ? 1 : 0;
    }
}
template <class S>
__global__ __launch_bounds__(64) void k_retain_check(Params P, Geo g, TreeView tv, int root, int N, unsigned char* __restrict__ ok,
                                                     RetainOut* __restrict__ out) {
    extern __shared__ double geo_lds[];
    retain_check_body<S>(P, g, tv, root, N, ok, out, geo_lds, (int)blockIdx.x);
}

// links of round 0; ok == nullptr: no revalidation, every edge passes
__device__ __forceinline__ void retain_init_body(const TreeView& tv, int root, int N, const unsigned char* __restrict__ ok,
                                                 RetainLink* __restrict__ a, int i) {
    if (i >= N) return;
    RetainLink l;
    l.pad = 0;
    if (i <= root) { l.jump = i; l.ok = 1; l.steps = 0; }
    else { l.jump = tv.pID[i]; l.ok = ok ? (int)ok[i] : 1; l.steps = tv.elen[i]; }
    a[i] = l;
}
__global__ void k_retain_init(TreeView tv, int root, int N, const unsigned char* __restrict__ ok, RetainLink* __restrict__ a) {
    retain_init_body(tv, root, N, ok, a, (int)(blockIdx.x * blockDim.x + threadIdx.x));
}

// one doubling round: b[i] = a[i] joined with a[a[i].jump].  Terminals (jump == i, ok 1, steps 0) are the identity.
__device__ __forceinline__ void retain_double_body(int N, const RetainLink* __restrict__ a, RetainLink* __restrict__ b, int i) {
    if (i >= N) return;
    RetainLink l = a[i];
    const RetainLink up = a[l.jump];
    l.ok = l.ok & up.ok;
    l.steps += up.steps;
    l.jump = up.jump;
    b[i] = l;
}
__global__ void k_retain_double(int N, const RetainLink* __restrict__ a, RetainLink* __restrict__ b) {
    retain_double_body(N, a, b, (int)(blockIdx.x * blockDim.x + threadIdx.x));
}

// keep flags + the categories of the dropped nodes, and the block-local exclusive scan of keep (first launch of the scan):
// local[i] = kept nodes of this block before i, sums[block] = kept nodes of the block.
__device__ __forceinline__ void retain_flags_body(int root, int N, const RetainLink* __restrict__ a, const unsigned char* __restrict__ ok,
                                                  unsigned char* __restrict__ keep, int* __restrict__ local, int* __restrict__ sums,
                                                  RetainOut* __restrict__ out, int blk) {
    __shared__ int sh[RETAIN_BLOCK];
    __shared__ int cnt[3];
    const int t = threadIdx.x, i = blk * RETAIN_BLOCK + t;
    if (t < 3) cnt[t] = 0;
    __syncthreads();
    int k = 0;
    if (i < N) {
        const RetainLink l = a[i];
        const bool insub = l.jump == root;                   // (the root itself: jump == root)
        const bool own = i == root || !ok || ok[i];
        k = (insub && l.ok) ? 1 : 0;
        keep[i] = (unsigned char)k;
        if (!insub) atomicAdd(&cnt[0], 1);
        else if (!own) atomicAdd(&cnt[1], 1);
        else if (!k) atomicAdd(&cnt[2], 1);
    }
    sh[t] = k;
    __syncthreads();
    for (int off = 1; off < RETAIN_BLOCK; off <<= 1) {
        const int v = t >= off ? sh[t - off] : 0;
        __syncthreads();
        sh[t] += v;
        __syncthreads();
    }
    if (i < N) local[i] = sh[t] - k;
    if (t == RETAIN_BLOCK - 1) sums[blk] = sh[t];
    if (t == 0) {
        if (cnt[0]) atomicAdd(&out->outside, cnt[0]);
        if (cnt[1]) atomicAdd(&out->infeasible, cnt[1]);
        if (cnt[2]) atomicAdd(&out->orphaned, cnt[2]);
    }
}
__global__ __launch_bounds__(RETAIN_BLOCK) void k_retain_flags(int root, int N, const RetainLink* __restrict__ a,
                                                               const unsigned char* __restrict__ ok, unsigned char* __restrict__ keep,
                                                               int* __restrict__ local, int* __restrict__ sums,
                                                               RetainOut* __restrict__ out) {
    retain_flags_body(root, N, a, ok, keep, local, sums, out, (int)blockIdx.x);
}

// second launch of the scan: exclusive scan of the block sums in place, by ONE workgroup that walks them in tiles of its
// size carrying the running total; out->kept = the total.
__device__ __forceinline__ void retain_scan_sums_body(int nblocks, int* __restrict__ sums, RetainOut* __restrict__ out) {
    __shared__ int sh[RETAIN_BLOCK];
    const int t = threadIdx.x;
    int carry = 0;
    for (int base = 0; base < nblocks; base += RETAIN_BLOCK) {
        const int idx = base + t;
        const int v = idx < nblocks ? sums[idx] : 0;
        sh[t] = v;
        __syncthreads();
        for (int off = 1; off < RETAIN_BLOCK; off <<= 1) {
            const int w = t >= off ? sh[t - off] : 0;
            __syncthreads();
            sh[t] += w;
            __syncthreads();
        }
        if (idx < nblocks) sums[idx] = carry + sh[t] - v;
        carry += sh[RETAIN_BLOCK - 1];
        __syncthreads();
    }
    if (t == 0) out->kept = carry;
}
__global__ __launch_bounds__(RETAIN_BLOCK) void k_retain_scan_sums(int nblocks, int* __restrict__ sums, RetainOut* __restrict__ out) {
    if (blockIdx.x != 0) return;
    retain_scan_sums_body(nblocks, sums, out);
}

// third launch: new id of every node (-1 = dropped), and the small per-node arrays of the new tree gathered by it:
// parents (remapped; the root's -1), edge lengths (the root's 1), step counts from the new root (its 1 included).
__device__ __forceinline__ void retain_ids_body(const TreeView& tv, int root, int N, const unsigned char* __restrict__ keep,
                                                const int* __restrict__ local, const int* __restrict__ sums,
                                                const RetainLink* __restrict__ a, int* __restrict__ newid, int* __restrict__ nelen,
                                                int* __restrict__ nsteps, int blk) {
    const int i = blk * RETAIN_BLOCK + threadIdx.x;
    if (i >= N) return;
    if (!keep[i]) { newid[i] = -1; return; }
    const int id = sums[blk] + local[i];
    newid[i] = id;
    nelen[id] = i == root ? 1 : tv.elen[i];
    nsteps[id] = a[i].steps + 1;
}
__global__ __launch_bounds__(RETAIN_BLOCK) void k_retain_ids(TreeView tv, int root, int N, const unsigned char* __restrict__ keep,
                                                             const int* __restrict__ local, const int* __restrict__ sums,
                                                             const RetainLink* __restrict__ a, int* __restrict__ newid,
                                                             int* __restrict__ nelen, int* __restrict__ nsteps) {
    retain_ids_body(tv, root, N, keep, local, sums, a, newid, nelen, nsteps, (int)blockIdx.x);
}
__device__ __forceinline__ void retain_parents_body(const TreeView& tv, int root, int N, const int* __restrict__ newid,
                                                    int* __restrict__ npid, int i) {
    if (i >= N) return;
    const int id = newid[i];
    if (id < 0) return;
    npid[id] = i == root ? -1 : newid[tv.pID[i]];            // (a kept node's parent is kept)
}
__global__ void k_retain_parents(TreeView tv, int root, int N, const int* __restrict__ newid, int* __restrict__ npid) {
    retain_parents_body(tv, root, N, newid, npid, (int)(blockIdx.x * blockDim.x + threadIdx.x));
}

// move, first half: `w` doubles per node from src[old id] to dst[new id].  per > 0: the pool holds edges, `per` doubles per
// recorded row, and only the first elen[i] * per doubles of a node are live (the rest is never read: not moved).
// One wavefront per old node.
__device__ __forceinline__ void retain_gather_body(const double* __restrict__ src, double* __restrict__ dst, const int* __restrict__ newid,
                                                   const int* __restrict__ elen, int N, int w, int per, int i) {
    if (i >= N) return;
    const int id = newid[i];
    if (id < 0) return;
    const int cnt = per ? elen[i] * per : w;
    const double* s = src + (size_t)i * w;
    double* d = dst + (size_t)id * w;
    for (int q = threadIdx.x; q < cnt; q += 64) d[q] = s[q];
}
__global__ __launch_bounds__(64) void k_retain_gather(const double* __restrict__ src, double* __restrict__ dst, const int* __restrict__ newid,
                                                      const int* __restrict__ elen, int N, int w, int per) {
    retain_gather_body(src, dst, newid, elen, N, w, per, (int)blockIdx.x);
}
// second half: back from the scratch into the pool, by new id (nelen: the NEW edge lengths)
__device__ __forceinline__ void retain_scatter_body(const double* __restrict__ src, double* __restrict__ dst, const int* __restrict__ nelen,
                                                    int kept, int w, int per, int id) {
    if (id >= kept) return;
    const int cnt = per ? nelen[id] * per : w;
    const double* s = src + (size_t)id * w;
    double* d = dst + (size_t)id * w;
    for (int q = threadIdx.x; q < cnt; q += 64) d[q] = s[q];
}
__global__ __launch_bounds__(64) void k_retain_scatter(const double* __restrict__ src, double* __restrict__ dst, const int* __restrict__ nelen,
                                                       int kept, int w, int per) {
    retain_scatter_body(src, dst, nelen, kept, w, per, (int)blockIdx.x);
}
// one component of an SoA table (one double per node): thread per node
__device__ __forceinline__ void retain_gather1_body(const double* __restrict__ src, double* __restrict__ dst, const int* __restrict__ newid,
                                                    int N, int i) {
    if (i >= N) return;
    const int id = newid[i];
    if (id >= 0) dst[id] = src[i];
}
__global__ void k_retain_gather1(const double* __restrict__ src, double* __restrict__ dst, const int* __restrict__ newid, int N) {
    retain_gather1_body(src, dst, newid, N, (int)(blockIdx.x * blockDim.x + threadIdx.x));
}

// the new root's edge: one row, its state with zero effort (tree.py:69-70)
__device__ __forceinline__ void retain_root_edge_body(const TreeView& tv, int n, int m) {
    const int t = threadIdx.x;
    if (t < n) tv.xedge[t] = tv.state[(size_t)t * tv.cap];
    if (t < m) tv.uedge[t] = 0.0;
}
__global__ void k_retain_root_edge(TreeView tv, int n, int m) {
    if (blockIdx.x != 0) return;
    retain_root_edge_body(tv, n, m);
}

// node i lies strictly inside the goal box (planner.py:442-447)
template <class S>
__device__ __forceinline__ bool goal_hit(const TreeView& tv, const Res& r, int i) {
    bool in = true;
#pragma unroll
    for (int d = 0; d < S::N; ++d) {
        const double x = tv.state[(size_t)d * tv.cap + i];
        in = in && (r.goal_lo[d] < x) && (x < r.goal_hi[d]);
    }
    return in;
}

// goal: thread per kept non-root node of the NEW tree.  ign: a zeroed bitmap of the new tree.
template <class S>
__device__ __forceinline__ void retain_goal_body(const TreeView& tv, const Res& r, int kept, const int* __restrict__ npid,
                                                 const int* __restrict__ nsteps, unsigned long long* __restrict__ ign,
                                                 RetainOut* __restrict__ out, int k) {
    if (k >= kept || !goal_hit<S>(tv, r, k)) return;
    atomicAdd(&out->hits, 1);
    atomicMin(&out->best, ((unsigned long long)(unsigned)nsteps[k] << 32) | (unsigned long long)(unsigned)k);
    // the hit's root path joins the ignore set (planner.py:270).  A climber may stop at a bit that is already set: whoever
    // set it goes on to the root.
    for (int v = k; v != -1; v = npid[v]) {
        const unsigned long long bit = 1ull << (v & 63);
        if (atomicOr(&ign[v >> 6], bit) & bit) break;
    }
}
template <class S>
__global__ void k_retain_goal(TreeView tv, Res r, int kept, const int* __restrict__ npid, const int* __restrict__ nsteps,
                              unsigned long long* __restrict__ ign, RetainOut* __restrict__ out) {
    retain_goal_body<S>(tv, r, kept, npid, nsteps, ign, out, (int)(1 + blockIdx.x * blockDim.x + threadIdx.x));
}

// ------------------------------------------------------------------------------------------
// The same stages for SEVERAL trees per launch (lqrrt_tree_retain_multi; update_plans jobs with a `root`).  One retain is ~45
// small dependent launches whose kernels are a minority of the call at 10^4 nodes: a fleet that replans every tick would pay them
// once per vehicle, one after another.  Here every stage is ONE launch whatever the number of trees, as in multi.hpp.
// What a workgroup needs beyond the engine's prototype -- per call, per engine -- is in device memory too, so the argument
// block stays at the pointer table, one pointer and the prefix table (~400 bytes).
struct RetainDesc {
    RetainLink* link[2];          // the two parities of the doubling rounds
    unsigned char *ok, *keep;
    int *local, *sums, *newid, *nelen, *npid, *nsteps;
    unsigned long long* ign;      // zeroed bitmap of the new tree
    RetainOut* out;
    double* big;                  // the engine's slice of the big scratch (set by the host before the moves)
    int root, N, revalidate, nblocks, has_goal, moves, pad0, pad1;      // moves: kept < N (known after the scan)
};
struct RetainGrid { int n, pad; int block0[MULTI_MAX + 2]; };      // block0 ascending, block0[n] = the grid size

#define RETAIN_MULTI_PROLOGUE                                             \
    const int e = multi_engine_of(gr.block0, gr.n, (int)blockIdx.x);      \
    const RetainDesc& d = ds[e];                                          \
    const int blk = (int)blockIdx.x - gr.block0[e];                       \
    const EngineProto& p = *pt.p[e];                                      \
    (void)p; (void)blk

template <class S>
__global__ __launch_bounds__(64) void k_retain_check_multi(ProtoTable pt, const RetainDesc* __restrict__ ds, RetainGrid gr) {
    extern __shared__ double geo_lds[];                          // (the launch reserves the largest geo_lds_bytes of the call)
    RETAIN_MULTI_PROLOGUE;
    if (!d.revalidate) return;
    retain_check_body<S>(p.P, p.g, p.tv, d.root, d.N, d.ok, d.out, geo_lds, blk);
}
__global__ __launch_bounds__(RETAIN_BLOCK) void k_retain_init_multi(ProtoTable pt, const RetainDesc* __restrict__ ds, RetainGrid gr) {
    RETAIN_MULTI_PROLOGUE;
    retain_init_body(p.tv, d.root, d.N, d.revalidate ? d.ok : (const unsigned char*)nullptr, d.link[0], blk * RETAIN_BLOCK + (int)threadIdx.x);
}
// One round for every tree of the call: link[from] -> link[from ^ 1].  The host runs ceil(log2(max N)) rounds for the whole call;
// a smaller tree's links are at their terminals after ceil(log2(its N)) of them, and joining with a terminal (jump == itself,
// ok 1, steps 0) is the identity, so the extra rounds leave its links as they are.
__global__ __launch_bounds__(RETAIN_BLOCK) void k_retain_double_multi(ProtoTable pt, const RetainDesc* __restrict__ ds, RetainGrid gr, int from) {
    RETAIN_MULTI_PROLOGUE;
    retain_double_body(d.N, d.link[from], d.link[from ^ 1], blk * RETAIN_BLOCK + (int)threadIdx.x);
}
__global__ __launch_bounds__(RETAIN_BLOCK) void k_retain_flags_multi(ProtoTable pt, const RetainDesc* __restrict__ ds, RetainGrid gr, int fin) {
    RETAIN_MULTI_PROLOGUE;
    if (blk >= d.nblocks) return;
    retain_flags_body(d.root, d.N, d.link[fin], d.revalidate ? d.ok : (const unsigned char*)nullptr, d.keep, d.local, d.sums, d.out, blk);
}
// one workgroup per tree
__global__ __launch_bounds__(RETAIN_BLOCK) void k_retain_scan_sums_multi(const RetainDesc* __restrict__ ds, int n) {
    if ((int)blockIdx.x >= n) return;
    const RetainDesc& d = ds[blockIdx.x];
    retain_scan_sums_body(d.nblocks, d.sums, d.out);
}
__global__ __launch_bounds__(RETAIN_BLOCK) void k_retain_ids_multi(ProtoTable pt, const RetainDesc* __restrict__ ds, RetainGrid gr, int fin) {
    RETAIN_MULTI_PROLOGUE;
    if (blk >= d.nblocks) return;
    retain_ids_body(p.tv, d.root, d.N, d.keep, d.local, d.sums, d.link[fin], d.newid, d.nelen, d.nsteps, blk);
}
__global__ __launch_bounds__(RETAIN_BLOCK) void k_retain_parents_multi(ProtoTable pt, const RetainDesc* __restrict__ ds, RetainGrid gr) {
    RETAIN_MULTI_PROLOGUE;
    retain_parents_body(p.tv, d.root, d.N, d.newid, d.npid, blk * RETAIN_BLOCK + (int)threadIdx.x);
}

// The moves.  A tree that keeps every node (kept == N: root 0, nothing dropped) moves nothing: its workgroups leave.
// SoA tables (which = 0: state, 1: trig): blockIdx.y = the component, all components of a table through the scratch at once,
// component c at big + c * kept.
__device__ __forceinline__ double* retain_soa_table(const TreeView& tv, int which) { return which == 0 ? tv.state : tv.trig; }
__global__ __launch_bounds__(RETAIN_BLOCK) void k_retain_gather1_multi(ProtoTable pt, const RetainDesc* __restrict__ ds, RetainGrid gr, int which) {
    RETAIN_MULTI_PROLOGUE;
    if (!d.moves) return;
    const size_t c = blockIdx.y;
    retain_gather1_body(retain_soa_table(p.tv, which) + c * p.tv.cap, d.big + c * (size_t)d.out->kept, d.newid, d.N,
                        blk * RETAIN_BLOCK + (int)threadIdx.x);
}
// back into the table by new id (lqrrt_tree_retain: a device-to-device copy per component)
__global__ __launch_bounds__(RETAIN_BLOCK) void k_retain_scatter1_multi(ProtoTable pt, const RetainDesc* __restrict__ ds, RetainGrid gr, int which) {
    RETAIN_MULTI_PROLOGUE;
    if (!d.moves) return;
    const size_t c = blockIdx.y;
    const int kept = d.out->kept, id = blk * RETAIN_BLOCK + (int)threadIdx.x;
    if (id < kept) retain_soa_table(p.tv, which)[c * p.tv.cap + id] = d.big[c * (size_t)kept + id];
}
// AoS pools (which = 0: K, 1: xedge, 2: uedge), one wavefront per old node / per kept node
__device__ __forceinline__ double* retain_aos_pool(const TreeView& tv, int which) { return which == 0 ? tv.K : which == 1 ? tv.xedge : tv.uedge; }
__global__ __launch_bounds__(64) void k_retain_gather_multi(ProtoTable pt, const RetainDesc* __restrict__ ds, RetainGrid gr, int which, int w, int per) {
    RETAIN_MULTI_PROLOGUE;
    if (!d.moves) return;
    retain_gather_body(retain_aos_pool(p.tv, which), d.big, d.newid, p.tv.elen, d.N, w, per, blk);      // (the OLD edge lengths)
}
__global__ __launch_bounds__(64) void k_retain_scatter_multi(ProtoTable pt, const RetainDesc* __restrict__ ds, RetainGrid gr, int which, int w, int per) {
    RETAIN_MULTI_PROLOGUE;
    if (!d.moves) return;
    retain_scatter_body(d.big, retain_aos_pool(p.tv, which), d.nelen, d.out->kept, w, per, blk);
}
// parents and edge lengths of the new tree (lqrrt_tree_retain: two device-to-device copies); a tree that moved nothing only takes
// its root's new edge length.  Last of the moves: the edge gathers read the old lengths.
__global__ __launch_bounds__(RETAIN_BLOCK) void k_retain_small_multi(ProtoTable pt, const RetainDesc* __restrict__ ds, RetainGrid gr) {
    RETAIN_MULTI_PROLOGUE;
    const int id = blk * RETAIN_BLOCK + (int)threadIdx.x;
    if (!d.moves) { if (id == 0) p.tv.elen[0] = d.nelen[0]; return; }
    if (id >= d.out->kept) return;
    p.tv.pID[id] = d.npid[id];
    p.tv.elen[id] = d.nelen[id];
}
// one workgroup per tree
__global__ __launch_bounds__(64) void k_retain_root_edge_multi(ProtoTable pt, int n_engines, int n, int m) {
    if ((int)blockIdx.x >= n_engines) return;
    retain_root_edge_body(pt.p[blockIdx.x]->tv, n, m);
}
template <class S>
__global__ __launch_bounds__(RETAIN_BLOCK) void k_retain_goal_multi(ProtoTable pt, const RetainDesc* __restrict__ ds, RetainGrid gr) {
    RETAIN_MULTI_PROLOGUE;
    if (!d.has_goal) return;
    retain_goal_body<S>(p.tv, p.r, d.out->kept, d.npid, d.nsteps, d.ign, d.out, 1 + blk * RETAIN_BLOCK + (int)threadIdx.x);
}
#undef RETAIN_MULTI_PROLOGUE
