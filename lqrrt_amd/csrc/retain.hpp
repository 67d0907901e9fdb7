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
__global__ __launch_bounds__(64) void k_retain_check(Params P, Geo g, TreeView tv, int root, int N, unsigned char* __restrict__ ok,
                                                     RetainOut* __restrict__ out) {
    extern __shared__ double geo_lds[];
    const int lane = threadIdx.x;
    const int i = root + (int)blockIdx.x;
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

// links of round 0; ok == nullptr: no revalidation, every edge passes
__global__ void k_retain_init(TreeView tv, int root, int N, const unsigned char* __restrict__ ok, RetainLink* __restrict__ a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    RetainLink l;
    l.pad = 0;
    if (i <= root) { l.jump = i; l.ok = 1; l.steps = 0; }
    else { l.jump = tv.pID[i]; l.ok = ok ? (int)ok[i] : 1; l.steps = tv.elen[i]; }
    a[i] = l;
}

// one doubling round: b[i] = a[i] joined with a[a[i].jump].  Terminals (jump == i, ok 1, steps 0) are the identity.
__global__ void k_retain_double(int N, const RetainLink* __restrict__ a, RetainLink* __restrict__ b) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    RetainLink l = a[i];
    const RetainLink up = a[l.jump];
    l.ok = l.ok & up.ok;
    l.steps += up.steps;
    l.jump = up.jump;
    b[i] = l;
}

// keep flags + the categories of the dropped nodes, and the block-local exclusive scan of keep (first launch of the scan):
// local[i] = kept nodes of this block before i, sums[block] = kept nodes of the block.
__global__ __launch_bounds__(RETAIN_BLOCK) void k_retain_flags(int root, int N, const RetainLink* __restrict__ a,
                                                               const unsigned char* __restrict__ ok, unsigned char* __restrict__ keep,
                                                               int* __restrict__ local, int* __restrict__ sums,
                                                               RetainOut* __restrict__ out) {
    __shared__ int sh[RETAIN_BLOCK];
    __shared__ int cnt[3];
    const int t = threadIdx.x, i = blockIdx.x * RETAIN_BLOCK + t;
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
    if (t == RETAIN_BLOCK - 1) sums[blockIdx.x] = sh[t];
    if (t == 0) {
        if (cnt[0]) atomicAdd(&out->outside, cnt[0]);
        if (cnt[1]) atomicAdd(&out->infeasible, cnt[1]);
        if (cnt[2]) atomicAdd(&out->orphaned, cnt[2]);
    }
}

// second launch of the scan: exclusive scan of the block sums in place, by ONE workgroup that walks them in tiles of its
// size carrying the running total; out->kept = the total.
__global__ __launch_bounds__(RETAIN_BLOCK) void k_retain_scan_sums(int nblocks, int* __restrict__ sums, RetainOut* __restrict__ out) {
    __shared__ int sh[RETAIN_BLOCK];
    if (blockIdx.x != 0) return;
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

// third launch: new id of every node (-1 = dropped), and the small per-node arrays of the new tree gathered by it:
// parents (remapped; the root's -1), edge lengths (the root's 1), step counts from the new root (its 1 included).
__global__ __launch_bounds__(RETAIN_BLOCK) void k_retain_ids(TreeView tv, int root, int N, const unsigned char* __restrict__ keep,
                                                             const int* __restrict__ local, const int* __restrict__ sums,
                                                             const RetainLink* __restrict__ a, int* __restrict__ newid,
                                                             int* __restrict__ nelen, int* __restrict__ nsteps) {
    const int i = blockIdx.x * RETAIN_BLOCK + threadIdx.x;
    if (i >= N) return;
    if (!keep[i]) { newid[i] = -1; return; }
    const int id = sums[blockIdx.x] + local[i];
    newid[i] = id;
    nelen[id] = i == root ? 1 : tv.elen[i];
    nsteps[id] = a[i].steps + 1;
}
__global__ void k_retain_parents(TreeView tv, int root, int N, const int* __restrict__ newid, int* __restrict__ npid) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int id = newid[i];
    if (id < 0) return;
    npid[id] = i == root ? -1 : newid[tv.pID[i]];            // (a kept node's parent is kept)
}

// move, first half: `w` doubles per node from src[old id] to dst[new id].  per > 0: the pool holds edges, `per` doubles per
// recorded row, and only the first elen[i] * per doubles of a node are live (the rest is never read: not moved).
// One wavefront per old node.
__global__ __launch_bounds__(64) void k_retain_gather(const double* __restrict__ src, double* __restrict__ dst, const int* __restrict__ newid,
                                                      const int* __restrict__ elen, int N, int w, int per) {
    const int i = blockIdx.x;
    if (i >= N) return;
    const int id = newid[i];
    if (id < 0) return;
    const int cnt = per ? elen[i] * per : w;
    const double* s = src + (size_t)i * w;
    double* d = dst + (size_t)id * w;
    for (int q = threadIdx.x; q < cnt; q += 64) d[q] = s[q];
}
// second half: back from the scratch into the pool, by new id (nelen: the NEW edge lengths)
__global__ __launch_bounds__(64) void k_retain_scatter(const double* __restrict__ src, double* __restrict__ dst, const int* __restrict__ nelen,
                                                       int kept, int w, int per) {
    const int id = blockIdx.x;
    if (id >= kept) return;
    const int cnt = per ? nelen[id] * per : w;
    const double* s = src + (size_t)id * w;
    double* d = dst + (size_t)id * w;
    for (int q = threadIdx.x; q < cnt; q += 64) d[q] = s[q];
}
// one component of an SoA table (one double per node): thread per node
__global__ void k_retain_gather1(const double* __restrict__ src, double* __restrict__ dst, const int* __restrict__ newid, int N) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int id = newid[i];
    if (id >= 0) dst[id] = src[i];
}

// the new root's edge: one row, its state with zero effort (tree.py:69-70)
__global__ void k_retain_root_edge(TreeView tv, int n, int m) {
    const int t = threadIdx.x;
    if (blockIdx.x != 0) return;
    if (t < n) tv.xedge[t] = tv.state[(size_t)t * tv.cap];
    if (t < m) tv.uedge[t] = 0.0;
}

// goal: thread per kept non-root node of the NEW tree.  ign: a zeroed bitmap of the new tree.
template <class S>
__global__ void k_retain_goal(TreeView tv, Res r, int kept, const int* __restrict__ npid, const int* __restrict__ nsteps,
                              unsigned long long* __restrict__ ign, RetainOut* __restrict__ out) {
    const int k = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= kept) return;
    bool in = true;
#pragma unroll
    for (int d = 0; d < S::N; ++d) {
        const double x = tv.state[(size_t)d * tv.cap + k];
        in = in && (r.goal_lo[d] < x) && (x < r.goal_hi[d]);     // planner.py:442-447
    }
    if (!in) return;
    atomicAdd(&out->hits, 1);
    atomicMin(&out->best, ((unsigned long long)(unsigned)nsteps[k] << 32) | (unsigned long long)(unsigned)k);
    // the hit's root path joins the ignore set (planner.py:270).  A climber may stop at a bit that is already set: whoever
    // set it goes on to the root.
    for (int v = k; v != -1; v = npid[v]) {
        const unsigned long long bit = 1ull << (v & 63);
        if (atomicOr(&ign[v >> 6], bit) & bit) break;
    }
}
