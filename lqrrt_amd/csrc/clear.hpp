// clear.hpp -- time-indexed clearance of the tree against moving discs (lqrrt_tree_clear, Planner.avoid): which nodes' root paths
// stay clear of D discs whose positions are given at L consecutive instants, and the best goal hit among them.  Reads the tree,
// writes nothing of it.  Fragment of kernels.hpp (included there, in order, inside namespace lq).
// The rule is restated in plain NumPy in tests/clear_reference.py; in short, for a tree of N nodes (root 0, pID[i] < i):
//   cum[0] = elen[0], cum[i] = cum[pID[i]] + elen[i]; row k of node i > 0 has time index tau = start + cum[pID[i]] + k, the root's
//     (last) row tau = start; at tau the discs stand at row min(tau, L - 1) of the track table
//   own[i]   = the smallest tau of a row of node i's edge that fails S::feasible against the discs of that instant (no other
//              obstacle, no occupancy grid), or -1
//   first[i] = the smallest own >= 0 over the nodes from i up to and including the root, or -1
//   dwell[i] = for a goal hit (a non-root node strictly inside the goal box): the smallest tau' in (start + cum[i] - 1, L - 1] at
//              which its last row fails against the discs of tau', or -1; -2 for every other node
//   best     = the hit with first == -1 and dwell == -1 of the smallest (cum << 32 | id)
//
// Execution: plain launches, one after another on one stream -- no grid-wide barrier, no flag another workgroup waits for.
//   steps      cum by the pointer doubling of retain.hpp (k_retain_init / k_retain_double with root 0 and no ok table)
//   check      one wavefront per node, rows in order up to the first failing one, the lanes split the hull x disc sweep; a goal
//              hit then waits at its last row while the discs move on
//   propagate  first down the parent chains by pointer doubling (k_clear_init<ClearLink> / k_clear_double<ClearLink>),
//              ceil(log2 N) double-buffered rounds, joined by minimum with -1 as +infinity
//   select     thread per node: counters, and best lowered with a global 64-bit atomic min
//
// The disc table [L][D][4] holds per instant and disc what upload_geometry derives for a static circle -- centre x, y | exact
// threshold on the squared distance | padded radius -- so that a disc that stands still decides bit for bit as that circle in the
// static map.  The kernel points GeoL::oc at the row of the instant (in HBM: D discs are read once per tested row) and hands
// S::feasible a Geo without an occupancy grid and with O = D: RosBoat::feasible reads both.
// hull_hits reads the hull points through an LDS address: stage_geo leaves them in HBM for an occupancy-grid engine whose hull is
// large (og_lds == 0), so the check stages the 2 V doubles itself, whatever the engine's map; the launch reserves exactly that.

// Systems whose feasible has a circle path (hull_hits, or the novice boats' centre test) declare DISCS.
template <class S, class = void> struct has_discs : std::false_type {};
template <class S> struct has_discs<S, std::enable_if_t<S::DISCS>> : std::true_type {};

// One node of the propagate rounds: `jump` is an ancestor (the root: itself), `first` the smallest failing time index over the
// nodes from this one up to AND INCLUDING `jump`, or -1.  (Inclusive, unlike RetainLink: the root's own row counts, and a chain
// of 2^k nodes reaches the root in its last round.)  A link type names the field it carries (Val, FIELD) and how two are joined: an
// idempotent join, so that the root (jump == itself) is the identity.  Here: the minimum with -1 as +infinity.
struct alignas(8) ClearLink {
    typedef int Val;
    int jump, first;
    static constexpr int ClearLink::* FIELD = &ClearLink::first;
    __device__ static int join(int a, int b) { return a < 0 ? b : (b < 0 ? a : (a < b ? a : b)); }
};

// counters of one call (device -> host in one copy)
struct ClearOut {
    unsigned long long best;      // (cum << 32 | id) of the best clear goal hit; ~0 = none
    int conflicts, blocked, hits, clear_hits;
};

constexpr int CLEAR_BLOCK = 256;

// What the two checks (this one and clear_wait.hpp's) share.  The hull points into LDS by `stride` threads, of which this is
// `tid`; the caller's __syncthreads() follows.
__device__ __forceinline__ void clear_stage_hull(const Geo& g, double* hull_lds, int tid, int stride) {
    for (int q = tid; q < 2 * g.V; q += stride) hull_lds[q] = g.vps[q];
}
// gd (the caller's copy of g) and gl for a test in which the D discs of one instant (gl.oc, set per row) are the whole world
__device__ __forceinline__ void clear_disc_world(const Geo& g, double* hull_lds, int D, Geo& gd, GeoL& gl) {
    gd.og = nullptr; gd.O = D;
    gl.vps = hull_lds; gl.V = g.V; gl.O = D;
#pragma unroll
    for (int k = 0; k < 4; ++k) gl.bb[k] = g.hbb[k];
}
// row k of an edge
template <class S>
__device__ __forceinline__ void clear_load_row(const double* xe, const double* ue, int k, double* x, double* u, double* trig) {
#pragma unroll
    for (int d = 0; d < S::N; ++d) x[d] = xe[(size_t)k * S::N + d];
#pragma unroll
    for (int j = 0; j < S::M; ++j) u[j] = ue[(size_t)k * S::M + j];
    trig_of<S>(x, trig);
}

// check: block i <-> node i.  `link` holds the finished step sums (RetainLink::steps = cum - elen[0]).
template <class S>
__device__ __forceinline__ void clear_check_body(const Params& P, const Geo& g, const TreeView& tv, const Res& r, int N,
                                                 const RetainLink* __restrict__ link, const double* __restrict__ table, int L, int D,
                                                 int start, int* __restrict__ own, int* __restrict__ dwell, double* hull_lds, int i) {
    const int lane = threadIdx.x;
    if (i >= N) return;
    clear_stage_hull(g, hull_lds, lane, 64);
    __syncthreads();
    Geo gd = g;
    GeoL gl;
    clear_disc_world(g, hull_lds, D, gd, gl);
    const int len = tv.elen[i];
    const double* xe = tv.xedge + (size_t)i * tv.H * S::N;
    const double* ue = tv.uedge + (size_t)i * tv.H * S::M;
    // time index of row 0 (the root: of its last row, the only one it has as a seed)
    const int k0 = i == 0 ? len - 1 : 0;
    const int base = i == 0 ? start - k0 : start + link[tv.pID[i]].steps + tv.elen[0];
    int first = -1;
    double x[S::N], u[S::M], trig[2 * S::NW + 1];
    for (int k = k0; k < len && first < 0; ++k) {
        clear_load_row<S>(xe, ue, k, x, u, trig);
        const int tau = base + k;
        gl.oc = table + (size_t)(tau < L - 1 ? tau : L - 1) * D * 4;
        if (!S::feasible(P.p, gd, gl, x, u, trig, lane)) first = tau;
    }
    // a goal hit waits at its last row (x, u, trig hold it when no row failed; when one did, the hit is not clear anyway, but
    // dwell is defined on the last row all the same: load it again)
    const bool in = goal_hit<S>(tv, r, i) && i > 0;             // (the root is no hit; its state is read all the same, as ever)
    int dw = -2;
    if (in) {
        dw = -1;
        if (first >= 0) clear_load_row<S>(xe, ue, len - 1, x, u, trig);
        for (int tau = base + len; tau <= L - 1 && dw < 0; ++tau) {      // (base + len - 1 = start + cum[i] - 1: the arrival)
            gl.oc = table + (size_t)tau * D * 4;
            if (!S::feasible(P.p, gd, gl, x, u, trig, lane)) dw = tau;
        }
    }
    if (lane == 0) { own[i] = first; dwell[i] = dw; }
}
template <class S>
__global__ __launch_bounds__(64) void k_clear_check(Params P, Geo g, TreeView tv, Res r, int N, const RetainLink* __restrict__ link,
                                                    const double* __restrict__ table, int L, int D, int start, int* __restrict__ own,
                                                    int* __restrict__ dwell) {
    extern __shared__ double hull_lds[];
    if constexpr (has_discs<S>::value) clear_check_body<S>(P, g, tv, r, N, link, table, L, D, start, own, dwell, hull_lds, (int)blockIdx.x);
}

// links of round 0: a node and its parent
template <class Link>
__global__ void k_clear_init(TreeView tv, int N, const typename Link::Val* __restrict__ own, Link* __restrict__ a) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= N) return;
    Link l{};
    if (i == 0) { l.jump = 0; l.*Link::FIELD = own[0]; }
    else { l.jump = tv.pID[i]; l.*Link::FIELD = Link::join(own[i], own[l.jump]); }
    a[i] = l;
}

// one doubling round: b[i] = a[i] joined with a[a[i].jump]
template <class Link>
__global__ void k_clear_double(int N, const Link* __restrict__ a, Link* __restrict__ b) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= N) return;
    Link l = a[i];
    const Link up = a[l.jump];
    l.*Link::FIELD = Link::join(l.*Link::FIELD, up.*Link::FIELD);
    l.jump = up.jump;
    b[i] = l;
}

// select: thread per node.  first_out[i] = the finished first; the counters go through the workgroup's LDS, best through a
// global atomic min on the key of k_retain_goal.
__device__ __forceinline__ void clear_select_body(const TreeView& tv, int N, const int* __restrict__ own, const int* __restrict__ dwell,
                                                  const ClearLink* __restrict__ a, const RetainLink* __restrict__ link,
                                                  int* __restrict__ first_out, ClearOut* __restrict__ out, int blk) {
    __shared__ int cnt[4];
    const int t = threadIdx.x, i = blk * CLEAR_BLOCK + t;
    if (t < 4) cnt[t] = 0;
    __syncthreads();
    if (i < N) {
        const int f = a[i].first, o = own[i], dw = dwell[i];
        first_out[i] = f;
        if (o >= 0) atomicAdd(&cnt[0], 1);
        else if (f >= 0) atomicAdd(&cnt[1], 1);
        if (dw != -2) {
            atomicAdd(&cnt[2], 1);
            if (f == -1 && dw == -1) {
                atomicAdd(&cnt[3], 1);
                const unsigned cum = (unsigned)(link[i].steps + tv.elen[0]);
                atomicMin(&out->best, ((unsigned long long)cum << 32) | (unsigned long long)(unsigned)i);
            }
        }
    }
    __syncthreads();
    if (t == 0) {
        if (cnt[0]) atomicAdd(&out->conflicts, cnt[0]);
        if (cnt[1]) atomicAdd(&out->blocked, cnt[1]);
        if (cnt[2]) atomicAdd(&out->hits, cnt[2]);
        if (cnt[3]) atomicAdd(&out->clear_hits, cnt[3]);
    }
}
__global__ __launch_bounds__(CLEAR_BLOCK) void k_clear_select(TreeView tv, int N, const int* __restrict__ own, const int* __restrict__ dwell,
                                                              const ClearLink* __restrict__ a, const RetainLink* __restrict__ link,
                                                              int* __restrict__ first_out, ClearOut* __restrict__ out) {
    clear_select_body(tv, N, own, dwell, a, link, first_out, out, (int)blockIdx.x);
}
