// clear_rects_wait.hpp -- clear_wait.hpp's query (W departure delays at once, every answer a 64-bit mask over the delays) against
// moving oriented RECTANGLES (lqrrt_tree_clear_rects_wait, Planner.avoid_rects with max_wait).  Reads the tree, writes nothing of
// it.  Fragment of kernels.hpp (included there behind clear_rects.hpp, inside namespace lq).  The rule is clear_wait.hpp's word
// for word -- wait, edges, root path, dwell, best -- with "the row test" read as clear_rects.hpp's: the hull points of the row's
// pose (the novice boats: its centre, against inflated extents) in the rectangles of its instant, the edge included, geometry
// only.  tests/clear_rects_wait_reference.py restates it in NumPy as W runs of tests/clear_rects_reference.py.  So bit w of
// clear[i] is (first[i] == -1 of lqrrt_tree_clear_rects at start + w) && root_ok bit w, and bit w of dwell_ok[i] is
// dwell[i] == -1 of that call.
//
// Execution: clear_wait.hpp's stages; only the check is this file's.  The steps (retain_links), the propagate rounds
// (k_clear_init / k_clear_double<ClearWaitLink>) and the select (k_clear_wait_select) are the existing kernels, unchanged.
// The check has clear_wait_check_body's shape -- one workgroup of four wavefronts per node, wavefront q owns the delays
// q, q + 4, ..., the partial masks and the latest dwell failure are joined through LDS -- and its three savings: (a) a row is
// loaded once for the delays still alive and the rows end when none is, (b) the delays whose instant is clamped to L - 1 share one
// test, (c) the dwell test descends from L - 1 once for all delays.  The row test is clear_rects_hit<S> as it stands, a
// whole-wavefront function; every branch round it depends on the wavefront's own mask, the node and the launch's arguments alone.
// The table is clear_rects.hpp's: [L][D][4], then [D][4].  The extents stay in it: clear_rects_hit reads a', b', rp of its
// rectangles at every call (96 bytes a lane tile that every wavefront of the device shares, a cache line or two), and holding
// them across rows and delays would take a second copy of that function; DESIGN.md section 22 gives the compiler's figures.

template <class S>
__device__ __forceinline__ void clear_rects_wait_check_body(const Geo& g, const TreeView& tv, const Res& r, int N,
                                                            const RetainLink* __restrict__ link, const double* __restrict__ table,
                                                            int L, int D, int start, int W, unsigned long long* __restrict__ own_ok,
                                                            unsigned long long* __restrict__ dwell_ok, int* __restrict__ hit,
                                                            double* hull_lds, int i) {
    __shared__ unsigned long long part[CLEAR_WAIT_WAVES];
    __shared__ int fail[CLEAR_WAIT_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;  // (every wavefront's control flow below is uniform)
    if (i >= N) return;
    clear_stage_hull(g, hull_lds, tid, CLEAR_WAIT_BLOCK);
    __syncthreads();
    const unsigned long long all = clear_wait_all(W);
    const unsigned long long mine = (0x1111111111111111ull << q) & all;     // the delays of this wavefront
    const int len = tv.elen[i];
    const double* xe = tv.xedge + (size_t)i * tv.H * S::N;
    const double* ue = tv.uedge + (size_t)i * tv.H * S::M;
    const double* ext = table + (size_t)L * D * 4;
    double x[S::N], u[S::M], trig[2 * S::NW + 1];
    auto load = [&](int k) { clear_load_row<S>(xe, ue, k, x, u, trig); };
    // the loaded row against the rectangles of table row t
    auto hits = [&](int t) { return clear_rects_hit<S>(table + (size_t)t * D * 4, ext, D, hull_lds, g.V, g.hbb, x[0], x[1], trig[0], trig[1], lane); };
    // time index of row 0 at delay 0 (the root: of its last row, the only one it has as a seed)
    const int base = i == 0 ? start : start + link[tv.pID[i]].steps + tv.elen[0];
    unsigned long long alive = mine;
    // the root: its one row at tau = start + w, bit w of `alive` = that instant passes (the prefix is taken when the parts are
    // joined); any other node: its rows in order
    const int k0 = i == 0 ? len - 1 : 0;
    for (int k = k0; k < len && alive; ++k) {                    // (a)
        load(k);
        const int at = i == 0 ? base : base + k;
        for (unsigned long long m = alive; m; m &= m - 1) {
            const int tau = at + __builtin_ctzll(m);
            if (tau >= L - 1) {                                  // (b): m holds this delay and the alive ones above it
                if (hits(L - 1)) alive &= ~m;
                break;
            }
            if (hits(tau)) alive &= ~(m & (~m + 1ull));
        }
    }
    // a goal hit waits at its last row: (c)
    const bool in = goal_hit<S>(tv, r, i) && i > 0;             // (the root is no hit; its state is read all the same, as ever)
    const int arrive = base + len;                               // start + cum[i]: the first instant of the wait at delay 0
    int tstar = -1;
    if (in) {
        load(len - 1);
        for (int tau = L - 1 - q; tau >= arrive; tau -= CLEAR_WAIT_WAVES)
            if (hits(tau)) { tstar = tau; break; }
    }
    if (lane == 0) { part[q] = alive; fail[q] = tstar; }
    __syncthreads();
    if (tid == 0) {
        unsigned long long ok = 0;
        int ts = -1;
#pragma unroll
        for (int j = 0; j < CLEAR_WAIT_WAVES; ++j) { ok |= part[j]; ts = fail[j] > ts ? fail[j] : ts; }
        if (i == 0) {                                            // root_ok: the delays below the first instant that fails
            const unsigned long long bad = ~ok;
            ok = bad ? ((1ull << __builtin_ctzll(bad)) - 1ull) & all : all;
        }
        unsigned long long dw = 0;
        if (in) {
            const long long s = (long long)ts - arrive + 1;      // the first delay that arrives after t*
            dw = ts < 0 ? all : (s >= W ? 0ull : all & ~((1ull << s) - 1ull));
        }
        own_ok[i] = ok; dwell_ok[i] = dw; hit[i] = in ? 1 : 0;
    }
}
template <class S>
__global__ __launch_bounds__(CLEAR_WAIT_BLOCK) void k_clear_rects_wait_check(Geo g, TreeView tv, Res r, int N,
                                                                             const RetainLink* __restrict__ link,
                                                                             const double* __restrict__ table, int L, int D, int start,
                                                                             int W, unsigned long long* __restrict__ own_ok,
                                                                             unsigned long long* __restrict__ dwell_ok, int* __restrict__ hit) {
    extern __shared__ double hull_lds[];
    if constexpr (has_discs<S>::value)
        clear_rects_wait_check_body<S>(g, tv, r, N, link, table, L, D, start, W, own_ok, dwell_ok, hit, hull_lds, (int)blockIdx.x);
}
