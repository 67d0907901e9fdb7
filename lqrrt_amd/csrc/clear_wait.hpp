// clear_wait.hpp -- the clearance query of clear.hpp for W departure delays at once (lqrrt_tree_clear_wait, Planner.avoid with
// max_wait): the vehicle may stand on the root's row for w = 0 .. W - 1 rows of dt before it leaves, 1 <= W <= 64, and every answer
// is a 64-bit mask over w.  Reads the tree, writes nothing of it.  Fragment of kernels.hpp (included there after clear.hpp).
// The rule is restated in plain NumPy in tests/clear_wait_reference.py on top of tests/clear_reference.py; cum, tau, the clamp
// min(tau, L - 1), the row test and the goal hit are clear.hpp's.  For delay w:
//   wait       the root's row is tested at tau = start .. start + w; root_ok bit w = all of them pass (prefix-closed)
//   edges      row k of node i > 0 has tau = start + w + cum[pID[i]] + k; own_ok[i] bit w = every row of the edge passes;
//              own_ok[0] = root_ok
//   root path  clear[i] = own_ok[i] & clear[pID[i]]: the AND over the nodes from i up to and including the root
//   dwell      for a goal hit, dwell_ok[i] bit w = its last row passes at every tau' in [start + w + cum[i], L - 1] (an empty range
//              passes); 0 for every other node
//   best       over hits i and delays w set in clear[i] & dwell_ok[i]: the smallest (w + cum[i], i); of one node only its lowest
//              set bit can win
// So bit w of clear[i] is (first[i] == -1 of lqrrt_tree_clear at start + w) && root_ok bit w, and bit w of dwell_ok[i] is
// dwell[i] == -1 of that call.
//
// Execution: plain launches, one after another on one stream, as clear.hpp -- no grid-wide barrier, no flag another workgroup
// waits for.
//   steps      cum by the pointer doubling of retain.hpp, exactly as clear.hpp's
//   check      one workgroup of four wavefronts per node; wavefront q owns the delays w = q, q + 4, ...  and writes one partial
//              mask, joined through LDS
//   propagate  clear.hpp's k_clear_init / k_clear_double on 16-byte links {jump, mask} joined by AND, ceil(log2 N)
//              double-buffered rounds
//   select     thread per node: m = clear & dwell_ok, w = ctz(m); counters through LDS, best by a global 64-bit atomic min on
//              ((w + cum) << 32 | id)
//
// What keeps the check far below W runs of k_clear_check:
//   (a) a wavefront carries the mask of its delays that are still alive; row k is tested for those only, loaded once for all of
//       them, and the rows end when the mask is empty
//   (b) every delay with base + k + w >= L - 1 reads the same (last) disc row: the delays ascend, so the first such one is tested
//       and its answer applied to all that follow
//   (c) the dwell test at tau' does not depend on w: tau' descends from L - 1 to start + cum[i] (the wavefronts take every
//       fourth) and each stops at its first failure; with t* the latest failure, dwell_ok is the delays with
//       start + w + cum[i] > t*

// One node of the propagate rounds, as ClearLink: `mask` is the AND of own_ok over the nodes from this one up to and including `jump`.
struct alignas(16) ClearWaitLink {
    typedef unsigned long long Val;
    int jump, pad;
    unsigned long long mask;
    static constexpr unsigned long long ClearWaitLink::* FIELD = &ClearWaitLink::mask;
    __device__ static unsigned long long join(unsigned long long a, unsigned long long b) { return a & b; }
};

// counters of one call (device -> host in one copy)
struct ClearWaitOut {
    unsigned long long best;      // ((wait + cum) << 32 | id) of the best clear goal hit; ~0 = none
    int hits, clear_hits, clear_now, pad;
};

constexpr int CLEAR_WAIT_BLOCK = 256;                            // check and select alike
constexpr int CLEAR_WAIT_WAVES = CLEAR_WAIT_BLOCK / 64;

__device__ __forceinline__ unsigned long long clear_wait_all(int W) { return W >= 64 ? ~0ull : (1ull << W) - 1ull; }

// check: block i <-> node i.  `link` holds the finished step sums (RetainLink::steps = cum - elen[0]).
template <class S>
__device__ __forceinline__ void clear_wait_check_body(const Params& P, const Geo& g, const TreeView& tv, const Res& r, int N,
                                                      const RetainLink* __restrict__ link, const double* __restrict__ table, int L,
                                                      int D, int start, int W, unsigned long long* __restrict__ own_ok,
                                                      unsigned long long* __restrict__ dwell_ok, int* __restrict__ hit,
                                                      double* hull_lds, int i) {
    __shared__ unsigned long long part[CLEAR_WAIT_WAVES];
    __shared__ int fail[CLEAR_WAIT_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;  // (every wavefront's control flow below is uniform)
    if (i >= N) return;
    clear_stage_hull(g, hull_lds, tid, CLEAR_WAIT_BLOCK);
    __syncthreads();
    Geo gd = g;
    GeoL gl;
    clear_disc_world(g, hull_lds, D, gd, gl);
    const unsigned long long all = clear_wait_all(W);
    const unsigned long long mine = (0x1111111111111111ull << q) & all;     // the delays of this wavefront
    const int len = tv.elen[i];
    const double* xe = tv.xedge + (size_t)i * tv.H * S::N;
    const double* ue = tv.uedge + (size_t)i * tv.H * S::M;
    const double* last = table + (size_t)(L - 1) * D * 4;
    double x[S::N], u[S::M], trig[2 * S::NW + 1];
    auto load = [&](int k) { clear_load_row<S>(xe, ue, k, x, u, trig); };
    // time index of row 0 at delay 0 (the root: of its last row, the only one it has as a seed)
    const int base = i == 0 ? start : start + link[tv.pID[i]].steps + tv.elen[0];
    unsigned long long alive = mine;
    if (i == 0) {
        // the root's row at tau = start + w: bit w of `alive` = that instant passes (the prefix is taken when the parts are joined)
        load(len - 1);
        for (unsigned long long m = mine; m; m &= m - 1) {
            const int tau = base + __builtin_ctzll(m);
            if (tau >= L - 1) {                                  // (b)
                gl.oc = last;
                if (!S::feasible(P.p, gd, gl, x, u, trig, lane)) alive &= ~m;
                break;
            }
            gl.oc = table + (size_t)tau * D * 4;
            if (!S::feasible(P.p, gd, gl, x, u, trig, lane)) alive &= ~(m & (~m + 1ull));
        }
    } else {
        for (int k = 0; k < len && alive; ++k) {                 // (a)
            load(k);
            for (unsigned long long m = alive; m; m &= m - 1) {
                const int tau = base + k + __builtin_ctzll(m);
                if (tau >= L - 1) {                              // (b): m holds this delay and the alive ones above it
                    gl.oc = last;
                    if (!S::feasible(P.p, gd, gl, x, u, trig, lane)) alive &= ~m;
                    break;
                }
                gl.oc = table + (size_t)tau * D * 4;
                if (!S::feasible(P.p, gd, gl, x, u, trig, lane)) alive &= ~(m & (~m + 1ull));
            }
        }
    }
    // a goal hit waits at its last row: (c)
    const bool in = goal_hit<S>(tv, r, i) && i > 0;             // (the root is no hit; its state is read all the same, as ever)
    const int arrive = base + len;                               // start + cum[i]: the first instant of the wait at delay 0
    int tstar = -1;
    if (in) {
        load(len - 1);
        for (int tau = L - 1 - q; tau >= arrive; tau -= CLEAR_WAIT_WAVES) {
            gl.oc = table + (size_t)tau * D * 4;
            if (!S::feasible(P.p, gd, gl, x, u, trig, lane)) { tstar = tau; break; }
        }
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
__global__ __launch_bounds__(CLEAR_WAIT_BLOCK) void k_clear_wait_check(Params P, Geo g, TreeView tv, Res r, int N,
                                                                       const RetainLink* __restrict__ link,
                                                                       const double* __restrict__ table, int L, int D, int start, int W,
                                                                       unsigned long long* __restrict__ own_ok,
                                                                       unsigned long long* __restrict__ dwell_ok, int* __restrict__ hit) {
    extern __shared__ double hull_lds[];
    if constexpr (has_discs<S>::value)
        clear_wait_check_body<S>(P, g, tv, r, N, link, table, L, D, start, W, own_ok, dwell_ok, hit, hull_lds, (int)blockIdx.x);
}

// select: thread per node.  clear_out[i] = the finished mask; the counters go through the workgroup's LDS, best through a global
// atomic min.
__device__ __forceinline__ void clear_wait_select_body(const TreeView& tv, int N, const unsigned long long* __restrict__ dwell_ok,
                                                       const int* __restrict__ hit, const ClearWaitLink* __restrict__ a,
                                                       const RetainLink* __restrict__ link, unsigned long long* __restrict__ clear_out,
                                                       ClearWaitOut* __restrict__ out, int blk) {
    __shared__ int cnt[3];
    const int t = threadIdx.x, i = blk * CLEAR_WAIT_BLOCK + t;
    if (t < 3) cnt[t] = 0;
    __syncthreads();
    if (i < N) {
        const unsigned long long c = a[i].mask;
        clear_out[i] = c;
        if (hit[i]) {
            atomicAdd(&cnt[0], 1);
            const unsigned long long m = c & dwell_ok[i];
            if (m) {
                atomicAdd(&cnt[1], 1);
                if (m & 1ull) atomicAdd(&cnt[2], 1);
                const unsigned long long arrival = (unsigned long long)__builtin_ctzll(m) + (unsigned)(link[i].steps + tv.elen[0]);
                atomicMin(&out->best, (arrival << 32) | (unsigned long long)(unsigned)i);
            }
        }
    }
    __syncthreads();
    if (t == 0) {
        if (cnt[0]) atomicAdd(&out->hits, cnt[0]);
        if (cnt[1]) atomicAdd(&out->clear_hits, cnt[1]);
        if (cnt[2]) atomicAdd(&out->clear_now, cnt[2]);
    }
}
__global__ __launch_bounds__(CLEAR_WAIT_BLOCK) void k_clear_wait_select(TreeView tv, int N, const unsigned long long* __restrict__ dwell_ok,
                                                                        const int* __restrict__ hit, const ClearWaitLink* __restrict__ a,
                                                                        const RetainLink* __restrict__ link,
                                                                        unsigned long long* __restrict__ clear_out,
                                                                        ClearWaitOut* __restrict__ out) {
    clear_wait_select_body(tv, N, dwell_ok, hit, a, link, clear_out, out, (int)blockIdx.x);
}
