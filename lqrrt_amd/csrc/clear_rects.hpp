// clear_rects.hpp -- clear.hpp's query against moving oriented RECTANGLES (lqrrt_tree_clear_rects, Planner.avoid_rects): which nodes'
// root paths stay clear of D rectangles whose poses (world x, y, heading) are given at L consecutive instants, and the best goal
// hit among them.  Reads the tree, writes nothing of it.  Fragment of kernels.hpp (included there behind the clear fragments,
// inside namespace lq).  The rule is restated in plain NumPy in tests/clear_rects_reference.py.  cum, tau, the clamp
// min(tau, L - 1), own / first / dwell, best and the counters are clear.hpp's word for word, with "disc" read as "rectangle";
// only the test of one row is new, and it is geometry only:
//   the vehicle's points   the hull points vps placed as hull_hits places them, vx = px + (c bx + (-s) by), vy = py + (s bx + c by)
//                          with c, s from trig_of<S>; for the novice boats the one point (px, py).  Not the car's vertex at 2p
//                          (a quirk of the reference's circle test; the reference has no rectangle), not BoatAdvanced's planning
//                          speed box (rows in a tree have passed it), no static map, no occupancy grid.
//   a point in a rectangle dx = vx - ox; dy = vy - oy; xi = co dx + so dy; eta = co dy + (-so) dx;
//                          inside = |xi| <= a' && |eta| <= b'     (fp64, these operations in this order, nothing contracted)
//   a row fails            when some point is inside some rectangle of its instant
//
// Execution: clear.hpp's stages; only the check is this file's.  The steps (retain_links), the propagate rounds
// (k_clear_init / k_clear_double<ClearLink>) and the select (k_clear_select) are the existing kernels, unchanged.
//
// The table: [L][D][4] = ox, oy, co, so per instant and rectangle (co, so the host's lq_sincos of the heading), then [D][4] =
// a', b', rp, 0 per rectangle: the half extents (for the novice boats grown by half the boat length on the host) and the padded half
// diagonal rp = sqrt(a'^2 + b'^2) (1 + 1e-9) + 1e-9 of the cull.
// The sweep has hull_hits's shape: lanes cull the rectangles in tiles of 64 -- a rectangle can only contain a hull point if its
// centre, seen from the vehicle's frame, lies within the hull's padded bounding box grown by rp: every point of the rectangle is
// within its half diagonal of the centre --, one ballot, then the lanes hold the hull points in tiles of 64, each rotated once per
// tile, and a near rectangle's six values come from the lane that culled it (lane_read).  The launch's LDS is the hull points'
// alone (16 V bytes, staged by the kernel itself whatever the engine's map, as k_clear_check does), so there is no LDS to pass
// them through; DESIGN.md section 21 gives the compiler's figures.

template <class S> struct clear_rects_centre : std::is_base_of<BoatNovice, S> {};       // the novice boats: the centre point alone

// Does some vehicle point of the pose (px, py | c, s) lie inside some of the D rectangles of one instant?  `pose`: that instant's
// [D][4], `ext`: [D][4].  The whole wavefront calls it.
template <class S>
__device__ __forceinline__ bool clear_rects_hit(const double* __restrict__ pose, const double* __restrict__ ext, int D, const double* hull_lds,
                                                int V, const double* bb, double px, double py, double c, double s, int lane) {
    bool hit = false;
    if constexpr (clear_rects_centre<S>::value) {
        for (int o = lane; o < D; o += 64) {
            const double co = pose[4 * o + 2], so = pose[4 * o + 3];
            const double dx = px - pose[4 * o], dy = py - pose[4 * o + 1];
            const double xi = co * dx + so * dy, eta = co * dy + (-so) * dx;
            hit |= (fabs(xi) <= ext[4 * o]) && (fabs(eta) <= ext[4 * o + 1]);
        }
    } else {
        const double ms = -s;
        const __attribute__((address_space(3))) double* vps = (const __attribute__((address_space(3))) double*)hull_lds;
        for (int o0 = 0; o0 < D; o0 += 64) {
            const int o = o0 + lane;
            bool near = false;
            double ox = 0.0, oy = 0.0, co = 0.0, so = 0.0, ea = 0.0, eb = 0.0;
            if (o < D) {
                ox = pose[4 * o]; oy = pose[4 * o + 1]; co = pose[4 * o + 2]; so = pose[4 * o + 3];
                ea = ext[4 * o]; eb = ext[4 * o + 1];
                const double rp = ext[4 * o + 2];
                const double dx = ox - px, dy = oy - py;
                const double cbx = c * dx + s * dy, cby = c * dy + ms * dx;
                near = (cbx >= bb[0] - rp) && (cbx <= bb[1] + rp) && (cby >= bb[2] - rp) && (cby <= bb[3] + rp);
            }
            const unsigned long long m = __ballot(near);
            if (m == 0) continue;
            for (int v0 = 0; v0 < V; v0 += 64) {
                const bool live = v0 + lane < V;
                const int v = live ? v0 + lane : 0;              // (a lane past the hull computes on point 0 and does not vote)
                const double bx = vps[v], by = vps[V + v];
                const double vx = px + (c * bx + ms * by);
                const double vy = py + (s * bx + c * by);
                for (unsigned long long mm = m; mm; mm &= mm - 1) {
                    const int j = __builtin_ctzll(mm);
                    const double rco = lane_read(co, j), rso = lane_read(so, j);
                    const double dx = vx - lane_read(ox, j), dy = vy - lane_read(oy, j);
                    const double xi = rco * dx + rso * dy, eta = rco * dy + (-rso) * dx;
                    hit |= live && (fabs(xi) <= lane_read(ea, j)) && (fabs(eta) <= lane_read(eb, j));
                }
            }
        }
    }
    return __any(hit) != 0;
}

// check: block i <-> node i, one wavefront.  `link` holds the finished step sums (RetainLink::steps = cum - elen[0]).
template <class S>
__device__ __forceinline__ void clear_rects_check_body(const Geo& g, const TreeView& tv, const Res& r, int N, const RetainLink* __restrict__ link,
                                                       const double* __restrict__ table, int L, int D, int start, int* __restrict__ own,
                                                       int* __restrict__ dwell, double* hull_lds, int i) {
    const int lane = threadIdx.x;
    if (i >= N) return;
    clear_stage_hull(g, hull_lds, lane, 64);
    __syncthreads();
    const double* ext = table + (size_t)L * D * 4;
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
        const double* pose = table + (size_t)(tau < L - 1 ? tau : L - 1) * D * 4;
        if (clear_rects_hit<S>(pose, ext, D, hull_lds, g.V, g.hbb, x[0], x[1], trig[0], trig[1], lane)) first = tau;
    }
    // a goal hit waits at its last row while the rectangles move on (as clear_check_body)
    const bool in = goal_hit<S>(tv, r, i) && i > 0;
    int dw = -2;
    if (in) {
        dw = -1;
        if (first >= 0) clear_load_row<S>(xe, ue, len - 1, x, u, trig);
        for (int tau = base + len; tau <= L - 1 && dw < 0; ++tau)       // (base + len - 1 = start + cum[i] - 1: the arrival)
            if (clear_rects_hit<S>(table + (size_t)tau * D * 4, ext, D, hull_lds, g.V, g.hbb, x[0], x[1], trig[0], trig[1], lane)) dw = tau;
    }
    if (lane == 0) { own[i] = first; dwell[i] = dw; }
}
template <class S>
__global__ __launch_bounds__(64) void k_clear_rects_check(Geo g, TreeView tv, Res r, int N, const RetainLink* __restrict__ link,
                                                          const double* __restrict__ table, int L, int D, int start, int* __restrict__ own,
                                                          int* __restrict__ dwell) {
    extern __shared__ double hull_lds[];
    if constexpr (has_discs<S>::value) clear_rects_check_body<S>(g, tv, r, N, link, table, L, D, start, own, dwell, hull_lds, (int)blockIdx.x);
}
