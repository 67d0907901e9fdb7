// clear_rects_multi.hpp -- the rectangle queries of clear_rects.hpp and clear_rects_wait.hpp for SEVERAL trees per launch
// (lqrrt_tree_clear_rects_multi, lqrrt_tree_clear_rects_wait_multi; lqrrt_amd.avoids_rects).  Reads the trees, writes nothing of
// them.  Fragment of kernels.hpp (included there behind clear_rects_wait.hpp, inside namespace lq).
// The rule is clear_rects.hpp's and clear_rects_wait.hpp's, per tree and unchanged: member k of a call answers exactly as the
// one-tree call on its engine with its own table, L, D, start (and W) does -- the per-node bodies are THOSE files'
// (clear_rects_check_body, clear_rects_wait_check_body) as they stand, so the row test has one body and member k cannot drift
// from the solo call.  This file holds the two check kernels that span several engines and nothing else.
//
// Execution: clear_multi.hpp's stages, plain launches one after another on one stream -- no grid-wide barrier, no flag another
// workgroup waits for.  Only the check is this file's:
//   steps      retain.hpp's k_retain_init_multi / k_retain_double_multi           (unchanged)
//   check      k_clear_rects_check_multi<S> (one wavefront per node) / k_clear_rects_wait_check_multi<S> (four wavefronts per node)
//   propagate  clear_multi.hpp's k_clear_init_multi<Link> / k_clear_double_multi<Link>   (unchanged; why a smaller tree's extra
//              rounds are the identity is stated there and does not depend on the obstacle's shape)
//   select     clear_multi.hpp's k_clear_select_multi / k_clear_wait_select_multi (unchanged)
// A workgroup finds its member from the ascending prefix table of workgroup counts in the arguments (multi_engine_of), reads
// g / tv / r from that engine's device-resident EngineProto and what belongs to the call -- the member's step sums, its table
// ([L][D][4] poses, then the [D][4] extents tail), L, D, start, W, its answers -- from its ClearDesc in device memory.  The launch
// reserves 16 V bytes of the largest hull of its members; a member with a smaller hull stages its own V points into the front of
// that and reads no further.

#define CLEAR_RECTS_MULTI_PROLOGUE                                        \
    const int e = multi_engine_of(gr.block0, gr.n, (int)blockIdx.x);      \
    const ClearDesc<Link>& d = ds[e];                                     \
    const int blk = (int)blockIdx.x - gr.block0[e];                       \
    const EngineProto& p = *pt.p[e]

// check: workgroup <-> (member, node)
template <class S>
__global__ __launch_bounds__(64) void k_clear_rects_check_multi(ProtoTable pt, const ClearDesc<ClearLink>* __restrict__ ds, RetainGrid gr) {
    typedef ClearLink Link;
    extern __shared__ double hull_lds[];
    if constexpr (has_discs<S>::value) {
        CLEAR_RECTS_MULTI_PROLOGUE;
        clear_rects_check_body<S>(p.g, p.tv, p.r, d.N, d.steps, d.table, d.L, d.D, d.start, d.own, d.dwell, hull_lds, blk);
    }
}
template <class S>
__global__ __launch_bounds__(CLEAR_WAIT_BLOCK) void k_clear_rects_wait_check_multi(ProtoTable pt, const ClearDesc<ClearWaitLink>* __restrict__ ds,
                                                                                   RetainGrid gr) {
    typedef ClearWaitLink Link;
    extern __shared__ double hull_lds[];
    if constexpr (has_discs<S>::value) {
        CLEAR_RECTS_MULTI_PROLOGUE;
        clear_rects_wait_check_body<S>(p.g, p.tv, p.r, d.N, d.steps, d.table, d.L, d.D, d.start, d.waits, d.own, d.dwell, d.hit, hull_lds, blk);
    }
}
#undef CLEAR_RECTS_MULTI_PROLOGUE
