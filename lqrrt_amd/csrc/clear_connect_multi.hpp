// clear_connect_multi.hpp -- goal chains clear of moving discs for SEVERAL trees per launch (lqrrt_tree_clear_connect_multi;
// lqrrt_amd.avoids(connect)).  Reads the trees, writes nothing of them.  Fragment of kernels.hpp (included there behind
// clear_connect.hpp, inside namespace lq).
// The rule is clear_connect.hpp's, per tree and unchanged: member k of a call answers exactly as the one-tree call on its engine
// with its own table, L, D, start, horizon, tries and id list does -- the per-candidate body is THAT file's
// (clear_connect_search_body), called as it stands.
//
// A fleet whose vehicles find every goal hit crossed would make the one-tree call once per vehicle, one after another: ~40 small
// dependent launches, four uploads and a wait each.  Here the clearance stages are clear_multi.hpp's, one launch each whatever the
// number of trees, and behind them stand two launches more:
//   seed    k_clear_connect_multi_seed: one thread per member turns the select's best (cum << 32 | id) into the member's start key
//   search  k_clear_connect_search_multi<S>: the members' candidate counts back to back, one wavefront per candidate.  As in
//           k_connect_search_multi a workgroup finds its member from the ascending prefix table of workgroup counts in the
//           arguments (multi_engine_of; a member without candidates has two equal entries there and is passed over) and reads
//           P / g / r / tv from that member's device-resident EngineProto; what belongs to the call is a ClearConnectDesc per member
//           in device memory.  The body polls the key with an atomic load, so both are read through launch_constant (connect.hpp
//           says why).
// Every member has its OWN key: the early stop prunes within one tree only, so each winner is the one the member's own call finds,
// whatever the scheduling.  Plain launches on one stream -- no grid-wide barrier, no flag another workgroup waits for.
// Dynamic LDS of the search: the largest refine_lds_bytes + 16 V among the launch's members.  The body derives where the hull
// points lie from the member's own geometry and horizon, so a smaller member lives inside a larger reservation.

struct ClearConnectDesc {
    ConnectArgs a;
    ClearConnectArgs c;
    ClearConnectOut* out;         // the member's key and its count of listed clear candidates
    const ClearOut* sel;          // what the select left of the member (the seed reads its best)
};

// the start keys of the search from the selects' bests (k_clear_connect_seed, per member): member q by thread q, an ordinary store
__global__ void k_clear_connect_multi_seed(ProtoTable pt, const ClearConnectDesc* __restrict__ ds, int n) {
    const int q = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (q >= n) return;
    const ClearConnectDesc& d = ds[q];
    const TreeView& tv = pt.p[q]->tv;
    const unsigned long long b = d.sel->best;
    const unsigned long long incumbent = b == ~0ull ? 0x7fffffffull : (b >> 32) - (unsigned long long)tv.elen[0] + 1ull;
    d.out->key = incumbent << 32;
}

// Grid = the members' candidate counts back to back.  Dynamic LDS: the largest refine_lds_bytes + 16 V of the launch.
template <class S>
__global__ __launch_bounds__(64) void k_clear_connect_search_multi(ProtoTable pt, const ClearConnectDesc* __restrict__ ds, RetainGrid gr) {
    extern __shared__ double geo_lds[];
    if constexpr (has_discs<S>::value) {
        const int e = multi_engine_of(gr.block0, gr.n, (int)blockIdx.x);
        const ClearConnectDesc& d = launch_constant(ds + e);
        const EngineProto& p = launch_constant(pt.p[e]);
        clear_connect_search_body<S>(p.P, p.g, p.r, p.tv, d.a, d.c, d.out, geo_lds, (int)blockIdx.x - gr.block0[e]);
    }
}
