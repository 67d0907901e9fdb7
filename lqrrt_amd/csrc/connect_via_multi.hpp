// connect_via_multi.hpp -- the goal chains through waypoints for SEVERAL trees per launch (lqrrt_connect_via_search_multi /
// lqrrt_connect_via_commit_multi; connect_vias).  Fragment of kernels.hpp (included there after connect_via.hpp, inside namespace
// lq).  A search through waypoints leaves most of the chip idle once its first chain has reached the goal and the early stop prunes
// the rest, exactly as connect.hpp's does: the searches of a fleet's trees run side by side in ONE launch.  As in
// k_connect_search_multi a workgroup finds its engine from the ascending prefix table of workgroup counts in the arguments
// (multi_engine_of) and reads P / g / r / tv from that engine's device-resident EngineProto; what belongs to the call -- the
// waypoint table and its length, the candidate ids, the depth table, count, tries, H, the goal and where the winner goes -- is a
// ConnectViaDesc per engine in device memory.  The candidate index handed to the body is relative to the engine's first workgroup,
// so the body decodes (pos, j) with that engine's own Q: neighbouring engines may have different strides.  Every engine has its
// OWN best key: the early stop prunes within one tree only, so each winner is the one the engine's own launch finds, whatever the
// scheduling.  Both kernels wrap connect_via.hpp's bodies and hold no copy of the chain.  Plain launches on one stream.
//
// The descriptor and the prototype are written by the host before the launch and by nothing during it: they are read through the
// constant address space (connect.hpp launch_constant), so that the body's wave-uniform reads stay scalar loads behind the atomic
// poll of the key (the search) and behind the node writer's stores (the commit).
struct ConnectViaDesc {
    ConnectViaArgs a;
    unsigned long long* best;     // the engine's key
};

// Grid = the engines' count (Q + 1) back to back.  Dynamic LDS: the largest refine_lds_bytes of the call.
template <class S>
__global__ __launch_bounds__(64) void k_connect_via_search_multi(ProtoTable pt, const ConnectViaDesc* __restrict__ ds, RetainGrid gr) {
    extern __shared__ double geo_lds[];
    const int e = multi_engine_of(gr.block0, gr.n, (int)blockIdx.x);
    const ConnectViaDesc& d = launch_constant(ds + e);
    const EngineProto& p = launch_constant(pt.p[e]);
    connect_via_search_body<S>(p.P, p.g, p.r, p.tv, d.a, d.best, geo_lds, (unsigned)blockIdx.x - (unsigned)gr.block0[e]);
}

// The replay of one winner: candidate (v, j) from cost `depth`, appended from node `base` on.  A chain through waypoints does not
// fit refine.hpp's RefineDesc (its targets are the plan's own nodes), so the batched commit has a descriptor and a kernel of its own.
struct ConnectViaCommitDesc {
    ConnectViaArgs a;             // way, Q, tries, H, goal (nodes, depth, count unused)
    int* out;                     // the engine's out[3]
    int* lens;                    // the engine's slice of the edge lengths
    int v, j, depth, base;        // the candidate, depth[v] and the tree size
};

// One workgroup per engine with a winner: ds and pt hold those engines only, in the same order.
template <class S>
__global__ __launch_bounds__(64) void k_connect_via_commit_multi(ProtoTable pt, const ConnectViaCommitDesc* __restrict__ ds, int n) {
    extern __shared__ double geo_lds[];
    if ((int)blockIdx.x >= n) return;
    const ConnectViaCommitDesc& d = launch_constant(ds + blockIdx.x);
    const EngineProto& p = launch_constant(pt.p[blockIdx.x]);
    connect_via_commit_body<S>(p.P, p.g, p.r, p.tv, d.a, d.v, d.j, d.depth, d.base, p.ra.fx, d.out, d.lens, geo_lds);
}
