// reach_multi.hpp -- SEVERAL trees asked about many goals per launch (lqrrt_reach_search_multi / lqrrt_reach_commit_multi;
// fleet_goal_costs / retargets).  Fragment of kernels.hpp (included there after reach.hpp, inside namespace lq).  A fleet's
// task-assignment matrix is P trees x T targets: a reach search per tree pays the fixed cost of a search P times and leaves most of
// the chip idle once its first chains have hit; the searches of a fleet's trees run side by side in ONE launch.  As in
// k_connect_search_multi a workgroup finds its engine from the ascending prefix table of workgroup counts in the arguments
// (multi_engine_of) and reads P / g / r / tv from that engine's device-resident EngineProto; what belongs to the call -- the target
// table and its length, the candidate ids, the depth table, count, tries, H and where the winners go -- is a ReachDesc per engine in
// device memory.  Engine k occupies T_k * count_k workgroups; the block index handed to the body is relative to the engine's first
// workgroup, so the body decodes (t, c) with that engine's own count: neighbouring engines may differ in T_k and count_k.  Every
// (engine, target) pair has its OWN best key: the early stop prunes within one target of one tree only, so each winner is the one
// the engine's own k_reach_search finds, whatever the scheduling.  Both kernels wrap bodies that exist (reach.hpp, refine.hpp) and
// hold no copy of the chain.  Plain launches on one stream: nothing here waits for another workgroup.
//
// The descriptors and the prototype are written by the host before the launch and by nothing during it: they are read through the
// constant address space (connect.hpp launch_constant), so that the body's wave-uniform reads stay scalar loads behind the atomic
// poll of the key (the search) and behind the node writer's stores (the commit).
struct ReachDesc {
    ReachArgs a;
    unsigned long long* keys;     // the engine's T keys
};

// Grid = the engines' T * count back to back.  Dynamic LDS: the largest refine_lds_bytes of the call.
template <class S>
__global__ __launch_bounds__(64) void k_reach_search_multi(ProtoTable pt, const ReachDesc* __restrict__ ds, RetainGrid gr) {
    extern __shared__ double geo_lds[];
    const int e = multi_engine_of(gr.block0, gr.n, (int)blockIdx.x);
    const ReachDesc& d = launch_constant(ds + e);
    const EngineProto& p = launch_constant(pt.p[e]);
    reach_search_body<S>(p.P, p.g, p.r, p.tv, d.a, d.keys, geo_lds, (unsigned)blockIdx.x - (unsigned)gr.block0[e]);
}

// The replay of one winner toward a target: k_refine_commit_multi's descriptor (the one-node plan [v] with the cost prefix
// [depth[v]], the candidate i = j = 0, RefineArgs::goal = the target) with a resolution block of its own -- the engine's, with the
// target's box as the goal box -- in place of the prototype's, which holds the engine's own box.
struct ReachCommitDesc {
    RefineArgs a;
    int* out;                     // the engine's out[3]
    int* lens;                    // the engine's slice of the edge lengths
    int i, j, base, pad;          // the candidate and the tree size
    Res r;                        // the engine's resolution block; goal_lo / goal_hi: the target's box
};

// One workgroup per engine with a winner: ds and pt hold those engines only, in the same order.
template <class S>
__global__ __launch_bounds__(64) void k_reach_commit_multi(ProtoTable pt, const ReachCommitDesc* __restrict__ ds, int n) {
    extern __shared__ double geo_lds[];
    if ((int)blockIdx.x >= n) return;
    const ReachCommitDesc& d = launch_constant(ds + blockIdx.x);
    const EngineProto& p = launch_constant(pt.p[blockIdx.x]);
    refine_commit_body<S>(p.P, p.g, d.r, p.tv, d.a, d.i, d.j, d.base, p.ra.fx, d.out, d.lens, geo_lds);
}
