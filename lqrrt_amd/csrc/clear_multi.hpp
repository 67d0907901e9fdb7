// clear_multi.hpp -- the clearance queries of clear.hpp and clear_wait.hpp for SEVERAL trees per launch (lqrrt_tree_clear_multi,
// lqrrt_tree_clear_wait_multi; lqrrt_amd.avoids and deconflict(batched=True)).  Reads the trees, writes nothing of them.
// Fragment of kernels.hpp (included there behind clear_wait.hpp, inside namespace lq).
// The rule is clear.hpp's and clear_wait.hpp's, per tree and unchanged: member k of a call answers exactly as the one-tree call on
// its engine with its own table, L, D, start (and W) does -- the per-node bodies are THOSE files' (clear_check_body,
// clear_wait_check_body, clear_select_body, clear_wait_select_body), their links and joins too.
//
// One solo call is ~38 small dependent launches whose kernels are the minority of the call at 10^4 nodes; a fleet that checks its
// plans every tick against tracked traffic would pay them once per vehicle, one after another.  Here every stage is ONE launch
// whatever the number of trees, as in retain.hpp's k_retain_*_multi: a workgroup finds its tree from the ascending prefix table of
// workgroup counts in the arguments (multi_engine_of), reads P / g / r / tv from that engine's device-resident EngineProto and what
// belongs to the call -- the member's slices of the scratch, its disc table, L, D, start, W, its counters -- from a ClearDesc in
// device memory, so the argument block stays at the pointer table, one pointer and the prefix table.
//
// Execution: plain launches, one after another on one stream -- no grid-wide barrier, no flag another workgroup waits for.
//   steps      retain.hpp's k_retain_init_multi / k_retain_double_multi over a RetainDesc table with root 0 and no ok table
//   check      k_clear_check_multi<S> (one wavefront per node) / k_clear_wait_check_multi<S> (four wavefronts per node)
//   propagate  k_clear_init_multi<Link> / k_clear_double_multi<Link>, ceil(log2 of the LARGEST tree of the launch) rounds
//   select     k_clear_select_multi / k_clear_wait_select_multi, one counter block per member
//
// Why the extra rounds are harmless.  A launch runs the rounds its largest tree needs; a smaller tree's links are finished earlier
// and then go through further rounds.  A finished link has jump == 0 (the root) and, the links being INCLUSIVE of their jump
// target, a value that already holds own[0]; the root's own link is {0, own[0]} from round 0 on.  A further round computes
// join(value, a[0].value) = join(value, own[0]).  Both joins -- the minimum with -1 as +infinity, and the bitwise AND -- are
// associative, commutative and idempotent, so joining in once more an operand that is already part of the value changes nothing:
// the round is the identity on a finished tree, the root included (join(own[0], own[0]) = own[0]).  The step sums are
// retain.hpp's: their terminals (jump == itself, ok 1, steps 0) are the identity of an additive join, as stated there.

template <class Link> struct clear_out_of;
template <> struct clear_out_of<ClearLink> { typedef ClearOut type; };
template <> struct clear_out_of<ClearWaitLink> { typedef ClearWaitOut type; };

// What a workgroup needs of the call, per member, in device memory.  Link = ClearLink: lqrrt_tree_clear_multi (Val = int);
// ClearWaitLink: lqrrt_tree_clear_wait_multi (Val = a 64-bit mask).
template <class Link>
struct ClearDesc {
    typedef typename Link::Val Node;
    const RetainLink* steps;      // the finished step sums (the parity the rounds of `steps` ended on)
    Link* link[2];                // the two parities of the propagate rounds
    const Link* done;             // the finished links (the parity the propagate rounds end on)
    Node *own, *dwell, *ans;      // per node: the check's two answers, the select's
    int* hit;                     // (wait call only)
    const double* table;          // the member's disc table [L][D][4]; members may share one
    typename clear_out_of<Link>::type* out;
    int N, L, D, start, waits, pad;
};

#define CLEAR_MULTI_PROLOGUE                                              \
    const int e = multi_engine_of(gr.block0, gr.n, (int)blockIdx.x);      \
    const ClearDesc<Link>& d = ds[e];                                     \
    const int blk = (int)blockIdx.x - gr.block0[e];                       \
    const EngineProto& p = *pt.p[e];                                      \
    (void)p; (void)blk

// check: workgroup <-> (member, node).  The launch reserves 16 V bytes of the largest hull of its members.
template <class S>
__global__ __launch_bounds__(64) void k_clear_check_multi(ProtoTable pt, const ClearDesc<ClearLink>* __restrict__ ds, RetainGrid gr) {
    typedef ClearLink Link;
    extern __shared__ double hull_lds[];
    if constexpr (has_discs<S>::value) {
        CLEAR_MULTI_PROLOGUE;
        clear_check_body<S>(p.P, p.g, p.tv, p.r, d.N, d.steps, d.table, d.L, d.D, d.start, d.own, d.dwell, hull_lds, blk);
    }
}
template <class S>
__global__ __launch_bounds__(CLEAR_WAIT_BLOCK) void k_clear_wait_check_multi(ProtoTable pt, const ClearDesc<ClearWaitLink>* __restrict__ ds,
                                                                             RetainGrid gr) {
    typedef ClearWaitLink Link;
    extern __shared__ double hull_lds[];
    if constexpr (has_discs<S>::value) {
        CLEAR_MULTI_PROLOGUE;
        clear_wait_check_body<S>(p.P, p.g, p.tv, p.r, d.N, d.steps, d.table, d.L, d.D, d.start, d.waits, d.own, d.dwell, d.hit, hull_lds, blk);
    }
}

// links of round 0: a node and its parent (k_clear_init, per member)
template <class Link>
__global__ __launch_bounds__(RETAIN_BLOCK) void k_clear_init_multi(ProtoTable pt, const ClearDesc<Link>* __restrict__ ds, RetainGrid gr) {
    CLEAR_MULTI_PROLOGUE;
    const int i = blk * RETAIN_BLOCK + (int)threadIdx.x;
    if (i >= d.N) return;
    Link l{};
    if (i == 0) { l.jump = 0; l.*Link::FIELD = d.own[0]; }
    else { l.jump = p.tv.pID[i]; l.*Link::FIELD = Link::join(d.own[i], d.own[l.jump]); }
    d.link[0][i] = l;
}

// one doubling round for every tree of the launch: link[from] -> link[from ^ 1] (k_clear_double, per member)
template <class Link>
__global__ __launch_bounds__(RETAIN_BLOCK) void k_clear_double_multi(ProtoTable pt, const ClearDesc<Link>* __restrict__ ds, RetainGrid gr,
                                                                      int from) {
    CLEAR_MULTI_PROLOGUE;
    const int i = blk * RETAIN_BLOCK + (int)threadIdx.x;
    if (i >= d.N) return;
    const Link* __restrict__ a = d.link[from];
    Link l = a[i];
    const Link up = a[l.jump];
    l.*Link::FIELD = Link::join(l.*Link::FIELD, up.*Link::FIELD);
    l.jump = up.jump;
    d.link[from ^ 1][i] = l;
}

// select: workgroup <-> (member, block of its nodes)
__global__ __launch_bounds__(CLEAR_BLOCK) void k_clear_select_multi(ProtoTable pt, const ClearDesc<ClearLink>* __restrict__ ds, RetainGrid gr) {
    typedef ClearLink Link;
    CLEAR_MULTI_PROLOGUE;
    clear_select_body(p.tv, d.N, d.own, d.dwell, d.done, d.steps, d.ans, d.out, blk);
}
__global__ __launch_bounds__(CLEAR_WAIT_BLOCK) void k_clear_wait_select_multi(ProtoTable pt, const ClearDesc<ClearWaitLink>* __restrict__ ds,
                                                                              RetainGrid gr) {
    typedef ClearWaitLink Link;
    CLEAR_MULTI_PROLOGUE;
    clear_wait_select_body(p.tv, d.N, d.dwell, d.hit, d.done, d.steps, d.ans, d.out, blk);
}
#undef CLEAR_MULTI_PROLOGUE
