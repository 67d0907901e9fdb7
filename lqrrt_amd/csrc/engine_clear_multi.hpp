// ABI: the clearance calls for several trees -- lqrrt_tree_clear_multi and lqrrt_tree_clear_wait_multi (lqrrt_amd.avoids,
// deconflict(batched=True); kernels in clear_multi.hpp).  Member k answers exactly as lqrrt_tree_clear / lqrrt_tree_clear_wait on
// engines[k] with its own table, L, D, start (and waits); nothing of any tree is written.  One host path, templated on the traits
// of engine_clear.hpp, which a second traits struct each extends by the two launches that span several engines.
// Fragment of engine.hip, behind engine_clear.hpp (clear_check, ClearPlain, ClearWait) and engine_refine.hpp (multi_engines_check,
// multi_chunks, multi_grid, Carve, StreamDrain).
//
// Every argument of every member is checked -- the engine list by multi_engines_check, the member's own arguments by the solo
// calls' clear_check -- before anything is allocated or enqueued; a refusal names the engine.  Then, per chunk of up to MULTI_MAX
// members (multi_chunks: fewer than 2^32 threads per launch), ONE transient allocation:
//   image     what is uploaded in one copy: a ClearOut / ClearWaitOut, a RetainDesc and a ClearDesc per member, and the disc tables
//             (32 L D bytes each); members that pass the same tracks and radii arrays with equal L, D (and, the novice boats, equal
//             inflation) share one table
//   per node  60 bytes (lqrrt_tree_clear_multi) / 92 bytes (lqrrt_tree_clear_wait_multi) as in engine_clear.hpp, the members'
//             slices of one kind back to back
// and every stage ONE launch over the chunk's members.  The chunks are enqueued one after another and waited for once; the scratch
// is freed before the call returns (on the error path behind a StreamDrain) and is not part of any engine's footprint.
// --------------------------------------------------------------------------------------------

struct ClearPlainMulti : ClearPlain {
    typedef ClearPlain Solo;
    typedef ClearDesc<ClearLink> Desc;
    static constexpr const char* NAME_MULTI = "lqrrt_tree_clear_multi";
    static constexpr long long CHECK_GROUPS = 1;                // 64-thread groups of the check per node (multi_chunks counts in those)
    template <class S>
    static void check_multi(unsigned grid, size_t hull_bytes, hipStream_t st, const ProtoTable& pt, const Desc* ds, const RetainGrid& gr) {
        hipLaunchKernelGGL((k_clear_check_multi<S>), dim3(grid), dim3(64), hull_bytes, st, pt, ds, gr);
    }
    static void select_multi(unsigned grid, hipStream_t st, const ProtoTable& pt, const Desc* ds, const RetainGrid& gr) {
        hipLaunchKernelGGL(k_clear_select_multi, dim3(grid), dim3(CLEAR_BLOCK), 0, st, pt, ds, gr);
    }
};

struct ClearWaitMulti : ClearWait {
    typedef ClearWait Solo;
    typedef ClearDesc<ClearWaitLink> Desc;
    static constexpr const char* NAME_MULTI = "lqrrt_tree_clear_wait_multi";
    static constexpr long long CHECK_GROUPS = CLEAR_WAIT_WAVES;  // (so a chunk of the wait call holds fewer than 2^24 nodes)
    template <class S>
    static void check_multi(unsigned grid, size_t hull_bytes, hipStream_t st, const ProtoTable& pt, const Desc* ds, const RetainGrid& gr) {
        hipLaunchKernelGGL((k_clear_wait_check_multi<S>), dim3(grid), dim3(CLEAR_WAIT_BLOCK), hull_bytes, st, pt, ds, gr);
    }
    static void select_multi(unsigned grid, hipStream_t st, const ProtoTable& pt, const Desc* ds, const RetainGrid& gr) {
        hipLaunchKernelGGL(k_clear_wait_select_multi, dim3(grid), dim3(CLEAR_WAIT_BLOCK), 0, st, pt, ds, gr);
    }
};

// the chunks' scratches: all live until the call's one synchronise
struct ClearMultiScratch {
    std::vector<char*> mem;
    ClearMultiScratch() = default;
    ClearMultiScratch(const ClearMultiScratch&) = delete;
    ~ClearMultiScratch() {
        for (char* m : mem)
            if (m) (void)hipFree(m);
    }
};

// what the check leaves of a member: its step sums, and its disc table or the earlier member whose table it shares
struct ClearMember {
    std::vector<long long> cum;
    std::vector<double> table;
    int shares = -1;
};

// What a caller adds to the two calls of this file (lqrrt_tree_clear_connect_multi adds its search: engine_clear_connect_multi.hpp).
// To the check: more(k), what else it asks of member k, behind the solo call's refusals.  To the run, per chunk: workgroups of its
// own per member (the chunks then hold fewer than 2^32 threads for its launch too), parts of its own in the uploaded image, what it
// enqueues behind the select, copies back included; the run's one synchronise covers them.  ClearNoExtra: nothing of all that.
struct ClearNoExtra {
    long long groups(int) const { return 0; }
    void carve(size_t, const MultiChunk&, Carve&) {}
    template <class Desc>
    void fill(size_t, const MultiChunk&, char*, char*, const Desc*) {}
    int enqueue(size_t, const MultiChunk&, const ProtoTable&, char*, hipStream_t) { return 0; }
};

// Every argument of every member, before anything is allocated or enqueued.  waits == nullptr: lqrrt_tree_clear_multi.  `args`:
// the caller's further arrays are all there.
template <class M, class More>
static int clear_multi_check(lqrrt_engine** engines, int n, const double* const* tracks, const double* const* radii, const int32_t* L,
                             const int32_t* D, const int32_t* start, const int32_t* waits, const typename M::Stats* out,
                             std::vector<ClearMember>& mem, bool args, More more) {
    mem.resize(n > 0 ? (size_t)n : 0);
    return multi_engines_check(engines, n, tracks && radii && L && D && start && out && (waits || !M::HIT_BYTES) && args, [&](int k) {
        ClearMember& me = mem[(size_t)k];
        const int rc = clear_check<typename M::Solo>(engines[k], out + k, tracks[k], radii[k], L[k], D[k], start[k], waits ? waits[k] : 1,
                                                     me.cum, me.table);
        if (rc) { g_err += engine_suffix(k); return rc; }
        TRY(more(k));
        // the shared-traffic case: the same arrays, read the same way, make the same table -- keep one
        const bool novice = model_novice(engines[k]->model);
        for (int q = 0; q < k && me.shares < 0; ++q)
            if (mem[(size_t)q].shares < 0 && tracks[q] == tracks[k] && radii[q] == radii[k] && L[q] == L[k] && D[q] == D[k] &&
                (!novice || engines[q]->P.p[18] == engines[k]->P.p[18]))
                me.shares = q;
        if (me.shares >= 0) std::vector<double>().swap(me.table);
        return 0;
    });
}

// a tree's per-node arrays come back in copies of their own from this size on
static bool clear_multi_direct(size_t N) { return N >= 65536; }

// The launches of a checked call, chunk by chunk, and the call's one synchronise.  `extra`: see ClearNoExtra.
template <class M, class X = ClearNoExtra>
static int clear_multi_run(lqrrt_engine** engines, int n, const std::vector<ClearMember>& mem, const int32_t* L, const int32_t* D,
                           const int32_t* start, const int32_t* waits, typename M::Stats* out, typename M::Node* const* ans_host,
                           typename M::Node* const* dwell_host, hipStream_t st, X&& extra = X()) {
    typedef typename M::Link Link;
    typedef typename M::Node Node;
    typedef typename M::Out Out;
    typedef typename M::Desc Desc;
    std::vector<long long> c_check((size_t)n), c_node((size_t)n), groups((size_t)n);
    for (int k = 0; k < n; ++k) {
        c_check[k] = engines[k]->N;
        c_node[k] = (engines[k]->N + RETAIN_BLOCK - 1) / RETAIN_BLOCK;
        groups[k] = std::max((long long)engines[k]->N * M::CHECK_GROUPS, extra.groups(k));
    }
    std::vector<MultiChunk> chunks = multi_chunks(groups);
    // per chunk: where its parts lie, and the host side of what comes back per node
    struct Layout { size_t o_ans = 0, o_dwell = 0, sumN = 0; std::vector<size_t> offN; std::vector<Node> h_ans, h_dwell; };
    std::vector<Layout> lay(chunks.size());
    // the prototypes first: an upload of one waits for the stream (multi_sync_proto), and nothing of this call is on it yet
    for (const MultiChunk& c : chunks)
        for (int k : c.members) TRY(multi_sync_proto(engines[k], st));
    ClearMultiScratch sc;
    StreamDrain drain(st);                                      // (the scratches are in use by the stream, the images sources and targets of copies)
    drain.arm();
    for (size_t ci = 0; ci < chunks.size(); ++ci) {
        MultiChunk& c = chunks[ci];
        Layout& y = lay[ci];
        const int m = (int)c.members.size();
        ProtoTable pt;
        memset(&pt, 0, sizeof pt);
        size_t hull_bytes = 0;
        int maxN = 1;
        y.offN.assign((size_t)m + 1, 0);
        for (int q = 0; q < m; ++q) {
            const lqrrt_engine* e = engines[c.members[q]];
            pt.p[q] = e->d_proto;
            hull_bytes = std::max(hull_bytes, sizeof(double) * (size_t)2 * e->geo.V);
            y.offN[q + 1] = y.offN[q] + (size_t)e->N;
            maxN = std::max(maxN, e->N);
        }
        const size_t sumN = y.sumN = y.offN[m];
        // ---- the image (uploaded in one copy), then the per-node arrays, carved out of one allocation
        Carve carve{0, 256};
        const size_t o_out = carve(sizeof(Out) * m), o_rdesc = carve(sizeof(RetainDesc) * m), o_desc = carve(sizeof(Desc) * m);
        std::vector<size_t> o_table((size_t)m, 0);
        for (int q = 0; q < m; ++q) {
            const int k = c.members[q];
            const int owner = mem[k].shares < 0 ? k : mem[k].shares;
            int at = -1;                                        // (a table is shared within a chunk; the first member of a chunk that needs it stages it)
            for (int j = 0; j < q && at < 0; ++j) {
                const int kj = c.members[j];
                if ((mem[kj].shares < 0 ? kj : mem[kj].shares) == owner) at = j;
            }
            o_table[q] = at >= 0 ? o_table[at] : carve(sizeof(double) * mem[owner].table.size());
        }
        extra.carve(ci, c, carve);
        const size_t image = carve.off;
        const size_t o_a = carve(sizeof(RetainLink) * sumN), o_b = carve(sizeof(RetainLink) * sumN);
        const size_t o_ca = carve(sizeof(Link) * sumN), o_cb = carve(sizeof(Link) * sumN);
        const size_t o_own = carve(sizeof(Node) * sumN), o_dwell = carve(sizeof(Node) * sumN), o_ans = carve(sizeof(Node) * sumN);
        const size_t o_hit = carve(M::HIT_BYTES * sumN);
        y.o_ans = o_ans; y.o_dwell = o_dwell;
        sc.mem.push_back(nullptr);
        TRY(dalloc_transient(&sc.mem.back(), carve.off));      // (transient: not part of any engine's footprint)
        char* dm = sc.mem.back();
        int rounds = 0;                                         // 2^rounds >= the LARGEST tree of the chunk (clear_multi.hpp: the extra rounds are the identity)
        while ((1ll << rounds) < (long long)maxN) ++rounds;
        const int fin = rounds & 1;
        c.img.assign(image, 0);
        Out* ho = (Out*)(c.img.data() + o_out);
        RetainDesc* hr = (RetainDesc*)(c.img.data() + o_rdesc);
        Desc* hd = (Desc*)(c.img.data() + o_desc);
        for (int q = 0; q < m; ++q) {
            const int k = c.members[q];
            const int owner = mem[k].shares < 0 ? k : mem[k].shares;
            const size_t at = y.offN[q];
            ho[q].best = ~0ull;
            RetainDesc& r = hr[q];
            r.link[0] = (RetainLink*)(dm + o_a) + at; r.link[1] = (RetainLink*)(dm + o_b) + at;
            r.root = 0; r.N = engines[k]->N; r.revalidate = 0;  // (root 0, no ok table: RetainLink::steps = cum - elen[0])
            Desc& d = hd[q];
            d.steps = r.link[fin];
            d.link[0] = (Link*)(dm + o_ca) + at; d.link[1] = (Link*)(dm + o_cb) + at;
            d.done = d.link[fin];
            d.own = (Node*)(dm + o_own) + at; d.dwell = (Node*)(dm + o_dwell) + at; d.ans = (Node*)(dm + o_ans) + at;
            d.hit = M::HIT_BYTES ? (int*)(dm + o_hit) + at : nullptr;
            d.table = (const double*)(dm + o_table[q]);
            d.out = (Out*)(dm + o_out) + q;
            d.N = engines[k]->N; d.L = L[k]; d.D = D[k]; d.start = start[k]; d.waits = waits ? waits[k] : 1;
            const std::vector<double>& table = mem[owner].table;
            memcpy(c.img.data() + o_table[q], table.data(), sizeof(double) * table.size());
        }
        extra.fill(ci, c, c.img.data(), dm, (const Desc*)hd);
        HIPCHK(hipMemcpyAsync(dm, c.img.data(), image, hipMemcpyHostToDevice, st));
        const RetainDesc* d_rdesc = (const RetainDesc*)(dm + o_rdesc);
        const Desc* d_desc = (const Desc*)(dm + o_desc);
        RetainGrid g_check, g_node;
        const unsigned n_check = multi_grid(c, c_check, g_check), n_node = multi_grid(c, c_node, g_node);
        const dim3 t256(RETAIN_BLOCK);
        // ---- steps
        hipLaunchKernelGGL(k_retain_init_multi, dim3(n_node), t256, 0, st, pt, d_rdesc, g_node);
        for (int r = 0; r < rounds; ++r) hipLaunchKernelGGL(k_retain_double_multi, dim3(n_node), t256, 0, st, pt, d_rdesc, g_node, r & 1);
        HIPCHK(hipGetLastError());
        // ---- check, with the largest hull of the chunk
        DISPATCH(engines[0], if constexpr (has_discs<S>::value) M::template check_multi<S>(n_check, hull_bytes, st, pt, d_desc, g_check));
        HIPCHK(hipGetLastError());
        // ---- propagate
        hipLaunchKernelGGL((k_clear_init_multi<Link>), dim3(n_node), t256, 0, st, pt, d_desc, g_node);
        for (int r = 0; r < rounds; ++r) hipLaunchKernelGGL((k_clear_double_multi<Link>), dim3(n_node), t256, 0, st, pt, d_desc, g_node, r & 1);
        // ---- select
        M::select_multi(n_node, st, pt, d_desc, g_node);
        HIPCHK(hipGetLastError());
        TRY(extra.enqueue(ci, c, pt, dm, st));
        // ---- back: the counters in one copy; the per-node arrays somebody asked for straight into the caller's memory where a
        // tree is large, and through ONE staged copy per kind for the small trees of the chunk (a copy per tree would cost them more
        // than it moves)
        HIPCHK(hipMemcpyAsync(c.img.data() + o_out, dm + o_out, sizeof(Out) * m, hipMemcpyDeviceToHost, st));
        bool want_ans = false, want_dwell = false;
        for (int q = 0; q < m; ++q) {
            const int k = c.members[q];
            const size_t N = (size_t)engines[k]->N;
            const bool direct = clear_multi_direct(N);
            if (ans_host && ans_host[k]) {
                if (direct) HIPCHK(hipMemcpyAsync(ans_host[k], dm + o_ans + sizeof(Node) * y.offN[q], sizeof(Node) * N, hipMemcpyDeviceToHost, st));
                else want_ans = true;
            }
            if (dwell_host && dwell_host[k]) {
                if (direct) HIPCHK(hipMemcpyAsync(dwell_host[k], dm + o_dwell + sizeof(Node) * y.offN[q], sizeof(Node) * N, hipMemcpyDeviceToHost, st));
                else want_dwell = true;
            }
        }
        if (want_ans) {
            y.h_ans.resize(sumN);
            HIPCHK(hipMemcpyAsync(y.h_ans.data(), dm + o_ans, sizeof(Node) * sumN, hipMemcpyDeviceToHost, st));
        }
        if (want_dwell) {
            y.h_dwell.resize(sumN);
            HIPCHK(hipMemcpyAsync(y.h_dwell.data(), dm + o_dwell, sizeof(Node) * sumN, hipMemcpyDeviceToHost, st));
        }
    }
    HIPCHK(hipStreamSynchronize(st));
    drain.disarm();
    for (size_t ci = 0; ci < chunks.size(); ++ci) {
        const MultiChunk& c = chunks[ci];
        const Layout& y = lay[ci];
        const Out* ho = (const Out*)c.img.data();              // (the image's first part)
        for (size_t q = 0; q < c.members.size(); ++q) {
            const int k = c.members[q];
            const size_t N = (size_t)engines[k]->N;
            M::stats(ho[q], mem[k].cum, (int)N, out + k);
            if (clear_multi_direct(N)) continue;
            if (ans_host && ans_host[k]) memcpy(ans_host[k], y.h_ans.data() + y.offN[q], sizeof(Node) * N);
            if (dwell_host && dwell_host[k]) memcpy(dwell_host[k], y.h_dwell.data() + y.offN[q], sizeof(Node) * N);
        }
    }
    return 0;
}

template <class M>
static int clear_multi_call(lqrrt_engine** engines, int n, const double* const* tracks, const double* const* radii, const int32_t* L,
                            const int32_t* D, const int32_t* start, const int32_t* waits, typename M::Stats* out,
                            typename M::Node* const* ans_host, typename M::Node* const* dwell_host, void* stream) {
    std::vector<ClearMember> mem;
    TRY(clear_multi_check<M>(engines, n, tracks, radii, L, D, start, waits, out, mem, true, [](int) { return 0; }));
    TRY(use_device(engines[0]));
    return clear_multi_run<M>(engines, n, mem, L, D, start, waits, out, ans_host, dwell_host, (hipStream_t)stream);
}

extern "C" int lqrrt_tree_clear_multi(lqrrt_engine** engines, int n, const double* const* tracks_host, const double* const* radii_host,
                                      const int32_t* L, const int32_t* D, const int32_t* start, lqrrt_clear_stats* out,
                                      int32_t* const* first_host, int32_t* const* dwell_host, void* stream) {
    return clear_multi_call<ClearPlainMulti>(engines, n, tracks_host, radii_host, L, D, start, nullptr, out, first_host, dwell_host, stream);
}

extern "C" int lqrrt_tree_clear_wait_multi(lqrrt_engine** engines, int n, const double* const* tracks_host, const double* const* radii_host,
                                           const int32_t* L, const int32_t* D, const int32_t* start, const int32_t* waits,
                                           lqrrt_clear_wait_stats* out, uint64_t* const* clear_host, uint64_t* const* dwell_host, void* stream) {
    return clear_multi_call<ClearWaitMulti>(engines, n, tracks_host, radii_host, L, D, start, waits, out,
                                            (unsigned long long* const*)clear_host, (unsigned long long* const*)dwell_host, stream);
}
