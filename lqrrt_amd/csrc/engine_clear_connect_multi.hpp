// ABI: goal chains clear of moving discs for several trees -- lqrrt_tree_clear_connect_multi (lqrrt_amd.avoids(connect); kernels in
// clear_connect_multi.hpp).  Member k answers exactly as lqrrt_tree_clear_connect on engines[k] with its own table, L, D, start,
// horizon, tries and id list: the seven counters, first, dwell_first and the five chain fields.  Nothing of any tree is written; the
// winners are replayed by the unchanged lqrrt_connect_commit_multi.
// Fragment of engine.hip, behind engine_clear_multi.hpp and engine_clear_connect.hpp.  The host path IS engine_clear_multi.hpp's:
// its check with what the search asks of a member behind the solo clearance call's refusals (in lqrrt_tree_clear_connect's order:
// connect_check, the id list, its ids, the depth table's 32-bit bound, the LDS of the search), and its run -- chunks, the one
// transient allocation and the one uploaded image per chunk, every stage one launch, the staged copies back, one synchronise --
// with ClearConnectExtra, which adds per chunk
//   to the chunking  a member's candidate count: an id list may repeat ids, so the count can exceed the tree's size, and the
//                    search's grid must stay below 2^32 threads as the check's does
//   to the image     per member a ClearConnectOut, a ClearConnectDesc, the depth table (4 B per node) and the id list
//   to the stream    behind the select: k_clear_connect_multi_seed, then k_clear_connect_search_multi<S> over the members'
//                    candidates back to back with the largest clear_connect_lds_bytes among them (no launch for a chunk without
//                    any candidate), then the ClearConnectOuts back in one copy
// Whether a chain won is decided on the host as in clear_connect_run: the key against the member's own incumbent.
// --------------------------------------------------------------------------------------------

struct ClearConnectExtra {
    lqrrt_engine** engines;
    const int32_t* L; const int32_t* D; const int32_t* start; const int32_t* horizons; const int32_t* tries;
    std::vector<const int32_t*> ids;          // per member: its id list, or null (every node)
    std::vector<int> counts;                  // per member: its candidates
    std::vector<std::vector<int>> depths;     // per member: connect_depths' table
    std::vector<ClearConnectOut> wins;        // per member: what comes back (the target of the chunks' copies)
    struct Part { size_t o_win = 0, o_desc = 0; std::vector<size_t> o_depth, o_ids; };
    std::vector<Part> parts;                  // per chunk: where its parts lie in the image

    long long groups(int k) const { return counts[(size_t)k]; }

    void carve(size_t ci, const MultiChunk& c, Carve& carve) {
        if (parts.size() <= ci) parts.resize(ci + 1);
        Part& p = parts[ci];
        const size_t m = c.members.size();
        p.o_win = carve(sizeof(ClearConnectOut) * m);
        p.o_desc = carve(sizeof(ClearConnectDesc) * m);
        p.o_depth.assign(m, 0); p.o_ids.assign(m, 0);
        for (size_t q = 0; q < m; ++q) {
            const size_t k = (size_t)c.members[q];
            p.o_depth[q] = carve(sizeof(int) * depths[k].size());
            p.o_ids[q] = carve(ids[k] ? sizeof(int) * (size_t)counts[k] : 0);
        }
    }

    // img: the host image (zeroed: the ClearConnectOuts start at listed_clear 0, the keys are the seed kernel's to write); dm: where
    // it goes on the device; hd: the members' ClearDescs, which hold the device addresses of what the clearance stages leave
    void fill(size_t ci, const MultiChunk& c, char* img, char* dm, const ClearDesc<ClearLink>* hd) {
        const Part& p = parts[ci];
        ClearConnectDesc* cd = (ClearConnectDesc*)(img + p.o_desc);
        for (size_t q = 0; q < c.members.size(); ++q) {
            const size_t k = (size_t)c.members[q];
            const bool listed = ids[k] && counts[k] > 0;
            memcpy(img + p.o_depth[q], depths[k].data(), sizeof(int) * depths[k].size());
            if (listed) memcpy(img + p.o_ids[q], ids[k], sizeof(int) * (size_t)counts[k]);
            connect_fill_args(engines[k], (const int*)(dm + p.o_depth[q]), listed ? (const int*)(dm + p.o_ids[q]) : nullptr, counts[k],
                              tries[k], horizons[k], &cd[q].a);
            cd[q].c = {hd[q].table, hd[q].ans, hd[q].steps, L[k], D[k], start[k], 0};
            cd[q].out = (ClearConnectOut*)(dm + p.o_win) + q;
            cd[q].sel = hd[q].out;
        }
    }

    template <class S>
    static void search(unsigned grid, size_t lds, hipStream_t st, const ProtoTable& pt, const ClearConnectDesc* ds, const RetainGrid& gr) {
        hipLaunchKernelGGL((k_clear_connect_search_multi<S>), dim3(grid), dim3(64), lds, st, pt, ds, gr);
    }

    int enqueue(size_t ci, const MultiChunk& c, const ProtoTable& pt, char* dm, hipStream_t st) {
        const Part& p = parts[ci];
        const int m = (int)c.members.size();
        const ClearConnectDesc* d_desc = (const ClearConnectDesc*)(dm + p.o_desc);
        hipLaunchKernelGGL(k_clear_connect_multi_seed, dim3(1), dim3(MULTI_MAX), 0, st, pt, d_desc, m);
        HIPCHK(hipGetLastError());
        std::vector<long long> cands;
        size_t lds = 0;
        for (int k : c.members) {
            cands.push_back(counts[(size_t)k]);
            lds = std::max(lds, clear_connect_lds_bytes(engines[k], horizons[k]));
        }
        RetainGrid gr;
        const unsigned grid = retain_grid(cands, gr);
        if (grid > 0) {
            DISPATCH(engines[0], if constexpr (has_discs<S>::value) search<S>(grid, lds, st, pt, d_desc, gr));
            HIPCHK(hipGetLastError());
        }
        // (the members of a chunk are consecutive engines of the call: every engine takes part in the clearance stages)
        HIPCHK(hipMemcpyAsync(wins.data() + c.members[0], dm + p.o_win, sizeof(ClearConnectOut) * m, hipMemcpyDeviceToHost, st));
        return 0;
    }
};

extern "C" int lqrrt_tree_clear_connect_multi(lqrrt_engine** engines, int n, const double* const* tracks_host,
                                              const double* const* radii_host, const int32_t* L, const int32_t* D, const int32_t* start,
                                              const int32_t* horizon_iters, const int32_t* goal_tries, const int32_t* const* nodes_host,
                                              const int32_t* counts, lqrrt_clear_stats* out, lqrrt_clear_connect_stats* chain,
                                              int32_t* const* first_host, int32_t* const* dwell_host, void* stream) {
    typedef ClearPlainMulti M;
    std::vector<ClearMember> mem;
    ClearConnectExtra x{engines, L, D, start, horizon_iters, goal_tries, {}, {}, {}, {}, {}};
    const size_t un = n > 0 ? (size_t)n : 0;
    x.ids.assign(un, nullptr); x.counts.assign(un, 0); x.depths.resize(un); x.wins.resize(un);
    TRY(clear_multi_check<M>(engines, n, tracks_host, radii_host, L, D, start, nullptr, out, mem, horizon_iters && goal_tries && chain, [&](int k) {
        lqrrt_engine* e = engines[k];
        const size_t uk = (size_t)k;
        int rc = connect_check(e, goal_tries[k], horizon_iters[k]);
        if (!rc) rc = multi_id_list(nodes_host, counts, k, &x.ids[uk], &x.counts[uk]);
        if (!rc) rc = connect_candidates_check(e, x.ids[uk], &x.counts[uk], k);
        if (!rc) {
            x.depths[uk].assign((size_t)e->N, 0);
            rc = connect_depths(e, goal_tries[k], horizon_iters[k], x.depths[uk].data());
        }
        const size_t lds = clear_connect_lds_bytes(e, horizon_iters[k]);
        if (!rc && e->lds_limit && lds > e->lds_limit)
            rc = fail(LQRRT_E_ARG, "the search stages the static geometry, an edge of %d rows and the hull points of the disc test in LDS: "
                      "%zu bytes (V = %d, O = %d), the device's limit is %zu", horizon_iters[k], lds, e->geo.V, e->geo.O, e->lds_limit);
        if (rc && g_err.find(engine_suffix(k)) == std::string::npos) g_err += engine_suffix(k);   // (some of the checkers name the engine themselves)
        return rc;
    }));
    TRY(use_device(engines[0]));
    TRY((clear_multi_run<M>(engines, n, mem, L, D, start, nullptr, out, first_host, dwell_host, (hipStream_t)stream, x)));
    for (int k = 0; k < n; ++k) {
        const lqrrt_engine* e = engines[k];
        const ClearConnectOut& w = x.wins[(size_t)k];
        lqrrt_clear_connect_stats* ch = chain + k;
        // every node with first == -1 is neither a conflict nor blocked; of an id list the search counted its entries
        ch->clear_candidates = x.ids[(size_t)k] ? w.listed_clear : e->N - out[k].conflicts - out[k].blocked;
        ch->reserved = 0;
        const long long incumbent = out[k].best_end >= 0 ? out[k].best_steps - e->h_elen[0] + 1 : 0x7fffffffLL;
        if (w.key != ((unsigned long long)incumbent << 32)) {
            const int v = (int)(w.key & 0xffffffffull);
            ch->chain_from = v;
            ch->chain_cost = (int64_t)(w.key >> 32);
            ch->chain_rows = (int32_t)(ch->chain_cost - x.depths[(size_t)k][(size_t)v]);
            ch->chain_arrival = (int64_t)(mem[(size_t)k].cum[(size_t)v] + ch->chain_rows);
        } else { ch->chain_from = -1; ch->chain_rows = -1; ch->chain_cost = -1; ch->chain_arrival = -1; }
    }
    return 0;
}
