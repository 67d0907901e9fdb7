// ABI: plan refinement -- the shortcut search over a found plan and the commit of its winner (Planner.refine_plan; kernels in
// refine.hpp, the rule restated from the C oracle's primitives in tests/refine_reference.py).  Fragment of engine.hip.
// --------------------------------------------------------------------------------------------

// Checks a plan (a parent chain from the root) and fills `buf` with its ids and cost prefix [2][P].  Writes nothing else.
static int refine_check(lqrrt_engine* e, const int32_t* plan, int P, int tries, int horizon, std::vector<int>& buf) {
    if (!plan || P < 1) return fail(LQRRT_E_ARG, "empty plan");
    if (P > 65535) return fail(LQRRT_E_ARG, "plan of %d nodes (at most 65535)", P);
    if (tries < 0) return fail(LQRRT_E_ARG, "goal_tries must be >= 0");
    if (!e->has_res || !e->has_goal) return fail(LQRRT_E_STATE, "set_resolution with a goal first");
    if (horizon < 1 || horizon > e->H) return fail(LQRRT_E_ARG, "horizon of %d steps (the edge pools hold %d)", horizon, e->H);
    if (plan[0] != 0) return fail(LQRRT_E_ARG, "a plan starts at the root (node 0), not at node %d", plan[0]);
    buf.assign((size_t)2 * P, 0);
    long long cost = 0;
    for (int k = 0; k < P; ++k) {
        TRY(range_ok(e, plan[k], 1));
        if (k > 0 && e->h_pid[(size_t)plan[k]] != plan[k - 1])
            return fail(LQRRT_E_ARG, "node %d of the plan is not a child of node %d", plan[k], plan[k - 1]);
        cost += k > 0 ? e->h_elen[(size_t)plan[k]] : 1;
        buf[k] = plan[k];
        buf[(size_t)P + k] = (int)cost;
    }
    if (cost + (long long)(P + tries) * horizon > 0x7fffffffLL) return fail(LQRRT_E_ARG, "plan too long for 32-bit step counts");
    return 0;
}

static void refine_fill_args(const lqrrt_engine* e, const int* plan_dev, int P, int tries, int horizon, RefineArgs* a) {
    a->plan = plan_dev;
    a->prefix = plan_dev + P;
    a->P = P; a->tries = tries; a->H = horizon; a->pad = 0;
    for (int d = 0; d < MAXN; ++d) a->goal[d] = d < e->n ? e->goal[d] : 0.0;
}

// Checks a plan and uploads its ids and cost prefix; `buf` holds the host copy until the caller has synchronised the stream.
static int refine_prepare(lqrrt_engine* e, const int32_t* plan, int P, int tries, int horizon, std::vector<int>& buf, RefineArgs* a,
                          hipStream_t st) {
    TRY(refine_check(e, plan, P, tries, horizon, buf));
    if (P > e->ref_cap) {
        const size_t keep = g_dalloc_bytes;
        if (e->d_ref) (void)hipFree(e->d_ref);
        e->ref_cap = 0;
        int rc = dalloc(&e->d_ref, (size_t)2 * P);
        if (!rc && !e->d_ref_key) rc = dalloc(&e->d_ref_key, (size_t)4);
        g_dalloc_bytes = keep;                                  // (a few kB, allocated on first use: not part of the footprint)
        if (rc) return rc;
        e->ref_cap = P;
    }
    HIPCHK(hipMemcpyAsync(e->d_ref, buf.data(), sizeof(int) * buf.size(), hipMemcpyHostToDevice, st));
    refine_fill_args(e, e->d_ref, P, tries, horizon, a);
    return 0;
}

static size_t refine_lds_bytes(const lqrrt_engine* e, int horizon) {
    return geo_lds_bytes(e) + ((size_t)horizon * (e->n + e->m) + e->n + 2 * e->nw + (size_t)e->m * e->n) * sizeof(double);
}

extern "C" int lqrrt_refine_search(lqrrt_engine* e, const int32_t* plan_host, int P, int goal_tries, int horizon_iters,
                                   int64_t incumbent, int64_t* cost, int32_t* i_out, int32_t* j_out, void* stream) {
    NOT_GENERIC(e);
    if (!e || !cost || !i_out || !j_out) return fail(LQRRT_E_ARG, "null argument");
    if (incumbent < 1 || incumbent > 0x7fffffffLL) return fail(LQRRT_E_ARG, "incumbent cost %lld out of range", (long long)incumbent);
    TRY(use_device(e));
    hipStream_t st = (hipStream_t)stream;
    std::vector<int> buf;
    RefineArgs a;
    TRY(refine_prepare(e, plan_host, P, goal_tries, horizon_iters, buf, &a, st));
    *cost = incumbent; *i_out = -1; *j_out = -1;
    const unsigned long long init = (unsigned long long)incumbent << 32;   // (incumbent, 0, 0): every candidate at its cost loses
    unsigned long long key = init;
    if (P >= 2) {
        // one 64-thread workgroup per candidate: the grid's thread count must stay below 2^32
        if ((long long)P * (P - 1) / 2 * 64 > 0xffffffffLL)
            return fail(LQRRT_E_ARG, "plan of %d nodes: %lld candidates exceed one launch (at most 11586 nodes)", P, (long long)P * (P - 1) / 2);
        HIPCHK(hipMemcpyAsync(e->d_ref_key, &init, sizeof init, hipMemcpyHostToDevice, st));
        const unsigned ncand = (unsigned)((long long)P * (P - 1) / 2);
        DISPATCH(e, hipLaunchKernelGGL((k_refine_search<S>), dim3(ncand), dim3(64), refine_lds_bytes(e, horizon_iters), st, e->P, e->geo,
                                       e->res, e->tv, a, e->d_ref_key));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&key, e->d_ref_key, sizeof key, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    if (key != init) {
        *cost = (int64_t)(key >> 32);
        *i_out = (int32_t)((key >> 16) & 0xffff);
        *j_out = (int32_t)(key & 0xffff);
    }
    return 0;
}

// host mirrors of `count` appended nodes (a parent chain below `parent`), as lqrrt_tree_append keeps them: parents, edge lengths,
// the ignore set (new nodes are not ignored)
static void refine_adopt(lqrrt_engine* e, int parent, int count, const int* lens, int32_t* ids_out) {
    const int base = e->N;
    for (int k = 0; k < count; ++k) {
        const int id = base + k;
        e->h_pid.push_back(k == 0 ? parent : id - 1);
        e->h_elen.push_back(lens[k]);
        if ((e->h_ign[id >> 6] >> (id & 63)) & 1ull) {
            e->h_ign[id >> 6] &= ~(1ull << (id & 63));
            e->ign_dirty = true; e->ign_patch_valid = false;
        }
        ids_out[k] = id;
    }
    e->N = base + count;
    e->ign_hi = std::max(e->ign_hi, e->N);
    e->tot.tree_size = e->N;
}

extern "C" int lqrrt_refine_commit(lqrrt_engine* e, const int32_t* plan_host, int P, int goal_tries, int horizon_iters, int i, int j,
                                   int32_t* ids_out, int cap_ids, void* stream) {
    NOT_GENERIC(e);
    if (!e) return fail(LQRRT_E_ARG, "null engine");
    if (i < 0 || j <= i || j >= P) return fail(LQRRT_E_ARG, "candidate (%d, %d) outside a plan of %d nodes", i, j, P);
    if (!ids_out || cap_ids < P - 1 - j + goal_tries) return fail(LQRRT_E_ARG, "ids_out must hold %d ids", P - 1 - j + goal_tries);
    TRY(use_device(e));
    hipStream_t st = (hipStream_t)stream;
    std::vector<int> buf;
    RefineArgs a;
    TRY(refine_prepare(e, plan_host, P, goal_tries, horizon_iters, buf, &a, st));
    const int base = e->N;
    int* d_out = (int*)(e->d_ref_key + 1);
    DISPATCH(e, hipLaunchKernelGGL((k_refine_commit<S>), dim3(1), dim3(64), refine_lds_bytes(e, horizon_iters), st, e->P, e->geo, e->res,
                                   e->tv, a, i, j, base, e->fix, d_out));
    HIPCHK(hipGetLastError());
    int out[3] = {0, 0, 0};
    HIPCHK(hipMemcpyAsync(out, d_out, sizeof out, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (out[0] < 0) return fail(LQRRT_E_CAPACITY, "tree capacity %d cannot hold the refined chain", e->cap);
    if (!out[2]) return fail(LQRRT_E_STATE, "candidate (%d, %d) does not reach the goal: nothing appended", i, j);
    const int count = out[0];
    std::vector<int> lens((size_t)count);
    HIPCHK(hipMemcpy(lens.data(), e->tv.elen + base, sizeof(int) * count, hipMemcpyDeviceToHost));
    refine_adopt(e, plan_host[i], count, lens.data(), ids_out);
    return count;
}

// --------------------------------------------------------------------------------------------
// Several plans per call: lqrrt_refine_search_multi / lqrrt_refine_commit_multi (refine_plans).  Per CHUNK of up to MULTI_MAX
// engines: one image in device memory -- the keys, the commits' outputs and edge lengths, then a RefineDesc per engine and the
// plans with their cost prefixes -- staged on the host, uploaded in one copy; one launch (refine.hpp k_refine_*_multi); the head
// of the image (keys / outputs) back in one copy.  The chunks of a call are enqueued one after another and waited for once.
// The image lives in a scratch of the chunk's first engine (d_refm: grown on demand, a few kB, like d_ref not part of the
// footprint); the calls are synchronous, so nothing reads it after they return.
struct RefineChunk {
    int first = 0, n = 0;                 // engines [first, first + n) of the call
    std::vector<int> members;             // indices (into the call) of the engines that take part in the launch
    std::vector<char> img;                // host image of the scratch
    size_t o_out = 0, o_lens = 0, o_desc = 0, back = 0;
    std::vector<size_t> lens_at;          // per member: its first edge length in the image (ints from o_lens)
};

static int refine_multi_scratch(lqrrt_engine* owner, size_t bytes, char** out) {
    if (bytes > owner->refm_cap) {
        if (owner->d_refm) (void)hipFree(owner->d_refm);
        owner->d_refm = nullptr; owner->refm_cap = 0;
        const size_t want = (bytes + 4095) / 4096 * 4096;
        TRY(dalloc(&owner->d_refm, want));                      // (the footprint is booked at creation and in alloc_wave: this is not in it)
        owner->refm_cap = want;
    }
    *out = owner->d_refm;
    return 0;
}

// every argument of every engine, before anything is written or launched; bufs[k]: engine k's plan and cost prefix
static int refine_multi_check(lqrrt_engine** engines, int n, const int32_t* const* plans, const int32_t* plan_lens, const int32_t* tries,
                              const int32_t* horizons, std::vector<std::vector<int>>& bufs) {
    if (!engines || n < 1) return fail(LQRRT_E_ARG, "no engines");
    if (!plans || !plan_lens || !tries || !horizons) return fail(LQRRT_E_ARG, "null argument");
    if (n > 4 * MULTI_MAX) return fail(LQRRT_E_ARG, "at most %d engines per call", 4 * (int)MULTI_MAX);
    lqrrt_engine* e0 = engines[0];
    bufs.resize((size_t)n);
    for (int k = 0; k < n; ++k) {
        lqrrt_engine* e = engines[k];
        if (!e) return fail(LQRRT_E_ARG, "null engine");
        NOT_GENERIC(e);
        for (int q = 0; q < k; ++q)
            if (engines[q] == e) return fail(LQRRT_E_ARG, "engine %d appears twice", k);
        if (e->device != e0->device || e->model != e0->model) return fail(LQRRT_E_ARG, "engines of one call share the device and the model");
        TRY(refine_check(e, plans[k], plan_lens[k], tries[k], horizons[k], bufs[k]));
    }
    return 0;
}

// lays out a chunk's image and fills the descriptors of its members (a, best / out / lens); i, j, base are left to the caller
static int refine_multi_stage(lqrrt_engine** engines, const std::vector<std::vector<int>>& bufs, const int32_t* plan_lens, const int32_t* tries,
                              const int32_t* horizons, const std::vector<int>& ids_room, RefineChunk& c, char** d_img) {
    const int m = (int)c.members.size();
    size_t off = 0;
    auto carve = [&](size_t bytes) { const size_t at = off; off += (bytes + 15) / 16 * 16; return at; };
    const size_t o_keys = carve(sizeof(unsigned long long) * m);
    c.o_out = carve(sizeof(int) * 4 * m);
    size_t sum_ids = 0;
    c.lens_at.assign((size_t)m, 0);
    for (int q = 0; q < m; ++q) { c.lens_at[q] = sum_ids; sum_ids += ids_room.empty() ? 0 : (size_t)ids_room[c.members[q]]; }
    c.o_lens = carve(sizeof(int) * sum_ids);
    c.back = off;
    c.o_desc = carve(sizeof(RefineDesc) * m);
    std::vector<size_t> o_plan((size_t)m);
    for (int q = 0; q < m; ++q) o_plan[q] = carve(sizeof(int) * bufs[c.members[q]].size());
    c.img.assign(off, 0);
    TRY(refine_multi_scratch(engines[c.first], off, d_img));
    RefineDesc* hd = (RefineDesc*)(c.img.data() + c.o_desc);
    for (int q = 0; q < m; ++q) {
        const int k = c.members[q];
        memcpy(c.img.data() + o_plan[q], bufs[k].data(), sizeof(int) * bufs[k].size());
        refine_fill_args(engines[k], (const int*)(*d_img + o_plan[q]), plan_lens[k], tries[k], horizons[k], &hd[q].a);
        hd[q].best = (unsigned long long*)(*d_img + o_keys) + q;
        hd[q].out = (int*)(*d_img + c.o_out) + 4 * q;
        hd[q].lens = (int*)(*d_img + c.o_lens) + c.lens_at[q];
        hd[q].i = hd[q].j = -1; hd[q].base = 0; hd[q].pad = 0;
    }
    return 0;
}

static int refine_multi_protos(lqrrt_engine** engines, const RefineChunk& c, const int32_t* horizons, hipStream_t st, ProtoTable& pt, size_t& lds) {
    memset(&pt, 0, sizeof pt);
    lds = 0;
    for (size_t q = 0; q < c.members.size(); ++q) {
        lqrrt_engine* e = engines[c.members[q]];
        TRY(multi_sync_proto(e, st));
        pt.p[q] = e->d_proto;
        lds = std::max(lds, refine_lds_bytes(e, horizons[c.members[q]]));
    }
    return 0;
}

// A failed call: the caller still holds the chunks (their host images are the source or the target of copies that may be in
// flight), so the stream is drained before they go.
static int refine_multi_fail(int rc, hipStream_t st) {
    const std::string keep = g_err;
    (void)hipStreamSynchronize(st);
    g_err = keep;
    return rc;
}

static int refine_search_multi_run(lqrrt_engine** engines, int n, const std::vector<std::vector<int>>& bufs, const int32_t* plan_lens,
                                   const int32_t* tries, const int32_t* horizons, const int64_t* incumbents, int64_t* cost, int32_t* i_out,
                                   int32_t* j_out, hipStream_t st, std::vector<RefineChunk>& chunks) {
    // chunks: up to MULTI_MAX engines with candidates, one 64-thread workgroup per candidate and fewer than 2^32 threads per launch
    long long cands = 0;
    for (int k = 0; k < n; ++k) {
        const long long nc = (long long)plan_lens[k] * (plan_lens[k] - 1) / 2;
        if (nc == 0) continue;
        if (chunks.empty() || (int)chunks.back().members.size() == MULTI_MAX || (cands + nc) * 64 > 0xffffffffLL) {
            chunks.emplace_back();
            chunks.back().first = k;
            cands = 0;
        }
        chunks.back().members.push_back(k);
        cands += nc;
    }
    for (RefineChunk& c : chunks) {
        const int m = (int)c.members.size();
        char* d_img = nullptr;
        TRY(refine_multi_stage(engines, bufs, plan_lens, tries, horizons, std::vector<int>(), c, &d_img));
        unsigned long long* keys = (unsigned long long*)c.img.data();
        std::vector<long long> counts((size_t)m);
        for (int q = 0; q < m; ++q) {
            const int k = c.members[q];
            keys[q] = (unsigned long long)incumbents[k] << 32;  // (incumbent, 0, 0): every candidate at its cost loses
            counts[q] = (long long)plan_lens[k] * (plan_lens[k] - 1) / 2;
        }
        ProtoTable pt;
        size_t lds = 0;
        TRY(refine_multi_protos(engines, c, horizons, st, pt, lds));
        RetainGrid gr;
        const unsigned grid = retain_grid(counts, gr);
        HIPCHK(hipMemcpyAsync(d_img, c.img.data(), c.img.size(), hipMemcpyHostToDevice, st));
        DISPATCH(engines[0], hipLaunchKernelGGL((k_refine_search_multi<S>), dim3(grid), dim3(64), lds, st, pt,
                                                (const RefineDesc*)(d_img + c.o_desc), gr));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(c.img.data(), d_img, sizeof(unsigned long long) * m, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    for (const RefineChunk& c : chunks) {
        const unsigned long long* keys = (const unsigned long long*)c.img.data();
        for (size_t q = 0; q < c.members.size(); ++q) {
            const int k = c.members[q];
            if (keys[q] == (unsigned long long)incumbents[k] << 32) continue;
            cost[k] = (int64_t)(keys[q] >> 32);
            i_out[k] = (int32_t)((keys[q] >> 16) & 0xffff);
            j_out[k] = (int32_t)(keys[q] & 0xffff);
        }
    }
    return 0;
}

extern "C" int lqrrt_refine_search_multi(lqrrt_engine** engines, int n, const int32_t* const* plans, const int32_t* plan_lens,
                                         const int32_t* goal_tries, const int32_t* horizon_iters, const int64_t* incumbents,
                                         int64_t* cost_out, int32_t* i_out, int32_t* j_out, void* stream) {
    std::vector<std::vector<int>> bufs;
    TRY(refine_multi_check(engines, n, plans, plan_lens, goal_tries, horizon_iters, bufs));
    if (!incumbents || !cost_out || !i_out || !j_out) return fail(LQRRT_E_ARG, "null argument");
    for (int k = 0; k < n; ++k) {
        if (incumbents[k] < 1 || incumbents[k] > 0x7fffffffLL)
            return fail(LQRRT_E_ARG, "incumbent cost %lld out of range (engine %d)", (long long)incumbents[k], k);
        if ((long long)plan_lens[k] * (plan_lens[k] - 1) / 2 * 64 > 0xffffffffLL)
            return fail(LQRRT_E_ARG, "plan of %d nodes: %lld candidates exceed one launch (at most 11586 nodes)", plan_lens[k],
                        (long long)plan_lens[k] * (plan_lens[k] - 1) / 2);
    }
    TRY(use_device(engines[0]));
    hipStream_t st = (hipStream_t)stream;
    for (int k = 0; k < n; ++k) { cost_out[k] = incumbents[k]; i_out[k] = -1; j_out[k] = -1; }
    std::vector<RefineChunk> chunks;                            // (outlives every copy of the call, also when the call fails)
    const int rc = refine_search_multi_run(engines, n, bufs, plan_lens, goal_tries, horizon_iters, incumbents, cost_out, i_out, j_out, st, chunks);
    return rc ? refine_multi_fail(rc, st) : 0;
}

static int refine_commit_multi_run(lqrrt_engine** engines, int n, const std::vector<std::vector<int>>& bufs, const int32_t* plan_lens,
                                   const int32_t* tries, const int32_t* horizons, const int32_t* ci, const int32_t* cj, int32_t* const* ids_out,
                                   int32_t* counts_out, hipStream_t st, std::vector<RefineChunk>& chunks) {
    std::vector<int> room((size_t)n, 0);
    for (int k = 0; k < n; ++k) {
        counts_out[k] = 0;
        if (ci[k] < 0) continue;                                // (no winner: not part of the launch)
        room[k] = plan_lens[k] - 1 - cj[k] + tries[k];
        if (chunks.empty() || (int)chunks.back().members.size() == MULTI_MAX) {
            chunks.emplace_back();
            chunks.back().first = k;
        }
        chunks.back().members.push_back(k);
    }
    for (RefineChunk& c : chunks) {
        const int m = (int)c.members.size();
        char* d_img = nullptr;
        TRY(refine_multi_stage(engines, bufs, plan_lens, tries, horizons, room, c, &d_img));
        RefineDesc* hd = (RefineDesc*)(c.img.data() + c.o_desc);
        for (int q = 0; q < m; ++q) {
            const int k = c.members[q];
            hd[q].i = ci[k]; hd[q].j = cj[k]; hd[q].base = engines[k]->N;
        }
        ProtoTable pt;
        size_t lds = 0;
        TRY(refine_multi_protos(engines, c, horizons, st, pt, lds));
        HIPCHK(hipMemcpyAsync(d_img, c.img.data(), c.img.size(), hipMemcpyHostToDevice, st));
        DISPATCH(engines[0], hipLaunchKernelGGL((k_refine_commit_multi<S>), dim3((unsigned)m), dim3(64), lds, st, pt,
                                                (const RefineDesc*)(d_img + c.o_desc), m));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(c.img.data(), d_img, c.back, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    for (const RefineChunk& c : chunks) {
        const int* outs = (const int*)(c.img.data() + c.o_out);
        const int* lens = (const int*)(c.img.data() + c.o_lens);
        for (size_t q = 0; q < c.members.size(); ++q) {
            const int k = c.members[q];
            const int* out = outs + 4 * q;
            if (out[0] < 0) { counts_out[k] = LQRRT_E_CAPACITY; continue; }
            if (!out[2]) { counts_out[k] = LQRRT_E_STATE; continue; }      // (the chain does not reach the goal: nothing appended)
            refine_adopt(engines[k], bufs[k][(size_t)ci[k]], out[0], lens + c.lens_at[q], ids_out[k]);
            counts_out[k] = out[0];
        }
    }
    return 0;
}

extern "C" int lqrrt_refine_commit_multi(lqrrt_engine** engines, int n, const int32_t* const* plans, const int32_t* plan_lens,
                                         const int32_t* goal_tries, const int32_t* horizon_iters, const int32_t* i, const int32_t* j,
                                         int32_t* const* ids_out, const int32_t* cap_ids, int32_t* counts_out, void* stream) {
    std::vector<std::vector<int>> bufs;
    TRY(refine_multi_check(engines, n, plans, plan_lens, goal_tries, horizon_iters, bufs));
    if (!i || !j || !ids_out || !cap_ids || !counts_out) return fail(LQRRT_E_ARG, "null argument");
    for (int k = 0; k < n; ++k) {
        if (i[k] == -1 && j[k] == -1) continue;                 // an engine without a winner
        const int P = plan_lens[k];
        if (i[k] < 0 || j[k] <= i[k] || j[k] >= P)
            return fail(LQRRT_E_ARG, "candidate (%d, %d) outside a plan of %d nodes (engine %d)", i[k], j[k], P, k);
        if (!ids_out[k] || cap_ids[k] < P - 1 - j[k] + goal_tries[k])
            return fail(LQRRT_E_ARG, "ids_out of engine %d must hold %d ids", k, P - 1 - j[k] + goal_tries[k]);
    }
    TRY(use_device(engines[0]));
    hipStream_t st = (hipStream_t)stream;
    std::vector<RefineChunk> chunks;                            // (outlives every copy of the call, also when the call fails)
    const int rc = refine_commit_multi_run(engines, n, bufs, plan_lens, goal_tries, horizon_iters, i, j, ids_out, counts_out, st, chunks);
    return rc ? refine_multi_fail(rc, st) : 0;
}
