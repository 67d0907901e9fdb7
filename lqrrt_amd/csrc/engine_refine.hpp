// ABI: plan refinement -- the shortcut search over a found plan and the commit of its winner (Planner.refine_plan; kernels in
// refine.hpp, the rule restated from the C oracle's primitives in tests/refine_reference.py).  Fragment of engine.hip.
//
// The refinement is the first of a family of calls -- goal connection (engine_connect.hpp), one tree asked about many goals
// (engine_reach.hpp), goal chains through waypoints (engine_connect_via.hpp, engine_connect_via_multi.hpp) -- that search candidates
// in one launch and replay the winner in another.  What their host sides share is stated once, here where its first user is: the
// rules of an argument (incumbent_check, goal_fill), the guard of a call's host images (StreamDrain), the one-engine calls' scratch
// and their two runners (solo_scratch, solo_search_run, solo_commit_run), and for the calls that take several engines the
// engine-list check and the two runners that string a call's chunks together (multi_search_run, multi_commit_run, with MultiChunk
// and the multi_* functions).  The kernel launched, its argument block or descriptor, the tables behind it and the decoding of a
// key are each caller's own: its hooks.
// --------------------------------------------------------------------------------------------

// " (engine k)" behind a message of a call for several engines; nothing behind that of a one-engine call (k < 0)
static std::string engine_suffix(int k) { return k < 0 ? std::string() : " (engine " + std::to_string(k) + ")"; }

static std::string strf(const char* fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return buf;
}

// the step count a search has to beat
static int incumbent_check(int64_t incumbent, int k) {
    if (incumbent < 1 || incumbent > 0x7fffffffLL)
        return fail(LQRRT_E_ARG, "incumbent cost %lld out of range%s", (long long)incumbent, engine_suffix(k).c_str());
    return 0;
}

// a search's best key before the launch, (incumbent, 0 ..): every candidate at the incumbent's cost loses against it
static unsigned long long incumbent_key(int64_t incumbent) { return (unsigned long long)incumbent << 32; }

// `goal` (the model's n entries) as the kernels' argument blocks hold it
static void goal_fill(const lqrrt_engine* e, const double* goal, double* out) {
    for (int d = 0; d < MAXN; ++d) out[d] = d < e->n ? goal[d] : 0.0;
}

// A call stages images in host memory of its own and reads results back into it; the copies are asynchronous and the call waits
// for them once, at its end.  When it leaves before that -- a later enqueue failed -- a copy may still be in flight, so the stream
// is drained before the memory goes: declare the guard BEHIND the memory it protects, arm it at the first copy, disarm it after
// the synchronise that succeeded.  (What a read-back targets after a synchronise that FAILED no second one can protect.)
struct StreamDrain {
    hipStream_t st;
    bool armed = false;
    explicit StreamDrain(hipStream_t s) : st(s) {}
    StreamDrain(const StreamDrain&) = delete;
    void arm() { armed = true; }
    void disarm() { armed = false; }
    ~StreamDrain() {
        if (!armed) return;
        const std::string keep = g_err;
        (void)hipStreamSynchronize(st);
        g_err = keep;
    }
};

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

// one 64-thread workgroup per candidate (i, j) of a plan: the grid's thread count must stay below 2^32
static long long refine_candidates(int P) { return (long long)P * (P - 1) / 2; }

static int refine_candidates_check(int P) {
    if (refine_candidates(P) * 64 > 0xffffffffLL)
        return fail(LQRRT_E_ARG, "plan of %d nodes: %lld candidates exceed one launch (at most 11586 nodes)", P, refine_candidates(P));
    return 0;
}

static void refine_fill_args(const lqrrt_engine* e, const int* plan_dev, int P, int tries, int horizon, RefineArgs* a) {
    a->plan = plan_dev;
    a->prefix = plan_dev + P;
    a->P = P; a->tries = tries; a->H = horizon; a->pad = 0;
    goal_fill(e, e->goal, a->goal);
}

static size_t refine_lds_bytes(const lqrrt_engine* e, int horizon) {
    return geo_lds_bytes(e) + ((size_t)horizon * (e->n + e->m) + e->n + 2 * e->nw + (size_t)e->m * e->n) * sizeof(double);
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

// --------------------------------------------------------------------------------------------
// One engine per call (refine, connect, via and reach: a search and a commit each).  Every argument is checked by the call's export
// before anything is written or launched.  A call has one image in device memory -- a head of SOLO_HEAD bytes for what comes back
// (a search's best keys, from byte 0; a commit's out[3] at ints 2 to 4), behind it what the call's hooks lay out -- staged on the
// host and uploaded in one copy; one launch; the keys or out[3] back in one copy; one synchronise.  The image lives in the engine's
// d_solo, which grows on demand, is shared by all these calls (they are synchronous: nothing reads it after they return) and is
// not part of lqrrt_engine_footprint.
static const size_t SOLO_HEAD = 8 * sizeof(int);

// An image's scratch (*mem of *cap bytes) with room for `bytes` bytes: allocated on first use and grown on demand in steps of 4 kB,
// not part of the footprint.  The one-engine calls' and, further down, the chunks' of a call for several engines.
static int scratch_grow(char** mem, size_t* cap, size_t bytes) {
    if (*mem && bytes <= *cap) return 0;
    if (*mem) (void)hipFree(*mem);
    *mem = nullptr; *cap = 0;
    const size_t want = (bytes + 4095) / 4096 * 4096;
    TRY(dalloc_transient(mem, want));
    *cap = want;
    return 0;
}

// room in d_solo for an image of `bytes` bytes, head included
static int solo_scratch(lqrrt_engine* e, size_t bytes) { return scratch_grow(&e->d_solo, &e->solo_cap, bytes); }

// The two solo runners: what multi_search_run and multi_commit_run below are to a call for several engines.  They own use_device
// and the order that makes a call safe -- the scratch is allocated before the guard, the guard stands behind the host image (whose
// head a search's keys come back into) and a commit's out[3], it is armed before the only upload and disarmed only after the
// synchronise that succeeded -- and a call states in a hooks object h only what is its own:
//   h.Args                       the kernel's argument block
//   h.bytes()                    the size of the image behind its head
//   h.fill(e, host, dev, a)      stages the image behind the head at `host` and fills a; device addresses are those of `dev`
//   h.launch<S>(...)             the one launch, which names the call's kernel
// and, a search: h.groups(), its workgroups (0: no launch, and the device is not touched); h.keys(), its number of keys, and
// h.incumbent(t), the cost behind key t, which starts as incumbent_key of it; h.won(t, key) for every key that the launch
// replaced.  A commit replays on one workgroup a chain that appends below tree size `base` and writes out[3] (the node count or
// -1: no room, -, 1: the chain reached its goal); the runner refuses what did not fit (`holds`: what the tree cannot hold) or fell
// short (`unreached`: the message), reads the new edges' lengths and adopts the nodes below `parent`.  It returns their number,
// their ids in ids_out.
template <class H>
static int solo_search_run(lqrrt_engine* e, int horizon, hipStream_t st, const H& h) {
    const long long groups = h.groups();
    if (groups == 0) return 0;                                  // (the outputs stay at "incumbent, -1")
    TRY(use_device(e));
    const size_t keys = (size_t)h.keys(), head = std::max(SOLO_HEAD, sizeof(unsigned long long) * keys);
    TRY(solo_scratch(e, head + h.bytes()));
    std::vector<char> img(head + h.bytes(), 0);
    StreamDrain drain(st);                                      // (img is the source of a copy, its head the target of one)
    unsigned long long* key = (unsigned long long*)img.data();
    for (size_t t = 0; t < keys; ++t) key[t] = incumbent_key(h.incumbent((int)t));
    typename H::Args a;
    h.fill(e, img.data() + head, e->d_solo + head, &a);
    drain.arm();
    HIPCHK(hipMemcpyAsync(e->d_solo, img.data(), img.size(), hipMemcpyHostToDevice, st));
    DISPATCH(e, h.template launch<S>(e, (unsigned)groups, refine_lds_bytes(e, horizon), st, a, (unsigned long long*)e->d_solo));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(key, e->d_solo, sizeof(unsigned long long) * keys, hipMemcpyDeviceToHost, st));     // the keys only
    HIPCHK(hipStreamSynchronize(st));                           // the call's one synchronise
    drain.disarm();
    for (size_t t = 0; t < keys; ++t)
        if (key[t] != incumbent_key(h.incumbent((int)t))) h.won((int)t, key[t]);
    return 0;
}

template <class H>
static int solo_commit_run(lqrrt_engine* e, int horizon, int parent, int32_t* ids_out, hipStream_t st, const H& h, const char* holds,
                           const char* unreached) {
    TRY(use_device(e));
    TRY(solo_scratch(e, SOLO_HEAD + h.bytes()));
    std::vector<char> img(SOLO_HEAD + h.bytes(), 0);
    int out[3] = {0, 0, 0};
    StreamDrain drain(st);                                      // (img is the source of a copy, out the target of one)
    typename H::Args a;
    h.fill(e, img.data() + SOLO_HEAD, e->d_solo + SOLO_HEAD, &a);
    const int base = e->N;
    int* d_out = (int*)e->d_solo + 2;
    drain.arm();
    HIPCHK(hipMemcpyAsync(e->d_solo, img.data(), img.size(), hipMemcpyHostToDevice, st));
    DISPATCH(e, h.template launch<S>(e, refine_lds_bytes(e, horizon), st, a, base, d_out));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d_out, sizeof out, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));                           // the call's one synchronise
    drain.disarm();
    if (out[0] < 0) return fail(LQRRT_E_CAPACITY, "tree capacity %d cannot hold %s", e->cap, holds);
    if (!out[2]) return fail(LQRRT_E_STATE, "%s", unreached);
    const int count = out[0];
    std::vector<int> lens((size_t)count);
    HIPCHK(hipMemcpy(lens.data(), e->tv.elen + base, sizeof(int) * count, hipMemcpyDeviceToHost));
    refine_adopt(e, parent, count, lens.data(), ids_out);
    return count;
}

// a winner's key: (cost, i, j)
static void refine_decode(unsigned long long key, int64_t* cost, int32_t* i, int32_t* j) {
    *cost = (int64_t)(key >> 32);
    *i = (int32_t)((key >> 16) & 0xffff);
    *j = (int32_t)(key & 0xffff);
}

// The refinement's solo hooks.  What its search and its commit share: behind the head the plan with its cost prefix (buf), and
// the argument block of chains that steer at `goal`.
struct RefineSolo {
    typedef RefineArgs Args;
    const std::vector<int>& buf;
    int P, tries, horizon;
    const double* goal;
    size_t bytes() const { return sizeof(int) * buf.size(); }
    void fill(const lqrrt_engine* e, char* host, const char* dev, RefineArgs* a) const {
        memcpy(host, buf.data(), bytes());
        refine_fill_args(e, (const int*)dev, P, tries, horizon, a);
        goal_fill(e, goal, a->goal);
    }
};

struct RefineSearchSolo : RefineSolo {
    int64_t best; int64_t* cost; int32_t* i_out; int32_t* j_out;
    long long groups() const { return refine_candidates(P); }
    int keys() const { return 1; }
    int64_t incumbent(int) const { return best; }
    template <class S>
    static void launch(const lqrrt_engine* e, unsigned grid, size_t lds, hipStream_t st, const RefineArgs& a, unsigned long long* key) {
        hipLaunchKernelGGL((k_refine_search<S>), dim3(grid), dim3(64), lds, st, e->P, e->geo, e->res, e->tv, a, key);
    }
    void won(int, unsigned long long key) const { refine_decode(key, cost, i_out, j_out); }
};

// The replay of candidate (i, j), its chain ending inside the goal box of `res`: the engine's own for a refinement; connect's
// and reach's commit is this one too (engine_connect.hpp: connect_commit_run).
struct RefineCommitSolo : RefineSolo {
    int i, j;
    const Res& res;
    template <class S>
    void launch(const lqrrt_engine* e, size_t lds, hipStream_t st, const RefineArgs& a, int base, int* out) const {
        hipLaunchKernelGGL((k_refine_commit<S>), dim3(1), dim3(64), lds, st, e->P, e->geo, res, e->tv, a, i, j, base, e->fix, out);
    }
};

extern "C" int lqrrt_refine_search(lqrrt_engine* e, const int32_t* plan_host, int P, int goal_tries, int horizon_iters,
                                   int64_t incumbent, int64_t* cost, int32_t* i_out, int32_t* j_out, void* stream) {
    NOT_GENERIC(e);
    if (!e || !cost || !i_out || !j_out) return fail(LQRRT_E_ARG, "null argument");
    TRY(incumbent_check(incumbent, -1));
    std::vector<int> buf;
    TRY(refine_check(e, plan_host, P, goal_tries, horizon_iters, buf));
    *cost = incumbent; *i_out = -1; *j_out = -1;
    TRY(refine_candidates_check(P));
    return solo_search_run(e, horizon_iters, (hipStream_t)stream,
                           RefineSearchSolo{{buf, P, goal_tries, horizon_iters, e->goal}, incumbent, cost, i_out, j_out});
}

extern "C" int lqrrt_refine_commit(lqrrt_engine* e, const int32_t* plan_host, int P, int goal_tries, int horizon_iters, int i, int j,
                                   int32_t* ids_out, int cap_ids, void* stream) {
    NOT_GENERIC(e);
    if (!e) return fail(LQRRT_E_ARG, "null engine");
    if (i < 0 || j <= i || j >= P) return fail(LQRRT_E_ARG, "candidate (%d, %d) outside a plan of %d nodes", i, j, P);
    if (!ids_out || cap_ids < P - 1 - j + goal_tries) return fail(LQRRT_E_ARG, "ids_out must hold %d ids", P - 1 - j + goal_tries);
    std::vector<int> buf;
    TRY(refine_check(e, plan_host, P, goal_tries, horizon_iters, buf));
    return solo_commit_run(e, horizon_iters, plan_host[i], ids_out, (hipStream_t)stream,
                           RefineCommitSolo{{buf, P, goal_tries, horizon_iters, e->goal}, i, j, e->res}, "the refined chain",
                           strf("candidate (%d, %d) does not reach the goal: nothing appended", i, j).c_str());
}

// --------------------------------------------------------------------------------------------
// Several engines per call (refine_plans: lqrrt_refine_search_multi / lqrrt_refine_commit_multi; connect_goals and connect_vias
// follow in their fragments).  Every argument of every engine is checked before anything is written or launched.  A call is cut
// into CHUNKS of up to MULTI_MAX engines that take part (fewer than 2^32 threads per launch).  Per chunk: one image in device
// memory -- what comes back at its head (a search's best keys; a commit's outputs and edge lengths), then a descriptor per engine
// and the tables the descriptors point to -- staged on the host and uploaded in one copy; one launch; the head back in one copy.
// The chunks of a call are enqueued one after another and waited for once.  The image lives in a scratch of the chunk's first
// engine (d_refm: grown on demand, a few kB, like d_solo not part of the footprint); the calls are synchronous, so nothing reads it
// after they return.  The host images are the sources and the targets of the copies: they outlive the call's synchronise, and a
// call that fails drains the stream before they go (StreamDrain).
struct MultiChunk {
    int first = 0;                        // the engine (index into the call) whose scratch holds the image
    std::vector<int> members;             // indices (into the call) of the engines that take part in the launch
    std::vector<char> img;                // host image of the scratch
    char* dev = nullptr;                  // the scratch: where the image goes on the device
    std::vector<size_t> key_at;           // search, per member: its first key (the keys lie at the image's head, member by member)
    size_t o_out = 0, o_lens = 0, back = 0;   // commit: the outputs [4] per member, the edge lengths, the bytes that come back
    std::vector<size_t> lens_at;          // commit, per member: its first edge length (ints from o_lens)
    unsigned long long* keys_of(char* image, size_t q) const { return (unsigned long long*)image + key_at[q]; }
    int* out_of(char* image, size_t q) const { return (int*)(image + o_out) + 4 * q; }
    int* lens_of(char* image, size_t q) const { return (int*)(image + o_lens) + lens_at[q]; }
};

// offsets into an image, each part aligned (16 bytes unless the owner says otherwise)
struct Carve {
    size_t off = 0, align = 16;
    size_t operator()(size_t bytes) { const size_t at = off; off += (bytes + align - 1) / align * align; return at; }
};

// Cuts a call into chunks: groups[k] 64-thread workgroups for engine k (0: the engine takes part in no launch; a commit asks for
// one per winner), up to MULTI_MAX members and fewer than 2^32 threads per chunk.
static std::vector<MultiChunk> multi_chunks(const std::vector<long long>& groups) {
    std::vector<MultiChunk> chunks;
    long long sum = 0;
    for (int k = 0; k < (int)groups.size(); ++k) {
        if (groups[k] == 0) continue;
        if (chunks.empty() || (int)chunks.back().members.size() == MULTI_MAX || (sum + groups[k]) * 64 > 0xffffffffLL) {
            chunks.emplace_back();
            chunks.back().first = k;
            sum = 0;
        }
        chunks.back().members.push_back(k);
        sum += groups[k];
    }
    return chunks;
}

static int refine_multi_scratch(lqrrt_engine* owner, size_t bytes, char** out) {
    TRY(scratch_grow(&owner->d_refm, &owner->refm_cap, bytes));
    *out = owner->d_refm;
    return 0;
}

// The engine list of a call: up to 4 * MULTI_MAX distinct engines of one device and model, none generic; `args`: the call's other
// arrays are all there; each(k): what the call asks of engine k, checked in the list's order.
template <class Each>
static int multi_engines_check(lqrrt_engine** engines, int n, bool args, Each each) {
    if (!engines || n < 1) return fail(LQRRT_E_ARG, "no engines");
    if (!args) return fail(LQRRT_E_ARG, "null argument");
    if (n > 4 * MULTI_MAX) return fail(LQRRT_E_ARG, "at most %d engines per call", 4 * (int)MULTI_MAX);
    for (int k = 0; k < n; ++k) {
        lqrrt_engine* e = engines[k];
        if (!e) return fail(LQRRT_E_ARG, "null engine");
        NOT_GENERIC(e);
        for (int q = 0; q < k; ++q)
            if (engines[q] == e) return fail(LQRRT_E_ARG, "engine %d appears twice", k);
        if (e->device != engines[0]->device || e->model != engines[0]->model)
            return fail(LQRRT_E_ARG, "engines of one call share the device and the model");
        TRY(each(k));
    }
    return 0;
}

// the prototypes of a chunk's members, current on the device, and the dynamic LDS of the launch that serves them all
static int refine_multi_protos(lqrrt_engine** engines, const MultiChunk& c, const int32_t* horizons, hipStream_t st, ProtoTable& pt, size_t& lds) {
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

// the grid of a chunk's search: groups[k] workgroups for member k, the members side by side
static unsigned multi_grid(const MultiChunk& c, const std::vector<long long>& groups, RetainGrid& gr) {
    std::vector<long long> counts;
    for (int k : c.members) counts.push_back(groups[k]);
    return retain_grid(counts, gr);
}

// A commit's image starts with what comes back: out[4] per member (solo_commit_run's three, padded), then room[k] edge lengths for
// every member k.
static void multi_commit_head(MultiChunk& c, const std::vector<int>& room, Carve& carve) {
    const size_t m = c.members.size();
    c.o_out = carve(sizeof(int) * 4 * m);
    size_t sum = 0;
    c.lens_at.assign(m, 0);
    for (size_t q = 0; q < m; ++q) { c.lens_at[q] = sum; sum += (size_t)room[c.members[q]]; }
    c.o_lens = carve(sizeof(int) * sum);
    c.back = carve.off;
}

// after the read-back of a commit's chunks: per member the refusal of its replay, or its new nodes below parent[k]
static void multi_commit_adopt(lqrrt_engine** engines, std::vector<MultiChunk>& chunks, const std::vector<int>& parent, int32_t* const* ids_out,
                               int32_t* counts_out) {
    for (MultiChunk& c : chunks)
        for (size_t q = 0; q < c.members.size(); ++q) {
            const int k = c.members[q];
            const int* out = c.out_of(c.img.data(), q);
            if (out[0] < 0) { counts_out[k] = LQRRT_E_CAPACITY; continue; }
            if (!out[2]) { counts_out[k] = LQRRT_E_STATE; continue; }      // (the chain does not reach the goal: nothing appended)
            refine_adopt(engines[k], parent[k], out[0], c.lens_of(c.img.data(), q), ids_out[k]);
            counts_out[k] = out[0];
        }
}

// The two runners: the launches of a checked call, chunk by chunk, and the call's one synchronise.  They own the order that makes
// a call safe -- the image is allocated before the guard is armed, the guard is armed before the first copy and disarmed only
// after the synchronise that succeeded -- and a call states in a hooks object h only what is its own:
//   h.Desc, h.Part           the descriptor per member; where a member's tables lie in the image
//   h.carve(c, q, carve)     carves the tables of member q of chunk c behind the descriptors, in the image's order
//   h.fill(c, q, at, d)      fills member q's descriptor d and its tables in c.img (at: what carve returned, per member); device
//                            addresses are those of c.dev
//   h.launch<S>(...)         the one launch, which names the call's kernel
// and, a search: h.groups(k), the workgroups of engine k (0: it takes part in no launch); h.keys(k), its number of keys, and
// h.incumbent(k, t), the cost behind key t, which starts as incumbent_key of it; h.won(k, t, key) for every key that a launch
// replaced.  A commit: h.winner(k), whether engine k has a candidate to replay (one workgroup each), with h.room(k) edges at most
// below node h.parent(k); the runner sets out / lens / base of its descriptor.
template <class H>
static int multi_search_run(lqrrt_engine** engines, int n, const int32_t* horizons, hipStream_t st, const H& h) {
    typedef typename H::Desc Desc;
    std::vector<long long> groups((size_t)n);
    for (int k = 0; k < n; ++k) groups[k] = h.groups(k);
    std::vector<MultiChunk> chunks = multi_chunks(groups);
    StreamDrain drain(st);
    for (MultiChunk& c : chunks) {
        const size_t m = c.members.size();
        size_t n_keys = 0;
        for (int k : c.members) { c.key_at.push_back(n_keys); n_keys += (size_t)h.keys(k); }
        Carve carve;
        carve(sizeof(unsigned long long) * n_keys);             // the keys: only they come back
        const size_t o_desc = carve(sizeof(Desc) * m);
        std::vector<typename H::Part> at;
        for (size_t q = 0; q < m; ++q) at.push_back(h.carve(c, q, carve));
        c.img.assign(carve.off, 0);
        TRY(refine_multi_scratch(engines[c.first], carve.off, &c.dev));
        Desc* hd = (Desc*)(c.img.data() + o_desc);
        for (size_t q = 0; q < m; ++q) {
            for (int t = 0; t < h.keys(c.members[q]); ++t) c.keys_of(c.img.data(), q)[t] = incumbent_key(h.incumbent(c.members[q], t));
            h.fill(c, q, at, &hd[q]);
        }
        ProtoTable pt;
        size_t lds = 0;
        TRY(refine_multi_protos(engines, c, horizons, st, pt, lds));
        RetainGrid gr;
        const unsigned grid = multi_grid(c, groups, gr);
        drain.arm();
        HIPCHK(hipMemcpyAsync(c.dev, c.img.data(), c.img.size(), hipMemcpyHostToDevice, st));
        DISPATCH(engines[0], h.template launch<S>(grid, lds, st, pt, (const Desc*)(c.dev + o_desc), gr));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(c.img.data(), c.dev, sizeof(unsigned long long) * n_keys, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));                           // the call's one synchronise
    drain.disarm();
    for (MultiChunk& c : chunks)
        for (size_t q = 0; q < c.members.size(); ++q) {
            const int k = c.members[q];
            const unsigned long long* keys = c.keys_of(c.img.data(), q);
            for (int t = 0; t < h.keys(k); ++t)
                if (keys[t] != incumbent_key(h.incumbent(k, t))) h.won(k, t, keys[t]);
        }
    return 0;
}

template <class H>
static int multi_commit_run(lqrrt_engine** engines, int n, const int32_t* horizons, int32_t* const* ids_out, int32_t* counts_out,
                            hipStream_t st, const H& h) {
    typedef typename H::Desc Desc;
    std::vector<int> room((size_t)n, 0), parent((size_t)n, -1);
    std::vector<long long> winner((size_t)n, 0);
    for (int k = 0; k < n; ++k) {
        counts_out[k] = 0;
        if (!h.winner(k)) continue;                             // (not part of the launch)
        room[k] = h.room(k);
        parent[k] = h.parent(k);
        winner[k] = 1;
    }
    std::vector<MultiChunk> chunks = multi_chunks(winner);
    StreamDrain drain(st);
    for (MultiChunk& c : chunks) {
        const size_t m = c.members.size();
        Carve carve;
        multi_commit_head(c, room, carve);
        const size_t o_desc = carve(sizeof(Desc) * m);
        std::vector<typename H::Part> at;
        for (size_t q = 0; q < m; ++q) at.push_back(h.carve(c, q, carve));
        c.img.assign(carve.off, 0);
        TRY(refine_multi_scratch(engines[c.first], carve.off, &c.dev));
        Desc* hd = (Desc*)(c.img.data() + o_desc);
        for (size_t q = 0; q < m; ++q) {
            hd[q].out = c.out_of(c.dev, q);
            hd[q].lens = c.lens_of(c.dev, q);
            hd[q].base = engines[c.members[q]]->N;
            h.fill(c, q, at, &hd[q]);
        }
        ProtoTable pt;
        size_t lds = 0;
        TRY(refine_multi_protos(engines, c, horizons, st, pt, lds));
        drain.arm();
        HIPCHK(hipMemcpyAsync(c.dev, c.img.data(), c.img.size(), hipMemcpyHostToDevice, st));
        DISPATCH(engines[0], h.template launch<S>((unsigned)m, lds, st, pt, (const Desc*)(c.dev + o_desc)));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(c.img.data(), c.dev, c.back, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));                           // the call's one synchronise
    drain.disarm();
    multi_commit_adopt(engines, chunks, parent, ids_out, counts_out);
    return 0;
}

// every argument of every engine, before anything is written or launched; bufs[k]: engine k's plan and cost prefix
static int refine_multi_check(lqrrt_engine** engines, int n, const int32_t* const* plans, const int32_t* plan_lens, const int32_t* tries,
                              const int32_t* horizons, std::vector<std::vector<int>>& bufs) {
    return multi_engines_check(engines, n, plans && plan_lens && tries && horizons, [&](int k) {
        bufs.emplace_back();
        return refine_check(engines[k], plans[k], plan_lens[k], tries[k], horizons[k], bufs.back());
    });
}

// The refinement's hooks.  What its search and its commit share: behind the descriptors the members' plans with their cost
// prefixes (bufs[k]), and the argument block of a RefineDesc.
struct RefineMulti {
    typedef RefineDesc Desc;
    typedef size_t Part;                                        // where the member's plan lies
    lqrrt_engine** engines;
    const std::vector<std::vector<int>>& bufs;
    const int32_t* plan_lens; const int32_t* tries; const int32_t* horizons;
    size_t carve(const MultiChunk& c, size_t q, Carve& carve) const { return carve(sizeof(int) * bufs[c.members[q]].size()); }
    void fill(MultiChunk& c, size_t q, const std::vector<size_t>& at, RefineDesc* d) const {
        const int k = c.members[q];
        memcpy(c.img.data() + at[q], bufs[k].data(), sizeof(int) * bufs[k].size());
        refine_fill_args(engines[k], (const int*)(c.dev + at[q]), plan_lens[k], tries[k], horizons[k], &d->a);
    }
};

struct RefineSearchMulti : RefineMulti {
    const int64_t* incumbents; int64_t* cost; int32_t* i_out; int32_t* j_out;
    long long groups(int k) const { return refine_candidates(plan_lens[k]); }
    int keys(int) const { return 1; }
    int64_t incumbent(int k, int) const { return incumbents[k]; }
    void fill(MultiChunk& c, size_t q, const std::vector<size_t>& at, RefineDesc* d) const {
        RefineMulti::fill(c, q, at, d);
        d->i = d->j = -1;
        d->best = c.keys_of(c.dev, q);
    }
    template <class S>
    static void launch(unsigned grid, size_t lds, hipStream_t st, const ProtoTable& pt, const RefineDesc* ds, const RetainGrid& gr) {
        hipLaunchKernelGGL((k_refine_search_multi<S>), dim3(grid), dim3(64), lds, st, pt, ds, gr);
    }
    void won(int k, int, unsigned long long key) const { refine_decode(key, &cost[k], &i_out[k], &j_out[k]); }
};

// The replay of one candidate (ci[k], cj[k]) per engine with a winner (ci[k] >= 0).  connect_goals' commit is this one too: per
// winner the one-node plan [v] with the cost prefix [depth[v]] and the candidate (0, 0).
struct RefineCommitMulti : RefineMulti {
    const int32_t* ci; const int32_t* cj;
    bool winner(int k) const { return ci[k] >= 0; }
    int room(int k) const { return plan_lens[k] - 1 - cj[k] + tries[k]; }
    int parent(int k) const { return bufs[k][(size_t)ci[k]]; }
    void fill(MultiChunk& c, size_t q, const std::vector<size_t>& at, RefineDesc* d) const {
        RefineMulti::fill(c, q, at, d);
        d->i = ci[c.members[q]]; d->j = cj[c.members[q]];
    }
    template <class S>
    static void launch(unsigned m, size_t lds, hipStream_t st, const ProtoTable& pt, const RefineDesc* ds) {
        hipLaunchKernelGGL((k_refine_commit_multi<S>), dim3(m), dim3(64), lds, st, pt, ds, (int)m);
    }
};

extern "C" int lqrrt_refine_search_multi(lqrrt_engine** engines, int n, const int32_t* const* plans, const int32_t* plan_lens,
                                         const int32_t* goal_tries, const int32_t* horizon_iters, const int64_t* incumbents,
                                         int64_t* cost_out, int32_t* i_out, int32_t* j_out, void* stream) {
    std::vector<std::vector<int>> bufs;
    TRY(refine_multi_check(engines, n, plans, plan_lens, goal_tries, horizon_iters, bufs));
    if (!incumbents || !cost_out || !i_out || !j_out) return fail(LQRRT_E_ARG, "null argument");
    for (int k = 0; k < n; ++k) {
        TRY(incumbent_check(incumbents[k], k));
        TRY(refine_candidates_check(plan_lens[k]));
    }
    TRY(use_device(engines[0]));
    for (int k = 0; k < n; ++k) { cost_out[k] = incumbents[k]; i_out[k] = -1; j_out[k] = -1; }
    return multi_search_run(engines, n, horizon_iters, (hipStream_t)stream,
                            RefineSearchMulti{{engines, bufs, plan_lens, goal_tries, horizon_iters}, incumbents, cost_out, i_out, j_out});
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
    return multi_commit_run(engines, n, horizon_iters, ids_out, counts_out, (hipStream_t)stream,
                            RefineCommitMulti{{engines, bufs, plan_lens, goal_tries, horizon_iters}, i, j});
}
