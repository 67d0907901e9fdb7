/*
 * lqrrt_hip.h -- C ABI of the MI355X (gfx950) lqRRT expansion engine.
 *
 * This is the drop-in boundary for the reference's extend path.  The reference
 * (jnez71/lqRRT) has no FFI: its hot path is Python calling user callbacks.  Each entry
 * point below names the reference code it replaces (file:line relative to the reference
 * tree); INTEGRATION.md shows the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error (LQRRT_E_*); the message is
 *     available from lqrrt_last_error(); nothing throws or aborts across the ABI;
 *   - all floating point is IEEE double; node/sample indices are int32;
 *   - "dev" pointers are device (HBM) addresses, e.g. torch tensor.data_ptr();
 *     "host" pointers are ordinary process memory;
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream); launches are
 *     asynchronous on it unless the function returns data to the host;
 *   - an engine handle owns its device buffers; handles are independent.  Process-wide state is limited to: the RCCL entry
 *     points, resolved once under std::call_once (lqrrt_comm_*), the environment switches, each read once, and the
 *     accumulators of the LQRRT_HOSTPROF / STEER_TIMING measurement builds (debug levers, not thread-safe, off by default).
 *
 * Layouts (all in HBM)
 *   tree state   : SoA, component d of node i at state[d*capacity + i]   (coalesced scans)
 *   tree trig    : cos/sin of every wrapped (angular) state, [2*NW][capacity]
 *   tree gains   : K of node i at K[i*m*n .. ) row-major m x n            (planner.py:373)
 *   tree edges   : node i owns xedge[i][H][n], uedge[i][H][m] + edge_len[i] (tree.py:69-70,90-93)
 *   ignore set   : 1 bit per node, 64 nodes per uint64 word               (planner.py:173,270)
 *   wave records : one fixed-size record per sample, see lqrrt_record_layout()
 */
#ifndef LQRRT_HIP_H
#define LQRRT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LQRRT_ABI_VERSION 1

/* error codes */
#define LQRRT_OK            0
#define LQRRT_E_ARG        -1   /* bad argument (the reference raises ValueError) */
#define LQRRT_E_HIP        -2   /* HIP runtime failure */
#define LQRRT_E_NODEVICE   -3   /* no usable gfx950 device */
#define LQRRT_E_CAPACITY   -4   /* tree / pool capacity exceeded */
#define LQRRT_E_STATE      -5   /* call sequence error (e.g. no goal, no tree) */

/* problem plugins compiled into the engine (the callbacks defined in the reference's demo scripts) */
#define LQRRT_MODEL_BOAT_ADVANCED      1  /* demos/demo_boat_advanced.py:78-225     */
#define LQRRT_MODEL_BOAT_INTERMEDIATE  2  /* demos/demo_boat_intermediate.py:48-210 */
#define LQRRT_MODEL_BOAT_NOVICE        3  /* demos/demo_boat_novice.py:45-164       */
#define LQRRT_MODEL_CAR                4  /* demos/demo_car.py:46-180               */
#define LQRRT_MODEL_PENDULUM           5  /* demos/demo_pendulum.py:54-157          */
#define LQRRT_MODEL_DOUBLE_INTEGRATOR  6  /* BASELINE.json config 5 (not in the reference) */
#define LQRRT_MODEL_ROS_BOAT           7  /* demos/lqrrt_ros/behaviors/{boat,car,escape}.py  */
#define LQRRT_MODEL_PENDULUM_LQR       8  /* demos/demo_pendulum.py dynamics with the lqr of the API contract (planner.py:39-42):
                                           * S, K from the discrete Riccati equation of the dynamics linearised about (x,u) by
                                           * central differences, recomputed per rollout step, per new node and per sample */

#define LQRRT_MODEL_BOAT_NOVICE_LQR    9  /* demos/demo_boat_novice.py dynamics (6 states, 3 controls) with the same Riccati lqr,
                                           * linearised about (x, 0): the north-star steer pipeline at the metric's dimension */

#define LQRRT_MODEL_USER               100  /* an out-of-tree problem compiled in with -DLQRRT_USER_SYSTEM='"header.hpp"'
                                             * (lqrrt_amd/csrc/models.def) */

#define LQRRT_MODEL_GENERIC            200  /* NO plugins compiled in: the reference's plugin API proper, arbitrary host callables
                                             * (planner.py:35-59, constraints.py:27).  The caller runs sample / steer / feasibility on the
                                             * host, in the reference's order (lqrrt_amd/callback.py), and the engine holds what the
                                             * reference spends 74-95 % of its time on: the node table (SoA states + cos/sin of the angular
                                             * ones, parents, ignore set) and Planner._costs_to_go + the nearest selection
                                             * (planner.py:239-247, 340-350).  lqrrt_system_desc: nstates 1..64 (beyond LQRRT_MAX_STATES the state dimension is a run-time value of the
                                             * kernels: host-form queries only), ncontrols (kept,
                                             * not used), params[0] = number of angular states (erf wraps them, e.g. demo_car.py:115-126),
                                             * params[1..] = their indices, ascending; no geometry.  Entry points that work: lqrrt_engine_create /
                                             * destroy, lqrrt_tree_reset / load / append / truncate / mark / rewind / size / set_ignored /
                                             * get_states / get_parents / get_ignored, lqrrt_nn_argmin, lqrrt_nn_argmin_host, lqrrt_nn_argmin_errors,
                                             * lqrrt_costs_to_go; every other one returns LQRRT_E_STATE. */

#define LQRRT_MAX_STATES   12
#define LQRRT_MAX_CONTROLS 6
#define LQRRT_MAX_PARAMS   96

typedef struct lqrrt_engine lqrrt_engine;

/* Plain-data description of a problem: replaces the python callables handed to
 * Planner.__init__ / Constraints.__init__ (planner.py:85-100, constraints.py:31-35). */
typedef struct {
    int32_t model;                    /* LQRRT_MODEL_*                                  */
    int32_t nstates, ncontrols;       /* constraints.py:32-33                            */
    int32_t n_params;                 /* doubles used in params[]                        */
    double  params[LQRRT_MAX_PARAMS]; /* model constants, layout in lqrrt_amd/systems.py */
    int32_t n_vertices;               /* V: body-frame hull points, vps is 2 x V row-major */
    int32_t n_obstacles;              /* O: rows of obs                                  */
    int32_t obs_stride;               /* doubles per obstacle: 3 = circle [x,y,r], 6 = box [lo3,hi3] */
    int32_t reserved;
    const double* vps;                /* host, may be NULL when V == 0                   */
    const double* obs;                /* host, may be NULL when O == 0                   */
    /* Optional occupancy-grid collision model for the planar vehicles (the ROS node's is_feasible,
     * demos/lqrrt_ros/nodes/lqrrt_node.py:719-745): when ogrid != NULL it replaces the circle sweep.
     * Cell of a hull point p: (int64)(cpm * (p - origin)) (truncation toward zero), value looked up
     * as ogrid[iy][ix] with NumPy's index rules (negative indices wrap once, anything else outside
     * is infeasible); feasible iff every value < threshold. */
    const int8_t* ogrid;              /* host, row-major [og_rows][og_cols], or NULL     */
    int32_t og_rows, og_cols;
    double  og_origin[2];
    double  og_cpm;                   /* cells per metre = 1 / resolution                */
    double  og_threshold;
} lqrrt_system_desc;

/* Resolution + goal (Planner.set_resolution planner.py:517-553, set_goal :468-487). */
typedef struct {
    double  dt;                          /* planner.py:86                                 */
    double  FPR;                         /* failed-path retention, planner.py:394-395     */
    int32_t horizon_iters;               /* int(horizon/dt), planner.py:549               */
    int32_t has_goal;
    double  error_tol[LQRRT_MAX_STATES]; /* planner.py:428,533                            */
    double  goal[LQRRT_MAX_STATES];      /* planner.py:476                                */
    double  goal_lo[LQRRT_MAX_STATES];   /* goal - buffer, strict test planner.py:442-447 */
    double  goal_hi[LQRRT_MAX_STATES];   /* goal + buffer                                 */
    /* Adaptive-horizon heuristic (horizon given as (min,max), planner.py:418-425, 538-547).  Because the
     * reference doubles horizon_iters whenever the step counter reaches it, a rollout is never stopped
     * by the horizon before max/dt steps; what the mode changes is the extra stop rule "every error
     * component grew -> discard the edge".  horizon_iters above must then be int(max/dt); the engine
     * replays the halving/doubling of the reference's horizon_iters over the committed attempts
     * (lqrrt_engine_horizon_iters) starting from horizon_iters_state, clipped to [hspan_min, horizon_iters]. */
    int32_t adaptive;
    int32_t hspan_min;
    int32_t horizon_iters_state;
    int32_t reserved;
} lqrrt_resolution;

/* Default sampler description (planner.py:176-211). */
typedef struct {
    double  centers[LQRRT_MAX_STATES];   /* mean(sample_space,1), planner.py:197          */
    double  spans[LQRRT_MAX_STATES];     /* diff(sample_space),   planner.py:198          */
    double  goal_bias[LQRRT_MAX_STATES]; /* planner.py:179-185                            */
    int32_t tries_limit;                 /* planner.py:188-191                            */
    int32_t reserved;
} lqrrt_sampler_desc;

/* Counters returned by lqrrt_engine_extend (host side). */
typedef struct {
    int64_t attempts;        /* extension attempts committed (= reference loop iterations) */
    int64_t accepted;        /* nodes appended                                             */
    int64_t candidates;      /* (n+1)-double sampler rows consumed from the MT19937 stream */
    int64_t waves;           /* waves launched                                             */
    int64_t fix_rounds;      /* exact-mode repair rounds (beyond the speculative pass)     */
    int64_t resteers;        /* samples re-steered in repair rounds                        */
    int64_t goal_hits;       /* accepted nodes inside the goal region                      */
    int64_t speculated;      /* samples evaluated (>= attempts: discarded tails included)  */
    int64_t chain_slots;     /* sum over waves of 1 + the longest chain of in-wave parents among the committed samples: the
                              * rollouts that HAD to run one after another (a child cannot be steered before the parent it
                              * starts from exists) -- the dependency bound of the exact-mode schedule, in launches          */
    int32_t tree_size;       /* nodes after the call                                       */
    int32_t stop_reason;     /* LQRRT_STOP_*                                               */
} lqrrt_extend_stats;

#define LQRRT_STOP_ATTEMPTS  1  /* max_attempts reached                                  */
#define LQRRT_STOP_NODES     2  /* tree.size > max_nodes (planner.py:311)                */
#define LQRRT_STOP_TARGET    3  /* tree.size >= until_size                                */
#define LQRRT_STOP_GOAL      4  /* a goal hit was committed and stop_on_goal was set      */

/* ---------------------------------------------------------------- lifecycle ---------- */

const char* lqrrt_last_error(void);

/* The environment switches this library reads (each once per process), one per line: "NAME  (default d)  effect" -- generated from
 * the one table lqrrt_amd/csrc/switches.def.  None of them changes a result; they are measurement and test levers. */
const char* lqrrt_switches_describe(void);
int lqrrt_abi_version(void);

/* Number of usable HIP devices (0 when there is no GPU: every compute call then fails). */
int lqrrt_device_count(void);

/* Creates an engine on `device`.  capacity = max nodes the tree may hold,
 * max_wave = largest wave size W.  Replaces Planner.set_system (planner.py:557-592). */
int lqrrt_engine_create(const lqrrt_system_desc* sys, int device, int capacity, int max_wave,
                        lqrrt_engine** out);
int lqrrt_engine_destroy(lqrrt_engine* e);

/* Memory this engine holds: device_bytes (HBM: node pools sized by `capacity` -- per node 8 (n + 3 nw + 2 + m n) + 8 bytes and the
 * edge pools 8 horizon_iters (n + m); wave buffers sized by max_wave; geometry) and pinned_bytes (page-locked host memory).  Either
 * pointer may be NULL.  No counterpart in the reference, whose tree is Python lists; INTEGRATION.md section 6 tabulates it. */
int lqrrt_engine_footprint(lqrrt_engine* e, int64_t* device_bytes, int64_t* pinned_bytes);

/* Replaces the model parameters, hull points, obstacle table and occupancy grid of an existing engine (same
 * model); the tree is kept, queued samples are regenerated from the first uncommitted row of the stream.
 * This is what the ROS node does between plans when a new map arrives: module globals of the behaviour
 * files + Constraints.set_feasibility_function (lqrrt_node.py:65, 260-263, 719-745). */
int lqrrt_engine_set_geometry(lqrrt_engine* e, const lqrrt_system_desc* sys, void* stream);

/* Wave semantics.  EXACT (default): the result is the tree the reference's sequential loop
 * builds -- samples are speculated against the wave-start snapshot, validated against the nodes accepted earlier
 * in the wave and re-steered on conflict; the wave size is chosen adaptively.  SYNCHRONOUS: all samples of a
 * wave see the wave-start snapshot (nodes and ignore set), accepted edges are committed in sample order and
 * the goal bookkeeping of the wave's hits follows in that order; waves have exactly the size asked for
 * (lqrrt_engine_extend's `wave`), size 1 is the reference's loop.  Its parity target is the restatement of
 * this rule in oracle/lqrrt_oracle.c (orc_extend_sync). */
#define LQRRT_WAVE_EXACT        0
#define LQRRT_WAVE_SYNCHRONOUS  1
int lqrrt_engine_set_wave_mode(lqrrt_engine* e, int mode);

/* Restricts the engine's native loops (lqrrt_engine_extend, lqrrt_engine_extend_sharded) to a subset of the GPU's compute units:
 * they then run on an engine-private stream created with this CU mask (n_words 32-bit words; bit k = the k-th CU as the driver
 * numbers them, dealt round-robin to the XCDs: bit k is a CU of XCD k mod 8 on an MI355X).  The caller's stream is drained when such
 * a call begins and the private stream when it returns, so the call stays ordered on the caller's stream.  n_words = 0 lifts the
 * restriction.  No counterpart in the reference (planner.py has no notion of a device); speed only, results are unchanged.  Use: one
 * planner on one XCD keeps its working set in that XCD's L2; several planners on disjoint masks share a GPU without contending. */
int lqrrt_engine_set_cu_mask(lqrrt_engine* e, const uint32_t* mask, int n_words);

/* Changing horizon_iters re-lays out the edge pools: call lqrrt_tree_reset afterwards. */
int lqrrt_engine_set_resolution(lqrrt_engine* e, const lqrrt_resolution* r);

/* Current value of the reference's Planner.horizon_iters in adaptive mode (planner.py:421,424). */
int lqrrt_engine_horizon_iters(lqrrt_engine* e);

/* Constant dense cost-to-go matrix S = lqr(x,u)[0] of the system (host, n x n row-major);
 * NULL = identity, which is what every demo of the reference returns (e.g.
 * demo_boat_advanced.py:149).  Used by lqrrt_nn_argmin / lqrrt_costs_to_go / the waves. */
int lqrrt_engine_set_dense_S(lqrrt_engine* e, const double* S_host);
int lqrrt_engine_set_sampler(lqrrt_engine* e, const lqrrt_sampler_desc* s);

/* Legacy MT19937 state of numpy.random (planner.py:204-205 draws np.random.sample):
 * key[624] + position, exactly np.random.get_state()[1:3]. */
int lqrrt_engine_set_mt19937(lqrrt_engine* e, const uint32_t* key624, int pos);
int lqrrt_engine_get_mt19937(lqrrt_engine* e, uint32_t* key624, int* pos);

/* ---------------------------------------------------------------- tree --------------- */

/* Tree(seed_state, lqr(seed)) -- tree.py:50-73 via planner.py:172.  Clears the ignore set. */
int lqrrt_tree_reset(lqrrt_engine* e, const double* x0_host, void* stream);
int lqrrt_tree_size(lqrrt_engine* e);

/* Puts an existing tree on the device: the reference's Tree features state / lqr[.][1] / pID / x_seq / u_seq
 * (tree.py:50-96) as flat host arrays.  Replaces whatever tree the engine holds; lqrrt_engine_set_resolution must
 * have been called (the edge pools are laid out for its horizon_iters).  Uses: teacher-forced parity (the reference's
 * own tree resident while lqrrt_nn_argmin / lqrrt_steer_batch are compared decision by decision with
 * planner.py:236-257), and warm-starting a replan from a tree kept by the caller (lqrrt_node.py:389-500).
 *   states   [count][n]       tree.state
 *   K        [count][m][n]    tree.lqr[i][1]   (node S is never read on the path, planner.py:373)
 *   pID      [count]          pID[0] = -1, 0 <= pID[i] < i   (tree.py:83-84 raises ValueError otherwise)
 *   edge_len [count]          len(tree.x_seq[i]), 1..horizon_iters; NULL = every edge is the single state of its node
 *   xedge    [sum(edge_len)][n], uedge [sum(edge_len)][m]: the edges back to back in node order; NULL = xedge rows
 *            are the node's own state, uedge rows zero
 *   ignored  [count] 0/1      membership in planner.py:173,270's `ignores`; NULL = none
 * Goal bookkeeping (lqrrt_plan_best) starts empty; the sample stream and counters are not touched. */
int lqrrt_tree_load(lqrrt_engine* e, int count, const double* states_host, const double* K_host, const int32_t* pID_host,
                    const int32_t* edge_len_host, const double* xedge_host, const double* uedge_host,
                    const uint8_t* ignored_host, void* stream);

/* Tree.add_node(pID, state, lqr, x_seq, u_seq) (tree.py:77-96) from host data: appends ONE node.  K [m][n] = lqr[1]; the edge is
 * `len` rows of xseq [len][n] / useq [len][m] (NULL xseq: the state itself, NULL useq: zeros), 1 <= len <= horizon_iters.
 * LQRRT_MODEL_GENERIC: only state and parent go to the device (as arguments of one small launch, asynchronous on `stream`); K, xseq
 * and useq stay with the caller and must be NULL.  A non-existent parent is LQRRT_E_ARG with tree.py:84's message. */
int lqrrt_tree_append(lqrrt_engine* e, int parent, const double* state_host, const double* K_host, int len,
                      const double* xseq_host, const double* useq_host, void* stream);

/* Forgets every node with id >= size (nodes are only ever appended, so the first `size` nodes are exactly the tree
 * as it stood when it had that size).  Ignore bits of the dropped nodes are cleared, those of kept nodes stay: if a
 * dropped node was a goal hit, the caller restates the ignore set of the kept nodes with lqrrt_tree_set_ignored.  The best
 * plan is forgotten if its end node was dropped; a mark (lqrrt_tree_mark) beyond the new size becomes void. */
int lqrrt_tree_truncate(lqrrt_engine* e, int size);

/* Keeps the subtree below node `new_root` as the tree of the next plan, in place (Planner.replan; not in the reference, which
 * starts every plan from one node, planner.py:172).  The rule (tests/retain_reference.py restates it):
 *   ok[i]   = revalidate ? every recorded row of node i's edge passes the feasibility test under the engine's CURRENT geometry
 *             (lqrrt_engine_set_geometry) : true
 *   keep[i] = i == new_root, or i > new_root and ok[i] and keep[pID[i]]       (the root's own edge is not part of the new tree)
 * Kept nodes are renumbered in ascending old-id order; parents are remapped; the root gets parent -1 and the one-row edge of a
 * seed (its state, zero effort; tree.py:69-70) and keeps its gain; everything else moves bit for bit.  Goal bookkeeping
 * (lqrrt_plan_best) and the ignore set are rebuilt against the CURRENT goal box (lqrrt_engine_set_resolution): a hit is a kept
 * non-root node strictly inside it, best = fewest steps from the new root (its 1 included), lowest new id on ties, the ignore
 * set = the root paths of all hits.  A mark (lqrrt_tree_mark) becomes void; the sample stream and the counters are not touched.
 * old_to_new_host [old size] (or NULL) receives the new id of every old node, -1 = dropped.  Synchronous.  Scratch is
 * transient (freed before returning; DESIGN.md section 10 gives its size).  LQRRT_E_ARG: no such node (tree.py:84's message);
 * LQRRT_E_STATE: no tree / no resolution.  On a failure before the first array is moved the tree is unchanged. */
typedef struct {
    int32_t old_size, kept;
    int32_t outside;          /* not in the subtree of new_root                              */
    int32_t infeasible;       /* in the subtree, own edge fails                              */
    int32_t orphaned;         /* in the subtree, own edge passes, an ancestor was dropped    */
    int32_t root_feasible;    /* the test of the last row of the root's old edge (1 when revalidate == 0) */
    int32_t goal_hits, best_end;   /* best_end / best_steps: -1 without a hit               */
    int64_t best_steps;
} lqrrt_retain_stats;
int lqrrt_tree_retain(lqrrt_engine* e, int new_root, int revalidate, lqrrt_retain_stats* out, int32_t* old_to_new_host, void* stream);

/* lqrrt_tree_retain for n engines at once (lqrrt_amd.update_plans jobs with a `root`: a fleet that replans every tick): engine i
 * keeps the subtree below new_roots[i], revalidating when revalidate[i] != 0 (NULL: nobody revalidates), by the rule above -- every
 * tree, out[i], old_to_new_host[i] [old size of engine i] (the array or single entries may be NULL) and every engine's host state
 * are exactly what n calls of lqrrt_tree_retain give.  What is shared is the work around the kernels: every stage is ONE launch
 * whose grid spans the engines, and allocations, waits and copies are per call, not per engine (DESIGN.md section 10 gives the
 * transient scratch).  More than 32 engines run as consecutive chunks of up to 32 on `stream`.  Synchronous.
 * The engines share the device, the model, the horizon and the form of S (as in lqrrt_engine_extend_multi; Riccati systems are
 * welcome: a retain computes no gain), n <= 128, and no engine appears twice.  EVERY argument of EVERY engine is checked before
 * anything is written, with lqrrt_tree_retain's codes and messages.  A failure before the first array of the first chunk is moved
 * (arguments, allocation of the scratch) leaves all trees unchanged; after a later failure the trees of the call's engines are
 * undefined, as after a failed lqrrt_engine_extend_multi: lqrrt_tree_reset or lqrrt_tree_load them before they are used again. */
int lqrrt_tree_retain_multi(lqrrt_engine** engines, int n, const int32_t* new_roots, const int32_t* revalidate,
                            lqrrt_retain_stats* out, int32_t** old_to_new_host, void* stream);

/* Which plans in the tree stay clear of obstacles that MOVE (Planner.avoid): D discs of radii radii_host[D] whose centres
 * tracks_host [L][D][2] (world x, y) are given at L consecutive instants spaced by the engine's dt; row `start` >= 0 of the
 * table coincides with the root's row, and a track that has ended stays where it ended (row min(tau, L - 1)).  The rule
 * (tests/clear_reference.py): cum[0] = edge length of the root, cum[i] = cum[pID[i]] + edge length of i;
 * row k of node i > 0 has time index tau = start + cum[pID[i]] + k, the root's row tau = start.  A row is tested with the
 * model's feasibility test against the D discs of its instant and nothing else -- no static obstacle, no occupancy grid -- each
 * disc a circular obstacle exactly as the static map derives one (the novice boats' inflation included).
 *   first[i]  = the smallest tau of a failing row over the edges of the nodes from i up to and including the root, or -1
 *   dwell[i]  = for a goal hit (a non-root node strictly inside the current goal box): the smallest tau' with
 *               start + cum[i] - 1 < tau' <= L - 1 at which its last row fails against the discs of tau', or -1; -2 for any other node
 *   best      = the hit with first == -1 and dwell == -1 that has the fewest steps cum, lowest id on ties
 * first_host / dwell_host [tree size] (or NULL) receive the per-node arrays.  The tree is not modified: pools, parents, ignore
 * set, lqrrt_plan_best, sample stream and counters stay as they were; all device memory of the call is transient and
 * lqrrt_engine_footprint is the same before and after.  Synchronous.  Every argument is checked before anything is enqueued:
 * LQRRT_E_ARG for L < 1, D < 1, start < 0, a position that is not finite, a radius that is not >= 0, start + the deepest cum
 * beyond 31 bits, or hull points that do not fit in a workgroup's LDS; LQRRT_E_STATE for no tree, no goal, or a model whose
 * feasibility test has no circle path (the pendulums, the double integrator, LQRRT_MODEL_GENERIC, an out-of-tree model that
 * does not declare DISCS). */
typedef struct {
    int32_t size;             /* nodes of the tree                                            */
    int32_t conflicts;        /* nodes with a failing row on their own edge                   */
    int32_t blocked;          /* nodes whose own edge is clear and an ancestor's is not       */
    int32_t hits, clear_hits; /* goal hits; those with first == -1 and dwell == -1            */
    int32_t best_end;         /* -1 without a clear hit                                       */
    int64_t best_steps;       /* cum of best_end; -1 without a clear hit                      */
} lqrrt_clear_stats;
int lqrrt_tree_clear(lqrrt_engine* e, const double* tracks_host, const double* radii_host, int L, int D, int start,
                     lqrrt_clear_stats* out, int32_t* first_host, int32_t* dwell_host, void* stream);

/* lqrrt_tree_clear for `waits` departure delays at once (Planner.avoid with max_wait): the vehicle may hold the root's row for
 * w = 0 .. waits - 1 rows of dt before it leaves, 1 <= waits <= 64, and every per-node answer is a 64-bit mask over w.  Tracks,
 * radii, L, D, start, cum, the clamp min(tau, L - 1), the row test and the goal hit are lqrrt_tree_clear's.  The rule
 * (tests/clear_wait_reference.py), for delay w:
 *   wait       the root's row is tested at every tau = start .. start + w; root_ok bit w = all of them pass (so root_ok is
 *              prefix-closed: above a 0 bit every bit is 0)
 *   edges      row k of node i > 0 has tau = start + w + cum[pID[i]] + k; own_ok[i] bit w = every row of i's edge passes;
 *              own_ok[0] = root_ok
 *   clear[i]   = own_ok[i] & clear[pID[i]]: the AND over the nodes from i up to and including the root
 *   dwell_ok[i] for a goal hit: bit w = its last row passes at every tau' in [start + w + cum[i], L - 1] (an empty range passes);
 *              0 for any other node
 *   best       over hits i and delays w set in clear[i] & dwell_ok[i]: the smallest (w + cum[i], i)
 * Bit w of clear[i] is therefore (first[i] == -1 of lqrrt_tree_clear at start + w) && root_ok bit w, and bit w of dwell_ok[i] is
 * (dwell[i] == -1 of that call).  clear_host / dwell_host [tree size] (or NULL) receive the per-node masks.  Reads only and
 * synchronous, as lqrrt_tree_clear: all device memory of the call is transient.  Every argument is checked before anything is
 * enqueued: lqrrt_tree_clear's refusals, LQRRT_E_ARG for waits outside 1 .. 64, and LQRRT_E_ARG when
 * start + (waits - 1) + the deepest cum goes beyond 31 bits. */
typedef struct {
    int32_t size;             /* nodes of the tree                                                    */
    int32_t hits;             /* goal hits                                                            */
    int32_t clear_hits;       /* hits with clear & dwell_ok != 0: clear at some delay                 */
    int32_t clear_now;        /* hits with bit 0 set in both: lqrrt_tree_clear's clear_hits           */
    int32_t best_end;         /* -1 without a clear hit                                               */
    int32_t best_wait;        /* the delay of the best; -1 without                                    */
    int64_t best_steps;       /* cum of best_end, without the wait; -1 without                        */
    int64_t best_arrival;     /* best_wait + best_steps; -1 without                                   */
} lqrrt_clear_wait_stats;
int lqrrt_tree_clear_wait(lqrrt_engine* e, const double* tracks_host, const double* radii_host, int L, int D, int start, int waits,
                          lqrrt_clear_wait_stats* out, uint64_t* clear_host, uint64_t* dwell_host, void* stream);

/* lqrrt_tree_clear against D oriented RECTANGLES instead of discs (Planner.avoid_rects; DESIGN.md section 21;
 * tests/clear_rects_reference.py restates the rule): tracks_host [L][D][3] = world x, y and heading of rectangle d at each of L
 * consecutive instants, extents_host [D][2] = (a, b), the half length along the heading and the half width, both >= 0.
 * cum, tau = start + cum[pID[i]] + k, the root's one row at tau = start, table row min(tau, L - 1), first / dwell, best = the
 * smallest (cum, id) among the hits with first == dwell == -1 and the counters are lqrrt_tree_clear's word for word, with "disc"
 * read as "rectangle".  Only the test of one row is new:
 *   table     per (instant, rectangle) the host derives co, so = lq_sincos(heading) (include/lqrrt_pmath.h: the function the
 *             vehicle's own heading goes through); for the novice boats a' = a + params[18], b' = b + params[18] (the half boat
 *             length that inflates their circles), for every other model a' = a, b' = b
 *   points    the hull-sweeping models (BoatAdvanced, BoatIntermediate, RosBoat, Car): the hull points, placed as the static
 *             test places them, vx = px + (c*bx + (-s)*by), vy = py + (s*bx + c*by) with c, s the row's portable cos / sin;
 *             the novice boats: the one point (px, py)
 *   test      dx = vx - ox; dy = vy - oy; xi = co*dx + so*dy; eta = co*dy + (-so)*dx;
 *             inside = (fabs(xi) <= a') && (fabs(eta) <= b')      -- fp64, these operations in this order, nothing contracted
 *   a row fails when some point is inside some rectangle of its instant.
 * Left out on purpose: the test is geometry only -- no static map and no occupancy grid, as in lqrrt_tree_clear; the car's extra
 * vertex at 2p is not used (it restates a quirk of the reference's circle test, and the reference has no rectangle); BoatAdvanced's
 * planning speed box is not used (rows in a tree have passed it).  The kernel may cull rectangles conservatively; the answers are
 * those of the test above on every (point, rectangle) pair.
 * Reads only and synchronous, as lqrrt_tree_clear: all device memory of the call is transient.  Every argument is checked before
 * anything is enqueued, in lqrrt_tree_clear's order: LQRRT_E_ARG for a null argument, L < 1, D < 1, start < 0, a table that is too
 * large, an x, y or heading that is not finite, an extent that is not >= 0 and finite; LQRRT_E_STATE for a model without the path
 * (lqrrt_tree_clear's models have it), no tree, no goal, parents that do not ascend; LQRRT_E_ARG for start + the deepest cum beyond
 * 31 bits or hull points that do not fit in a workgroup's LDS (the launch reserves exactly 16 V bytes). */
int lqrrt_tree_clear_rects(lqrrt_engine* e, const double* tracks_host /*[L][D][3]*/, const double* extents_host /*[D][2]*/,
                           int L, int D, int start, lqrrt_clear_stats* out, int32_t* first_host, int32_t* dwell_host, void* stream);

/* lqrrt_tree_clear_rects for `waits` departure delays at once (Planner.avoid_rects with max_wait; DESIGN.md section 22;
 * tests/clear_rects_wait_reference.py restates the rule).  Nothing is new: the rule is lqrrt_tree_clear_wait's comment above --
 * wait, edges, clear, dwell_ok, best, the counters of lqrrt_clear_wait_stats -- with "the row test" read as the test of
 * lqrrt_tree_clear_rects's comment above: table, points and test as stated there, geometry only, what is left out there left out
 * here.  tracks_host, extents_host, L, D, start are lqrrt_tree_clear_rects's; waits, out, clear_host, dwell_host are
 * lqrrt_tree_clear_wait's.  Bit w of clear[i] is therefore (first[i] == -1 of lqrrt_tree_clear_rects at start + w) && root_ok bit
 * w, where root_ok bit w = the root's row passes at every tau = start .. start + w, and bit w of dwell_ok[i] is (dwell[i] == -1 of
 * that call), 0 for a node that is no hit.  One call replaces `waits` calls of lqrrt_tree_clear_rects and the test of the root's
 * row during the wait.  Reads only and synchronous: all device memory of the call is transient (92 bytes per node and the table).
 * Every argument is checked before anything is enqueued: lqrrt_tree_clear_rects's refusals in their order, with LQRRT_E_ARG for
 * waits outside 1 .. 64 behind the extents, LQRRT_E_ARG when start + (waits - 1) + the deepest cum goes beyond 31 bits, and the
 * hull points' 16 V bytes + 64 against a workgroup's LDS. */
int lqrrt_tree_clear_rects_wait(lqrrt_engine* e, const double* tracks_host /*[L][D][3]*/, const double* extents_host /*[D][2]*/,
                                int L, int D, int start, int waits, lqrrt_clear_wait_stats* out, uint64_t* clear_host,
                                uint64_t* dwell_host, void* stream);

/* lqrrt_tree_clear and lqrrt_tree_clear_wait for n engines at once (lqrrt_amd.avoids, deconflict(batched=True): a fleet that
 * checks its plans every tick against tracked traffic).  The rule is the one stated above (DESIGN.md sections 16 and 17),
 * unchanged: member k's out[k] and per-node arrays are exactly what the one-tree call on engines[k] with tracks_host[k],
 * radii_host[k], L[k], D[k], start[k] (and waits[k]) gives -- every counter, every per-node value.  first_host / dwell_host
 * (clear_host / dwell_host) are arrays of n pointers, each [tree size of engine k]; the array or single entries may be NULL.
 * What is shared is the work around the kernels: every stage is ONE launch whose grid spans the engines,
 * and there is one allocation per chunk of up to 32 engines and one synchronise per call.  Members that pass the same
 * tracks_host[k] and radii_host[k] pointers with equal L and D (the novice boats: and equal inflation) share one uploaded table.
 * Nothing of any tree is written; all device memory of the call is transient and no engine's lqrrt_engine_footprint changes.
 * Synchronous.  The engines share the device and the model, n <= 128, no engine appears twice, none is generic.  EVERY argument
 * of EVERY member is checked before anything is allocated or enqueued, with the one-tree calls' codes and messages followed by
 * "(engine k)"; a refused call writes nothing into any output. */
int lqrrt_tree_clear_multi(lqrrt_engine** engines, int n, const double* const* tracks_host, const double* const* radii_host,
                           const int32_t* L, const int32_t* D, const int32_t* start, lqrrt_clear_stats* out /*[n]*/,
                           int32_t* const* first_host, int32_t* const* dwell_host, void* stream);
int lqrrt_tree_clear_wait_multi(lqrrt_engine** engines, int n, const double* const* tracks_host, const double* const* radii_host,
                                const int32_t* L, const int32_t* D, const int32_t* start, const int32_t* waits,
                                lqrrt_clear_wait_stats* out /*[n]*/, uint64_t* const* clear_host, uint64_t* const* dwell_host, void* stream);

/* lqrrt_tree_clear_rects and lqrrt_tree_clear_rects_wait for n engines at once (lqrrt_amd.avoids_rects: a fleet of long hulls in a
 * channel that checks its plans every tick against tracked hulls).  The rule is the one stated at those two calls (DESIGN.md
 * sections 21 and 22), unchanged: member k's out[k] and per-node arrays are exactly what the one-tree call on engines[k] with
 * tracks_host[k] ([L[k]][D[k]][3]), extents_host[k] ([D[k]][2]), L[k], D[k], start[k] (and waits[k]) gives -- every counter, every
 * per-node value.  Everything else is lqrrt_tree_clear_multi's comment above with "radii" read as "extents" (DESIGN.md section
 * 23): the output arrays of n pointers, ONE launch per stage whose grid spans the engines, one allocation per chunk of up to 32
 * engines and one synchronise per call; members that pass the same tracks_host[k] and extents_host[k] pointers with equal L and D
 * (the novice boats: and equal inflation) share one uploaded table, its extents included; nothing of any tree is written, all
 * device memory of the call is transient and no engine's lqrrt_engine_footprint changes.  Synchronous.  The engines share the
 * device and the model, n <= 128, no engine appears twice, none is generic.  EVERY argument of EVERY member is checked, in list
 * order, before anything is allocated or enqueued, with lqrrt_tree_clear_rects's / lqrrt_tree_clear_rects_wait's codes and messages
 * followed by "(engine k)"; a refused call writes nothing into any output. */
int lqrrt_tree_clear_rects_multi(lqrrt_engine** engines, int n, const double* const* tracks_host, const double* const* extents_host,
                                 const int32_t* L, const int32_t* D, const int32_t* start, lqrrt_clear_stats* out /*[n]*/,
                                 int32_t* const* first_host, int32_t* const* dwell_host, void* stream);
int lqrrt_tree_clear_rects_wait_multi(lqrrt_engine** engines, int n, const double* const* tracks_host, const double* const* extents_host,
                                      const int32_t* L, const int32_t* D, const int32_t* start, const int32_t* waits,
                                      lqrrt_clear_wait_stats* out /*[n]*/, uint64_t* const* clear_host, uint64_t* const* dwell_host,
                                      void* stream);

/* lqrrt_tree_clear and lqrrt_connect_search in one call (Planner.avoid(connect); DESIGN.md section 19;
 * tests/clear_connect_reference.py): when every goal hit of the tree is crossed by the discs, or only a long one is clear, which
 * node whose root path is clear reaches the goal by a short chain of goal-directed steers that stays clear too?  Everything of
 * lqrrt_tree_clear holds unchanged and is computed first -- cum, tau, the clamp min(tau, L - 1), the row test against the D discs
 * of that instant alone, first, dwell, best and every counter of *out.  On top of that:
 *   incumbent  = depth of the best clear hit in lqrrt_connect_search's cost units (depth[0] = 1, depth[v] = depth[pID[v]] + edge
 *                length of v, so depth = cum - edge length of the root + 1); 2^31 - 1 without a clear hit.  None is passed in.
 *   candidate  = a node v with first[v] == -1: every such node, or those among nodes_host[count] (NULL: every node).  The
 *                propagated first counts: a node below a conflict is no candidate; the root is one when its row passes at start.
 *   chain      = exactly lqrrt_connect_search's: up to goal_tries steers at the goal against the STATIC map with the fixed horizon
 *                horizon_iters, an empty edge ends it, valid when an edge ends strictly inside the goal box.  The discs cut no
 *                edge, they accept or reject the chain: lqrrt_connect_commit(v, goal_tries, horizon_iters), unchanged, replays
 *                exactly the chain that was judged.
 *   time       = row k of the chain's j-th non-empty edge has tau = start + cum[v] + (rows of the chain's earlier edges) + k,
 *                which is the time lqrrt_tree_clear gives that row after a commit.  A chain is clear when every row of every edge
 *                passes at its tau and its last row passes at every tau' in [start + cum[v] + chain rows, L - 1] (the wait at the
 *                goal; an empty range passes).
 *   winner     = the valid and clear candidate of smallest (cost, v) with cost = depth[v] + chain rows < incumbent -- strictly: a
 *                chain that only ties with the best clear hit does not win.  The search stops a chain early as
 *                lqrrt_connect_search does (key cost << 32 | v, seeded with incumbent << 32, lowered by valid and clear chains
 *                only), so the winner depends neither on scheduling nor on the order of the id list.
 * Reads only and synchronous, as lqrrt_tree_clear: all device memory of the call is one transient allocation, and everything is
 * enqueued back to back on the stream with one wait.  Every argument is checked before anything is allocated or enqueued:
 * first lqrrt_tree_clear's refusals in their order, then lqrrt_connect_search's (goal_tries < 1, horizon_iters outside the edge
 * pools, an id outside the tree, depths beyond 32 bits), then LQRRT_E_ARG when the search's LDS -- the refinement's layout plus
 * 16 V bytes of hull points for the disc test -- exceeds the device's limit.  A refused call writes nothing into any output. */
typedef struct {
    int32_t clear_candidates; /* candidates with first == -1 (entries of the id list, or nodes)       */
    int32_t chain_from;       /* v, the winning candidate; -1 without a winner                        */
    int32_t chain_rows;       /* rows of the winning chain; -1 without                                */
    int32_t reserved;
    int64_t chain_cost;       /* depth[v] + chain rows; -1 without                                    */
    int64_t chain_arrival;    /* cum[v] + chain rows: best_steps after a commit; -1 without           */
} lqrrt_clear_connect_stats;
int lqrrt_tree_clear_connect(lqrrt_engine* e, const double* tracks_host, const double* radii_host, int L, int D, int start,
                             int horizon_iters, int goal_tries, const int32_t* nodes_host, int count /* nodes_host NULL: every node */,
                             lqrrt_clear_stats* out, lqrrt_clear_connect_stats* chain, int32_t* first_host, int32_t* dwell_host,
                             void* stream);

/* lqrrt_tree_clear_connect for n trees in one call (lqrrt_amd.avoids(connect)).  Member k answers EXACTLY as
 * lqrrt_tree_clear_connect(engines[k], tracks_host[k], radii_host[k], L[k], D[k], start[k], horizon_iters[k], goal_tries[k],
 * nodes_host ? nodes_host[k] : NULL, counts[k], out + k, chain + k, first_host ? first_host[k] : NULL, dwell_host ? dwell_host[k] : NULL)
 * does: the seven counters, first, dwell_first, the five chain fields, clear_candidates with its "entries of an id list are counted,
 * not nodes" rule.  nodes_host: NULL, or per engine NULL (every node) or an id list of counts[k] entries (it may repeat ids, and it
 * may be empty: the member then gets its clearance answer and no chain); counts is read only where a list is given.  Nothing of any
 * tree is written; a winner is replayed by lqrrt_connect_commit(_multi).
 * Execution: per chunk of up to 32 members one transient allocation and one uploaded image; the stages of lqrrt_tree_clear_multi,
 * one launch each over the chunk; one launch that seeds every member's key; one search launch over the members' candidates back to
 * back, every member with a key of its own (the early stop prunes within one tree only); the copies back.  The chunks are enqueued
 * back to back and waited for once.  Members that pass the same tracks and radii arrays with equal L and D share one table.
 * Refusals, all before anything is allocated or enqueued, the message naming the engine, and a refused call writes nothing into any
 * output: no engines, a null argument (chain included), more than 128 engines, a null or generic engine, an engine twice, mixed
 * device or model; then per member, in lqrrt_tree_clear_connect's order: lqrrt_tree_clear's refusals, lqrrt_connect_search's, an
 * id list without its count, an id outside the tree, depths beyond 32 bits, the LDS of the search. */
int lqrrt_tree_clear_connect_multi(lqrrt_engine** engines, int n, const double* const* tracks_host, const double* const* radii_host,
                                   const int32_t* L, const int32_t* D, const int32_t* start, const int32_t* horizon_iters,
                                   const int32_t* goal_tries, const int32_t* const* nodes_host /* NULL, or per engine NULL = every node */,
                                   const int32_t* counts, lqrrt_clear_stats* out, lqrrt_clear_connect_stats* chain,
                                   int32_t* const* first_host, int32_t* const* dwell_host, void* stream);

/* Overwrites the ignore bits of nodes [first, first+count) (planner.py:270 `ignores`). */
int lqrrt_tree_set_ignored(lqrrt_engine* e, int first, int count, const uint8_t* flags_host);

/* Remember / restore the current tree size, ignore set and goal bookkeeping.  Nodes are only
 * ever appended, so rewinding is O(1); used by bench.py to keep the tree inside the size
 * window the metric is quoted at. (build-only; the reference rebuilds its tree per call) */
int lqrrt_tree_mark(lqrrt_engine* e);
int lqrrt_tree_rewind(lqrrt_engine* e);

/* Host copies of tree features (planner.tree.state / .pID / .lqr / .x_seq / .u_seq). */
int lqrrt_tree_get_states(lqrrt_engine* e, int first, int count, double* out_host /*[count][n]*/);
int lqrrt_tree_get_gains(lqrrt_engine* e, int first, int count, double* out_host /*[count][m][n]*/);
int lqrrt_tree_get_parents(lqrrt_engine* e, int first, int count, int32_t* out_host);
int lqrrt_tree_get_edge_lengths(lqrrt_engine* e, int first, int count, int32_t* out_host);
/* edge of one node: x [len][n], u [len][m]; returns len (root: 1, tree.py:69-70) */
int lqrrt_tree_get_edge(lqrrt_engine* e, int id, double* x_host, double* u_host);
int lqrrt_tree_get_ignored(lqrrt_engine* e, int first, int count, uint8_t* out_host);
/* Tree.climb (tree.py:100-117) on the engine's host mirror of the parent array: node ids from the seed (first) down to `id` (last)
 * into out_ids [cap]; returns their number (LQRRT_E_CAPACITY when cap is too small).  No device access. */
int lqrrt_tree_climb(lqrrt_engine* e, int id, int32_t* out_ids, int cap);
/* Tree.trajectory's reads (tree.py:121-132) for a whole list of nodes at once: gathered on the device, two copies out.
 * x [count][H][n], u [count][H][m] (rows beyond a node's edge length unspecified), len [count]; any output may be NULL. */
int lqrrt_tree_get_edges_of(lqrrt_engine* e, const int32_t* ids_host, int count, double* x_host, double* u_host, int32_t* len_host);
/* edges of nodes [first, first+count) in one copy: x [count][H][n], u [count][H][m] (H = horizon_iters; rows beyond a
 * node's edge length are unspecified) */
int lqrrt_tree_get_edges(lqrrt_engine* e, int first, int count, double* x_host, double* u_host);

/* ---------------------------------------------------------------- operators ---------- */

/* Constraints.is_feasible over a batch (constraints.py:53-61, plugins e.g.
 * demo_boat_advanced.py:209-225).  x [B][n], u [B][m] (NULL = zeros) -> ok [B] (0/1). */
int lqrrt_feasible_batch(lqrrt_engine* e, const double* x_dev, const double* u_dev, int B,
                         uint8_t* ok_dev, void* stream);

/* dynamics(x,u,dt) over a batch (e.g. demo_boat_advanced.py:78-130). x [B][n], u [B][m]. */
int lqrrt_dynamics_batch(lqrrt_engine* e, const double* x_dev, const double* u_dev, int B,
                         double* xnext_dev, void* stream);

/* lqr(x,u)[1] over a batch (e.g. demo_boat_advanced.py:139-151): K [B][m][n]. */
int lqrrt_gain_batch(lqrrt_engine* e, const double* x_dev, const double* u_dev, int B,
                     double* K_dev, void* stream);

/* erf(xgoal,x) over a batch (e.g. demo_boat_advanced.py:153-164): e [B][n]. */
int lqrrt_erf_batch(lqrrt_engine* e, const double* xg_dev, const double* x_dev, int B,
                    double* e_dev, void* stream);

/* The general lqr(x,u) of the API contract (planner.py:39-42: "S solves the local Riccati equation",
 * K the feedback gain), which no demo of the reference implements: per item, A = df/dx and B = df/du
 * by central differences (step eps) of the compiled-in dynamics about (x,u), then the discrete
 * algebraic Riccati equation for weights Q (n x n), R (m x m) by structure-preserving doubling, and
 * K = (R + B'SB)^-1 B'SA.  One problem per wavefront.  Outputs S [B][n][n], K [B][m][n]; optional
 * A [B][n][n], B [B][n][m], iterations [B] (NULL to skip).  Golden: scipy.linalg.solve_discrete_are. */
int lqrrt_lqr_dare_batch(lqrrt_engine* e, const double* x_dev, const double* u_dev, int B,
                         const double* Q_dev, const double* R_dev, double eps,
                         double* S_dev, double* K_dev, double* A_dev, double* B_dev, int32_t* iters_dev,
                         void* stream);

/* Planner._costs_to_go + nearest selection (planner.py:239-247, 340-350) for W samples
 * against the current tree: id[W] = lowest-cost non-ignored node (lowest id on ties; the
 * overall best when every node is ignored), cost[W] its cost.  S_dev: NULL = the system's
 * own S; else a dense n x n matrix used for every sample (planner.py:313-318 guide search).
 * use_ignore = 0 reproduces pruning=False (np.argmin, planner.py:247). */
int lqrrt_nn_argmin(lqrrt_engine* e, const double* xs_dev /*[W][n]*/, int W, const double* S_dev,
                    int use_ignore, int32_t* id_dev, double* cost_dev, void* stream);

/* The same for ONE query given and answered in host memory (x [n]; S [n][n] or NULL = the system's own S, identity for
 * LQRRT_MODEL_GENERIC) -- the form a host loop that steers with Python callables between two queries needs: synchronous, the
 * query travels as kernel arguments and the answer returns through mapped pinned memory (LQRRT_MODEL_GENERIC: two launches and
 * one wait, no copy).  cost_out may be NULL. */
int lqrrt_nn_argmin_host(lqrrt_engine* e, const double* x_host /*[n]*/, const double* S_host, int use_ignore,
                         int32_t* id_out, double* cost_out, void* stream);

/* LQRRT_MODEL_GENERIC only: the selection for a query whose error rows erf(x, node i) the caller evaluated itself
 * (errors_host [tree_size][n] row-major; planner.py:588's erf_v for an erf that is not of the subtract-and-wrap form):
 * contraction with S (NULL = identity), ignore set and tie rule as above.  One host-to-device copy of the rows per call. */
int lqrrt_nn_argmin_errors(lqrrt_engine* e, const double* errors_host, const double* S_host, int use_ignore,
                           int32_t* id_out, double* cost_out, void* stream);

/* Full cost vector of one sample against the tree (planner.py:340-350), cost [tree_size]. */
int lqrrt_costs_to_go(lqrrt_engine* e, const double* x_dev /*[n]*/, const double* S_dev,
                      double* cost_dev, void* stream);

/* Planner._steer(ID, xtar, force_arrive=False) for W problems (planner.py:354-438), one per
 * wavefront.  Outputs: len[W] recorded steps, xseq [W][H][n], useq [W][H][m] (first len rows
 * valid), xend [W][n] (= xseq[len-1]), Kend [W][m][n] = lqr(xend, ulast)[1]. Any output may
 * be NULL. */
int lqrrt_steer_batch(lqrrt_engine* e, const int32_t* parent_dev, const double* xtar_dev, int W,
                      int32_t* len_dev, double* xseq_dev, double* useq_dev, double* xend_dev,
                      double* Kend_dev, void* stream);

/* Planner._steer(ID, xtar, force_arrive=True) (planner.py:354-410, used by finish_on_goal :294-303):
 * one rollout from tree node `parent` until np.allclose(x, xtar, rtol, atol) (that step is not
 * recorded), an infeasible step (FPR truncation) or max_steps -- a deterministic stand-in for the
 * reference's wall-clock timeout (:402-406).  len_dev[0] = recorded steps; xseq [max_steps][n],
 * useq [max_steps][m]. */
int lqrrt_steer_force(lqrrt_engine* e, int parent, const double* xtar_dev, int max_steps, double rtol, double atol,
                      int32_t* len_dev, double* xseq_dev, double* useq_dev, void* stream);

/* Plan refinement (Planner.refine_plan; not in the reference).  plan_host [P] is a found plan, node ids from the root (0)
 * down a parent chain.  Candidate (i, j), 0 <= i < j < P, starts at node plan[i] (state and gain) at cost
 * sum_{k<=i} L_k (L_0 = 1, else the node's edge length) and steers (planner.py:354-438 with a fixed horizon of
 * horizon_iters steps, no adaptive heuristic) toward plan[j] .. plan[P-2], then toward the goal up to goal_tries times;
 * an empty edge adds nothing, a non-empty one moves the chain to its end state with lqr(x_end, u_last)[1].  The chain
 * ends after the first edge ending strictly inside the goal box; if the targets run out first it is invalid.
 *
 * lqrrt_refine_search: the valid candidate of smallest (cost, i, j) with cost < incumbent -> *cost, *i_out, *j_out;
 * none: *cost = incumbent, *i_out = *j_out = -1.  One launch, one wavefront per candidate; synchronous.  Plans of at most
 * 11586 nodes (the launch's 2^32 threads; LQRRT_E_ARG above). */
int lqrrt_refine_search(lqrrt_engine* e, const int32_t* plan_host, int P, int goal_tries, int horizon_iters,
                        int64_t incumbent, int64_t* cost, int32_t* i_out, int32_t* j_out, void* stream);

/* lqrrt_refine_commit: replays candidate (i, j) and appends its non-empty edges to the tree as a parent chain below
 * plan[i] (state, gain, parent, edge, angle-error table; the host mirrors and the ignore set stay valid, the new nodes are
 * not ignored).  ids_out [cap_ids >= P-1-j+goal_tries] receives the new ids; returns their count.  LQRRT_E_CAPACITY when
 * the tree cannot hold the chain, LQRRT_E_STATE when the chain does not reach the goal: the tree is then unchanged.
 * Synchronous. */
int lqrrt_refine_commit(lqrrt_engine* e, const int32_t* plan_host, int P, int goal_tries, int horizon_iters, int i, int j,
                        int32_t* ids_out, int cap_ids, void* stream);

/* The two calls above for n engines at once (refine_plans): engine k refines plans[k] (plan_lens[k] node ids) with goal_tries[k]
 * and horizon_iters[k]; horizon, goal tries, goal box and edge-pool length may differ between the engines, which share the device
 * and the model (Riccati systems included); no engine appears twice, n <= 128.  EVERY argument of EVERY engine is checked with the
 * rules of the one-engine calls before anything is written or launched.  Up to 32 engines share a launch (more: consecutive
 * chunks on `stream`, also where one launch would exceed 2^32 threads), and the whole call waits for the stream once.  The few kB
 * of device scratch behind a call are, like those of the one-engine calls, not part of lqrrt_engine_footprint.  Synchronous.
 *
 * lqrrt_refine_search_multi: one search launch per chunk, every engine with a best key of its own -- per engine the result of
 * lqrrt_refine_search(incumbents[k]) in cost_out[k], i_out[k], j_out[k] (none: incumbents[k], -1, -1). */
int lqrrt_refine_search_multi(lqrrt_engine** engines, int n, const int32_t* const* plans, const int32_t* plan_lens,
                              const int32_t* goal_tries, const int32_t* horizon_iters, const int64_t* incumbents,
                              int64_t* cost_out, int32_t* i_out, int32_t* j_out, void* stream);

/* lqrrt_refine_commit_multi: one commit launch per chunk, one workgroup per engine with a candidate; i[k] = j[k] = -1 leaves
 * engine k out (counts_out[k] = 0).  ids_out[k] [cap_ids[k] >= plan_lens[k]-1-j[k]+goal_tries[k]] receives engine k's new ids and
 * counts_out[k] their number; counts_out[k] = LQRRT_E_CAPACITY when that tree cannot hold the chain, LQRRT_E_STATE when the chain
 * does not reach the goal: that engine's tree and host mirrors are then unchanged, the others commit, and the call returns 0. */
int lqrrt_refine_commit_multi(lqrrt_engine** engines, int n, const int32_t* const* plans, const int32_t* plan_lens,
                              const int32_t* goal_tries, const int32_t* horizon_iters, const int32_t* i, const int32_t* j,
                              int32_t* const* ids_out, const int32_t* cap_ids, int32_t* counts_out, void* stream);

/* Tree-wide goal connection (Planner.connect_goal; not in the reference): from which node of the WHOLE tree does a short chain of
 * goal-directed steers reach the goal, and which gives the shortest plan?  For a tree of N nodes with pID[v] < v, depth[0] = 1 and
 * depth[v] = depth[pID[v]] + L_v (L_v the node's edge length).  A candidate is a node v -- every node (nodes_host = NULL; count is
 * then ignored) or those of nodes_host [count], in any order -- and starts at v's state and gain at cost depth[v].  Its targets are
 * the goal, up to goal_tries times, one edge each: planner.py:354-438 with a fixed horizon of horizon_iters steps, the FPR cut, no
 * adaptive heuristic; an empty edge adds nothing, a non-empty one moves the chain to its end state with lqr(x_end, u_last)[1].
 * The chain is valid when an edge ends strictly inside the goal box, and ends there; when the tries run out first it is invalid.  A
 * candidate that itself lies in the goal box needs a non-empty edge like any other.
 *
 * lqrrt_connect_search: the valid candidate of smallest (cost, node id) with cost < incumbent -> *cost, *node_out; none:
 * *cost = incumbent, *node_out = -1.  incumbent in [1, 2^31-1]; 2^31-1: no plan to beat.  One launch, one wavefront per candidate,
 * with a global early stop that cannot change the winner; synchronous.  The depth table is computed on the host from the engine's
 * mirrors and uploaded with the call; it lives in device scratch that grows on demand (4 B per node plus the id list) and is, like
 * that of lqrrt_refine_search, not part of lqrrt_engine_footprint. */
int lqrrt_connect_search(lqrrt_engine* e, const int32_t* nodes_host, int count, int goal_tries, int horizon_iters,
                         int64_t incumbent, int64_t* cost, int32_t* node_out, void* stream);

/* lqrrt_connect_commit: replays the chain of candidate `node` and appends its non-empty edges to the tree as a parent chain below
 * it (as lqrrt_refine_commit: state, gain, parent, edge, angle-error table; host mirrors and ignore set stay valid, the new nodes
 * are not ignored).  ids_out [cap_ids >= goal_tries] receives the new ids; returns their count.  LQRRT_E_CAPACITY when the tree
 * cannot hold the chain, LQRRT_E_STATE when the chain does not reach the goal: the tree is then unchanged.  The loop-time goal
 * bookkeeping (lqrrt_plan_best) is not rewritten; a later lqrrt_tree_retain rebuilds it and sees the chain's last node as a hit.
 * Synchronous. */
int lqrrt_connect_commit(lqrrt_engine* e, int node, int goal_tries, int horizon_iters, int32_t* ids_out, int cap_ids,
                         void* stream);

/* One tree asked about many goals (Planner.goal_costs / Planner.retarget; not in the reference): lqrrt_connect_search's question for
 * T targets in one launch.  A tree rooted at the vehicle is a single-source reachability structure; which goal it was grown for
 * matters to the goal bias of its samples only.  Target t is a goal state goals[t][n] with the box lo[t][d] < x[d] < hi[t][d]
 * (host arrays [T][n] of doubles, n the model's state count).  The rule is lqrrt_connect_search's with the target's goal and box in
 * place of the engine's own, for every target independently: the winner of target t is the valid candidate of smallest (cost, node
 * id) with cost < incumbents[t] -> cost_out[t], node_out[t]; none (or count = 0): cost_out[t] = incumbents[t], node_out[t] = -1.
 * incumbents = NULL: 2^31-1 for every target.  The engine's own goal and box are neither read nor written.
 *
 * Every argument is checked before anything is written or launched, with the rules of lqrrt_connect_search (candidates, id list,
 * goal_tries, horizon_iters, every incumbent in [1, 2^31-1]) and LQRRT_E_ARG also for T outside [1, 1024], T count workgroups of 64
 * threads beyond one launch (2^32 - 1 threads), a goal that is not finite, and lo > hi in any dimension.  One launch of T count
 * workgroups, target-major, every target with a best key of its own; synchronous.  The keys, the target table, the depth table and
 * the id list go up in one copy into the scratch of lqrrt_connect_search (8 + 288 bytes per target more), which is not part of
 * lqrrt_engine_footprint; the T keys come back in one copy. */
int lqrrt_reach_search(lqrrt_engine* e, const double* goals, const double* lo, const double* hi, int T,
                       const int32_t* nodes_host, int count, int goal_tries, int horizon_iters, const int64_t* incumbents,
                       int64_t* cost_out, int32_t* node_out, void* stream);

/* lqrrt_reach_commit: lqrrt_connect_commit for one target (goal[n], lo[n], hi[n]) -- replays the chain of candidate `node` toward
 * that goal and appends its non-empty edges to the tree as a parent chain below it.  ids_out [cap_ids >= goal_tries] receives the
 * new ids; returns their count.  LQRRT_E_CAPACITY when the tree cannot hold the chain, LQRRT_E_STATE when the chain does not end
 * in the target's box: the tree is then unchanged.  The engine's own goal and box are not touched, and the loop-time goal
 * bookkeeping (lqrrt_plan_best) is not rewritten.  Synchronous. */
int lqrrt_reach_commit(lqrrt_engine* e, const double* goal, const double* lo, const double* hi, int node, int goal_tries,
                       int horizon_iters, int32_t* ids_out, int cap_ids, void* stream);

/* Tree-wide goal chains through waypoints (Planner.connect_via; not in the reference): lqrrt_connect_search's question with a
 * caller's list of states between the tree and the goal -- the rest of an older plan that the tree no longer holds, the path of a
 * coarser planner.  waypoints_host [Q][n] doubles, Q >= 0 (NULL allowed when Q = 0); a waypoint need be neither a tree node nor a
 * feasible state.  A candidate is a pair (v, j), 0 <= j <= Q: v every node (nodes_host = NULL; count is then ignored) or one of
 * nodes_host [count], STRICTLY ASCENDING.  It starts at v's state and gain at cost depth[v]; its targets are w_j .. w_{Q-1} in order
 * and then the goal up to goal_tries >= 1 times, one edge per target as in lqrrt_refine_search.  An empty edge adds nothing and the
 * chain goes on to its next target.  After every non-empty edge, a waypoint's included, the chain ends valid if its end lies
 * strictly inside the goal box; when the targets run out first it is invalid.  j = Q is lqrrt_connect_search's candidate, and with
 * Q = 0 the two calls give the same result bit for bit.  A chain does not steer round an obstacle that blocks it: an infeasible
 * rollout is cut (FPR) and the chain goes on from where the cut left it.
 *
 * lqrrt_connect_via_search: the valid candidate of smallest (cost, node id, j) with cost < incumbent -> *cost, *node_out, *j_out;
 * none: *cost = incumbent, *node_out = *j_out = -1.  Every argument is checked before anything is written or launched;
 * LQRRT_E_ARG also for an id list that is not strictly ascending, a waypoint that is not finite, count (Q + 1) candidates of 64
 * threads beyond one launch (2^32 - 1 threads), and a deepest candidate whose depth plus (Q + goal_tries) horizon_iters leaves
 * 32-bit step counts.  One launch, one wavefront per candidate, with lqrrt_connect_search's early stop; synchronous.  The depth
 * table, the id list, the waypoints and the key go up in one copy into the scratch of lqrrt_connect_search (8 Q n bytes more),
 * which is not part of lqrrt_engine_footprint. */
int lqrrt_connect_via_search(lqrrt_engine* e, const int32_t* nodes_host, int count, const double* waypoints_host, int Q,
                             int goal_tries, int horizon_iters, int64_t incumbent, int64_t* cost, int32_t* node_out,
                             int32_t* j_out, void* stream);

/* lqrrt_connect_via_commit: replays the chain of candidate (node, j) over the same waypoints and appends its non-empty edges to the
 * tree as a parent chain below `node`, exactly as lqrrt_connect_commit does.  ids_out [cap_ids >= Q - j + goal_tries] receives the
 * new ids; returns their count.  LQRRT_E_CAPACITY when the tree cannot hold the chain, LQRRT_E_STATE when the chain does not reach
 * the goal: the tree is then unchanged.  Synchronous. */
int lqrrt_connect_via_commit(lqrrt_engine* e, int node, int j, const double* waypoints_host, int Q, int goal_tries,
                             int horizon_iters, int32_t* ids_out, int cap_ids, void* stream);

/* The two calls above for n engines at once (connect_goals), with the conventions of lqrrt_refine_*_multi: horizon, goal tries,
 * goal box and tree size may differ between the engines, which share the device and the model (Riccati systems included); no
 * engine appears twice, n <= 128.  EVERY argument of EVERY engine is checked with the rules of the one-engine calls before
 * anything is written or launched.  Up to 32 engines share a launch (more: consecutive chunks on `stream`, also where one launch
 * would exceed 2^32 threads), and the whole call waits for the stream once.  The device scratch behind a call (4 B per node of
 * every tree of a chunk plus the id lists, held by the chunk's first engine) is not part of lqrrt_engine_footprint.  Synchronous.
 *
 * lqrrt_connect_search_multi: one search launch per chunk, every engine with a best key of its own (the early stop prunes within
 * one tree only) -- per engine the result of lqrrt_connect_search(incumbents[k]) in cost_out[k], node_out[k] (none:
 * incumbents[k], -1).  nodes = NULL: every node of every tree; else nodes[k] = NULL: every node of tree k, or its id list
 * [counts[k]].  An engine with an empty id list takes part in no launch and has no winner. */
int lqrrt_connect_search_multi(lqrrt_engine** engines, int n, const int32_t* const* nodes, const int32_t* counts,
                               const int32_t* goal_tries, const int32_t* horizon_iters, const int64_t* incumbents,
                               int64_t* cost_out, int32_t* node_out, void* stream);

/* lqrrt_connect_commit_multi: one commit launch per chunk, one workgroup per engine with a candidate; nodes[k] = -1 leaves engine k
 * out (counts_out[k] = 0).  ids_out[k] [cap_ids[k] >= goal_tries[k]] receives engine k's new ids and counts_out[k] their number;
 * counts_out[k] = LQRRT_E_CAPACITY when that tree cannot hold the chain, LQRRT_E_STATE when the chain does not reach the goal:
 * that engine's tree and host mirrors are then unchanged, the others commit, and the call returns 0. */
int lqrrt_connect_commit_multi(lqrrt_engine** engines, int n, const int32_t* nodes, const int32_t* goal_tries,
                               const int32_t* horizon_iters, int32_t* const* ids_out, const int32_t* cap_ids, int32_t* counts_out,
                               void* stream);

/* lqrrt_connect_via_search / lqrrt_connect_via_commit for n engines at once (connect_vias), with the conventions of the two calls
 * above: the engines share the device and the model, no engine appears twice, n <= 128; up to 32 engines share a launch (more:
 * consecutive chunks on `stream`, also where one launch would exceed 2^32 threads) and the call waits for the stream once.  Every
 * engine has its OWN waypoint table waypoints[k] [Q[k]][n] (Q[k] >= 0; waypoints or waypoints[k] may be NULL where Q[k] = 0), id
 * list, goal tries, horizon, incumbent and best key: the early stop prunes within one tree only.  EVERY argument of EVERY engine is
 * checked with the rules of the one-engine calls before anything is written or launched: LQRRT_E_ARG for a null entry, an engine
 * twice, mixed devices or models, more than 128 engines, Q[k] < 0 or Q[k] > 0 without a table, a waypoint that is not finite, an id
 * list that is not strictly ascending, an incumbent out of range, counts[k] (Q[k] + 1) candidates of 64 threads beyond one launch,
 * and a deepest candidate whose depth plus (Q[k] + goal_tries[k]) horizon_iters[k] leaves 32-bit step counts; LQRRT_E_STATE for an
 * LQRRT_MODEL_GENERIC engine.  The device scratch behind a call (per chunk the keys, a descriptor per engine and every engine's
 * waypoints, depth table and id list, held by the chunk's first engine) is that of lqrrt_refine_*_multi and is not part of
 * lqrrt_engine_footprint.  Synchronous.
 *
 * lqrrt_connect_via_search_multi: one search launch per chunk -- per engine the result of lqrrt_connect_via_search in cost_out[k],
 * node_out[k], j_out[k] (none: incumbents[k], -1, -1).  nodes = NULL: every node of every tree; else nodes[k] = NULL: every node
 * of tree k, or its strictly ascending id list [counts[k]].  An engine with an empty id list takes part in no launch and has no
 * winner. */
int lqrrt_connect_via_search_multi(lqrrt_engine** engines, int n, const int32_t* const* nodes, const int32_t* counts,
                                   const double* const* waypoints, const int32_t* Q, const int32_t* goal_tries,
                                   const int32_t* horizon_iters, const int64_t* incumbents, int64_t* cost_out, int32_t* node_out,
                                   int32_t* j_out, void* stream);

/* lqrrt_connect_via_commit_multi: one commit launch per chunk, one workgroup per engine with a candidate (nodes[k], j[k]) over its
 * own waypoints; nodes[k] = -1 leaves engine k out (counts_out[k] = 0).  ids_out[k] [cap_ids[k] >= Q[k] - j[k] + goal_tries[k]]
 * receives engine k's new ids and counts_out[k] their number; counts_out[k] = LQRRT_E_CAPACITY when that tree cannot hold the
 * chain, LQRRT_E_STATE when the chain does not reach the goal: that engine's tree and host mirrors are then unchanged, the others
 * commit, and the call returns 0.  The edge lengths of every chain come back with the outputs in one copy per chunk. */
int lqrrt_connect_via_commit_multi(lqrrt_engine** engines, int n, const int32_t* nodes /* -1: no winner */, const int32_t* j,
                                   const double* const* waypoints, const int32_t* Q, const int32_t* goal_tries,
                                   const int32_t* horizon_iters, int32_t* const* ids_out, const int32_t* cap_ids,
                                   int32_t* counts_out, void* stream);

/* lqrrt_reach_search / lqrrt_reach_commit for n engines at once (fleet_goal_costs / retargets: the task-assignment matrix of a fleet,
 * P trees x T targets), with the conventions of lqrrt_connect_search_multi: 1 <= n <= 128 distinct engines of one device and one
 * compiled-in model, cut into chunks of up to 32 engines that take part and fewer than 2^32 threads per launch; per chunk one image
 * in a scratch of its first engine (not part of lqrrt_engine_footprint), one copy up, one launch, one copy back; one synchronise
 * per call.  Every argument of every engine and target is checked, with the rules of the one-engine calls (messages name the
 * engine), before anything is written or launched.
 *
 * lqrrt_reach_search_multi: engine k is asked about its own T[k] targets (1 to 1024) -- goals[k], lo[k], hi[k]: host arrays
 * [T[k]][n_states] as lqrrt_reach_search takes them; nodes / counts: lqrrt_connect_search_multi's id lists (nodes NULL or nodes[k]
 * NULL: every node of tree k; counts[k] = 0: no launch share, no winner); goal_tries and horizon_iters [n]; incumbents NULL, or n
 * pointers each NULL (2^31-1 for every target) or [T[k]].  cost_out[k] and node_out[k] point to [T[k]]: per target the result of
 * lqrrt_reach_search.  Engine k occupies T[k] * count_k workgroups of its chunk's launch, target-major; every (engine, target) pair
 * has a best key of its own, so each winner is the one the engine's own lqrrt_reach_search finds. */
int lqrrt_reach_search_multi(lqrrt_engine** engines, int n, const double* const* goals, const double* const* lo,
                             const double* const* hi, const int32_t* T, const int32_t* const* nodes, const int32_t* counts,
                             const int32_t* goal_tries, const int32_t* horizon_iters, const int64_t* const* incumbents,
                             int64_t* const* cost_out, int32_t* const* node_out, void* stream);

/* lqrrt_reach_commit_multi: one commit launch per chunk, one workgroup per engine with a winner nodes[k] toward its ONE target
 * goal[k], lo[k], hi[k] ([n_states] each); ids_out[k] [cap_ids[k] >= goal_tries[k]] receives the new ids and counts_out[k] their
 * number -- 0 for nodes[k] = -1 (that engine's other arguments but goal_tries and horizon_iters are not read),
 * LQRRT_E_CAPACITY when that tree cannot hold the chain, LQRRT_E_STATE when the chain does not end in the target's box: that
 * engine's tree and host mirrors are then unchanged, the others commit, and the call returns 0.  The engines' own goals and boxes
 * are neither read nor written. */
int lqrrt_reach_commit_multi(lqrrt_engine** engines, int n, const double* const* goal, const double* const* lo,
                             const double* const* hi, const int32_t* nodes /* -1: no winner */, const int32_t* goal_tries,
                             const int32_t* horizon_iters, int32_t* const* ids_out, const int32_t* cap_ids, int32_t* counts_out,
                             void* stream);

/* ---------------------------------------------------------------- wave engine -------- */

/* Explicit sample stream: the caller supplies the samples (a user xrand_gen function,
 * planner.py:213-216) instead of the default sampler; xs_host [count][n] are queued after what is
 * already queued.  lqrrt_engine_set_sampler switches back to the default sampler. */
int lqrrt_engine_push_samples(lqrrt_engine* e, const double* xs_host, int count);
int lqrrt_engine_queued_samples(lqrrt_engine* e);


/* Doubles per wave record and field offsets (for the RCCL all-gather of records):
 * layout[0]=record doubles, [1]=off_cost, [2]=off_parent, [3]=off_len, [4]=off_flags,
 * [5]=off_xend, [6]=off_trig, [7]=off_K, [8]=off_xseq, [9]=off_useq, [10]=off_xrand. */
int lqrrt_record_layout(lqrrt_engine* e, int32_t* layout11);

/* Device address of the engine's wave record buffer [max_wave][record doubles]. */
int lqrrt_wave_records(lqrrt_engine* e, void** dev_ptr);

/* Wave size the engine would pick now (<= wave_cap): ~N/6 while the tree is small, then steered by
 * feedback from the last commits (waves cut short by goal hits, repair rounds).  Any W gives the
 * same tree; this only tunes speed.  All ranks of a sharded run get the same answer. */
int lqrrt_wave_suggest(lqrrt_engine* e, int wave_cap);

/* Phase A of a wave (shardable): prepares samples [k0, k0+W) of the sample stream if needed,
 * then runs the speculative nearest-neighbour + steer for the slice [lo,hi) of the wave
 * against the current tree and writes records lo..hi-1.  Other ranks fill the rest
 * (all-gather of the record buffer), then every rank calls lqrrt_wave_commit. */
int lqrrt_wave_speculate(lqrrt_engine* e, int W, int lo, int hi, void* stream);

/* Tree-sharded wave (the alternative of SURVEY 8e for large trees, e.g. BASELINE config 5): every rank holds the whole
 * tree but scans only nodes [node_lo, node_hi) -- node_lo a multiple of 64 -- for ALL W samples of the wave, and reduces
 * them to one candidate per sample: best_dev [W][2] doubles = (cost, node id as a double; id -1 = nothing eligible in
 * the range).  The candidates of all ranks are all-gathered (16*W bytes per rank: the path's one collective) in
 * ascending node-range order into [parts][W][2] and handed to lqrrt_wave_steer_candidates, which picks each sample's
 * nearest node by (cost, id) -- exactly the node a single scan returns, incl. the every-node-ignored fallback of
 * planner.py:241,245 -- and runs the speculative steer of the whole wave on every rank.  No record exchange:
 * lqrrt_wave_commit follows directly and the replicas stay bit-identical. */
int lqrrt_wave_scan_nodes(lqrrt_engine* e, int W, int node_lo, int node_hi, double* best_dev, void* stream);
int lqrrt_wave_steer_candidates(lqrrt_engine* e, int W, int parts, const double* best_dev, void* stream);

/* Phase B (replicated): exact-mode validation/repair of the W records in sample order,
 * then append.  max_commit caps the attempts committed from this wave; node_limit is the
 * reference's max_nodes (stop once size > max_nodes, planner.py:311).  Advances the sample
 * cursor by the number of committed attempts.  Returns stats for this wave. */
int lqrrt_wave_commit(lqrrt_engine* e, int W, int64_t max_commit, int64_t node_limit,
                      int pruning, lqrrt_extend_stats* out, void* stream);

/* The planner loop body planner.py:233-290 run natively for many waves on one GPU:
 * grows the tree until max_attempts more attempts were committed, or size > node_limit, or
 * size >= until_size (0 = off), or (stop_on_goal) a goal hit was committed. wave = W cap. */
int lqrrt_engine_extend(lqrrt_engine* e, int wave, int64_t max_attempts, int64_t node_limit,
                        int until_size, int pruning, int stop_on_goal,
                        lqrrt_extend_stats* out, void* stream);

/* ---- sharded waves over the GPUs of one node, natively (one process per GPU) ----
 * The reference is single-threaded (planner.py:233-290); this is the build's own multi-GPU form of that loop.  Every rank
 * holds the whole tree and the same sample stream, every wave has ONE collective (RCCL all-gather on `stream`), and the
 * commit is replicated, so the replicas stay bit-identical and equal to the single-GPU tree.
 *
 * Communicator: librccl.so is resolved at run time (the copy already loaded in the process -- PyTorch's -- if any;
 * LQRRT_RCCL names another).  Rank 0 calls lqrrt_comm_unique_id and hands the 128 bytes to the other ranks by any means
 * (lqrrt_amd/parallel.py broadcasts them with torch.distributed); every rank then calls lqrrt_comm_create.
 * lqrrt_comm_create_loopback is a test double: one process plays `rank` of `world` and computes what the other ranks would
 * contribute itself, through the same blocks and unpack path, on one GPU. */
typedef struct lqrrt_comm lqrrt_comm;
#define LQRRT_COMM_RCCL      0
#define LQRRT_COMM_LOOPBACK  1
int lqrrt_comm_unique_id(uint8_t* id128);
int lqrrt_comm_create(const uint8_t* id128, int rank, int world, int device, lqrrt_comm** out);
int lqrrt_comm_create_loopback(int rank, int world, lqrrt_comm** out);
int lqrrt_comm_destroy(lqrrt_comm* c);

/* LQRRT_SHARD_SAMPLES (north_star's scheme): rank g speculates samples [g*ceil(W/G), ...) of the wave; what the others need
 * of its records -- {cost, parent, len, flags, xend, trig, K} per sample + the edges of the samples that added a node,
 * compacted -- is written into the rank's all-gather block by the speculative launch itself; blocks are gathered in place;
 * one kernel unpacks them into the local records and prepares the repair rounds.  A block's edge tail holds
 * LQRRT_SHARD_TAIL (default 0.4) of the worst case; a sample whose edge did not fit is re-steered by the receivers.
 * LQRRT_SHARD_TREE (SURVEY 8e's alternative for large trees): lqrrt_wave_scan_nodes over 1/G of the nodes, all-gather of
 * 16*W bytes per rank, lqrrt_wave_steer_candidates. */
#define LQRRT_SHARD_SAMPLES  0
#define LQRRT_SHARD_TREE     1

/* SURVEY 8(b) `lqrrt_allgather_nodes`: one sample-sharded wave of W samples up to, not including, its commit (speculate
 * this rank's slice, exchange, unpack); lqrrt_wave_commit follows. */
int lqrrt_allgather_nodes(lqrrt_engine* e, lqrrt_comm* c, int W, void* stream);

/* lqrrt_engine_extend with sharded waves: same arguments and stopping rules, same tree on every rank. */
int lqrrt_engine_extend_sharded(lqrrt_engine* e, lqrrt_comm* c, int scheme, int wave, int64_t max_attempts,
                                int64_t node_limit, int until_size, int pruning, int stop_on_goal,
                                lqrrt_extend_stats* out, void* stream);

/* Measurement aid: lqrrt_engine_extend_multi rewinds this engine to its mark (lqrrt_tree_mark) whenever a wave would begin above
 * `size` nodes; 0 switches it off.  The benches quote the metric with the tree inside a size window. */
int lqrrt_tree_set_rewind_above(lqrrt_engine* e, int size);

/* Several INDEPENDENT engines (trees) advanced together, natively: the loop of lqrrt_engine_extend for each of the n engines, in
 * lock step, with two kernel launches per step whose grids span all of them (the scans of the engines that begin a wave; every
 * engine's steer launch -- speculative launch, fused repair round or append).  No counterpart in the reference, which plans one
 * tree per Planner on one core (planner.py:233-290); the ROS node keeps three Planners and uses one at a time (lqrrt_node.py).  Every
 * engine's result is exactly what lqrrt_engine_extend gives it alone (same stop rules per engine: max_attempts, node_limit,
 * until_size, stop_on_goal); only the wall clock is shared -- a single planner cannot fill the chip (its launches are dependent
 * and small), n planners can.  Calls with 4 or more engines are cut into groups, each advanced by a host thread and a stream of
 * its own.  out: n stats blocks (or NULL).  Restrictions: 1 <= n <= 128 distinct engines of one model, one
 * horizon and one device, exact wave mode, analytic-gain systems, waves of up to 256 samples.  After an error every engine of the
 * call must be reset (lqrrt_tree_reset) before it is used again. */
int lqrrt_engine_extend_multi(lqrrt_engine** engines, int n, int wave, int64_t max_attempts, int64_t node_limit, int until_size,
                              int pruning, int stop_on_goal, lqrrt_extend_stats* out, void* stream);

/* Goal bookkeeping (planner.py:260-283): number of goal hits so far and the node id of
 * the best (shortest, first on ties) plan end, its length in steps; -1 if none. */
int lqrrt_plan_best(lqrrt_engine* e, int32_t* end_node, int64_t* steps, int64_t* hits);

/* Total attempts / candidate rows consumed since the last tree reset. */
int lqrrt_engine_counters(lqrrt_engine* e, lqrrt_extend_stats* out);

/* Timing of the dominant kernel (NN scan) accumulated with HIP events on `stream` (attached to each
 * dispatch as its start/stop events) when enabled: total ms, launches, algorithmic bytes (sum of W*N*(8n+1)).
 * on = 0 off, 1 NN scan launches only, 2 NN scan and steer launches (enabling resets the sums);
 * add 16 * (k - 1) to time only every k-th NN scan launch (sums and launch counts then refer to those). */
int lqrrt_profile_enable(lqrrt_engine* e, int on);
int lqrrt_profile_read(lqrrt_engine* e, double* nn_ms, int64_t* nn_launches, double* nn_bytes,
                       double* steer_ms, int64_t* steer_launches);

/* Measurement aid (bench.py): effective shader clock = s_memtime ticks / s_memrealtime (100 MHz) over a
 * chain of dependent fp64 FMAs on one wavefront, and what a dependent / an independent fp64 FMA costs that wavefront. */
int lqrrt_clock_probe(int device, double* shader_mhz, double* ns_dependent_fma, double* ns_independent_fma, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LQRRT_HIP_H */
