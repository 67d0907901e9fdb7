"""
Planner -- drop-in for the reference's lqrrt.Planner (lqrrt/planner.py) whose extend path runs on an MI355X.

Same as the reference: constructor / update_plan / set_* / kill_update / unkill signatures, result attributes
(tree, node_seq, x_seq, u_seq, t_seq, T, plan_reached_goal, get_state, get_effort), which arguments raise
ValueError and with which message, and update_plan's return value.

Different: the loop body of planner.py:233-290 (sample, cost-to-go nearest neighbour, LQR-policy steer with a
feasibility sweep per step, tree append, goal test) is executed by the HIP engine (csrc/engine.hip) in WAVES of
up to `wave_size` samples.  In 'exact' mode, the default, a wave's outcome is the one the samples would have
produced one after another: all samples are first evaluated against the tree as of the start of the wave, then
each is re-checked against the nodes accepted earlier in the same wave and the few whose true parent was born
inside the wave are steered again, to the fix-point.  'synchronous' mode skips that validation (every sample of
a wave of exactly `wave_size` sees the wave-start tree): not the reference's tree any more but the one
oracle/lqrrt_oracle.c's orc_extend_sync defines, several times faster.

Two kinds of plugins are accepted:
  * the handles of ONE native system object (lqrrt_amd.systems: the reference's demo problems, the ROS behaviours, an
    out-of-tree header): the whole loop body runs on the device as described above;
  * arbitrary Python callables with the reference's signatures (planner.py:35-59, constraints.py:27) -- "callback mode"
    (lqrrt_amd/callback.py): a GPU cannot call back into Python, so sampling, steering and feasibility run on the host in
    the reference's order of events, one iteration at a time, and the device keeps the node table and does
    Planner._costs_to_go + the nearest selection (95 % of the reference's time at 8k nodes).
There is no CPU path in either: without the HIP library and a device, update_plan raises.
"""
from __future__ import division

import os
import time

import numpy as np
import scipy.interpolate

from . import _native as nat
from .constraints import Constraints
from .engine import Engine
from . import callback
from .systems import native_system_of
from .tree import Tree, held_elsewhere


def _callable(f):
    return hasattr(f, '__call__')


class Planner:
    """
    dynamics, lqr, erf: handles of an lqrrt_amd.systems object, called like the reference's plugins
        (xnext = dynamics(x, u, dt);  (S, K) = lqr(x, u);  e = erf(xgoal, x)).
    constraints: a Constraints instance (feasibility handle of the same system, goal buffer).
    horizon: seconds simulated per tree extension, or (min, max) for the adaptive heuristic.
    dt: simulation step [s].   FPR: failed-path retention factor (planner.py:394-395).
    error_tol: state error (scalar or per state) below which a steer counts as converged.
    min_time, max_time, max_nodes, goal0, sys_time, printing: as in the reference (planner.py:61-82).
    wave_size, wave_mode, device: new and optional -- samples per wave (upper bound), 'exact' | 'synchronous',
        HIP device ordinal.
    angle_dims: new and optional, callback mode only -- the states `erf` wraps to (-pi, pi]; checked against a probe of erf
        (ValueError when they disagree).  None: the probe alone decides (lqrrt_amd/callback.py classify_erf).
    """

    plan_wait = 0                          # rows of dt the current plan stands on its first row before it leaves (avoid(max_wait))

    def __init__(self, dynamics, lqr, constraints,
                 horizon, dt=0.05, FPR=0,
                 error_tol=0.05, erf=np.subtract,
                 min_time=0.5, max_time=1, max_nodes=1E5,
                 goal0=None, sys_time=time.time, printing=True,
                 wave_size=1024, device=0, wave_mode='exact', angle_dims=None):
        if wave_mode not in ('exact', 'synchronous'):
            raise ValueError("wave_mode must be 'exact' or 'synchronous'")
        self.device, self.wave_size, self.wave_mode = device, int(wave_size), wave_mode
        self._engine = self._engine_key = None
        self._callback_run = None
        self.angle_dims = angle_dims
        self.tree = None
        self.set_system(dynamics, lqr, constraints, erf)
        self.set_resolution(horizon, dt, FPR, error_tol)
        self.set_runtime(min_time, max_time, max_nodes, sys_time)
        self.set_goal(goal0)
        self.printing = printing
        self.killed = False
        self.stats = None
        # A user sampling function (xrand_gen = a callable, planner.py:213-216) is called once per iteration on the tree the previous
        # iteration left, like the reference calls it (planner.py:236): one sample per native call.  False: a function that never looks at
        # planner.tree / plan_reached_goal may be called a batch AHEAD of the waves that consume its samples (same samples, same tree, no
        # host turn per iteration).
        self.xrand_gen_sees_tree = True
        # HBM pools are sized by max_nodes (Engine.footprint(): ~1.7 kB per node for the boats with horizon_iters = 20, i.e. ~170 MB at
        # the reference's default of 1e5 nodes).  A planner built with an explicit max_nodes gets them now, outside any plan's time
        # budget; one left at the default gets them with its first update_plan -- or when the caller asks (warm_up()) -- so that a fleet
        # of planners built with defaults does not pin gigabytes before anyone plans.
        if max_nodes != 1E5:
            self.warm_up()
        else:
            self.warm_up_error = None if nat.available() else RuntimeError("lqrrt_amd: no engine created: %s" % (
                "liblqrrt_hip.so is not built" if not os.path.exists(nat.LIB_PATH) else "no HIP device visible"))

    # ------------------------------------------------------------------------------------------ engine
    def warm_up(self):
        """Creates the device engine (HBM pools sized by max_nodes, geometry upload) ahead of the first update_plan,
        so that none of it is charged to a plan's time budget.  Where there is no GPU or no built library nothing is created --
        constructing and configuring a Planner works anywhere, planning does not -- and the reason is kept in
        `self.warm_up_error` (None when the engine exists), so that a broken install can be diagnosed before the first plan;
        update_plan raises it in full."""
        self.warm_up_error = None
        if self.callback_mode:
            if not nat.available():
                self.warm_up_error = RuntimeError("lqrrt_amd: no engine created: %s" % (
                    "liblqrrt_hip.so is not built" if not os.path.exists(nat.LIB_PATH) else "no HIP device visible"))
            return
        try:
            if nat.available():
                self._get_engine()
            else:
                self.warm_up_error = RuntimeError("lqrrt_amd: no engine created: %s" % (
                    "liblqrrt_hip.so is not built" if not os.path.exists(nat.LIB_PATH) else "no HIP device visible"))
        except (nat.NativeError, RuntimeError, OSError) as ex:
            self._engine = self._engine_key = None
            self.warm_up_error = ex

    def _retire_tree(self):
        """The engine is about to be reused: the previous plan's Tree keeps its contents (copied out of HBM once -- tens of milliseconds
        for a 100k-node tree) IF anybody still holds it (the ROS node does, lqrrt_node.py:477); a tree that only this planner refers to
        is simply dropped, like the reference drops its Tree at planner.py:172."""
        t = self.tree
        if t is None or not getattr(t, "on_device", False):
            return
        del t
        if held_elsewhere(self, "tree"):
            self.tree._detach()
        else:
            self.tree._e, self.tree._generation = None, None        # nobody can read it again
            self.tree = None

    def _get_engine(self):
        """The native engine for the current system / capacity / device (recreated when one of them changed)."""
        capacity = int(self.max_nodes) + self.wave_size + 8
        key = (id(self.system), capacity, self.wave_size, self.device)
        if self._engine is None or self._engine_key != key:
            self._retire_tree()
            if self._engine is not None:
                self._engine.close()
            self._engine = Engine(self.system, capacity=capacity, max_wave=self.wave_size, device=self.device)
            self._engine_key = key
        self._engine.sync_geometry()        # the world may have changed since the last plan (new map, new obstacles)
        self._engine.set_wave_mode(self.wave_mode)
        return self._engine

    # ------------------------------------------------------------------------------------------ planning
    def update_plan(self, x0, sample_space, goal_bias=0,
                    guide=None, xrand_gen=None, pruning=True,
                    finish_on_goal=False, specific_time=None):
        """
        Grows a new tree from the seed x0 toward the goal and extracts a plan from it (planner.py:104-336);
        arguments as in the reference.  xrand_gen: None, an integer >= 1 (tries allowed per feasible random sample)
        or a function of the planner returning a sample.

        Returns True if it ran to completion, False if it was halted (killed, tree larger than max_nodes, no goal).
        """
        # the feasibility function may have been swapped on the Constraints object itself since set_system (the ROS node does:
        # lqrrt_node.py:65 planner.constraints.set_feasibility_function(...)): the mode follows the plugins as they are NOW
        self._resolve_mode()
        if self.callback_mode:
            return self._update_plan_callback(x0, sample_space, goal_bias, guide, xrand_gen, pruning, finish_on_goal, specific_time)
        run = self._plan_begin(x0, sample_space, goal_bias, guide, xrand_gen, pruning, finish_on_goal, specific_time)
        if run is None:
            return False
        return self._plan_loop(run)

    def _plan_loop(self, run):
        """The native calls of one plan (update_plan, replan) and its wrap-up."""
        # Each native call grows the tree by a few waves.  The clock and the kill flag are looked at between calls, so a
        # call is sized to what the time budget still allows.
        while True:
            budget = self._plan_budget(run)
            # The call only has to come back AT a goal hit when that hit can end the plan (min_time already elapsed,
            # planner.py:293); before that, hits are bookkept by the engine (lqrrt_plan_best) and reported with the call.
            t_call = time.perf_counter()
            st = run.eng.extend(self.wave_size, max_attempts=budget, node_limit=int(self.max_nodes),
                                pruning=run.pruning, stop_on_goal=bool(run.time_elapsed >= run.min_time))
            if self._plan_after_call(run, st, time.perf_counter() - t_call):
                break
        return self._plan_end(run)

    def _update_plan_callback(self, x0, sample_space, goal_bias, guide, xrand_gen, pruning, finish_on_goal, specific_time, resume=None):
        """update_plan for plugins that are host callables: the reference's loop on the host, the nearest-neighbour stage on the
        device (lqrrt_amd/callback.py)."""
        if self.goal is not None:
            callback.require_device()
        if self._erf_angles is False:                               # erf is classified once per erf, at its first use
            self._erf_angles = callback.classify_erf(self.erf, self.nstates, self.angle_dims)
        if self._callback_run is None:
            self._callback_run = callback.CallbackRun(self)
        self._retire_tree()                                         # a tree grown by the native engine before the plugins were swapped
        return self._callback_run.run(x0, sample_space, goal_bias, guide, xrand_gen, pruning, finish_on_goal, specific_time, resume=resume)

    # The three phases of update_plan, separately callable so that several planners can share native calls (update_plans below):
    # set-up (planner.py:157-231), what follows each native call (:260-311 as far as the host is concerned), wrap-up (:313-336).
    def _plan_begin(self, x0, sample_space, goal_bias, guide, xrand_gen, pruning, finish_on_goal, specific_time, seed=None, retain=None):
        """retain = (root, revalidate): the plan is seeded with node `root` of the tree this planner's engine holds (replan) --
        tree_retain instead of tree_reset; x0 is then the root's state.  Three steps, separately callable so that the planners of
        an update_plans group can share the middle one (one tree_retain_multi for all of them)."""
        run = self._plan_prepare(x0, sample_space, goal_bias, guide, xrand_gen, pruning, finish_on_goal, specific_time, seed)
        if run is None:
            return None
        if retain is None:
            run.eng.tree_reset(run.x0)                              # planner.py:172
            return self._plan_start(run, None)
        return self._plan_start(run, run.eng.tree_retain(retain[0], revalidate=retain[1])[0])

    def _plan_prepare(self, x0, sample_space, goal_bias, guide, xrand_gen, pruning, finish_on_goal, specific_time, seed=None):
        """First step of _plan_begin, this planner alone: arguments, the old Tree object retired, geometry synchronised, sample
        stream and resolution set.  The device tree is as the last plan left it."""
        x0 = np.array(x0, dtype=np.float64)
        if self.goal is None:
            print("No goal has been set yet!")
            self.get_state = lambda t: x0
            self.get_effort = lambda t: np.zeros(self.ncontrols)
            return None
        run = _PlanRun()
        run.min_time, run.max_time = (self.min_time, self.max_time) if specific_time is None else (specific_time, specific_time)
        run.pruning, run.finish_on_goal, run.xrand_gen = pruning, finish_on_goal, xrand_gen

        run.user_sampler = not (xrand_gen is None or type(xrand_gen) is int)
        if run.user_sampler:
            # planner.py:213-216.  The function is called once per sample, in order: by default once per native call of ONE attempt --
            # the reference's order of events exactly (planner.py:236: sample, extend, goal bookkeeping, next sample), so it may read
            # planner.tree / planner.plan_reached_goal.  `planner.xrand_gen_sees_tree = False` lets a function that does not look at
            # the tree be called a batch ahead of the wave that consumes the samples (it then sees the tree as of the batch start).
            if not _callable(xrand_gen):
                raise ValueError("Expected xrand_gen to be None, an integer >= 1,  or a function.")
        else:
            # description of the default sampler (planner.py:176-198)
            if goal_bias is None:
                bias = np.zeros(self.nstates)
            elif hasattr(goal_bias, '__contains__'):
                if len(goal_bias) != self.nstates:
                    raise ValueError("Expected goal_bias to be scalar or have same length as state.")
                bias = np.array(goal_bias, dtype=np.float64)
            else:
                bias = np.full(self.nstates, goal_bias, dtype=np.float64)
            tries_limit = xrand_gen if (xrand_gen is not None and xrand_gen > 0) else 10
            space = np.array(sample_space, dtype=np.float64)
            if space.shape != (self.nstates, 2):
                raise ValueError("Expected sample_space to be list of nstates tuples.")

        self.xguide = np.copy(self.goal) if guide is None else np.array(guide, dtype=np.float64)

        # the device tree is about to be overwritten: a Tree object from the previous plan keeps its contents
        self._retire_tree()
        eng = run.eng = self._get_engine()
        run.own_stream = seed is not None                           # (update_plans: a sample stream per planner, np.random untouched)
        if run.own_stream and not run.user_sampler:
            # (seeded before anything else: set_resolution rewinds the generator to the first uncommitted candidate of the plan before --
            #  a replay of every draw that plan consumed, milliseconds after a long one -- unless the stream has just been replaced;
            #  update_plan's own path ends with sync_numpy_global, which leaves nothing to replay)
            st = np.random.RandomState(seed).get_state()
            eng.set_mt19937(st[1], st[2])
        self._engine_resolution(eng)
        run.x0, run.seed = x0, seed
        if not run.user_sampler:
            run.sampler = (space, bias, tries_limit)
        return run

    def _engine_resolution(self, eng):
        """The planner's resolution, goal and goal box onto the engine.  An unchanged horizon keeps the engine's tree."""
        if self.hfactor:
            # adaptive horizon: rollouts may run hspan[1] steps (include/lqrrt_hip.h, lqrrt_resolution.adaptive)
            eng.set_resolution(self.dt, self.FPR, int(self.hspan[1]), self.error_tol, self.goal, self.constraints.goal_buffer,
                               adaptive=True, hspan_min=int(self.hspan[0]), horizon_iters_state=int(self.horizon_iters))
        else:
            eng.set_resolution(self.dt, self.FPR, self.horizon_iters, self.error_tol, self.goal, self.constraints.goal_buffer)

    def _plan_start(self, run, retained):
        """Last step of _plan_begin, after the engine's tree was reset (retained = None) or retained (its stats): sampler, the new
        Tree bound to the device tree, the run's clock; a kept plan counts as found from the start."""
        eng, x0, seed = run.eng, run.x0, run.seed
        self.retained = retained
        if retained is not None:
            x0 = eng.states(0, 1)[0]
        self._grown_with = self._tree_resolution()
        self._grown_goal = np.array(self.goal, dtype=np.float64)    # (the engine's goal box: what connect_goal steers at)
        if not run.user_sampler:
            space, bias, tries_limit = run.sampler
            eng.set_sampler(np.mean(space, axis=1), np.diff(space).flatten(), bias, tries_limit)
            if run.own_stream:
                st = np.random.RandomState(seed).get_state()
                eng.set_mt19937(st[1], st[2])
            else:
                eng.seed_from_numpy_global()
        S0 = self.system.Smatrix()
        self.tree = Tree(x0, (S0, np.zeros((self.ncontrols, self.nstates))))
        self.tree._bind(eng, S0)

        if self.printing:
            print("\n...planning...")
        self.plan_reached_goal = False
        self.T = np.inf
        run.time_elapsed = 0
        run.time_start = self.sys_time()
        run.best_end = -1
        run.total = None
        run.rate = None                                             # attempts per second of real time, measured
        run.adopted = False
        if retained is not None and retained["goal_hits"] > 0:
            # a kept plan: _plan_after_call asks plan_best() only after a call with NEW hits, so the run starts with it
            self.plan_reached_goal = True
            self.T = self.retained["best_steps"] * self.dt
            run.best_end = self.retained["best_end"]
        return run

    def _tree_resolution(self):
        """What the device tree's edges depend on and replan cannot change: dt and the layout of the edge pools."""
        return (float(self.dt), int(self.hspan[1]) if self.hfactor else int(self.horizon_iters), bool(self.hfactor))

    def replan(self, root, sample_space, goal_bias=0,
               guide=None, xrand_gen=None, pruning=True,
               finish_on_goal=False, specific_time=None, revalidate=True):
        """
        update_plan whose seed is node `root` of the tree the last plan left on this planner's engine -- typically a node of the
        plan being driven, `planner.node_seq[k]` (see plan_node_after).  Not in the reference, which starts every plan from one
        node (planner.py:172) and spends its budget finding the goal again.  The subtree below `root` is kept on the device,
        goal hits included: with `revalidate` every kept edge is first tested against the world as it is NOW (the system's
        obstacles / occupancy grid are synchronised first) and whatever hangs below a failing edge is dropped; the kept nodes are
        renumbered (ascending), goal bookkeeping and ignore set are rebuilt against the current goal (csrc/retain.hpp; the rule:
        tests/retain_reference.py).  Then the same loop, budget, kill and exit rules, wrap-up and return value as update_plan;
        x_seq[0] is the root's state, the kept nodes count toward max_nodes, and a kept plan counts as found from the start.
        `planner.retained` holds what was kept (old_size, kept, outside, infeasible, orphaned, root_feasible, goal_hits, best_end,
        best_steps).  Node ids of the previous plan are void afterwards; a Tree object kept from it stays what it was.  A
        finish_on_goal node lives on the host and is not part of the kept tree.

        ValueError: `root` is not a node of the device tree.  RuntimeError: there is no tree to keep (no previous plan; system,
        max_nodes, wave_size or device changed, which recreates the engine; dt or horizon differ from the ones the tree grew with).
        NotImplementedError: callback mode.
        """
        self._resolve_mode()
        if self.callback_mode:
            raise NotImplementedError("replan: in callback mode the tree's gains and edges live in Python lists and feasibility is the "
                                      "user's Python function, which the device cannot call; use update_plan.")
        root = self._replan_check(root)
        eng = self._engine
        run = self._plan_begin(eng.states(root, 1)[0], sample_space, goal_bias, guide, xrand_gen, pruning, finish_on_goal, specific_time,
                               retain=(root, bool(revalidate)))
        if run is None:
            return False
        return self._plan_loop(run)

    def _replan_check(self, root):
        """What replan refuses (update_plans checks it for every job with a `root` before it touches a planner); returns int(root)."""
        eng = self._engine
        key = (id(self.system), int(self.max_nodes) + self.wave_size + 8, self.wave_size, self.device)
        if eng is None or self._engine_key != key or getattr(self, "_grown_with", None) is None or eng.size < 1:
            raise RuntimeError("replan: there is no tree to keep (no previous plan on this planner's engine, or system / max_nodes / "
                               "wave_size / device changed since); use update_plan.")
        if self._grown_with != self._tree_resolution():
            raise RuntimeError("replan: dt or horizon differ from the ones the tree grew with; use update_plan.")
        root = int(root)
        if not 0 <= root < eng.size:
            raise ValueError("The given parent ID, {}, doesn't exist.".format(root))       # tree.py:84
        return root

    def plan_node_after(self, t):
        """(k, node_id, t_k): the first node of the current plan that is reached at or after time `t` along it -- node_seq[k],
        reached at t_k (the last node when t lies beyond the plan's end).  What a plan-drive-plan loop seeds the next plan with
        (replan) where the reference's loop takes get_state(next_runtime).  Host only."""
        if getattr(self, "node_seq", None) is None or self.tree is None:
            raise RuntimeError("plan_node_after: there is no plan.")
        steps = self.plan_wait                                      # (rows of a wait at the start: avoid(max_wait))
        for k, node in enumerate(self.node_seq):
            steps += len(self.tree.x_seq[int(node)])
            t_k = (steps - 1) * self.dt                             # the node's state is the last row of its edge
            if t_k >= t or k == len(self.node_seq) - 1:
                return k, int(node), t_k

    def _plan_budget(self, run):
        """Attempts the next native call may commit for this plan; a user sampling function is called for as many samples."""
        exit_at = run.min_time if self.plan_reached_goal else run.max_time
        budget = self._attempt_budget(run.rate, exit_at - run.time_elapsed)
        if run.user_sampler and self.xrand_gen_sees_tree:
            budget = 1
        if run.user_sampler:
            missing = budget - run.eng.queued_samples()
            if missing > 0:
                run.eng.push_samples(np.array([np.array(run.xrand_gen(self), dtype=np.float64) for _ in range(missing)]))
        return budget

    def _plan_after_call(self, run, st, dt_call, wrap_up=True):
        """Goal bookkeeping, clock, kill flag and exit rules after a native call (planner.py:260-323); True when the plan is over.
        The wrap-up of a finished plan (plan extraction, finish_on_goal, fallback search, interpolators: milliseconds of host work and
        copies out of HBM) follows at once, or -- wrap_up=False, several planners sharing native calls -- when the caller gets to it
        (`_plan_wrap_up`), so that one planner's wrap-up is not charged to the others' clocks."""
        eng = run.eng
        if st.attempts > 0 and dt_call > 0:
            run.rate = st.attempts / dt_call if run.rate is None else 0.5 * run.rate + 0.5 * st.attempts / dt_call
        run.total = st if run.total is None else _add_stats(run.total, st)

        if st.goal_hits:
            self.plan_reached_goal = True
            end, steps, _ = eng.plan_best()
            if end != run.best_end:                                 # a faster plan (planner.py:276)
                run.best_end = end
                self.T = steps * self.dt
                if self.printing:
                    print("Found plan at elapsed time: {} s".format(np.round(run.time_elapsed, 6)))

        run.time_elapsed = self.sys_time() - run.time_start

        run.outcome = None
        if self.killed:
            run.outcome = "killed"
        elif self.plan_reached_goal and run.time_elapsed >= run.min_time:
            run.outcome = "goal"
        elif run.time_elapsed >= run.max_time or self.tree.size > self.max_nodes:
            run.outcome = "fallback"
        if run.outcome is not None and wrap_up:
            self._plan_wrap_up(run)
        return run.outcome is not None

    def _plan_wrap_up(self, run):
        """What the reference does between leaving its loop and returning (planner.py:293-328) for a plan that `_plan_after_call` ended."""
        if run.outcome == "goal":
            self._adopt_plan(run.best_end)
            run.adopted = True
            if run.finish_on_goal:
                self._finish_on_goal()
            if self.printing:
                print("Tree size: {0}\nETA: {1} s".format(self.tree.size, np.round(self.T, 2)))
            self._prepare_interpolators()
        elif run.outcome == "fallback":
            # no goal hit (or not enough time spent): plan to the node nearest the guide state (planner.py:311-323)
            if getattr(self.system, "riccati", False):
                self.system._engine(self.dt)       # the lqr handle of a Riccati system linearises with THIS planner's dt
            Sguide = np.array(self.lqr(self.xguide, np.zeros(self.ncontrols))[0], dtype=np.float64)
            Sguide[:, np.isinf(np.asarray(self.constraints.goal_buffer, dtype=np.float64))] = 0
            ids, _ = run.eng.nn_argmin(self.xguide.reshape(1, -1), S=Sguide, use_ignore=False)
            self._adopt_plan(int(ids[0]))
            run.adopted = True
            if self.printing:
                print("Didn't reach goal.\nTree size: {0}\nETA: {1} s".format(self.tree.size, np.round(self.T, 2)))
            self._prepare_interpolators()

    def _plan_end(self, run):
        eng = run.eng
        if not run.user_sampler and not run.own_stream:
            eng.sync_numpy_global()
        if self.hfactor:
            self.horizon_iters = eng.horizon_iters_state()           # planner.py:421,424: the heuristic's state persists
        self.stats = run.total.as_dict() if run.total is not None else None

        if self.killed or self.tree.size > self.max_nodes:
            # The reference keeps node_seq / x_seq / u_seq / t_seq up to date inside the loop (planner.py:276-281), so
            # after a kill they describe the best plan of THIS tree whenever one was found.
            if self.killed and not run.adopted and run.best_end >= 0:
                self._adopt_plan(run.best_end)
            if self.printing:
                print("Plan update terminated abruptly!")
            self.killed = False
            return False
        return True

    def _attempt_budget(self, rate, remaining):
        """Attempts the next native call may commit: at most 4 waves, at most what fits in about half of the time left
        at the measured throughput, at least a small wave.  Before a rate is known: one wave."""
        cap = 4 * self.wave_size
        if rate is None:
            return min(cap, self.wave_size)
        if not np.isfinite(remaining):
            return cap
        budget = int(min(cap, max(32, 0.5 * rate * max(float(remaining), 0.0))))
        if self.wave_mode == 'synchronous':                        # whole waves only: the wave size defines the result
            budget = max(self.wave_size, budget // self.wave_size * self.wave_size)
        return budget

    def _adopt_plan(self, end_node):
        """The plan that ends in `end_node`: climb to the seed, lay the edges end to end (planner.py:266-281, :319-323)."""
        self.node_seq = self.tree.climb(end_node)
        self.x_seq, self.u_seq = self.tree.trajectory(self.node_seq)
        self.T = len(self.x_seq) * self.dt
        self.t_seq = np.arange(len(self.x_seq)) * self.dt
        self.plan_wait = 0                                          # (only avoid(max_wait) puts wait rows in front)

    def _finish_on_goal(self):
        """
        planner.py:294-303: steer from the plan's last node to the exact goal (force_arrive) and, if that produced
        anything, tack it onto the plan and the tree.  The reference ends this rollout on a wall-clock timeout of
        clip(min_time/2, 0.1, inf) seconds (:402-406); here the same budget becomes a step cap at the reference's
        measured ~0.3 ms per simulated step, which is deterministic.
        """
        budget_s = float(np.clip(self.min_time / 2, 0.1, np.inf))
        max_steps = int(min(max(budget_s / 3e-4, 64), 20000))
        if getattr(self, "force_arrive_max_steps", None):
            max_steps = int(self.force_arrive_max_steps)            # explicit override of the timeout stand-in
        xgoal_seq, ugoal_seq = self._engine.steer_force(self.node_seq[-1], self.goal, max_steps)
        if len(xgoal_seq) == max_steps and self.printing:
            print("(exact goal-convergence timed-out)")
        if len(xgoal_seq) > 0:
            xs, us = list(xgoal_seq), list(ugoal_seq)
            self.tree.add_node(self.node_seq[-1], self.goal, None, xs, us)
            self.node_seq.append(self.tree.size - 1)
            self.x_seq.extend(xs)
            self.u_seq.extend(us)
            self.t_seq = np.arange(len(self.x_seq)) * self.dt

    def refine_plan(self, max_rounds=8, goal_tries=8):
        """
        Shortens the plan the last update_plan found (not in the reference, whose plan is the tree path of its first goal hit).
        One round tries every shortcut (i, j) of the plan p_0 .. p_{P-1}: from p_i, steer toward p_j .. p_{P-2} and then toward
        the goal (up to `goal_tries` times), one _steer(force_arrive=False) edge per target with the fixed horizon
        `horizon_iters` (no adaptive heuristic), until an edge ends inside the goal region.  The cheapest such chain (fewest
        steps; ties to the smaller i, then j) replaces the plan after p_i if it is shorter; its edges are appended to the tree.
        Rounds repeat until one finds nothing shorter, after `max_rounds`, or when the tree cannot hold the next chain.  The
        search is one kernel launch per round on the device (csrc/refine.hpp); tests/refine_reference.py restates the rule.

        A plan that ends in the finish_on_goal node is refined without it, and the exact-goal steer is then run again from the
        new last node.  Returns the number of rounds accepted (0: nothing changed, e.g. no plan reached the goal).  If a native call
        fails, the rounds accepted before it are adopted (plan, interpolators) and the error is raised.
        """
        if self.callback_mode:                                      # (as the last set_system left it; _resolve_mode would drop the plan)
            raise NotImplementedError("refine_plan: in callback mode the steer is the user's Python function, which every candidate "
                                      "of the search would have to run; the device cannot call it.")
        if int(max_rounds) < 0 or int(goal_tries) < 1:
            raise ValueError("max_rounds must be >= 0 and goal_tries >= 1.")
        run = self._refine_begin()
        if run is None:
            return 0
        eng, error = self._engine, None
        while run.rounds < int(max_rounds):
            try:
                win = eng.refine_round(run.core, run.H, self._refine_incumbent(run), goal_tries)
                if win is None:
                    break
                cost, i, j = win
                ids = eng.refine_commit(run.core, run.H, i, j, goal_tries)
            except (nat.NativeError, ValueError) as ex:
                if getattr(ex, "code", None) != nat.E_CAPACITY:
                    error = ex                                      # raised below, once the rounds already accepted are adopted
                break
            self._refine_accept(run, cost, i, ids)
        rounds = self._refine_end(run)
        if error is not None:
            raise error
        return rounds

    # The three steps of a refinement that refine_plan (one planner, its engine's own calls) and refine_plans (a fleet, batched
    # calls) share: what is refined, what a round's winner changes, what the planner adopts at the end.
    def _refine_begin(self, need_goal=True):
        """The refinement's state (_RefineRun), or None when there is nothing to refine.  Reads only.  connect_goal (need_goal=False)
        also takes a plan that did not reach the goal."""
        tree, eng = self.tree, self._engine
        if (need_goal and not self.plan_reached_goal) or getattr(self, "node_seq", None) is None or tree is None or not tree.on_device \
                or tree._e is not eng:
            return None
        plan = [int(v) for v in self.node_seq]
        finish = len(plan) > 1 and plan[-1] >= eng.size                    # the finish_on_goal node lives on the host (tree.add_node)
        if tree._host_nodes() != (1 if finish else 0):
            raise RuntimeError("refine_plan: the tree holds nodes added with Tree.add_node; refine before adding nodes by hand.")
        run = _RefineRun()
        run.core, run.finish, run.H, run.rounds, run.cost = (plan[:-1] if finish else plan), finish, int(self.horizon_iters), 0, None
        return run

    def _refine_incumbent(self, run):
        """Steps of the plan as it stands: what the next round has to beat (an accepted winner's cost is its plan's)."""
        if run.cost is None:
            lens = self._engine.edge_lengths()
            run.cost = 1 + int(sum(int(lens[p]) for p in run.core[1:]))
        return run.cost

    def _refine_accept(self, run, cost, i, ids):
        """A committed winner: the plan continues below core[i] with the appended nodes."""
        if run.rounds == 0 and run.finish:
            self.tree._drop_host_tail()                                     # refined away; a new one follows in _refine_end
        run.core = run.core[:i + 1] + list(ids)
        run.cost = int(cost)
        run.rounds += 1

    def _refine_end(self, run):
        if run.rounds:
            # the plan describes the tree as it now is, also when a later round failed (a failed commit appends nothing)
            self._adopt_plan(run.core[-1])
            if run.finish:
                self._finish_on_goal()
            self._prepare_interpolators()
        return run.rounds

    def connect_goal(self, goal_tries=8, nodes=None, finish_on_goal=None):
        """
        Asks the WHOLE tree of the last plan the question the loop never asks (it steers a goal-biased sample from the one nearest
        node only): from which node does a short chain of goal-directed steers reach the goal, and which gives the shortest plan?
        Not in the reference.  Every node v (or those of the id list `nodes`) is a candidate: from v's state and gain, steer toward
        the goal up to `goal_tries` times, one _steer(force_arrive=False) edge per try with the fixed horizon `horizon_iters` (no
        adaptive heuristic), until an edge ends inside the goal region.  The candidate with the fewest steps from the root (ties to
        the smaller node id) wins if it beats the current plan -- any valid chain does when that plan did not reach the goal, the
        fallback of a budget that ran out ("Didn't reach goal.").  Its edges are appended to the tree below v and the plan becomes
        climb(v) + the new nodes; plan_reached_goal is set.  The search is one kernel launch on the device (csrc/connect.hpp);
        tests/connect_reference.py restates the rule.  refine_plan() may follow and starts from the new plan.

        `finish_on_goal`: run the exact-goal steer from the new last node -- True / False, or None: as the replaced plan had it (a
        fallback plan has none).  Returns True when the plan was replaced; False, with everything unchanged, when there is no tree
        of this planner on the device, no chain is shorter, or the tree cannot hold the winner's chain.
        """
        self._device_search_check("connect_goal", goal_tries)
        run = self._connect_begin()
        if run is None:
            return False
        eng = self._engine
        win = eng.connect_search(run.H, self._connect_incumbent(run), goal_tries, nodes)
        if win is None:
            return False
        cost, node = win
        ids = self._commit_winner(lambda: eng.connect_commit(node, run.H, goal_tries))
        if ids is None:
            return False
        self._connect_accept(run, cost, node, ids, finish_on_goal)
        return True

    def connect_via(self, waypoints, goal_tries=8, nodes=None, finish_on_goal=None):
        """
        connect_goal with a list of states between the tree and the goal (not in the reference, whose `guide` argument is one state
        for the fallback).  `waypoints` is an array [Q][nstates]: the rest of an earlier plan that this tree no longer holds
        (plan_waypoints(), saved before replan dropped the branch or before a budget ran out on a smaller tree), or the path of a
        coarser planner.  A waypoint need be neither a tree node nor a feasible state.  Every pair (v, j) of a tree node v (or a node
        of the id list `nodes`) and 0 <= j <= Q is a candidate: from v's state and gain, steer toward waypoints[j], waypoints[j + 1],
        ... and then toward the goal up to `goal_tries` times, one _steer(force_arrive=False) edge per target with the fixed horizon
        `horizon_iters`; an empty edge is skipped; the chain ends with the first edge that ends inside the goal region.  The
        candidate with the fewest steps from the root (ties to the smaller node id, then the smaller j) wins if it beats the
        current plan.  j = Q is connect_goal's candidate, so the result is never longer than connect_goal's; without waypoints it
        is connect_goal's.  The appended nodes are candidates of the next call, which may find a shorter plan still (a chain from
        a new node may skip waypoints the first one went through).  The search is one kernel launch on the device
        (csrc/connect_via.hpp); tests/connect_via_reference.py restates the rule.

        What it cannot do: a chain does not steer round an obstacle that blocks it -- the LQR steer is cut where it becomes
        infeasible and the next edge starts there.  After a map change the waypoints beyond a new obstacle are reached only from
        tree nodes that already see them; the feature adds to sampling (update_plan, replan), it does not replace it.

        Return value, refusals, `finish_on_goal` and plan_reached_goal are connect_goal's.  refine_plan() may follow.
        """
        self._device_search_check("connect_via", goal_tries)
        way = np.ascontiguousarray(waypoints, dtype=np.float64)
        if way.size == 0 and way.ndim <= 2:
            way = way.reshape(0, self.nstates)
        if way.ndim != 2 or way.shape[1] != self.nstates:
            raise ValueError("Expected waypoints of shape (Q, %d)." % self.nstates)
        run = self._connect_begin()
        if run is None:
            return False
        eng = self._engine
        win = eng.connect_via_search(way, run.H, self._connect_incumbent(run), goal_tries, nodes)
        if win is None:
            return False
        cost, node, j = win
        ids = self._commit_winner(lambda: eng.connect_via_commit(node, j, way, run.H, goal_tries))
        if ids is None:
            return False
        self._connect_accept(run, cost, node, ids, finish_on_goal)
        return True

    def plan_waypoints(self, start=0):
        """The states of the plan's nodes node_seq[start:] as an array [len][nstates] -- what connect_via takes as waypoints.  Save
        them before a replan or a new update_plan voids the node ids.  Host only; an empty array when there is no plan."""
        seq = getattr(self, "node_seq", None)
        if seq is None or self.tree is None:
            return np.zeros((0, self.nstates))
        state = np.asarray(self.tree.state, dtype=np.float64)
        return np.array([state[v] for v in list(seq)[int(start):]], dtype=np.float64).reshape(-1, self.nstates)

    # The steps of a goal connection that connect_goal (one planner, its engine's own calls) and connect_goals (a fleet, batched
    # calls) share: what is searched, what the search has to beat, what a committed winner changes.  They go through the
    # refinement's own steps.  connect_via, goal_costs and retarget go through them too.
    def _device_search_check(self, name, goal_tries):
        """What the device searches refuse alike, before they look at the tree."""
        if self.callback_mode:                                      # (as the last set_system left it; _resolve_mode would drop the plan)
            raise NotImplementedError("%s: in callback mode the steer is the user's Python function, which every candidate "
                                      "of the search would have to run; the device cannot call it." % name)
        if int(goal_tries) < 1:
            raise ValueError("goal_tries must be >= 1.")

    @staticmethod
    def _commit_winner(commit):
        """The new node ids of commit(), a search's winner replayed into the tree; None, with the tree unchanged, when it cannot
        hold the chain."""
        try:
            return commit()
        except nat.NativeError as ex:
            if ex.code == nat.E_CAPACITY:
                return None
            raise

    def _connect_begin(self):
        """The connection's state (_RefineRun), or None when there is no tree of this planner on the device.  Reads only."""
        run = self._refine_begin(need_goal=False)
        if run is None:
            return None
        if not np.array_equal(self.goal, self._grown_goal):
            raise RuntimeError("connect_goal: the goal changed since the tree was grown; use update_plan or replan.")
        return run

    def _connect_incumbent(self, run):
        """Steps of the plan to beat; a plan that did not reach the goal is beaten by any valid chain."""
        return self._refine_incumbent(run) if self.plan_reached_goal else 2 ** 31 - 1

    def _connect_accept(self, run, cost, node, ids, finish_on_goal):
        """A committed winner: the plan is climb(node) + the appended nodes, and it reaches the goal."""
        run.core = self._engine.climb(node)                         # the plan continues below `node`, its last node
        self._refine_accept(run, cost, len(run.core) - 1, ids)
        if finish_on_goal is not None:
            run.finish = bool(finish_on_goal)
        self.plan_reached_goal = True
        self._refine_end(run)

    def _in_goal(self, x):
        """True if x lies strictly inside the goal box (planner.py:442-447)."""
        x = np.asarray(x, dtype=np.float64)
        lo, hi = np.array(self.goal_region, dtype=np.float64).T
        return bool(np.all((lo < x) & (x < hi)))

    def _prepare_interpolators(self):
        """get_state(t) / get_effort(t) over the current plan; held at the last sample beyond its end (planner.py:451-464)."""
        if len(self.x_seq) == 1:
            only, zero = self.x_seq[0], np.zeros(self.ncontrols)
            self.get_state = lambda t: only
            self.get_effort = lambda t: zero
            return
        for name, seq in (("get_state", self.x_seq), ("get_effort", self.u_seq)):
            table = np.array(seq)
            setattr(self, name, scipy.interpolate.interp1d(self.t_seq, table, axis=0, assume_sorted=True,
                                                           bounds_error=False, fill_value=table[-1].copy()))

    # ------------------------------------------------------------------------------------------ one tree, many goals
    def _goal_costs_targets(self, goals, goal_buffers):
        """(goals [T][nstates], buffers) as goal_costs takes them, or ValueError; fleet_goal_costs asks every planner the same."""
        goals = np.ascontiguousarray(goals, dtype=np.float64)
        if goals.ndim != 2 or goals.shape[1] != self.nstates or len(goals) < 1:
            raise ValueError("Expected goals of shape (T, %d) with T >= 1." % self.nstates)
        buffers = np.asarray(self.constraints.goal_buffer if goal_buffers is None else goal_buffers, dtype=np.float64)
        if buffers.shape not in [(self.nstates,), (len(goals), self.nstates)]:
            raise ValueError("Expected goal_buffers to be None, one buffer of %d entries, or one per goal." % self.nstates)
        if not np.all(buffers >= 0):
            raise ValueError("A goal buffer must not be negative.")
        return goals, buffers

    def goal_costs(self, goals, goal_buffers=None, goal_tries=8, nodes=None):
        """
        What would it cost to go to each of these places instead?  Not in the reference.  The tree of the last plan is rooted at
        the vehicle: which goal it was grown for matters to the goal bias of its samples only.  `goals` is an array [T][nstates];
        `goal_buffers` is None (constraints.goal_buffer for every goal), one buffer, or one per goal.  For every goal on its own,
        connect_goal's question is asked of the whole tree (or of the nodes of the id list `nodes`): from a node's state and gain,
        steer toward the goal up to `goal_tries` times, one _steer(force_arrive=False) edge per try with the fixed horizon
        `horizon_iters`, until an edge ends inside goal -/+ buffer; the chain with the fewest steps from the root wins (ties to the
        smaller node id).  All T searches are ONE kernel launch on the device (csrc/reach.hpp); tests/reach_reference.py restates
        the rule.

        Returns (steps, nodes), two integer arrays of length T: steps[t] is the step count of the cheapest chain to goal t from the
        root (steps * dt is seconds; -1: no chain reaches it), nodes[t] the tree node that chain leaves from (-1: none).  Reads
        only: tree, plan, planner.goal and the device footprint stay as they are, and the answer depends neither on what
        planner.goal currently is nor on whether the plan reached it.  Returns None when there is no tree of this planner on the
        device (refine_plan's condition).  retarget(goals[t]) then makes goal t the planner's.
        """
        self._device_search_check("goal_costs", goal_tries)
        goals, buffers = self._goal_costs_targets(goals, goal_buffers)
        run = self._refine_begin(need_goal=False)
        if run is None:
            return None
        wins = self._engine.reach_search(goals, buffers, run.H, None, goal_tries, nodes)
        steps = np.array([-1 if w is None else w[0] for w in wins], dtype=np.int64)
        start = np.array([-1 if w is None else w[1] for w in wins], dtype=np.int64)
        return steps, start

    def retarget(self, goal, goal_tries=8, nodes=None, finish_on_goal=None):
        """
        The goal has moved: a plan to the new one from the tree the planner already holds, without sampling.  Not in the
        reference, where a new goal means a new plan from one node.  goal_costs' search for the one goal `goal` with
        constraints.goal_buffer; the winner's edges are appended to the tree below its node, `goal` becomes the planner's goal (as
        set_goal does) and the engine's, the plan becomes climb(node) + the new nodes and plan_reached_goal is set.  Afterwards
        connect_goal, connect_via, refine_plan and replan work against the new goal.  `finish_on_goal` is connect_goal's.

        Returns True when the plan was replaced; False, with everything unchanged (planner.goal included), when there is no tree of
        this planner on the device, no chain reaches the goal, or the tree cannot hold the winner's chain.  With the goal the tree
        was grown for -- when it still is the planner's -- this is connect_goal, which replaces a plan only with a shorter one.
        """
        self._device_search_check("retarget", goal_tries)
        goal = np.array(goal, dtype=np.float64)
        if goal.shape != (self.nstates,):
            raise ValueError("The goal state must have same dimensionality as state space.")
        run = self._refine_begin(need_goal=False)
        if run is None:
            return False
        if self.goal is not None and np.array_equal(goal, self._grown_goal) and np.array_equal(self.goal, self._grown_goal):
            return self.connect_goal(goal_tries, nodes, finish_on_goal)
        eng, buff = self._engine, self.constraints.goal_buffer
        win = eng.reach_search(goal[None, :], buff, run.H, None, goal_tries, nodes)[0]
        if win is None:
            return False
        cost, node = win
        ids = self._commit_winner(lambda: eng.reach_commit(goal, buff, node, run.H, goal_tries))
        if ids is None:
            return False
        self.set_goal(goal)
        self._engine_resolution(eng)                                # (the horizon is the tree's: the tree stays)
        self._grown_goal = np.array(self.goal, dtype=np.float64)
        self._connect_accept(run, cost, node, ids, finish_on_goal)
        return True

    # ------------------------------------------------------------------------------------------ moving obstacles
    def avoid(self, tracks, radii, start=0, adopt=True, max_wait=0, connect=0):
        """
        Which plan in the tree stays clear of obstacles that move?  Not in the reference, whose ROS node re-evaluates its one
        plan on the host.  `tracks` gives the centres (world x, y) of D discs at consecutive instants spaced by `dt`: an array
        (L, D, 2), or a list of D arrays (L_d, 2), each held at its last row once it has ended (a vehicle that has arrived sits
        in its berth); `radii` is one radius or one per disc; row `start` of the tracks coincides with the plan's first row.
        Every recorded row of every edge of the tree is tested at ITS time -- its index in a plan's x_seq plus `start` -- with the
        system's feasibility test against the discs of that instant alone (no static map: the tree's edges passed that when
        they were grown), and every goal hit is tested at its last row for as long as the tracks go on after it has arrived.
        The best plan is the goal hit whose whole root path and whose wait at the goal stay clear, fewest steps first, lowest
        node id on ties.  One call on the device (csrc/clear.hpp); tests/clear_reference.py restates the rule.

        Returns a dict: size, conflicts (nodes with a conflict on their own edge), blocked (clear themselves, below a
        conflict), hits, clear_hits, best_end, best_steps (-1: no clear hit) and plan_first -- the time in seconds, from the
        plan's first row, of the first conflict on the CURRENT plan (en route or, for a plan that reached the goal, while it waits
        there; a finish_on_goal tail is not part of the check), None when that plan is clear.  With `adopt` and a clear hit the
        plan becomes that hit's root path (node_seq, x_seq, u_seq, t_seq, T, the interpolators) and plan_reached_goal is set; a
        finish_on_goal tail is not applied to it, because it would not have been checked.  Otherwise the plan is untouched.
        The tree is never modified (but for `connect`, below).  Returns None when there is no tree of this planner on the device
        (refine_plan's condition).  Not covered: chains that connect_goal / connect_via / retarget appended are tested like any
        other edge, but without `connect` nothing is appended here; waiting anywhere but at the start; obstacles that are not discs
        (see avoid_rects).

        `max_wait` in 1 .. 63 also asks "and if I left later?": the vehicle may stand on the plan's first row (the root's) for
        w = 0 .. max_wait rows of dt and follow the tree w rows later; while it stands there the root's row is tested at every
        instant of the wait.  This is meant for a vehicle that can hold station -- as the wait at the goal already assumes.
        All delays are answered by one call on the device (csrc/clear_wait.hpp; tests/clear_wait_reference.py restates the rule).
        The best plan is then the clear (goal hit, delay) that arrives first, wait included -- lowest node id on ties, and of one
        node its shortest clear delay.  The dict holds size, hits, clear_hits (hits that are clear at some delay), clear_now (at
        delay 0: what clear_hits is without max_wait), best_end, best_wait, best_steps (without the wait), best_arrival
        (= best_wait + best_steps) and plan_first, which is None when the current plan is clear as it stands (with the wait it was
        adopted with) and otherwise comes from one more call of the plain query.  On adoption `best_wait` copies of the plan's
        first x_seq and u_seq rows stand in front of it: node_seq is the tree path as ever, T, t_seq and the interpolators go
        over the longer sequence, and `plan_wait` = best_wait says how many rows are the wait (0 after every other call that sets
        a plan).  With max_wait = 0 the call, its cost and its dict are what they were.

        `connect` = goal_tries >= 1 (with max_wait = 0) also asks the nodes that are NOT goal hits: every node whose root path is
        clear is a candidate of connect_goal's search -- up to `connect` steers at the goal with the fixed horizon `horizon_iters`,
        against the static map -- and its chain is accepted only when every row of it is clear of the discs at the time the
        vehicle would be on it, the wait at the goal included, and the plan it gives is strictly shorter than the best clear hit
        (any such chain wins when no hit is clear).  The discs cut no edge: they accept or reject a chain.  Still ONE call on the
        device (csrc/clear_connect.hpp; tests/clear_connect_reference.py restates the rule).  The dict gains clear_candidates,
        chain_from (the node the winning chain leaves from, -1: none), chain_cost (steps from the root, the root's row included),
        chain_rows, chain_arrival (best_steps of the plan the chain gives) and chain_committed.  With `adopt` and a winning chain
        its edges are appended to the tree below chain_from, as connect_goal appends them, and the plan becomes climb(chain_from) +
        the new nodes, without a finish_on_goal tail (it would not have been checked); plan_reached_goal is set and plan_wait is 0.
        THIS IS THE ONE CASE IN WHICH avoid MODIFIES THE TREE.  When the tree cannot hold the chain it stays as it is,
        chain_committed is False and the best clear hit, if any, is adopted as without `connect`; so it is without a winning chain.
        With adopt=False nothing is committed.  plan_first keeps its meaning: it refers to the plan held on entry.  Not covered:
        `connect` together with `max_wait` (ValueError); chains through waypoints.  A fleet asks avoids(connect=...), which shares
        the native calls.  connect = 0 keeps the call, its cost and its dict what they were.
        """
        if self.callback_mode:                                      # (as the last set_system left it; _resolve_mode would drop the plan)
            raise NotImplementedError("avoid: in callback mode the feasibility test is the user's Python function; the device "
                                      "cannot call it on the rows of the tree.")
        table, radii, start = Engine.track_table(tracks, radii, start)
        max_wait = Engine.wait_count(max_wait, "max_wait", 0, 63)
        connect = Engine.wait_count(connect, "connect (goal tries)", 0, 2 ** 31 - 1)
        if connect and max_wait:
            raise ValueError("avoid: connect together with max_wait is not covered; ask one or the other.")
        run = self._avoid_begin()
        if run is None:
            return None
        if connect:
            return self._avoid_connect(run, table, radii, start, adopt, connect)
        if max_wait == 0:
            out, first, dwell = self._engine.tree_clear(table, radii, start, per_node=True)
        else:
            out, clear, dwell_ok = self._engine.tree_clear_wait(table, radii, start, max_wait + 1, per_node=True)
            if self._avoid_plan_holds(run, clear, dwell_ok, max_wait):
                first = dwell = None
            else:                                                   # the time of its first conflict: the plain query, once
                _, first, dwell = self._engine.tree_clear(table, radii, start + self.plan_wait, per_node=True)
        return self._avoid_end(run, out, first, dwell, start, adopt)

    def avoid_rects(self, tracks, extents, start=0, adopt=True, max_wait=0):
        """
        avoid against obstacles that are oriented rectangles -- other hulls: a 6 m x 0.4 m vessel is covered by a disc of 3 m
        radius, and two of them can then never pass in a channel.  `tracks` gives world x, y and heading of D rectangles at
        consecutive instants spaced by `dt`: an array (L, D, 3), or a list of D arrays (L_d, 3), each held at its last row once it
        has ended; `extents` is (half length along the heading, half width), one pair for all or one per rectangle; `start` is
        avoid's.  Time, the wait at the goal, the best plan, the dict (size, conflicts, blocked, hits, clear_hits, best_end,
        best_steps, plan_first), adoption and the refusals are avoid's; only the test of one row differs: the hull points of the
        row's pose (the novice boats: its centre, against extents grown by half the boat length) against the rectangles of its
        instant, point in rectangle with the edge included.  It is geometry only: no static map, not the car's vertex at 2p, not
        BoatAdvanced's planning speed box.  One call on the device (csrc/clear_rects.hpp); tests/clear_rects_reference.py restates
        the rule.  The tree is never modified.  Returns None when there is no tree of this planner on the device.

        `max_wait` in 1 .. 63 is avoid's: the vehicle may stand on the plan's first row for w = 0 .. max_wait rows of dt, tested
        there against the rectangles at every instant of the wait, and follow the tree w rows later -- in a channel the answer
        to an oncoming hull is often "hold the berth two ticks, then take the short branch".  All delays are answered by one call
        on the device (csrc/clear_rects_wait.hpp; tests/clear_rects_wait_reference.py restates the rule); the best plan, the dict
        (size, hits, clear_hits, clear_now, best_end, best_wait, best_steps, best_arrival, plan_first), the adoption with
        `best_wait` copies of the first row in front and `plan_wait`, and the one more plain call for plan_first when the current
        plan does not hold are avoid's with max_wait.  With max_wait = 0 the call, its cost and its dict are what they were.
        A fleet asks avoids_rects, which shares the native calls.  Not covered (DESIGN.md sections 21 to
        23): connect, deconflict(extents=...) with batched or max_wait, discs and rectangles in one call, convex polygons.
        """
        if self.callback_mode:                                      # (as avoid)
            raise NotImplementedError("avoid_rects: in callback mode the feasibility test is the user's Python function; the device "
                                      "cannot call it on the rows of the tree.")
        table, extents, start = Engine.rect_table(tracks, extents, start)
        max_wait = Engine.wait_count(max_wait, "max_wait", 0, 63)
        run = self._avoid_begin()
        if run is None:
            return None
        if max_wait == 0:
            out, first, dwell = self._engine.tree_clear_rects(table, extents, start, per_node=True)
        else:
            out, clear, dwell_ok = self._engine.tree_clear_rects_wait(table, extents, start, max_wait + 1, per_node=True)
            if self._avoid_plan_holds(run, clear, dwell_ok, max_wait):
                first = dwell = None
            else:                                                   # the time of its first conflict: the plain query, once
                _, first, dwell = self._engine.tree_clear_rects(table, extents, start + self.plan_wait, per_node=True)
        return self._avoid_end(run, out, first, dwell, start, adopt)

    # The parts of avoid that it shares with avoids and deconflict(batched=True), which make the device calls for several planners
    # at once: who takes part (_avoid_begin), whether the wait query already shows the current plan to be clear
    # (_avoid_plan_holds), and what an answer leaves behind (_avoid_end).
    def _avoid_begin(self):
        """avoid's state (_RefineRun), or None when there is no tree of this planner on the device.  Reads only."""
        run = self._refine_begin(need_goal=False)
        if run is None:
            return None
        if self.goal is None or not np.array_equal(self.goal, self._grown_goal):
            raise RuntimeError("avoid: the goal changed since the tree was grown; use update_plan, replan or retarget.")
        return run

    def _avoid_connect(self, run, table, radii, start, adopt, goal_tries):
        """avoid(connect=goal_tries): one native call; a winning chain is committed and adopted as connect_goal's winner is, else
        everything is avoid's own."""
        eng = self._engine
        out, chain, first, dwell = eng.tree_clear_connect(table, radii, start, run.H, goal_tries, per_node=True)
        ids = None
        if adopt and chain["chain_from"] >= 0:
            ids = self._commit_winner(lambda: eng.connect_commit(chain["chain_from"], run.H, goal_tries))
        return self._avoid_connect_end(run, out, chain, first, dwell, start, adopt, ids)

    def _avoid_connect_end(self, run, out, chain, first, dwell, start, adopt, ids):
        """What avoid(connect) and avoids(connect) share behind their native calls: the dict of one query's answer and, with the
        new node ids `ids` of a committed chain (None: none was committed), its adoption."""
        out = self._avoid_end(run, out, first, dwell, start, adopt and ids is None)     # (plan_first: of the plan held on entry)
        out.update(chain)
        out["chain_committed"] = ids is not None
        if ids is not None:
            self._connect_accept(run, chain["chain_cost"], chain["chain_from"], ids, False)     # (no tail: it would not have been checked)
            self.plan_wait = 0
        return out

    def _avoid_plan_holds(self, run, clear, dwell_ok, max_wait):
        """From the wait query's masks: the current plan is clear as it stands, with the wait it was adopted with."""
        end, now = run.core[-1], self.plan_wait
        bit = (1 << now) if now <= max_wait else 0
        return bool(int(clear[end]) & bit and (not self.plan_reached_goal or int(dwell_ok[end]) & bit))

    def _avoid_end(self, run, out, first, dwell, start, adopt):
        """avoid's dict from the counters `out` and the plain query's per-node arrays at the current plan's departure (None: the
        plan is clear), and the adoption of the best hit."""
        end = run.core[-1]
        if first is None:
            out["plan_first"] = None
        else:
            taus = [int(first[end])] + ([int(dwell[end])] if self.plan_reached_goal else [])
            taus = [t for t in taus if t >= 0]
            out["plan_first"] = (min(taus) - start) * self.dt if taus else None
        if adopt and out["best_end"] >= 0:
            if run.finish:
                self.tree._drop_host_tail()                         # (the tail of the replaced plan; none is steered for the new one)
            self._adopt_plan(out["best_end"])
            wait = out.get("best_wait", 0)
            if wait > 0:                                            # stand on the first row, then go
                self.x_seq = [np.array(self.x_seq[0]) for _ in range(wait)] + list(self.x_seq)
                self.u_seq = [np.array(self.u_seq[0]) for _ in range(wait)] + list(self.u_seq)
                self.T = len(self.x_seq) * self.dt
                self.t_seq = np.arange(len(self.x_seq)) * self.dt
                self.plan_wait = wait
            self.plan_reached_goal = True
            self._prepare_interpolators()
        return out

    # ------------------------------------------------------------------------------------------ setters
    def set_goal(self, goal):
        """New goal state and goal region (planner.py:468-487); update the plan afterwards."""
        if goal is None:
            self.goal = None
            return
        if len(goal) != self.nstates:
            raise ValueError("The goal state must have same dimensionality as state space.")
        self.goal = np.array(goal, dtype=np.float64)
        buff = np.asarray(self.constraints.goal_buffer, dtype=np.float64)
        self.goal_region = list(zip(self.goal - buff, self.goal + buff))
        self.plan_reached_goal = False

    def set_runtime(self, min_time=None, max_time=None, max_nodes=None, sys_time=None):
        """planner.py:491-513; arguments left at None keep their value."""
        if sys_time is not None and not _callable(sys_time):
            raise ValueError("Expected sys_time to be a function.")
        lo = self.min_time if min_time is None else min_time
        hi = self.max_time if max_time is None else max_time
        self.min_time, self.max_time = lo, hi
        if lo > hi:
            raise ValueError("The min_time must be less than or equal to the max_time.")
        if max_nodes is not None:
            self.max_nodes = max_nodes
        if sys_time is not None:
            self.sys_time = sys_time

    def set_resolution(self, horizon=None, dt=None, FPR=None, error_tol=None):
        """planner.py:517-553; arguments left at None keep their value.  horizon may be a (min, max) pair, which
        switches the adaptive-horizon heuristic on (hfactor = 2, starting from one step)."""
        for name, value in (("horizon", horizon), ("dt", dt), ("FPR", FPR)):
            if value is not None:
                setattr(self, name, value)
        if error_tol is not None:
            if np.shape(error_tol) not in [(), (self.nstates,)]:
                raise ValueError("Shape of error_tol must be scalar or length of state.")
            self.error_tol = np.abs(error_tol).astype(np.float64)
        if hasattr(self.horizon, '__contains__'):
            if len(self.horizon) != 2:
                raise ValueError("Expected horizon to be tuple (min, max) or a single scalar.")
            shortest, longest = self.horizon
            if shortest < self.dt:
                raise ValueError("The minimum horizon must be at least as big as dt.")
            if shortest >= longest:
                raise ValueError("A horizon range tuple must be given as (min, max) where min < max.")
            self.hspan = np.divide(self.horizon, self.dt).astype(np.int64)
            self.horizon_iters, self.hfactor = 1, 2
        else:
            if self.horizon < self.dt:
                raise ValueError("The horizon must be at least as big as dt.")
            steps = int(self.horizon / self.dt)
            self.horizon_iters, self.hspan, self.hfactor = steps, (steps, steps), 0

    def set_system(self, dynamics=None, lqr=None, constraints=None, erf=None):
        """
        planner.py:557-592; arguments left at None keep their value, and dynamics and lqr can only be replaced
        together.  All handles must belong to one native system object.
        """
        if dynamics is not None or lqr is not None:
            if not _callable(dynamics):
                raise ValueError("Expected dynamics to be a function.")
            if not _callable(lqr):
                raise ValueError("Expected lqr to be a function.")
            self.dynamics, self.lqr = dynamics, lqr
        if constraints is not None:
            if not isinstance(constraints, Constraints):
                raise ValueError("Expected constraints to be an instance of the Constraints class.")
            self.constraints = constraints
            self.nstates, self.ncontrols = constraints.nstates, constraints.ncontrols
        if erf is not None:
            if not _callable(erf):
                raise ValueError("Expected erf to be a function.")
            self.erf = erf
            self._erf_angles = False                                # (callback mode: not classified yet)
        self._resolve_mode()
        self.plan_reached_goal = False

    def _resolve_mode(self):
        """Native mode when every plugin is a handle of ONE native system object (then the whole loop runs on the device), callback
        mode as soon as one of them is a plain Python callable.  Handles of different native systems, or np.subtract as the erf of
        a native system with angular states, are mistakes and raise."""
        handles = [(getattr(self, "dynamics", None), "dynamics"), (getattr(self, "lqr", None), "lqr")]
        erf = getattr(self, "erf", None)
        cons = getattr(self, "constraints", None)
        if erf is not None and erf is not np.subtract:
            handles.append((erf, "erf"))
        if cons is not None:
            handles.append((cons.is_feasible, "is_feasible"))
        systems = [native_system_of(f, kind) for f, kind in handles if f is not None]
        if any(sysobj is None for sysobj in systems):
            self.callback_mode, self.system = True, None
            return
        if len(set(id(sysobj) for sysobj in systems)) > 1:
            raise ValueError("dynamics, lqr, erf and constraints.is_feasible belong to different native systems.")
        self.callback_mode, self.system = False, (systems[0] if systems else None)
        if self.system is not None and erf is np.subtract and self.system.wrap_dims:
            raise ValueError("This system has angular states; pass its .erf handle.")
        self.plan_reached_goal = False

    def kill_update(self):
        """Asks a running update_plan (another thread's) to stop; it returns False at its next check."""
        self.killed = True

    def unkill(self):
        """Withdraws a kill_update that has not been honoured yet."""
        self.killed = False

    def visualize(self, dx, dy, show=True):
        """Plots the (dx, dy) cross-section of the tree with the current plan highlighted (planner.py:614-624)."""
        if not hasattr(self, "node_seq"):
            print("There is no plan to visualize!")
            return None
        return self.tree.visualize(dx, dy, node_seq=self.node_seq, show=show)


class _PlanRun(object):
    """What update_plan keeps between native calls of one plan."""


class _RefineRun(object):
    """What refine_plan / refine_plans keep between the rounds of one planner: core (the plan without a finish_on_goal node), finish,
    H (the fixed steer horizon), rounds accepted, cost (steps of core; None until counted)."""


def update_plans(jobs):
    """
    Several planners plan at once: `jobs` is a list of dicts, each with the keys `planner`, `x0`, `sample_space` and, optionally,
    update_plan's keyword arguments (goal_bias, guide, xrand_gen, pruning, finish_on_goal, specific_time) plus `seed` and `group`.
    A job that gives `root` INSTEAD of `x0` is that planner's replan(root, ...): the subtree below node `root` of the tree its last
    plan left on the device is kept, with `revalidate` (default True) against the world as it is now, and the plan is seeded with it
    -- a fleet in a plan-drive-plan loop replans every vehicle every tick without searching for the goal again.  The kept trees of a
    group come from ONE batched native call (lqrrt_tree_retain_multi, csrc/retain.hpp: every stage of the retain one launch for all
    trees), the jobs with `x0` of the same call reset theirs; both kinds may be mixed.  Per planner the result -- `retained`, tree,
    plan -- is that of np.random.seed(seed); planner.replan(root, ...).  Whatever replan refuses (no tree to keep, dt or horizon
    changed: RuntimeError; a root that does not exist: ValueError; replan's messages) is refused here too.
    Every planner gets exactly what its own update_plan would give it -- its tree is the one it grows alone from the same sample
    stream -- but the native calls are shared: lqrrt_engine_extend_multi advances all trees of a GROUP in lock step with two kernel
    launches per tick whatever their number (csrc/engine_multi.hpp), which is how one MI355X is filled by planners that each use ~2 %
    of it (a fleet's vehicles, the behaviours of one vehicle, restarts of one query: 16 trees 6 x, 64 trees 10 x the throughput of one).

    Groups: the planners of one device form a group (a job's `group` key splits a device's planners further); every group runs its own
    shared loop on a host thread of its own (the native call releases the GIL), with no exchange between groups -- planners on the 8
    GPUs of a node are 8 independent fleets, which is the one multi-GPU form of this path that scales with the device count
    (DESIGN.md section 8).  Within a group the planners must share the native system type, horizon, max_nodes, wave_size and pruning,
    and run exact waves of an analytic-gain system (ValueError otherwise -- checked for EVERY job before any planner is touched).

    `seed`: the default sampler of that planner draws from np.random.RandomState(seed) and np.random itself is left alone.  Without it
    a planner starts from np.random's current state, as its own update_plan would: unseeded planners therefore grow THE SAME tree from
    the same start (a warning is printed when that happens), and np.random is left where the first unseeded planner's sampler stopped.

    Time: each planner's clock starts when its group's loop does and is read right after every native call, before anyone's wrap-up;
    a call is sized by the smallest remaining budget of the group and the wrap-up of finished plans is deferred until the group's
    loop has ended, so a planner overruns its max_time by at most one shared call (the same bound as a solo update_plan) whatever
    the number of jobs.  A goal hit of ANY planner ends the running call early once some planner of the group is past its min_time
    (the others just continue with the next call).  Set-up -- per planner, then the group's batched retain, then per planner again --
    happens before the groups' loops start, outside every planner's clock.  If the batched retain fails, the trees of that group's
    planners are unreadable and their next plan builds a fresh engine, as after a failed shared extend call.  Returns the list of
    update_plan's return values.  Not in the reference: its Planner plans one tree on one core.
    """
    keys = ("goal_bias", "guide", "xrand_gen", "pruning", "finish_on_goal", "specific_time", "seed", "group", "revalidate")
    jobs = [dict(j) for j in jobs]
    if not jobs:
        return []
    planners = [j.get("planner") for j in jobs]
    if len(set(id(p) for p in planners)) != len(planners):
        raise ValueError("update_plans: a planner appears twice.")
    groups = {}
    for k, (p, j) in enumerate(zip(planners, jobs)):
        unknown = set(j) - set(keys) - {"planner", "x0", "root", "sample_space"}
        if unknown:
            raise ValueError("update_plans: unknown job key(s) %s." % sorted(unknown))
        if not isinstance(p, Planner) or ("x0" in j) == ("root" in j) or "sample_space" not in j:
            raise ValueError("update_plans: every job needs a planner, sample_space and exactly one of x0 and root.")
        if "revalidate" in j and "root" not in j:
            raise ValueError("update_plans: `revalidate` belongs to a job with a `root`.")
        p._resolve_mode()
        if p.callback_mode:
            raise ValueError("update_plans: planners whose plugins are Python callables plan one by one (update_plan).")
        if p.wave_mode != "exact" or getattr(p.system, "riccati", False):
            raise ValueError("update_plans: exact waves of analytic-gain systems only.")
        # what update_plan itself would refuse, before anything is reset (planner.py:183,196,216)
        xg = j.get("xrand_gen")
        if not (xg is None or type(xg) is int or _callable(xg)):
            raise ValueError("Expected xrand_gen to be None, an integer >= 1,  or a function.")
        if xg is None or type(xg) is int:
            gb = j.get("goal_bias", 0)
            if gb is not None and hasattr(gb, '__contains__') and len(gb) != p.nstates:
                raise ValueError("Expected goal_bias to be scalar or have same length as state.")
            if np.array(j["sample_space"], dtype=np.float64).shape != (p.nstates, 2):
                raise ValueError("Expected sample_space to be list of nstates tuples.")
        groups.setdefault((p.device, j.get("group")), []).append(k)
    for members in groups.values():
        p0, prun0 = planners[members[0]], bool(jobs[members[0]].get("pruning", True))
        if len(members) > 128:
            raise ValueError("update_plans: at most 128 planners per group (split them with the `group` key).")
        for k in members:
            p, j = planners[k], jobs[k]
            same = (type(p.system) is type(p0.system) and tuple(int(v) for v in p.hspan) == tuple(int(v) for v in p0.hspan)
                    and p.hfactor == p0.hfactor and int(p.max_nodes) == int(p0.max_nodes) and p.wave_size == p0.wave_size
                    and bool(j.get("pruning", True)) == prun0)
            if not same:
                raise ValueError("update_plans: the planners of a group must share system type, horizon, max_nodes, wave_size, pruning and device.")
    # what replan refuses, with its messages, for every job with a root
    for p, j in zip(planners, jobs):
        if "root" in j:
            j["root"] = p._replan_check(j["root"])
    unseeded = [k for k, j in enumerate(jobs) if j.get("seed") is None and (j.get("xrand_gen") is None or type(j.get("xrand_gen")) is int)]
    if len(unseeded) > 1 and any(getattr(planners[k], "printing", False) for k in unseeded):
        print("update_plans: %d planners use the default sampler without a `seed`: they all start from np.random's current state." % len(unseeded))

    # Set-up in three steps (Planner._plan_begin's), so that every group does ONE batched retain: each planner alone, the group's
    # trees (tree_retain_multi over the jobs with a root, tree_reset for the others), each planner alone again.
    results = [None] * len(jobs)
    runs = {}
    for k, (p, j) in enumerate(zip(planners, jobs)):
        x0 = p._engine.states(j["root"], 1)[0] if "root" in j else j["x0"]
        run = p._plan_prepare(x0, j["sample_space"], j.get("goal_bias", 0), j.get("guide"), j.get("xrand_gen"),
                              bool(j.get("pruning", True)), j.get("finish_on_goal", False), j.get("specific_time"), seed=j.get("seed"))
        if run is None:
            results[k] = False
        else:
            runs[k] = run
    for g in sorted(groups, key=lambda g: min(groups[g])):
        members = [k for k in groups[g] if k in runs]
        rooted = [k for k in members if "root" in jobs[k]]
        kept = {}
        try:
            if rooted:
                done = Engine.tree_retain_multi([runs[k].eng for k in rooted], [jobs[k]["root"] for k in rooted],
                                                [bool(jobs[k].get("revalidate", True)) for k in rooted])
                kept = {k: stats for k, (stats, _) in zip(rooted, done)}
            for k in members:
                if k not in kept:
                    runs[k].eng.tree_reset(runs[k].x0)              # planner.py:172
        except Exception:
            # as in group_loop below: nothing of these device trees may be read, the next plan builds a fresh engine.  (A Tree
            # object of the plan before was detached in the first step: it is a host copy and stays what it was.)
            for k in members:
                tree = planners[k].tree
                if tree is not None and tree.on_device:
                    tree._e, tree._snap = None, None
                planners[k]._engine_key = None
            raise
        for k in members:
            planners[k]._plan_start(runs[k], kept.get(k))

    def group_loop(members):
        mine = [(k, planners[k], runs[k]) for k in members if k in runs]
        if not mine:
            return
        p0, prun0 = mine[0][1], bool(jobs[mine[0][0]].get("pruning", True))
        # every planner's clock starts when the shared loop does: the others' set-up is not part of its time budget
        for _, p, run in mine:
            run.time_start, run.time_elapsed = p.sys_time(), 0
        active = list(mine)
        try:
            while active:
                budget = min(p._plan_budget(run) for _, p, run in active)
                stop = any(run.time_elapsed >= run.min_time for _, _, run in active)
                t_call = time.perf_counter()
                sts = Engine.extend_multi([run.eng for _, _, run in active], p0.wave_size, max_attempts=budget, node_limit=int(p0.max_nodes),
                                          pruning=prun0, stop_on_goal=bool(stop))
                dt_call = time.perf_counter() - t_call
                # clocks and exit rules of ALL planners first (cheap), wrap-ups after the loop
                active = [(k, p, run) for (k, p, run), st in zip(active, sts) if not p._plan_after_call(run, st, dt_call, wrap_up=False)]
        except Exception:
            # a failed native call leaves every engine of the group mid-wave (include/lqrrt_hip.h): nothing of these trees may be read
            for _, p, run in mine:
                p.tree._e, p.tree._snap = None, None
                p._engine_key = None                                 # the next plan builds a fresh engine
            raise
        for _, p, run in mine:
            p._plan_wrap_up(run)

    order = sorted(groups, key=lambda g: min(groups[g]))
    if len(order) == 1:
        group_loop(groups[order[0]])
    else:
        import threading
        errors = []

        def guarded(members):
            try:
                group_loop(members)
            except Exception as ex:                                  # surfaced on the caller's thread below
                errors.append(ex)
        threads = [threading.Thread(target=guarded, args=(groups[g],)) for g in order]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        if errors:
            raise errors[0]
    synced = False
    for k in sorted(runs):
        run = runs[k]
        if not run.user_sampler and not run.own_stream:
            if synced:
                run.own_stream = True                                # (np.random: left where the first unseeded planner's sampler stopped)
            synced = True
        results[k] = planners[k]._plan_end(run)
    return results


def _add_stats(a, b):
    out = nat.ExtendStats()
    for k, _ in nat.ExtendStats._fields_:
        setattr(out, k, getattr(a, k) + getattr(b, k))
    out.tree_size = b.tree_size
    out.stop_reason = b.stop_reason
    out.candidates = b.candidates
    return out


# What refine_plans, connect_vias and connect_goals share: who may take part, which planners share a native call, and what a commit
# call leaves behind when one of its engines fails.
def _fleet_check(name, planners, goal_tries, nodes=None):
    """Refuses, before any planner is touched: goal_tries < 1, a `nodes` sequence of the wrong length, a planner that appears twice,
    an object that is not a Planner, a callback-mode planner."""
    if int(goal_tries) < 1:
        raise ValueError("goal_tries must be >= 1.")
    if nodes is not None and len(nodes) != len(planners):
        raise ValueError("%s: expected one id list (or None) per planner." % name)
    if len(set(id(p) for p in planners)) != len(planners):
        raise ValueError("%s: a planner appears twice." % name)
    for p in planners:
        if not isinstance(p, Planner):
            raise ValueError("%s: expected Planner objects." % name)
        if p.callback_mode:                                         # (as the last set_system left it, as in the planner's own method)
            raise ValueError("%s: planners whose plugins are Python callables cannot take part (the device cannot call them)." % name)


def _fleet_begin(name, planners, begin):
    """begin(p) of every planner -- its _RefineRun, or None when it takes part in no launch; what the planner's own method refuses
    with RuntimeError is a ValueError here, raised before any planner is touched."""
    try:
        return [begin(p) for p in planners]
    except RuntimeError as ex:
        raise ValueError(str(ex).replace("refine_plan:", name + ":").replace("connect_goal:", name + ":"))


def _fleet_groups(planners, runs):
    """The planners (their indices) that share a native call: those with a run, of one (device, native system type), in slices of
    128 (a native call takes at most 128 engines); groups in the order of their first members."""
    groups = {}
    for k, (p, run) in enumerate(zip(planners, runs)):
        if run is not None:
            groups.setdefault((p.device, type(p.system)), []).append(k)
    for members in groups.values():
        for first in range(0, len(members), 128):
            yield members[first:first + 128]


def _fleet_commit(commit):
    """(new ids per engine, error) of commit(), a commit call for several engines: when it fails after some of its engines did
    commit, their results are kept (their plans follow) and the error is handed back to be raised once they are adopted."""
    try:
        return commit(), None
    except nat.NativeError as ex:
        if getattr(ex, "results", None) is None:
            raise
        return ex.results, ex


def refine_plans(planners, max_rounds=8, goal_tries=8):
    """
    refine_plan for a fleet: every planner gets exactly what its own refine_plan(max_rounds, goal_tries) gives it -- node_seq, x_seq,
    u_seq, t_seq, T, the appended tree nodes, the interpolators, a finish_on_goal node dropped and steered again -- but the native
    calls are shared.  The planners of one (device, native system type) form a group; each round is ONE search launch over the plans
    of the group's still-active planners (Engine.refine_round_multi: a search is bound by its longest chain, not by its width, so the
    rounds of many plans fit side by side) and ONE commit launch over those with a winner (Engine.refine_commit_multi).  A planner
    leaves the active set at its fix-point, after max_rounds or when its tree cannot hold the next chain.  A planner with nothing to
    refine (where refine_plan returns 0 at once) gets 0 and takes part in no launch.  Returns the list of accepted round counts.

    Refused with ValueError for EVERY planner before any is touched: a planner that appears twice, a callback-mode planner, a tree
    that holds hand-added host nodes.  If a native call fails, the rounds accepted so far are adopted by every planner -- those of
    the failing commit call included, for the engines that did commit in it -- then the error is raised (as refine_plan does).
    """
    planners = list(planners)
    if not planners:
        return []
    if int(max_rounds) < 0 or int(goal_tries) < 1:
        raise ValueError("max_rounds must be >= 0 and goal_tries >= 1.")
    _fleet_check("refine_plans", planners, goal_tries)
    runs = _fleet_begin("refine_plans", planners, lambda p: p._refine_begin())
    error = None
    for active in _fleet_groups(planners, runs):
        try:
            while True:
                active = [k for k in active if runs[k].rounds < int(max_rounds)]
                if not active:
                    break
                wins = Engine.refine_round_multi([planners[k]._engine for k in active], [runs[k].core for k in active],
                                                 [runs[k].H for k in active], [planners[k]._refine_incumbent(runs[k]) for k in active],
                                                 goal_tries)
                winners = [(k, w) for k, w in zip(active, wins) if w is not None]
                if not winners:
                    break
                new, failed = _fleet_commit(lambda: Engine.refine_commit_multi(
                    [planners[k]._engine for k, _ in winners], [runs[k].core for k, _ in winners], [runs[k].H for k, _ in winners],
                    [(w[1], w[2]) for _, w in winners], goal_tries))
                active = []
                for (k, w), ids in zip(winners, new):
                    if ids is None:                                 # capacity (or a failed chain): this planner stops with what it has
                        continue
                    planners[k]._refine_accept(runs[k], w[0], w[1], ids)
                    active.append(k)
                if failed is not None:
                    raise failed
        except (nat.NativeError, ValueError) as ex:
            error = ex                                              # raised below, once the rounds already accepted are adopted
            break
    results = [0 if run is None else p._refine_end(run) for p, run in zip(planners, runs)]
    if error is not None:
        raise error
    return results


def connect_vias(planners, waypoints, goal_tries=8, nodes=None, finish_on_goal=None):
    """
    connect_via for a fleet: every planner gets exactly what its own connect_via(waypoints[k], goal_tries, nodes[k], finish_on_goal)
    gives it -- node_seq, x_seq, u_seq, t_seq, T, plan_reached_goal, the appended tree nodes, the interpolators, a finish_on_goal node
    dropped and steered again -- but the native calls are shared.  `waypoints`: one entry per planner, an array [Q_k][nstates] (the
    rest of that planner's last plan, saved with plan_waypoints() before update_plans dropped the branch) or None / empty: that
    planner's search is connect_goal's.  The planners of one (device, native system type) form a group; a group makes ONE search call
    over its trees (Engine.connect_via_search_multi: every tree with its own waypoint table and a best key of its own, so each winner
    is the one the planner's own search finds) and ONE commit call over those with a winner (Engine.connect_via_commit_multi), in
    slices of 128.  `nodes`: None, or one entry per planner, each None (every node) or an id list.  A planner with no tree of its own
    on the device (where connect_via returns False at once) takes part in no launch; one whose tree cannot hold the chain gets False
    and is unchanged.  Returns the list of bools.

    Refused with ValueError for EVERY planner before any is touched: everything connect_goals refuses, a `waypoints` sequence of the
    wrong length, an array not of shape (Q, nstates).  If a native call fails, the planners that did commit adopt their plans -- those
    of the failing commit call included -- then the error is raised.
    """
    planners, waypoints, nodes = list(planners), list(waypoints), None if nodes is None else list(nodes)
    if len(waypoints) != len(planners):
        raise ValueError("connect_vias: expected one waypoint array (or None) per planner.")
    _fleet_check("connect_vias", planners, goal_tries, nodes)
    ways = []
    for k, (p, w) in enumerate(zip(planners, waypoints)):
        way = np.ascontiguousarray(() if w is None else w, dtype=np.float64)
        if way.size == 0 and way.ndim <= 2:
            way = way.reshape(0, p.nstates)
        if way.ndim != 2 or way.shape[1] != p.nstates:
            raise ValueError("connect_vias: expected waypoints of shape (Q, %d) for planner %d." % (p.nstates, k))
        ways.append(way)
    runs = _fleet_begin("connect_vias", planners, lambda p: p._connect_begin())
    results = [False] * len(planners)
    for mine in _fleet_groups(planners, runs):
        wins = Engine.connect_via_search_multi([planners[k]._engine for k in mine], [ways[k] for k in mine], [runs[k].H for k in mine],
                                               [planners[k]._connect_incumbent(runs[k]) for k in mine], goal_tries,
                                               None if nodes is None else [nodes[k] for k in mine])
        winners = [(k, w) for k, w in zip(mine, wins) if w is not None]
        if not winners:
            continue
        new, failed = _fleet_commit(lambda: Engine.connect_via_commit_multi(
            [planners[k]._engine for k, _ in winners], [(w[1], w[2]) for _, w in winners], [ways[k] for k, _ in winners],
            [runs[k].H for k, _ in winners], goal_tries))
        for (k, w), ids in zip(winners, new):
            if ids is None:                                         # capacity (or a failed chain): this planner keeps what it has
                continue
            planners[k]._connect_accept(runs[k], w[0], w[1], ids, finish_on_goal)
            results[k] = True
        if failed is not None:
            raise failed
    return results


def connect_goals(planners, goal_tries=8, nodes=None, finish_on_goal=None):
    """
    connect_goal for a fleet: every planner gets exactly what its own connect_goal(goal_tries, nodes[k], finish_on_goal) gives it --
    node_seq, x_seq, u_seq, t_seq, T, plan_reached_goal, the appended tree nodes, the interpolators, a finish_on_goal node dropped
    and steered again -- but the native calls are shared.  The planners of one (device, native system type) form a group; a group
    makes ONE search call over its trees (Engine.connect_search_multi: every tree with a best key of its own, so each winner is the
    one the planner's own search finds) and ONE commit call over those with a winner (Engine.connect_commit_multi), in slices of 128.
    `nodes`: None, or one entry per planner, each None (every node) or an id list.  A planner with no tree of its own on the device
    (where connect_goal returns False at once) takes part in no launch; one whose tree cannot hold the chain gets False and is
    unchanged.  Returns the list of bools.

    Refused with ValueError for EVERY planner before any is touched: a planner that appears twice, an object that is not a Planner,
    a callback-mode planner, a tree that holds hand-added host nodes, a goal changed since the tree was grown, goal_tries < 1, a
    `nodes` sequence of the wrong length.  If a native call fails, the planners that did commit adopt their plans -- those of the
    failing commit call included -- then the error is raised.
    """
    planners, nodes = list(planners), None if nodes is None else list(nodes)
    _fleet_check("connect_goals", planners, goal_tries, nodes)
    runs = _fleet_begin("connect_goals", planners, lambda p: p._connect_begin())
    results = [False] * len(planners)
    for mine in _fleet_groups(planners, runs):
        wins = Engine.connect_search_multi([planners[k]._engine for k in mine], [runs[k].H for k in mine],
                                           [planners[k]._connect_incumbent(runs[k]) for k in mine], goal_tries,
                                           None if nodes is None else [nodes[k] for k in mine])
        winners = [(k, w) for k, w in zip(mine, wins) if w is not None]
        if not winners:
            continue
        new, failed = _fleet_commit(lambda: Engine.connect_commit_multi(
            [planners[k]._engine for k, _ in winners], [w[1] for _, w in winners], [runs[k].H for k, _ in winners], goal_tries))
        for (k, w), ids in zip(winners, new):
            if ids is None:                                         # capacity (or a failed chain): this planner keeps what it has
                continue
            planners[k]._connect_accept(runs[k], w[0], w[1], ids, finish_on_goal)
            results[k] = True
        if failed is not None:
            raise failed
    return results


def fleet_goal_costs(planners, goals, goal_buffers=None, goal_tries=8, nodes=None):
    """
    goal_costs for a fleet: the task-assignment matrix, P planners x T places, with the native calls shared.  `goals` is ONE array
    [T][nstates] that every planner is asked about (berths, tasks); `goal_buffers` is None (each planner's own
    constraints.goal_buffer), one buffer, or one per goal.  Returns (steps, nodes), two integer arrays of shape (P, T): row k is
    exactly what planners[k].goal_costs(goals, goal_buffers, goal_tries, nodes[k]) returns, and all -1 where that returns None (no
    tree of that planner on the device: it takes part in no launch).  The planners of one (device, native system type) form a
    group; a group makes ONE search call over its trees (Engine.reach_search_multi: every (tree, goal) pair with a best key of its
    own, so each entry is the one the planner's own search finds), in slices of 128.  `nodes`: None, or one entry per planner, each
    None (every node) or an id list.  Reads only.  An assignment can be drawn from the matrix on the host; retargets() then gives
    every planner its goal.

    Refused with ValueError for EVERY planner before any is touched: a planner that appears twice, an object that is not a Planner,
    a callback-mode planner, a tree that holds hand-added host nodes, goal_tries < 1, a `nodes` sequence of the wrong length, goals
    not of shape (T, nstates) with T >= 1 for every planner's nstates, goal buffers of the wrong shape or negative.
    """
    planners, nodes = list(planners), None if nodes is None else list(nodes)
    _fleet_check("fleet_goal_costs", planners, goal_tries, nodes)
    goals = np.ascontiguousarray(goals, dtype=np.float64)
    if goals.ndim != 2 or len(goals) < 1:
        raise ValueError("fleet_goal_costs: expected goals of shape (T, nstates) with T >= 1.")
    buffers = []
    for k, p in enumerate(planners):
        if p.nstates != goals.shape[1]:
            raise ValueError("fleet_goal_costs: planner %d has %d states, the goals have %d." % (k, p.nstates, goals.shape[1]))
        buffers.append(p._goal_costs_targets(goals, goal_buffers)[1])
    runs = _fleet_begin("fleet_goal_costs", planners, lambda p: p._refine_begin(need_goal=False))
    steps = np.full((len(planners), len(goals)), -1, dtype=np.int64)
    start = np.full((len(planners), len(goals)), -1, dtype=np.int64)
    for mine in _fleet_groups(planners, runs):
        wins = Engine.reach_search_multi([planners[k]._engine for k in mine], [goals] * len(mine), [buffers[k] for k in mine],
                                         [runs[k].H for k in mine], None, goal_tries, None if nodes is None else [nodes[k] for k in mine])
        for k, row in zip(mine, wins):
            for t, w in enumerate(row):
                if w is not None:
                    steps[k, t], start[k, t] = w
    return steps, start


def retargets(planners, goals, goal_tries=8, nodes=None, finish_on_goal=None):
    """
    retarget for a fleet: every planner gets exactly what its own retarget(goals[k], goal_tries, nodes[k], finish_on_goal) gives it --
    the appended tree nodes, node_seq, x_seq, u_seq, t_seq, T, plan_reached_goal, planner.goal and the engine's goal and box, the
    interpolators, a finish_on_goal node dropped and steered again; on False everything unchanged -- but the native calls are shared.
    `goals`: one entry per planner, its new goal [nstates] or None: that planner sits out and gets False.  The planners whose goal is
    the one their tree was grown for (and still is theirs) go together through connect_goals, as retarget hands them to connect_goal.
    The others form groups by (device, native system type); a group makes ONE search call over its trees with one target each
    (Engine.reach_search_multi) and ONE commit call over those with a winner (Engine.reach_commit_multi), in slices of 128.
    `nodes`: None, or one entry per planner, each None (every node) or an id list.  Returns the list of bools.

    Refused with ValueError for EVERY planner before any is touched: everything connect_goals refuses but a changed goal, a `goals`
    sequence of the wrong length, a goal not of shape (nstates,).  If a native call fails, the planners that did commit adopt their
    plans and goals -- those of the failing commit call included -- then the error is raised.
    """
    planners, goals, nodes = list(planners), list(goals), None if nodes is None else list(nodes)
    if len(goals) != len(planners):
        raise ValueError("retargets: expected one goal (or None) per planner.")
    _fleet_check("retargets", planners, goal_tries, nodes)
    new = []
    for k, (p, g) in enumerate(zip(planners, goals)):
        g = None if g is None else np.array(g, dtype=np.float64)
        if g is not None and g.shape != (p.nstates,):
            raise ValueError("retargets: the goal of planner %d must have the dimensionality of its state space." % k)
        new.append(g)
    runs = _fleet_begin("retargets", planners, lambda p: p._refine_begin(need_goal=False))
    runs = [None if g is None else run for g, run in zip(new, runs)]
    results = [False] * len(planners)
    # where retarget is connect_goal: the goal the tree was grown for, still the planner's
    same = [k for k, (p, g) in enumerate(zip(planners, new)) if runs[k] is not None and p.goal is not None
            and np.array_equal(g, p._grown_goal) and np.array_equal(p.goal, p._grown_goal)]
    if same:
        for k, ok in zip(same, connect_goals([planners[k] for k in same], goal_tries, None if nodes is None else [nodes[k] for k in same],
                                             finish_on_goal)):
            results[k] = ok
            runs[k] = None
    for mine in _fleet_groups(planners, runs):
        buffs = dict((k, planners[k].constraints.goal_buffer) for k in mine)
        wins = Engine.reach_search_multi([planners[k]._engine for k in mine], [new[k][None, :] for k in mine], [buffs[k] for k in mine],
                                         [runs[k].H for k in mine], None, goal_tries, None if nodes is None else [nodes[k] for k in mine])
        winners = [(k, w[0]) for k, w in zip(mine, wins) if w[0] is not None]
        if not winners:
            continue
        ids_of, failed = _fleet_commit(lambda: Engine.reach_commit_multi(
            [planners[k]._engine for k, _ in winners], [new[k] for k, _ in winners], [buffs[k] for k, _ in winners],
            [w[1] for _, w in winners], [runs[k].H for k, _ in winners], goal_tries))
        for (k, w), ids in zip(winners, ids_of):
            if ids is None:                                         # capacity (or a failed chain): this planner keeps what it has
                continue
            p = planners[k]
            p.set_goal(new[k])                                      # (retarget's steps, in retarget's order)
            p._engine_resolution(p._engine)
            p._grown_goal = np.array(p.goal, dtype=np.float64)
            p._connect_accept(runs[k], w[0], w[1], ids, finish_on_goal)
            results[k] = True
        if failed is not None:
            raise failed
    return results


def deconflict(planners, radii, order=None, start=0, max_wait=0, batched=False, connect=0, extents=None):
    """
    Prioritised planning over the trees as they stand: in `order` (default: as listed) every planner picks, with Planner.avoid, the
    best plan of its tree that stays clear of the plans of the planners before it -- each of those a disc of its radius that moves
    along its plan's x_seq[:, :2] and then sits where it arrived.  `radii`: one radius for every vehicle, or one per planner (in the
    order of `planners`).  `start` is avoid's: row `start` of the earlier plans coincides with a later planner's first row (0: all
    plans begin at the same instant).  The first planner of the order has nothing to avoid and is not asked.  A planner without a
    clear hit keeps its plan, is reported as such (best_end -1), and still counts as a track for the later ones.  `max_wait` is
    avoid's too: a planner may leave up to max_wait rows of dt late ("the other one crosses my short branch: I leave two ticks
    later"); the rows of its wait stand in its x_seq, so the planners after it see it waiting at its start.

    Returns one entry per planner, in the order of `planners`: avoid's dict, or None for the first of the order and for a planner
    without a tree on the device.  It costs one device call per planner after the first: a planner's tracks are the plans the
    earlier ones ended up with, so the priority order makes the calls sequential by nature; by default nothing is batched across
    planners.

    `batched=True` gives the same results, plans and dicts through launches that span the trees (avoids' calls,
    csrc/clear_multi.hpp), in rounds: every planner keeps a candidate plan -- on entry the one it holds --, a round asks all
    "dirty" planners in ONE batched call, each against the current candidates of those before it, and a planner is dirty in the
    next round iff a candidate before it changed; the first round asks everybody but the first of the order, the loop ends when
    nothing changed, and the plans are adopted once, at the end.  The fixed point is the sequential answer: by induction,
    position r of the order is final after round r -- the positions before it were final one round earlier, so in round r it is
    asked against exactly the tracks the loop would show it, or it was asked against them before and nothing has changed since --
    so there are at most n - 1 rounds.  What it costs: in the worst case (every round changes only the next position) each round
    checks every tree behind the change again, n (n - 1) / 2 tree checks instead of the loop's n - 1, in exchange for rounds of
    one launch sequence each instead of n - 1 dependent calls; when the first answers already stand -- traffic that rarely
    conflicts -- it is two rounds, or one.  What avoid refuses with RuntimeError (the goal changed) is a ValueError then, raised
    before any planner is touched, as in avoids.

    `connect` = goal_tries >= 1 is avoid's as well: the sequential form hands it to every Planner.avoid, and a planner that adopts
    a goal chain is then a track with that chain's rows for the planners after it.  Not covered, and refused with ValueError:
    `connect` with batched=True -- a chain candidate has no rows in any tree until it is committed, and the rounds adopt only at
    the end -- and `connect` together with `max_wait`, as in avoid.

    `extents` = (half length, half width), one pair for every vehicle or one per planner (n, 2), makes every earlier planner an
    oriented RECTANGLE instead of a disc: it moves along its plan's x_seq[:, :3] -- x, y and heading, state index 2 -- and then sits
    where it arrived, and every planner asks Planner.avoid_rects.  `radii` must then be None.  Sequential form only: with `extents`,
    `max_wait`, batched=True and `connect` are not covered and refused with ValueError.  Without `extents` nothing changes.

    Refused with ValueError before any planner is touched: planners that do not share `dt`, a planner twice, an `order` that is no
    permutation, `radii` of the wrong shape or negative, a `max_wait` that is no integer in 0 .. 63, a planner without a plan (it
    cannot be a track).  Callback mode raises
    NotImplementedError, as avoid does.
    """
    planners = list(planners)
    n = len(planners)
    order = list(range(n)) if order is None else [int(k) for k in order]
    if sorted(order) != list(range(n)):
        raise ValueError("deconflict: order must be a permutation of the planners' indices.")
    if len(set(id(p) for p in planners)) != n:
        raise ValueError("deconflict: a planner appears twice.")
    if extents is not None:
        if radii is not None:
            raise ValueError("deconflict: with extents the vehicles are rectangles; radii must be None.")
        ext = np.asarray(extents, dtype=np.float64)
        if ext.shape not in [(2,), (n, 2)]:
            raise ValueError("deconflict: expected extents as one (half length, half width), or one pair per planner.")
        ext = np.broadcast_to(ext, (n, 2))
        if not (np.all(ext >= 0) and np.all(np.isfinite(ext))):
            raise ValueError("deconflict: an extent must be >= 0 and finite.")
        if max_wait != 0 or batched or connect != 0:
            raise ValueError("deconflict: with extents, max_wait, batched=True and connect are not covered.")
        r = np.zeros(n)
    else:
        r = np.asarray(radii, dtype=np.float64)
        if r.shape not in [(), (n,)]:
            raise ValueError("deconflict: expected one radius, or one per planner.")
        r = np.broadcast_to(r, (n,))
        if not np.all(r >= 0):
            raise ValueError("deconflict: a radius must be >= 0.")
    if int(start) != start or int(start) < 0:
        raise ValueError("deconflict: start must be an integer >= 0.")
    max_wait = Engine.wait_count(max_wait, "deconflict: max_wait", 0, 63)
    connect = Engine.wait_count(connect, "deconflict: connect (goal tries)", 0, 2 ** 31 - 1)
    if connect and max_wait:
        raise ValueError("deconflict: connect together with max_wait is not covered; ask one or the other.")
    if connect and batched:
        raise ValueError("deconflict: connect with batched=True is not covered: a chain has no rows in any tree until it is "
                         "committed, and the rounds adopt only at the end.")
    for k, p in enumerate(planners):
        if p.callback_mode:
            raise NotImplementedError("deconflict: planner %d is in callback mode; the device cannot call its Python feasibility test." % k)
    if any(p.dt != planners[0].dt for p in planners):
        raise ValueError("deconflict: the planners must share dt (the tracks are sampled at it).")
    for k, p in enumerate(planners):
        if getattr(p, "x_seq", None) is None or len(p.x_seq) < 1:
            raise ValueError("deconflict: planner %d has no plan; it cannot be a track." % k)
    if batched:
        return _deconflict_batched(planners, r, order, int(start), max_wait)[0]
    results = [None] * n
    for at, k in enumerate(order):
        if at == 0:
            continue
        before = order[:at]
        if extents is not None:
            tracks = [np.asarray(planners[j].x_seq, dtype=np.float64)[:, :3] for j in before]
            results[k] = planners[k].avoid_rects(tracks, ext[before], start)
            continue
        tracks = [np.asarray(planners[j].x_seq, dtype=np.float64)[:, :2] for j in before]
        results[k] = planners[k].avoid(tracks, r[before], start, max_wait=max_wait, connect=connect)
    return results


def _deconflict_rounds(order, entry, ask):
    """
    The schedule of deconflict(batched=True), with nothing of the device in it.  `order`: the priority order (planner indices);
    `entry`: per planner (by index) the candidate it comes with -- any value that compares with ==; ask(ks, candidates): for the
    planners `ks` (in the order's order) their answers as (candidate, answer) pairs, planner k asked against candidates[j] of the
    planners j before it in the order -- one batched launch; `answer` is kept for the caller and not looked at here.

    Round 1 asks everybody but the first of the order; a planner is asked again in the next round iff the candidate of a planner
    before it changed in this one, i.e. the planners behind the earliest change are.  The loop ends when a round changed nothing.
    Why the fixed point is the sequential answer, by induction on the position r in the order: position 0 is never asked, so it is
    final from the start; if the positions before r are final after round r - 1, then in round r position r is either asked against
    exactly the candidates the sequential loop would show it, or it is not dirty -- nothing before it has changed since it was
    last asked -- and the answer it holds is already that one.  So position r is final after round r, a change in round r lies at a
    position >= r, and after at most n - 1 rounds nothing is dirty.

    Returns (candidates, answers, log): the final candidate and the last answer per planner (None where never asked) and, per
    round, the list of planners asked.
    """
    order = list(order)
    cand, answers, log = list(entry), [None] * len(entry), []
    dirty = order[1:]
    while dirty:
        got = ask(list(dirty), list(cand))
        log.append(list(dirty))
        earliest = None
        for k, (c, answer) in zip(dirty, got):
            answers[k] = answer
            if not c == cand[k]:
                cand[k] = c
                at = order.index(k)
                earliest = at if earliest is None else min(earliest, at)
        dirty = [] if earliest is None else order[earliest + 1:]
    return cand, answers, log


def _fleet_avoid_runs(name, planners):
    """Every planner's _avoid_begin; what avoid refuses with RuntimeError is a ValueError here, raised before any planner is touched."""
    try:
        return [p._avoid_begin() for p in planners]
    except RuntimeError as ex:
        raise ValueError(str(ex).replace("avoid:", name + ":").replace("refine_plan:", name + ":"))


def _avoids_query(planners, runs, tables, radii, starts, max_wait, query=None):
    """The device calls of avoid for the planners that have a run, batched: per planner (counters, first, dwell) -- first / dwell the
    plain query's per-node arrays at the current plan's departure, or None where the wait query shows that plan to be clear -- and
    None for a planner without a run.  One native call per group of _fleet_groups, and with max_wait ONE more (the plain query for
    the planners whose current plan is not clear).  Touches no planner.  Returns (results, native calls made).  `query`: the pair
    of Engine calls (plain, wait) that answer; None: the discs' (tree_clear_multi, tree_clear_wait_multi).  avoids_rects passes the
    rectangles' pair, and `radii` then holds the extents."""
    plain_multi, wait_multi = (Engine.tree_clear_multi, Engine.tree_clear_wait_multi) if query is None else query
    res, calls = [None] * len(planners), 0
    for members in _fleet_groups(planners, runs):
        pick = lambda seq, ks: [seq[k] for k in ks]
        engines = [planners[k]._engine for k in members]
        if max_wait == 0:
            got = plain_multi(engines, pick(tables, members), pick(radii, members), pick(starts, members), per_node=True)
            calls += 1
            for k, g in zip(members, got):
                res[k] = g
            continue
        got = wait_multi(engines, pick(tables, members), pick(radii, members), pick(starts, members), max_wait + 1, per_node=True)
        calls += 1
        again = []
        for k, (out, clear, dwell_ok) in zip(members, got):
            res[k] = (out, None, None)
            if not planners[k]._avoid_plan_holds(runs[k], clear, dwell_ok, max_wait):
                again.append(k)
        if again:                                                   # the time of their plans' first conflict: the plain query, once for all
            got = plain_multi([planners[k]._engine for k in again], pick(tables, again), pick(radii, again),
                              [starts[k] + planners[k].plan_wait for k in again], per_node=True)
            calls += 1
            for k, (_, first, dwell) in zip(again, got):
                res[k] = (res[k][0], first, dwell)
    return res, calls


def avoids(planners, tracks, radii, start=0, adopt=True, max_wait=0, connect=0):
    """
    avoid for a fleet: every planner gets exactly what its own avoid(tracks, radii, start, adopt, max_wait) returns and leaves --
    the dict (plan_first included), the adopted plan, plan_wait, plan_reached_goal, the dropped finish_on_goal tail, None for a
    planner without a tree of its own on the device -- but the device calls are shared: the planners of one (device, native system
    type) form a group, and a group's trees are checked in ONE native call (Engine.tree_clear_multi / tree_clear_wait_multi,
    csrc/clear_multi.hpp: every stage one launch that spans the trees), in slices of 128.  With `max_wait` the planners whose
    current plan is not clear get the plain query at their plan's departure, for plan_first, in ONE further call per group.
    `tracks`, `radii`: one set for everybody, as avoid takes it -- the shared-traffic case: the table is uploaded once per launch,
    not once per tree -- or a list with one such entry per planner (tracks: a list of len(planners) entries, each an array
    (L, D, 2) or a list of D arrays (L_d, 2); radii: the matching list).  The trees are never modified (but for `connect`).

    `connect` = goal_tries >= 1 (with max_wait = 0) is avoid's: every planner gets exactly what its own avoid(..., connect=connect)
    returns and leaves -- the dict with the five chain fields and chain_committed, plan_first of the plan held on entry, the committed
    chain and the adopted plan, plan_wait = 0, plan_reached_goal.  A group makes ONE query (Engine.tree_clear_connect_multi,
    csrc/clear_connect_multi.hpp: the clearance stages, one seed and one search launch over all its trees, every tree with a key of
    its own) and then, over the members that have `adopt` and a winning chain, ONE commit (Engine.connect_commit_multi), as
    connect_goals does it.  A member whose tree cannot hold its chain gets chain_committed = False and adopts its best clear hit as
    without `connect`.  If a native commit call fails, the planners that did commit adopt their plans, then the error is raised.
    connect = 0 keeps the calls and the dicts what they were.

    Refused before any planner is touched: `connect` together with `max_wait`; everything avoid refuses (a changed goal, which avoid refuses with RuntimeError, is a
    ValueError here, as in the other fleet calls), a planner that appears twice, an object that is no Planner, per-planner tracks
    without per-planner radii.  Callback mode raises NotImplementedError, as in deconflict.
    """
    planners = list(planners)
    n = len(planners)
    if len(set(id(p) for p in planners)) != n:
        raise ValueError("avoids: a planner appears twice.")
    for k, p in enumerate(planners):
        if not isinstance(p, Planner):
            raise ValueError("avoids: expected Planner objects.")
        if p.callback_mode:
            raise NotImplementedError("avoids: planner %d is in callback mode; the device cannot call its Python feasibility test." % k)
    per = n > 0 and isinstance(tracks, (list, tuple)) and len(tracks) == n and all(isinstance(t, (list, tuple)) or np.ndim(t) == 3 for t in tracks)
    if per:
        if not isinstance(radii, (list, tuple, np.ndarray)) or len(radii) != n:
            raise ValueError("avoids: tracks per planner need radii per planner (a list of %d entries)." % n)
        tabs = [Engine.track_table(tracks[k], radii[k], start) for k in range(n)]
    else:
        tabs = [Engine.track_table(tracks, radii, start)] * n
    max_wait = Engine.wait_count(max_wait, "max_wait", 0, 63)
    connect = Engine.wait_count(connect, "connect (goal tries)", 0, 2 ** 31 - 1)
    if connect and max_wait:
        raise ValueError("avoids: connect together with max_wait is not covered; ask one or the other.")
    if not planners:
        return []
    start = tabs[0][2]
    runs = _fleet_avoid_runs("avoids", planners)
    if connect:
        return _avoids_connect(planners, runs, [t[0] for t in tabs], [t[1] for t in tabs], start, adopt, connect)
    got, _ = _avoids_query(planners, runs, [t[0] for t in tabs], [t[1] for t in tabs], [start] * n, max_wait)
    return [None if run is None else p._avoid_end(run, g[0], g[1], g[2], start, adopt) for p, run, g in zip(planners, runs, got)]


def avoids_rects(planners, tracks, extents, start=0, adopt=True, max_wait=0):
    """
    avoid_rects for a fleet, as avoids is avoid for a fleet: every planner gets exactly what its own avoid_rects(tracks, extents,
    start, adopt, max_wait) returns and leaves -- the dict (plan_first included), the adopted plan with its wait rows, plan_wait, T,
    t_seq, plan_reached_goal, the dropped finish_on_goal tail, None for a planner without a tree of its own on the device -- but the
    device calls are shared: the planners of one (device, native system type) form a group, and a group's trees are checked in ONE
    native call (Engine.tree_clear_rects_multi / tree_clear_rects_wait_multi, csrc/clear_rects_multi.hpp: every stage one launch that
    spans the trees), in slices of 128.  With `max_wait` the planners whose current plan is not clear get the plain query at their
    plan's departure, for plan_first, in ONE further call per group.  `tracks`, `extents`: one set for everybody, as avoid_rects
    takes it -- the shared-traffic case: the table (poses and extents) is built and uploaded once per launch, not once per tree --
    or a list with one such entry per planner (tracks: a list of len(planners) entries, each an array (L, D, 3) or a list of D
    arrays (L_d, 3); extents: the matching list).  The trees are never modified.  Both fleets run one path (_avoids_query).

    Refused before any planner is touched: everything avoid_rects refuses (a changed goal, which avoid_rects refuses with
    RuntimeError, is a ValueError here, as in the other fleet calls), a planner that appears twice, an object that is no Planner,
    per-planner tracks without per-planner extents.  Callback mode raises NotImplementedError.  There is no `connect`: there is no
    rectangle connect yet.  Not covered: deconflict(extents=...) with batched or max_wait, connect against
    rectangles, discs and rectangles in one call, convex polygons.
    """
    planners = list(planners)
    n = len(planners)
    if len(set(id(p) for p in planners)) != n:
        raise ValueError("avoids_rects: a planner appears twice.")
    for k, p in enumerate(planners):
        if not isinstance(p, Planner):
            raise ValueError("avoids_rects: expected Planner objects.")
        if p.callback_mode:
            raise NotImplementedError("avoids_rects: planner %d is in callback mode; the device cannot call its Python feasibility test." % k)
    per = n > 0 and isinstance(tracks, (list, tuple)) and len(tracks) == n and all(isinstance(t, (list, tuple)) or np.ndim(t) == 3 for t in tracks)
    if per:
        if not isinstance(extents, (list, tuple, np.ndarray)) or len(extents) != n:
            raise ValueError("avoids_rects: tracks per planner need extents per planner (a list of %d entries)." % n)
        tabs = [Engine.rect_table(tracks[k], extents[k], start) for k in range(n)]
    else:
        tabs = [Engine.rect_table(tracks, extents, start)] * n
    max_wait = Engine.wait_count(max_wait, "max_wait", 0, 63)
    if not planners:
        return []
    start = tabs[0][2]
    runs = _fleet_avoid_runs("avoids_rects", planners)
    got, _ = _avoids_query(planners, runs, [t[0] for t in tabs], [t[1] for t in tabs], [start] * n, max_wait,
                           (Engine.tree_clear_rects_multi, Engine.tree_clear_rects_wait_multi))
    return [None if run is None else p._avoid_end(run, g[0], g[1], g[2], start, adopt) for p, run, g in zip(planners, runs, got)]


def _avoids_connect(planners, runs, tables, radii, start, adopt, goal_tries):
    """avoids(connect=goal_tries) behind its checks: per group of _fleet_groups ONE query and, over the members with `adopt` and a
    winning chain, ONE commit; then every planner's own _avoid_connect_end."""
    results = [None] * len(planners)
    pick = lambda seq, ks: [seq[k] for k in ks]
    for mine in _fleet_groups(planners, runs):
        got = Engine.tree_clear_connect_multi([planners[k]._engine for k in mine], pick(tables, mine), pick(radii, mine),
                                              [start] * len(mine), [runs[k].H for k in mine], goal_tries, per_node=True)
        winners = [(k, g[1]["chain_from"]) for k, g in zip(mine, got) if adopt and g[1]["chain_from"] >= 0]
        new, failed = {}, None
        if winners:
            ids, failed = _fleet_commit(lambda: Engine.connect_commit_multi(
                [planners[k]._engine for k, _ in winners], [v for _, v in winners], [runs[k].H for k, _ in winners], goal_tries))
            new = {k: i for (k, _), i in zip(winners, ids)}         # (None: capacity, or a failed chain -- that tree is unchanged)
        for k, (out, chain, first, dwell) in zip(mine, got):
            results[k] = planners[k]._avoid_connect_end(runs[k], out, chain, first, dwell, start, adopt, new.get(k))
        if failed is not None:
            raise failed
    return results


def _deconflict_batched(planners, r, order, start, max_wait):
    """deconflict's loop as rounds of batched launches (_deconflict_rounds has the schedule and why it ends at the loop's answer).
    A candidate is (end node, wait) with its rows [:, :2]; on entry it is the plan the planner holds, and a planner without a clear
    hit keeps that one.  Adoption happens once, at the end, from the last answer of every planner -- which was given against the
    final candidates of those before it, and about the plan it held on entry.  Returns (results, rounds, native calls)."""
    n = len(planners)
    runs = _fleet_avoid_runs("deconflict", planners)
    held = [(int(p.node_seq[-1]) if getattr(p, "node_seq", None) else -1, int(getattr(p, "plan_wait", 0))) for p in planners]
    rows = [{held[k]: np.ascontiguousarray(np.asarray(p.x_seq, dtype=np.float64)[:, :2])} for k, p in enumerate(planners)]
    calls = [0]

    def rows_of(k, c):
        if c not in rows[k]:                                        # the tree path of the hit, `wait` rows of its first row in front
            p = planners[k]
            x = np.asarray(p.tree.trajectory(p.tree.climb(c[0]))[0], dtype=np.float64)[:, :2]
            rows[k][c] = np.ascontiguousarray(np.concatenate((np.repeat(x[:1], c[1], axis=0), x)))
        return rows[k][c]

    def ask(ks, cand):
        asked = [k for k in ks if runs[k] is not None]              # (a planner without a tree on the device keeps its plan)
        tables, radii = [None] * n, [None] * n
        for k in asked:
            before = order[:order.index(k)]
            tables[k], radii[k], _ = Engine.track_table([rows_of(j, cand[j]) for j in before], r[before], start)
        sub = [runs[k] if k in asked else None for k in range(n)]
        got, made = _avoids_query(planners, sub, tables, radii, [start] * n, max_wait)
        calls[0] += made
        out = []
        for k in ks:
            if got[k] is None:
                out.append((cand[k], None))
            else:
                best = got[k][0]
                out.append(((int(best["best_end"]), int(best.get("best_wait", 0))) if best["best_end"] >= 0 else held[k], got[k]))
        return out

    _, answers, log = _deconflict_rounds(order, held, ask)
    results = [None] * n
    for k in order[1:]:
        if answers[k] is not None:
            results[k] = planners[k]._avoid_end(runs[k], answers[k][0], answers[k][1], answers[k][2], start, True)
    return results, len(log), calls[0]
