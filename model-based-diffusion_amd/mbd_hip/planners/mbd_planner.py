"""Drop-in for mbd/planners/mbd_planner.py: same ``Args`` fields and defaults (:18-35), same
recommended-parameter overrides (:45-68), same RNG chain (:40,79,150,103), same return value (:182).

The reverse loop (:138-148) runs through libmbd_hip.so.  With ``torch.distributed`` initialised the N
candidates are sharded over ranks (one process per GPU): per diffusion step each rank rolls out its
shard, ONE all-gather (RCCL over xGMI) exchanges the N mean rewards, and every rank finishes the
step redundantly from identical inputs — results are bit-identical for every world size.
"""
from __future__ import annotations

import ctypes as C
import os
import time
from dataclasses import dataclass

import numpy as np

from .. import _capi
from ..envs import get_env
from ..envs.base import prng_impl


@dataclass
class Args:
    # exp
    seed: int = 0
    disable_recommended_params: bool = False
    not_render: bool = False
    # env
    env_name: str = "ant"  # in scope here: "car2d", "hopper", "halfcheetah", "humanoidrun", "humanoidtrack"
    # diffusion
    Nsample: int = 2048  # number of samples
    Hsample: int = 50  # horizon
    Ndiffuse: int = 100  # number of diffusion steps
    temp_sample: float = 0.1  # temperature for sampling
    beta0: float = 1e-4  # initial beta
    betaT: float = 1e-2  # final beta
    enable_demo: bool = False


# mbd_planner.py:45-63
TEMP_RECOMMEND = {"ant": 0.1, "halfcheetah": 0.4, "hopper": 0.1, "humanoidstandup": 0.1, "humanoidrun": 0.1,
                  "walker2d": 0.1, "pushT": 0.2}
NDIFFUSE_RECOMMEND = {"pushT": 200, "humanoidrun": 300}
NSAMPLE_RECOMMEND = {"humanoidrun": 8192}
HSAMPLE_RECOMMEND = {"pushT": 40}


def apply_recommended(args: Args) -> None:
    if not args.disable_recommended_params:  # mbd_planner.py:64-69
        args.temp_sample = TEMP_RECOMMEND.get(args.env_name, args.temp_sample)
        args.Ndiffuse = NDIFFUSE_RECOMMEND.get(args.env_name, args.Ndiffuse)
        args.Nsample = NSAMPLE_RECOMMEND.get(args.env_name, args.Nsample)
        args.Hsample = HSAMPLE_RECOMMEND.get(args.env_name, args.Hsample)
        print(f"override temp_sample to {args.temp_sample}")


class _Records:
    """The records a ``Plan`` and a ``Sweep`` both take, written once: ``_prefix`` is the C prefix of the handle's entries
    ("mbd_plan_" / "mbd_sweep_"), ``self.h`` the handle.  A sweep's record is one record for all its plans."""

    _prefix = None

    def _c(self, name):
        return getattr(self.lib, self._prefix + name)

    def _set(self, name, rec):
        _capi.check(self._c("set_" + name)(self.h, None if rec is None else C.byref(rec)))

    def set_mpc_pick(self, mean=True, prev=True, best=True):
        """Choose what a tick hands on (include/mbd_hip.h mbd_mpc_pick): of its mean, the incumbent (the last tick's plan shifted)
        and the best candidate of its last step — those enabled here — the one the plan's env values most.  The picked plan
        stands wherever the mean stood: the rows executed, the next tick's warm start, ``means``.  ``run_mpc`` then also returns
        ``pick`` = dict(choice [T], rets [T, 3], best [T]) (a sweep: one dict per episode); a session has ``pick`` after each
        collect.  ``mean`` alone leaves the episode's bits unchanged and logs the value of every executed plan."""
        self._set("mpc_pick", _capi.pick_record(mean, prev, best))

    def clear_mpc_pick(self):
        self._set("mpc_pick", None)

    def has_mpc_pick(self) -> bool:
        """Whether the handle carries a pick record: asked of the library, so a record set through the C ABI counts."""
        return _capi.has_mpc_pick(self._c("peek_mpc_pick"), self.h, self._pick_k)

    def set_mpc_demo(self, clip, start_row: int = 0, rew_xref: float = None):
        """Follow a demonstration on the episode's clock (include/mbd_hip.h mbd_mpc_demo; demo plans only): tick t of
        ``run_mpc`` plans under the 50 rows of ``clip`` [n_track, L, 3] (car2d: [L, 2]) from row
        ``start_row + (t + delay_ticks) * exec_steps`` on, rows past the clip's end holding its last row, with ``rew_xref``
        (None: the env's) as the demo's reward level.  ``run_mpc`` then also returns ``track_err`` [T*E, K] — the distance of
        every executed control step's tracked positions from its clip row — and ``demo_windows`` [T, K, 50, 3] (car2d: 2; a
        sweep: one clip and one clock, ``track_err`` [P, T*E, K]).  ``run`` ignores it."""
        rec, keep = _demo_record(self.env, clip, start_row, rew_xref)
        self._set("mpc_demo", rec)
        self._demo_shape = (keep.shape[0], keep.shape[2])
        del keep  # (the set call has copied the clip)

    def clear_mpc_demo(self):
        self._set("mpc_demo", None)
        self._demo_shape = None

    def set_mpc_delay(self, ticks: int, rows0=None):
        """Plan ahead of the plant (include/mbd_hip.h mbd_mpc_delay): a plan made in tick t of ``run_mpc`` is first executed in
        tick t + ``ticks`` (1..8).  Meanwhile the system executes the rows it is already committed to — ``rows0``
        [ticks * exec_steps, Nu] when the episode starts, None: zeros — and every tick plans from the state the plan's env
        predicts those rows will reach.  ``run_mpc`` then also returns ``predicted`` [T, state_size] (a sweep:
        [P, T, state_size]), and ``means[t]``'s row 0 belongs to control step (t + ticks) * exec_steps.  ``run`` ignores it."""
        rec, keep = _delay_record(ticks, rows0, self.Nu)
        self._set("mpc_delay", rec)
        self._has_delay = True
        del keep  # (the set call has copied the rows)

    def clear_mpc_delay(self):
        self._set("mpc_delay", None)
        self._has_delay = False

    def set_mpc_sigma(self, cold: float = 1.0, warm: float = 1.0, gain: float = 0.0):
        """Run a path-integral plan (``update_method`` 1 / 2 / 3: mppi, cma-es, cem) as a receding-horizon controller
        (include/mbd_hip.h mbd_mpc_sigma): ``run_mpc`` and ``mpc_open`` then accept the plan; a cold tick (tick 0; a session's
        tick after ``reset_mean``) starts from sigma ``cold``, every other tick from ``warm`` — or, with ``gain`` > 0 (cma-es
        only, ``warm`` <= ``cold``), from clamp(gain * the sigma the last tick ended with, warm, cold).  ``run_mpc`` then also
        returns ``sigmas`` [T, 2] (a sweep: [P, T, 2]): what every tick started from and ended with.  ``run`` ignores it.
        Sessions of path-integral sweeps stay refused."""
        self._set("mpc_sigma", _sigma_record(cold, warm, gain))
        self._has_sigma = True

    def clear_mpc_sigma(self):
        self._set("mpc_sigma", None)
        self._has_sigma = False

    def set_noise_shape(self, scale, when: str = "always"):
        """Shape the sampling noise per horizon row and actuator (include/mbd_hip.h mbd_noise_shape): ``scale`` [H, Nu] (or
        anything that broadcasts to it) of finite values >= 0; a candidate is clip((eps * scale) * sigma_i + Ybar_i).
        ``when``: "always" — every diffusion step of every call that samples — or "warm": only the ticks t >= 1 of
        ``run_mpc`` (``mpc.tail_shape`` gives the rows a warm tick has just appended the noise a cold plan starts with).  All
        ones is no shape, bit for bit; zeros freeze their elements at clip(Ybar_i)."""
        rec, keep = _noise_record(scale, when, self.H, self.Nu)
        self._set("noise_shape", rec)
        del keep  # (the set call has copied the table)

    def clear_noise_shape(self):
        self._set("noise_shape", None)

    def set_noise_basis(self, W, when: str = "always"):
        """Correlate the sampling noise along the horizon (include/mbd_hip.h mbd_noise_basis): ``W`` [H, n_knots] of finite
        values, n_knots <= 16; a step then draws normal(key, (N, n_knots, Nu)) and a candidate is
        clip(((sum_k W[h, k] eps[n, k, a]) * shape) * sigma_i + Ybar_i) (``mpc.knot_basis`` builds interpolation and hold
        tables).  ``when`` as ``set_noise_shape``'s, independently of the shape's.  None clears."""
        rec, keep = (None, None) if W is None else _basis_record(W, when, self.H)
        self._set("noise_basis", rec)
        del keep  # (the set call has copied the table)

    def set_objective(self, row_weight=None, effort: float = 0.0, rate: float = 0.0, act_weight=None, prev0=None):
        """Shape what the plan maximises (include/mbd_hip.h mbd_objective): a candidate's reward becomes
        sum_h w[h] r[h] / sum(w) - (1 / H) sum_a q[a] (effort * sum_h u^2 + rate * sum_h (u[h] - u[h-1])^2) with ``row_weight`` w
        [H] (None: the plain mean; ``mpc.discount_weights`` builds a discount with a terminal weight), ``act_weight`` q [Nu] (None:
        ones) and u[-1] the action executed before the plan begins — ``prev0`` [Nu] (None: the first term is left out; a sweep:
        every plan's) for ``run`` and the first tick of an episode, the last committed row afterwards.  Every call that samples
        reads it; ``eval``, the final reward and an episode's reward log keep the env's own rewards."""
        rec, keep = _objective_record(row_weight, effort, rate, act_weight, prev0, self.H, self.Nu)
        self._set("objective", rec)
        del keep  # (the set call has copied the tables)

    def clear_objective(self):
        self._set("objective", None)

    def set_value(self, net, scale: float = None):
        """Score every candidate's end state with a terminal value net (include/mbd_hip.h mbd_value): ``net`` is a
        ``planners.value.ValueNet`` over the env's state record, and a candidate's reward becomes its reward without the record
        plus ``scale`` * V(final state) (``scale`` None: the net's own; ``value.terminal_scale(weight, Hsample)`` weighs V like
        ``weight`` further rows).  Every call that samples reads it; ``eval``, the final reward and an episode's reward log keep the
        env's own rewards.  None clears."""
        self._set("value", None if net is None else net.record(scale))  # (the set call has copied the net)

    def set_weighting(self, reject_nonfinite=True, ess_frac: float = 0.0, temp_min=None, temp_max=None, iters: int = 12):
        """Weigh the candidates robustly (include/mbd_hip.h mbd_weighting): with ``reject_nonfinite`` a candidate whose reward is
        NaN or infinite gets weight 0 and leaves the step's statistics, so one diverged rollout no longer turns the plan's mean
        into NaN; with ``ess_frac`` in (0, 1] every step chooses its softmax temperature inside [``temp_min``, ``temp_max``] by
        ``iters`` bisection steps so that the effective sample size of the weights is about ``ess_frac`` times the candidates
        kept (0: the plan's ``temp_sample``; a sweep: each plan at its own temperature).  Not for plans created with
        ``enable_demo``."""
        self._set("weighting", _capi.weighting_record(reject_nonfinite, ess_frac, temp_min, temp_max, iters))

    def clear_weighting(self):
        self._set("weighting", None)

    def set_elites(self, n_elites: int, nominal=False, carry=False):
        """Carry a step's best candidates into the next step (include/mbd_hip.h mbd_elites): the ``n_elites`` best candidates of
        every diffusion step (0 to 32, by the rewards its score read) overwrite the next step's first candidates; ``nominal``:
        candidate 0 of every step is the step's mean itself, noise-free; ``carry``: a tick boundary shifts the elites with the mean
        (False: every tick starts without elites).  MBD and mppi plans, unsharded, without ``enable_demo``.  A sweep's plans each
        have their own elites, count and log."""
        self._set("elites", _capi.elites_record(n_elites, nominal, carry))
        self._elites = int(n_elites)

    def clear_elites(self):
        self._set("elites", None)
        self._elites = None

    @property
    def has_elites(self) -> bool:
        return getattr(self, "_elites", None) is not None

    def set_togo(self, block: int = 1, min_tail: int = 1):
        """Weigh each horizon row by the return still ahead of it (include/mbd_hip.h mbd_togo): the rows fall into groups of
        ``block``, a group starting only where at least ``min_tail`` rows are still ahead, and group j's rows are the step's update
        under weights from the candidates' mean reward from the group's first row onwards (a sweep: each plan under its own
        temperature).  MBD and mppi plans, unsharded, without ``enable_demo``, at most 12288 candidates, and without an objective,
        value, weighting, adapt or ensemble record."""
        self._set("togo", _capi.togo_record(block, min_tail))
        self._togo = (int(block), int(min_tail))

    def clear_togo(self):
        self._set("togo", None)
        self._togo = None

    @property
    def has_togo(self) -> bool:
        return getattr(self, "_togo", None) is not None

    def _put_zones(self, call, zones):
        zones = list(zones)
        _capi.check(self._c(call)(self.h, C.byref(_zones_record(self.env, zones))))
        self._zones = len(zones)
        self._zone_entries = zones

    def set_zones(self, zones):
        """Keep-out regions and goals for the env's tracked links (include/mbd_hip.h mbd_zones): ``zones`` is a list of
        ``mpc.zone`` entries.  Every step subtracts from each candidate's reward the mean over the horizon of the entries'
        penalties at the tracked positions its rollout passed through.  The env must track links (``get_env(name, track=...)``);
        unsharded plans without ``enable_demo`` and without an ensemble, to-go or pick record.  ``run_mpc`` then also returns
        ``zone_pen`` and ``zone_clear`` [T*E] (a sweep: [P, T*E]): the penalty and the keep-out clearance of every executed
        control step."""
        self._put_zones("set_zones", zones)

    def clear_zones(self):
        self._set("zones", None)
        self._zones = None

    @property
    def has_zones(self) -> bool:
        return getattr(self, "_zones", None) is not None

    def update_zones(self, zones):
        """Replace the table of the handle's zone record — move a goal or an obstacle.  Allowed between the ticks of an open
        session (``MpcSession.update_zones``); the next step plans under the new table."""
        self._put_zones("update_zones", zones)


class Sweep(_Records):
    """Owner of an ``mbd_sweep`` handle: several plans of one env (same sizes and schedule; seeds, start states and
    temperatures may differ) advanced in lockstep — ONE rollout launch over all their candidates and ONE score launch per
    diffusion step (mbd/scripts/run_mbd.py:17-64).  Every plan's result is bit-identical to ``Plan.run`` on its own.
    ``update_method``: 0 MBD plans; 1 / 2 / 3 the path-integral baselines mppi / cma-es / cem (``args`` is then a
    path_integral.Args: Nrefine plays Ndiffuse).  A record set on the sweep is one record for all its plans, and the guarantee
    holds under every one of them: plan k of ``run``, episode k of ``run_mpc`` and of a session, is the single plan's with the
    same record, bit for bit."""

    _prefix, _pick_k = "mbd_sweep_", 0

    def __init__(self, env, args, n_plans: int, temps=None, literal_score: bool = True, update_method: int = 0):
        self.lib = _capi.load()
        self.env = env
        cfg = _capi.PlanConfig()
        cfg.Nsample, cfg.Hsample = args.Nsample, args.Hsample
        cfg.Ndiffuse = getattr(args, "Ndiffuse", None) or args.Nrefine  # path_integral.Args calls it Nrefine
        cfg.temp_sample = args.temp_sample
        cfg.beta0, cfg.betaT = getattr(args, "beta0", 1e-4), getattr(args, "betaT", 1e-2)
        cfg.enable_demo = int(getattr(args, "enable_demo", False))
        cfg.update_method = int(update_method)
        cfg.prng_impl = prng_impl()
        cfg.shard_begin, cfg.shard_count = 0, args.Nsample
        cfg.literal_score = int(literal_score)
        self.cfg, self.P = cfg, int(n_plans)
        t = None if temps is None else np.ascontiguousarray(temps, np.float32).reshape(self.P)
        h = C.c_void_p()
        _capi.check(self.lib.mbd_sweep_create(env.handle, C.byref(cfg), self.P, None if t is None else _capi.np_ptr(t),
                                              C.byref(h)))
        self.h = h
        self.Nd, self.H, self.Nu = cfg.Ndiffuse, args.Hsample, env.action_size
        self._plant_envs = {}  # episode -> the plant env of its record (kept alive: a record does not own its plant)
        self._has_delay = False
        self._has_sigma = False
        self._demo_shape = None  # (K, C) of the clip of the sweep's demo record

    def set_state0(self, k: int, state):
        st = np.ascontiguousarray(state.pipeline_state, np.float32).reshape(-1)
        _capi.check(self.lib.mbd_sweep_set_state0(self.h, int(k), _capi.np_ptr(st)))

    def run(self, keys, outputs: bool = True):
        """keys [P, 2] = rng_exp of every plan.  Returns (mu_0ts [P, Nd-1, H, Nu], rew_means [P, Nd-1], rew_final [P],
        seconds of the lockstep loop).  ``outputs=False``: the lockstep loop only — no host copies, no final evaluation
        (timing runs); the three arrays are then None."""
        k = np.ascontiguousarray(keys, np.uint32).reshape(self.P, 2)
        secs = C.c_double()
        if not outputs:
            _capi.check(self.lib.mbd_sweep_run(self.h, _capi.np_ptr(k), None, None, None, C.byref(secs)))
            return None, None, None, secs.value
        mu = np.zeros((self.P, self.Nd - 1, self.H, self.Nu), np.float32)
        rm = np.zeros((self.P, self.Nd - 1), np.float32)
        rf = np.zeros(self.P, np.float32)
        _capi.check(self.lib.mbd_sweep_run(self.h, _capi.np_ptr(k), _capi.np_ptr(mu), _capi.np_ptr(rm), _capi.np_ptr(rf),
                                           C.byref(secs)))
        return mu, rm, rf, secs.value

    def run_mpc(self, keys, n_ticks: int, warm_steps: int, exec_steps: int = 1) -> dict:
        """P closed-loop episodes in lockstep (include/mbd_hip.h mbd_sweep_run_mpc): episode k is ``Plan.run_mpc`` from plan
        k's state0 with ``keys[k]`` and plan k's temperature, bit for bit; a diffusion step of a tick is one rollout launch
        over all the episodes' candidates.  Returns dict(actions [P, T*E, Nu], rewards [P, T*E], states [P, T+1, state_size],
        means [P, T, H, Nu], seconds)."""
        mc = _capi.MpcConfig()
        mc.n_ticks, mc.warm_steps, mc.exec_steps = int(n_ticks), int(warm_steps), int(exec_steps)
        T, E, P = max(mc.n_ticks, 0), max(mc.exec_steps, 0), self.P
        S = self.env._state_size
        k = np.ascontiguousarray(keys, np.uint32).reshape(P, 2)
        out = dict(actions=np.zeros((P, T * E, self.Nu), np.float32), rewards=np.zeros((P, T * E), np.float32),
                   states=np.zeros((P, T + 1, S), np.float32), means=np.zeros((P, T, self.H, self.Nu), np.float32))
        secs = C.c_double()
        _capi.check(self.lib.mbd_sweep_run_mpc(self.h, C.byref(mc), _capi.np_ptr(k), _capi.np_ptr(out["actions"]),
                                               _capi.np_ptr(out["rewards"]), _capi.np_ptr(out["states"]),
                                               _capi.np_ptr(out["means"]), C.byref(secs)))
        out["seconds"] = secs.value
        if self._has_delay:  # (the states the ticks planned from: shat_{k,0} .. shat_{k,T-1})
            out["predicted"] = np.zeros((P, T, S), np.float32)
            _capi.check(self.lib.mbd_sweep_peek_mpc_predicted(self.h, _capi.np_ptr(out["predicted"])))
        if self._has_sigma:  # (the sigma every tick of every episode started from and ended with)
            out["sigmas"] = np.zeros((P, T, 2), np.float32)
            for e in range(P):
                _capi.check(self.lib.mbd_sweep_peek_mpc_sigma(self.h, e, _capi.np_ptr(out["sigmas"][e])))
        if self._demo_shape is not None:  # (every episode's distances from the clip, and the one table of windows)
            Kt, Cc = self._demo_shape
            out["track_err"] = np.zeros((P, T * E, Kt), np.float32)
            out["demo_windows"] = np.zeros((T, Kt, _capi.XREF_ROWS, Cc), np.float32)
            for e in range(P):
                _capi.check(self.lib.mbd_sweep_peek_mpc_track(self.h, e, _capi.np_ptr(out["track_err"][e]),
                                                              _capi.np_ptr(out["demo_windows"]) if e == 0 else None))
        if self.has_mpc_pick():  # (what every tick of every episode handed on, and the three plans' values)
            out["pick"] = [self.peek_mpc_pick(e, T) for e in range(P)]
        if self.has_zones:  # (every episode's penalties and keep-out clearances of its executed control steps)
            out["zone_pen"], out["zone_clear"] = np.zeros((P, T * E), np.float32), np.zeros((P, T * E), np.float32)
            for e in range(P):
                _capi.check(self.lib.mbd_sweep_peek_mpc_zones(self.h, e, _capi.np_ptr(out["zone_pen"][e]),
                                                              _capi.np_ptr(out["zone_clear"][e])))
        return out

    def mpc_open(self, keys, warm_steps: int, exec_steps: int = 1, max_ticks: int = None):
        """Open P sessions in lockstep (include/mbd_hip.h mbd_sweep_mpc_open; ``MpcSession``): episode k is ``Plan.mpc_open``'s
        session with ``keys[k]`` and plan k's temperature, bit for bit, whatever the other episodes are fed.  A tick takes the
        episodes' states [P, state_size]; ``reset_mean(k)`` makes episode k's next tick a cold one."""
        return MpcSession(self, keys, warm_steps, exec_steps, max_ticks)

    def set_mpc_plant(self, k: int, env=None, key=None, act_std: float = 0.0, kick_std: float = 0.0, kick_every: int = 1):
        """The plant of episode ``k`` (``Plan.set_mpc_plant``): episode k of ``run_mpc`` is then ``Plan.run_mpc`` with that
        record, bit for bit.  Episodes may carry different plants, keys and stds, or none; consecutive episodes that share
        a plant env are executed in one launch.  The sweep keeps a reference to ``env``."""
        rec = _plant_record(env, key, act_std, kick_std, kick_every)
        _capi.check(self.lib.mbd_sweep_set_mpc_plant(self.h, int(k), C.byref(rec)))
        self._plant_envs[int(k)] = env

    def clear_mpc_plant(self, k: int):
        _capi.check(self.lib.mbd_sweep_set_mpc_plant(self.h, int(k), None))
        self._plant_envs.pop(int(k), None)

    def peek_weighting(self, k: int) -> dict:
        """Plan k's ``temp``, ``ess`` and ``kept`` of every score step of the last run or tick (``Plan.peek_weighting``)."""
        return _capi.peek_weighting(self.lib.mbd_sweep_peek_weighting, self.h, k, self.cfg.Ndiffuse - 1)

    def peek_elites(self, k: int, capacity: int = None) -> dict:
        """Plan k's ``E`` [count, H, Nu], ``R``, ``src``, ``count`` and log (``Plan.peek_elites``)."""
        fn = lambda h, *a: self.lib.mbd_sweep_peek_elites(h, int(k), *a)  # noqa: E731
        if not self.has_elites:
            _capi.check(fn(self.h, None, None, None, None, None, None, None, 0, None))
        out = _capi.peek_elites(fn, self.h, self._elites or 0, self.H * self.Nu, capacity)
        out["E"] = out["E"].reshape(-1, self.H, self.Nu)
        return out

    def peek_togo(self, k: int) -> dict:
        """Plan k's ``starts`` [G], ``R`` and ``W`` [G, Nsample] of the last step (``Plan.peek_togo``)."""
        fn = lambda h, *a: self.lib.mbd_sweep_peek_togo(h, int(k), *a)  # noqa: E731
        if not self.has_togo:
            _capi.check(fn(self.h, None, None, None, None))
        return _capi.peek_togo(fn, self.h, self.H, self.cfg.Nsample)

    def peek_zones(self, k: int) -> dict:
        """Plan ``k``'s ``pen`` and ``clr`` [Nsample] of the last step (``Plan.peek_zones``)."""
        if not self.has_zones:
            _capi.check(self.lib.mbd_sweep_peek_zones(self.h, int(k), None, None))
        return _capi.peek_zones(self.lib.mbd_sweep_peek_zones, self.h, int(k), self.cfg.Nsample)

    def peek_mpc_pick(self, k: int, capacity: int = None) -> dict:
        """Episode k's ``choice`` [n], ``rets`` [n, 3] and ``best`` [n] of the ticks served so far (``Plan.peek_mpc_pick``)."""
        return _capi.peek_mpc_pick(self.lib.mbd_sweep_peek_mpc_pick, self.h, k, capacity)

    def peek_objective(self, k: int):
        """Plan k's ``ret`` [N] and ``cost`` [N] of the last step (a sweep with an objective record)."""
        N = self.cfg.Nsample
        ret, cost = np.zeros(N, np.float32), np.zeros(N, np.float32)
        _capi.check(self.lib.mbd_sweep_peek_objective(self.h, int(k), _capi.np_ptr(ret), _capi.np_ptr(cost)))
        return ret, cost

    def get_sigmas(self):
        """path-integral sweeps: every plan's carried sigma after the last run (path_integral.py:113,131)."""
        out = np.zeros(self.P, np.float32)
        _capi.check(self.lib.mbd_sweep_get_sigmas(self.h, _capi.np_ptr(out)))
        return out

    def kernel_time(self, enable=True):
        ms, n = C.c_float(), C.c_int()
        _capi.check(self.lib.mbd_sweep_kernel_time(self.h, int(enable), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def close(self):
        if self.h is not None:
            self.lib.mbd_sweep_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _sigma_record(cold, warm, gain):
    """The mbd_mpc_sigma of ``set_mpc_sigma``'s arguments."""
    rec = _capi.MpcSigma()
    rec.sigma_cold, rec.sigma_warm, rec.gain = float(cold), float(warm), float(gain)
    return rec


def _plant_record(env, key, act_std, kick_std, kick_every):
    """The mbd_mpc_plant of ``set_mpc_plant``'s arguments (``key`` None: the key of seed 0)."""
    rec = _capi.MpcPlant()
    rec.plant = None if env is None else env.handle
    k = np.ascontiguousarray(_capi.prng_key(0) if key is None else key, np.uint32).reshape(2)
    rec.key[0], rec.key[1] = int(k[0]), int(k[1])
    rec.act_std, rec.kick_std, rec.kick_every = float(act_std), float(kick_std), int(kick_every)
    return rec


def _demo_record(env, clip, start_row, rew_xref):
    """The mbd_mpc_demo of ``set_mpc_demo``'s arguments, and the float32 array [K, L, C] its pointer reads (``clip``
    [n_track, L, 3]; car2d: [L, 2]; ``rew_xref`` None: the env's; everything else goes to the library, which names the field)."""
    c = np.ascontiguousarray(clip, np.float32)
    if c.ndim == 2:  # (car2d: one track)
        c = c[None]
    # (an env without tracked links has no demo at all: the library refuses the record before it reads the clip)
    want = (1, 2) if getattr(env, "sys", None) is None else (max(int(env.sys.fields["n_track"]), 1), 3)
    if c.ndim != 3 or (c.shape[0], c.shape[2]) != want:
        raise ValueError(f"demo clip of shape {np.shape(clip)}: must be [n_track={want[0]}, n_rows, {want[1]}]"
                         + (" or [n_rows, 2]" if want[1] == 2 else ""))
    rec = _capi.MpcDemo()
    rec.clip = c.ctypes.data_as(C.POINTER(C.c_float))
    rec.n_rows, rec.start_row = c.shape[1], int(start_row)
    rec.rew_xref = float(env.rew_xref if rew_xref is None else rew_xref)
    return rec, c


def _delay_record(ticks, rows0, Nu):
    """The mbd_mpc_delay of ``set_mpc_delay``'s arguments, and the float32 array its pointer reads (``rows0`` [n_rows, Nu], or
    None: zeros; rows of another count or with non-finite values go to the library, which names the field)."""
    rec = _capi.MpcDelay()
    rec.delay_ticks = int(ticks)
    r = None
    if rows0 is not None:
        r = np.ascontiguousarray(rows0, np.float32).reshape(-1, Nu)
        rec.rows0 = r.ctypes.data_as(C.POINTER(C.c_float))
        rec.n_rows = r.shape[0]
    return rec, r


def _noise_record(scale, when, H, Nu):
    """The mbd_noise_shape of ``set_noise_shape``'s arguments, and the float32 array its pointer reads (``scale`` [H, Nu], or
    anything that broadcasts to it: a column [H, 1] is a horizon-row schedule, a row [Nu] a per-actuator one)."""
    if when not in _capi.NOISE_WHEN:
        raise ValueError(f"when={when!r}: one of {sorted(_capi.NOISE_WHEN)}")
    g = np.asarray(scale, np.float32)
    if g.ndim < 2 or g.shape[-2:] != (H, Nu):  # (a full table of another size goes to the library, which names the field)
        g = np.broadcast_to(g, (H, Nu))
    g = np.ascontiguousarray(g, np.float32)
    rec = _capi.NoiseShape()
    rec.scale = g.ctypes.data_as(C.POINTER(C.c_float))
    rec.rows, rec.cols, rec.when = g.shape[0], g.shape[1], _capi.NOISE_WHEN[when]
    return rec, g


def _basis_record(W, when, H):
    """The mbd_noise_basis of ``set_noise_basis``'s arguments, and the float32 array its pointer reads (``W`` [H, n_knots]; a
    table of another size or with non-finite values goes to the library, which names the field)."""
    if when not in _capi.NOISE_WHEN:
        raise ValueError(f"when={when!r}: one of {sorted(_capi.NOISE_WHEN)}")
    W = np.ascontiguousarray(W, np.float32)
    if W.ndim != 2 or W.shape[0] != H:
        raise ValueError(f"noise basis of shape {W.shape}: must be [Hsample={H}, n_knots]")
    rec = _capi.NoiseBasis()
    rec.basis = W.ctypes.data_as(C.POINTER(C.c_float))
    rec.n_knots, rec.when = W.shape[1], _capi.NOISE_WHEN[when]
    return rec, W


def _objective_record(row_weight, effort, rate, act_weight, prev0, H, Nu):
    """The mbd_objective of ``set_objective``'s arguments, and the float32 arrays its pointers read (tables of another length
    or with refused values go to the library, which names the field)."""
    rec = _capi.Objective()
    keep = []
    for field, x in (("row_weight", row_weight), ("act_weight", act_weight), ("prev0", prev0)):
        if x is not None:
            a = np.ascontiguousarray(x, np.float32).reshape(-1)
            setattr(rec, field, a.ctypes.data_as(C.POINTER(C.c_float)))
            keep.append(a)
    rec.effort, rec.rate = float(effort), float(rate)
    rec.rows = H if row_weight is None else keep[0].size
    rec.cols = Nu
    for x in (act_weight, prev0):
        if x is not None:
            rec.cols = int(np.size(x))
    return rec, keep


def _zones_record(env, zones):
    """The mbd_zones of a list of ``mpc.zone`` entries against ``env``'s track slots (link names resolve to slots)."""
    sys_ = getattr(env, "sys", None)
    K = int(sys_.fields["n_track"]) if sys_ is not None else 0
    names = None
    if sys_ is not None and sys_.link_names:
        names = [sys_.link_names[int(l)] for l in np.asarray(sys_.fields["track_link"])[:K]]
    return _capi.zones_record(zones, K, names)


def _ensemble_record(envs, risk):
    """The mbd_ensemble of ``set_ensemble``'s arguments (an entry None: the plan's own env)."""
    envs = list(envs)
    if risk not in _capi.RISKS:
        raise ValueError(f"risk={risk!r}: one of {sorted(_capi.RISKS)}")
    if not 1 <= len(envs) <= _capi.MAX_ENSEMBLE:
        raise ValueError(f"an ensemble has 1..{_capi.MAX_ENSEMBLE} members, not {len(envs)}")
    rec = _capi.Ensemble()
    for m, e in enumerate(envs):
        rec.members[m] = None if e is None else e.handle
    rec.n_members, rec.risk = len(envs), _capi.RISKS[risk]
    return rec


class MpcSession:
    """An episode the caller drives (include/mbd_hip.h mbd_plan_mpc_open): opened once by ``Plan.mpc_open``, advanced one tick
    per ``tick`` from the state of a system the library does not own — the caller is the plant.  A context manager; ``close``
    (or leaving the block) gives the plan back to its other calls.  Fed the states of ``Plan.run_mpc`` it returns that
    episode's means and rows bit for bit.  Opened by ``Sweep.mpc_open`` it is P such sessions in lockstep
    (mbd_sweep_mpc_open): ``key`` is then ``keys`` [P, 2], a tick takes states [P, state_size] (or q [P, n_q], qd [P, n_qd]), every
    array it returns has a leading episode axis, ``flags`` and ``rew_mean`` are arrays [P], and ``reset_mean`` takes the episode."""

    def __init__(self, plan, key, warm_steps: int, exec_steps: int = 1, max_ticks: int = None):
        for name, v in (("warm_steps", warm_steps), ("exec_steps", exec_steps)) + ((("max_ticks", max_ticks),) if max_ticks is not None else ()):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"{name}={v!r}: an int")
        if not 1 <= warm_steps <= plan.Nd - 1:
            raise ValueError(f"warm_steps={warm_steps} outside [1, Ndiffuse-1={plan.Nd - 1}]")
        if not 1 <= exec_steps < plan.H:
            raise ValueError(f"exec_steps={exec_steps} outside [1, Hsample={plan.H})")
        if max_ticks is not None and not 1 <= max_ticks <= 2 ** 31 - 1:
            raise ValueError(f"max_ticks={max_ticks} outside [1, 2^31-1]")
        self.P = getattr(plan, "P", None)  # (a sweep's episodes; None: a plan)
        k = np.ascontiguousarray(key, np.uint32)
        if k.size != 2 * (self.P or 1):
            raise ValueError(f"key of shape {k.shape}: " + ("two uint32 words" if self.P is None else f"[{self.P}, 2] uint32 words"))
        self.plan, self.lib = plan, plan.lib
        self.E, self.S = int(exec_steps), plan.env._state_size
        self._call = "mbd_plan_mpc_" if self.P is None else "mbd_sweep_mpc_"
        mc = _capi.MpcConfig()
        mc.n_ticks = 2 ** 31 - 1 if max_ticks is None else int(max_ticks)
        mc.warm_steps, mc.exec_steps = int(warm_steps), int(exec_steps)
        self._open = False
        self._pick, self._pick_tick = None, -1  # (the last collected tick's pick entry, fetched when ``pick`` is first read)
        self._ticks = 0
        _capi.check(self._fn("open")(plan.h, C.byref(mc), _capi.key_array(key) if self.P is None else _capi.np_ptr(k)))
        self._open = True

    def _fn(self, what):
        return getattr(self.lib, self._call + what)

    def _state(self, state, q, qd):
        if (state is None) == (q is None):
            raise ValueError("a tick takes a state, or generalized coordinates q (and qd): one of the two")
        if state is not None and qd is not None:
            raise ValueError("qd goes with q, not with a state")
        n = self.P or 1
        if state is None:
            init = self.plan.env.pipeline_init
            if self.P is None:
                state = init(q, qd)
            else:
                state = np.stack([np.asarray(init(q[k], None if qd is None else qd[k]), np.float32).reshape(-1) for k in range(n)])
        elif self.P is not None and not isinstance(state, np.ndarray):
            state = np.stack([np.asarray(getattr(x, "pipeline_state", x), np.float32).reshape(-1) for x in state])
        st = np.ascontiguousarray(getattr(state, "pipeline_state", state), np.float32).reshape(-1)
        if st.size != n * self.S:
            raise ValueError(f"a state of {st.size} floats: the env's state_size is {self.S}" + ("" if self.P is None else f", times {n} episodes"))
        return st

    def submit(self, state=None, q=None, qd=None) -> None:
        """Enqueue the next tick from ``state`` (a State, or its pipeline state as an array [state_size]) or from generalized
        coordinates ``q`` (and ``qd``; through ``env.pipeline_init``) and return; ``collect`` waits for it."""
        st = self._state(state, q, qd)
        _capi.check(self._fn("submit")(self.plan.h, _capi.np_ptr(st)))

    def collect(self) -> dict:
        """The tick in flight: dict(rows [E, Nu] — the plan's first rows, unclipped —, mean [H, Nu], head [E, Nu] — with a delay
        record the rows to execute NOW, rows being due in ``delay_ticks`` ticks; otherwise rows again —, predicted [state_size]
        — the state the tick planned from under a delay record, else None —, flags, rew_mean, seconds, tick)."""
        p = self.plan
        lead = () if self.P is None else (self.P,)
        rows, head = (np.zeros(lead + (self.E, p.Nu), np.float32) for _ in range(2))
        mean, pred = np.zeros(lead + (p.H, p.Nu), np.float32), np.zeros(lead + (self.S,), np.float32)
        info = (_capi.MpcTickInfo * (self.P or 1))()
        _capi.check(self._fn("collect")(p.h, _capi.np_ptr(rows), _capi.np_ptr(mean), _capi.np_ptr(head), _capi.np_ptr(pred), info))
        flags, rew = np.array([i.flags for i in info], np.int32), np.array([i.rew_mean for i in info], np.float32)
        self._ticks += 1
        return dict(rows=rows, mean=mean, head=head, predicted=pred if p._has_delay else None,
                    flags=int(flags[0]) if self.P is None else flags, rew_mean=float(rew[0]) if self.P is None else rew,
                    seconds=info[0].seconds, tick=info[0].tick)

    @property
    def pick(self):
        """With a pick record: what the last collected tick handed on — dict(choice, rets [3], best); a sweep's session: arrays [P],
        [P, 3], [P].  None without a record or before the first collect.  Read from the device log when asked for (one peek per
        tick at the most), so a loop that never looks pays nothing."""
        p = self.plan
        if self._ticks == 0 or not p.has_mpc_pick():
            return None
        if self._pick_tick != self._ticks:
            if self.P is None:
                last = p.peek_mpc_pick(1)
                self._pick = dict(choice=int(last["choice"][0]), rets=last["rets"][0], best=int(last["best"][0]))
            else:
                last = [p.peek_mpc_pick(e, 1) for e in range(self.P)]
                self._pick = dict(choice=np.array([x["choice"][0] for x in last], np.int32), rets=np.stack([x["rets"][0] for x in last]),
                                  best=np.array([x["best"][0] for x in last], np.int32))
            self._pick_tick = self._ticks
        return self._pick

    def tick(self, state=None, q=None, qd=None) -> dict:
        """``submit`` then ``collect``."""
        self.submit(state, q, qd)
        return self.collect()

    def update_zones(self, zones) -> None:
        """Replace the table of the handle's zone record between two ticks (``Plan.update_zones``): the next tick plans under it.
        Refused while a tick is in flight."""
        self.plan.update_zones(zones)

    def reset_mean(self, k: int = None) -> None:
        """The next tick is a cold one (Ybar = 0, Ndiffuse-1 steps, flagged TICK_COLD): what a controller does after rows it
        could not use.  The delay queue stays.  A sweep's session: episode ``k``'s (None: every episode's)."""
        if self.P is None:
            _capi.check(self._fn("reset_mean")(self.plan.h))
            return
        for e in range(self.P) if k is None else (int(k),):
            _capi.check(self._fn("reset_mean")(self.plan.h, e))

    def close(self) -> None:
        if self._open and self.plan.h is not None:
            self._open = False
            _capi.check(self._fn("close")(self.plan.h))
        self._open = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Plan(_Records):
    """Thin owner of an ``mbd_plan`` handle."""

    _prefix, _pick_k = "mbd_plan_", None

    def __init__(self, env, args, shard_begin: int = 0, shard_count: int = None, literal_score: bool = True,
                 update_method: int = 0, shares_device: bool = False):
        self.lib = _capi.load()
        self.env = env
        cfg = _capi.PlanConfig()
        cfg.Nsample, cfg.Hsample = args.Nsample, args.Hsample
        cfg.Ndiffuse = getattr(args, "Ndiffuse", None) or args.Nrefine  # path_integral.Args calls it Nrefine
        cfg.temp_sample = args.temp_sample
        cfg.beta0, cfg.betaT = getattr(args, "beta0", 1e-4), getattr(args, "betaT", 1e-2)
        cfg.enable_demo = int(getattr(args, "enable_demo", False))
        cfg.update_method = update_method
        cfg.prng_impl = prng_impl()
        cfg.shard_begin = shard_begin
        cfg.shard_count = args.Nsample if shard_count is None else shard_count
        cfg.literal_score = int(literal_score)
        cfg.shares_device = int(shares_device)  # other plans run on this GPU at the same time (concurrent sweeps)
        self.cfg = cfg
        h = C.c_void_p()
        _capi.check(self.lib.mbd_plan_create(env.handle, C.byref(cfg), C.byref(h)))
        self.h = h
        self.Nd, self.H, self.Nu = cfg.Ndiffuse, args.Hsample, env.action_size
        self._plant_env = None  # the plant env of the plan's record (kept alive: a record does not own its plant)
        self._ens_envs = None   # the member envs of the plan's ensemble record (kept alive likewise)
        self._has_delay = False
        self._has_sigma = False
        self._demo_shape = None  # (K, C) of the clip of the plan's demo record

    def schedule(self):
        a, ab, s = (np.zeros(self.Nd, np.float32) for _ in range(3))
        _capi.check(self.lib.mbd_plan_schedule(self.h, _capi.np_ptr(a), _capi.np_ptr(ab), _capi.np_ptr(s)))
        return a, ab, s

    def set_state0(self, state):
        st = np.ascontiguousarray(state.pipeline_state, np.float32).reshape(-1)
        _capi.check(self.lib.mbd_plan_set_state0(self.h, _capi.np_ptr(st)))

    def enable_timing(self, on=True):
        _capi.check(self.lib.mbd_plan_enable_timing(self.h, int(on)))

    def kernel_time(self, reset=True):
        ms, n = C.c_float(), C.c_int()
        _capi.check(self.lib.mbd_plan_kernel_time(self.h, C.byref(ms), C.byref(n), int(reset)))
        return ms.value, n.value

    def run(self, key):
        """Whole reverse loop on one GPU. Returns (mu_0ts [Nd-1,H,Nu], rew_means [Nd-1], rew_final, secs)."""
        mu = np.zeros((self.Nd - 1, self.H, self.Nu), np.float32)
        rm = np.zeros(self.Nd - 1, np.float32)
        rf, secs = C.c_float(), C.c_double()
        _capi.check(self.lib.mbd_plan_run(self.h, _capi.key_array(key), _capi.np_ptr(mu), _capi.np_ptr(rm),
                                          C.byref(rf), C.byref(secs)))
        return mu, rm, rf.value, secs.value

    def run_mpc(self, key, n_ticks: int, warm_steps: int, exec_steps: int = 1) -> dict:
        """Closed-loop episode from the plan's state0 (include/mbd_hip.h mbd_plan_run_mpc): every tick replans from the
        state reached, warm-started from the previous tick's mean shifted by ``exec_steps`` and diffused over steps
        ``warm_steps``..1 (tick 0: a cold plan from ``key``'s first split), then executes its first ``exec_steps`` rows.
        Returns dict(actions [T*E, Nu], rewards [T*E], states [T+1, state_size], means [T, H, Nu], seconds)."""
        mc = _capi.MpcConfig()
        mc.n_ticks, mc.warm_steps, mc.exec_steps = int(n_ticks), int(warm_steps), int(exec_steps)
        T, E = max(mc.n_ticks, 0), max(mc.exec_steps, 0)
        S = self.env._state_size
        out = dict(actions=np.zeros((T * E, self.Nu), np.float32), rewards=np.zeros(T * E, np.float32),
                   states=np.zeros((T + 1, S), np.float32), means=np.zeros((T, self.H, self.Nu), np.float32))
        secs = C.c_double()
        _capi.check(self.lib.mbd_plan_run_mpc(self.h, C.byref(mc), _capi.key_array(key), _capi.np_ptr(out["actions"]),
                                              _capi.np_ptr(out["rewards"]), _capi.np_ptr(out["states"]),
                                              _capi.np_ptr(out["means"]), C.byref(secs)))
        out["seconds"] = secs.value
        if self._has_delay:  # (the states the ticks planned from: shat_0 .. shat_{T-1})
            out["predicted"] = np.zeros((T, S), np.float32)
            _capi.check(self.lib.mbd_plan_peek_mpc_predicted(self.h, _capi.np_ptr(out["predicted"])))
        if self._has_sigma:  # (the sigma every tick started from and ended with)
            out["sigmas"] = np.zeros((T, 2), np.float32)
            _capi.check(self.lib.mbd_plan_peek_mpc_sigma(self.h, _capi.np_ptr(out["sigmas"])))
        if self._demo_shape is not None:  # (how far the executed steps were from the clip, and the windows the ticks planned under)
            Kt, Cc = self._demo_shape
            out["track_err"] = np.zeros((T * E, Kt), np.float32)
            out["demo_windows"] = np.zeros((T, Kt, _capi.XREF_ROWS, Cc), np.float32)
            _capi.check(self.lib.mbd_plan_peek_mpc_track(self.h, _capi.np_ptr(out["track_err"]), _capi.np_ptr(out["demo_windows"])))
        if self.has_mpc_pick():  # (what every tick handed on, and the three plans' values)
            out["pick"] = self.peek_mpc_pick(T)
        if self.has_zones:  # (the penalty and the keep-out clearance of every executed control step)
            out["zone_pen"], out["zone_clear"] = np.zeros(T * E, np.float32), np.zeros(T * E, np.float32)
            _capi.check(self.lib.mbd_plan_peek_mpc_zones(self.h, _capi.np_ptr(out["zone_pen"]), _capi.np_ptr(out["zone_clear"])))
        return out

    def peek_mpc_pick(self, capacity: int = None) -> dict:
        """``choice`` [n], ``rets`` [n, 3] and ``best`` [n] of the ticks the last episode or the session has served (the most
        recent ``capacity``, oldest first; None: all)."""
        return _capi.peek_mpc_pick(self.lib.mbd_plan_peek_mpc_pick, self.h, None, capacity)

    def mpc_open(self, key, warm_steps: int, exec_steps: int = 1, max_ticks: int = None) -> MpcSession:
        """Open a session (include/mbd_hip.h mbd_plan_mpc_open): ``run_mpc``'s episode advanced one tick per call from a state
        the caller supplies — ``with plan.mpc_open(key, K) as s: rows = s.tick(state)["rows"]``.  The plan's noise, ensemble,
        delay and demo records are read now; a plant record is refused (the caller is the plant).  ``max_ticks`` None: no limit.
        Until the session is closed the plan's other calls are refused."""
        return MpcSession(self, key, warm_steps, exec_steps, max_ticks)

    def set_mpc_plant(self, env=None, key=None, act_std: float = 0.0, kick_std: float = 0.0, kick_every: int = 1):
        """The plant of the plan's episodes (include/mbd_hip.h mbd_mpc_plant): ``run_mpc`` then executes the rows on ``env``
        (None: the plan's own env; any env of the same topology, e.g. ``RigidBodyEnv(name, model=env.sys.scaled(mass=1.3))``)
        with normal noise of std ``act_std`` on every executed action and a velocity kick of std ``kick_std`` on link 0
        after every ``kick_every``-th tick, drawn on the device from ``key``'s own chain.  ``run`` ignores it.  The plan keeps
        a reference to ``env``."""
        rec = _plant_record(env, key, act_std, kick_std, kick_every)
        _capi.check(self.lib.mbd_plan_set_mpc_plant(self.h, C.byref(rec)))
        self._plant_env = env

    def clear_mpc_plant(self):
        _capi.check(self.lib.mbd_plan_set_mpc_plant(self.h, None))
        self._plant_env = None

    def set_ensemble(self, envs, risk: str = "mean"):
        """Plan over an ensemble of perturbed models (include/mbd_hip.h mbd_ensemble): every candidate of every diffusion
        step is rolled out on each env of ``envs`` (1..8 of them, None: the plan's own env; any env of the same topology,
        e.g. ``RigidBodyEnv(name, model=env.sys.scaled(mass=1.2))``) and scored by its ``risk`` over them — "mean" or
        "min" (the worst member).  ``run``, ``run_mpc`` and the step calls read it; ``eval`` and the final reward keep
        the plan's own env.  The plan keeps references to the envs."""
        rec = _ensemble_record(envs, risk)
        _capi.check(self.lib.mbd_plan_set_ensemble(self.h, C.byref(rec)))
        self._ens_envs = list(envs)

    def clear_ensemble(self):
        _capi.check(self.lib.mbd_plan_set_ensemble(self.h, None))
        self._ens_envs = None

    def peek_value(self):
        """The last step's V [shard_count] (a plan with a value record)."""
        v = np.zeros(self.cfg.shard_count, np.float32)
        _capi.check(self.lib.mbd_plan_peek_value(self.h, _capi.np_ptr(v)))
        return v

    def eval_value(self, states):
        """V [B] of ``states`` [B, state_size], by the kernel the steps run (a check of an imported net)."""
        states = np.ascontiguousarray(states, np.float32)
        if states.ndim != 2 or states.shape[1] != self.env._state_size:
            raise ValueError(f"states {states.shape}: expected [B, {self.env._state_size}]")
        v = np.full(states.shape[0], np.nan, np.float32)
        _capi.check(self.lib.mbd_plan_eval_value(self.h, _capi.np_ptr(states), states.shape[0], _capi.np_ptr(v)))
        return v

    def peek_weighting(self) -> dict:
        """``temp``, ``ess`` and ``kept``, one entry per score step of the last ``run``, the last phase call or the last tick (a
        plan with a weighting record)."""
        return _capi.peek_weighting(self.lib.mbd_plan_peek_weighting, self.h, None, self.cfg.Ndiffuse - 1)

    def set_adapt(self, rate: float, a_min: float, a_max: float, carry=True):
        """Shape the sampling noise from the weighted spread of the candidates (include/mbd_hip.h mbd_adapt): the plan keeps a table
        ``a`` [H, Nu], all ones at the start, samples under ``a`` times the noise shape in force, and moves ``a`` behind every
        diffusion step by ``rate`` towards where the spread of the step's weighted candidates says the noise should go, every
        entry within [``a_min``, ``a_max``].  ``carry``: a tick boundary shifts the table with the mean (False: every tick starts
        from ones).  MBD and mppi plans, unsharded, without ``enable_demo``."""
        rec = _capi.adapt_record(rate, a_min, a_max, carry)
        _capi.check(self.lib.mbd_plan_set_adapt(self.h, C.byref(rec)))

    def clear_adapt(self):
        _capi.check(self.lib.mbd_plan_set_adapt(self.h, None))

    def peek_adapt(self, capacity: int = None) -> dict:
        """``a`` [H, Nu], the table as it stands, and ``ratio`` / ``skipped``: S and the skipped flag of every step since the last
        ``run``, episode or session began — or the most recent ``capacity`` of them (a plan with an adapt record)."""
        out = _capi.peek_adapt(self.lib.mbd_plan_peek_adapt, self.h, self.H * self.Nu, capacity)
        out["a"] = out["a"].reshape(self.H, self.Nu)
        return out

    def peek_elites(self, capacity: int = None) -> dict:
        """``E`` [count, H, Nu], ``R`` and ``src`` [count]: the elites as they stand; ``log_count`` / ``log_kept`` / ``log_top``: per
        step since the last ``run``, episode or session began — or the most recent ``capacity`` of them — how many elites the step
        selected, how many of them were candidates it had injected, and the best return (a plan with an elite record)."""
        if not self.has_elites:
            _capi.check(self.lib.mbd_plan_peek_elites(self.h, None, None, None, None, None, None, None, 0, None))
        out = _capi.peek_elites(self.lib.mbd_plan_peek_elites, self.h, self._elites or 0, self.H * self.Nu, capacity)
        out["E"] = out["E"].reshape(-1, self.H, self.Nu)
        return out

    def peek_togo(self) -> dict:
        """``starts`` [G] the groups' first rows, ``R`` and ``W`` [G, Nsample] the groups' returns and weights of the last step (a
        plan with a to-go record); row 0 is the rewards the score read and the weights ``peek`` returns."""
        if not self.has_togo:
            _capi.check(self.lib.mbd_plan_peek_togo(self.h, None, None, None, None))
        return _capi.peek_togo(self.lib.mbd_plan_peek_togo, self.h, self.H, self.cfg.Nsample)

    def peek_zones(self) -> dict:
        """``pen`` and ``clr`` [Nsample] of the last step (a plan with a zone record): each candidate's penalty and its smallest
        distance to a keep-out surface (negative: inside; +inf without keep-out entries)."""
        if not self.has_zones:
            _capi.check(self.lib.mbd_plan_peek_zones(self.h, None, None))
        return _capi.peek_zones(self.lib.mbd_plan_peek_zones, self.h, None, self.cfg.shard_count)

    def peek_objective(self):
        """The last step's ``ret`` [shard_count] ([M, N] under an ensemble record) and ``cost`` [shard_count] (a plan with an
        objective record)."""
        M = len(self._ens_envs or ())
        sh = self.cfg.shard_count
        ret = np.zeros((M, sh) if M else sh, np.float32)
        cost = np.zeros(sh, np.float32)
        _capi.check(self.lib.mbd_plan_peek_objective(self.h, _capi.np_ptr(ret), _capi.np_ptr(cost)))
        return ret, cost

    def peek_ensemble(self):
        """The last step's per-member rewards [M, N] and combined rewards [N] (a plan with an ensemble record)."""
        M = len(self._ens_envs or ())
        rm = np.zeros((M, self.cfg.Nsample), np.float32)
        r = np.zeros(self.cfg.Nsample, np.float32)
        _capi.check(self.lib.mbd_plan_peek_ensemble(self.h, _capi.np_ptr(rm), _capi.np_ptr(r)))
        return rm, r

    def get_sigma(self) -> float:
        v = C.c_float()
        _capi.check(self.lib.mbd_plan_get_sigma(self.h, C.byref(v)))
        return v.value

    def set_sigma(self, v: float):
        _capi.check(self.lib.mbd_plan_set_sigma(self.h, float(v)))

    def eval(self, Y) -> float:
        Y = np.ascontiguousarray(Y, np.float32)
        rf = C.c_float()
        _capi.check(self.lib.mbd_plan_eval(self.h, _capi.np_ptr(Y), C.byref(rf)))
        return rf.value

    def peek(self, want_weights=True):
        N, sh = self.cfg.Nsample, self.cfg.shard_count
        Y0s = np.zeros((N, self.H, self.Nu), np.float32)
        rewss = np.zeros((sh, self.H), np.float32)
        w = np.zeros(N, np.float32)
        _capi.check(self.lib.mbd_plan_peek(self.h, _capi.np_ptr(Y0s), _capi.np_ptr(rewss), _capi.np_ptr(w)))
        return Y0s, rewss, w

    def close(self):
        if self.h is not None:
            self.lib.mbd_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostProgress:
    """The per-step mean rewards the reference shows on its progress bar (mbd_planner.py:147), delivered WITHOUT a
    stream synchronisation: one slot per diffusion step in pinned, device-visible host memory, pre-filled with NaN;
    ``mbd_plan_score_update`` is handed the slot's address as its ``d_rew_mean`` and the score kernel's own store
    lands there.  ``wait(k)`` spins on the slot (falling back to a device synchronisation after ``timeout_s``, e.g.
    when the mean itself is NaN); the device meanwhile runs on into the weighted mean and the next step."""

    def __init__(self, n: int, device):
        import torch
        self.t = torch.full((max(n, 1),), float("nan"), dtype=torch.float32).pin_memory()
        self.v = self.t.numpy()
        self.device = device
        self.gave_up = False  # a slot stayed NaN past the timeout (a diverged plan's mean IS NaN): synchronise from then on

    def ptr(self, k: int) -> int:
        return self.t.data_ptr() + 4 * k

    def reset(self, k: int) -> None:
        self.v[k] = np.nan

    def wait(self, k: int, timeout_s: float = 2.0) -> float:
        import torch
        v, t0, spins = self.v, None, 0
        if self.gave_up:  # (a genuinely NaN mean looks like "not written yet": do not spin the timeout again every step)
            torch.cuda.synchronize(self.device)
            return float(v[k])
        while v[k] != v[k]:  # NaN: not written yet
            spins += 1
            if spins & 0xfff == 0:
                t0 = t0 or time.perf_counter()
                if time.perf_counter() - t0 > timeout_s:
                    torch.cuda.synchronize(self.device)
                    self.gave_up = True
                    break
        return float(v[k])


def shard_bounds(N: int, world: int, rank: int):
    """Candidates [begin, begin+count) owned by `rank`: contiguous, equal shards (N % world == 0)."""
    if N % world:
        raise ValueError(f"Nsample={N} must be divisible by the world size {world}")
    sh = N // world
    return rank * sh, sh


class P2PExchange:
    """Owner of an ``mbd_exchange`` handle: the step's all-gather as direct peer writes into every rank's receive
    window (include/mbd_hip.h "in-library exchange") instead of a collective-library call.  The IPC handles of the
    windows travel once, at construction, through the process group (any backend)."""

    def __init__(self, device: int, rows: int, shard: int, group=None):
        """Collective over ``group``: every rank must construct it.  A failure on ANY rank (no IPC, no peer access) is
        agreed on before anybody returns — all ranks raise, nobody is left waiting in a collective."""
        import torch
        import torch.distributed as dist
        self.lib = _capi.load()
        self.rank, self.world = dist.get_rank(group), dist.get_world_size(group)
        self.rows, self.shard = rows, shard
        self.h = None
        why = None
        mine = (C.c_ubyte * 64)()
        try:
            h = C.c_void_p()
            _capi.check(self.lib.mbd_exchange_create(device, self.rank, self.world, rows, shard, C.byref(h)))
            self.h = h
            _capi.check(self.lib.mbd_exchange_local_handle(self.h, mine))
        except Exception as e:  # noqa: BLE001
            why = f"rank {self.rank}: {e}"
        handles = [None] * self.world
        dist.all_gather_object(handles, bytes(mine), group=group)
        if why is None:
            try:
                blob = (C.c_ubyte * (64 * self.world)).from_buffer_copy(b"".join(handles))
                _capi.check(self.lib.mbd_exchange_connect(self.h, blob))
            except Exception as e:  # noqa: BLE001
                why = f"rank {self.rank}: {e}"
        on_gpu = dist.get_backend(group) == "nccl"
        ok = torch.tensor([0 if why else 1], dtype=torch.int32, device=torch.device("cuda", device) if on_gpu else "cpu")
        dist.all_reduce(ok, op=dist.ReduceOp.MIN, group=group)  # (also the barrier: every window is mapped everywhere)
        if int(ok.item()) == 0:
            self.close()
            raise _capi.MbdError(_capi.MBD_ERR_STATE, why or "the in-library exchange could not be set up on another rank")

    def all_gather(self, local, stream: int) -> int:
        """local: CUDA tensor [rows, shard].  Returns the device address of the gathered [rows, world * shard] values
        (valid until the next call); asynchronous on ``stream``."""
        out = C.c_void_p()
        _capi.check(self.lib.mbd_exchange_all_gather(self.h, local.data_ptr(), C.byref(out), stream))
        return out.value

    def status(self):
        _capi.check(self.lib.mbd_exchange_status(self.h))

    def close(self):
        if self.h is not None:
            self.lib.mbd_exchange_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def exchange_rewards(local, world: int, group=None):
    """The ONE exchange step of a diffusion step: every rank contributes the per-candidate values of its
    shard (``local`` [rows, shard]) and receives all N of them, rank-major = candidate order, as
    [rows, N].  One all-gather (RCCL over xGMI on GPUs; gloo in the CPU tests and in the two-ranks-on-one-GPU
    dry runs, where device tensors are staged through the host)."""
    import torch
    import torch.distributed as dist
    if world == 1:
        return local
    rows, sh = local.shape
    if local.is_cuda and dist.get_backend(group) == "gloo":
        host = torch.empty((world * rows, sh), dtype=local.dtype)
        dist.all_gather_into_tensor(host, local.detach().cpu().contiguous(), group=group)
        gathered = host.to(local.device)
    else:
        gathered = torch.empty((world * rows, sh), dtype=local.dtype, device=local.device)
        dist.all_gather_into_tensor(gathered, local.contiguous(), group=group)  # concatenation along dim 0
    return gathered.view(world, rows, sh).permute(1, 0, 2).reshape(rows, world * sh).contiguous()


def reverse_distributed(plan: Plan, key, device, group=None, sync_every_step: bool = False, progress=None,
                        phase_times: dict = None, collective: str = None):
    """reverse() (mbd_planner.py:138-148) with the candidates sharded over the ranks of ``group``.
    One all-gather of the per-candidate mean rewards per diffusion step (plus the demo log-densities
    when enabled, packed in the same buffer). Returns (mu_0ts, rew_means) as CUDA tensors.

    ``sync_every_step`` / ``progress``: the reference formats the step's mean reward for its progress bar every
    step (:147), which is a device->host read per step; ``progress(i, rew)`` receives that value.
    ``phase_times``: a dict that receives HIP-event milliseconds per step of phase 1 (sample + rollout), the
    exchange and phase 2 (score + weighted mean) — each phase is then fenced, for measurement only.
    ``collective``: "torch" (all_gather_into_tensor: RCCL over xGMI, or gloo) or "p2p" (the in-library exchange:
    peer writes into every rank's window, no collective library on the step's path); default: $MBD_COLLECTIVE or
    "torch".  Same values either way."""
    import torch
    import torch.distributed as dist

    N, sh = plan.cfg.Nsample, plan.cfg.shard_count
    # the exchange follows the PLAN's shard layout, not whatever process group happens to be initialised: an unsharded
    # plan (force_single under torchrun) must not all-gather — it would score rank 0's rewards on every rank
    world = N // sh
    if sh * world != N:
        raise ValueError(f"shard_count={sh} does not divide Nsample={N}")
    if world > 1:
        group_world = dist.get_world_size(group) if dist.is_initialized() else 1
        if group_world != world:
            raise ValueError(f"the plan is sharded over {world} ranks but the process group has {group_world}")
    demo = bool(plan.cfg.enable_demo)
    rows = 2 if demo else 1
    HNu = plan.H * plan.Nu
    dev = torch.device("cuda", device)
    stream = torch.cuda.current_stream(dev).cuda_stream
    mu = torch.zeros((plan.Nd - 1, HNu), dtype=torch.float32, device=dev)
    rew_means = torch.zeros(plan.Nd - 1, dtype=torch.float32, device=dev)
    Ybar = torch.zeros(HNu, dtype=torch.float32, device=dev)  # YN = zeros (mbd_planner.py:95)
    local = torch.zeros((rows, sh), dtype=torch.float32, device=dev)
    rng = np.asarray(key, np.uint32)
    impl = plan.cfg.prng_impl
    lib = plan.lib
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if phase_times is not None else None
    acc = [0.0, 0.0, 0.0]
    collective = collective or os.environ.get("MBD_COLLECTIVE", "torch")
    p2p = None
    if world > 1 and collective == "p2p":
        # the constructor agrees on a failure across the ranks (all raise, or none): a runtime without fine-grained device
        # memory or peer mappings (mbd_exchange_create: MBD_ERR_UNSUPPORTED) falls back — on EVERY rank — to the collective
        # library's all-gather, as include/mbd_hip.h tells the caller to; same values either way
        try:
            p2p = P2PExchange(device, rows, sh, group)
        except _capi.MbdError as e:
            import warnings
            warnings.warn(f"in-library exchange unavailable ({e}): falling back to torch.distributed all-gather")
            p2p = None
    host = HostProgress(plan.Nd - 1, dev) if (sync_every_step or progress is not None) else None
    # Host work that does not depend on the GPU — the key chain (rng, Y0s_rng = split(rng), mbd_planner.py:103) and the
    # declaration of the FOLLOWING step's key (its normals are generated beside this step's rollout) — is done while
    # the device runs the previous step, before the host waits for that step's mean reward: the wait is followed by
    # the rollout launch and nothing else.
    keys = _capi.prng_split(rng, 2, impl)
    rng, ks = keys[0], _capi.key_array(keys[1])
    keys = _capi.prng_split(rng, 2, impl)
    if plan.Nd - 1 > 1:
        _capi.check(lib.mbd_plan_prefetch_noise(plan.h, _capi.key_array(keys[1]), stream))
    p_loc0, p_loc1 = local[0].data_ptr(), (local[1].data_ptr() if demo else None)
    for i in range(plan.Nd - 1, 0, -1):
        if ev:
            ev[0].record()
        _capi.check(lib.mbd_plan_sample_rollout(plan.h, i, ks, Ybar.data_ptr(), p_loc0, p_loc1, stream))
        if ev:
            ev[1].record()
        if p2p is not None:
            base = p2p.all_gather(local, stream)
            p_all0, p_all1 = base, (base + 4 * N if demo else None)
        else:
            allv = exchange_rewards(local, world, group)
            p_all0, p_all1 = allv[0].data_ptr(), (allv[1].data_ptr() if demo else None)
        if ev:
            ev[2].record()
        out = mu[plan.Nd - 1 - i]
        k = plan.Nd - 1 - i
        _capi.check(lib.mbd_plan_score_update(plan.h, i, ks, Ybar.data_ptr(), p_all0, p_all1, out.data_ptr(),
                                              host.ptr(k) if host else rew_means[k:].data_ptr(), stream))
        Ybar = out
        if ev:
            ev[3].record()
            ev[3].synchronize()
            for j in range(3):
                acc[j] += ev[j].elapsed_time(ev[j + 1])
        if i > 1:  # the next step's keys, and the declaration of the one after it
            rng, ks = keys[0], _capi.key_array(keys[1])
            keys = _capi.prng_split(rng, 2, impl)
            if i > 2:
                _capi.check(lib.mbd_plan_prefetch_noise(plan.h, _capi.key_array(keys[1]), stream))
        if host is not None:  # the reference formats the reward every step (:147): one host read per step
            r = host.wait(k)
            if progress is not None:
                progress(i, r)
    if phase_times is not None:
        n = max(plan.Nd - 1, 1)
        phase_times.update(phase1_ms=acc[0] / n, exchange_ms=acc[1] / n, phase2_ms=acc[2] / n, steps=plan.Nd - 1)
    if host is not None:
        torch.cuda.synchronize(dev)
        rew_means.copy_(host.t[: plan.Nd - 1])
    if p2p is not None:
        p2p.status()  # (raises when a wait ran into its time limit: a peer never arrived)
        p2p.close()
    return mu.view(plan.Nd - 1, plan.H, plan.Nu), rew_means


def run_diffusion(args: Args, device: int = None, return_details: bool = False, progress=None,
                  force_single: bool = False, measure_phases: bool = False, collective: str = None, ensemble=None):
    """mbd_planner.py:38-182. Returns rew_final (float); ``return_details`` adds a dict with mu_0ts,
    per-step mean rewards and the reverse-loop wall time.  ``progress(i, rew)`` is called after every diffusion
    step with the step's mean reward, like the reference's progress bar (:147) — one device->host read per step;
    without it the loop runs asynchronously and the means are read once at the end.  ``force_single`` ignores an
    initialised process group (every rank then runs the whole plan).  ``ensemble``: plan over perturbed models
    (``Plan.set_ensemble``) — a list of member envs (None: the env itself), or a dict(envs=[...], risk="mean" | "min");
    unsharded plans only."""
    import torch
    import torch.distributed as dist

    distributed = (not force_single) and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0")) if distributed else 0
    rng = _capi.prng_key(args.seed)  # :40
    apply_recommended(args)
    env = get_env(args.env_name, device=device)  # :70
    impl = prng_impl()
    rng, rng_reset = _capi.prng_split(rng, 2, impl)  # :79  NOTE: rng_reset should never be changed.
    state_init = env.reset(rng_reset)  # :80
    rng_exp, rng = _capi.prng_split(rng, 2, impl)  # :150

    if distributed:
        begin, sh = shard_bounds(args.Nsample, dist.get_world_size(), dist.get_rank())
        plan = Plan(env, args, shard_begin=begin, shard_count=sh)
    else:
        plan = Plan(env, args)
    plan.set_state0(state_init)
    if ensemble is not None:
        ens = ensemble if isinstance(ensemble, dict) else dict(envs=ensemble)
        plan.set_ensemble(ens["envs"], ens.get("risk", "mean"))
    _, _, sigmas = plan.schedule()
    print(f"init sigma = {sigmas[-1]:.2e}")  # :93

    phases = {} if measure_phases else None
    if distributed or progress is not None or measure_phases:
        torch.cuda.set_device(device)
        torch.cuda.synchronize(device)
        t0 = time.time()
        mu_t, rm_t = reverse_distributed(plan, rng_exp, device, progress=progress, phase_times=phases,
                                         collective=collective)
        torch.cuda.synchronize(device)
        secs = time.time() - t0
        mu, rew_means = mu_t.cpu().numpy(), rm_t.cpu().numpy()
        rew_final = plan.eval(mu[-1])  # :179-180
    else:
        mu, rew_means, rew_final, secs = plan.run(rng_exp)

    if not args.not_render and (not distributed or dist.get_rank() == 0):  # :152-156 (mu_0ts.npy only)
        path = os.path.join(os.getcwd(), "results", args.env_name)
        os.makedirs(path, exist_ok=True)
        np.save(os.path.join(path, "mu_0ts.npy"), mu)
        # stand-in for rollout.html / rollout.png (:157-178): the replayed final plan as arrays
        from ..utils import rollout_states
        np.savez_compressed(os.path.join(path, "rollout_states.npz"), **rollout_states(env, state_init, mu[-1]))
    plan.close()
    if return_details:
        return rew_final, dict(mu_0ts=mu, rew_means=rew_means, loop_seconds=secs, state_init=state_init,
                               steps_per_sec=(args.Ndiffuse - 1) / secs, sharded=bool(distributed),
                               world=dist.get_world_size() if distributed else 1, phase_ms=phases)
    return rew_final


if __name__ == "__main__":
    import argparse

    p = argparse.ArgumentParser()
    for f in Args.__dataclass_fields__.values():
        if f.type in ("bool", bool):
            p.add_argument(f"--{f.name}", action="store_true")
        else:
            p.add_argument(f"--{f.name}", type=type(f.default), default=f.default)
    ns = p.parse_args()
    rew_final = run_diffusion(Args(**vars(ns)), progress=lambda i, rew: print(f"\rDiffusing i={i:4d} rew {rew:.2e}",
                                                                                 end="", flush=True))  # :141-147
    print(f"\nfinal reward = {rew_final:.2e}")  # :187
