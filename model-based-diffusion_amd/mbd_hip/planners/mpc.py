"""Receding-horizon control on top of the planner (include/mbd_hip.h mbd_plan_run_mpc):
every control tick replans from the state the system reached, warm-started from the previous tick's plan, and executes the
first ``exec_steps`` rows of the new one — the whole episode on the device.  The reference plans open loop only
(mbd_planner.py); the reset and the episode key follow its seed chain (:40,79,150), so tick 0 is ``run_diffusion``'s plan.

    python -m mbd_hip.planners.mpc --env_name hopper --n_ticks 100 --warm_steps 20

prints one JSON line (timings of a second episode, after a warm-up one in the same process).
"""
from __future__ import annotations

import os
from dataclasses import dataclass

import numpy as np

from .. import _capi
from ..envs import get_env
from ..envs.base import prng_impl
from .mbd_planner import Args, Plan, apply_recommended


@dataclass
class MpcArgs(Args):
    n_ticks: int = 50  # control ticks T of the episode
    warm_steps: int = 20  # diffusion steps K..1 of every tick after the first (the noise level it restarts from: sigma_K)
    exec_steps: int = 1  # control steps E executed per tick; the plan then shifts by E rows


def _setup(args: MpcArgs, device: int):
    rng = _capi.prng_key(args.seed)  # mbd_planner.py:40
    apply_recommended(args)
    env = get_env(args.env_name, device=device)
    rng, rng_reset = _capi.prng_split(rng, 2, prng_impl())  # :79
    state_init = env.reset(rng_reset)  # :80
    rng_exp, rng = _capi.prng_split(rng, 2, prng_impl())  # :150
    plan = Plan(env, args)
    plan.set_state0(state_init)
    return env, plan, state_init, rng_exp


def _save(args: MpcArgs, ep: dict) -> None:
    path = os.path.join(os.getcwd(), "results", args.env_name)
    os.makedirs(path, exist_ok=True)
    np.savez_compressed(os.path.join(path, "mpc_episode.npz"), actions=ep["actions"], rewards=ep["rewards"],
                        states=ep["states"], means=ep["means"])


def run_mpc(args: MpcArgs, device: int = None, return_details: bool = False):
    """One closed-loop episode of ``args.n_ticks`` ticks.  Returns the episode's mean reward (over its T * E executed control
    steps); ``return_details`` adds a dict with the episode's actions, rewards, states (s_0 .. s_T), per-tick means, the
    loop's wall time (seconds), the reset state, the episode key and the control dt.  Unless ``not_render``:
    results/<env>/mpc_episode.npz."""
    env, plan, state_init, key = _setup(args, 0 if device is None else device)
    try:
        ep = plan.run_mpc(key, args.n_ticks, args.warm_steps, args.exec_steps)
    finally:
        plan.close()
    reward = float(ep["rewards"].mean())
    if not args.not_render:
        _save(args, ep)
    if return_details:
        return reward, dict(ep, state_init=state_init, key=key, dt=env.dt)
    return reward


def _main(argv=None) -> dict:
    """The CLI: a warm-up episode, an open-loop run_diffusion loop of the same plan (its ms per diffusion step, for
    comparison) and the timed episode, all in one process; returns what it prints."""
    import argparse
    import contextlib
    import json
    import sys

    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    for f in MpcArgs.__dataclass_fields__.values():
        if f.type in ("bool", bool):
            p.add_argument(f"--{f.name}", action="store_true")
        else:
            p.add_argument(f"--{f.name}", type=type(f.default), default=f.default)
    args = MpcArgs(**vars(p.parse_args(argv)))
    with contextlib.redirect_stdout(sys.stderr):  # (stdout carries the JSON line only)
        env, plan, state_init, key = _setup(args, 0)
        T, K, E, Nd = args.n_ticks, args.warm_steps, args.exec_steps, args.Ndiffuse
        plan.run_mpc(key, T, K, E)  # warm-up
        _, _, _, open_secs = plan.run(key)
        ep = plan.run_mpc(key, T, K, E)
        plan.close()
    steps = (Nd - 1) + (T - 1) * K  # diffusion steps the episode ran
    secs = ep["seconds"]
    open_ms = 1e3 * open_secs / (Nd - 1)
    res = dict(env=args.env_name, Nsample=args.Nsample, Hsample=args.Hsample, Ndiffuse=Nd, n_ticks=T, warm_steps=K,
               exec_steps=E, ms_per_tick=1e3 * secs / T, ticks_per_s=T / secs, ms_per_diffusion_step=1e3 * secs / steps,
               open_loop_ms_per_diffusion_step=open_ms,
               # what a tick costs beyond its diffusion steps at the open-loop rate: the two boundary launches
               boundary_ms_per_tick=(1e3 * secs - steps * open_ms) / T,
               real_time_factor=T * E * env.dt / secs, episode_reward=float(ep["rewards"].mean()))
    if not args.not_render:
        _save(args, ep)
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    _main()
