"""Receding-horizon control on top of the planner (include/mbd_hip.h mbd_plan_run_mpc):
every control tick replans from the state the system reached, warm-started from the previous tick's plan, and executes the
first ``exec_steps`` rows of the new one — the whole episode on the device.  The reference plans open loop only
(mbd_planner.py); the reset and the episode key follow its seed chain (:40,79,150), so tick 0 is ``run_diffusion``'s plan.

    python -m mbd_hip.planners.mpc --env_name hopper --n_ticks 100 --warm_steps 20

prints one JSON line (timings of a second episode, after a warm-up one in the same process).  ``--n_episodes P`` runs the
seeds ``seed .. seed+P-1`` as ONE batch of lockstep episodes (mbd_sweep_run_mpc; ``run_mpc_batch``): a diffusion step of a tick
is one rollout launch over all the episodes' candidates, and every episode is the single one bit for bit.
"""
from __future__ import annotations

import os
from dataclasses import dataclass

import numpy as np

from .. import _capi
from ..envs import get_env
from ..envs.base import prng_impl
from .mbd_planner import Args, Plan, Sweep, apply_recommended

MAX_EPISODES = 32  # include/mbd_hip.h MBD_SWEEP_MAX_PLANS


@dataclass
class MpcArgs(Args):
    n_ticks: int = 50  # control ticks T of the episode
    warm_steps: int = 20  # diffusion steps K..1 of every tick after the first (the noise level it restarts from: sigma_K)
    exec_steps: int = 1  # control steps E executed per tick; the plan then shifts by E rows


def _reset_and_key(env, seed: int):
    """The reset state and the episode key of a seed, by the reference's chain."""
    rng = _capi.prng_key(seed)  # mbd_planner.py:40
    rng, rng_reset = _capi.prng_split(rng, 2, prng_impl())  # :79
    state_init = env.reset(rng_reset)  # :80
    rng_exp, rng = _capi.prng_split(rng, 2, prng_impl())  # :150
    return state_init, rng_exp


def _setup(args: MpcArgs, device: int):
    apply_recommended(args)
    env = get_env(args.env_name, device=device)
    state_init, rng_exp = _reset_and_key(env, args.seed)
    plan = Plan(env, args)
    plan.set_state0(state_init)
    return env, plan, state_init, rng_exp


def _check_batch(arg_list) -> None:
    """What a batch of lockstep episodes takes (the rule of scripts.run_mbd._batchable): up to 32 episodes of one rigid-body
    env with one set of sizes, schedule and (T, K, E); seeds and temperatures may differ.  Decided from the arguments alone."""
    from dataclasses import asdict

    from ..scripts.run_mbd import _resolved
    if not 1 <= len(arg_list) <= MAX_EPISODES:
        raise ValueError(f"{len(arg_list)} episodes: a batch holds 1 to {MAX_EPISODES}")
    ds = [asdict(_resolved(a)) for a in arg_list]
    for k, d in enumerate(ds):
        for f, v in d.items():
            if f not in ("seed", "temp_sample", "not_render") and v != ds[0][f]:
                raise ValueError(f"{f} differs between episodes 0 and {k} ({ds[0][f]!r}, {v!r}): the episodes of a batch "
                                 "may differ in seed and temp_sample only")
    if ds[0]["env_name"] in ("car2d", "pushT"):
        raise ValueError(f"env_name={ds[0]['env_name']!r}: batches run rigid-body envs; run its episodes one by one")
    if ds[0]["Nsample"] * 4 > 48 * 1024:
        raise ValueError(f"Nsample={ds[0]['Nsample']}: plans of more than 12288 candidates fill the chip on their own; "
                         "run their episodes one by one")
    if ds[0]["enable_demo"]:
        raise ValueError("enable_demo: demos are time-indexed, an episode has no clock for them")


def _setup_batch(arg_list, device: int):
    for a in arg_list:
        apply_recommended(a)
    a0 = arg_list[0]
    env = get_env(a0.env_name, device=device)
    sweep = Sweep(env, a0, len(arg_list), temps=[a.temp_sample for a in arg_list])
    states, keys = [], []
    for k, a in enumerate(arg_list):
        state_init, rng_exp = _reset_and_key(env, a.seed)
        sweep.set_state0(k, state_init)
        states.append(state_init)
        keys.append(rng_exp)
    return env, sweep, states, np.array(keys, np.uint32)


_LOGS = ("actions", "rewards", "states", "means")


def run_mpc_batch(arg_list, device: int = None, return_details: bool = False):
    """The episodes of ``arg_list`` (MpcArgs that differ in ``seed`` and ``temp_sample`` only, else ValueError naming the field)
    as ONE batch in lockstep.  Episode k is ``run_mpc(arg_list[k])`` bit for bit.  Returns the list of the episodes' mean
    rewards; ``return_details`` adds the list of their detail dicts (as ``run_mpc``'s; ``seconds`` is the whole batch's).
    Unless the first episode says ``not_render``: results/<env>/mpc_episode.npz, its arrays with a leading episode axis when
    there is more than one episode."""
    arg_list = list(arg_list)
    _check_batch(arg_list)
    env, sweep, states, keys = _setup_batch(arg_list, 0 if device is None else device)
    try:
        ep = sweep.run_mpc(keys, arg_list[0].n_ticks, arg_list[0].warm_steps, arg_list[0].exec_steps)
    finally:
        sweep.close()
    rewards = [float(r.mean()) for r in ep["rewards"]]
    if not arg_list[0].not_render:
        _save(arg_list[0], ep if len(arg_list) > 1 else {k: ep[k][0] for k in _LOGS})
    if return_details:
        return rewards, [dict({f: ep[f][k] for f in _LOGS}, seconds=ep["seconds"], state_init=states[k], key=keys[k], dt=env.dt)
                         for k in range(len(arg_list))]
    return rewards


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
    p.add_argument("--n_episodes", type=int, default=1, help="seeds seed .. seed+P-1 as one batch of lockstep episodes")
    ns = vars(p.parse_args(argv))
    n_episodes = ns.pop("n_episodes")
    args = MpcArgs(**ns)
    if n_episodes != 1:
        return _main_batch(args, n_episodes)
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


def _main_batch(args: MpcArgs, P: int) -> dict:
    """``--n_episodes P``: the batch after a warm-up batch, the sweep's and one plan's open-loop loops, and ONE sequential episode
    of the first seed (what the batch replaces P times) after a warm-up one, all in one process."""
    import contextlib
    import json
    import sys
    from dataclasses import replace

    arg_list = [replace(args, seed=args.seed + k) for k in range(P)]
    _check_batch(arg_list)
    with contextlib.redirect_stdout(sys.stderr):  # (stdout carries the JSON line only)
        env, sweep, states, keys = _setup_batch(arg_list, 0)
        a0 = arg_list[0]
        T, K, E, Nd = a0.n_ticks, a0.warm_steps, a0.exec_steps, a0.Ndiffuse
        sweep.run_mpc(keys, T, K, E)  # warm-up
        _, _, _, open_secs = sweep.run(keys, outputs=False)
        ep = sweep.run_mpc(keys, T, K, E)
        sweep.close()
        plan = Plan(env, a0)
        plan.set_state0(states[0])
        plan.run_mpc(keys[0], T, K, E)  # warm-up
        _, _, _, open_secs_1 = plan.run(keys[0])
        seq = plan.run_mpc(keys[0], T, K, E)
        plan.close()
    steps = (Nd - 1) + (T - 1) * K  # diffusion steps every episode ran
    secs = ep["seconds"]
    open_ms, open_ms_1 = 1e3 * open_secs / (Nd - 1), 1e3 * open_secs_1 / (Nd - 1)
    rews = [float(r.mean()) for r in ep["rewards"]]
    res = dict(env=a0.env_name, Nsample=a0.Nsample, Hsample=a0.Hsample, Ndiffuse=Nd, n_ticks=T, warm_steps=K, exec_steps=E,
               n_episodes=P, ms_per_tick=1e3 * secs / T, ticks_per_s=T / secs, episode_ticks_per_s=P * T / secs,
               ms_per_diffusion_step=1e3 * secs / steps, open_loop_ms_per_diffusion_step=open_ms,
               # what a tick of the batch costs beyond its diffusion steps at the sweep's open-loop rate: the two boundary launches
               boundary_ms_per_tick=(1e3 * secs - steps * open_ms) / T,
               real_time_factor=T * E * env.dt / secs, episode_reward=float(np.mean(rews)), episode_rewards=rews,
               episode_reward_mean=float(np.mean(rews)), episode_reward_std=float(np.std(rews)),
               # one episode of the first seed on a plan of its own, and what P of them one after another cost against the batch
               sequential_episode_seconds=seq["seconds"], single_open_loop_ms_per_diffusion_step=open_ms_1,
               speedup=P * seq["seconds"] / secs, open_loop_ratio=P * open_ms_1 / open_ms)
    if not a0.not_render:
        _save(a0, ep)
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    _main()
