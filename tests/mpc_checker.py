"""The checker's restatement of a receding-horizon episode (include/mbd_hip.h mbd_plan_run_mpc):
oracle.planner.reverse_once for the diffusion steps, the checker's rollout for the executed rows, numpy for the shift."""
from __future__ import annotations

import numpy as np

from oracle import planner as op


def shift(M, E):
    """shift_E(M)[h] = M[h + E] for h < H - E, else 0 (the cold plan's prior)."""
    out = np.zeros_like(M)
    out[: M.shape[0] - E] = M[E:]
    return out


def execute(oenv, s, rows):
    """rewards [E] and the state after the executed rows, fed unclipped (the env clips them to its ctrlrange)."""
    us = np.ascontiguousarray(rows, np.float32)[None]
    if oenv.name == "car2d":
        rewss, qs = oenv.orc.car2d_rollout(s, us, want_qs=True)
        return rewss[0], qs[0, -1].copy()
    rewss, fin = oenv.orc.rollout(oenv.ms, s, us, want_final=True)
    return rewss[0], fin[0].reshape(-1)


def episode(oenv, state0, key, N, H, Nd, temp, T, K, E, impl=1, beta0=1e-4, betaT=1e-2):
    """A closed-loop episode of T ticks.  Returns dict(actions [T*E, Nu], rewards [T*E], states [T+1, S], means [T, H, Nu])."""
    orc = oenv.orc
    sched = orc.schedule(beta0, betaT, Nd)
    rng = np.asarray(key, np.uint32)
    s = np.ascontiguousarray(state0, np.float32).reshape(-1)
    Ybar, i_start = np.zeros((H, oenv.Nu), np.float32), Nd - 1
    actions, rewards, states, means = [], [], [s], []
    for _ in range(T):
        keys = orc.split(rng, 2, impl)
        rng, r = keys[0], keys[1]  # rng, k_t = split(rng)
        for i in range(i_start, 0, -1):
            r, Ybar, _, _ = op.reverse_once(orc, oenv, s, i, r, Ybar, sched, N, H, temp, impl)
        M = Ybar
        rew, s = execute(oenv, s, M[:E])
        actions.append(M[:E])
        rewards.append(rew)
        states.append(s)
        means.append(M)
        Ybar, i_start = shift(M, E), K
    return dict(actions=np.concatenate(actions), rewards=np.concatenate(rewards), states=np.stack(states),
                means=np.stack(means))
