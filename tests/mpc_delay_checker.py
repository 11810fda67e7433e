"""The checker's restatement of a receding-horizon episode whose plans arrive D ticks late (include/mbd_hip.h mbd_mpc_delay,
DESIGN.md section 1 "N9 delay"): tests/mpc_plant_checker.py's episode with a committed queue C [D, E, Nu] in front of the plant —
the tick executes C[0], predicts with the PLAN's env where the whole queue leaves the system (ONE ``mpc_checker.execute`` over
the concatenated queue), plans from that predicted state with oracle.planner.reverse_once, and appends its plan's first E
rows.  The disturbances, the kick and the shift are mpc_plant_checker's and mpc_checker's own functions."""
from __future__ import annotations

import numpy as np

from mpc_checker import execute, shift
from mpc_plant_checker import disturbances, kick, rows_of
from oracle import planner as op


def queue_of(rows0, D, E, Nu):
    """The committed queue at the start of an episode: rows0 [D*E, Nu] as D blocks of E rows, or zeros."""
    if rows0 is None:
        return np.zeros((D, E, Nu), np.float32)
    return np.ascontiguousarray(rows0, np.float32).reshape(D, E, Nu).copy()


def episode(oenv, state0, key, N, H, Nd, temp, T, K, E, D, rows0=None, plant=None, dkey=(0, 0), act_std=0.0, kick_std=0.0,
            kick_every=1, impl=1, beta0=1e-4, betaT=1e-2):
    """A closed-loop episode of T ticks planned with ``oenv`` D ticks ahead and executed on ``plant`` (None: oenv itself).
    Returns dict(actions [T*E, Nu] (the rows the plant was fed), rewards [T*E], states [T+1, S], means [T, H, Nu] (row 0 of
    means[t] belongs to control step (t + D) E), predicted [T, S] (the states the ticks planned from))."""
    orc = oenv.orc
    plant = oenv if plant is None else plant
    Nu = oenv.Nu
    sched = orc.schedule(beta0, betaT, Nd)
    rng, dk = np.asarray(key, np.uint32), np.asarray(dkey, np.uint32)
    s = np.ascontiguousarray(state0, np.float32).reshape(-1)
    C = queue_of(rows0, D, E, Nu)
    Ybar, i_start = np.zeros((H, Nu), np.float32), Nd - 1
    actions, rewards, states, means, predicted = [], [], [s], [], []
    for t in range(T):
        keys = orc.split(rng, 2, impl)
        rng, r = keys[0], keys[1]  # rng, k_t = split(rng)
        _, shat = execute(oenv, s, C.reshape(D * E, Nu))  # the PLAN's env over the undisturbed queue, in queue order
        shat = np.asarray(shat, np.float32).reshape(-1)
        for i in range(i_start, 0, -1):
            r, Ybar, _, _ = op.reverse_once(orc, oenv, shat, i, r, Ybar, sched, N, H, temp, impl)
        M = Ybar
        dk, eps = disturbances(orc, dk, E, Nu, impl)
        rows = rows_of(C[0], E, eps, act_std)  # (C[0] is E rows: the head block, itself or with the action noise)
        rew, s = execute(plant, s, rows)
        if kick_std > 0 and (t + 1) % kick_every == 0:
            s = kick(plant, s, (np.float32(kick_std) * eps[E * Nu:].astype(np.float32)).astype(np.float32))
        actions.append(rows)
        rewards.append(rew)
        states.append(s)
        means.append(M)
        predicted.append(shat)
        C = np.concatenate([C[1:], M[:E][None]]).astype(np.float32)  # (copied: -0.0 stays -0.0)
        Ybar, i_start = shift(M, E), K
    return dict(actions=np.concatenate(actions), rewards=np.concatenate(rewards), states=np.stack(states),
                means=np.stack(means), predicted=np.stack(predicted))
