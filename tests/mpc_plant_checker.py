"""The checker's restatement of a receding-horizon episode on a plant that is not the planner's model (include/mbd_hip.h
mbd_mpc_plant, DESIGN.md section 1 "N5 plant"): tests/mpc_checker.py's episode with the executed rows disturbed, run through a
second OracleEnv, and the reached state kicked — oracle.planner.reverse_once for the diffusion steps, Oracle.split /
Oracle.normal for the disturbance chain, numpy float32 for the arithmetic (a product, then a sum: two roundings)."""
from __future__ import annotations

import numpy as np

from mpc_checker import execute, shift
from oracle import planner as op

FLAG_PLANAR = 2  # include/mbd_hip.h MBD_FLAG_PLANAR


def _header_constant(name):
    """A #define of include/mbd_hip.h: kernel and checker read the state layout from the same place."""
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mbd_hip.h")
    with open(path) as f:
        return int(re.search(rf"#define {name} (\d+)", f.read()).group(1))


V0 = _header_constant("MBD_LINK_VEL")  # link 0's linear velocity inside a state (p[3], r[4], v[3], w[3] per link)


def kick(oenv, s, k3):
    """s with k3 [3] added to link 0's linear velocity; planar models leave the y component alone."""
    s = np.array(s, np.float32).reshape(-1)
    planar = bool(oenv.ms.flags & FLAG_PLANAR)
    for j in range(3):
        if not (planar and j == 1):
            s[V0 + j] = np.float32(s[V0 + j]) + np.float32(k3[j])
    return s


def disturbances(orc, dk, E, Nu, impl):
    """dk, d_t = split(dk); eps = normal(d_t, (E*Nu + 3,)) — always this many.  Returns (dk', eps)."""
    keys = orc.split(dk, 2, impl)
    return keys[0], orc.normal(keys[1], (E * Nu + 3,), impl)


def rows_of(M, E, eps, act_std):
    """The rows the plant is fed: M[0:E] itself (a copy: -0.0 stays -0.0) or M[0:E] + act_std * eps."""
    Nu = M.shape[1]
    if act_std == 0:
        return M[:E].copy()
    noise = (np.float32(act_std) * eps[: E * Nu].astype(np.float32)).astype(np.float32)
    return (M[:E].astype(np.float32) + noise.reshape(E, Nu)).astype(np.float32)


def episode(oenv, state0, key, N, H, Nd, temp, T, K, E, plant=None, dkey=(0, 0), act_std=0.0, kick_std=0.0, kick_every=1,
            impl=1, beta0=1e-4, betaT=1e-2):
    """A closed-loop episode of T ticks planned with ``oenv`` and executed on ``plant`` (None: oenv itself).  Returns
    dict(actions [T*E, Nu] (the rows the plant was fed), rewards [T*E] (the plant's), states [T+1, S] (after the kicks),
    means [T, H, Nu] (undisturbed))."""
    orc = oenv.orc
    plant = oenv if plant is None else plant
    sched = orc.schedule(beta0, betaT, Nd)
    rng, dk = np.asarray(key, np.uint32), np.asarray(dkey, np.uint32)
    s = np.ascontiguousarray(state0, np.float32).reshape(-1)
    Ybar, i_start = np.zeros((H, oenv.Nu), np.float32), Nd - 1
    actions, rewards, states, means = [], [], [s], []
    for t in range(T):
        keys = orc.split(rng, 2, impl)
        rng, r = keys[0], keys[1]  # rng, k_t = split(rng)
        for i in range(i_start, 0, -1):  # the planner plans with ITS env from the state the plant reached
            r, Ybar, _, _ = op.reverse_once(orc, oenv, s, i, r, Ybar, sched, N, H, temp, impl)
        M = Ybar
        dk, eps = disturbances(orc, dk, E, oenv.Nu, impl)
        rows = rows_of(M, E, eps, act_std)
        rew, s = execute(plant, s, rows)
        if kick_std > 0 and (t + 1) % kick_every == 0:
            s = kick(plant, s, (np.float32(kick_std) * eps[E * oenv.Nu:].astype(np.float32)).astype(np.float32))
        actions.append(rows)
        rewards.append(rew)
        states.append(s)
        means.append(M)
        Ybar, i_start = shift(M, E), K  # (the shift takes the undisturbed mean)
    return dict(actions=np.concatenate(actions), rewards=np.concatenate(rewards), states=np.stack(states),
                means=np.stack(means))
