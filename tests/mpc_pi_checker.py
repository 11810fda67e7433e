"""The checker's restatement of a receding-horizon episode of a path-integral plan (include/mbd_hip.h mbd_mpc_sigma, DESIGN.md
section 1 "N12 path-integral episodes"): mppi, cma-es or cem (path_integral.py:111-127) as the planning loop of
tests/mpc_checker.py's episode, from the checker's own parts — Oracle.split and Oracle.sample for the candidates,
OracleEnv.rollout and oracle.planner.mean_h for the rewards, Oracle.pi_update for the update rule, mpc_checker.execute and
mpc_checker.shift for the tick boundary, mpc_plant_checker's disturbances and mpc_delay_checker's queue where a plant or a delay
is given.  sigma is carried as numpy float32 and the boundary formula is three float32 operations.  A noise shape or basis
composes by wrapping the env (noise_shape_checker / noise_basis_checker wrap ``sample``)."""
from __future__ import annotations

import numpy as np

from mpc_checker import execute, shift
from mpc_delay_checker import queue_of
from mpc_plant_checker import disturbances, kick, rows_of
from oracle import planner as op

METHODS = op.PI_METHODS  # {"mppi": 1, "cma-es": 2, "cem": 3}: the library's update_method


def next_sigma(sigma_end, cold, warm, gain):
    """The sigma a warm tick starts from: sigma_warm when gain == 0, else clamp(gain * sigma_end, sigma_warm, sigma_cold) —
    a product and two selects, each a float32, written so that a NaN sigma stays NaN."""
    f = np.float32
    if f(gain) == f(0):
        return f(warm)
    with np.errstate(all="ignore"):
        x = f(f(gain) * f(sigma_end))
    x = f(warm) if x < f(warm) else x
    x = f(cold) if x > f(cold) else x
    return f(x)


def orc_update(orc, m, rews, Y0s, mu, sigma, temp):
    """The update rule of a refinement: (mu, sigma) of Oracle.pi_update."""
    mu, sigma, _, _ = orc.pi_update(m, rews, Y0s, mu, float(sigma), temp)  # :122-125
    return mu, sigma


def plan_tick(oenv, s_plan, r, mu, sigma, n_it, N, H, temp, method, impl=1, update=orc_update):
    """n_it refinements (path_integral.py:113-126) from the state ``s_plan``.  Returns (r', mu, sigma: float32).  ``update``: a
    stand-in for ``orc_update`` with its signature (a weighting record's: tests/weighting_checker.py)."""
    orc = oenv.orc
    m = METHODS[method] if isinstance(method, str) else int(method)
    for _ in range(n_it):
        keys = orc.split(r, 2, impl)
        r, ks = keys[0], keys[1]  # rng, Y0s_rng = split(rng)  (:114)
        Y0s = orc.sample(ks, impl, N, H, oenv.Nu, 0, N, float(sigma), mu)  # :115-119
        rews = op.mean_h(orc, np.ascontiguousarray(oenv.rollout(s_plan, Y0s)))  # :121
        mu, sigma = update(orc, m, rews, Y0s, mu, sigma, temp)
        sigma = np.float32(sigma)
    return r, mu, np.float32(sigma)


def episode(oenv, state0, key, N, H, Nd, temp, T, K, E, method, sigma_cold=1.0, sigma_warm=1.0, gain=0.0, D=0, rows0=None,
            plant=None, dkey=None, act_std=0.0, kick_std=0.0, kick_every=1, impl=1, plan_tick=plan_tick):
    """A closed-loop episode of T ticks.  ``D`` > 0: the plans arrive D ticks late (mpc_delay_checker).  ``dkey`` not None: a
    plant record (mpc_plant_checker).  Returns dict(actions [T*E, Nu], rewards [T*E], states [T+1, S], means [T, H, Nu],
    sigmas [T, 2] — the sigma each tick started from and ended with —, and with a delay predicted [T, S]).  ``plan_tick``: a stand-in
    for this module's, with its signature."""
    orc = oenv.orc
    Nu = oenv.Nu
    has_plant = dkey is not None
    plant = oenv if plant is None else plant
    rng = np.asarray(key, np.uint32)
    dk = np.asarray(dkey if has_plant else (0, 0), np.uint32)
    s = np.ascontiguousarray(state0, np.float32).reshape(-1)
    C = queue_of(rows0, D, E, Nu) if D > 0 else None
    mu, n_it, sigma = np.zeros((H, Nu), np.float32), Nd - 1, np.float32(sigma_cold)
    actions, rewards, states, means, sigmas, predicted = [], [], [s], [], [], []
    for t in range(T):
        keys = orc.split(rng, 2, impl)
        rng, r = keys[0], keys[1]  # rng, k_t = split(rng)
        s_plan = s
        if D > 0:  # the PLAN's env over the undisturbed queue
            _, s_plan = execute(oenv, s, C.reshape(D * E, Nu))
            s_plan = np.asarray(s_plan, np.float32).reshape(-1)
            predicted.append(s_plan)
        sigma_start = np.float32(sigma)
        _, M, sigma = plan_tick(oenv, s_plan, r, mu, sigma, n_it, N, H, temp, method, impl)
        sigmas.append((sigma_start, np.float32(sigma)))
        head = C[0] if D > 0 else M[:E]
        if has_plant:
            dk, eps = disturbances(orc, dk, E, Nu, impl)
            rows = rows_of(head, E, eps, act_std)
        else:
            rows = np.array(head, np.float32)
        rew, s = execute(plant, s, rows)
        if has_plant and kick_std > 0 and (t + 1) % kick_every == 0:
            s = kick(plant, s, (np.float32(kick_std) * eps[E * Nu:].astype(np.float32)).astype(np.float32))
        actions.append(rows)
        rewards.append(rew)
        states.append(s)
        means.append(M)
        if D > 0:
            C = np.concatenate([C[1:], M[:E][None]]).astype(np.float32)
        mu, n_it = shift(M, E), K
        sigma = next_sigma(sigma, sigma_cold, sigma_warm, gain)
    out = dict(actions=np.concatenate(actions), rewards=np.concatenate(rewards), states=np.stack(states),
               means=np.stack(means), sigmas=np.array(sigmas, np.float32).reshape(T, 2))
    if D > 0:
        out["predicted"] = np.stack(predicted)
    return out


class Session:
    """The episode fed one state per tick (include/mbd_hip.h mbd_plan_mpc_open on a path-integral plan): ``tick(state)`` plans
    from it and returns dict(mean, rows, sigma: (start, end)); ``reset_mean`` makes the next tick cold, sigma included;
    ``sigma`` is what the next tick starts from."""

    def __init__(self, oenv, key, N, H, Nd, temp, K, E, method, sigma_cold=1.0, sigma_warm=1.0, gain=0.0, impl=1, plan_tick=plan_tick):
        self.oenv, self.rng = oenv, np.asarray(key, np.uint32)
        self.plan_tick = plan_tick
        self.cfg = (N, H, temp, method, impl)
        self.Nd, self.K, self.E = Nd, K, E
        self.rec = (sigma_cold, sigma_warm, gain)
        self.reset_mean()

    def reset_mean(self):
        self.mu = np.zeros((self.cfg[1], self.oenv.Nu), np.float32)
        self.n_it, self.sigma = self.Nd - 1, np.float32(self.rec[0])

    def tick(self, state):
        N, H, temp, method, impl = self.cfg
        keys = self.oenv.orc.split(self.rng, 2, impl)
        self.rng, r = keys[0], keys[1]
        s = np.ascontiguousarray(state, np.float32).reshape(-1)
        start = np.float32(self.sigma)
        _, M, end = self.plan_tick(self.oenv, s, r, self.mu, start, self.n_it, N, H, temp, method, impl)
        self.mu, self.n_it = shift(M, self.E), self.K
        self.sigma = next_sigma(end, *self.rec)
        return dict(mean=M, rows=M[: self.E].copy(), sigma=(start, np.float32(end)))
