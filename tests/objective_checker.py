"""The checker's restatement of the objective record (include/mbd_hip.h mbd_objective, DESIGN.md section 1 "N13 objective"): what
phase 1 of a diffusion step leaves in the rewards buffer in place of mean_H(rewss), in numpy float32 with every operation spelled
out and rounded — the products before the sums, no fused multiply-add, the sums in the contract's order (over h ascending; per
actuator over h, then over the actuators ascending).  ``ret``, ``cost`` and ``step`` are that pseudo-code; ``ObjectiveEnv`` hands
the shaped rewards to the existing checkers as a one-column array, in the manner of ensemble_checker.EnsembleEnv, with a mutable
previous action that ``episode`` sets per tick — the ticks themselves are mpc_online_checker's and mpc_pi_checker's sessions, the
executed rows mpc_checker's and mpc_plant_checker's functions."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

f32 = np.float32


@dataclass
class Record:
    """mbd_objective: row_weight [H] or None, act_weight [Nu] or None (ones), prev0 [Nu] or None, effort, rate."""
    row_weight: object = None
    effort: float = 0.0
    rate: float = 0.0
    act_weight: object = None
    prev0: object = None

    def kwargs(self):
        return dict(row_weight=self.row_weight, effort=self.effort, rate=self.rate, act_weight=self.act_weight, prev0=self.prev0)

    def costs(self):
        return f32(self.effort) != 0 or f32(self.rate) != 0


def clip(x):
    """clip(x, -1, 1) of a previous action; None stays None."""
    return None if x is None else np.clip(np.asarray(x, f32), f32(-1), f32(1)).astype(f32)


def wsum_of(w):
    """The f32 left-to-right sum of w, as the set call forms it."""
    acc = f32(0)
    for x in np.asarray(w, f32):
        acc = f32(acc + x)
    return acc


def ret(rewss, rews, w):
    """ret [B]: rews as the rollout stored it (w None), or acc / wsum with acc = +0; acc = acc + (w[h] * rewss[b][h]), h ascending."""
    rewss = np.asarray(rewss, f32)
    if w is None:
        return np.array(rews, f32)
    w = np.asarray(w, f32)
    acc = np.zeros(rewss.shape[0], f32)
    with np.errstate(all="ignore"):
        for h in range(rewss.shape[1]):
            acc = (acc + (w[h] * rewss[:, h]).astype(f32)).astype(f32)
        return (acc / wsum_of(w)).astype(f32)


def cost(Y, q, effort, rate, prev):
    """cost [N] of the candidates Y [N, H, Nu]: per actuator a over h ascending eff_a += u u and rat_a += (u - u_prev)^2 (u_prev =
    prev[a] at h = 0, the term left out when prev is None), then c += q[a] * ((effort * eff_a) + (rate * rat_a)) over a ascending
    from +0, and ONE division by float(H)."""
    Y = np.asarray(Y, f32)
    N, H, Nu = Y.shape
    q = np.ones(Nu, f32) if q is None else np.asarray(q, f32)
    effort, rate = f32(effort), f32(rate)
    c = np.zeros(N, f32)
    with np.errstate(all="ignore"):
        for a in range(Nu):
            eff, rat = np.zeros(N, f32), np.zeros(N, f32)
            up = None if prev is None else np.full(N, np.asarray(prev, f32)[a], f32)
            for h in range(H):
                u = Y[:, h, a]
                eff = (eff + (u * u).astype(f32)).astype(f32)
                if up is not None:
                    d = (u - up).astype(f32)
                    rat = (rat + (d * d).astype(f32)).astype(f32)
                up = u
            inner = ((effort * eff).astype(f32) + (rate * rat).astype(f32)).astype(f32)
            c = (c + (q[a] * inner).astype(f32)).astype(f32)
        return (c / f32(H)).astype(f32)


def step(rewss, rews, Y, rec: Record, prev):
    """(rews' [B], ret [B], cost [N]) of one step: rows b of rewss [B, H] are candidates b % N of Y [N, H, Nu]; ``prev`` is the
    clipped previous action or None.  With effort == rate == 0 the cost pass is skipped: cost is all +0 and rews' = ret."""
    r = ret(rewss, rews, rec.row_weight)
    N = np.shape(Y)[0]
    if not rec.costs():
        return r.copy(), r, np.zeros(N, f32)
    c = cost(Y, rec.act_weight, rec.effort, rec.rate, prev)
    with np.errstate(all="ignore"):
        out = (r - c[np.arange(r.shape[0]) % N]).astype(f32)
    return out, r, c


class Prev:
    """The previous action the envs of one plan share: clipped [Nu], or None."""

    def __init__(self, value=None):
        self.value = clip(value)


class ObjectiveEnv:
    """An OracleEnv (or a wrapper of one) whose ``rollout`` returns the SHAPED reward of every candidate as a one-column [B, 1]
    array — the checkers' mean over that column, (0 + r) / 1, is r itself.  ``rollout(state0, us)`` sees the candidates, so the
    cost is taken on exactly what was rolled out; everything else is the wrapped env's.  ``prev``: a ``Prev`` (shared between the
    members of an ensemble).  ``last``: (rews', ret, cost) of the last rollout."""

    def __init__(self, oenv, rec: Record, prev: Prev = None):
        self.oenv, self.rec = oenv, rec
        self.prev = Prev(rec.prev0) if prev is None else prev
        self.last = None

    def __getattr__(self, name):  # (orc, name, ms, Nu, xref, rew_xref, init_q, reset, logpd: the wrapped env's)
        return getattr(self.oenv, name)

    def rollout(self, state0, us, want_xpos=False):
        from oracle import planner as op
        out = self.oenv.rollout(state0, us, want_xpos=True) if want_xpos else self.oenv.rollout(state0, us)
        rewss = np.ascontiguousarray(out[0] if want_xpos else out, f32)
        self.last = step(rewss, op.mean_h(self.oenv.orc, rewss), us, self.rec, self.prev.value)
        shaped = self.last[0][:, None]
        return (shaped, out[1]) if want_xpos else shaped


def demo_episode(oenv, rec: Record, clip, c0, rew_xref, state0, key, N, H, Nd, temp, T, K, E, impl=1):
    """An episode of a demo plan under a demo record (tests/mpc_demo_checker.py: tick t plans under window_t of the clip and the
    record's reward level) AND the objective record: the log-densities are the window's, untouched; the blend runs on ret - cost."""
    import functools

    import mpc_demo_checker as mdc
    from oracle import planner as op

    def env_of_tick(t, prev):
        return ObjectiveEnv(mdc.windowed(oenv, mdc.window(clip, c0, t, E), rew_xref), rec, prev)

    return episode(oenv, rec, state0, key, N, H, Nd, temp, T, K, E, env_of_tick=env_of_tick, impl=impl,
                   reverse_once=functools.partial(op.reverse_once, enable_demo=True))


def plan(orc, oenv, rec: Record, state0, key, N, H, Nd, temp, impl=1, enable_demo=False, beta0=1e-4, betaT=1e-2, env=None):
    """A whole reverse loop from ``key`` (mbd_plan_run's) under the record: dict(mu_0ts, rew_means, rew_final (the env's own
    reward), last (the last step's rews', ret, cost))."""
    from oracle import planner as op
    sched = orc.schedule(beta0, betaT, Nd)
    oe = ObjectiveEnv(oenv, rec) if env is None else env
    r, Ybar = np.asarray(key, np.uint32), np.zeros((H, oenv.Nu), f32)
    mus, rms = [], []
    for i in range(Nd - 1, 0, -1):
        r, Ybar, rm, _ = op.reverse_once(orc, oe, state0, i, r, Ybar, sched, N, H, temp, impl, enable_demo)
        mus.append(Ybar)
        rms.append(rm)
    rew_final = op.mean_h(orc, np.ascontiguousarray(oenv.rollout(state0, Ybar[None])))[0]
    return dict(mu_0ts=np.stack(mus), rew_means=np.array(rms, f32), rew_final=rew_final, last=getattr(oe, "last", None))


def pi_plan(orc, oenv, rec: Record, state0, key, N, H, Nd, temp, method, impl=1):
    """mbd_plan_run of a path-integral plan under the record: dict(mu_0ts [Nd-1, H, Nu], last)."""
    import mpc_pi_checker as pic
    oe = ObjectiveEnv(oenv, rec)
    r, mu, sigma = np.asarray(key, np.uint32), np.zeros((H, oenv.Nu), f32), f32(1.0)
    mus = []
    for _ in range(Nd - 1):
        r, mu, sigma = pic.plan_tick(oe, state0, r, mu, sigma, 1, N, H, temp, method, impl)
        mus.append(mu)
    return dict(mu_0ts=np.stack(mus), last=oe.last)


def episode(oenv, rec: Record, state0, key, N, H, Nd, temp, T, K, E, D=0, rows0=None, plant=None, dkey=None, act_std=0.0,
            kick_std=0.0, kick_every=1, method=None, sigma=(1.0, 1.0, 0.0), env=None, prev=None, reset_at=(), env_of_tick=None, impl=1, **session_kw):
    """A closed-loop episode of T ticks under the record.  The previous action: in the first tick the clipped last row of the
    committed queue (D > 0), else clip(prev0) or none; afterwards clip(M_{t-1}[E-1]) — the commanded row, whatever a plant adds.
    ``env`` / ``prev``: an env that already wraps ObjectiveEnvs (an ensemble) and the ``Prev`` they share.  ``method``: a
    path-integral update (mpc_pi_checker.Session, no delay) instead of the MBD session.  ``reset_at``: ticks in front of which the
    mean is reset (a session's reset_mean: prev stays).  ``env_of_tick(t, prev)``: the env tick t plans with (a demo record: the tick's
    window wrapped in an ObjectiveEnv on the shared ``prev``; ``session_kw`` then carries a ``reverse_once`` with enable_demo; a
    weighting record: weighting_checker's ``reverse_once``, or its ``plan_tick`` for a path-integral session).  Returns dict(actions, rewards, states, means, last)."""
    import mpc_online_checker as online
    import mpc_pi_checker as pic
    from mpc_checker import execute
    from mpc_plant_checker import disturbances, kick, rows_of
    orc, Nu = oenv.orc, oenv.Nu
    if env_of_tick is not None:
        prev = Prev(rec.prev0)
        env = env_of_tick(0, prev)
    elif env is None:
        env = ObjectiveEnv(oenv, rec)
        prev = env.prev
    if method is None:
        sess = online.Session(env, key, N, H, Nd, temp, K, E, D, rows0, impl=impl, **session_kw)
    else:
        sess = pic.Session(env, key, N, H, Nd, temp, K, E, method, *sigma, impl=impl, **session_kw)
    prev.value = clip(sess.C.reshape(-1, Nu)[-1]) if D else clip(rec.prev0)
    plant = oenv if plant is None else plant
    dk = None if dkey is None else np.asarray(dkey, np.uint32)
    s = np.ascontiguousarray(state0, f32).reshape(-1)
    actions, rewards, states, means = [], [], [s], []
    for t in range(T):
        if t in reset_at:
            sess.reset_mean()
        if env_of_tick is not None:
            env = sess.oenv = env_of_tick(t, prev)
        o = sess.tick(s)
        M = o["mean"]
        rows = np.array(o.get("head", o["rows"]), f32)
        if dk is not None:
            dk, eps = disturbances(orc, dk, E, Nu, impl)
            rows = rows_of(rows, E, eps, act_std)
        rew, s = execute(plant, s, rows)
        s = np.asarray(s, f32).reshape(-1)
        if dk is not None and kick_std > 0 and (t + 1) % kick_every == 0:  # (mpc_plant_checker.episode's kick)
            s = kick(plant, s, (f32(kick_std) * eps[E * Nu:].astype(f32)).astype(f32))
        actions.append(rows)
        rewards.append(rew)
        states.append(s)
        means.append(M)
        prev.value = clip(M[E - 1])
    return dict(actions=np.concatenate(actions), rewards=np.concatenate(rewards), states=np.stack(states), means=np.stack(means),
                last=getattr(env, "last", None))
