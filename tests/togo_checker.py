"""The checker's restatement of a to-go record (include/mbd_hip.h mbd_togo, DESIGN.md section 1 "N19 to-go"): numpy float32 for the
group layout and the descending returns, and the oracle as it stands for everything else — the rows of group j are the rows of
``Oracle.score_update`` (MBD) or ``Oracle.pi_update(1, ...)`` (mppi) called with R_j in place of the rewards.

``TogoOracle`` wraps an ``Oracle``: its ``rollout`` / ``car2d_rollout`` remember the rewards per step they return, and its
``score_update`` / ``pi_update`` are the per-group update over what the last rollout left.  oracle.planner.reverse_once,
tests/mpc_checker.py, mpc_pi_checker.py, mpc_online_checker.py, mpc_plant_checker.py, mpc_delay_checker.py and the noise wrappers
run unchanged on top of it (``togo_env``): they reach rollouts and updates through ``oenv.orc``."""
from __future__ import annotations

import copy

import numpy as np

f32 = np.float32


def groups(H, block, min_tail):
    """The groups' first rows: s_0 = 0 and s_j = j * block for every j >= 1 with s_j < H and H - s_j >= min_tail."""
    starts = [0]
    j = 1
    while j * block < H:
        if H - j * block >= min_tail:
            starts.append(j * block)
        j += 1
    return np.array(starts, np.int32)


def returns(rews, rewss, starts):
    """R [G, N]: R_0 = rews; for the other groups one descending float32 pass per candidate, acc = +0, acc = acc + rewss[n][t] for
    t = H - 1 down to s_1, R_j[n] = acc / float32(H - s_j) whenever t == s_j.  Nothing is skipped."""
    rewss = np.asarray(rewss, f32)
    N, H = rewss.shape
    R = np.zeros((len(starts), N), f32)
    R[0] = np.asarray(rews, f32)
    if len(starts) < 2:
        return R
    where = {int(s): j for j, s in enumerate(starts) if j}
    acc = np.zeros(N, f32)
    with np.errstate(all="ignore"):
        for t in range(H - 1, int(starts[1]) - 1, -1):
            acc = (acc + rewss[:, t]).astype(f32)
            if t in where:
                R[where[t]] = (acc / f32(H - t)).astype(f32)
    return R


def update(orc, method, rews, rewss, Y0s, Ybar_i, starts, temp, alphas=None, literal=True, sigma=1.0):
    """One step's update under the record: dict(out [H, Nu], R, W [G, N], rew_mean, sigma).  ``method`` 0: ``orc.score_update``
    with ``alphas`` = (alpha_i, alpha_bar_i, alpha_bar_im1); 1: ``orc.pi_update(1, ...)``.  One call per group with R_j; the call's
    rows [s_j, s_{j+1}) are kept.  rew_mean is group 0's call's: the mean of ``rews``."""
    Ybar_i = np.asarray(Ybar_i, f32)
    H = Ybar_i.shape[0]
    R = returns(rews, rewss, starts)
    out, W = np.zeros_like(Ybar_i), np.zeros_like(R)
    mean = sig_out = None
    ends = list(starts[1:]) + [H]
    for j, (a, b) in enumerate(zip(starts, ends)):
        if method == 0:
            o, w, m = orc.score_update(R[j], Y0s, Ybar_i, *[float(x) for x in alphas], temp, literal=literal)
            sg = sigma
        else:
            o, sg, w, m = orc.pi_update(1, R[j], Y0s, Ybar_i, float(sigma), temp)
        out[a:b], W[j] = np.asarray(o, f32).reshape(Ybar_i.shape)[a:b], w
        if j == 0:
            mean, sig_out = m, sg
    return dict(out=out, R=R, W=W, rew_mean=mean, sigma=sig_out)


class TogoOracle:
    """An oracle whose update is the record's; everything else is the oracle's.  ``steps``: every update's dict(R, W)."""

    def __init__(self, orc, block, min_tail=1):
        self._orc, self.block, self.min_tail = orc, int(block), int(min_tail)
        self.rewss = None
        self.steps = []

    def __getattr__(self, name):
        return getattr(self._orc, name)

    def _keep(self, out):
        self.rewss = np.array(out[0] if isinstance(out, tuple) else out, f32)
        return out

    def rollout(self, *a, **kw):
        return self._keep(self._orc.rollout(*a, **kw))

    def car2d_rollout(self, *a, **kw):
        return self._keep(self._orc.car2d_rollout(*a, **kw))

    def _update(self, method, rews, Y0s, Ybar_i, temp, **kw):
        assert self.rewss is not None and self.rewss.shape[0] == len(rews), "the update follows the candidates' rollout"
        res = update(self._orc, method, rews, self.rewss, Y0s, Ybar_i, groups(self.rewss.shape[1], self.block, self.min_tail), temp, **kw)
        self.steps.append(dict(R=res["R"], W=res["W"]))
        return res

    def score_update(self, rews, Y0s, Ybar_i, alpha_i, ab_i, ab_im1, temp, lp_demo=None, rew_xref=0.0, literal=True):
        assert lp_demo is None, "a to-go record is refused on demo plans"
        res = self._update(0, rews, Y0s, Ybar_i, temp, alphas=(alpha_i, ab_i, ab_im1), literal=literal)
        return res["out"], res["W"][0], res["rew_mean"]

    def pi_update(self, method, rews, Y0s, mu_t, sigma, temp):
        assert method == 1, "a to-go record takes MBD and mppi plans"
        res = self._update(1, rews, Y0s, mu_t, temp, sigma=sigma)
        return res["out"], res["sigma"], res["W"][0], res["rew_mean"]


def togo_env(oenv, block, min_tail=1):
    """A copy of the OracleEnv whose ``orc`` is a ``TogoOracle`` around the env's own."""
    e = copy.copy(oenv)
    e.orc = TogoOracle(oenv.orc, block, min_tail)
    return e


def run(oenv, state0, key, N, H, Nd, temp, block, min_tail=1, method=0, impl=1, beta0=1e-4, betaT=1e-2, wrap=None, step=None):
    """mbd_plan_run's loop under the record from ``key``: dict(mu_0ts [Nd-1, H, Nu], rew_means [Nd-1], steps — every step's dict(R,
    W) —, details — every step's (MBD)).  ``wrap``: a function env -> env around the record's env (a noise shape or basis: the
    sampler's wrappers); ``step``: a stand-in for oracle.planner.reverse_once with its signature (an elite record's)."""
    from oracle import planner as op
    env = togo_env(oenv, block, min_tail)
    torc = env.orc
    if wrap is not None:
        env = wrap(env)
    orc = env.orc
    r = np.asarray(key, np.uint32)
    mus, rms, details = [], [], []
    if method == 0:
        sched = orc.schedule(beta0, betaT, Nd)
        Ybar = np.zeros((H, oenv.Nu), f32)
        for i in range(Nd - 1, 0, -1):
            r, Ybar, rm, d = (step or op.reverse_once)(orc, env, state0, i, r, Ybar, sched, N, H, temp, impl)
            mus.append(Ybar)
            rms.append(rm)
            details.append(d)
    else:
        import mpc_pi_checker as pic
        mu, sigma = np.zeros((H, oenv.Nu), f32), f32(1.0)

        def upd(o, m, rews, Y0s, mu_t, sig, T0):
            out, sg, _, rm = o.pi_update(m, rews, Y0s, mu_t, float(sig), T0)
            rms.append(rm)
            details.append(dict(rews=np.asarray(rews, f32), Y0s=Y0s))
            return out, sg

        for _ in range(Nd - 1):
            r, mu, sigma = pic.plan_tick(env, state0, r, mu, sigma, 1, N, H, temp, method, impl, update=upd)
            mus.append(mu)
    return dict(mu_0ts=np.stack(mus), rew_means=np.array(rms, f32), steps=torc.steps, details=details)


def episode(oenv, state0, key, N, H, Nd, temp, T, K, E, block, min_tail=1, method=0, sigma=(1.0, 1.0, 0.0), impl=1, wrap=None,
            checker_episode=None, **kw):
    """A closed-loop episode of T ticks under the record: tests/mpc_checker.episode (MBD), tests/mpc_pi_checker.episode (mppi under
    the sigma record ``sigma``) or ``checker_episode`` — mpc_plant_checker.episode, mpc_delay_checker.episode — over the record's env;
    ``kw`` goes to it.  Returns its dict plus ``steps``."""
    env = togo_env(oenv, block, min_tail)
    torc = env.orc
    if wrap is not None:
        env = wrap(env)
    if checker_episode is not None:
        out = checker_episode(env, state0, key, N, H, Nd, temp, T, K, E, **kw)
    elif method == 0:
        import mpc_checker
        out = mpc_checker.episode(env, state0, key, N, H, Nd, temp, T, K, E, impl=impl, **kw)
    else:
        import mpc_pi_checker as pic
        out = pic.episode(env, state0, key, N, H, Nd, temp, T, K, E, method, *sigma, impl=impl, **kw)
    return dict(out, steps=torc.steps)


def session(oenv, key, N, H, Nd, temp, K, E, block, min_tail=1, method=0, sigma=(1.0, 1.0, 0.0), impl=1):
    """The episode fed one state per tick: mpc_online_checker.Session (MBD) or mpc_pi_checker.Session (mppi) over the record's env."""
    env = togo_env(oenv, block, min_tail)
    if method == 0:
        import mpc_online_checker as online
        return online.Session(env, key, N, H, Nd, temp, K, E, impl=impl)
    import mpc_pi_checker as pic
    return pic.Session(env, key, N, H, Nd, temp, K, E, method, *sigma, impl=impl)
