"""The checker's restatement of the adapt record (include/mbd_hip.h mbd_adapt, DESIGN.md section 1 "N17 adapt"): how a diffusion step
rewrites the table ``a`` its successor samples under, in numpy float32 with every operation spelled out and rounded.  The two fused
operations of the contract — m1 = fma(w, d, m1), m2 = fma(w, d * d, m2) — go through the oracle's ``dot`` (weighting_checker._fma),
the square roots through the oracle's ``sqrt_floor`` where it is the plain square root (from 1e-30 up; below, numpy's, which is
IEEE's), divisions and products through numpy's float32.

``update`` is the contract.  ``State`` is the table as a plan carries it through runs, ticks and sessions; ``AdaptOracle`` wraps an
oracle so that ``sample`` draws under G = a * g (noise_shape_checker / noise_basis_checker form the candidates) and remembers what
the step sampled with; ``reverse_once`` and ``plan_tick`` are weighting_checker's with the update behind them, so that ``run``,
``episode`` and the sessions of the existing checkers run unchanged on top."""
from __future__ import annotations

import copy
from dataclasses import dataclass

import numpy as np

import weighting_checker as wc

f32 = np.float32
G64 = 64  # the groups of wsum64


@dataclass(frozen=True)
class Record:
    """mbd_adapt."""
    rate: float = 0.3
    a_min: float = 0.25
    a_max: float = 4.0
    carry: bool = True

    def kwargs(self):
        return dict(rate=self.rate, a_min=self.a_min, a_max=self.a_max, carry=self.carry)


def _sqrt(orc, x):
    x = np.ascontiguousarray(x, f32)
    flat = x.reshape(-1)
    with np.errstate(all="ignore"):
        small = flat < f32(1e-30)
        out = np.where(small, np.sqrt(flat), orc.sp_eval("sqrt_floor", np.where(small, f32(1), flat).astype(f32))).astype(f32)
    return out.reshape(x.shape)


def values(z, sigma, ybar):
    """A lazy plan's candidates from its shaped normals z [N, HNu]: clip((z * sigma) + Ybar, -1, 1), NaN passed through."""
    with np.errstate(all="ignore"):
        y = (np.asarray(z, f32) * f32(sigma)).astype(f32)
        y = (y + np.asarray(ybar, f32).reshape(1, -1)).astype(f32)
        return np.ascontiguousarray(np.clip(y, f32(-1), f32(1)), f32)


def moments(orc, w, Y, ybar):
    """(m1, m2) [HNu] in wsum64's order: 64 groups, group k a sequential fma chain over n = k, k + 64, ... from +0, the 64 partials
    added in group order."""
    Y = np.ascontiguousarray(Y, f32).reshape(np.shape(Y)[0], -1)
    w = np.ascontiguousarray(w, f32)
    N, HNu = Y.shape
    yb = np.asarray(ybar, f32).reshape(1, HNu)
    p1, p2 = np.zeros((G64, HNu), f32), np.zeros((G64, HNu), f32)
    with np.errstate(all="ignore"):
        for n0 in range(0, N, G64):
            m = min(G64, N - n0)
            d = (Y[n0:n0 + m] - yb).astype(f32)
            p1[:m] = wc._fma(orc, w[n0:n0 + m, None], d, p1[:m])
            p2[:m] = wc._fma(orc, w[n0:n0 + m, None], (d * d).astype(f32), p2[:m])
        m1, m2 = p1[0].copy(), p2[0].copy()
        for k in range(1, G64):
            m1 = (m1 + p1[k]).astype(f32)
            m2 = (m2 + p2[k]).astype(f32)
    return m1, m2


def update(orc, w, Y, ybar, sigma, a, g, rec: Record):
    """The contract: dict(a [HNu], G [HNu], S, skipped, s [HNu], active [HNu]) from the step's weights w [N], candidate VALUES Y
    [N, HNu], Ybar_i, the sigma it sampled with, the table ``a`` and the caller's shape ``g`` in force (None: none)."""
    a = np.ascontiguousarray(a, f32).reshape(-1)
    HNu = a.shape[0]
    gg = None if g is None else np.ascontiguousarray(g, f32).reshape(-1)
    with np.errstate(all="ignore"):
        G = a.copy() if gg is None else (a * gg).astype(f32)
        m1, m2 = moments(orc, w, Y, ybar)
        var = (m2 - (m1 * m1).astype(f32)).astype(f32)
        var = np.where(var < 0, f32(0), var).astype(f32)  # (a NaN stays)
        active = G > 0
        den = (f32(sigma) * G).astype(f32)
        s = np.where(active, (_sqrt(orc, var) / np.where(active, den, f32(1))).astype(f32), f32(0)).astype(f32)
        acc, n_active = f32(0), 0
        for e in range(HNu):
            if active[e]:
                acc = f32(acc + f32(s[e] * s[e]))
                n_active += 1
        S = _sqrt(orc, np.array([f32(acc / f32(n_active))], f32))[0] if n_active else f32(np.nan)
        skipped = n_active == 0 or not (S > 0) or not np.isfinite(S)
        a2 = a.copy()
        if not skipped:
            t = (a * (s / S).astype(f32)).astype(f32)
            v = (a + (f32(rec.rate) * (t - a).astype(f32)).astype(f32)).astype(f32)
            v = np.where(v < f32(rec.a_min), f32(rec.a_min), np.where(v > f32(rec.a_max), f32(rec.a_max), v)).astype(f32)
            a2 = np.where(active, v, a).astype(f32)
        G2 = a2.copy() if gg is None else (a2 * gg).astype(f32)
    return dict(a=a2, G=G2, S=f32(S), skipped=bool(skipped), s=s, active=active)


class State:
    """The table as a plan carries it.  ``g_always`` / ``g_warm``: the caller's shape in force outside / inside warm ticks (None:
    none; a shape set MBD_NOISE_WARM_TICKS has g_always None).  ``W``: a noise basis in force throughout, or None.  ``log``: one
    (S, skipped) per update; ``tables``: ``a`` after each update."""

    def __init__(self, rec: Record, H, Nu, g_always=None, g_warm=None, W=None):
        self.rec, self.H, self.Nu = rec, H, Nu
        self.g_always = None if g_always is None else np.ascontiguousarray(g_always, f32).reshape(-1)
        self.g_warm = None if g_warm is None else np.ascontiguousarray(g_warm, f32).reshape(-1)
        self.W = W
        self.log, self.tables = [], []
        self.reset(warm=False)

    def _form(self):
        with np.errstate(all="ignore"):
            self.G = self.a.copy() if self.g is None else (self.a * self.g).astype(f32)

    def reset(self, warm=False):
        """a = ones (a run, a cold tick, reset_mean, a tick without carry) under the shape of that kind of tick."""
        self.a = np.ones(self.H * self.Nu, f32)
        self.g = self.g_warm if warm else self.g_always
        self._form()

    def tick(self, cold, E):
        """The launch in front of a tick's first step."""
        if cold or not self.rec.carry:
            self.reset(warm=not cold)
            return
        sh = E * self.Nu
        self.a = np.concatenate([self.a[sh:], np.ones(sh, f32)]).astype(f32)
        self.g = self.g_warm
        self._form()

    def step(self, orc, w, Y0s, ybar, sigma):
        res = update(orc, w, np.ascontiguousarray(Y0s, f32).reshape(np.shape(Y0s)[0], -1), np.asarray(ybar, f32).reshape(-1), sigma,
                     self.a, self.g, self.rec)
        self.a, self.G = res["a"], res["G"]
        self.log.append((res["S"], res["skipped"]))
        self.tables.append(self.a.copy())
        return res


class AdaptOracle:
    """An oracle whose ``sample`` draws under the state's G (and basis); everything else is the oracle's."""

    def __init__(self, orc, state: State):
        self._orc, self.state = orc, state

    def __getattr__(self, name):
        return getattr(self._orc, name)

    def sample(self, key, impl, N, H, Nu, begin, count, sigma, Ybar, want_eps=False):
        from noise_basis_checker import BasisOracle
        st = self.state
        return BasisOracle(self._orc, st.W, st.G).sample(key, impl, N, H, Nu, begin, count, sigma, Ybar, want_eps=want_eps)


def adapt_env(oenv, state: State):
    """A copy of the env whose ``orc`` samples under the state's table."""
    e = copy.copy(oenv)
    e.orc = AdaptOracle(oenv.orc, state)
    return e


def reverse_once(orc, env, state0, i, rng, Ybar_i, sched, N, H, T0, impl=1, enable_demo=False, literal=True, timers=None, *,
                 state: State, rec: wc.Record = wc.Record(reject_nonfinite=False), log=None):
    """weighting_checker.reverse_once (the score without a record where ``rec`` is its default) sampling under the state's table,
    then the update from the step's weights, candidates, Ybar_i and sigma_i.  ``functools.partial(reverse_once, state=...)`` stands
    wherever a checker takes a ``reverse_once``."""
    base = getattr(orc, "_orc", orc)
    out = wc.reverse_once(AdaptOracle(base, state), env, state0, i, rng, Ybar_i, sched, N, H, T0, impl, enable_demo, literal, timers,
                          rec=rec, log=log)
    d = out[3]
    state.step(base, d["weights"], d["Y0s"], Ybar_i, f32(sched[2][i]))
    return out


def run(orc, env, state0, key, N, H, Nd, T0, state: State, rec: wc.Record = wc.Record(reject_nonfinite=False), impl=1, beta0=1e-4,
        betaT=1e-2):
    """mbd_plan_run's loop under the record: dict(mu_0ts, rew_means, log (a weighting record's))."""
    sched = orc.schedule(beta0, betaT, Nd)
    state.reset()
    r, Ybar = np.asarray(key, np.uint32), np.zeros((H, env.Nu), f32)
    mus, rms, log = [], [], []
    for i in range(Nd - 1, 0, -1):
        r, Ybar, rm, _ = reverse_once(orc, env, state0, i, r, Ybar, sched, N, H, T0, impl, state=state, rec=rec, log=log)
        mus.append(Ybar)
        rms.append(rm)
    return dict(mu_0ts=np.stack(mus), rew_means=np.array(rms, f32), log=log)


def plan_tick(oenv, s_plan, r, mu, sigma, n_it, N, H, temp, method, impl=1, *, state: State,
              rec: wc.Record = wc.Record(reject_nonfinite=False), log=None):
    """mpc_pi_checker.plan_tick for an mppi plan sampling under the state's table, the update behind every refinement (the sigma it
    sampled with: the carried one)."""
    import mpc_pi_checker as pic
    base = oenv.orc
    env = adapt_env(oenv, state)

    def upd(orc, m, rews, Y0s, mu_t, sig, T0):
        res = wc.weigh(base, rews, T0, rec)
        if log is not None:
            log.append((res["temp"], res["ess"], res["kept"]))
        out = wc.pi_update(base, m, res, Y0s, mu_t, sig)
        state.step(base, res["weights"], Y0s, mu_t, f32(sig))
        return out

    return pic.plan_tick(env, s_plan, r, mu, sigma, n_it, N, H, temp, method, impl, update=upd)


def pi_run(oenv, state0, key, N, H, Nd, temp, method, state: State, impl=1, rec: wc.Record = wc.Record(reject_nonfinite=False)):
    """mbd_plan_run of an mppi plan under the record: dict(mu_0ts [Nd-1, H, Nu])."""
    state.reset()
    r, mu, sigma = np.asarray(key, np.uint32), np.zeros((H, oenv.Nu), f32), f32(1.0)
    mus = []
    for _ in range(Nd - 1):
        r, mu, sigma = plan_tick(oenv, state0, r, mu, sigma, 1, N, H, temp, method, impl, state=state, rec=rec)
        mus.append(mu)
    return dict(mu_0ts=np.stack(mus))


class Session:
    """mpc_online_checker.Session (an MBD plan's; ``method`` None) or mpc_pi_checker.Session (mppi under a sigma record) with the
    table carried across ticks: in front of every tick the state's ``tick``, ``reset_mean`` resets it as well.  ``tick`` returns the
    inner session's dict plus ``a`` [H, Nu], the table behind the tick."""

    def __init__(self, oenv, key, N, H, Nd, temp, K, E, state: State, D=0, rows0=None, method=None, sigma=(1.0, 1.0, 0.0), impl=1,
                 rec: wc.Record = wc.Record(reject_nonfinite=False)):
        import functools

        import mpc_online_checker as online
        import mpc_pi_checker as pic
        self.state, self.E = state, E
        if method is None:
            self.inner = online.Session(oenv, key, N, H, Nd, temp, K, E, D, rows0, impl=impl,
                                        reverse_once=functools.partial(reverse_once, state=state, rec=rec))
        else:
            self.inner = pic.Session(oenv, key, N, H, Nd, temp, K, E, method, *sigma, impl=impl,
                                     plan_tick=functools.partial(plan_tick, state=state, rec=rec))
        self.cold = True
        state.reset()

    def reset_mean(self):
        self.inner.reset_mean()
        self.cold = True
        self.state.reset()

    def tick(self, x):
        self.state.tick(self.cold, self.E)
        out = dict(self.inner.tick(x))
        self.cold = False
        out["a"] = self.state.a.reshape(self.state.H, self.state.Nu).copy()
        return out


def episode(oenv, state0, key, N, H, Nd, temp, T, K, E, state: State, D=0, rows0=None, method=None, sigma=(1.0, 1.0, 0.0), impl=1,
            rec: wc.Record = wc.Record(reject_nonfinite=False), pick_mask=None):
    """A closed-loop episode of T ticks under the record: the session above fed the states the env itself reaches by executing each
    tick's rows (the queue's head under a delay record).  ``pick_mask``: a pick record (mpc_pick_checker.pick on the tick's result;
    MBD plans without a delay).  Returns dict(actions, rewards, states, means, tables [T, H, Nu] — ``a`` behind every tick)."""
    import mpc_pick_checker as pk
    from mpc_checker import execute, shift
    sess = Session(oenv, key, N, H, Nd, temp, K, E, state, D, rows0, method, sigma, impl, rec)
    s = np.ascontiguousarray(state0, f32).reshape(-1)
    actions, rewards, states, means, tables = [], [], [s], [], []
    if pick_mask is not None:
        assert method is None and D == 0
        last = {}
        inner_step = sess.inner.reverse_once

        def step(*a, **kw):
            out = inner_step(*a, **kw)
            last.update(out[3])
            return out
        sess.inner.reverse_once = step
    for t in range(T):
        cold = sess.cold
        B = sess.inner.Ybar if method is None else None
        o = sess.tick(s)
        M = o["mean"]
        if pick_mask is not None:
            M, _, _, _, _ = pk.pick(oenv, s, M, B, cold, last["rews"], last["Y0s"], pick_mask)
            sess.inner.Ybar = shift(M, E)
        rows = np.array(o.get("head", o["rows"]) if pick_mask is None else M[:E], f32)
        rew, s = execute(oenv, s, rows)
        s = np.asarray(s, f32).reshape(-1)
        actions.append(rows)
        rewards.append(rew)
        states.append(s)
        means.append(M)
        tables.append(o["a"])
    return dict(actions=np.concatenate(actions), rewards=np.concatenate(rewards), states=np.stack(states), means=np.stack(means),
                tables=np.stack(tables))
