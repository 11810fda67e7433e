"""The checker's restatement of the weighting record (include/mbd_hip.h mbd_weighting, DESIGN.md section 1 "N14 weighting"): how a
diffusion step turns the rewards buffer into weights when a record is in force, in numpy float32 with every operation spelled out
and rounded, the block reductions restated (``sumB`` / ``maxB``: 1024 partials in ascending index, a xor-butterfly over each
wavefront's 64, the 16 wavefront values in order) and ``exp_`` and the square root taken from the oracle's primitives
(``orc.sp_eval``).  The one fused operation of the contract — the squared deviations accumulate as acc = fma(d, d, acc), the score's
own — goes through the oracle's ``dot``: dot((d, 1, 0), (d, acc, 0)) = fma(d, d, fma(1, acc, 0 * 0)) = fma(d, d, acc).

``weigh`` is the contract; ``update`` is what the untouched downstream kernels make of given weights (the weighted mean in wsum64's
order with the score form, cem's selection), restated so that a step, a run and an episode can be checked with ``weigh`` standing
in the score's place; ``reverse_once`` is oracle.planner's step with that (same signature, same return value: it stands wherever
a checker takes a ``reverse_once``), ``run`` / ``episode`` the loops over it; ``pi_update`` / ``plan_tick`` are the path-integral
plans' update (cma-es' sigma from the given weights included) and mpc_pi_checker's tick with it."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

f32 = np.float32
B = 1024  # the score workgroup's threads


@dataclass(frozen=True)
class Record:
    """mbd_weighting."""
    reject_nonfinite: bool = True
    ess_frac: float = 0.0
    temp_min: float = 0.0
    temp_max: float = 0.0
    iters: int = 12

    def kwargs(self):
        return dict(reject_nonfinite=self.reject_nonfinite, ess_frac=self.ess_frac, temp_min=self.temp_min, temp_max=self.temp_max,
                    iters=self.iters)


def _fma(orc, a, b, c):
    """fma(a, b, c) elementwise, exactly: the oracle's dot((a, 1, 0), (b, c, 0)).  (c = -0 would enter as +0: no accumulator here
    is ever -0, they start at +0 and +0 + -0 = +0.)"""
    a, b, c = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32))
    rows = np.zeros((a.size, 6), f32)
    rows[:, 0], rows[:, 1], rows[:, 3], rows[:, 4] = a.reshape(-1), 1.0, b.reshape(-1), c.reshape(-1)
    return orc.sp_eval("dot", rows).reshape(a.shape)


def _sqrt(orc, x):
    """The correctly rounded square root (``sqrt_floor``: from 1e-30 up; its floor below only meets a zero variance, which the
    1e-4 guard replaces by 1 either way)."""
    return f32(orc.sp_eval("sqrt_floor", np.array([x], f32))[0])


def _reduce(part, op):
    """The 1024 partials -> one value: per wavefront the xor-butterfly (every lane takes op(own, lane ^ off's), off = 32 .. 1),
    then the 16 wavefront values combined in order."""
    x = part.reshape(B // 64, 64).copy()
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        x = op(x, x[:, lanes ^ off]).astype(f32)
    s = x[0, 0]
    for w in range(1, B // 64):
        s = f32(op(s, x[w, 0]))
    return f32(s)


def _add(a, b):
    return a + b


def _max(a, b):
    return np.where(a > b, a, b)


def _partials(x, keep, step, init):
    """partial t over its entries i = t, t + 1024, ... ascending: part = step(part, x[i]) where keep[i], unchanged where not."""
    part = np.full(B, init, f32)
    for k in range(0, x.shape[0], B):
        seg, kp = x[k:k + B], keep[k:k + B]
        m = seg.shape[0]
        part[:m] = np.where(kp, step(part[:m], seg).astype(f32), part[:m])
    return part


def sumB(x, keep):
    return _reduce(_partials(x, keep, _add, 0.0), _add)


def maxB(x, keep):
    return _reduce(_partials(x, keep, _max, -np.inf), _max)


def sumsq_devB(orc, x, keep, mean):
    def step(part, seg):
        d = (seg - mean).astype(f32)
        return _fma(orc, d, d, part)
    return _reduce(_partials(x, keep, step, 0.0), _add)


def weigh(orc, rews, T0, rec: Record = Record(reject_nonfinite=False)):
    """The contract.  Returns dict(weights [N], rew_mean, temp, ess, kept, branch) — branch: which arm of the selection chose the
    temperature ("fixed", "min", "max", "loop"; "none" with nothing kept)."""
    r = np.ascontiguousarray(rews, f32)
    N = r.shape[0]
    T0 = f32(T0)
    with np.errstate(all="ignore"):
        keep = np.isfinite(r) if rec.reject_nonfinite else np.ones(N, bool)
        kept = int(keep.sum())
        if kept == 0:
            return dict(weights=np.zeros(N, f32), rew_mean=f32(np.nan), temp=T0, ess=f32(0), kept=0, branch="none")
        mean = f32(sumB(r, keep) / f32(kept))
        sd = _sqrt(orc, f32(sumsq_devB(orc, r, keep, mean) / f32(kept)))
        if sd < f32(1e-4):
            sd = f32(1)
        z = ((r - mean).astype(f32) / sd).astype(f32)
        zmax = f32(f32(maxB(r, keep) - mean) / sd)

        def E(T):
            T = f32(T)
            x = ((z / T).astype(f32) - f32(zmax / T)).astype(f32)
            e = np.where(keep, orc.sp_eval("exp_", np.where(keep, x, f32(0))), f32(0)).astype(f32)
            S1, S2 = sumB(e, keep), sumB((e * e).astype(f32), keep)
            return e, S1, f32(f32(S1 * S1) / S2)

        if f32(rec.ess_frac) == 0:
            Ts, branch = T0, "fixed"
        else:
            target = f32(f32(rec.ess_frac) * f32(kept))
            tmin, tmax = f32(rec.temp_min), f32(rec.temp_max)
            if not E(tmin)[2] < target:
                Ts, branch = tmin, "min"
            elif not E(tmax)[2] > target:
                Ts, branch = tmax, "max"
            else:
                lo, hi = tmin, tmax
                for _ in range(int(rec.iters)):
                    mid = _sqrt(orc, f32(lo * hi))
                    if E(mid)[2] < target:
                        lo = mid
                    else:
                        hi = mid
                Ts, branch = hi, "loop"
        e, S1, ess = E(Ts)
        w = np.where(keep, (e / S1).astype(f32), f32(0)).astype(f32)
    return dict(weights=w, rew_mean=mean, temp=f32(Ts), ess=ess, kept=kept, branch=branch, target=None if branch == "fixed" else target)


# ---- downstream of the weights: the untouched kernels, restated for given weights ----------------------------------------------
def wmean(orc, w, Y0s):
    """sum_n w[n] Y0s[n] in wsum64's order: 64 partials, partial g a sequential fma over n = g, g + 64, ..., then added in g order."""
    Y = np.ascontiguousarray(Y0s, f32).reshape(Y0s.shape[0], -1)
    N, HNu = Y.shape
    part = np.zeros((64, HNu), f32)
    with np.errstate(all="ignore"):
        for n0 in range(0, N, 64):
            m = min(64, N - n0)
            part[:m] = _fma(orc, w[n0:n0 + m, None], Y[n0:n0 + m], part[:m])
        s = part[0].copy()
        for g in range(1, 64):
            s = (s + part[g]).astype(f32)
    return s


def score_form(orc, Ybar, Ybar_i, alpha_i, ab_i, ab_im1):
    """mbd_planner.py:100,130-133 on the weighted mean, operation by operation (the literal score form)."""
    a_i, ab_i, ab_im1 = f32(alpha_i), f32(ab_i), f32(ab_im1)
    sab = _sqrt(orc, ab_i)
    with np.errstate(all="ignore"):
        Yi = (np.asarray(Ybar_i, f32).reshape(-1) * sab).astype(f32)
        t1 = f32(f32(1) / f32(f32(1) - ab_i))
        t2 = (sab * Ybar).astype(f32)
        score = (t1 * (-Yi + t2).astype(f32)).astype(f32)
        t3 = (f32(f32(1) - ab_i) * score).astype(f32)
        Yim1 = (f32(f32(1) / _sqrt(orc, a_i)) * (Yi + t3).astype(f32)).astype(f32)
        return (Yim1 / _sqrt(orc, ab_im1)).astype(f32)


def cem_mean(w, Y0s, K=10):
    """argsort(weights)[::-1][:K] of a stable NaN-last sort (ties towards the higher index), then the sequential mean."""
    Y = np.ascontiguousarray(Y0s, f32).reshape(Y0s.shape[0], -1)
    key = np.where(np.isnan(w), np.inf, w)
    K = min(K, Y.shape[0])
    idx = sorted(range(Y.shape[0]), key=lambda n: (key[n], n), reverse=True)[:K]
    acc = np.zeros(Y.shape[1], f32)
    for n in idx:
        acc = (acc + Y[n]).astype(f32)
    return (acc / f32(K)).astype(f32)


def update(orc, method, w, Y0s, Ybar_i, sched=None, i=None, literal=True):
    """The new mean [H, Nu] from given weights: method 0 MBD (the score form on the weighted mean), 1 / 2 mppi / cma-es (the
    weighted mean), 3 cem."""
    shape = np.shape(Ybar_i)
    if method == 3:
        return cem_mean(w, Y0s).reshape(shape)
    m = wmean(orc, w, Y0s)
    if method == 0 and literal:
        alphas, alphas_bar, _ = sched
        m = score_form(orc, m, Ybar_i, alphas[i], alphas_bar[i], alphas_bar[i - 1])
    return m.reshape(shape)


def reverse_once(orc, env, state0, i, rng, Ybar_i, sched, N, H, T0, impl=1, enable_demo=False, literal=True, timers=None, *,
                 rec: Record = Record(reject_nonfinite=False), log=None):
    """oracle.planner.reverse_once with ``weigh`` in the score's place, in its signature and with its return value — (rng',
    Ybar_im1, rew_mean, details) — so that ``functools.partial(reverse_once, rec=..., log=...)`` stands wherever a checker takes a
    ``reverse_once`` (mpc_online_checker.Session, objective_checker.episode).  ``env`` is seen through ``.rollout`` only: an
    ObjectiveEnv, an EnsembleEnv, a plain OracleEnv.  ``log``: a list the step's (temp, ess, kept) is appended to."""
    from oracle import planner as op
    if enable_demo:
        raise ValueError("a weighting record is refused on demo plans")
    keys = orc.split(rng, 2, impl)
    rng, ks = keys[0], keys[1]
    Y0s = orc.sample(ks, impl, N, H, env.Nu, 0, N, float(sched[2][i]), Ybar_i)
    rewss = env.rollout(state0, Y0s)
    rews = op.mean_h(orc, np.ascontiguousarray(rewss))
    res = weigh(orc, rews, T0, rec)
    if log is not None:
        log.append((res["temp"], res["ess"], res["kept"]))
    out = update(orc, 0, res["weights"], Y0s, Ybar_i, sched, i, literal=literal)
    return rng, out, res["rew_mean"], dict(Y0s=Y0s, rewss=rewss, rews=rews, weights=res["weights"], res=res)


def run(orc, env, state0, key, N, H, Nd, T0, rec: Record, impl=1, beta0=1e-4, betaT=1e-2):
    """mbd_plan_run's loop from ``key``: dict(mu_0ts [Nd-1, H, Nu], rew_means [Nd-1], log [(temp, ess, kept)])."""
    sched = orc.schedule(beta0, betaT, Nd)
    r, Ybar = np.asarray(key, np.uint32), np.zeros((H, env.Nu), f32)
    mus, rms, log = [], [], []
    for i in range(Nd - 1, 0, -1):
        r, Ybar, rm, _ = reverse_once(orc, env, state0, i, r, Ybar, sched, N, H, T0, impl, rec=rec, log=log)
        mus.append(Ybar)
        rms.append(rm)
    return dict(mu_0ts=np.stack(mus), rew_means=np.array(rms, f32), log=log)


def ticks_of(log, Nd, K, T):
    """A flat episode log as one list per tick: Nd - 1 entries for the cold tick 0, K for every warm one."""
    cuts = np.cumsum([0, Nd - 1] + [K] * (T - 1))
    assert len(log) == cuts[-1], (len(log), cuts)
    return [log[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def episode(oenv, state0, key, N, H, Nd, T0, T, K, E, rec: Record, impl=1, beta0=1e-4, betaT=1e-2, **kw):
    """objective_checker.episode (mpc_online_checker's session tick by tick, mpc_checker's executed rows; no objective record
    unless ``kw`` brings an ``env`` that holds one) with ``reverse_once`` in the step's place; beside its results, ``log``: per
    tick the (temp, ess, kept) of the tick's steps.  ``kw``: D, rows0, plant, dkey, act_std, env, prev, orec (an objective
    record: objective_checker.Record)."""
    import functools

    import objective_checker as oc
    log = []
    orec = kw.pop("orec", None)
    if orec is None:
        orec = oc.Record()
        kw.setdefault("env", oenv)
        kw.setdefault("prev", oc.Prev())
    out = oc.episode(oenv, orec, state0, key, N, H, Nd, T0, T, K, E, impl=impl, beta0=beta0, betaT=betaT,
                     reverse_once=functools.partial(reverse_once, rec=rec, log=log), **kw)
    out["log"] = ticks_of(log, Nd, K, T)
    return out


# ---- path-integral plans under a record ------------------------------------------------------------------------------------------
def _wave_sum(part):
    """One wavefront's xor-butterfly sum of 64 partials (lane 0's value)."""
    x = np.asarray(part, f32).copy()
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        x = (x + x[lanes ^ off]).astype(f32)
    return f32(x[0])


def cma_sigma(orc, w, Y0s, mu, sigma):
    """cma_spread_kernel and cma_sigma_kernel restated for given weights: s[e] = sqrt(acc), acc = fma(w[n], d * d, acc) over n
    ascending from +0 with d = Y0s[n][e] - mu[e] and d * d rounded; part[t] = sum of s[i], i = t, t + 64, ...; the wavefront's
    butterfly; / HNu, * sigma, and max(., 1e-3) as ``sig < 1e-3 ? 1e-3 : sig``, which keeps a NaN."""
    Y = np.ascontiguousarray(Y0s, f32).reshape(np.shape(Y0s)[0], -1)
    m = np.asarray(mu, f32).reshape(-1)
    HNu = Y.shape[1]
    with np.errstate(all="ignore"):
        acc = np.zeros(HNu, f32)
        for n in range(Y.shape[0]):
            d = (Y[n] - m).astype(f32)
            acc = _fma(orc, w[n], (d * d).astype(f32), acc)
        s = np.sqrt(acc).astype(f32)
        part = np.zeros(64, f32)
        for i0 in range(0, HNu, 64):
            seg = s[i0:i0 + 64]
            part[:seg.shape[0]] = (part[:seg.shape[0]] + seg).astype(f32)
        sig = f32(f32(_wave_sum(part) / f32(HNu)) * f32(sigma))
        return f32(1e-3) if sig < f32(1e-3) else sig


def pi_update(orc, method, res, Y0s, mu, sigma):
    """What a path-integral plan makes of ``weigh``'s result ``res``: (the new mean — ``update`` —, sigma: cma-es' new one,
    otherwise the one given)."""
    out = update(orc, int(method), res["weights"], Y0s, mu)
    if int(method) == 2:
        return out, cma_sigma(orc, res["weights"], Y0s, mu, sigma)
    return out, f32(sigma)


def plan_tick(oenv, s_plan, r, mu, sigma, n_it, N, H, temp, method, impl=1, *, rec: Record = Record(reject_nonfinite=False), log=None):
    """mpc_pi_checker.plan_tick with ``weigh`` and ``pi_update`` in orc.pi_update's place.  ``log``: a list every refinement's
    (temp, ess, kept) is appended to."""
    import mpc_pi_checker as pic

    def upd(orc, m, rews, Y0s, mu_t, sig, T0):
        res = weigh(orc, rews, T0, rec)
        if log is not None:
            log.append((res["temp"], res["ess"], res["kept"]))
        return pi_update(orc, m, res, Y0s, mu_t, sig)

    return pic.plan_tick(oenv, s_plan, r, mu, sigma, n_it, N, H, temp, method, impl, update=upd)
