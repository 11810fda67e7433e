"""The checker's restatement of planning over an ensemble of perturbed models (include/mbd_hip.h mbd_ensemble, DESIGN.md
section 1 "N6 ensemble"): one set of candidates per diffusion step, rolled out on M OracleEnvs, the M mean returns combined
per candidate — left to right in numpy float32, the mean with ONE division — and the oracle's score update on the result.
``step`` is that pseudo-code spelled out; ``EnsembleEnv`` hands the same combined rewards to the existing checkers
(oracle.planner.reverse_once, tests/mpc_checker.py, tests/mpc_plant_checker.py), so whole plans and episodes reuse them."""
from __future__ import annotations

import numpy as np

from oracle import planner as op

RISK_MEAN, RISK_MIN = "mean", "min"


def member_rewards(orc, members, state0, Y0s):
    """r_m[n] = mean_H(rollout_{member m}(state0, Y0s[n])): [M, N] float32."""
    return np.stack([op.mean_h(orc, np.ascontiguousarray(m.rollout(state0, Y0s))) for m in members])


def combine(r, risk):
    """[M, N] -> [N]: ((r_0 + r_1) + ... + r_{M-1}) / float32(M), or min(min(r_0, r_1), ...) — NaN wins: float32, left to right."""
    r = np.asarray(r, np.float32)
    acc = r[0].copy()
    for m in range(1, r.shape[0]):
        if risk == RISK_MIN:  # min(a, b) = b if b < a or b is NaN, else a: a NaN return wins (include/mbd_hip.h)
            with np.errstate(invalid="ignore"):
                acc = np.where((r[m] < acc) | np.isnan(r[m]), r[m], acc).astype(np.float32)
        else:
            acc = (acc + r[m]).astype(np.float32)
    if risk == RISK_MIN:
        return acc
    if risk != RISK_MEAN:
        raise ValueError(f"risk={risk!r}")
    return (acc / np.float32(r.shape[0])).astype(np.float32)


def step(orc, oenv, members, risk, state0, i, rng, Ybar_i, sched, N, H, temp, impl=1, literal=True):
    """One diffusion step with an ensemble record.  ``members``: the M OracleEnvs (None: oenv itself).  Returns
    (rng', Ybar_im1, rew_mean, dict(Y0s, r_members [M, N], rews [N], weights [N]))."""
    members = [oenv if m is None else m for m in members]
    alphas, alphas_bar, sigmas = sched
    keys = orc.split(rng, 2, impl)  # rng, Y0s_rng = split(rng): ONE set of normals and candidates
    rng, ks = keys[0], keys[1]
    Y0s = orc.sample(ks, impl, N, H, oenv.Nu, 0, N, float(sigmas[i]), Ybar_i)
    r = member_rewards(orc, members, state0, Y0s)
    rews = combine(r, risk)
    Ybar_im1, w, rew_mean = orc.score_update(rews, Y0s, Ybar_i, float(alphas[i]), float(alphas_bar[i]),
                                             float(alphas_bar[i - 1]), temp, lp_demo=None, rew_xref=oenv.rew_xref,
                                             literal=literal)
    return rng, Ybar_im1, rew_mean, dict(Y0s=Y0s, r_members=r, rews=rews, weights=w)


class EnsembleEnv:
    """An OracleEnv whose ``rollout`` returns the COMBINED reward of every candidate as a one-column [N, 1] array — the
    checkers' mean over that column, (0 + r) / 1, is r itself — so that oracle.planner.reverse_once and the episode checkers
    score candidates by the ensemble while everything else (the env's name, model, action size, the rows an episode
    executes through ``orc.rollout(ms, ...)``) stays the plan's own env's."""

    def __init__(self, oenv, members, risk):
        self.oenv, self.members, self.risk = oenv, [oenv if m is None else m for m in members], risk
        self.orc, self.name, self.ms, self.Nu = oenv.orc, oenv.name, oenv.ms, oenv.Nu
        self.xref, self.rew_xref, self.init_q = oenv.xref, oenv.rew_xref, oenv.init_q

    def reset(self, key, impl):
        return self.oenv.reset(key, impl)

    def rollout(self, state0, us, want_xpos=False):
        if want_xpos:
            raise ValueError("an ensemble has no demo log-density")
        return combine(member_rewards(self.orc, self.members, state0, us), self.risk)[:, None]


def plan(orc, oenv, members, risk, state0, key, N, H, Nd, temp, impl=1, beta0=1e-4, betaT=1e-2):
    """A whole reverse loop from ``key`` (mbd_plan_run's): dict(mu_0ts [Nd-1, H, Nu], rew_means [Nd-1], rew_final) — the final
    reward on the plan's OWN env."""
    sched = orc.schedule(beta0, betaT, Nd)
    ee = EnsembleEnv(oenv, members, risk)
    r, Ybar = np.asarray(key, np.uint32), np.zeros((H, oenv.Nu), np.float32)
    mus, rms = [], []
    for i in range(Nd - 1, 0, -1):
        r, Ybar, rm, _ = op.reverse_once(orc, ee, state0, i, r, Ybar, sched, N, H, temp, impl)
        mus.append(Ybar)
        rms.append(rm)
    rew_final = op.mean_h(orc, np.ascontiguousarray(oenv.rollout(state0, Ybar[None])))[0]
    return dict(mu_0ts=np.stack(mus), rew_means=np.array(rms, np.float32), rew_final=rew_final)


def episode(oenv, members, risk, state0, key, N, H, Nd, temp, T, K, E, plant=None, **plant_kw):
    """A closed-loop episode planned with the ensemble: tests/mpc_checker.episode, or with a plant / disturbances
    (``plant``, dkey, act_std, kick_std, kick_every) tests/mpc_plant_checker.episode — the executed rows go through the
    plant, or through the plan's own env."""
    import mpc_checker
    import mpc_plant_checker
    ee = EnsembleEnv(oenv, members, risk)
    if plant is None and not plant_kw:
        return mpc_checker.episode(ee, state0, key, N, H, Nd, temp, T, K, E)
    return mpc_plant_checker.episode(ee, state0, key, N, H, Nd, temp, T, K, E, plant=oenv if plant is None else plant,
                                     **plant_kw)
