"""The inputs of the tests that run the weighting record TOGETHER with the other records and behind rollouts that really diverge
(tests/test_gpu_weighting_combined.py on the device, the reach assertions of tests/test_weighting.py on the CPU): the sizes, the
records, the models and the checker's compositions, so that the CPU test can assert of the very cases the GPU tests run that they
take the branches and drop the candidates they are there for.  numpy and the checker only; nothing here touches the library or a
device.

HOW SOME CANDIDATES OF A LAUNCH DIVERGE.  containment_inputs.poison_model sets one actuator's gear of the hopper to 1e30.  Every
candidate whose action in that column is an ordinary clipped normal then diverges (measured with the checker: 0 of 33, 64 and 96
candidates keep a finite reward, at sigma = 0.09 from the reset state), and a column of exact zeros keeps all of them — no seed gives
a launch in between.  A noise shape of G0 = 3e-5 on that column (finite, legal, not zero) puts the torques 1e30 * 3e-5 * sigma * eps
around the size at which the hopper's four control steps overflow float32: candidates with a small normal there stay finite, the
others do not.  ``divergence_step`` is that launch in the checker; tests/test_weighting.py asserts 0 < kept < N of it."""
from __future__ import annotations

import functools

import numpy as np

import containment_inputs as ci
import ensemble_checker as ec
import noise_basis_checker as nbc
import objective_checker as oc
import weighting_checker as wc
import weighting_inputs as wi
from noise_shape_checker import ShapedOracle, shaped_env

H, NAME, TEMP = 4, "hopper", 0.1
G0 = 3e-5
T, K, E = 3, 2, 1
FULL = wc.Record(reject_nonfinite=True, ess_frac=1.0, temp_min=0.01, temp_max=10.0, iters=12)  # the target is never exceeded: temp_max
STEP = dict(N=64, Nd=8, i=3, state_seed=3, key_seed=75, pi_sigma=0.1)  # the one-step divergence launch
LOOP = dict(N=64, Nd=5, state_seed=3, key_seed=5)  # the closed loops


def shape(Nu, g0=G0):
    g = np.ones((H, Nu), np.float32)
    g[:, 0] = np.float32(g0)
    return g


@functools.lru_cache(maxsize=None)
def models():
    """(the hopper, the hopper with actuator 0's gear at 1e30, a heavier and weaker hopper)."""
    m = ci.model(NAME)[0]
    return m, ci.poison_model(m), m.scaled(mass=1.25, friction=0.7, gear=0.9)


def oenv(orc, m):
    from oracle.planner import OracleEnv
    return OracleEnv(orc, NAME, m.to_struct(), init_q=m.init_q)


def start(orc, m, seed, impl=1):
    return np.asarray(oenv(orc, m).reset(orc.prng_key(seed), impl), np.float32).reshape(-1)


def objective(Nu):
    """The objective record of the combined tests: a discount with a terminal weight, both costs, actuator weights, a prev0."""
    w = (np.float64(0.9) ** np.arange(H, dtype=np.float64))
    w[-1] *= 2.0  # (mbd_hip.planners.mpc.discount_weights(H, 0.9, terminal=2.0), restated: the GPU test asserts the two agree)
    return oc.Record(row_weight=w.astype(np.float32), effort=0.1, rate=0.2,
                     act_weight=np.linspace(0.5, 2.0, Nu).astype(np.float32), prev0=np.linspace(0.3, -0.2, Nu).astype(np.float32))


def branch_of(entry, rec):
    """Which arm of the selection a log entry (temp, ess, kept) shows under ``rec``."""
    temp, _, kept = entry
    if kept == 0:
        return "none"
    if np.float32(rec.ess_frac) == 0:
        return "fixed"
    if temp == np.float32(rec.temp_min):
        return "min"
    if temp == np.float32(rec.temp_max):
        return "max"
    return "loop"


# ---- real divergence, one step -----------------------------------------------------------------------------------------------------
def divergence_step(orc, method, impl=1):
    """The launch of the one-step divergence test in the checker: dict(s0, mu, sigma, Y0s, rews, sched)."""
    m, bad, _ = models()
    oe = oenv(orc, bad)
    s0 = start(orc, bad, STEP["state_seed"], impl)
    sched = orc.schedule(1e-4, 1e-2, STEP["Nd"])
    sigma = float(sched[2][STEP["i"]]) if method == 0 else STEP["pi_sigma"]
    Nu = oe.Nu
    mu = (np.random.default_rng([H, Nu]).normal(size=(H, Nu)) * 0.3).astype(np.float32)
    mu[:, 0] = 0.0  # (the poisoned column is centred: what a candidate feels there is its own shaped normal)
    Y0s = ShapedOracle(orc, shape(Nu)).sample(orc.prng_key(STEP["key_seed"]), impl, STEP["N"], H, Nu, 0, STEP["N"], sigma, mu)
    from oracle import planner as op
    rews = op.mean_h(orc, np.ascontiguousarray(oe.rollout(s0, Y0s)))
    return dict(s0=s0, mu=mu, sigma=sigma, Y0s=Y0s, rews=rews, sched=sched)


def divergence_episode(orc, rec, impl=1):
    """The closed loop on the poisoned hopper, planned and executed on it, under the shape (always) and ``rec``."""
    _, bad, _ = models()
    oe = oenv(orc, bad)
    s0 = start(orc, bad, LOOP["state_seed"], impl)
    key = orc.prng_key(LOOP["key_seed"])
    return wc.episode(shaped_env(oe, shape(oe.Nu)), s0, key, LOOP["N"], H, LOOP["Nd"], TEMP, T, K, E, rec, impl)


# ---- an objective in front ---------------------------------------------------------------------------------------------------------
def objective_run(orc, rec, with_objective=True, N=65, Nd=5, impl=1):
    m = models()[0]
    oe = oenv(orc, m)
    env = oc.ObjectiveEnv(oe, objective(oe.Nu)) if with_objective else oe
    return wc.run(orc, env, start(orc, m, 3, impl), orc.prng_key(7), N, H, Nd, TEMP, rec, impl)


def objective_episode(orc, rec, with_objective=True, N=65, Nd=5, impl=1, states=False, **kw):
    """``kw``: D, plant (a model), dkey, act_std."""
    m = models()[0]
    oe = oenv(orc, m)
    if kw.get("plant") is not None:
        kw["plant"] = oenv(orc, kw["plant"])
    if with_objective:
        kw["orec"] = objective(oe.Nu)
    return wc.episode(oe, start(orc, m, 3, impl), orc.prng_key(5), N, H, Nd, TEMP, T, K, E, rec, impl, **kw)


# ---- an ensemble in front ----------------------------------------------------------------------------------------------------------
def ensemble_members(bad):
    """The M = 3 member models: the plan's own (None), a heavier one, and at position ``bad`` the one with the 1e30 gear."""
    m, poisoned, other = models()
    out = [None, other]
    out.insert(bad, poisoned)
    return out


def ensemble_env(orc, bad, risk, with_objective=False):
    """(the plan's OracleEnv, the EnsembleEnv sampling under the shape, the shared Prev or None, the objective record or None)."""
    m = models()[0]
    oe = oenv(orc, m)
    mem = [oe if x is None else oenv(orc, x) for x in ensemble_members(bad)]
    prev = orec = None
    if with_objective:
        orec = objective(oe.Nu)
        prev = oc.Prev(orec.prev0)
        mem = [oc.ObjectiveEnv(x, orec, prev) for x in mem]
    return oe, shaped_env(ec.EnsembleEnv(oe, mem, risk), shape(oe.Nu)), prev, orec


def ensemble_step(orc, N, bad, risk, rec, with_objective=False, Nd=5, impl=1):
    """One reverse_once (step Nd - 2, from a mean that is not zero off the poisoned column): dict(out, rew_mean, log, det, Ybar, s0)."""
    m = models()[0]
    oe, ee, prev, orec = ensemble_env(orc, bad, risk, with_objective)
    s0 = start(orc, m, 3, impl)
    Ybar = (np.random.default_rng(N).normal(size=(H, oe.Nu)) * 0.3).astype(np.float32)
    Ybar[:, 0] = 0.0
    log = []
    sched = orc.schedule(1e-4, 1e-2, Nd)
    _, out, rm, det = wc.reverse_once(ee.orc, ee, s0, Nd - 2, orc.prng_key(10 + N), Ybar, sched, N, H, TEMP, impl, rec=rec, log=log)
    return dict(out=out, rew_mean=rm, log=log, det=det, Ybar=Ybar, s0=s0, sched=sched)


def ensemble_episode(orc, N, bad, risk, rec, with_objective=False, Nd=5, impl=1):
    m = models()[0]
    oe, ee, prev, orec = ensemble_env(orc, bad, risk, with_objective)
    kw = dict(env=ee, prev=prev, orec=orec) if with_objective else dict(env=ee, prev=oc.Prev())
    return wc.episode(oe, start(orc, m, 3, impl), orc.prng_key(6), N, H, Nd, TEMP, T, K, E, rec, impl, **kw)


ENSEMBLES = [(N, bad, risk, False) for N in (33, 32) for bad in (0, 2) for risk in ("mean", "min")] + [(33, 2, "min", True)]


# ---- noise shape and basis, plant, delay -------------------------------------------------------------------------------------------
def composed_episode(orc, rec, N=48, Nd=5, impl=1):
    """A warm-ticks-only shape, a knot basis (always), D = 1 with given rows, a heavier plant with action noise and kicks."""
    m, _, other = models()
    oe = oenv(orc, m)
    Nu = oe.Nu
    g, W = composed_tables(Nu)
    rows0 = composed_rows0(Nu)
    return nbc.episode(lambda e, *a, **kw: wc.episode(e, *a, **kw), oe, W, "always", Nd, start(orc, m, 3, impl), orc.prng_key(5), N, H, Nd,
                       TEMP, T, K, E, rec, impl, shape=g, shape_when="warm", D=1, rows0=rows0, plant=oenv(orc, other),
                       dkey=orc.prng_key(11), act_std=0.05, kick_std=0.02, kick_every=2)


def composed_tables(Nu):
    g = (0.5 + np.arange(H * Nu, dtype=np.float64) / (H * Nu)).astype(np.float32).reshape(H, Nu)
    return g, nbc.basis_of(H, 3)


def composed_rows0(Nu):
    return (np.random.default_rng(1).normal(size=(E, Nu)) * 0.5).astype(np.float32)


# ---- cem with fewer than ten positive weights --------------------------------------------------------------------------------------
def cem_ties(N=64):
    """name -> (rews [N], record).  ``few_positive``: 12 kept — three at 1.0 (indices 3, 20, 41) and nine at -1.0, the LOWEST
    indices of the rest — and 52 dropped, under a bracket whose temp_min the target of 3 already meets: the nine kept weights
    underflow to +0 and tie with the dropped candidates', all of which have higher indices."""
    cases = {c.name: (c.rews, c.rec) for c in wi.cases(N) if c.name in ("one_kept", "all_dropped")}
    r = np.array([wi.NONFINITE[i % 3] for i in range(N)], np.float32)
    top, low = (3, 20, 41), (0, 1, 2, 4, 5, 6, 7, 8, 9)
    r[list(top)] = 1.0
    r[list(low)] = -1.0
    cases["few_positive"] = (r, wc.Record(True, 0.25, 0.01, 10.0, 12))
    return cases
