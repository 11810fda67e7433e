"""Oracle pinning: update rules of mbd/planners/path_integral.py:33-52,122-125 against numpy (float64).

The first tests pin each rule on one organic input.  The rest run the checker over tests/pi_inputs.py — every reward shape
and temperature at candidate counts N in SIZES (around every boundary of the kernels that the checker stands in for: K = N
below ten, one element per lane at 64, rewards in registers up to 8192, the fused launch up to 12 288, LDS up to 36 864),
H x Nu = 5 x 3 — against numpy float64 of path_integral.py:123-124, 33-45.  The reference of every figure is numpy float64,
never the checker or the kernels.

MEASURED (the committed generator, worst over every N, shape and temperature with a meaningful float64 reference) and
ASSERTED (4 x the measured value: the seeds are fixed, so the margin covers another libm or numpy summation order, not
chance):

  weights, of the largest weight       measured 2.27e-06 (normal, temp 0.01, N = 40 001)        asserted 9.08e-06
  weighted mean (mppi, cma-es), abs    measured 3.11e-06 (normal, temp 0.01, N = 40 001)        asserted 1.24e-05
  cma-es sigma, relative               measured 7.33e-06 (boundary_tie, temp 1.0, N = 40 001)   asserted 2.93e-05
  mean reward, of max(1, |mean|)       measured 1.50e-07 (negative, temp 0.1, N = 8193)         asserted 6.00e-07
  cem mean, abs                        measured 8.68e-08 (boundary_tie, temp 0.1, N = 11)       asserted 3.47e-07
                                       (and the 1e-6 of test_cem_takes_the_ten_best)

DEGENERATE WEIGHTS (numerics): cem ranks by the key isnan(w) ? +inf : w with ties towards the higher index —
argsort(weights)[::-1][:10] of a stable NaN-last sort (:50) — and the cma-es floor is jnp.maximum (:44), which propagates
NaN.  Zero-spread rewards (no guard at :123) therefore give: mppi and cma-es a NaN mean, cma-es a NaN sigma, cem the finite
mean of candidates N-1 .. N-10.  Comparisons with equal_nan are made for the constant shapes and at N = 1 only.
"""
import numpy as np
import pytest

import pi_inputs as pi

SIZES = (1, 9, 10, 11, 64, 65, 1000, 1025, 8193, 12289, 36865, 40001)
BOUND_W = 4 * 2.27e-6
BOUND_WM = 4 * 3.11e-6
BOUND_SIG = 4 * 7.33e-6
BOUND_RM = 4 * 1.50e-7
BOUND_CEM = 4 * 8.68e-8


def _inputs(N=64, H=5, Nu=3, seed=0):
    g = np.random.default_rng(seed)
    rews = g.normal(size=N).astype(np.float32)
    mu = (g.normal(size=(H, Nu)) * 0.1).astype(np.float32)
    Y0s = np.clip(mu + g.normal(size=(N, H, Nu)) * 0.7, -1, 1).astype(np.float32)
    return rews, Y0s, mu


def _weights(rews, temp):
    r = rews.astype(np.float64)
    l = (r - r.mean()) / r.std() / temp
    w = np.exp(l - l.max())
    return w / w.sum()


def test_mppi_is_the_weighted_mean_and_keeps_sigma(orc):
    rews, Y0s, mu = _inputs()
    out, sigma, w, m = orc.pi_update(1, rews, Y0s, mu, 0.8, 0.1)
    wr = _weights(rews, 0.1)
    assert np.allclose(w, wr, rtol=3e-5, atol=1e-10) and abs(m - rews.astype(np.float64).mean()) < 1e-6
    assert np.abs(out - np.einsum("n,nij->ij", wr, Y0s.astype(np.float64))).max() < 2e-6
    assert sigma == np.float32(0.8)


def test_cma_es_sigma_update(orc):
    rews, Y0s, mu = _inputs(seed=1)
    out, sigma, w, _ = orc.pi_update(2, rews, Y0s, mu, 0.5, 0.2)
    wr = _weights(rews, 0.2)
    err2 = (Y0s.astype(np.float64) - mu) ** 2
    ref = np.sqrt(np.einsum("n,nij->ij", wr, err2)).mean() * 0.5
    assert abs(sigma - max(ref, 1e-3)) < 1e-6
    assert np.abs(out - np.einsum("n,nij->ij", wr, Y0s.astype(np.float64))).max() < 2e-6
    # the floor (:44)
    _, s2, _, _ = orc.pi_update(2, rews, np.repeat(mu[None], 64, 0), mu, 0.5, 0.2)
    assert s2 == np.float32(1e-3)


def test_cem_takes_the_ten_best(orc):
    rews, Y0s, mu = _inputs(seed=2)
    out, sigma, w, _ = orc.pi_update(3, rews, Y0s, mu, 1.0, 0.1)
    idx = np.argsort(w)[::-1][:10]
    assert np.abs(out - Y0s[idx].astype(np.float64).mean(0)).max() < 1e-6 and sigma == 1.0
    # ties: argsort()[::-1] prefers the HIGHER index among equal weights
    rews[:] = 0.0
    rews[5] = 1.0
    out, _, w, _ = orc.pi_update(3, rews, Y0s, mu, 1.0, 0.1)
    idx = [5] + list(range(63, 54, -1))
    assert np.abs(out - Y0s[idx].astype(np.float64).mean(0)).max() < 1e-6


def _mean_of_rows(Y0s, idx):
    """The float32 sequential sum of the rows idx, in that order, divided by their number: cem_update's mean as the checker
    and cem_mean_kernel add it."""
    acc = np.zeros(Y0s.shape[1:], np.float32)
    for i in idx:
        acc = acc + Y0s[i]
    return acc / np.float32(len(idx))


def test_no_std_guard(orc):
    """path_integral.py:123 divides by rews.std() unguarded: constant rewards give NaN weights (as in JAX).  mppi and cma-es
    then have a NaN mean and cma-es a NaN sigma (jnp.maximum, :44); cem's argsort ranks the NaNs first, by descending index
    (:50): the finite mean of candidates 63 .. 54."""
    rews, Y0s, mu = _inputs(seed=3)
    rews[:] = 0.3
    out, sigma, w, _ = orc.pi_update(1, rews, Y0s, mu, 1.0, 0.1)
    assert np.isnan(w).all() and np.isnan(out).all()
    assert sigma == 1.0
    out, sigma, w, _ = orc.pi_update(2, rews, Y0s, mu, 0.5, 0.1)
    assert np.isnan(w).all() and np.isnan(out).all() and np.isnan(sigma)
    out, sigma, w, m = orc.pi_update(3, rews, Y0s, mu, 0.5, 0.1)
    assert np.isnan(w).all() and sigma == 0.5 and m == np.float32(0.3)
    assert np.array_equal(out, _mean_of_rows(Y0s, [63, 62, 61, 60, 59, 58, 57, 56, 55, 54]))


def _ref64(rews, Y0s, mu, sigma, temp):
    """path_integral.py:123-124, 33-45 in float64: weights, weighted mean, cma-es sigma, mean reward."""
    w = _weights(rews, temp)
    Y = Y0s.astype(np.float64)
    mean = np.einsum("n,nij->ij", w, Y)
    sig = max(np.sqrt(np.einsum("n,nij->ij", w, (Y - mu.astype(np.float64)) ** 2)).mean() * sigma, 1e-3)
    return w, mean, sig, rews.astype(np.float64).mean()


def measure(orc, N):
    """Worst errors of the checker against float64 over every meaningful case of pi_inputs at N: a dict of the five figures
    of the module docstring, each with the case that set it."""
    worst = {k: (0.0, None) for k in ("weights", "wmean", "sigma", "rew_mean", "cem")}

    def note(k, v, case):
        if v > worst[k][0]:
            worst[k] = (float(v), case)
    Y0s, mu = pi.candidates(N)
    for name, temp, rews in pi.cases(N):
        if not pi.float64_meaningful(name, N):
            continue
        wr, mean_r, sig_r, rm_r = _ref64(rews, Y0s, mu, 0.7, temp)
        for method in (1, 2):
            out, sigma, w, m = orc.pi_update(method, rews, Y0s, mu, 0.7, temp)
            assert np.isfinite(w).all() and np.isfinite(out).all(), (name, temp, N, method)
            note("weights", np.abs(w - wr).max() / wr.max(), (name, temp, N))
            note("wmean", np.abs(out - mean_r).max(), (name, temp, N))
            note("rew_mean", abs(m - rm_r) / max(1.0, abs(rm_r)), (name, temp, N))
            if method == 2:
                note("sigma", abs(sigma - sig_r) / sig_r, (name, temp, N))
            else:
                assert sigma == np.float32(0.7)
        out, sigma, w, m = orc.pi_update(3, rews, Y0s, mu, 0.7, temp)
        idx = _stable_top(w, N)
        note("cem", np.abs(out - Y0s[idx].astype(np.float64).mean(0)).max(), (name, temp, N))
    return worst


def _stable_top(w, N):
    """argsort(w)[::-1][:K] of a stable sort that places NaN last (path_integral.py:50), as the key form of the contract."""
    key = np.where(np.isnan(w), np.inf, w)
    return np.argsort(key, kind="stable")[::-1][:min(pi.K_CEM, N)]


@pytest.mark.parametrize("N", [n for n in SIZES if n > 1])
def test_update_rules_against_float64_at_every_size(orc, N):
    """The checker's weights, weighted mean, cma-es sigma, mean reward and cem mean against numpy float64, every shape and
    temperature of pi_inputs at N, within the bounds of the module docstring."""
    worst = measure(orc, N)
    print(f"N={N}: " + ", ".join(f"{k} {v:.3g} {c}" for k, (v, c) in worst.items()))
    assert worst["weights"][0] <= BOUND_W, worst["weights"]
    assert worst["wmean"][0] <= BOUND_WM, worst["wmean"]
    assert worst["sigma"][0] <= BOUND_SIG, worst["sigma"]
    assert worst["rew_mean"][0] <= BOUND_RM, worst["rew_mean"]
    assert worst["cem"][0] <= min(BOUND_CEM, 1e-6), worst["cem"]


@pytest.mark.parametrize("N", SIZES)
def test_cem_selection_order_at_every_size(orc, N):
    """cem at every shape (the constant ones included) and temperature: the mean is the float64 mean of Y0s[idx] within
    1e-6, idx the stable NaN-last argsort of the checker's own float32 weights, reversed; and for the shapes whose order is
    known by construction — one_hot, boundary_tie, the constant ones — it is EXACTLY the float32 sequential sum of the
    expected rows, in their order, divided by K."""
    Y0s, mu = pi.candidates(N)
    seen = set()
    for name, temp, rews in pi.cases(N):
        out, sigma, w, _ = orc.pi_update(3, rews, Y0s, mu, 0.7, temp)
        assert sigma == np.float32(0.7)
        idx = _stable_top(w, N)
        assert np.isfinite(out).all(), (name, temp, N)
        assert np.abs(out - Y0s[idx].astype(np.float64).mean(0)).max() < 1e-6, (name, temp, N)
        if name in ("one_hot", "boundary_tie") + pi.CONSTANT:
            exp = pi.expected_cem_indices(name, N)
            assert list(idx) == exp, (name, temp, N, list(idx), exp)
            assert np.array_equal(out, _mean_of_rows(Y0s, exp)), (name, temp, N)
        seen.add(name)
    assert seen == set(pi.shapes(N))
    # three of the lists, written out
    if N == 64:
        assert pi.expected_cem_indices("constant", 64) == [63, 62, 61, 60, 59, 58, 57, 56, 55, 54]
        assert pi.expected_cem_indices("one_hot", 64) == [32, 63, 62, 61, 60, 59, 58, 57, 56, 55]
    if N == 9:
        assert pi.expected_cem_indices("constant", 9) == [8, 7, 6, 5, 4, 3, 2, 1, 0]
        assert pi.expected_cem_indices("one_hot", 9) == [4, 8, 7, 6, 5, 3, 2, 1, 0]
    if N == 1000:
        top, block = pi.boundary_tie_layout(1000)
        assert block == [333, 334, 870, 934, 998] and pi.expected_cem_indices("boundary_tie", 1000) == top + [998]


@pytest.mark.parametrize("N", SIZES)
def test_zero_spread_rewards_at_every_size(orc, N):
    """The constant shapes (and, at N = 1, any reward): all N weights tie.  Where the float32 mean of the rewards is exact
    (constant_exact at every N; constant at N = 1 and 64) every weight is NaN: mppi and cma-es give a NaN mean, cma-es a NaN
    sigma, mppi and cem leave sigma alone, cem gives the finite mean of candidates N-1 .. N-10.  Where the mean of 0.3f
    rounds, every candidate has the same nonzero deviation and every weight is float32(1) / N; the rules then run on
    numbers."""
    Y0s, mu = pi.candidates(N)
    K = min(pi.K_CEM, N)
    cases = [c for c in pi.cases(N) if c[0] in pi.CONSTANT]
    if N == 1:
        cases += [("normal", 0.1, np.array([-1.75], np.float32)), ("offset", 1.0, np.array([50.01], np.float32))]
    assert {c[0] for c in cases} >= set(pi.CONSTANT)
    for name, temp, rews in cases:
        must_nan = name != "constant" or N in (1, 64)
        o1, s1, w, m = orc.pi_update(1, rews, Y0s, mu, 0.7, temp)
        o2, s2, w2, _ = orc.pi_update(2, rews, Y0s, mu, 0.7, temp)
        o3, s3, w3, _ = orc.pi_update(3, rews, Y0s, mu, 0.7, temp)
        assert np.array_equal(w, w2, equal_nan=True) and np.array_equal(w, w3, equal_nan=True)
        assert m == rews[0] or not must_nan
        assert s1 == np.float32(0.7) and s3 == np.float32(0.7)
        assert np.array_equal(o3, _mean_of_rows(Y0s, list(range(N - 1, N - 1 - K, -1)))), (name, temp, N)
        if np.isnan(w).any() or must_nan:
            assert np.isnan(w).all() and np.isnan(o1).all() and np.isnan(o2).all() and np.isnan(s2), (name, temp, N)
        else:
            assert np.array_equal(w, np.full(N, np.float32(1.0) / np.float32(N))), (name, temp, N)
            mean_r = Y0s.astype(np.float64).mean(0)
            assert np.abs(o1 - mean_r).max() <= BOUND_WM and np.array_equal(o1, o2), (name, temp, N)
            sig_r = np.sqrt(((Y0s.astype(np.float64) - mu.astype(np.float64)) ** 2).mean(0)).mean() * 0.7
            assert abs(s2 - sig_r) / sig_r <= BOUND_SIG, (name, temp, N)
