"""The checker's restatement of a noise basis (include/mbd_hip.h mbd_noise_basis, DESIGN.md section 1 "N8 noise basis"): a thin
wrapper around an ``Oracle``, as tests/noise_shape_checker.ShapedOracle is, whose ``sample`` draws the oracle's own normals for
the KNOT tensor — ``orc.normal(key, (N, n_knots, Nu), impl)``: the step's key, the layout's counters and pairing for a tensor
of that size — and forms the contract in numpy float32,

    c   = +0;  for k ascending:  if W[h][k] != 0:  c = fl(c + fl(W[h][k] * eps[n][k][a]))
    z   = c                      (no shape)        z = fl(c * g[h][a])      (with one: the basis first, then the shape)
    Y0s = clip(fl(fl(z * sigma) + Ybar), -1, 1)

and hands every other call to the oracle.  oracle.planner.reverse_once, tests/mpc_checker.py, tests/mpc_plant_checker.py and
tests/ensemble_checker.py run unchanged on top of it (the plant's disturbance normals come from ``orc.normal`` directly and
pass no basis).  ``basis_flat`` / ``shape_flat``: that many calls of ``sample`` pass before the basis / the shape comes into
force — the Ndiffuse - 1 steps of an episode's tick 0 under MBD_NOISE_WARM_TICKS, each setting with its own ``when``."""
from __future__ import annotations

import numpy as np

from noise_shape_checker import ShapedOracle


def combine(W, eps):
    """c [N, H, Nu] from W [H, K] and eps [N, K, Nu]: the contract's sum, zero weights (of either sign) left out."""
    W = np.asarray(W, np.float32)
    eps = np.asarray(eps, np.float32)
    N, K, Nu = eps.shape
    H = W.shape[0]
    assert W.shape == (H, K)
    c = np.zeros((N, H, Nu), np.float32)
    for h in range(H):
        for k in range(K):
            w = W[h, k]
            if w != 0:
                term = (w * eps[:, k, :]).astype(np.float32)
                c[:, h, :] = (c[:, h, :] + term).astype(np.float32)
    return c


def basis_of(H, K):
    """A dense W [H, K] of distinct values in [-1.5, 1.75] — negative ones, ones above 1 — with, where the table has room for
    them, a row of zeros, a column of zeros and every fifth of the remaining entries exactly zero (one of them -0.0)."""
    W = np.linspace(-1.5, 1.75, H * K, dtype=np.float64).astype(np.float32).reshape(H, K)
    W[W == 0] = 0.125
    assert np.unique(W).size == H * K
    if H * K >= 6:
        flat = W.reshape(-1)
        flat[1::5] = 0.0
        flat[1] = -0.0
    if H >= 3:
        W[H // 2] = 0.0
    if K >= 3:
        W[:, K // 2] = 0.0
    if H * K > 1:
        assert (W < 0).any() and (W > 1).any()
    return W


class BasisOracle:
    def __init__(self, orc, W, g=None, basis_flat: int = 0, shape_flat: int = 0):
        self._orc = orc
        self.W = None if W is None else np.ascontiguousarray(W, np.float32)
        self.g = None if g is None else np.ascontiguousarray(g, np.float32)
        self.basis_flat, self.shape_flat = int(basis_flat), int(shape_flat)

    def __getattr__(self, name):  # (everything but the sampler is the oracle's)
        return getattr(self._orc, name)

    def sample(self, key, impl, N, H, Nu, begin, count, sigma, Ybar, want_eps=False):
        W = self.W if self.basis_flat <= 0 else None
        g = self.g if self.shape_flat <= 0 else None
        self.basis_flat, self.shape_flat = max(self.basis_flat - 1, 0), max(self.shape_flat - 1, 0)
        if W is None:
            return ShapedOracle(self._orc, g).sample(key, impl, N, H, Nu, begin, count, sigma, Ybar, want_eps=want_eps)
        assert W.shape[0] == H, (W.shape, H)
        eps = self._orc.normal(key, (N, W.shape[1], Nu), impl)
        z = combine(W, eps)
        if g is not None:
            z = (z * g.reshape(1, H, Nu)).astype(np.float32)
        z = np.ascontiguousarray(z[begin:begin + count])
        y = (z * np.float32(sigma)).astype(np.float32)
        y = (y + np.asarray(Ybar, np.float32).reshape(1, H, Nu)).astype(np.float32)
        Y0s = np.ascontiguousarray(np.clip(y, np.float32(-1.0), np.float32(1.0)), np.float32)
        return (Y0s, z) if want_eps else Y0s


def basis_env(oenv, W, g=None, basis_flat: int = 0, shape_flat: int = 0):
    """A copy of the OracleEnv (or EnsembleEnv) whose ``orc`` samples under the basis ``W`` (and the shape ``g``)."""
    import copy
    e = copy.copy(oenv)
    e.orc = BasisOracle(oenv.orc, W, g, basis_flat, shape_flat)
    return e


def reverse_once(orc, oenv, W, *args, g=None, **kw):
    """oracle.planner.reverse_once under the basis ``W`` (None: none) and the shape ``g``."""
    from oracle import planner as op
    return op.reverse_once(BasisOracle(orc, W, g), oenv, *args, **kw)


def episode(checker_episode, oenv, W, when, Nd, *args, shape=None, shape_when="always", **kw):
    """``checker_episode(oenv', *args, **kw)`` with oenv' sampling under ``W`` in every step (``when`` "always") or from
    tick 1 on ("warm": the Nd - 1 steps of tick 0 stay white), and under ``shape`` likewise by ``shape_when``."""
    for w in (when, shape_when):
        if w not in ("always", "warm"):
            raise ValueError(f"when={w!r}")
    flat = {"always": 0, "warm": Nd - 1}
    return checker_episode(basis_env(oenv, W, shape, flat[when], flat[shape_when]), *args, **kw)
