"""The checker's restatement of a noise shape (include/mbd_hip.h mbd_noise_shape, DESIGN.md section 1 "N7 noise shape"): a
thin wrapper around an ``Oracle`` whose ``sample`` takes the oracle's own normals and forms the contract's three roundings in
numpy float32,

    z   = eps * g                      (eps: Oracle.sample(..., want_eps=True)'s: same key, counters, layout)
    Y0s = clip((z * sigma) + Ybar, -1, 1)

and hands every other call to the oracle.  oracle.planner.reverse_once, tests/mpc_checker.py, tests/mpc_plant_checker.py and
tests/ensemble_checker.py run unchanged on top of it: they reach the sampler through ``orc.sample`` and everything else —
the key chain, the plant's disturbance normals (``orc.normal``: never shaped), rollouts, the score update — through the same
object.  ``flat_samples``: that many calls of ``sample`` stay flat before the shape comes into force — the Ndiffuse - 1
steps of an episode's tick 0 under MBD_NOISE_WARM_TICKS (``episode``)."""
from __future__ import annotations

import numpy as np


class ShapedOracle:
    def __init__(self, orc, g, flat_samples: int = 0):
        self._orc = orc
        self.g = None if g is None else np.ascontiguousarray(g, np.float32)
        self.flat_samples = int(flat_samples)

    def __getattr__(self, name):  # (everything but the sampler is the oracle's)
        return getattr(self._orc, name)

    def sample(self, key, impl, N, H, Nu, begin, count, sigma, Ybar, want_eps=False):
        if self.flat_samples > 0:
            self.flat_samples -= 1
            return self._orc.sample(key, impl, N, H, Nu, begin, count, sigma, Ybar, want_eps=want_eps)
        if self.g is None:
            return self._orc.sample(key, impl, N, H, Nu, begin, count, sigma, Ybar, want_eps=want_eps)
        _, eps = self._orc.sample(key, impl, N, H, Nu, begin, count, sigma, Ybar, want_eps=True)
        g = self.g.reshape(H, Nu)
        z = (eps.astype(np.float32) * g[None]).astype(np.float32)
        y = (z * np.float32(sigma)).astype(np.float32)
        y = (y + np.asarray(Ybar, np.float32).reshape(1, H, Nu)).astype(np.float32)
        # the oracle's clip: min(max(y, -1), 1) with NaN passed through, as numpy's
        Y0s = np.ascontiguousarray(np.clip(y, np.float32(-1.0), np.float32(1.0)), np.float32)
        return (Y0s, z) if want_eps else Y0s


def shaped_env(oenv, g, flat_samples: int = 0):
    """A copy of the OracleEnv (or EnsembleEnv) whose ``orc`` samples under the shape ``g``; its rollouts, resets and
    everything else stay the env's own."""
    import copy
    e = copy.copy(oenv)
    e.orc = ShapedOracle(oenv.orc, g, flat_samples)
    return e


def reverse_once(orc, oenv, g, *args, **kw):
    """oracle.planner.reverse_once under the shape ``g`` (None: flat)."""
    from oracle import planner as op
    return op.reverse_once(ShapedOracle(orc, g), oenv, *args, **kw)


def episode(checker_episode, oenv, g, when, Nd, *args, **kw):
    """``checker_episode(oenv', *args, **kw)`` — tests/mpc_checker.episode, mpc_plant_checker.episode, or a lambda around
    ensemble_checker.episode — with oenv' sampling under ``g``: in every step (``when`` "always"), or from tick 1 on
    ("warm": the Nd - 1 steps of tick 0 stay flat)."""
    if when not in ("always", "warm"):
        raise ValueError(f"when={when!r}")
    return checker_episode(shaped_env(oenv, g, Nd - 1 if when == "warm" else 0), *args, **kw)
