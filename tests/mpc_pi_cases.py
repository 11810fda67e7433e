"""The inputs the path-integral episode tests share (tests/test_mpc_pi.py without a GPU, tests/test_gpu_mpc_pi.py with one): the
sizes of the other episode tests, the sigma records, the start state and episode key of a seed by the reference's chain — the
checker's own, which the GPU tests hold the library's reset to — and the checker's episodes, computed once per process."""
from __future__ import annotations

import functools

import numpy as np

import mpc_pi_checker
from conftest import load_model

H, ND, K, T, TEMP, SEED = 20, 6, 2, 5, 0.1, 3
N_OF = {"hopper": 64, "humanoidrun": 128, "car2d": 64}
METHODS = ("mppi", "cma-es", "cem")
PLAIN = (1.0, 1.0, 0.0)     # every tick is the reference's update() from the shifted mean
RESET = (0.7, 0.25, 0.0)    # a cold and a warm sigma of their own
CARRY = (0.6, 0.3, 100.0)   # cma-es: a warm tick's sigma follows the one the last tick ended with, between the two clamps


@functools.lru_cache(maxsize=None)
def _orc():
    from oracle import oracle
    oracle.build()
    return oracle.Oracle("f32_omp")


@functools.lru_cache(maxsize=None)
def oenv(name):
    from oracle.planner import OracleEnv
    if name == "car2d":
        return OracleEnv(_orc(), "car2d")
    m = load_model(name)
    return OracleEnv(_orc(), name, m.to_struct(), init_q=m.init_q)


@functools.lru_cache(maxsize=None)
def _start(name, seed):
    orc = _orc()
    rng, rng_reset = orc.split(orc.prng_key(seed), 2, 1)  # mbd_planner.py:40,79
    s0 = np.asarray(oenv(name).reset(rng_reset, 1), np.float32).reshape(-1)  # :80
    return s0, orc.split(rng, 2, 1)[0]  # :150


def start(name, seed=SEED):
    """(s_0 [S], the episode key) of a seed — mbd_hip.planners.mpc._reset_and_key's values."""
    s0, key = _start(name, seed)
    return s0.copy(), key.copy()


@functools.lru_cache(maxsize=None)
def _episode(name, method, E, rec, T_, extra):
    s0, key = start(name)
    return mpc_pi_checker.episode(oenv(name), s0, key, N_OF[name], H, ND, TEMP, T_, K, E, method, *rec, **dict(extra))


def episode(name, method, E=1, rec=PLAIN, T_=T, **extra):
    """The checker's episode of the case, shared: treat the arrays as read-only."""
    return _episode(name, method, E, tuple(rec), T_, tuple(sorted(extra.items())))
