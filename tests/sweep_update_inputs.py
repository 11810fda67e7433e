"""Inputs for tests/test_gpu_sweep_updates.py: what mbd_debug_sweep_update is fed, per plan of a sweep.  numpy only; seeded;
nothing here touches the checker, the library or a device (tests/test_sweep_updates.py checks the lists on the CPU).

The reward vectors are tests/pi_inputs.py's shapes.  In one call plan k of a sweep gets ANOTHER shape than its neighbours and
the sweep gives it another temperature, so a crossed stride or a shared temperature shows; `rounds(N, P)` lists the calls that
take every shape of `pi.shapes(N)` through at every N.

  normals(P, N, HNu)       z [P][N][HNu] ~ N(0, 1), float32: the step's normals of an MBD sweep
  means(P, HNu)            ybar [P][HNu] ~ 0.3 N(0, 1)
  values(z, sigma, ybar)   the candidates the lazy plans form from them, in float32 numpy: z * sigma rounded, + ybar rounded
                           (two roundings, no fma), then the clip to [-1, 1]
  candidates(P, N, HNu)    (Y0s [P][N][HNu], mu [P][HNu]) of a path-integral sweep: clipped normals around a small mean
  plan_rewards(k, N)       plan k's rewards of the plan-count matrix: the shape cycle at k, permuted by a generator seeded with k
                           — plans 9 apart share a shape and still differ
"""
import numpy as np

import pi_inputs as pi

# (a) around 64 (16 / V), 64 (16 / V + 32 / V), the tail of 16 / V rows and a partial group of 64, for V = 1, 2, 4:
# prefetch 1024 / 512 / 256 candidates, prefetch + first round 3072 / 1536 / 768, prefetch + tail 2048 / 1024 / 512
RAGGED_N = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 767, 769, 1023, 1024, 1025, 1087, 1089, 1535, 1537, 2047, 2049, 3071,
            3072, 3073, 3137, 4097, 8192, 8193, 12288)
WMEAN_V = (1, 2, 4, -1)  # MBD_WMEAN_V; -1: not set
WIDTHS = (("cartpole", 7), ("hopper", 30), ("humanoidrun", 20))  # H Nu = 7, 90, 340
MBD_TEMPS = (0.1, 1.0, 0.3)
# (b) Nu = 1: under V = 1 the tile count is ceil(H / 16) = 1, 1, 1, 2, 3, 4, 5, 7, 8, 8, 9, 9
TILE_H = (1, 15, 16, 17, 33, 64, 65, 112, 113, 128, 129, 144)
MATRIX_N = (65, 300)
MAX_PLANS = 32
# (c)
PI_N = (1, 2, 9, 10, 11, 63, 64, 65, 1000, 1024, 1025, 8192, 8193, 12288)
PI_TEMPS = (0.1, 1.0, 0.01)
PI_SIGMAS = (0.7, 0.5, 1.3)
# (d)
WEIGHTED_N = (1, 65, 1025, 3073)


def ragged_plans(N):
    return 3 if N < 8192 else 2


def _rng(*seed):
    return np.random.default_rng([int(s) for s in seed])


def normals(P, N, HNu, seed=0):
    return _rng(seed, P, N, HNu).standard_normal((P, N, HNu), dtype=np.float32)


def means(P, HNu, seed=1):
    return (_rng(seed, P, HNu).standard_normal((P, HNu)) * 0.3).astype(np.float32)


def values(z, sigma, ybar):
    """clip((z * sigma) + ybar, -1, 1) per plan: z [P][N][HNu], ybar [P][HNu]; every operation float32 and rounded."""
    z, ybar = np.asarray(z, np.float32), np.asarray(ybar, np.float32)
    t = z * np.float32(sigma)
    assert t.dtype == np.float32
    t += ybar[:, None, :]
    return np.clip(t, np.float32(-1), np.float32(1), out=t)


def candidates(P, N, HNu, seed=2):
    g = _rng(seed, P, N, HNu)
    mu = (g.standard_normal((P, HNu)) * 0.1).astype(np.float32)
    Y = g.standard_normal((P, N, HNu), dtype=np.float32)
    Y *= np.float32(0.7)
    Y += mu[:, None, :]
    return np.clip(Y, np.float32(-1), np.float32(1), out=Y), mu


def rounds(N, P):
    """The calls of a sweep of P plans that take every shape that exists at N through: a list of P-tuples of shape names, plan k's
    at position k; within a call the plans' shapes differ wherever more than one shape exists."""
    S = pi.shapes(N)
    n = -(-len(S) // P)
    return [tuple(S[(c * P + k) % len(S)] for k in range(P)) for c in range(n)]


def pi_rounds(N):
    """The calls of a path-integral sweep of three plans at PI_TEMPS that take every case of `pi.cases(N)` through: plan 0 runs
    the shapes at 0.1, plan 1 — one shape further — at 1.0, plan 2 `normal` at 0.01 (where it exists: two shapes further
    otherwise, an extra).  A list of 3-tuples of shape names."""
    S = pi.shapes(N)
    third = (lambda c: "normal") if "normal" in S else (lambda c: S[(c + 2) % len(S)])
    return [(S[c], S[(c + 1) % len(S)], third(c)) for c in range(len(S))]


def weighted_rounds(N, P=3):
    """The calls of a sweep under a weighting record: rews [P][N] each.  First weighting_inputs' planted vector — NaN, +inf, -inf at
    0, 63, 64, 1023, 1024, N - 1 — rolled by 0, 7, 130 places, so every plan has them elsewhere (N = 1: the one entry is NaN; plan
    1 gets a finite one); then a plan that keeps nothing, one that keeps one candidate, and a healthy one."""
    import weighting_inputs as wi
    assert P == 3
    a = np.stack([np.roll(wi.planted(N), s) for s in (0, 7, 130)])
    if N == 1:
        a[1] = 0.3
    drop = np.array([wi.NONFINITE[i % 3] for i in range(N)], np.float32)
    one = drop.copy()
    one[N // 2] = -2.5
    return [a.astype(np.float32), np.stack([drop, one, wi._base(N)]).astype(np.float32)]


def plan_rewards(k, N):
    S = pi.shapes(N)
    r = pi.rewards(S[k % len(S)], N)
    return _rng(77, k, N).permutation(r)
