"""Reward vectors for the path-integral update rules (update_method 1 / 2 / 3 = mppi / cma-es / cem), by name.

Shared by tests/test_oracle_path_integral.py (the checker against numpy float64, on the CPU) and tests/test_gpu_pi_updates.py
(the kernels against the checker, by bit pattern): both are fed the same arrays.  numpy only; seeded; nothing here touches
the checker, the library or a device.

`cases(N)` yields `(name, temp, rews float32 [N])` for every reward shape that exists at N and every temperature it is run
at:

  normal         N(0, 1).  Also at temperature 0.01: most weights underflow to exactly 0 and tie there.
  offset         50 + 0.01 N(0, 1), and
  negative       -300 + 5 N(0, 1): rewards of the size the envs produce, the spread a small part of the mean.
  quantised      round(2 N(0, 1)) / 2: a handful of distinct values, so the tenth and the eleventh best tie, within a lane of
                 the selection kernel and across lanes.
  ties_outlier   N(0, 1) with the first third equal to rews[0] and one value 40 at N // 2 (the MBD score test's case).
  one_hot        zeros and a single 1 at N // 2: every weight but one ties.  cem takes N // 2, then the highest indices.
  boundary_tie   exactly nine distinct top values and a block of equal values next (`boundary_tie_layout`): the tenth pick is
                 the block's highest index, and the block has members in one lane (b, b - 64, b - 128), in other lanes and in
                 other 1024-strides.  The block's highest index is NOT the last candidate.
  constant       all 0.3.  The spread is zero, path_integral.py:123 has no guard: where the float32 mean of the rewards is
                 exactly 0.3f every weight is NaN (N = 1, 64: every partial sum is a power of two times 0.3f); where the
                 rounded mean is a float off, every candidate has the SAME nonzero deviation and every weight is the same
                 number.  Either way all N weights tie.  (In the contract's summation order the mean comes out as 0.3f up to
                 N = 8192 and a float off from 8193 on — observed, not asserted: the tests accept both and assert NaN only
                 where exactness is provable.)
  constant_exact all 0.25: every partial sum is exact in float32 in any order, so every weight is NaN at every N.

At N = 1 a candidate has zero spread whatever its reward: only the two constant cases exist there.  A case needs N >= 2,
boundary_tie N >= 9 (at N = 9 and 10 the block has zero and one member: nothing ties, the case still selects).

`float64_meaningful(name, N)`: whether a float64 evaluation of :123-124 is a reference for the case — not for the constant
cases and not at N = 1, where the result is decided by rounding (0 / 0, or a deviation that is pure rounding error).  Every
other case has std / max(1, |mean|) >= 1e-4 in float64, asserted here.
"""
import zlib

import numpy as np

TEMPS = (0.1, 1.0)
SHAPES = ("normal", "offset", "negative", "quantised", "ties_outlier", "one_hot", "boundary_tie", "constant", "constant_exact")
CONSTANT = ("constant", "constant_exact")
K_CEM = 10  # path_integral.py:50


def _rng(name, N):
    return np.random.default_rng([zlib.crc32(name.encode()), N])


def float64_meaningful(name, N):
    return name not in CONSTANT and N > 1


def boundary_tie_layout(N):
    """(top, block): the indices of the nine distinct top values in DESCENDING order of value, and the indices of the block of
    equal values below them (ascending).  b = N - 2 is the block's highest index; b - 64 and b - 128 share its lane of the
    64-lane selection; a = N // 3 and a + 1 sit in two other lanes, a + 1024 + 3 and a + 2048 + 5 in other 1024-strides of the
    score kernel.  Up to N = 11 the block is simply every index that is not a top."""
    assert N >= 9
    g = _rng("boundary_tie/layout", N)
    if N <= 11:
        top = g.permutation(N)[:9]
        return [int(i) for i in top], sorted(set(range(N)) - set(int(i) for i in top))
    b, a = N - 2, N // 3
    block = sorted({i for i in (b, b - 64, b - 128, a, a + 1, a + 1024 + 3, a + 2048 + 5) if 0 <= i <= b})
    rest = np.array(sorted(set(range(N)) - set(block)))
    top = g.permutation(rest)[:9]
    return [int(i) for i in top], block


def rewards(name, N):
    """The float32 reward vector [N] of a shape."""
    g = _rng(name, N)
    if name == "normal":
        r = g.normal(size=N)
    elif name == "offset":
        r = 50.0 + 0.01 * g.normal(size=N)
    elif name == "negative":
        r = -300.0 + 5.0 * g.normal(size=N)
    elif name == "quantised":
        r = np.round(2.0 * g.normal(size=N)) / 2.0
        if N == 2:
            r[1] = r[0] + 0.5  # (two draws may round to one value: keep a spread)
    elif name == "ties_outlier":
        r = g.normal(size=N)
        r[N // 2] = 40.0
        r[: N // 3] = r[0]
    elif name == "one_hot":
        r = np.zeros(N)
        r[N // 2] = 1.0
    elif name == "boundary_tie":
        top, block = boundary_tie_layout(N)
        r = -2.0 - np.abs(g.normal(size=N))  # everything else: below the block
        r[block] = 1.0
        r[top] = 2.0 + 0.25 * np.arange(9, 0, -1)  # 4.25, 4.0, ... 2.25
    elif name == "constant":
        r = np.full(N, 0.3)
    elif name == "constant_exact":
        r = np.full(N, 0.25)
    else:
        raise KeyError(name)
    r = r.astype(np.float32)
    if float64_meaningful(name, N):
        r64 = r.astype(np.float64)
        assert r64.std() / max(1.0, abs(r64.mean())) >= 1e-4, (name, N)
    return r


def shapes(N):
    if N == 1:
        return CONSTANT
    return tuple(s for s in SHAPES if s != "boundary_tie" or N >= 9)


def cases(N):
    """(name, temp, rews) of every shape that exists at N, at every temperature it is run at."""
    for name in shapes(N):
        r = rewards(name, N)
        for temp in TEMPS + ((0.01,) if name == "normal" else ()):
            yield name, temp, r


def candidates(N, H=5, Nu=3, seed=0):
    """(Y0s [N][H][Nu], mu [H][Nu]) float32 for the CPU tests: clipped normals around a small mean, like the sampler's."""
    g = np.random.default_rng([seed, N, H, Nu])
    mu = (g.normal(size=(H, Nu)) * 0.1).astype(np.float32)
    Y0s = np.clip(mu + g.normal(size=(N, H, Nu)) * 0.7, -1, 1).astype(np.float32)
    return Y0s, mu


def expected_cem_indices(name, N):
    """The index list cem must take, written out from the construction of the shape (no sort): one_hot, boundary_tie and the
    constant cases only."""
    K = min(K_CEM, N)
    if name in CONSTANT:
        return list(range(N - 1, N - 1 - K, -1))
    if name == "one_hot":
        return ([N // 2] + [i for i in range(N - 1, -1, -1) if i != N // 2])[:K]
    if name == "boundary_tie":
        top, block = boundary_tie_layout(N)
        return (top + block[::-1])[:K]
    raise KeyError(name)
