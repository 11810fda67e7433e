"""The table of cases for the weighting record (include/mbd_hip.h mbd_weighting), shared by tests/test_weighting.py (the checker
against the existing C checker and against the library's host restatement, on the CPU) and tests/test_gpu_weighting.py (the kernel
against the checker, by bit pattern).  numpy only; seeded; nothing here touches the checker, the library or a device.

A case is ``Case(name, N, rews float32 [N], temp, rec)``: the rewards buffer a score step receives, the plan's temperature T0 and the
record (weighting_checker.Record).  The reward shapes are tests/pi_inputs.py's; on top of them, per size:

  plain/<shape>      every shape that exists at N, at temperature 0.1, rejection on, ess_frac = 0: nothing is dropped — where the
                     spread is not below the guard these must have the bits of the score without a record
  planted            `normal` with NaN, +inf and -inf planted, in turn, at the indices 0, 63, 64, 1023, 1024 and N - 1 that exist
  planted_ess        the same rewards under ess_frac = 0.25, bracket [0.01, 10], 12 steps
  all_dropped        every entry NaN, +inf or -inf
  one_kept           the same with one finite entry, at N // 2
  tied_max           the maximum tied k = min(4, N) times and the target below k: ess(temp_min) >= k already — the temp_min clamp
  target_kept        ess_frac = 1: the target is the kept count, which no temperature of the bracket exceeds — the temp_max clamp
                     (shape `normal`; at N = 1 the one entry already meets it: temp_min)
  bracket            `normal` under ess_frac = 0.25, bracket [0.01, 10], 12 steps: the target lies inside, the loop runs (N >= 8)
  bracket32          the same with 32 steps (N = 1025 only: the most passes the kernel makes)

SIZES are the smallest sizes at which each code path of the weigh kernel can go wrong: one and two entries, around a wavefront
(63, 64, 65), around the workgroup's 1024 threads (1023, 1024, 1025), a third stride (2049), beyond the 8192 candidates held in
registers (8193), beyond the 12 288 whose weights fit the default LDS window (12 289: the raised window and the row-major
weighted mean), beyond the 36 864 that fit the raised window (36 865: e[] in the plan's global scratch).  `reach(cases, branch_of)` asserts that the table hits every arm of the selection and both regimes."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import pi_inputs as pi
from weighting_checker import Record

SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 8193, 12289, 36865)
PLANT_AT = (0, 63, 64, 1023, 1024, -1)
NONFINITE = (np.nan, np.inf, -np.inf)
TEMP = 0.1
REJECT = Record(reject_nonfinite=True)
ESS = Record(reject_nonfinite=True, ess_frac=0.25, temp_min=0.01, temp_max=10.0, iters=12)
REGS_MAX = 8192  # candidates held in registers
LDS_MAX = 36 * 1024  # candidates whose e[] fits the raised LDS window (csrc/mbd_internal.h kLdsN)


@dataclass(frozen=True)
class Case:
    name: str
    N: int
    rews: np.ndarray
    temp: float
    rec: Record

    @property
    def id(self):
        return f"{self.name}-N{self.N}"

    @property
    def dropped(self):
        return int((~np.isfinite(self.rews)).sum()) if self.rec.reject_nonfinite else 0


def _base(N):
    return pi.rewards("normal", N) if N >= 2 else np.array([0.3], np.float32)


def planted(N):
    r = _base(N).copy()
    for j, at in enumerate(sorted({a % N for a in PLANT_AT if -N <= a < N})):
        r[at] = NONFINITE[j % 3]
    return r


def cases(N):
    out = []
    for shape in pi.shapes(N):
        out.append(Case(f"plain/{shape}", N, pi.rewards(shape, N), TEMP, REJECT))
    out.append(Case("planted", N, planted(N), TEMP, REJECT))
    out.append(Case("planted_ess", N, planted(N), TEMP, ESS))
    out.append(Case("all_dropped", N, np.array([NONFINITE[i % 3] for i in range(N)], np.float32), TEMP, REJECT))
    one = np.array([NONFINITE[i % 3] for i in range(N)], np.float32)
    one[N // 2] = -2.5
    out.append(Case("one_kept", N, one, TEMP, ESS))
    k = min(4, N)
    tied = -np.abs(_base(N)) - 1.0
    tied[np.linspace(0, N - 1, k).astype(int)] = 3.0
    out.append(Case("tied_max", N, tied.astype(np.float32), TEMP, Record(True, min(1.0, 0.5 * k / N), 0.01, 10.0, 12)))
    out.append(Case("target_kept", N, _base(N), TEMP, Record(True, 1.0, 0.01, 10.0, 12)))
    if N >= 8:
        out.append(Case("bracket", N, _base(N), TEMP, ESS))
    if N == 1025:
        out.append(Case("bracket32", N, _base(N), TEMP, Record(True, 0.25, 0.01, 10.0, 32)))
    return out


def table():
    return [c for N in SIZES for c in cases(N)]


def reach(cs, branch_of):
    """Every arm of the selection — the fixed temperature, both clamps, the loop, nothing kept — is taken by some case, in the
    register regime (N <= 8192) and beyond it; some case drops entries in each regime; the planted indices exist where they can."""
    seen = {(branch_of(c), c.N > REGS_MAX) for c in cs}
    for beyond in (False, True):
        for b in ("fixed", "min", "max", "loop", "none"):
            assert (b, beyond) in seen, (b, beyond)
        assert any(c.dropped and 0 < c.dropped < c.N and (c.N > REGS_MAX) == beyond for c in cs)
    assert any(48 * 1024 < c.N * 4 <= LDS_MAX * 4 for c in cs)  # beyond the default LDS window, inside the raised one
    assert any(c.N > LDS_MAX for c in cs)  # beyond the raised one: the global scratch
    big = [c for c in cs if c.name == "planted" and c.N > 1024]
    assert big and all((~np.isfinite(c.rews[[0, 63, 64, 1023, 1024, c.N - 1]])).all() for c in big)
