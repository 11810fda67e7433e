"""The case table of the to-go record's tests (tests/test_togo.py on the checker and the host entry; tests/test_gpu_togo.py on the
device): the update alone over sizes, layouts, candidate forms, update rules and reward shapes, and the whole-plan, episode and
other-record cases with the checker's reference for each, computed once per process."""
from __future__ import annotations

import itertools
from dataclasses import dataclass

import numpy as np

import togo_checker as tc

f32 = np.float32

# ---- the update alone ------------------------------------------------------------------------------------------------------------
# N: one candidate per group of the chain and fewer (2), around a wavefront (63, 65), around the workgroup's 1024 threads (1000,
# 1025), and 2049: thirty-two rows per chain thread — the prefetch's sixteen, no round of 48, one tail block of sixteen — plus one
# more row for chain 0, so prefetch, tail block and the single-row loop all run, and three rewards per thread of score_block
NS = (2, 63, 65, 1000, 1025, 2049)
# (H, Nu): one element; one tile over two rows; Nu = 17 and 24: a group's last tile partial and tile starts off multiples of 16
SHAPES = ((1, 1), (2, 3), (7, 17), (50, 17), (5, 24))
# (block, min_tail), "H" standing for the case's H: every row a group; blocks of three; a tail of four; G = 1 both ways
LAYOUTS = ((1, 1), (3, 1), (1, 4), ("H", 1), (2, "H"))
# nan_step_t: one candidate NaN in step t ("from step t on" as the descending pass meets it: the groups with s_j <= t have it, the groups
# with s_j > t stay finite); nan_from_t: the same candidate NaN in every step from t to the end, as a diverged rollout leaves it —
# every group then holds it
KINDS = ("random", "late_tie", "all_equal", "nan_step_t", "nan_from_t", "inf_step0")
# (lazy, method, literal): lazy and materialised candidates under MBD's literal and identity updates and mppi
MODES = tuple(itertools.product((True, False), ((0, True), (0, False), (1, False))))
TEMP, SIGMA = 0.1, 0.37
ALPHAS = (0.9975, 0.93, 0.9323)  # (alpha_i, alpha_bar_i, alpha_bar_im1) of a mid-schedule step


def layout(H, lay):
    """(block, min_tail) of a LAYOUTS entry at horizon H; min_tail is held to [1, H]."""
    b, m = (H if x == "H" else x for x in lay)
    return int(b), int(min(max(m, 1), H))


def rewards(kind, N, H, seed):
    """(rews [N], rewss [N, H], t): the rewards per step of ``kind`` and their mean over the horizon in the oracle's order (a
    float32 ascending sum and one division would do for a test of the update alone: what the update reads is the pair as given).
    t: the step the kind is about (or -1)."""
    g = np.random.default_rng([seed, N, H])
    rewss = (g.normal(size=(N, H)) * 0.5 - 0.2).astype(f32)
    t = -1
    if kind == "late_tie":  # all candidates equal in one late step only
        t = H - 1
        rewss[:, t] = f32(0.25)
    elif kind == "all_equal":  # zero spread everywhere: the guard for MBD, NaN for mppi
        rewss[:] = rewss[0]
    elif kind == "nan_step_t":  # one candidate NaN in step t: groups with s_j > t stay finite
        t = H // 2
        rewss[N // 2, t] = np.nan
    elif kind == "nan_from_t":  # one candidate NaN from step t to the end: every group holds it
        t = H // 2
        rewss[N // 2, t:] = np.nan
    elif kind == "inf_step0":  # one candidate +inf in step 0 only: group 0 alone sees it
        t = 0
        rewss[N - 1, 0] = np.inf
    with np.errstate(all="ignore"):
        acc = np.zeros(N, f32)
        for h in range(H):
            acc = (acc + rewss[:, h]).astype(f32)
        rews = (acc / f32(H)).astype(f32)
    return rews, rewss, t


def step_case(N, H, Nu, lay, kind, mode):
    """One call of the update alone: dict of the arrays and settings ``mbd_debug_togo_step`` takes."""
    lazy, (method, literal) = mode
    block, min_tail = layout(H, lay)
    g = np.random.default_rng([N, H, Nu, block, min_tail])
    ybar = (g.normal(size=(H, Nu)) * 0.3).astype(f32)
    z = g.normal(size=(N, H, Nu)).astype(f32)
    rews, rewss, t = rewards(kind, N, H, 5)
    return dict(N=N, H=H, Nu=Nu, block=block, min_tail=min_tail, kind=kind, lazy=lazy, method=method, literal=literal, ybar=ybar,
                cand=z if lazy else values(z, SIGMA, ybar), rews=rews, rewss=rewss, t=t)


def values(z, sigma, ybar):
    """clip((z * sigma) + ybar, -1, 1), each operation a float32: what the consumers of a lazy plan's normals form."""
    y = (np.asarray(z, f32) * f32(sigma)).astype(f32)
    y = (y + np.asarray(ybar, f32)[None]).astype(f32)
    return np.ascontiguousarray(np.clip(y, f32(-1.0), f32(1.0)), f32)


def step_cases(N, H, Nu):
    """Every layout x reward shape at this size.  Below the largest N the candidate form and update rule rotate, so that each mode
    meets every shape and layout somewhere; at the largest N, where the chain runs its prefetch, its tail block and its single-row
    loop (which depend on N alone), every layout x reward shape meets all six modes — except at H = 50, where the checker's fifty
    updates of 2049 x 850 values per case would take the test from three seconds to eighteen, and the rotation stays."""
    out = []
    base = NS.index(N) + SHAPES.index((H, Nu))
    for li, lay in enumerate(LAYOUTS):
        for ki, kind in enumerate(KINDS):
            modes = MODES if N == NS[-1] and H < 50 else (MODES[(base + li + ki) % len(MODES)],)
            out.extend(step_case(N, H, Nu, lay, kind, mode) for mode in modes)
    return out


def checked_step(orc, c):
    """The checker's result for a step case."""
    Y = values(c["cand"], SIGMA, c["ybar"]) if c["lazy"] else c["cand"]
    return tc.update(orc, c["method"], c["rews"], c["rewss"], Y, c["ybar"], tc.groups(c["H"], c["block"], c["min_tail"]), TEMP,
                     alphas=ALPHAS, literal=c["literal"], sigma=SIGMA)


def what(c):
    return (f"N={c['N']} H={c['H']} Nu={c['Nu']} block={c['block']} min_tail={c['min_tail']} {c['kind']} "
            f"{'lazy' if c['lazy'] else 'materialised'} {'mppi' if c['method'] else 'mbd'}{'' if c['literal'] else '-identity'}")


def same(got, ref, what, same_bits):
    """Equality by bit pattern with a NaN — whatever its payload — where and only where the checker has one."""
    got, ref = np.asarray(got, f32).reshape(-1), np.asarray(ref, f32).reshape(-1)
    assert got.size == ref.size, f"{what}: {got.size} values against {ref.size}"
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN at {np.flatnonzero(np.isnan(got) != nan)[:8]} where the checker has none, or the reverse"
    same_bits(got[~nan], ref[~nan], what)


# ---- whole plans, episodes, other records ----------------------------------------------------------------------------------------
ND, H = 6, 8
T, K, E = 4, 2, 1
SIGMA_REC = (1.0, 0.5, 0.0)
CAR2D_S0 = (0.5, 0.5, 0.0)  # car2d's mppi cases start beside the goal region: from its reset state all rewards are equal


@dataclass(frozen=True)
class PlanCase:
    name: str
    N: int
    block: int
    method: int = 0

    @property
    def state0(self):
        return np.array(CAR2D_S0, f32) if self.name == "car2d" and self.method == 1 else None

    @property
    def id(self):
        return f"{self.name}-N{self.N}-block{self.block}-{'mppi' if self.method else 'mbd'}"


PLAN_CASES = [PlanCase(n, N, b, m) for n in ("hopper", "cartpole", "humanoidrun", "car2d") for N in (64, 130) for b in (1, 3)
              for m in (0, 1)]
EPISODE_CASES = [PlanCase("hopper", 64, 3, 0), PlanCase("hopper", 64, 1, 1)]

_CACHE = {}


def plan_reference(oenv, s0, key, case: PlanCase, impl=1):
    k = ("plan", case, bytes(np.asarray(s0, f32)), bytes(np.asarray(key, np.uint32)), impl)
    if k not in _CACHE:
        _CACHE[k] = tc.run(oenv, s0, key, case.N, H, ND, TEMP, case.block, 1, case.method, impl)
    return _CACHE[k]


def episode_reference(oenv, s0, key, case: PlanCase, impl=1):
    k = ("episode", case, bytes(np.asarray(s0, f32)), bytes(np.asarray(key, np.uint32)), impl)
    if k not in _CACHE:
        _CACHE[k] = tc.episode(oenv, s0, key, case.N, H, ND, TEMP, T, K, E, case.block, 1, case.method, SIGMA_REC, impl)
    return _CACHE[k]
