"""The whole-plan and episode cases of the adapt record's tests (tests/test_adapt.py holds them to "no step is skipped" on the checker
alone; tests/test_gpu_adapt.py runs them on the device), and the checker's reference for each, computed once per process."""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import adapt_checker as ac
import weighting_checker as wc
from noise_basis_checker import basis_of

f32 = np.float32
ND, TEMP = 6, 0.1
T, K, E = 3, 2, 2
SIZES = {"hopper": (70, 7, 3), "ant": (33, 4, 8), "humanoidrun": (40, 5, 17), "car2d": (33, 6, 2)}  # env: (N, H, Nu)
RULE = ac.Record(rate=0.5, a_min=0.5, a_max=2.0, carry=True)
ESS = wc.Record(reject_nonfinite=True, ess_frac=0.3, temp_min=0.02, temp_max=5.0, iters=8)
SIGMA = (1.0, 0.5, 0.0)  # an mppi episode's sigma record
CAR2D_S0 = (0.5, 0.5, 0.0)  # (x, y, theta): PlanCase.state0


def plan_shape(H, Nu):
    """The noise shape of the whole-plan tests: distinct values around 1, the last actuator of row 1 frozen."""
    g = (0.75 + 0.5 * np.linspace(0, 1, H * Nu)).astype(f32).reshape(H, Nu)
    g[1, Nu - 1] = 0.0
    return g


@dataclass(frozen=True)
class PlanCase:
    name: str
    method: int = 0       # 0 MBD, 1 mppi
    shape: bool = False
    knots: int = 0        # a noise basis of that many knots
    ess: bool = False     # a weighting record with an ESS target

    @property
    def wrec(self):
        return ESS if self.ess else wc.Record(reject_nonfinite=False)

    @property
    def state0(self):
        """The start state where it is not the env's reset state.  car2d's rewards over six steps from its reset state are all
        equal, and mppi's score, which has no guard against a zero spread, then makes every weight NaN with or without an adapt
        record: its mppi cases start beside the goal region instead, where the candidates' rewards differ in every step."""
        return np.array(CAR2D_S0, f32) if self.name == "car2d" and self.method == 1 else None

    @property
    def id(self):
        return "-".join([self.name, "mppi" if self.method else "mbd"] + (["shape"] if self.shape else []) +
                        ([f"knots{self.knots}"] if self.knots else []) + (["ess"] if self.ess else []))


PLAN_CASES = [PlanCase(n, m, s) for n in sorted(SIZES) for m in (0, 1) for s in (False, True)] + \
    [PlanCase("hopper", 0, True, knots=3), PlanCase("ant", 0, False, ess=True)]


@dataclass(frozen=True)
class EpisodeCase:
    name: str = "hopper"
    method: int = 0
    carry: bool = True
    shape: str = ""       # "", "always" or "warm" (MBD_NOISE_WARM_TICKS)
    D: int = 0            # a delay record of D ticks
    pick: int = 0         # a pick record's mask

    @property
    def id(self):
        return "-".join([self.name, "mppi" if self.method else "mbd", "carry" if self.carry else "nocarry"] +
                        ([f"shape_{self.shape}"] if self.shape else []) + ([f"D{self.D}"] if self.D else []) +
                        ([f"pick{self.pick}"] if self.pick else []))


EPISODE_CASES = [EpisodeCase(carry=True, shape="warm"), EpisodeCase(carry=False, shape="always"), EpisodeCase(carry=True, D=1),
                 EpisodeCase(carry=True, pick=7), EpisodeCase(method=1, carry=True, shape="always"),
                 EpisodeCase(name="car2d", carry=True, shape="warm")]


def state_of(case, rule=RULE):
    """The checker's table state for a case."""
    N, H, Nu = SIZES[case.name]
    g = plan_shape(H, Nu)
    if isinstance(case, PlanCase):
        ga = gw = g if case.shape else None
        W = basis_of(H, case.knots) if case.knots else None
        return ac.State(rule, H, Nu, ga, gw, W)
    ga = g if case.shape == "always" else None
    gw = g if case.shape else None
    return ac.State(ac.Record(**dict(rule.kwargs(), carry=case.carry)), H, Nu, ga, gw)


_CACHE = {}


def plan_reference(orc, oenv, s0, key, case: PlanCase, impl=1):
    """dict(mu_0ts, tables [Nd-1, HNu], log [(S, skipped)]) of mbd_plan_run under the case's records."""
    k = ("plan", case, bytes(np.asarray(s0, f32)), bytes(np.asarray(key, np.uint32)), impl)
    if k not in _CACHE:
        N, H, Nu = SIZES[case.name]
        st = state_of(case)
        if case.method == 0:
            out = ac.run(orc, oenv, s0, key, N, H, ND, TEMP, st, rec=case.wrec, impl=impl)
        else:
            out = ac.pi_run(oenv, s0, key, N, H, ND, TEMP, 1, st, impl, rec=case.wrec)
        _CACHE[k] = dict(out, tables=np.stack(st.tables), log=list(st.log))
    return _CACHE[k]


def episode_reference(orc, oenv, s0, key, case: EpisodeCase, impl=1):
    """dict(actions, rewards, states, means, tables [T, H, Nu], log) of mbd_plan_run_mpc under the case's records."""
    k = ("episode", case, bytes(np.asarray(s0, f32)), bytes(np.asarray(key, np.uint32)), impl)
    if k not in _CACHE:
        N, H, Nu = SIZES[case.name]
        st = state_of(case)
        out = ac.episode(oenv, s0, key, N, H, ND, TEMP, T, K, E, st, D=case.D, method=1 if case.method else None, sigma=SIGMA,
                         impl=impl, pick_mask=case.pick or None)
        _CACHE[k] = dict(out, log=list(st.log))
    return _CACHE[k]


@functools.lru_cache(maxsize=None)
def cpu_env(orc, name):
    """(OracleEnv, state0) without a device: the env's reset from prng_key(3), layout 1."""
    from conftest import load_model
    from oracle.planner import OracleEnv
    if name == "car2d":
        oe = OracleEnv(orc, "car2d")
    else:
        m = load_model(name)
        oe = OracleEnv(orc, name, m.to_struct(), init_q=m.init_q)
    return oe, np.asarray(oe.reset(orc.prng_key(3), 1), f32).reshape(-1)
