"""The table of inputs the elite record's two launches and their host restatement are held to the checker over (tests/test_elites.py
on the host form, tests/test_gpu_elites.py on the kernels), and the whole-plan and episode cases with the checker's reference for
each, computed once per process."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import adapt_cases as ac_cases
import elites_checker as ec
import weighting_checker as wc

f32 = np.float32
NS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 8193, 12289)  # a wavefront, the workgroup, the registers' 8192, beyond
KS = (1, 5, 32)
KINDS = ("random", "equal", "ties", "zeros", "nonfinite", "few", "none")
PLANTED = (0, 63, 64, 1023, 1024)  # ... and N - 1
HNU = 5
SIGMA = f32(0.37)


def rewards(N, kind, seed=0):
    """[N] rewards of a kind.  random: distinct values; equal: one value; ties: four values, so that the equal maxima and every
    later rank cross the wavefronts' and the workgroup's boundaries, with one larger value planted at the boundaries themselves;
    zeros: +0 beside -0 above negative values; nonfinite: NaN, +inf and -inf planted at 0, 63, 64, 1023, 1024 and N - 1; few: fewer
    finite entries than any k > 3; none: no finite entry."""
    rng = np.random.default_rng(1000 * N + seed)
    r = rng.standard_normal(N).astype(f32)
    if kind == "equal":
        r[:] = f32(-1.25)
    elif kind == "ties":
        r = rng.integers(0, 4, N).astype(f32)
        for i in (63, 64, 1023, 1024, N - 1):
            if 0 <= i < N:
                r[i] = f32(7)
    elif kind == "zeros":
        r = -np.abs(r) - f32(1)
        z = rng.permutation(N)[:max(N // 3, 1)]
        r[z] = np.where(np.arange(z.size) % 2 == 0, f32(-0.0), f32(0.0))
    elif kind == "nonfinite":
        bad = (np.nan, np.inf, -np.inf)
        for j, i in enumerate(PLANTED + (N - 1,)):
            if 0 <= i < N:
                r[i] = f32(bad[j % 3])
        if N > 8:  # (a NaN with its sign bit set and a payload, and the largest finite value beside an infinity)
            r[5] = np.array([0xffc12345], np.uint32).view(f32)[0]
            r[6] = np.finfo(f32).max
    elif kind == "few":
        keep = rng.permutation(N)[:min(3, N)]
        out = np.full(N, np.nan, f32)
        out[1::2] = np.inf
        out[keep] = r[keep]
        r = out
    elif kind == "none":
        r = np.where(np.arange(N) % 3 == 0, np.nan, np.where(np.arange(N) % 3 == 1, np.inf, -np.inf)).astype(f32)
    return np.ascontiguousarray(r, f32)


def case(N, k, kind, lazy, nominal=1, with_shape=True, seed=0):
    """One input of the table, or None where the record would be refused (n_elites + nominal >= N): rews, cand [N, HNu] (normals
    when lazy), ybar, sigma, g (one frozen element; None without a shape), E_in — min(k, 2) elites the step finds —, rec."""
    if k + nominal >= N:
        return None
    rng = np.random.default_rng(7 * N + 13 * k + seed)
    cand = rng.standard_normal((N, HNU)).astype(f32)
    if not lazy:
        cand = ec.clip(cand * f32(0.6))
    ybar = (rng.standard_normal(HNU) * 0.4).astype(f32)
    ybar[0] = f32(1.5)  # (outside the clip: the nominal of a materialised plan is clip(Ybar))
    g = None
    if with_shape:
        g = (0.5 + rng.random(HNU)).astype(f32)
        g[2] = 0.0
    E_in = ec.clip(rng.standard_normal((min(k, 2), HNU)) * 0.8)
    return dict(rews=rewards(N, kind, seed), cand=cand, ybar=ybar, sigma=SIGMA, lazy=lazy, g=g, E_in=E_in,
                rec=ec.Record(n_elites=k, nominal=bool(nominal), carry=False), N=N, k=k, kind=kind)


def table():
    """Every (N, k, kind) with lazy and materialised candidates; the nominal and the shape alternate so that both values of each
    meet every kind."""
    out = []
    for a, N in enumerate(NS):
        for b, k in enumerate(KS):
            for c, kind in enumerate(KINDS):
                for lazy in (True, False):
                    x = case(N, k, kind, lazy, nominal=(a + b + c) % 2, with_shape=(a + c) % 2 == 0)
                    if x is not None:
                        out.append(x)
    return out


def what(c):
    return f"N={c['N']} k={c['k']} {c['kind']} lazy={c['lazy']} nominal={c['rec'].nominal} shape={c['g'] is not None}"


def checked(c):
    return ec.step(c["rews"], c["cand"], c["ybar"], c["sigma"], c["lazy"], c["g"], c["rec"], c["E_in"])


def assert_step(got, ref, what_, same_bits, with_cand=True):
    """A host or device result against the checker's, by bit pattern; what lies behind count' has all bits set."""
    n = ref["count"]
    assert got["count"] == n and got["kept"] == ref["kept"], f"{what_}: count {got['count']} / {n}, kept {got['kept']} / {ref['kept']}"
    same_bits(np.asarray(got["top"], f32), np.asarray(ref["top"], f32), f"{what_}: top")
    assert list(got["src"][:n]) == list(ref["src"]), f"{what_}: src"
    same_bits(got["R"][:n], ref["R"], f"{what_}: R")
    same_bits(got["E"][:n], ref["E"], f"{what_}: E")
    for name in ("src", "R", "E"):
        rest = np.ascontiguousarray(got[name][n:]).view(np.uint32)
        assert (rest == 0xffffffff).all(), f"{what_}: {name} behind count' is untouched"
    if with_cand:
        same_bits(got["cand"], ref["cand"], f"{what_}: the candidates behind the injection")


# ---- whole plans and episodes ----------------------------------------------------------------------------------------------------
ND, TEMP = ac_cases.ND, ac_cases.TEMP
T, K, E = ac_cases.T, ac_cases.K, ac_cases.E
SIZES = ac_cases.SIZES
RECORDS = {"e3n": (3, 1), "e1": (1, 0), "n": (0, 1), "e32n": (32, 1)}  # (n_elites, nominal)
SIGMA_REC = ac_cases.SIGMA


def lazy_of(name, method):
    return method == 0 and name != "car2d"


@dataclass(frozen=True)
class PlanCase:
    name: str
    method: int = 0       # 0 MBD, 1 mppi
    rec: str = "e3n"      # a key of RECORDS
    shape: bool = False   # adapt_cases.plan_shape: one frozen element
    knots: int = 0        # a noise basis of that many knots
    ess: bool = False     # a weighting record with an ESS target
    adapt: bool = False   # an adapt record beside the elite record

    @property
    def record(self):
        n, nom = RECORDS[self.rec]
        return ec.Record(n_elites=n, nominal=bool(nom), carry=False)

    @property
    def wrec(self):
        return ac_cases.ESS if self.ess else wc.Record(reject_nonfinite=False)

    @property
    def state0(self):
        """car2d's rewards from its reset state are all equal (adapt_cases.PlanCase.state0): its cases start beside the goal."""
        return np.array(ac_cases.CAR2D_S0, f32) if self.name == "car2d" else None

    @property
    def id(self):
        return "-".join([self.name, "mppi" if self.method else "mbd", self.rec] + (["shape"] if self.shape else []) +
                        ([f"knots{self.knots}"] if self.knots else []) + (["ess"] if self.ess else []) +
                        (["adapt"] if self.adapt else []))


PLAN_CASES = [PlanCase(n, m, r) for n in sorted(SIZES) for m in (0, 1) for r in RECORDS] + \
    [PlanCase("hopper", 0, "e3n", shape=True), PlanCase("ant", 1, "e3n", shape=True), PlanCase("hopper", 0, "e3n", knots=3),
     PlanCase("ant", 0, "e3n", ess=True), PlanCase("hopper", 0, "e3n", shape=True, adapt=True),
     PlanCase("car2d", 1, "e3n", adapt=True)]


def state_of(case, carry=False):
    N, H, Nu = SIZES[case.name]
    rec = ec.Record(**dict(case.record.kwargs(), carry=carry))
    g = ac_cases.plan_shape(H, Nu) if getattr(case, "shape", False) else None
    return ec.State(rec, H, Nu, lazy_of(case.name, case.method), g)


_CACHE = {}


def plan_reference(orc, oenv, s0, key, case: PlanCase, impl=1):
    """dict(mu_0ts, details, elog [(count, kept, top)], steps, E, R, src) of mbd_plan_run under the case's records."""
    k = ("plan", case, bytes(np.asarray(s0, f32)), bytes(np.asarray(key, np.uint32)), impl)
    if k not in _CACHE:
        import adapt_checker as ac
        from noise_basis_checker import BasisOracle, basis_of
        N, H, Nu = SIZES[case.name]
        st = state_of(case)
        g = ac_cases.plan_shape(H, Nu) if case.shape else None
        W = basis_of(H, case.knots) if case.knots else None
        adapt = ac.State(ac_cases.RULE, H, Nu, g, g, W) if case.adapt else None
        env = oenv
        if adapt is None and (g is not None or W is not None):  # (under an adapt record its oracle samples under shape and basis)
            import copy
            env = copy.copy(oenv)
            env.orc = BasisOracle(oenv.orc, W, g)
        if case.method == 0:
            out = ec.run(env.orc, env, s0, key, N, H, ND, TEMP, st, rec=case.wrec, impl=impl, adapt=adapt)
        else:
            out = ec.pi_run(env, s0, key, N, H, ND, TEMP, 1, st, impl, rec=case.wrec, adapt=adapt)
        _CACHE[k] = dict(out, elog=list(st.log), steps=list(st.steps), E=st.E, R=st.R, src=st.src,
                         table=None if adapt is None else adapt.a.copy())
    return _CACHE[k]


@dataclass(frozen=True)
class EpisodeCase:
    name: str = "hopper"
    method: int = 0
    carry: bool = True
    D: int = 0            # a delay record of D ticks
    pick: int = 0         # a pick record's mask
    plant: float = 0.0    # a plant whose masses are scaled by this
    rec: str = "e3n"
    shape: bool = False

    @property
    def record(self):
        n, nom = RECORDS[self.rec]
        return ec.Record(n_elites=n, nominal=bool(nom), carry=self.carry)

    @property
    def id(self):
        return "-".join([self.name, "mppi" if self.method else "mbd", "carry" if self.carry else "nocarry"] +
                        ([f"D{self.D}"] if self.D else []) + ([f"pick{self.pick}"] if self.pick else []) +
                        ([f"plant{self.plant}"] if self.plant else []))


EPISODE_CASES = [EpisodeCase(carry=True), EpisodeCase(carry=False), EpisodeCase(carry=True, D=1), EpisodeCase(carry=True, pick=7),
                 EpisodeCase(method=1, carry=True), EpisodeCase(carry=True, plant=1.3), EpisodeCase(name="car2d", carry=True)]


def episode_reference(orc, oenv, s0, key, case: EpisodeCase, impl=1, plant=None):
    """dict(actions, rewards, states, means, elites, picks, elog, E, R, src) of mbd_plan_run_mpc under the case's records."""
    k = ("episode", case, bytes(np.asarray(s0, f32)), bytes(np.asarray(key, np.uint32)), impl)
    if k not in _CACHE:
        N, H, Nu = SIZES[case.name]
        st = state_of(case, carry=case.carry)
        out = ec.episode(oenv, s0, key, N, H, ND, TEMP, T, K, E, st, D=case.D, method=1 if case.method else None, sigma=SIGMA_REC,
                         impl=impl, pick_mask=case.pick or None, plant=plant)
        _CACHE[k] = dict(out, elog=list(st.log), steps=list(st.steps), E=st.E, R=st.R, src=st.src)
    return _CACHE[k]


cpu_env = ac_cases.cpu_env
