"""-m gpu: the update kernels of a SWEEP on their own (mbd_debug_sweep_update, include/mbd_hip_debug.h) against the checker, by bit
pattern, at every plan count and size.

A sweep advances P plans in lockstep, and behind its one rollout launch it runs update code a single plan never runs:
score_wmean_batch_kernel<V, GIVEN> (rounds of 32 rows, rewards re-read on every pass), per-plan temperatures and strides, xcd_tile
with a non-zero first workgroup, the plan-to-XCD remap of a multiple of 8 plans, and the blockIdx.y forms of the path-integral
kernels.  Every other sweep test is a whole run on organic rewards compared with plans run alone.  Here the step under test is what
a lockstep step launches behind its rollout, on uploaded arrays (tests/sweep_update_inputs.py): normals or candidates, means, and
the reward shapes of tests/pi_inputs.py — exact ties inside and across lanes, underflowed weights, zero spread, outliers —, plan k
of a call with another shape and another temperature than its neighbours.  Nothing rolls out.

  a  MBD sweeps at candidate counts around every boundary of the batch body (prefetch of 16 / V rows, rounds of 32 / V, tail of
     16 / V, the 64-group remainder) for V = 1, 2, 4 and the library's choice, three row widths
  b  every plan count 1 .. 32 and tile counts 1 .. 9 (the bijection (plan, tile) is held through the NaN-filled outputs)
  c  mppi, cma-es and cem sweeps at every size and case of pi_inputs
  d  MBD and mppi sweeps under a weighting record (the GIVEN form), rewards with NaN and infinite entries
  e  the demo blend
  f  a plan whose rewards are all NaN leaves the other plans' outputs alone
  g  the entry's refusals, and a run after entry calls

Every comparison is by bit pattern (state_inputs.same_bits).  equal_nan stands only where the checker itself yields NaN: the
path-integral constant shapes and N = 1 (zero spread, no guard), and the mean reward of a plan whose every reward a weighting
record drops.  No tolerance anywhere.  A checker result is computed once and reused across the lever values.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import pi_inputs as pi
import sweep_update_inputs as su
import weighting_checker as wc
from state_inputs import same_bits

pytestmark = pytest.mark.gpu

ND, I = 30, 17  # the MBD sweeps' diffusion steps and the step whose schedule values the entry takes
BETA0, BETAT = 1e-4, 1e-2  # (Args' defaults)
PI_ND = 4
RECORDS = (wc.Record(True, 0.0), wc.Record(True, 0.5, 0.01, 10.0, 12))


@pytest.fixture(scope="module")
def gpu(lib):
    from mbd_hip import _capi
    if _capi.device_count() < 1:
        pytest.fail("tests/test_gpu_sweep_updates.py needs a GPU")
    return _capi


@functools.lru_cache(maxsize=None)
def _env(name):
    from mbd_hip.envs import get_env
    return get_env(name)


def _mbd_sweep(name, H, N, P, temps, demo=False, literal=True, Nd=ND):
    from mbd_hip.planners.mbd_planner import Args, Sweep
    args = Args(env_name=name, Nsample=N, Hsample=H, Ndiffuse=Nd, temp_sample=0.2, enable_demo=demo,
                disable_recommended_params=True, not_render=True)
    return Sweep(_env(name), args, P, temps=temps, literal_score=literal)


def _pi_sweep(name, H, N, P, temps, method, Nd=PI_ND):
    from mbd_hip.planners.mbd_planner import Sweep
    from mbd_hip.planners.path_integral import Args
    args = Args(env_name=name, Nsample=N, Hsample=H, Nrefine=Nd, temp_sample=0.2, disable_recommended_params=True)
    return Sweep(_env(name), args, P, temps=temps, update_method=method)


def _temp(temps, k):
    """Plan k's temperature: the k-th the sweep was created with."""
    return float(np.float32(temps[k]))


def _mbd_ref(orc, sched, rews, Y, ybar, temp, literal=True, lp=None, rew_xref=0.0):
    """(Ybar_{i-1} [HNu], weights [N], mean reward) of one plan by the checker."""
    a, ab, _ = sched
    out, w, m = orc.score_update(rews, Y, ybar, float(a[I]), float(ab[I]), float(ab[I - 1]), temp, lp_demo=lp, rew_xref=rew_xref,
                                 literal=literal)
    assert np.isfinite(out).all() and np.isfinite(w).all() and np.isfinite(m)  # (the guard: an MBD step has no NaN)
    return out, w, np.float32(m)


def _same_plans(got, refs, what):
    """The outputs of all plans of a call against the checker's (out, weights, mean reward) per plan."""
    same_bits(got["weights"], np.stack([r[1] for r in refs]), f"{what}: weights")
    same_bits(got["rew_mean"], np.array([r[2] for r in refs], np.float32), f"{what}: mean reward")
    same_bits(got["ybar"], np.stack([r[0] for r in refs]), f"{what}: Ybar_(i-1)")


def _run_mbd(gpu, orc, levers, name, H, N, P, vs, literal=True):
    HNu = H * _env(name).action_size
    temps = su.MBD_TEMPS[:P]
    sched = orc.schedule(BETA0, BETAT, ND)
    z, ybar = su.normals(P, N, HNu), su.means(P, HNu)
    Y = su.values(z, sched[2][I], ybar)
    sweep = _mbd_sweep(name, H, N, P, temps, literal=literal)
    seen = set()
    try:
        for shapes in su.rounds(N, P):
            rews = np.stack([pi.rewards(s, N) for s in shapes])
            refs = [_mbd_ref(orc, sched, rews[k], Y[k], ybar[k], _temp(temps, k), literal) for k in range(P)]
            seen.update(shapes)
            for v in vs:
                levers(MBD_WMEAN_V=v)
                _same_plans(gpu.debug_sweep_update(sweep.h, I, z, ybar, rews), refs, f"{name} N={N} P={P} {shapes} MBD_WMEAN_V={v}")
    finally:
        sweep.close()
    assert seen == set(pi.shapes(N))


# ---- a: ragged sizes, MBD sweeps ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", su.RAGGED_N)
@pytest.mark.parametrize("name,H", su.WIDTHS)
def test_mbd_sweep_update_ragged_sizes(gpu, orc, levers, name, H, N):
    """score_wmean_batch_kernel<V> of an MBD sweep (std_guard = 1, the literal score form, lazy candidates formed from the normals)
    at candidate counts on either side of the prefetch (64 x 16 / V), of prefetch + one round (64 x 48 / V), of prefetch + tail
    (64 x 32 / V) and of a partial group of 64, for MBD_WMEAN_V = 1, 2, 4 and unset; H Nu = 7, 90 and 340 (an odd row stride);
    three plans (two from N = 8192 on), each with its own reward shape and temperature; every shape at every N.  Weights, the
    mean reward and Ybar_(i-1) of every plan against orc.score_update, bit for bit.  At N = 12 288 the launch of V = 4 would ask
    for more than 64 KiB of LDS: the library takes V = 2 there (same bits)."""
    _run_mbd(gpu, orc, levers, name, H, N, su.ragged_plans(N), su.WMEAN_V)


def test_mbd_sweep_update_without_the_literal_score_form(gpu, orc, levers):
    """The same with literal_score off (the weighted mean itself is the new Ybar), at a size with a round, a tail and a remainder."""
    _run_mbd(gpu, orc, levers, "hopper", 30, 3137, 3, su.WMEAN_V, literal=False)


def test_sweep_of_more_than_12288_candidates_is_refused(gpu):
    with pytest.raises(gpu.MbdError, match="12288") as e:
        _mbd_sweep("cartpole", 7, 12289, 2, None)
    assert e.value.code == gpu.MBD_ERR_UNSUPPORTED


# ---- b: plan counts and tile counts ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", su.MATRIX_N)
@pytest.mark.parametrize("name,H", [("cartpole", h) for h in su.TILE_H] + [("humanoidrun", 20)])
def test_mbd_sweep_update_plan_and_tile_counts(gpu, orc, levers, name, H, N):
    """Every plan count P = 1 .. 32 — the remap of a multiple of 8 plans (k = c + 8 (m / T), tile = m % T) and xcd_tile with every
    first workgroup otherwise — at tile counts 1 .. 9 under V = 1 (cartpole, Nu = 1, H = 1 .. 144; the last tile ragged under V = 2
    and 4) and at humanoidrun's 22 / 11 / 6 tiles, each under V = 1, 2, 4.  Plan k's normals, mean, rewards (the shape cycle at k,
    permuted by k) and temperature depend on k alone, so its checker result is computed once and serves every P.  The outputs of
    ALL plans are compared: they were NaN before the launch, so a (plan, tile) pair no workgroup took shows, and a pair taken by
    the wrong plan's data differs."""
    PM = su.MAX_PLANS
    HNu = H * _env(name).action_size
    temps = (0.1 + 0.03 * np.arange(PM)).astype(np.float32)
    sched = orc.schedule(BETA0, BETAT, ND)
    z, ybar = su.normals(PM, N, HNu), su.means(PM, HNu)
    Y = su.values(z, sched[2][I], ybar)
    rews = np.stack([su.plan_rewards(k, N) for k in range(PM)])
    refs = [_mbd_ref(orc, sched, rews[k], Y[k], ybar[k], _temp(temps, k)) for k in range(PM)]
    for P in range(1, PM + 1):
        sweep = _mbd_sweep(name, H, N, P, temps[:P])
        try:
            for v in (1, 2, 4):
                levers(MBD_WMEAN_V=v)
                _same_plans(gpu.debug_sweep_update(sweep.h, I, z[:P], ybar[:P], rews[:P]), refs[:P],
                            f"{name} H={H} N={N} P={P} MBD_WMEAN_V={v}")
        finally:
            sweep.close()


# ---- c: path-integral sweeps -------------------------------------------------------------------------------------------------
def _same_pi(method, N, shape, got, k, ref, what):
    mu_r, sigma_r, w_r, rm_r = ref
    mu, w, rm = got["ybar"][k], got["weights"][k], got["rew_mean"][k]
    same_bits(rm, np.float32(rm_r), f"{what}: mean reward")
    if shape in pi.CONSTANT or N == 1:  # (zero spread and no guard: the checker's weights may be NaN)
        assert np.array_equal(w, w_r, equal_nan=True), f"{what}: weights"
        if method == 3:
            assert np.isfinite(mu_r).all(), what
            same_bits(mu, mu_r, f"{what}: cem mean")
        else:
            assert np.array_equal(mu, mu_r.reshape(-1), equal_nan=True), f"{what}: mean"
        if method == 2:
            assert np.array_equal(got["sigma"][k], np.float32(sigma_r), equal_nan=True), f"{what}: sigma"
    else:
        assert np.isfinite(w_r).all() and np.isfinite(mu_r).all() and np.isfinite(sigma_r), what
        same_bits(w, w_r, f"{what}: weights")
        same_bits(mu, mu_r, f"{what}: mean")
        if method == 2:
            same_bits(got["sigma"][k], np.float32(sigma_r), f"{what}: sigma")
    if method == 3 and shape in pi.CONSTANT + ("one_hot", "boundary_tie"):
        assert got["idx"][k].tolist() == pi.expected_cem_indices(shape, N), f"{what}: cem indices"


@pytest.mark.parametrize("N", su.PI_N)
@pytest.mark.parametrize("name,H", su.WIDTHS)
@pytest.mark.parametrize("method", [1, 2, 3])
def test_pi_sweep_update(gpu, orc, levers, method, name, H, N):
    """The update kernels of mppi, cma-es and cem sweeps — score_wmean_batch_kernel with std_guard = 0 on materialised candidates,
    and the blockIdx.y forms of score_kernel, cem_select_kernel, cem_mean_kernel, cma_spread_kernel, cma_sigma_kernel strided through
    PiBatch — with three plans at temperatures 0.1, 1.0, 0.01 and sigmas 0.7, 0.5, 1.3, around every boundary of those kernels, three
    widths, and every case of pi_inputs.cases(N) (plan k of a call has another shape than its neighbours): weights, the new mean,
    sigma and the mean reward against orc.pi_update bit for bit, and cem's indices against the list written out from the shape's
    construction.  At N = 12 288 mppi and cma-es run under MBD_WMEAN_V = 1, 2, 4 as well."""
    P = 3
    HNu = H * _env(name).action_size
    Y, mu = su.candidates(P, N, HNu)
    sweep = _pi_sweep(name, H, N, P, su.PI_TEMPS, method)
    vs = su.WMEAN_V if (N == 12288 and method != 3) else (-1,)
    cache, seen = {}, set()
    sig = np.array(su.PI_SIGMAS, np.float32)
    try:
        for shapes in su.pi_rounds(N):
            rews = np.stack([pi.rewards(s, N) for s in shapes])
            for k, s in enumerate(shapes):
                if (k, s) not in cache:
                    cache[(k, s)] = orc.pi_update(method, rews[k], Y[k], mu[k], float(sig[k]), _temp(su.PI_TEMPS, k))
                seen.add((s, su.PI_TEMPS[k]))
            for v in vs:
                levers(MBD_WMEAN_V=v)
                got = gpu.debug_sweep_update(sweep.h, 1, Y, mu, rews, sigma_in=sig if method == 2 else None, sigma=method == 2,
                                             idx=method == 3)
                for k, s in enumerate(shapes):
                    _same_pi(method, N, s, got, k, cache[(k, s)], f"method {method} {name} N={N} plan {k} {s} MBD_WMEAN_V={v}")
    finally:
        sweep.close()
    assert seen >= {(s, t) for s, t, _ in pi.cases(N)}


# ---- d: under a weighting record ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", su.WEIGHTED_N)
@pytest.mark.parametrize("ri", [0, 1])
@pytest.mark.parametrize("method", [0, 1])
def test_sweep_update_under_a_weighting_record(gpu, orc, levers, method, ri, N):
    """weigh_kernel over the P plans (blockIdx.y, every plan's temperature) and the GIVEN form of score_wmean_batch_kernel, which loads
    the weights it is given, for MBD and mppi sweeps of three plans, under rejection alone and under rejection with an ESS target
    of half the kept candidates; rewards of weighting_inputs with NaN, +inf and -inf planted at other places in every plan, and a
    call with a plan that keeps nothing and one that keeps one candidate; V = 1, 2, 4; H Nu = 7 and 340.  Weights, mean reward and
    the new mean against weighting_checker, and the step's temperature, ESS and kept count through mbd_sweep_peek_weighting (the
    entry restarts the log: the step is entry 0), bit for bit.  The mean reward of a plan that keeps nothing is NaN in the
    checker: isnan there."""
    rec, P = RECORDS[ri], 3
    sched = orc.schedule(BETA0, BETAT, ND)
    for name, H in (("cartpole", 7), ("humanoidrun", 20)):
        HNu = H * _env(name).action_size
        if method == 0:
            temps = su.MBD_TEMPS
            cand, ybar = su.normals(P, N, HNu), su.means(P, HNu)
            Y = su.values(cand, sched[2][I], ybar)
            sweep = _mbd_sweep(name, H, N, P, temps)
        else:
            temps = su.PI_TEMPS[:2] + (0.3,)
            Y, ybar = su.candidates(P, N, HNu)
            cand = Y
            sweep = _pi_sweep(name, H, N, P, temps, 1)
        sweep.set_weighting(**rec.kwargs())
        try:
            for rews in su.weighted_rounds(N, P):
                res = [wc.weigh(orc, rews[k], _temp(temps, k), rec) for k in range(P)]
                outs = [wc.update(orc, method, res[k]["weights"], Y[k], ybar[k], sched, I) for k in range(P)]
                for v in (1, 2, 4):
                    levers(MBD_WMEAN_V=v)
                    what = f"method {method} {name} N={N} {rec} MBD_WMEAN_V={v}"
                    got = gpu.debug_sweep_update(sweep.h, I if method == 0 else 1, cand, ybar, rews)
                    same_bits(got["weights"], np.stack([r["weights"] for r in res]), f"{what}: weights")
                    same_bits(got["ybar"], np.stack(outs), f"{what}: the new mean")
                    for k in range(P):
                        if res[k]["kept"] == 0:
                            assert np.isnan(res[k]["rew_mean"]) and np.isnan(got["rew_mean"][k]), what
                        else:
                            same_bits(got["rew_mean"][k], res[k]["rew_mean"], f"{what}: plan {k} mean reward")
                        log = sweep.peek_weighting(k)
                        assert len(log["temp"]) == 1 and int(log["kept"][0]) == res[k]["kept"], (what, k, log)
                        same_bits(log["temp"][0], res[k]["temp"], f"{what}: plan {k} temperature")
                        same_bits(log["ess"][0], res[k]["ess"], f"{what}: plan {k} ESS")
        finally:
            sweep.close()


# ---- e: the demo blend -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [3, 65, 1025])
def test_mbd_sweep_update_demo_blend(gpu, orc, levers, N):
    """A humanoidtrack sweep with enable_demo (H = 50): the blend with the demo's log-densities through ScoreBatch::lp, standardised
    twice, two plans at two temperatures; the rewards and lp = 3 N(0, 1) - 2 of test_score_update_ragged_sizes — normals, and
    normals with a tied third and an outlier; its constant case has zero spread at the second standardisation, which has no guard
    (NaN in the reference too), and is left out —, each plan with the other case in the second call.  Against
    orc.score_update(lp_demo=, rew_xref=env.rew_xref), bit for bit, under every lever value."""
    name, H, P, temps = "humanoidtrack", 50, 2, (0.2, 0.5)
    env = _env(name)
    HNu = H * env.action_size
    sched = orc.schedule(BETA0, BETAT, ND)
    z, ybar = su.normals(P, N, HNu), su.means(P, HNu)
    Y = su.values(z, sched[2][I], ybar)
    g = np.random.default_rng(N)
    cases = []
    for case in (0, 2):
        r = g.normal(size=N).astype(np.float32)
        if case == 2:
            r[N // 2] = 40.0
            r[: N // 3] = r[0]
        cases.append((r, (g.normal(size=N) * 3 - 2).astype(np.float32)))
    sweep = _mbd_sweep(name, H, N, P, temps, demo=True)
    try:
        for order in ((0, 1), (1, 0)):
            rews, lp = np.stack([cases[c][0] for c in order]), np.stack([cases[c][1] for c in order])
            refs = [_mbd_ref(orc, sched, rews[k], Y[k], ybar[k], _temp(temps, k), lp=lp[k], rew_xref=float(env.rew_xref)) for k in range(P)]
            for v in su.WMEAN_V:
                levers(MBD_WMEAN_V=v)
                _same_plans(gpu.debug_sweep_update(sweep.h, I, z, ybar, rews, lp=lp), refs, f"demo N={N} {order} MBD_WMEAN_V={v}")
    finally:
        sweep.close()


# ---- f: isolation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,sick", [(3, 1), (8, 3)])
@pytest.mark.parametrize("method", [0, 3])
def test_a_plan_of_nan_rewards_stays_alone(gpu, method, P, sick):
    """With one plan's rewards all NaN, every other plan's outputs are those of the same call with healthy rewards on that plan, bit
    for bit: MBD and cem sweeps of three plans and of eight (the remap)."""
    name, H, N = "hopper", 30, 300
    HNu = H * _env(name).action_size
    rews = np.stack([su.plan_rewards(k % 7, N) for k in range(P)])  # (the seven shapes with a spread: cem's weights are finite)
    if method == 0:
        cand, ybar = su.normals(P, N, HNu), su.means(P, HNu)
        sweep, i = _mbd_sweep(name, H, N, P, None), I
    else:
        cand, ybar = su.candidates(P, N, HNu)
        sweep, i = _pi_sweep(name, H, N, P, None, 3), 1
    try:
        well = gpu.debug_sweep_update(sweep.h, i, cand, ybar, rews, idx=method == 3)
        bad = rews.copy()
        bad[sick] = np.nan
        ill = gpu.debug_sweep_update(sweep.h, i, cand, ybar, bad, idx=method == 3)
    finally:
        sweep.close()
    others = [k for k in range(P) if k != sick]
    assert np.isfinite(well["ybar"]).all() and np.isfinite(well["weights"]).all() and np.isfinite(well["rew_mean"]).all()
    for key in well:
        same_bits(ill[key][others].astype(np.float32), well[key][others].astype(np.float32), f"method {method} P={P}: {key}")
    assert np.isnan(ill["rew_mean"][sick])


# ---- g: the entry itself -----------------------------------------------------------------------------------------------------
def test_entry_refusals(gpu, lib):
    """Every refusal of mbd_debug_sweep_update by code and by the field mbd_last_error names; MBD_ERR_STATE while a session is open."""
    lib.mbd_debug_sweep_update.argtypes = gpu.SWEEP_UPDATE_ARGTYPES
    lib.mbd_last_error.restype = C.c_char_p
    name, H, N, P = "hopper", 6, 16, 2
    HNu = H * _env(name).action_size
    cand, ybar, rews, sig = (np.zeros(n, np.float32) for n in (P * N * HNu, P * HNu, P * N, P))
    c, y, r, s = (a.ctypes.data for a in (cand, ybar, rews, sig))

    def refused(sweep, code, field, i=1, c=c, y=y, r=r, lp=None, sigma_in=None):
        h = None if sweep is None else sweep.h
        assert lib.mbd_debug_sweep_update(h, i, c, y, r, lp, sigma_in, None, None, None, None, None) == code, field
        assert field in lib.mbd_last_error(), (field, lib.mbd_last_error())

    INVALID = gpu.MBD_ERR_INVALID
    refused(None, INVALID, b"sweep is NULL")
    mbd = _mbd_sweep(name, H, N, P, None, Nd=5)
    try:
        refused(mbd, INVALID, b"cand is NULL", c=None)
        refused(mbd, INVALID, b"ybar is NULL", y=None)
        refused(mbd, INVALID, b"rews is NULL", r=None)
        refused(mbd, INVALID, b"lp given", lp=r)
        refused(mbd, INVALID, b"sigma_in given", sigma_in=s)
        for i in (0, -1, 5, 30):
            refused(mbd, INVALID, b"i=%d outside [1,4]" % i, i=i)
        assert lib.mbd_debug_sweep_update(mbd.h, 4, c, y, r, None, None, None, None, None, None, None) == 0  # (every output may be NULL)
        with mbd.mpc_open(np.array([[1, 2], [3, 4]], np.uint32), 1):
            refused(mbd, gpu.MBD_ERR_STATE, b"a session is open")
    finally:
        mbd.close()
    for method in (1, 3):
        sw = _pi_sweep(name, H, N, P, None, method)
        refused(sw, INVALID, b"sigma_in given", sigma_in=s)
        sw.close()
    cma = _pi_sweep(name, H, N, P, None, 2)
    refused(cma, INVALID, b"sigma_in is NULL")
    refused(cma, INVALID, b"lp given", lp=r, sigma_in=s)
    cma.close()
    demo = _mbd_sweep("humanoidtrack", 50, 4, 1, None, demo=True, Nd=5)
    refused(demo, INVALID, b"lp is NULL")
    demo.close()


@pytest.mark.parametrize("method", [0, 2, 3])
def test_run_after_entry_calls_is_a_fresh_sweeps_run(gpu, method):
    """Sweep.run behind a series of entry calls — which write ring buffer 0 or the candidates, the rewards, the weights, sigma, slot 0
    and the buffer the final evaluation stages its means in — equals the run of a sweep that never saw the entry, bit for bit (MBD,
    cma-es, cem), and again after another entry call."""
    name, H, N, P, Nd = "hopper", 10, 64, 3, 6
    env = _env(name)
    HNu = H * env.action_size
    keys = np.stack([gpu.prng_key(40 + k) for k in range(P)])

    def make():
        sw = _mbd_sweep(name, H, N, P, su.MBD_TEMPS, Nd=Nd) if method == 0 else _pi_sweep(name, H, N, P, su.PI_TEMPS, method, Nd=Nd)
        for k in range(P):
            sw.set_state0(k, env.reset(gpu.prng_key(7 + k)))
        return sw

    def poke(sw, seed):
        cand, ybar = (su.normals(P, N, HNu, seed), su.means(P, HNu, seed)) if method == 0 else su.candidates(P, N, HNu, seed)
        rews = np.stack([su.plan_rewards(k + seed, N) for k in range(P)])
        gpu.debug_sweep_update(sw.h, 1 + seed % (Nd - 1), cand, ybar, rews, sigma_in=np.full(P, 0.4, np.float32) if method == 2 else None)

    fresh = make()
    ref = fresh.run(keys)[:3]
    ref_sigma = fresh.get_sigmas() if method else None
    fresh.close()
    sw = make()
    try:
        for rnd in range(2):
            for seed in range(3 * rnd, 3 * rnd + 3):
                poke(sw, seed)
            got = sw.run(keys)[:3]
            for a, b, what in zip(got, ref, ("mu_0ts", "mean rewards", "final rewards")):
                assert np.isfinite(b).all()
                same_bits(a, b, f"method {method} run {rnd}: {what}")
            if method:
                same_bits(sw.get_sigmas(), ref_sigma, f"method {method} run {rnd}: sigma")
    finally:
        sw.close()
