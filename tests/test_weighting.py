"""The weighting record without a GPU (include/mbd_hip.h mbd_weighting, DESIGN.md section 1 "N14 weighting"): the new checker
(tests/weighting_checker.py) held to the existing C checker where the two must coincide, the library's host restatement of
weigh_kernel (mbd_debug_weighting_host: the kernel's own per-entry functions and selection, its reductions as loops) held to the
checker bit for bit over the whole table of tests/weighting_inputs.py, the contract's properties on every case, and the C ABI."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import pi_inputs as pi
import weighting_checker as wc
import weighting_inputs as wi
from conftest import ROOT
from state_inputs import same_bits

TABLE = wi.table()


@functools.lru_cache(maxsize=None)
def _checked(orc, k):
    c = TABLE[k]
    return wc.weigh(orc, c.rews, c.temp, c.rec)


def test_table_reaches_every_branch_and_regime(orc):
    """Both clamps, the loop, the fixed temperature and the nothing-kept exit are each taken by some case, in the register regime
    and beyond it; entries are dropped in both; a case lies beyond the default LDS window."""
    wi.reach(TABLE, lambda c: _checked(orc, TABLE.index(c))["branch"])
    assert {c.N for c in TABLE} == set(wi.SIZES)


@pytest.mark.parametrize("N", wi.SIZES)
def test_checker_equals_the_c_checker_where_nothing_changes(orc, N):
    """Nothing dropped, ess_frac = 0, sd >= 1e-4: weights and mean reward of the new checker are orc.score_update's (the MBD
    score) and orc.pi_update's (the path-integral score, which has no guard) bit for bit, at every shape and temperature of
    pi_inputs."""
    Y0s, mu = pi.candidates(N, H=2, Nu=1)
    n = 0
    for shape, temp, rews in pi.cases(N):
        r64 = rews.astype(np.float64)
        if not pi.float64_meaningful(shape, N) or r64.std() < 2e-4:
            continue
        for rec in (wc.Record(reject_nonfinite=True), wc.Record(reject_nonfinite=False)):
            res = wc.weigh(orc, rews, temp, rec)
            assert res["kept"] == N and res["branch"] == "fixed" and res["temp"] == np.float32(temp)
            _, w0, m0 = orc.score_update(rews, Y0s, mu, 0.99, 0.5, 0.6, temp)
            _, _, w1, m1 = orc.pi_update(1, rews, Y0s, mu, 1.0, temp)
            same_bits(res["weights"], w0, f"{shape} N={N} temp={temp}: weights against score_update")
            same_bits(res["weights"], w1, f"{shape} N={N} temp={temp}: weights against pi_update")
            same_bits(res["rew_mean"], np.float32(m0), f"{shape} N={N}: mean reward")
            same_bits(res["rew_mean"], np.float32(m1), f"{shape} N={N}: mean reward (pi)")
        n += 1
    assert n >= (5 if N > 1 else 0)


@pytest.mark.parametrize("N", [5, 64, 1025])
def test_checker_update_equals_the_c_checker(orc, N):
    """``update`` — the weighted mean in wsum64's order, the literal score form, cem's selection — from the C checker's own weights
    gives the C checker's new mean: the restated downstream is the existing one."""
    Y0s, mu = pi.candidates(N, H=3, Nu=2)
    sched = orc.schedule(1e-4, 1e-2, 6)
    for shape in ("normal", "quantised"):
        rews = pi.rewards(shape, N)
        out, w, _ = orc.score_update(rews, Y0s, mu, float(sched[0][3]), float(sched[1][3]), float(sched[1][2]), 0.5)
        same_bits(wc.update(orc, 0, w, Y0s, mu, sched, 3), out, f"{shape} N={N}: MBD")
        for method in (1, 3):
            out, _, w, _ = orc.pi_update(method, rews, Y0s, mu, 1.0, 0.5)
            same_bits(wc.update(orc, method, w, Y0s, mu), out, f"{shape} N={N}: method {method}")


@pytest.mark.parametrize("N", wi.SIZES)
def test_host_restatement_equals_checker(lib, orc, N):
    """mbd_debug_weighting_host against the checker over the whole table: weights, mean reward, T*, ess and kept, bit for bit."""
    from mbd_hip import _capi
    for k, c in enumerate(TABLE):
        if c.N != N:
            continue
        ref = _checked(orc, k)
        w, mean, T, ess, kept = _capi.debug_weighting_host(c.rews, c.temp, _capi.weighting_record(**c.rec.kwargs()))
        same_bits(w, ref["weights"], f"{c.id}: weights")
        if ref["kept"] == 0:
            assert np.isnan(mean) and np.isnan(ref["rew_mean"]), c.id
        else:
            same_bits(mean, ref["rew_mean"], f"{c.id}: mean reward")
        same_bits(T, ref["temp"], f"{c.id}: temperature")
        same_bits(ess, ref["ess"], f"{c.id}: ess")
        assert kept == ref["kept"], c.id


@pytest.mark.parametrize("N", wi.SIZES)
def test_properties(orc, N):
    """On every case: dropped weights are +0 with the sign bit clear; 1 <= ess <= kept; temp_min <= T* <= temp_max; when the loop
    ran, ess(T*) >= target; rejection on and off give the same bits where nothing is non-finite."""
    for k, c in enumerate(TABLE):
        if c.N != N:
            continue
        res = _checked(orc, k)
        w = res["weights"]
        drop = ~np.isfinite(c.rews) if c.rec.reject_nonfinite else np.zeros(c.N, bool)
        assert res["kept"] == c.N - drop.sum(), c.id
        assert (w[drop].view(np.uint32) == 0).all(), f"{c.id}: a dropped weight is not +0"
        if res["kept"] == 0:
            assert (w.view(np.uint32) == 0).all() and res["ess"] == 0 and res["temp"] == np.float32(c.temp), c.id
            continue
        assert np.isfinite(w).all() and (w >= 0).all(), c.id
        assert np.float32(1) <= res["ess"] <= np.float32(res["kept"]), f"{c.id}: ess {res['ess']!r} outside [1, {res['kept']}]"
        if c.rec.ess_frac > 0:
            assert np.float32(c.rec.temp_min) <= res["temp"] <= np.float32(c.rec.temp_max), c.id
        if res["branch"] == "loop":
            assert res["ess"] >= res["target"], f"{c.id}: ess(T*) {res['ess']!r} below the target {res['target']!r}"
        if not drop.any():
            off = wc.weigh(orc, c.rews, c.temp, wc.Record(**dict(c.rec.kwargs(), reject_nonfinite=False)))
            same_bits(off["weights"], w, f"{c.id}: rejection off")
            same_bits(off["rew_mean"], res["rew_mean"], f"{c.id}: rejection off, mean reward")
            same_bits(off["temp"], res["temp"], f"{c.id}: rejection off, temperature")
            same_bits(off["ess"], res["ess"], f"{c.id}: rejection off, ess")


def _header_struct_bytes(name):
    text = open(os.path.join(ROOT, "include", "mbd_hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size = 0
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ctype, names = decl.split(None, 1)
        assert ctype in ("int32_t", "float"), decl
        for nm in names.split(","):
            m = re.search(r"\[(\d+)\]", nm)
            size += 4 * (int(m.group(1)) if m else 1)
    return size


def test_abi(lib):
    """The four entries and the debug one are exported; sizeof(mbd_weighting) agrees between the ctypes mirror and the header; NULL
    handles and bad records are refused without a device, the message naming the field."""
    from mbd_hip import _capi
    for n in ("mbd_plan_set_weighting", "mbd_plan_peek_weighting", "mbd_sweep_set_weighting", "mbd_sweep_peek_weighting",
              "mbd_debug_weighting_host"):
        assert hasattr(lib, n), n
    assert C.sizeof(_capi.Weighting) == _header_struct_bytes("mbd_weighting") == 44
    rec = _capi.weighting_record()
    n = C.c_int(0)
    assert lib.mbd_plan_set_weighting(None, C.byref(rec)) == _capi.MBD_ERR_INVALID
    assert lib.mbd_sweep_set_weighting(None, C.byref(rec)) == _capi.MBD_ERR_INVALID
    assert lib.mbd_plan_peek_weighting(None, None, None, None, 0, C.byref(n)) == _capi.MBD_ERR_INVALID
    assert lib.mbd_sweep_peek_weighting(None, 0, None, None, None, 0, C.byref(n)) == _capi.MBD_ERR_INVALID
    r = np.zeros(4, np.float32)
    bad = [(dict(reject_nonfinite=2), b"reject_nonfinite"), (dict(ess_frac=1.5), b"ess_frac"), (dict(ess_frac=float("nan")), b"ess_frac"),
           (dict(ess_frac=-0.1), b"ess_frac"), (dict(ess_frac=0.5, temp_min=0.0, temp_max=1.0), b"temp_min"),
           (dict(ess_frac=0.5, temp_min=2.0, temp_max=1.0), b"temp_max"), (dict(ess_frac=0.5, temp_min=1.0, temp_max=float("inf")), b"temp_max"),
           (dict(ess_frac=0.5, temp_min=0.1, temp_max=1.0, iters=0), b"iters"), (dict(ess_frac=0.5, temp_min=0.1, temp_max=1.0, iters=33), b"iters")]
    for kw, field in bad:
        with pytest.raises(_capi.MbdError):
            _capi.debug_weighting_host(r, 0.1, _capi.weighting_record(**kw))
        assert field in lib.mbd_last_error(), (kw, lib.mbd_last_error())
    rec = _capi.weighting_record()
    rec.reserved[3] = 1
    with pytest.raises(_capi.MbdError):
        _capi.debug_weighting_host(r, 0.1, rec)
    assert b"reserved[3]" in lib.mbd_last_error()


def test_cli_flags_map_to_the_record():
    """mpc.MpcArgs' weighting flags: none set means no record; each flag reaches the field of ``Plan.set_weighting`` it names, and
    the bracket only travels with a target."""
    from mbd_hip.planners import mpc
    assert not mpc._has_weighting(mpc.MpcArgs()) and mpc._weighting_settings(mpc.MpcArgs()) == {}
    a = mpc.MpcArgs(reject_nonfinite=True)
    assert mpc._has_weighting(a)
    assert mpc._weighting_of(a) == dict(reject_nonfinite=True, ess_frac=0.0, temp_min=None, temp_max=None, iters=12)
    a = mpc.MpcArgs(ess_frac=0.3, temp_min=0.02, temp_max=5.0, ess_iters=7)
    assert mpc._has_weighting(a)
    assert mpc._weighting_of(a) == dict(reject_nonfinite=False, ess_frac=0.3, temp_min=0.02, temp_max=5.0, iters=7)
    from mbd_hip import _capi
    rec = _capi.weighting_record(**mpc._weighting_of(a))
    assert (rec.reject_nonfinite, rec.iters) == (0, 7)
    assert (np.float32(rec.ess_frac), np.float32(rec.temp_min), np.float32(rec.temp_max)) == (np.float32(0.3), np.float32(0.02), np.float32(5.0))
    assert mpc._weighting_settings(a) == dict(reject_nonfinite=False, ess_frac=0.3, temp_min=0.02, temp_max=5.0, ess_iters=7)


# ---- the record together with the other records (tests/weighting_combined_inputs.py; tests/test_gpu_weighting_combined.py) ---------
@pytest.mark.parametrize("N", [5, 64, 1025])
@pytest.mark.parametrize("H,Nu", [(3, 2), (30, 3)], ids=["HNu6", "HNu90"])
def test_pi_update_sigma_equals_the_c_checker(orc, N, H, Nu):
    """``wc.pi_update`` — cma-es' sigma restated from given weights: the sequential fma per output, the 64 strided partials, the
    wavefront's butterfly, the floor — against orc.pi_update where the two must coincide: nothing dropped, ess_frac = 0, spread >=
    1e-4 (the path-integral score has no guard).  HNu = 6 leaves 58 partials at +0, HNu = 90 gives 26 of them two terms."""
    Y0s, mu = pi.candidates(N, H=H, Nu=Nu)
    n = 0
    for shape in ("normal", "quantised", "two_values"):
        if shape not in pi.shapes(N):
            continue
        rews = pi.rewards(shape, N)
        if rews.astype(np.float64).std() < 2e-4:
            continue
        for sigma0 in (0.7, 1e-3):
            res = wc.weigh(orc, rews, 0.5, wc.Record(reject_nonfinite=True))
            assert res["kept"] == N and res["branch"] == "fixed"
            for method in (1, 2, 3):
                mu_r, sig_r, w_r, _ = orc.pi_update(method, rews, Y0s, mu, sigma0, 0.5)
                out, sig = wc.pi_update(orc, method, res, Y0s, mu, sigma0)
                same_bits(res["weights"], w_r, f"{shape} N={N}: weights")
                same_bits(out, mu_r, f"{shape} N={N} method {method}: mean")
                same_bits(sig, np.float32(sig_r), f"{shape} N={N} method {method}: sigma from {sigma0}")
                if method != 2:
                    assert sig == np.float32(sigma0)
                elif sigma0 == 1e-3:  # (the spread of candidates within [-1, 1] is below 1: the floor holds the carry)
                    assert sig == np.float32(1e-3)
        n += 1
    assert n >= 2


def test_pi_update_sigma_floor_and_nan(orc):
    """Every weight +0 (all dropped): the spread is +0 and sigma is the 1e-3 floor; a NaN weight keeps sigma NaN."""
    Y0s, mu = pi.candidates(64, H=3, Nu=2)
    res = wc.weigh(orc, np.full(64, np.nan, np.float32), 0.1, wc.Record(reject_nonfinite=True))
    assert wc.pi_update(orc, 2, res, Y0s, mu, 0.7)[1].view(np.uint32) == np.float32(1e-3).view(np.uint32)
    res = wc.weigh(orc, np.full(64, np.nan, np.float32), 0.1, wc.Record(reject_nonfinite=False))
    assert np.isnan(wc.pi_update(orc, 2, res, Y0s, mu, 0.7)[1])


@pytest.mark.parametrize("method", ["mppi", "cma-es", "cem"])
def test_plan_tick_under_a_record_that_changes_nothing(method):
    """``wc.plan_tick`` under rejection alone on healthy rollouts is mpc_pi_checker.plan_tick, and an episode over it the plain
    episode, sigmas included; the defaults of ``plan_tick=`` / ``update=`` leave mpc_pi_checker's own results alone (the other
    CPU tests of tests/test_mpc_pi.py run on them)."""
    import mpc_pi_cases as cases
    import mpc_pi_checker as pic
    oe, o = cases.oenv("hopper"), cases._orc()
    s0, key = cases.start("hopper")
    N, H = 33, 4
    mu = (np.random.default_rng(2).normal(size=(H, oe.Nu)) * 0.3).astype(np.float32)
    a = pic.plan_tick(oe, s0, key, mu, np.float32(0.7), 2, N, H, 0.1, method)
    log = []
    b = wc.plan_tick(oe, s0, key, mu, np.float32(0.7), 2, N, H, 0.1, method, rec=wi.REJECT, log=log)
    for x, y, what in zip(a, b, ("key", "mean", "sigma")):
        same_bits(np.asarray(x), np.asarray(y), f"{method}: {what}")
    assert [e[2] for e in log] == [N, N] and all(e[0] == np.float32(0.1) for e in log)
    rec = (1.0, 0.5, 0.9 if method == "cma-es" else 0.0)
    plain = pic.episode(oe, s0, key, N, H, 4, 0.1, 2, 2, 1, method, *rec)
    under = pic.episode(oe, s0, key, N, H, 4, 0.1, 2, 2, 1, method, *rec, plan_tick=functools.partial(wc.plan_tick, rec=wi.REJECT))
    for k in plain:
        same_bits(under[k], plain[k], f"{method} episode: {k}")
    sess = pic.Session(oe, key, N, H, 4, 0.1, 2, 1, method, *rec, plan_tick=functools.partial(wc.plan_tick, rec=wi.REJECT))
    for t in range(2):
        same_bits(sess.tick(plain["states"][t])["mean"], plain["means"][t], f"{method} session, tick {t}")


# wc.episode of the commit before ``reverse_once`` took oracle.planner's signature — its own loop over mpc_checker.execute and
# shift —, recorded from that code: hopper from mpc_pi_cases.start, N = 33, H = 4, Ndiffuse = 4, T = 3, K = 2, E = 1 under wi.ESS.
# sha256 of the float32 arrays' bytes, and the log as (temp bits, ess bits, kept) per step per tick.
_EPISODE_BEFORE = dict(
    actions="d83204212266dd4243aaf7e33b61051384de2997056fa8da2fabb97453f4374c",
    rewards="2c5ade4529a7e148f215ec96797ffa0692fce34692c388cc920d25052779c1de",
    states="5af2c46d3c94e4d73c66bfd3fec9b8553074e7c4c58033c85545d235feca2c84",
    means="df8586a100b7b958d5bc89f43fc5a6d5f53ee40804640c6f26a253b3d3e5a52c",
    log=[[(1052168149, 1090781429, 33), (1054513261, 1090795796, 33), (1061922109, 1090781706, 33)],
         [(1051849190, 1090784108, 33), (1057540026, 1090794013, 33)], [(1056390106, 1090783122, 33), (1061436012, 1090795477, 33)]])


def test_episode_keeps_the_bits_it_had_before_it_became_a_composition():
    """``wc.episode`` is now objective_checker.episode over ``wc.reverse_once``; its results are the recorded ones, bit for bit; so
    is mpc_online_checker's session handed ``wc.reverse_once`` directly."""
    import hashlib

    import mpc_online_checker as online
    import mpc_pi_cases as cases
    oe = cases.oenv("hopper")
    s0, key = cases.start("hopper")
    ep = wc.episode(oe, s0, key, 33, 4, 4, 0.1, 3, 2, 1, wi.ESS)
    for k in ("actions", "rewards", "states", "means"):
        assert hashlib.sha256(np.ascontiguousarray(ep[k], np.float32).tobytes()).hexdigest() == _EPISODE_BEFORE[k], k
    bits = [[(int(np.float32(t).view(np.uint32)), int(np.float32(e).view(np.uint32)), int(k)) for t, e, k in tick] for tick in ep["log"]]
    assert bits == _EPISODE_BEFORE["log"]
    got = online.session(oe, key, ep["states"][:3], 33, 4, 4, 0.1, 2, 1, reverse_once=functools.partial(wc.reverse_once, rec=wi.ESS))
    same_bits(got["means"], ep["means"], "a session over wc.reverse_once")


def test_combined_cases_reach_what_they_are_there_for(orc):
    """Of the very cases tests/test_gpu_weighting_combined.py runs, in the checker: the real-divergence launches drop between 1 and
    N - 1 candidates (one step under every method's sigma; every tick of the closed loop, whose means and states stay finite); behind
    an objective and behind an ensemble the selection takes the loop and a clamp; an ensemble with a diverged member drops some
    candidates and keeps some; the objective moves the temperatures; the cem case has three positive weights among twelve kept."""
    import weighting_combined_inputs as wci
    for method in (0, 1):  # (one sigma for MBD, one for the path-integral plans)
        d = wci.divergence_step(orc, method)
        kept = int(np.isfinite(d["rews"]).sum())
        assert 0 < kept < wci.STEP["N"], (method, kept)
        assert (d["Y0s"][:, :, 0] != 0).all()  # (no candidate is spared by a zero: the shape is not zero there)
    ep = wci.divergence_episode(orc, wi.REJECT)
    assert np.isfinite(ep["means"]).all() and np.isfinite(ep["states"]).all()
    assert all(0 < e[2] < wci.LOOP["N"] for tick in ep["log"] for e in tick), ep["log"]
    with_o, without = wci.objective_episode(orc, wi.ESS), wci.objective_episode(orc, wi.ESS, with_objective=False)
    assert all(a[0] != b[0] for ta, tb in zip(with_o["log"], without["log"]) for a, b in zip(ta, tb))
    seen = {wci.branch_of(e, wi.ESS) for tick in with_o["log"] for e in tick} | {wci.branch_of(e, wci.FULL) for e in wci.objective_run(orc, wci.FULL)["log"]}
    assert {"loop", "max"} <= seen, seen
    seen, drops = set(), []
    for N, bad, risk, with_obj in wci.ENSEMBLES:
        st = wci.ensemble_step(orc, N, bad, risk, wi.ESS, with_obj)
        kept = st["log"][0][2]
        assert kept == int(np.isfinite(st["det"]["rews"]).sum())
        drops.append(N - kept)
        seen.add(wci.branch_of(st["log"][0], wi.ESS))
        assert 0 < kept < N, (N, bad, risk, kept)
    for N, bad, risk, with_obj in (wci.ENSEMBLES[0], wci.ENSEMBLES[-1]):  # (the later steps of an episode keep more: the loop)
        ep = wci.ensemble_episode(orc, N, bad, risk, wi.ESS, with_obj)
        assert np.isfinite(ep["means"]).all() and all(0 < e[2] < N for tick in ep["log"] for e in tick)
        seen |= {wci.branch_of(e, wi.ESS) for tick in ep["log"] for e in tick}
    seen |= {wci.branch_of(e, wci.FULL) for e in wci.ensemble_step(orc, 33, 2, "min", wci.FULL)["log"]}
    assert {"loop", "min", "max"} <= seen, seen
    r, rec = wci.cem_ties()["few_positive"]
    res = wc.weigh(orc, r, 0.1, rec)
    assert res["kept"] == 12 and int((res["weights"] > 0).sum()) == 3 and res["branch"] == "min"
    assert (res["weights"][[0, 1, 2, 4, 5, 6, 7, 8, 9]].view(np.uint32) == 0).all()  # kept, and +0 like the dropped ones
