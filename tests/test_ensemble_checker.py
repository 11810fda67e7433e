"""The checker of planning over an ensemble of perturbed models (tests/ensemble_checker.py; include/mbd_hip.h mbd_ensemble,
DESIGN.md section 1 "N6 ensemble") held to its own identities, without a GPU: one member is the oracle planner's step and
whole plan, MIN does not depend on the members' order, MEAN of M identical members is the single member wherever
(r + ... + r) / M is exact (M a power of two; M = 3: within one ulp), an episode over identical members is
tests/mpc_checker.py's, and members that differ give other rewards.  Also what the front ends decide from their arguments
alone: the exports, the record's layout, the member lists of mbd_hip.planners.mpc, and the refusal of ensembles in batches."""
import ctypes as C
import os
import shutil
import subprocess
from dataclasses import replace

import numpy as np
import pytest

import ensemble_checker as ec
import mpc_checker
import mpc_plant_checker
from conftest import ROOT, load_model
from oracle import planner as op

SCALES = [dict(mass=0.8, friction=1.3, gear=1.1), dict(), dict(mass=1.25, friction=0.7, gear=0.9), dict(mass=1.5, gear=1.2)]


def _oenv(orc, name, **scale):
    from oracle.planner import OracleEnv
    m = load_model(name).scaled(**scale)
    return OracleEnv(orc, name, m.to_struct(), init_q=m.init_q)


def _reset(orc, oe, seed):
    return np.asarray(oe.reset(orc.split(orc.prng_key(seed), 2, 1)[1], 1), np.float32)


def _setup(orc, name="hopper", N=32, H=8, Nd=5):
    oe = _oenv(orc, name)
    return oe, _reset(orc, oe, 3), orc.schedule(1e-4, 1e-2, Nd), orc.prng_key(9)


@pytest.mark.parametrize("risk", ["mean", "min"])
@pytest.mark.parametrize("name", ["hopper", "humanoidrun"])
def test_one_member_is_the_oracle_planners_step_and_plan(orc, name, risk):
    N, H, Nd = 32, 8, 5
    oe, s0, sched, key = _setup(orc, name, N, H, Nd)
    Ybar = (0.1 * orc.normal(orc.prng_key(1), (H, oe.Nu), 1)).astype(np.float32)
    want = op.reverse_once(orc, oe, s0, 3, key, Ybar, sched, N, H, 0.1, 1)
    for members in ([None], [oe], [_oenv(orc, name)]):
        got = ec.step(orc, oe, members, risk, s0, 3, key, Ybar, sched, N, H, 0.1)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
        assert np.array_equal(got[3]["Y0s"], want[3]["Y0s"]) and np.array_equal(got[3]["rews"], want[3]["rews"])
        assert np.array_equal(got[3]["weights"], want[3]["weights"]) and np.array_equal(got[3]["r_members"][0], want[3]["rews"])
        # the adaptor the existing checkers are run through gives the same step
        via = op.reverse_once(orc, ec.EnsembleEnv(oe, members, risk), s0, 3, key, Ybar, sched, N, H, 0.1, 1)
        assert np.array_equal(via[1], want[1]) and via[2] == want[2] and np.array_equal(via[3]["weights"], want[3]["weights"])
    # the whole plan: the loop of oracle.planner.run_diffusion from the same state and key
    r, Yb, mus, rms = key, np.zeros((H, oe.Nu), np.float32), [], []
    for i in range(Nd - 1, 0, -1):
        r, Yb, rm, _ = op.reverse_once(orc, oe, s0, i, r, Yb, sched, N, H, 0.1, 1)
        mus.append(Yb)
        rms.append(rm)
    got = ec.plan(orc, oe, [None], risk, s0, key, N, H, Nd, 0.1)
    assert np.array_equal(got["mu_0ts"], np.stack(mus)) and np.array_equal(got["rew_means"], np.array(rms, np.float32))
    assert got["rew_final"] == op.mean_h(orc, np.ascontiguousarray(oe.rollout(s0, Yb[None])))[0]


def test_step_and_adaptor_agree_on_distinct_members(orc):
    """The pseudo-code spelled out (step) and the adaptor the existing checkers run through give the same step, under both
    risk modes; r_m is member m's own rollout of the step's candidates; the members do differ."""
    N, H, Nd = 32, 8, 5
    oe, s0, sched, key = _setup(orc, "hopper", N, H, Nd)
    members = [_oenv(orc, "hopper", **s) for s in SCALES]
    Ybar = (0.2 * orc.normal(orc.prng_key(2), (H, oe.Nu), 1)).astype(np.float32)
    outs = {}
    for risk in ("mean", "min"):
        rng, Y, rm, d = ec.step(orc, oe, members, risk, s0, 2, key, Ybar, sched, N, H, 0.1)
        via = op.reverse_once(orc, ec.EnsembleEnv(oe, members, risk), s0, 2, key, Ybar, sched, N, H, 0.1, 1)
        assert np.array_equal(via[1], Y) and via[2] == rm and np.array_equal(via[3]["weights"], d["weights"])
        for m, me in enumerate(members):
            assert np.array_equal(d["r_members"][m], op.mean_h(orc, np.ascontiguousarray(me.rollout(s0, d["Y0s"]))))
        assert np.array_equal(d["r_members"][1], op.reverse_once(orc, oe, s0, 2, key, Ybar, sched, N, H, 0.1, 1)[3]["rews"])
        assert not np.array_equal(d["r_members"][0], d["r_members"][2])
        r = d["r_members"]
        if risk == "min":
            assert np.array_equal(d["rews"], r.min(axis=0))
        else:
            assert np.array_equal(d["rews"], (((r[0] + r[1]) + r[2]) + r[3]) / np.float32(4))
        outs[risk] = Y
    assert not np.array_equal(outs["mean"], outs["min"])


def test_min_is_permutation_invariant(orc):
    N, H, Nd = 32, 8, 5
    oe, s0, sched, key = _setup(orc, "hopper", N, H, Nd)
    members = [_oenv(orc, "hopper", **s) for s in SCALES]
    Ybar = np.zeros((H, oe.Nu), np.float32)
    want = ec.step(orc, oe, members, "min", s0, 4, key, Ybar, sched, N, H, 0.1)
    for perm in ((3, 2, 1, 0), (1, 3, 0, 2), (2, 0, 3, 1)):
        got = ec.step(orc, oe, [members[k] for k in perm], "min", s0, 4, key, Ybar, sched, N, H, 0.1)
        assert np.array_equal(got[1], want[1]) and got[2] == want[2]
        assert np.array_equal(got[3]["rews"], want[3]["rews"]) and np.array_equal(got[3]["weights"], want[3]["weights"])
    want = ec.plan(orc, oe, members, "min", s0, key, N, H, Nd, 0.1)
    got = ec.plan(orc, oe, members[::-1], "min", s0, key, N, H, Nd, 0.1)
    assert np.array_equal(got["mu_0ts"], want["mu_0ts"]) and np.array_equal(got["rew_means"], want["rew_means"])


@pytest.mark.parametrize("M", [1, 2, 3, 4, 8])
def test_mean_of_identical_members(orc, M):
    """(r + ... + r) / M equals r wherever the left-to-right float32 sum is exact, i.e. wherever every partial sum k r is a
    float32 (decided here in float64, which holds k r exactly for k <= 8).  M = 1, 2: always (2 r is r's next binade).  M = 4:
    always as well — 3 r may round, by at most half an ulp of its binade, and adding r then lands within half an ulp of 4 r
    with ties going to 4 r's even mantissa — so the whole step is the single member's, bit for bit.  M = 8: 5 r, 6 r and 7 r
    round too and do NOT always recover (four candidates in ten do not), so equality is asserted for the candidates whose
    partial sums are all exact and, for the others, the bound those three roundings give: each at most half an ulp of a
    binade no higher than 8 r's, i.e. 1.5 ulp of the result in all — asserted as <= 2 ulp.  M = 3: <= 1 ulp (one rounding
    of 3 r, one of the division)."""
    N, H, Nd = 32, 8, 5
    oe, s0, sched, key = _setup(orc, "hopper", N, H, Nd)
    Ybar = np.zeros((H, oe.Nu), np.float32)
    single = op.reverse_once(orc, oe, s0, 4, key, Ybar, sched, N, H, 0.1, 1)
    got = ec.step(orc, oe, [None] * M, "mean", s0, 4, key, Ybar, sched, N, H, 0.1)
    r = single[3]["rews"]
    r64 = r.astype(np.float64)
    exact = np.ones(N, bool)
    for k in range(2, M + 1):
        exact &= (k * r64).astype(np.float32).astype(np.float64) == k * r64
    ulps = np.abs(got[3]["rews"].astype(np.float64) - r64) / np.spacing(np.abs(r)).astype(np.float64)
    assert np.array_equal(got[3]["rews"][exact], r[exact])
    if M in (1, 2, 4):
        assert np.array_equal(got[3]["rews"], r)
        assert np.array_equal(got[1], single[1]) and got[2] == single[2] and np.array_equal(got[3]["weights"], single[3]["weights"])
    else:
        assert ulps.max() <= (1 if M == 3 else 2)
    if M == 8:  # (on exactly representable rewards — multiples of 2^-10 below 2^10 — every partial sum is exact)
        q = (np.round(r64 * 1024) / 1024).astype(np.float32)
        assert np.array_equal(ec.combine(np.stack([q] * 8), "mean"), q)
    assert np.array_equal(ec.step(orc, oe, [None] * M, "min", s0, 4, key, Ybar, sched, N, H, 0.1)[3]["rews"], r)


def test_combine_is_left_to_right_float32():
    r = np.array([[1e8], [1.0], [-1e8], [1.0]], np.float32)
    assert ec.combine(r, "mean")[0] == np.float32(0.25)  # ((1e8 + 1) - 1e8) + 1 = 1 in float32, / 4
    assert ec.combine(r[[1, 3, 0, 2]], "mean")[0] == np.float32(0.0)
    assert ec.combine(r, "min")[0] == np.float32(-1e8)
    nan = np.float32("nan")  # a diverged member wins under MIN wherever it stands, as it spreads under MEAN
    for rows in ([[nan], [1.0], [2.0]], [[1.0], [nan], [2.0]], [[2.0], [1.0], [nan]]):
        assert np.isnan(ec.combine(np.array(rows, np.float32), "min")[0]) and np.isnan(ec.combine(np.array(rows, np.float32), "mean")[0])
    assert ec.combine(np.array([[0.1], [0.2], [0.4]], np.float32), "mean")[0] == \
        np.float32(np.float32(np.float32(np.float32(0.1) + np.float32(0.2)) + np.float32(0.4)) / np.float32(3))
    with pytest.raises(ValueError):
        ec.combine(r, "cvar")


@pytest.mark.parametrize("risk", ["mean", "min"])
def test_episode_over_identical_members_is_the_episode(orc, risk):
    oe = _oenv(orc, "hopper")
    N, H, Nd, K, E, T = 16, 10, 6, 2, 2, 4
    s0, key = _reset(orc, oe, 1), orc.prng_key(4)
    ref = mpc_checker.episode(oe, s0, key, N, H, Nd, 0.1, T, K, E)
    for members in ([None], [None, _oenv(orc, "hopper")], [oe] * 4):
        got = ec.episode(oe, members, risk, s0, key, N, H, Nd, 0.1, T, K, E)
        for k in ("actions", "rewards", "states", "means"):
            assert np.array_equal(got[k], ref[k]), k
    # ... and with a plant and disturbances it is tests/mpc_plant_checker.py's
    plant = _oenv(orc, "hopper", mass=1.3, friction=0.5, gear=0.8)
    kw = dict(dkey=orc.prng_key(6), act_std=0.3, kick_std=0.5, kick_every=2)
    ref = mpc_plant_checker.episode(oe, s0, key, N, H, Nd, 0.1, T, K, E, plant=plant, **kw)
    got = ec.episode(oe, [None, None], risk, s0, key, N, H, Nd, 0.1, T, K, E, plant=plant, **kw)
    for k in ("actions", "rewards", "states", "means"):
        assert np.array_equal(got[k], ref[k]), k


def test_episode_with_distinct_members(orc):
    """Tick 0's mean is the whole plan from k_0 with the same members; T ticks are a prefix of T + 2; the executed rows go
    through the plan's own env; the ensemble changes the episode."""
    oe = _oenv(orc, "hopper")
    members = [None, _oenv(orc, "hopper", mass=1.25, friction=0.7), _oenv(orc, "hopper", mass=0.8, gear=1.2)]
    N, H, Nd, K, E = 16, 10, 6, 2, 1
    s0, key = _reset(orc, oe, 1), orc.prng_key(4)
    long = ec.episode(oe, members, "min", s0, key, N, H, Nd, 0.1, 5, K, E)
    short = ec.episode(oe, members, "min", s0, key, N, H, Nd, 0.1, 3, K, E)
    for k, v in short.items():
        assert np.array_equal(v, long[k][: len(v)]), k
    k0 = orc.split(key, 2, 1)[1]
    assert np.array_equal(long["means"][0], ec.plan(orc, oe, members, "min", s0, k0, N, H, Nd, 0.1)["mu_0ts"][-1])
    for t in range(5):
        rew, s = mpc_checker.execute(oe, long["states"][t], long["means"][t][:E])
        assert np.array_equal(rew, long["rewards"][t * E:(t + 1) * E]) and np.array_equal(s, long["states"][t + 1])
    assert not np.array_equal(long["means"][0], mpc_checker.episode(oe, s0, key, N, H, Nd, 0.1, 1, K, E)["means"][0])


# ---- the boundary and the front ends, from their arguments alone ---------------------------------------------------------

def test_ensemble_entries_are_exported_and_refuse_null_handles_before_any_device_access(lib):
    """Without the feature the first lookup of mbd_plan_set_ensemble fails."""
    from mbd_hip import _capi
    for name in ("mbd_plan_set_ensemble", "mbd_plan_peek_ensemble"):
        assert name in _capi.EXPORTS and hasattr(lib, name), name
    rec = _capi.Ensemble(n_members=1)
    assert lib.mbd_plan_set_ensemble(None, C.byref(rec)) == _capi.MBD_ERR_INVALID
    assert b"plan" in lib.mbd_last_error()
    assert lib.mbd_plan_set_ensemble(None, None) == _capi.MBD_ERR_INVALID
    out = np.zeros(4, np.float32)
    assert lib.mbd_plan_peek_ensemble(None, _capi.np_ptr(out), _capi.np_ptr(out)) == _capi.MBD_ERR_INVALID
    assert b"plan" in lib.mbd_last_error()
    assert "MBD_ENS_SPLIT" in _capi.LEVERS and _capi.debug_get("MBD_ENS_SPLIT") == -1


def test_the_ctypes_record_has_the_headers_layout(tmp_path):
    from mbd_hip import _capi
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a C compiler is what builds the checker as well"
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mbd_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %d %d %d\\n", sizeof(mbd_ensemble), offsetof(mbd_ensemble, members), '
                   'offsetof(mbd_ensemble, n_members), offsetof(mbd_ensemble, risk), offsetof(mbd_ensemble, reserved), '
                   'MBD_MAX_ENSEMBLE, MBD_RISK_MEAN, MBD_RISK_MIN); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    E = _capi.Ensemble
    assert got == [C.sizeof(E), E.members.offset, E.n_members.offset, E.risk.offset, E.reserved.offset, _capi.MAX_ENSEMBLE,
                   _capi.RISK_MEAN, _capi.RISK_MIN]
    assert _capi.RISKS == {"mean": _capi.RISK_MEAN, "min": _capi.RISK_MIN}


def test_mpc_arguments_list_the_members():
    from mbd_hip.planners import mpc
    a = mpc.MpcArgs(env_name="hopper", Nsample=64, Hsample=20, Ndiffuse=6, n_ticks=3, warm_steps=2,
                    disable_recommended_params=True, not_render=True)
    assert not mpc._has_ensemble(a) and mpc.ensemble_triples(a) == [] and not mpc._has_plant(replace(a, ens_mass="1.2"))
    assert mpc.ensemble_triples(replace(a, ens_mass="0.8,1,1.25", ens_friction="0.7", ens_gear="1,1.1,0.9")) == \
        [(0.8, 0.7, 1.0), (1.0, 0.7, 1.1), (1.25, 0.7, 0.9)]
    assert mpc.ensemble_triples(replace(a, ens_risk="min")) == [(1.0, 1.0, 1.0)]
    assert mpc.ensemble_triples(replace(a, ens_gear="1.5")) == [(1.0, 1.0, 1.5)]
    assert mpc._ensemble_settings(replace(a, ens_mass="2", ens_risk="min")) == \
        dict(ensemble=[dict(mass=2.0, friction=1.0, gear=1.0)], ens_risk="min")
    with pytest.raises(ValueError, match="ens_friction"):
        mpc.ensemble_triples(replace(a, ens_mass="1,2,3", ens_friction="1,2"))
    with pytest.raises(ValueError, match="ens_risk"):
        mpc.ensemble_triples(replace(a, ens_mass="1,2", ens_risk="cvar"))
    with pytest.raises(ValueError, match="9 ensemble members"):
        mpc.ensemble_triples(replace(a, ens_mass=",".join(["1"] * 9)))
    # Args itself mirrors the reference's dataclass: the ensemble is a keyword of run_diffusion, not a field
    from mbd_hip.planners.mbd_planner import Args
    assert not any(f.startswith("ens") for f in Args.__dataclass_fields__)


def test_batches_refuse_ensemble_flags():
    from mbd_hip.planners import mpc
    a = mpc.MpcArgs(env_name="hopper", Nsample=64, Hsample=20, Ndiffuse=6, n_ticks=3, warm_steps=2,
                    disable_recommended_params=True, not_render=True)
    mpc._check_batch([a, replace(a, seed=1)])
    for bad in (replace(a, seed=1, ens_mass="0.8,1.2"), replace(a, seed=1, ens_risk="min")):
        with pytest.raises(ValueError, match="ensemble"):
            mpc._check_batch([a, bad])
        with pytest.raises(ValueError, match="ensemble"):
            mpc.run_mpc_batch([a, bad])
