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
