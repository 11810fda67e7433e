"""Noise shapes without a GPU (include/mbd_hip.h mbd_noise_shape, mbd_plan_set_noise_shape, mbd_sweep_set_noise_shape;
mbd_hip.planners.mpc.tail_shape and its arguments; DESIGN.md section 1 "N7 noise shape").

The two setters are exported and refuse every bad record with MBD_ERR_INVALID, naming the field, before touching a device;
the ctypes record has the header's layout; tail_shape is the table computed by hand; and the checker's restatement
(tests/noise_shape_checker.py) keeps the contract's two consequences bit for bit — all ones is no shape, zeros freeze their
elements at clip(Ybar) — and the warm mode's "tick 0 does not see the shape".  The kernels are held to that restatement in
tests/test_gpu_noise_shape.py."""
import ctypes as C
import os
import shutil
import subprocess
from dataclasses import replace

import numpy as np
import pytest

import mpc_checker
import noise_shape_checker as nsc
from conftest import ROOT, load_model
from oracle import planner as op


def _oenv(orc, name):
    m = load_model(name)
    return op.OracleEnv(orc, name, m.to_struct(), init_q=m.init_q)


def _reset(orc, oe, seed):
    return np.asarray(oe.reset(orc.split(orc.prng_key(seed), 2, 1)[1], 1), np.float32)


def _record(_capi, g, rows=None, cols=None, when=0):
    g = np.ascontiguousarray(g, np.float32)
    rec = _capi.NoiseShape()
    rec.scale = g.ctypes.data_as(C.POINTER(C.c_float))
    rec.rows = g.shape[0] if rows is None else rows
    rec.cols = g.shape[1] if cols is None else cols
    rec.when = when
    return rec, g


def test_setters_are_exported(lib):
    from mbd_hip import _capi
    for name in ("mbd_plan_set_noise_shape", "mbd_sweep_set_noise_shape"):
        assert name in _capi.EXPORTS and hasattr(lib, name), name
    assert (_capi.NOISE_ALWAYS, _capi.NOISE_WARM_TICKS) == (0, 1)
    text = open(os.path.join(ROOT, "include", "mbd_hip.h")).read()
    assert "#define MBD_NOISE_ALWAYS     0" in text and "#define MBD_NOISE_WARM_TICKS 1" in text


def test_the_ctypes_record_has_the_headers_layout(tmp_path):
    from mbd_hip import _capi
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a C compiler is what builds the checker as well"
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mbd_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(mbd_noise_shape), offsetof(mbd_noise_shape, scale), '
                   'offsetof(mbd_noise_shape, rows), offsetof(mbd_noise_shape, cols), offsetof(mbd_noise_shape, when), '
                   'offsetof(mbd_noise_shape, reserved)); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = _capi.NoiseShape
    assert got == [C.sizeof(S), S.scale.offset, S.rows.offset, S.cols.offset, S.when.offset, S.reserved.offset]


@pytest.mark.parametrize("setter", ["mbd_plan_set_noise_shape", "mbd_sweep_set_noise_shape"])
def test_argument_errors_come_before_any_device_access(lib, setter):
    """Every refusal the record alone decides, on a box with no device: MBD_ERR_INVALID and the field's name.  The handle is
    a zeroed stand-in (Hsample = 0, action_size = 0), so a record that passes its own checks is refused for its rows — still
    before the device is touched."""
    from mbd_hip import _capi
    fn = getattr(lib, setter)
    ok, keep = _record(_capi, np.ones((4, 3), np.float32))

    def refused(rec, field, handle):
        assert fn(handle, C.byref(rec)) == _capi.MBD_ERR_INVALID, field
        assert field in lib.mbd_last_error(), (field, lib.mbd_last_error())

    refused(ok, b"plan" if "plan" in setter else b"sweep", None)
    stand_in = C.create_string_buffer(1 << 16)
    r, _ = _record(_capi, keep)
    r.reserved[3] = 1
    refused(r, b"reserved[3]", stand_in)
    for when in (-1, 2, 7):
        refused(_record(_capi, keep, when=when)[0], b"when", stand_in)
    r, _ = _record(_capi, keep)
    r.scale = None
    refused(r, b"scale is NULL", stand_in)
    refused(_record(_capi, keep, rows=0)[0], b"rows=0", stand_in)
    refused(_record(_capi, keep, rows=-4)[0], b"rows=-4", stand_in)
    refused(_record(_capi, keep, cols=0)[0], b"cols=0", stand_in)
    for bad in (-1.0, -1e-30, np.nan, np.inf, -np.inf):
        g = np.ones((4, 3), np.float32)
        g[2, 1] = bad
        rec, g = _record(_capi, g)
        refused(rec, b"scale[2][1]", stand_in)
    g = np.ones((4, 3), np.float32)
    g[0, 0] = -0.0  # (-0.0 >= 0: accepted by the value check, then refused for the stand-in's sizes)
    g[3, 2] = 0.0
    rec, g = _record(_capi, g)
    refused(rec, b"rows=4", stand_in)
    refused(ok, b"Hsample", stand_in)


def test_tail_shape_is_the_table_computed_by_hand():
    from mbd_hip.planners.mpc import tail_shape
    g = tail_shape(6, 2, 3, 4.0)
    assert g.dtype == np.float32 and g.shape == (6, 2) and g.flags["C_CONTIGUOUS"]
    assert np.array_equal(g, np.array([[1, 1], [1, 1], [1, 1], [2, 2], [3, 3], [4, 4]], np.float32))
    # 1 + 1.5 k / 4 for k = 1..4: exact in float32
    assert np.array_equal(tail_shape(5, 1, 4, 2.5)[:, 0], np.array([1.0, 1.375, 1.75, 2.125, 2.5], np.float32))
    # 1 + 3.2 k / 5: float64, rounded once
    assert np.array_equal(tail_shape(7, 3, 5, 4.2)[:, 2], np.array([1, 1, 1.64, 2.28, 2.92, 3.56, 4.2], np.float32))
    # a peak below 1 ramps down; 0 switches the last row's noise off
    assert np.array_equal(tail_shape(4, 1, 2, 0.0)[:, 0], np.array([1, 1, 0.5, 0], np.float32))
    assert np.array_equal(tail_shape(4, 2, 0, 9.0), np.ones((4, 2), np.float32))
    assert np.array_equal(tail_shape(3, 1, 3, 4.0)[:, 0], np.array([2, 3, 4], np.float32))
    for bad in (dict(rows=-1), dict(rows=5), dict(peak=-0.5), dict(peak=np.nan), dict(peak=np.inf)):
        kw = dict(H=4, Nu=2, rows=2, peak=2.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            tail_shape(**kw)


def test_arguments_without_a_shape_set_none_and_a_batch_shares_one(tmp_path):
    from mbd_hip.planners import mpc
    a = mpc.MpcArgs(env_name="hopper", Nsample=16, Hsample=6, Ndiffuse=6, disable_recommended_params=True, not_render=True)
    assert not mpc._has_shape(a) and (a.tail_rows, a.tail_sigma, a.noise_shape) == (0, 1.0, "")
    b = replace(a, tail_rows=2, tail_sigma=4.0)
    g, when = mpc._shape_of(b, 3)
    assert mpc._has_shape(b) and when == "warm" and np.array_equal(g, mpc.tail_shape(6, 3, 2, 4.0))
    path = str(tmp_path / "g.npy")
    np.save(path, np.array([1.0, 0.5, 2.0], np.float32))
    c = replace(a, noise_shape=path)
    g, when = mpc._shape_of(c, 3)
    assert mpc._has_shape(c) and when == "always" and np.array_equal(g, np.array([1.0, 0.5, 2.0], np.float32))
    with pytest.raises(ValueError, match="one noise shape"):
        mpc._shape_of(replace(b, noise_shape=path), 3)
    mpc._check_batch([b, replace(b, seed=1)])
    with pytest.raises(ValueError, match="tail_rows"):
        mpc._check_batch([b, replace(a, seed=1)])


# hopper, N = 16, H = 4: the sizes of the issue's checker tests
N, H, ND = 16, 4, 6


def _step_inputs(orc):
    oe = _oenv(orc, "hopper")
    s0 = _reset(orc, oe, 2)
    sched = orc.schedule(1e-4, 1e-2, ND)
    Ybar = (np.random.default_rng(5).normal(size=(H, oe.Nu)) * 0.3).astype(np.float32)
    Ybar[1, 2], Ybar[3, 0] = 1.5, -0.0  # (outside the clip; a signed zero)
    return oe, s0, sched, Ybar


def test_checker_with_all_ones_is_reverse_once(orc):
    oe, s0, sched, Ybar = _step_inputs(orc)
    key = orc.prng_key(11)
    for i in (ND - 1, 1):
        ref = op.reverse_once(orc, oe, s0, i, key, Ybar, sched, N, H, 0.1, 1)
        got = nsc.reverse_once(orc, oe, np.ones((H, oe.Nu), np.float32), s0, i, key, Ybar, sched, N, H, 0.1, 1)
        flat = nsc.reverse_once(orc, oe, None, s0, i, key, Ybar, sched, N, H, 0.1, 1)
        for other in (got, flat):
            assert np.array_equal(other[0], ref[0])
            assert other[1].tobytes() == ref[1].tobytes() and np.float32(other[2]).tobytes() == np.float32(ref[2]).tobytes()
            for k in ("Y0s", "rewss", "rews", "weights"):
                assert other[3][k].tobytes() == ref[3][k].tobytes(), k


def test_checker_zeros_freeze_their_elements_at_the_clipped_mean(orc):
    oe, s0, sched, Ybar = _step_inputs(orc)
    key = orc.prng_key(12)
    g = np.ones((H, oe.Nu), np.float32)
    g[:, 1] = 0.0   # actuator 1 frozen
    g[2, :] = 0.0   # row 2 frozen
    g[0, 0] = 2.5
    i = ND - 1
    _, Ybar_im1, _, det = nsc.reverse_once(orc, oe, g, s0, i, key, Ybar, sched, N, H, 0.1, 1)
    Y0s = det["Y0s"]
    clipped = np.clip(Ybar, np.float32(-1), np.float32(1))
    assert np.array_equal(Y0s[:, :, 1], np.broadcast_to(clipped[:, 1], (N, H)))
    assert np.array_equal(Y0s[:, 2, :], np.broadcast_to(clipped[2], (N, oe.Nu)))
    # the other elements move, and by the three roundings of the contract
    flat = op.reverse_once(orc, oe, s0, i, key, Ybar, sched, N, H, 0.1, 1)[3]["Y0s"]
    _, eps = orc.sample(orc.split(key, 2, 1)[1], 1, N, H, oe.Nu, 0, N, float(sched[2][i]), Ybar, want_eps=True)
    assert np.array_equal(Y0s[:, 1, 0], flat[:, 1, 0]) and not np.array_equal(Y0s[:, 0, 0], flat[:, 0, 0])
    want = np.clip(((eps[:, 0, 0] * np.float32(2.5)).astype(np.float32) * np.float32(sched[2][i])).astype(np.float32)
                   + Ybar[0, 0], np.float32(-1), np.float32(1)).astype(np.float32)
    assert Y0s[:, 0, 0].tobytes() == want.tobytes()
    assert np.isfinite(Ybar_im1).all()


def test_checker_warm_episode_leaves_tick_0_alone(orc):
    """MBD_NOISE_WARM_TICKS in the checker: tick 0 is mpc_checker.episode's, T ticks are a prefix of T + 1, the later ticks
    differ from the flat episode's; MBD_NOISE_ALWAYS with all ones is the flat episode throughout."""
    oe = _oenv(orc, "hopper")
    s0 = _reset(orc, oe, 1)
    key = orc.prng_key(4)
    T, K, E = 3, 2, 1
    g = np.ones((H, oe.Nu), np.float32)
    g[-2:] = np.array([[2.5], [4.0]], np.float32)
    ref = mpc_checker.episode(oe, s0, key, N, H, ND, 0.1, T, K, E)
    warm = nsc.episode(mpc_checker.episode, oe, g, "warm", ND, s0, key, N, H, ND, 0.1, T, K, E)
    assert np.array_equal(warm["means"][0], ref["means"][0]) and np.array_equal(warm["states"][:2], ref["states"][:2])
    assert np.array_equal(warm["actions"][:E], ref["actions"][:E]) and np.array_equal(warm["rewards"][:E], ref["rewards"][:E])
    assert not np.array_equal(warm["means"][1], ref["means"][1])
    shorter = nsc.episode(mpc_checker.episode, oe, g, "warm", ND, s0, key, N, H, ND, 0.1, T - 1, K, E)
    for k in ("means", "actions", "rewards"):
        assert np.array_equal(shorter[k], warm[k][: len(shorter[k])]), k
    assert np.array_equal(shorter["states"], warm["states"][:T])
    always = nsc.episode(mpc_checker.episode, oe, g, "always", ND, s0, key, N, H, ND, 0.1, T, K, E)
    assert not np.array_equal(always["means"][0], ref["means"][0])
    ones = nsc.episode(mpc_checker.episode, oe, np.ones_like(g), "always", ND, s0, key, N, H, ND, 0.1, T, K, E)
    for k in ("means", "actions", "rewards", "states"):
        assert ones[k].tobytes() == ref[k].tobytes(), k
