"""Episodes that follow a demonstration on the episode's clock (include/mbd_hip.h mbd_mpc_demo; DESIGN.md section 1 "N10 demo
clock") — what holds without a GPU.

  binding        the four symbols are exported, the ctypes struct has the header's layout, NULL handles are refused first
  the checker    tests/mpc_demo_checker.py: tick 0 under the env's own demo is oracle.planner.run_diffusion's demo plan; the
                 window formula at c0 = 0, inside the clip, across its end and wholly past it; asking the executed rows'
                 rollout for the tracked positions changes neither its rewards nor its final state
  able to tell   for every case tests/test_gpu_mpc_demo.py runs, the checker's means under the moving windows differ, at some
                 tick >= 1, from its means with tick 0's window frozen — so an implementation without a clock cannot pass.  (The
                 "held" shape starts past the clip's end: all its windows ARE one row, moving or not; there the checker tells
                 the held row from the clip's start instead.)
  cycle_clip     the rows of the clip untouched, the period displacement to 1 float32 ulp, the refusals
  arguments      the command line's demo flags and what a batch of episodes accepts
"""
import ctypes as C
import os
import re
from dataclasses import replace
from types import SimpleNamespace

import numpy as np
import pytest

import mpc_checker
import mpc_demo_checker as mdc
from conftest import ROOT

NAMES = ("mbd_plan_set_mpc_demo", "mbd_sweep_set_mpc_demo", "mbd_plan_peek_mpc_track", "mbd_sweep_peek_mpc_track")


# ---- the binding ------------------------------------------------------------------------------------------------------------

def _header_struct(name):
    """[(field, ctype, count)] of a struct of include/mbd_hip.h, in order."""
    with open(os.path.join(ROOT, "include", "mbd_hip.h")) as f:
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), f.read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.fullmatch(r"(const float\*|int32_t|float|uint32_t)\s+(\w+)(?:\[(\d+)\])?", re.sub(r"\s+", " ", decl))
        assert m, decl
        out.append((m.group(2), m.group(1), int(m.group(3) or 1)))
    return out


def test_the_symbols_are_exported_and_the_struct_has_the_headers_layout(lib):
    from mbd_hip import _capi
    for n in NAMES:
        assert n in _capi.EXPORTS and hasattr(lib, n), n
    size_align = {"const float*": (C.sizeof(C.c_void_p),) * 2, "int32_t": (4, 4), "float": (4, 4), "uint32_t": (4, 4)}
    off, worst = 0, 1
    fields = _header_struct("mbd_mpc_demo")
    assert [f for f, _, _ in fields] == ["clip", "n_rows", "start_row", "rew_xref", "reserved"]
    for f, ctype, count in fields:
        size, align = size_align[ctype]
        off = (off + align - 1) // align * align
        assert getattr(_capi.MpcDemo, f).offset == off and getattr(_capi.MpcDemo, f).size == size * count, f
        off, worst = off + size * count, max(worst, align)
    assert C.sizeof(_capi.MpcDemo) == (off + worst - 1) // worst * worst


def test_null_handles_are_refused_before_any_device_access(lib):
    from mbd_hip import _capi
    clip = np.zeros((1, 3, 3), np.float32)
    rec = _capi.MpcDemo(clip=clip.ctypes.data_as(C.POINTER(C.c_float)), n_rows=3, start_row=0, rew_xref=1.0)
    out = np.zeros(4, np.float32)
    for call, word in ((lambda: lib.mbd_plan_set_mpc_demo(None, C.byref(rec)), b"plan"),
                       (lambda: lib.mbd_sweep_set_mpc_demo(None, C.byref(rec)), b"sweep"),
                       (lambda: lib.mbd_plan_peek_mpc_track(None, _capi.np_ptr(out), None), b"plan"),
                       (lambda: lib.mbd_sweep_peek_mpc_track(None, 0, _capi.np_ptr(out), None), b"sweep")):
        assert call() == _capi.MBD_ERR_INVALID and word in lib.mbd_last_error()


# ---- the checker ------------------------------------------------------------------------------------------------------------

def test_tick0_under_the_envs_own_demo_is_run_diffusions_demo_plan(orc):
    """clip = the env's xref, c0 = 0, rew_xref = the env's, T = 1 (car2d, N = 32, Nd = 5): the tick's mean is the reverse loop
    with enable_demo on the UNCHANGED env from k_0 = split(key)[1] — and that loop, from run_diffusion's own rng_exp, is
    oracle.planner.run_diffusion's demo plan, bit for bit."""
    from oracle import planner as op
    oe = mdc.oracle_env(orc, "car2d")
    N, H, Nd, temp, seed = 32, mdc.ROWS, 5, 0.1, 3
    sched = orc.schedule(1e-4, 1e-2, Nd)

    def loop(r, s0):
        Y = np.zeros((H, oe.Nu), np.float32)
        for i in range(Nd - 1, 0, -1):
            r, Y, _, _ = op.reverse_once(orc, oe, s0, i, r, Y, sched, N, H, temp, 1, enable_demo=True)
        return Y

    ref = op.run_diffusion(orc, oe, seed, N, H, Nd, temp, impl=1, enable_demo=True)
    rng, _ = orc.split(orc.prng_key(seed), 2, 1)
    rng_exp = orc.split(rng, 2, 1)[0]
    s0 = ref["state_init"]
    assert np.array_equal(loop(rng_exp, s0), ref["mu_0ts"][-1])  # (the loop below is run_diffusion's)
    key = orc.prng_key(9)
    ep = mdc.episode(oe, oe.xref, 0, oe.rew_xref, s0, key, N, H, Nd, temp, T=1, K=2, E=1, impl=1)
    assert np.array_equal(ep["means"][0], loop(orc.split(key, 2, 1)[1], s0))
    assert np.array_equal(ep["demo_windows"][0, 0], oe.xref)
    plain = mpc_checker.episode(oe, s0, key, N, H, Nd, temp, T=1, K=2, E=1)
    assert not np.array_equal(plain["means"][0], ep["means"][0])  # (the demo term takes part)


def test_window_formula():
    L, K = 57, 2
    clip = np.arange(K * L * 3, dtype=np.float32).reshape(K, L, 3)
    E = 3
    w = mdc.window(clip, 0, 0, E)
    assert w.shape == (K, 50, 3) and np.array_equal(w, clip[:, :50])  # c0 = 0, tick 0: the first 50 rows
    assert np.array_equal(mdc.window(clip, 2, 1, E), clip[:, 5:55])  # inside the clip
    w = mdc.window(clip, 2, 2, E)  # across the end: rows 8 .. 56, then 56 held
    assert np.array_equal(w[:, :49], clip[:, 8:57]) and np.array_equal(w[:, 49], clip[:, 56])
    w = mdc.window(clip, 60, 1, 1)  # wholly past it
    assert np.array_equal(w, np.broadcast_to(clip[:, 56:57], (K, 50, 3)))
    assert np.array_equal(mdc.window(clip, 2, 0, 2, D=1), clip[:, 4:54])  # a delayed tick plans for tick t + D
    assert np.array_equal(mdc.window(clip, 2**31 - 1, 10**6, 7), mdc.window(clip, 60, 0, 1))  # (no overflow)
    car = np.arange(2 * L, dtype=np.float32).reshape(L, 2)
    assert np.array_equal(mdc.window(car, 3, 0, 1)[0], car[3:53]) and mdc.windows(car, 3, 4, 1).shape == (4, 1, 50, 2)
    for xref in (clip[:, :50], car[:50]):
        ext = mdc.as_tracks(mdc.extended(xref))
        assert ext.shape[1] == 57
        for k in range(ext.shape[0]):
            assert len({r.tobytes() for r in ext[k]}) == 57


@pytest.mark.parametrize("name", ["humanoidtrack", "car2d"])
def test_asking_for_the_positions_changes_neither_rewards_nor_state(orc, name):
    oe = mdc.oracle_env(orc, name)
    s0 = np.asarray(oe.reset(orc.prng_key(5), 1), np.float32).reshape(-1)
    rows = np.random.default_rng(1).uniform(-1, 1, (4, oe.Nu)).astype(np.float32)
    rew, s1 = mpc_checker.execute(oe, s0, rows)
    rew2, s2, xpos = mdc.execute_tracked(oe, s0, rows)
    assert np.array_equal(rew, rew2) and np.array_equal(np.asarray(s1).reshape(-1), s2)
    assert xpos.shape == (4, 1 if name == "car2d" else oe.ms.n_track, 3) and np.isfinite(xpos).all()
    clip = mdc.extended(oe.xref)
    err = mdc.track_err(xpos, clip, 2)
    c = mdc.as_tracks(clip)
    assert err.shape == xpos.shape[:2]
    assert np.isclose(err[1, 0], np.linalg.norm(xpos[1, 0, : c.shape[2]].astype(np.float64) - c[0, 3].astype(np.float64)))


# ---- the inputs must be able to tell ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,variant", [("humanoidtrack", "moving"), ("humanoidtrack", "delay"), ("humanoidtrack", "plant"),
                                          ("car2d", "moving")])
def test_moving_windows_differ_from_a_frozen_window(orc_omp, name, variant):
    ep, info = mdc.case(orc_omp, name, variant)
    frozen, _ = mdc.case(orc_omp, name, variant, frozen=True)
    T = info["T"]
    assert not np.array_equal(ep["demo_windows"][1], ep["demo_windows"][0])
    assert np.array_equal(ep["means"][0], frozen["means"][0])  # (tick 0 plans under the same window either way)
    assert any(not np.array_equal(ep["means"][t], frozen["means"][t]) for t in range(1, T)), \
        f"{name} {variant}: the means cannot tell the moving windows from tick 0's"
    assert np.isfinite(ep["states"]).all() and np.isfinite(ep["track_err"]).all() and (ep["track_err"] > 0).all()


@pytest.mark.parametrize("name", ["humanoidtrack", "car2d"])
def test_held_windows_differ_from_the_clips_start(orc_omp, name):
    """c0 = 60 is past the 57-row clip: every window is the last row, whatever the tick — the means tell that row from the
    clip's first 50 rows.  (The case's clip is the synthetic one played backwards, so that its last row is where the system
    starts: see mpc_demo_checker.case.)"""
    ep, info = mdc.case(orc_omp, name, "held")
    clip = mdc.as_tracks(info["clip"])
    assert np.array_equal(ep["demo_windows"], np.broadcast_to(clip[None, :, -1:], ep["demo_windows"].shape))
    oe = mdc.oracle_env(orc_omp, name)
    from mbd_hip.envs.base import prng_impl
    start = mdc.episode(oe, info["clip"], 0, info["rew_xref"], info["state0"], info["key"], mdc.N, mdc.ROWS, mdc.ND, mdc.TEMP, 1,
                        mdc.WARM, info["E"], impl=prng_impl())
    assert not np.array_equal(start["means"][0], ep["means"][0])
    for e in (ep, start):
        assert np.isfinite(e["means"]).all() and np.isfinite(e["states"]).all() and np.isfinite(e["track_err"]).all()


# ---- cycle_clip -------------------------------------------------------------------------------------------------------------

def test_cycle_clip():
    from mbd_hip.planners.mpc import cycle_clip
    g = np.random.default_rng(0)
    K, L0, period, n = 3, 46, 11, 46 + 3 * 11 + 5
    t = np.arange(L0)[None, :, None]
    xref = (g.normal(size=(K, 1, 3)) + 0.03 * t * np.array([1.0, 0.1, 0.0]) + 0.05 * np.sin(0.4 * t + g.normal(size=(K, 1, 3)))).astype(np.float32)
    out = cycle_clip(xref, n, period)
    assert out.dtype == np.float32 and out.shape == (K, n, 3)
    assert np.array_equal(out[:, :L0], xref)
    disp = xref[:, L0 - 1].astype(np.float64) - xref[:, L0 - 1 - period].astype(np.float64)
    for i in range(n - L0):
        got = out[:, L0 + i].astype(np.float64) - out[:, L0 - period + i].astype(np.float64)
        ulp = np.maximum(np.spacing(np.abs(out[:, L0 + i])), np.spacing(np.abs(out[:, L0 - period + i]))).astype(np.float64)
        assert (np.abs(got - disp) <= ulp).all(), i
    assert np.array_equal(cycle_clip(xref, 20, period), xref[:, :20])  # (fewer rows than the clip: its head)
    flat = cycle_clip(xref[0, :, :2], L0 + 4, 5)  # a car2d clip [L0, 2]
    assert flat.shape == (L0 + 4, 2) and np.array_equal(flat[:L0], xref[0, :, :2])
    for bad in (0, -1, L0, L0 + 3):
        with pytest.raises(ValueError, match="period"):
            cycle_clip(xref, n, bad)
    with pytest.raises(ValueError, match="n_rows"):
        cycle_clip(xref, 0, period)


# ---- the arguments ----------------------------------------------------------------------------------------------------------

def _args(**kw):
    from mbd_hip.planners.mpc import MpcArgs
    return MpcArgs(env_name="humanoidtrack", Nsample=64, Hsample=50, Ndiffuse=6, temp_sample=0.1, n_ticks=4, warm_steps=2,
                   exec_steps=3, disable_recommended_params=True, not_render=True, **kw)


def test_demo_arguments(tmp_path):
    from mbd_hip.planners import mpc
    a = _args()
    assert (a.demo_clip, a.demo_start, a.demo_period) == ("", 0, 0) and not mpc._has_demo(a) and mpc._demo_settings(a) == {}
    xref = np.load(os.path.join(ROOT, "model-based-diffusion_amd", "assets", "compiled", "jog_xref.npy")).astype(np.float32)
    env = SimpleNamespace(xref=xref)
    clip, c0 = mpc._demo_of(env, _args(enable_demo=True, demo_clip="env", demo_start=4))
    assert c0 == 4 and np.array_equal(clip, xref)
    d = _args(enable_demo=True, demo_clip="env", demo_start=4, demo_period=20, delay_ticks=2)
    clip, _ = mpc._demo_of(env, d)
    assert clip.shape == (5, 4 + (4 + 2) * 3 + 50, 3) and np.array_equal(clip, mpc.cycle_clip(xref, clip.shape[1], 20))
    path = str(tmp_path / "clip.npy")
    np.save(path, xref[:, :30])
    clip, _ = mpc._demo_of(env, _args(enable_demo=True, demo_clip=path))
    assert np.array_equal(clip, xref[:, :30])
    with pytest.raises(ValueError, match="demo_clip"):
        mpc._demo_of(SimpleNamespace(xref=None), _args(enable_demo=True, demo_clip="env"))
    with pytest.raises(ValueError, match="demo_period"):
        mpc._demo_of(env, _args(enable_demo=True, demo_clip="env", demo_period=-2))
    assert mpc._demo_settings(d) == dict(demo_clip="env", demo_start=4, demo_period=20)


def test_what_a_batch_accepts():
    from mbd_hip.planners.mpc import _check_batch
    with pytest.raises(ValueError, match="enable_demo"):  # as before: a demo plan has no clock of its own
        _check_batch([_args(enable_demo=True), _args(enable_demo=True, seed=1)])
    ok = _args(enable_demo=True, demo_clip="env", demo_start=2)
    _check_batch([ok, replace(ok, seed=1, temp_sample=0.2)])
    for field, other in (("demo_clip", "other.npy"), ("demo_start", 3), ("demo_period", 7)):
        with pytest.raises(ValueError, match=field):
            _check_batch([ok, replace(ok, seed=1, **{field: other})])
    with pytest.raises(ValueError, match="enable_demo"):
        _check_batch([_args(demo_clip="env")])
