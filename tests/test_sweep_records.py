"""The elite and to-go records of sweeps without a GPU (include/mbd_hip.h mbd_sweep_set_elites, mbd_sweep_set_togo): the header,
mbd_hip._capi.EXPORTS and the library agree on the new names; the argument errors that need no device; mpc.py's argument handling
builds the sweep's set_* calls from the flags.  tests/test_gpu_sweep_elites.py and tests/test_gpu_sweep_togo.py hold the device code."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = ("mbd_sweep_set_elites", "mbd_sweep_peek_elites", "mbd_sweep_set_togo", "mbd_sweep_peek_togo")
DEBUG = ("mbd_debug_sweep_elites_step", "mbd_debug_sweep_togo_step")


def _header(name):
    text = open(os.path.join(ROOT, "include", name)).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_exports_and_library_agree(lib):
    from mbd_hip import _capi
    text, code = _header("mbd_hip.h")
    for n in NEW:
        assert re.search(rf"\bint {n}\s*\(", code), f"{n} is not declared in include/mbd_hip.h"
        assert n in _capi.EXPORTS and hasattr(lib, n), n
    _, dbg = _header("mbd_hip_debug.h")
    for n in DEBUG:
        assert re.search(rf"\bint {n}\s*\(", dbg) and hasattr(lib, n), n
        assert n not in _capi.EXPORTS, "the debug entries are no part of the boundary"
    assert "Sweeps have no such call" not in text


def test_argument_errors_need_no_device(lib):
    from mbd_hip import _capi
    INVALID = _capi.MBD_ERR_INVALID
    erec, trec = _capi.elites_record(3, True, False), _capi.togo_record(5, 1)
    assert lib.mbd_sweep_set_elites(None, C.byref(erec)) == INVALID and b"sweep is NULL" in lib.mbd_last_error()
    assert lib.mbd_sweep_set_elites(None, None) == INVALID
    assert lib.mbd_sweep_set_togo(None, C.byref(trec)) == INVALID and b"sweep is NULL" in lib.mbd_last_error()
    assert lib.mbd_sweep_peek_elites(None, 0, None, None, None, None, None, None, None, 0, None) == INVALID
    assert lib.mbd_sweep_peek_togo(None, 0, None, None, None, None) == INVALID
    # the debug entries: their argument errors come before the device
    f32 = np.float32
    P, N, HNu = 2, 8, 3
    rews, cand, ybar = np.zeros((P, N), f32), np.zeros((P, N, HNu), f32), np.zeros((P, HNu), f32)
    E, cnt = np.zeros((P, 2, HNu), f32), np.zeros(P, np.int32)
    for kw, field in ((dict(n_elites=33), "n_elites=33"), (dict(nominal=2), "nominal=2"), (dict(n_elites=7, nominal=1), "must lie below N"),
                      (dict(sigma=0.0), "sigma=0")):
        a = dict(sigma=0.5, n_elites=2, nominal=1)
        a.update(kw)
        with pytest.raises(_capi.MbdError) as e:
            _capi.debug_sweep_elites_step(rews, cand, ybar, a["sigma"], True, None, a["n_elites"], a["nominal"],
                                          np.zeros((P, max(a["n_elites"], 1), HNu), f32), cnt)
        assert e.value.code == INVALID and field in str(e.value), field
    with pytest.raises(_capi.MbdError) as e:
        _capi.debug_sweep_elites_step(rews, cand, ybar, 0.5, True, None, 2, 1, E, np.array([0, 3], np.int32))
    assert e.value.code == INVALID and "count[1]=3" in str(e.value)
    big = 33
    with pytest.raises(_capi.MbdError) as e:
        _capi.debug_sweep_elites_step(np.zeros((big, N), f32), np.zeros((big, N, HNu), f32), np.zeros((big, HNu), f32), 0.5, True, None, 2, 1,
                                      np.zeros((big, 2, HNu), f32), np.zeros(big, np.int32))
    assert e.value.code == INVALID and "P=33" in str(e.value)
    H, Nu = 4, 2
    tc = np.zeros((P, N, H * Nu), f32), np.zeros((P, H * Nu), f32), np.zeros((P, N), f32), np.zeros((P, N, H), f32)
    for (block, mt), field in (((0, 1), "block=0"), ((1, 0), "min_tail=0"), ((1, H + 1), "min_tail=5")):
        with pytest.raises(_capi.MbdError) as e:
            _capi.debug_sweep_togo_step(np.ones(P, f32), *tc, Nu, block, mt, True, 0.5, True, 0.99, 0.9, 0.91, True, 1)
        assert e.value.code == INVALID and field in str(e.value), field


class _Recorder:
    """Stands in for a Sweep: records the set_* calls ``mpc._setup_batch`` makes."""

    def __init__(self, *a, **kw):
        self.calls, self.P = {}, a[2]

    def __getattr__(self, name):
        if name.startswith("set_"):
            return lambda *a, **kw: self.calls.__setitem__(name, (a, kw))
        raise AttributeError(name)


def test_the_python_layer_maps_every_flag(monkeypatch):
    """--n_episodes 8 --elites 4 --elite_carry --togo_block 10 reaches Sweep.set_elites and Sweep.set_togo with the right arguments;
    --adapt_rate with --n_episodes 8 ends with a ValueError that names the adapt record; _check_togo's refusals hold for batches."""
    from dataclasses import replace

    from mbd_hip.planners import mpc
    base = mpc.MpcArgs(env_name="hopper", not_render=True, disable_recommended_params=True)
    args = replace(base, elites=4, elite_carry=True, togo_block=10)
    arg_list = [replace(args, seed=k) for k in range(8)]
    mpc._check_batch_records(arg_list)
    with pytest.raises(ValueError, match="of its own"):  # (the episodes' own arguments take none: the record is the batch's)
        mpc._check_batch(arg_list)

    class _Env:
        action_size = 3
    made = []
    monkeypatch.setattr(mpc, "get_env", lambda name, device=0: _Env())
    monkeypatch.setattr(mpc, "Sweep", lambda *a, **kw: made.append(_Recorder(*a, **kw)) or made[-1])
    monkeypatch.setattr(mpc, "_reset_and_key", lambda env, seed: (seed, (0, seed)))
    mpc._setup_batch(arg_list, 0)
    calls = made[0].calls
    assert made[0].P == 8
    assert calls["set_elites"] == ((), dict(n_elites=4, nominal=False, carry=True))
    assert calls["set_togo"] == ((), dict(block=10, min_tail=1))
    made.clear()
    mpc._setup_batch([replace(base, seed=k) for k in range(2)], 0)
    assert "set_elites" not in made[0].calls and "set_togo" not in made[0].calls, "no flag, no record"
    made.clear()
    mpc._setup_batch([replace(base, elite_nominal=True, togo_block=5, togo_min_tail=10, seed=k) for k in range(2)], 0)
    assert made[0].calls["set_elites"] == ((), dict(n_elites=0, nominal=True, carry=False))
    assert made[0].calls["set_togo"] == ((), dict(block=5, min_tail=10))
    with pytest.raises(ValueError, match="adapt record"):
        mpc._check_batch_records([replace(base, adapt_rate=0.3, seed=k) for k in range(8)])
    with pytest.raises(ValueError, match="adapt record"):
        mpc._main(["--env_name", "hopper", "--adapt_rate", "0.3", "--n_episodes", "8"])
    with pytest.raises(ValueError, match="togo_block"):
        mpc._check_batch_records([replace(args, effort_cost=0.1, seed=k) for k in range(8)])
    with pytest.raises(ValueError, match="elites"):
        mpc._check_batch_records([args, replace(args, elites=3, seed=1)])
    with pytest.raises(ValueError, match="togo_min_tail"):
        mpc._check_batch_records([args, replace(args, togo_min_tail=3, seed=1)])
