"""Receding-horizon episodes planned ahead of the plant, without a GPU (include/mbd_hip.h mbd_mpc_delay, mbd_plan_set_mpc_delay,
mbd_sweep_set_mpc_delay, mbd_plan_peek_mpc_predicted, mbd_sweep_peek_mpc_predicted; DESIGN.md section 1 "N9 delay").

The four calls are exported, the ctypes record has the header's layout, the set calls refuse every bad record with
MBD_ERR_INVALID, naming the field, before touching a device, and the peek calls answer MBD_ERR_STATE without a record.  The
handles are zeroed stand-ins, as in tests/test_noise_shape.py; their action_size is 0, so the one refusal that needs a row to
look at — a non-finite row value — is reached through mbd_debug_check_mpc_delay (include/mbd_hip_debug.h), the function both
set calls run on their record (tests/test_gpu_mpc_delay.py reaches it through real handles, and the run call's refusal too).
The checker's restatement (tests/mpc_delay_checker.py) keeps the semantics' consequences bit for bit: the D = 1 shift
identity, the prefix property, and a prediction that is the PLAN's env's, not the plant's."""
import ctypes as C
import os
import shutil
import subprocess
from dataclasses import replace

import numpy as np
import pytest

import mpc_checker
import mpc_delay_checker as mdc
import mpc_plant_checker
from conftest import ROOT, load_model
from oracle import planner as op

_LOGS = ("means", "actions", "rewards", "states")


def _oenv(orc, name, **scale):
    m = load_model(name).scaled(**scale)
    return op.OracleEnv(orc, name, m.to_struct(), init_q=m.init_q)


def _reset(orc, oe, seed):
    return np.asarray(oe.reset(orc.split(orc.prng_key(seed), 2, 1)[1], 1), np.float32)


def _record(_capi, ticks=1, rows0=None, n_rows=None):
    rec = _capi.MpcDelay()
    rec.delay_ticks = ticks
    keep = None
    if rows0 is not None:
        keep = np.ascontiguousarray(rows0, np.float32)
        rec.rows0 = keep.ctypes.data_as(C.POINTER(C.c_float))
        rec.n_rows = keep.shape[0]
    if n_rows is not None:
        rec.n_rows = n_rows
    return rec, keep


def test_calls_are_exported(lib):
    from mbd_hip import _capi
    for name in ("mbd_plan_set_mpc_delay", "mbd_sweep_set_mpc_delay", "mbd_plan_peek_mpc_predicted",
                 "mbd_sweep_peek_mpc_predicted"):
        assert name in _capi.EXPORTS and hasattr(lib, name), name
    assert _capi.MAX_MPC_DELAY == 8
    assert "#define MBD_MAX_MPC_DELAY 8" in open(os.path.join(ROOT, "include", "mbd_hip.h")).read()


def test_the_ctypes_record_has_the_headers_layout(tmp_path):
    from mbd_hip import _capi
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a C compiler is what builds the checker as well"
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mbd_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(mbd_mpc_delay), offsetof(mbd_mpc_delay, rows0), '
                   'offsetof(mbd_mpc_delay, delay_ticks), offsetof(mbd_mpc_delay, n_rows), offsetof(mbd_mpc_delay, reserved)); '
                   'return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = _capi.MpcDelay
    assert got == [C.sizeof(S), S.rows0.offset, S.delay_ticks.offset, S.n_rows.offset, S.reserved.offset]


@pytest.mark.parametrize("setter", ["mbd_plan_set_mpc_delay", "mbd_sweep_set_mpc_delay"])
def test_argument_errors_come_before_any_device_access(lib, setter):
    """Every refusal of the set call that a handle of action_size 0 can reach, on a box with no device: MBD_ERR_INVALID and
    the field's name, in the header's order."""
    from mbd_hip import _capi
    fn = getattr(lib, setter)
    rows = np.zeros((2, 3), np.float32)

    def refused(rec, field, handle):
        assert fn(handle, C.byref(rec)) == _capi.MBD_ERR_INVALID, field
        assert field in lib.mbd_last_error(), (field, lib.mbd_last_error())

    ok, keep = _record(_capi, 1, rows)
    refused(ok, b"plan" if "plan" in setter else b"sweep", None)
    stand_in = C.create_string_buffer(1 << 16)
    for ticks in (0, -1, 9, 1 << 20):
        refused(_record(_capi, ticks)[0], b"delay_ticks", stand_in)
    for r in range(4):
        rec, _ = _record(_capi, 2)
        rec.reserved[r] = 1
        refused(rec, b"reserved[%d]" % r, stand_in)
    # (delay_ticks is looked at first, reserved second)
    rec, _ = _record(_capi, 0)
    rec.reserved[0] = 1
    refused(rec, b"delay_ticks", stand_in)
    for n in (1, -1, 6):
        refused(_record(_capi, 2, None, n_rows=n)[0], b"rows0 is NULL", stand_in)
    for n in (0, -2):
        rec, keep = _record(_capi, 2, rows, n_rows=n)
        refused(rec, b"n_rows=%d" % n, stand_in)
    assert b"n_rows" in lib.mbd_last_error()


@pytest.mark.parametrize("peek", ["mbd_plan_peek_mpc_predicted", "mbd_sweep_peek_mpc_predicted"])
def test_peek_without_a_record_is_a_state_error_before_any_device_access(lib, peek):
    from mbd_hip import _capi
    fn = getattr(lib, peek)
    out = np.zeros(16, np.float32)
    assert fn(None, _capi.np_ptr(out)) == _capi.MBD_ERR_INVALID
    assert (b"plan" if "plan" in peek else b"sweep") in lib.mbd_last_error()
    stand_in = C.create_string_buffer(1 << 16)  # (zeroed: a handle that never had a record)
    assert fn(stand_in, _capi.np_ptr(out)) == _capi.MBD_ERR_STATE
    assert b"no delay record" in lib.mbd_last_error()
    assert not out.any()


def test_the_records_own_refusals_with_rows_to_look_at(lib):
    """mbd_debug_check_mpc_delay, the set calls' check for a handle of action_size 3: a non-finite row value is refused and
    named by row and column, after the fields in front of it; finite rows of either sign, zeros of either sign and large values
    pass."""
    from mbd_hip import _capi
    rows = np.random.default_rng(3).uniform(-1, 1, (4, 3)).astype(np.float32)
    rows[0, 0], rows[1, 1], rows[3, 2] = -0.0, 0.0, 3e38
    rec, keep = _record(_capi, 2, rows)
    assert _capi.debug_check_mpc_delay(rec, 3) == _capi.MBD_OK
    assert _capi.debug_check_mpc_delay(_record(_capi, 8)[0], 3) == _capi.MBD_OK
    for bad in (np.nan, np.inf, -np.inf):
        r = rows.copy()
        r[2, 1] = bad
        rec, keep = _record(_capi, 2, r)
        assert _capi.debug_check_mpc_delay(rec, 3) == _capi.MBD_ERR_INVALID
        assert b"rows0[2][1]" in lib.mbd_last_error(), lib.mbd_last_error()
        rec.delay_ticks = 9  # (the fields in front of the rows come first)
        assert _capi.debug_check_mpc_delay(rec, 3) == _capi.MBD_ERR_INVALID and b"delay_ticks" in lib.mbd_last_error()
    # the last element of the last row is looked at, and nothing behind it
    r = np.concatenate([rows, np.full((1, 3), np.nan, np.float32)])
    rec, keep = _record(_capi, 2, r, n_rows=4)
    assert _capi.debug_check_mpc_delay(rec, 3) == _capi.MBD_OK
    r[3, 2] = np.nan
    assert _capi.debug_check_mpc_delay(rec, 3) == _capi.MBD_ERR_INVALID and b"rows0[3][2]" in lib.mbd_last_error()
    for fields in ((0, None, None, b"delay_ticks"), (1, None, 2, b"rows0 is NULL"), (1, rows, 0, b"n_rows=0")):
        rec, keep = _record(_capi, fields[0], fields[1], n_rows=fields[2])
        assert _capi.debug_check_mpc_delay(rec, 3) == _capi.MBD_ERR_INVALID and fields[3] in lib.mbd_last_error()


def test_batch_arguments_share_one_delay():
    from mbd_hip.planners import mpc
    a = mpc.MpcArgs(env_name="hopper", Nsample=64, Hsample=20, Ndiffuse=6, n_ticks=3, warm_steps=2,
                    disable_recommended_params=True, not_render=True)
    assert a.delay_ticks == 0 and not mpc._has_delay(a) and mpc._delay_settings(a) == {}
    b = replace(a, delay_ticks=2)
    assert mpc._has_delay(b) and mpc._delay_settings(b) == dict(delay_ticks=2)
    mpc._check_batch([b, replace(b, seed=1, plant_mass=1.3)])
    with pytest.raises(ValueError, match="delay_ticks"):
        mpc._check_batch([b, replace(a, seed=1)])
    with pytest.raises(ValueError, match="delay_ticks"):
        mpc._check_batch([b, replace(b, seed=1, delay_ticks=1)])


# ---- the checker alone: hopper, N = 32, H = 12, Nd = 5, K = 2, E = 2, T = 4 ----------------------------------------------
N, H, ND, K, E, T = 32, 12, 5, 2, 2, 4


@pytest.fixture(scope="module")
def hopper(orc):
    oe = _oenv(orc, "hopper")
    rows0 = np.random.default_rng(7).uniform(-1, 1, (E, oe.Nu)).astype(np.float32)
    rows0[0, 1] = -0.0
    return oe, _reset(orc, oe, 1), orc.prng_key(4), rows0


@pytest.fixture(scope="module")
def delayed(hopper):
    """The D = 1 episode of T + 1 ticks from s_0 with a random committed block (computed once, shared, left unchanged)."""
    oe, s0, key, rows0 = hopper
    return mdc.episode(oe, s0, key, N, H, ND, 0.1, T + 1, K, E, 1, rows0=rows0)


def test_checker_d1_is_the_undelayed_episode_shifted_by_one_tick(hopper, delayed):
    """With D = 1 and no disturbance the prediction and the execution are the same rollout, so shat_t == s_{t+1}, and the
    delayed episode of T + 1 ticks from s_0 is the undelayed one of T ticks from s_1 with the same key, one tick later."""
    oe, s0, key, rows0 = hopper
    d = delayed
    assert np.array_equal(d["predicted"], d["states"][1:])
    assert d["actions"][:E].tobytes() == rows0.tobytes()  # (the signed zero included)
    u = mpc_checker.episode(oe, d["states"][1], key, N, H, ND, 0.1, T, K, E)
    assert np.array_equal(d["means"][:T], u["means"])
    assert np.array_equal(d["states"][1:], u["states"])
    assert np.array_equal(d["actions"][E:], u["actions"]) and np.array_equal(d["rewards"][E:], u["rewards"])
    # a record of a plant that is the model and disturbs nothing changes no bit
    same = mdc.episode(oe, s0, key, N, H, ND, 0.1, T + 1, K, E, 1, rows0=rows0, plant=oe, dkey=oe.orc.prng_key(9), kick_every=2)
    for k in _LOGS + ("predicted",):
        assert same[k].tobytes() == d[k].tobytes(), k


@pytest.mark.parametrize("D", [1, 3])
def test_checker_episodes_are_prefixes_of_longer_ones(hopper, delayed, D):
    oe, s0, key, rows0 = hopper
    r0 = rows0 if D == 1 else None
    long = delayed if D == 1 else mdc.episode(oe, s0, key, N, H, ND, 0.1, T + 1, K, E, D)
    short = mdc.episode(oe, s0, key, N, H, ND, 0.1, T, K, E, D, rows0=r0)
    for k in _LOGS + ("predicted",):
        assert np.array_equal(short[k], long[k][: len(short[k])]), k
    assert short["states"].shape[0] == T + 1 and short["predicted"].shape[0] == T
    if D == 3:  # zeros are executed for D ticks; tick t >= D executes tick t - D's plan
        assert not long["actions"][: D * E].any()
        for t in range(D, T + 1):
            assert np.array_equal(long["actions"][t * E:(t + 1) * E], long["means"][t - D][:E]), t
        # tick 0's mean is the cold plan from shat_0
        r, Ybar = oe.orc.split(key, 2, 1)[1], np.zeros((H, oe.Nu), np.float32)
        sched = oe.orc.schedule(1e-4, 1e-2, ND)
        for i in range(ND - 1, 0, -1):
            r, Ybar, _, _ = op.reverse_once(oe.orc, oe, long["predicted"][0], i, r, Ybar, sched, N, H, 0.1, 1)
        assert np.array_equal(Ybar, long["means"][0])


@pytest.mark.parametrize("D", [1, 2])
def test_checker_predicts_with_the_plans_env_not_the_plant(orc, hopper, D):
    """Under a plant of mass 1.3 the predicted state is not the state the plant reaches: shat_t != s_{t+D}, while it IS the
    plan's env's rollout of the queue — the rows executed in ticks t .. t+D-1 — from s_t.  A checker that predicted with the
    plant would give shat_t == s_{t+D}."""
    oe, s0, key, rows0 = hopper
    plant = _oenv(orc, "hopper", mass=1.3)
    ep = mdc.episode(oe, s0, key, N, H, ND, 0.1, T + D, K, E, D, plant=plant)
    for t in range(T):
        assert not np.array_equal(ep["predicted"][t], ep["states"][t + D]), t
        queue = ep["actions"][t * E:(t + D) * E]  # (no action noise: what was executed is what was committed)
        _, want = mpc_checker.execute(oe, ep["states"][t], queue)
        assert np.array_equal(ep["predicted"][t], want), t
        _, reached = mpc_checker.execute(plant, ep["states"][t], queue)
        assert np.array_equal(reached, ep["states"][t + D]), t
    # with action noise and kicks the queue keeps the undisturbed rows and the shift takes the undisturbed mean
    kw = dict(plant=plant, dkey=orc.prng_key(5), act_std=0.1, kick_std=0.3, kick_every=2)
    noisy = mdc.episode(oe, s0, key, N, H, ND, 0.1, T, K, E, D, **kw)
    assert np.array_equal(noisy["means"][0], ep["means"][0])  # (tick 0 plans from shat_0: the zeros' rollout from s_0)
    dk = kw["dkey"]
    for t in range(T):
        dk, eps = mpc_plant_checker.disturbances(orc, dk, E, oe.Nu, 1)
        clean = np.zeros((E, oe.Nu), np.float32) if t < D else noisy["means"][t - D][:E]
        assert np.array_equal(noisy["actions"][t * E:(t + 1) * E], mpc_plant_checker.rows_of(clean, E, eps, 0.1)), t
