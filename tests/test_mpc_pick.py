"""The pick record without a GPU (include/mbd_hip.h mbd_mpc_pick, DESIGN.md section 1 "N15 pick"): the checker
(tests/mpc_pick_checker.py) held to its own invariants, and the refusals the C ABI decides on the host."""
import ctypes as C
import functools

import numpy as np
import pytest

import mpc_checker
import mpc_pick_checker as pc
from conftest import load_model

NAMES = ("mbd_plan_set_mpc_pick", "mbd_plan_peek_mpc_pick", "mbd_sweep_set_mpc_pick", "mbd_sweep_peek_mpc_pick")
# the small episode in which all three choices occur (hopper, prng impl 1)
ALL3 = dict(N=8, H=20, Nd=6, temp=2.0, T=12, K=1, E=1)


def _oenv_cpu(orc, name):
    from oracle.planner import OracleEnv
    m = load_model(name)
    return OracleEnv(orc, name, m.to_struct(), init_q=m.init_q)


def all3_inputs(orc):
    """(state0, episode key) of the all-three-choices episode: key = prng_key(0), keys = split(key, 2), state0 = reset(keys[1])."""
    oe = _oenv_cpu(orc, "hopper")
    keys = orc.split(orc.prng_key(0), 2, 1)
    return oe, oe.reset(keys[1], 1), keys[0]


@functools.lru_cache(maxsize=None)
def _all3(orc, mask):
    oe, s0, key = all3_inputs(orc)
    return pc.episode(oe, s0, key, mask=mask, **ALL3)


def test_best_index_and_choice_rules():
    nan, inf = np.float32("nan"), np.float32("inf")
    assert pc.best_index([nan, -inf, inf]) == -1
    assert pc.best_index([nan, -3.0, inf, -1.0, -1.0]) == 3
    assert pc.best_index([-0.0, 0.0]) == 0 and pc.best_index([0.0, -0.0]) == 0
    assert pc.best_index([-2.0]) == 0
    # ties keep the earlier slot; disabled, absent and non-finite slots never take over; nothing eligible: 0
    assert pc.choose(np.float32([1, 1, 1]), 7, (True, True, True)) == 0
    assert pc.choose(np.float32([1, 2, 3]), 7, (True, True, True)) == 2
    assert pc.choose(np.float32([1, 2, 3]), 3, (True, True, True)) == 1
    assert pc.choose(np.float32([1, 2, 3]), 7, (True, False, False)) == 0
    assert pc.choose(np.float32([nan, 2, inf]), 7, (True, True, True)) == 1
    assert pc.choose(np.float32([nan, nan, nan]), 7, (True, True, True)) == 0
    assert pc.choose(np.float32([1, 5, 3]), 5, (True, True, True)) == 2
    assert pc.choose(np.float32([9, 5, 3]), 6, (True, True, True)) == 1


def test_mask_mean_is_the_episode_without_a_record(orc):
    """Mask MEAN equals mpc_checker.episode by bytes, and logs the value of every executed plan."""
    oe, s0, key = all3_inputs(orc)
    kw = dict(ALL3, T=4)
    ref = mpc_checker.episode(oe, s0, key, kw["N"], kw["H"], kw["Nd"], kw["temp"], kw["T"], kw["K"], kw["E"], impl=1)
    got = pc.episode(oe, s0, key, mask=pc.MEAN, **kw)
    for k in ("actions", "rewards", "states", "means"):
        assert np.asarray(ref[k], np.float32).tobytes() == np.asarray(got[k], np.float32).tobytes(), k
    assert (got["choice"] == 0).all() and np.isfinite(got["rets"][:, 0]).all()
    none = pc.episode(oe, s0, key, mask=None, **kw)
    assert none["means"].tobytes() == got["means"].tobytes() and "choice" not in none


def test_best_return_is_the_maximum_finite_reward_by_bytes(orc):
    ep = _all3(orc, 7)
    for t in range(ALL3["T"]):
        r = ep["last_rews"][t]
        assert ep["best"][t] == pc.best_index(r) >= 0
        assert ep["rets"][t, 2].tobytes() == r[np.isfinite(r)].max().tobytes(), t


def test_slot1_is_the_shifted_previous_pick(orc):
    ep = _all3(orc, 7)
    assert ep["rets"][0, 1].tobytes() == ep["rets"][0, 0].tobytes()  # (tick 0 is cold: the absent slot holds M_0)
    for t in range(1, ALL3["T"]):
        assert np.array_equal(ep["slot1"][t], mpc_checker.shift(ep["means"][t - 1], ALL3["E"])), t
    assert ep["choice"][0] != 1


def test_all_three_choices_occur_in_one_small_episode(orc):
    ep = _all3(orc, 7)
    assert set(ep["choice"].tolist()) == {0, 1, 2}, ep["choice"]
    # the picked plan's return is the largest finite one among the present slots, and never below the mean's
    for t in range(ALL3["T"]):
        c = ep["choice"][t]
        assert ep["rets"][t, c] >= ep["rets"][t, 0]
    # and the masks restrict it
    assert set(_all3(orc, 3)["choice"].tolist()) <= {0, 1} and set(_all3(orc, 5)["choice"].tolist()) <= {0, 2}


def test_entry_points_are_exported_and_refuse_on_the_host(lib):
    """NULL handles, and on a stand-in handle with an open session the session refusal, before any device access."""
    from mbd_hip import _capi
    for name in NAMES:
        assert name in _capi.EXPORTS and hasattr(lib, name), name
    lib.mbd_last_error.restype = C.c_char_p
    rec = _capi.pick_record()
    assert rec.candidates == 7 and C.sizeof(rec) == 32
    assert lib.mbd_plan_set_mpc_pick(None, C.byref(rec)) == _capi.MBD_ERR_INVALID and b"plan" in lib.mbd_last_error()
    assert lib.mbd_sweep_set_mpc_pick(None, C.byref(rec)) == _capi.MBD_ERR_INVALID and b"sweep" in lib.mbd_last_error()
    assert lib.mbd_plan_peek_mpc_pick(None, None, None, None, 0, None) == _capi.MBD_ERR_INVALID
    assert lib.mbd_sweep_peek_mpc_pick(None, 0, None, None, None, 0, None) == _capi.MBD_ERR_INVALID
    lib.mbd_debug_pick_best.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    buf = np.zeros(4, np.float32)
    out = np.zeros(1, np.int32)
    assert lib.mbd_debug_pick_best(None, 1, 4, out.ctypes.data) == _capi.MBD_ERR_INVALID
    assert lib.mbd_debug_pick_best(buf.ctypes.data, 0, 4, out.ctypes.data) == _capi.MBD_ERR_INVALID
    assert lib.mbd_debug_pick_best(buf.ctypes.data, 1, 0, out.ctypes.data) == _capi.MBD_ERR_INVALID
    if _capi.device_count() == 0:
        assert lib.mbd_debug_pick_best(buf.ctypes.data, 1, 4, out.ctypes.data) == _capi.MBD_ERR_NO_DEVICE


@pytest.mark.parametrize("candidates,reserved,field", [(0, 0, b"candidates"), (8, 0, b"candidates"), (15, 0, b"candidates"),
                                                       (-1, 0, b"candidates"), (7, 1, b"reserved")])
def test_record_refusals_come_before_the_handle_is_touched(lib, candidates, reserved, field):
    """The record's own refusals name the field; the stand-in handle is zeroed memory (no session, no device behind it), which the
    call must not reach past its session flag."""
    from mbd_hip import _capi
    lib.mbd_last_error.restype = C.c_char_p
    stand_in = C.create_string_buffer(1 << 16)
    rec = _capi.MpcPick()
    rec.candidates = candidates
    rec.reserved[3] = reserved
    assert lib.mbd_plan_set_mpc_pick(stand_in, C.byref(rec)) == _capi.MBD_ERR_INVALID
    assert field in lib.mbd_last_error()
    assert lib.mbd_sweep_set_mpc_pick(stand_in, C.byref(rec)) == _capi.MBD_ERR_INVALID
    assert field in lib.mbd_last_error()


# ---- the checker under the other records ----------------------------------------------------------------------------------------

def divergence_episode(orc, mask=7, impl=1):
    """The closed loop of tests/weighting_combined_inputs.py on the hopper whose actuator 0 has a gear of 1e30 — planned and executed
    on it under the noise shape that lets some candidates of every launch diverge — under rejection and a pick record."""
    import functools

    import weighting_checker as wc
    import weighting_combined_inputs as wci
    import weighting_inputs as wi
    from noise_shape_checker import shaped_env
    oe = wci.oenv(orc, wci.models()[1])
    c = wci.LOOP
    s0 = wci.start(orc, wci.models()[1], c["state_seed"], impl)
    return pc.episode(shaped_env(oe, wci.shape(oe.Nu)), s0, orc.prng_key(c["key_seed"]), c["N"], wci.H, c["Nd"], wci.TEMP, wci.T,
                      wci.K, wci.E, mask, impl=impl, reverse_once=functools.partial(wc.reverse_once, rec=wi.REJECT))


def test_checker_under_rejection_never_picks_a_diverged_candidate(orc):
    """Candidates really diverge in every tick's last step; ``best`` is a finite one, its return the largest finite reward by bytes,
    and the episode stays finite."""
    import weighting_combined_inputs as wci
    ep = divergence_episode(orc)
    N = wci.LOOP["N"]
    for t in range(wci.T):
        r = ep["last_rews"][t]
        fin = np.isfinite(r)
        assert 0 < fin.sum() < N, (t, int(fin.sum()))
        assert fin[ep["best"][t]] and ep["rets"][t, 2].tobytes() == r[fin].max().tobytes(), t
    assert np.isfinite(ep["means"]).all() and np.isfinite(ep["states"]).all() and np.isfinite(ep["rets"]).all()


def test_checker_delay_evaluates_from_the_predicted_state(orc):
    """D = 1: the rows executed in tick t are P_{t-1}[:E] (zeros in tick 0), the pick's returns are taken from the predicted state
    (ret[2] is the last step's best reward, which was rolled out from there), and slot 1 is still the shifted previous pick."""
    oe, s0, key = all3_inputs(orc)
    kw = dict(ALL3, T=5)
    ep = pc.episode(oe, s0, key, mask=7, D=1, **kw)
    assert not ep["actions"][0].any() and np.array_equal(ep["actions"][1:], ep["means"][:-1, 0])
    assert not np.array_equal(ep["predicted"][1], ep["states"][1])
    for t in range(kw["T"]):
        r = ep["last_rews"][t]
        assert ep["rets"][t, 2].tobytes() == r[np.isfinite(r)].max().tobytes(), t
    for t in range(1, kw["T"]):
        assert np.array_equal(ep["slot1"][t], mpc_checker.shift(ep["means"][t - 1], 1)), t


@pytest.mark.parametrize("method", ["mppi", "cma-es", "cem"])
def test_checker_path_integral_slot2_is_a_materialised_row(orc, method):
    """Mask MEAN is mpc_pi_checker.episode by bytes; under the full mask ret[2] is the last refinement's largest reward by bytes."""
    import mpc_pi_checker as pic
    oe, s0, key = all3_inputs(orc)
    N, H, Nd, temp, T, K, E, sig = 16, 12, 5, 0.5, 4, 2, 1, (1.0, 0.5, 0.0)
    ref = pic.episode(oe, s0, key, N, H, Nd, temp, T, K, E, method, *sig)
    got = pc.episode(oe, s0, key, N, H, Nd, temp, T, K, E, pc.MEAN, method=method, sigma=sig)
    for k in ("actions", "rewards", "states", "means"):
        assert np.asarray(ref[k], np.float32).tobytes() == np.asarray(got[k], np.float32).tobytes(), k
    full = pc.episode(oe, s0, key, N, H, Nd, temp, T, K, E, 7, method=method, sigma=sig)
    for t in range(T):
        assert full["rets"][t, 2].tobytes() == full["last_rews"][t].max().tobytes(), t
    assert (full["choice"] != 0).any()
