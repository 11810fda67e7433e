"""Path-integral episodes (include/mbd_hip.h mbd_mpc_sigma; DESIGN.md section 1 "N12 path-integral episodes") without a GPU: the
four entry points are exported and refuse NULL before any device access; the record's own refusals; the checker's restatement
(tests/mpc_pi_checker.py) keeps the contract's consequences — tick 0 under sigma_cold = 1 is the open-loop refinement loop,
episodes are prefixes of longer ones, the record {1, 1, 0} is the reference's update() per tick —; the boundary function the
kernel calls, run on the host, against the checker's numpy; and the inputs of tests/test_gpu_mpc_pi.py can tell their settings
apart and reach every branch of the clamp."""
import ctypes as C

import numpy as np
import pytest

import mpc_checker
import mpc_pi_cases as cases
import mpc_pi_checker as pic
from oracle import planner as op

NAMES = ("mbd_plan_set_mpc_sigma", "mbd_plan_peek_mpc_sigma", "mbd_sweep_set_mpc_sigma", "mbd_sweep_peek_mpc_sigma")


def test_the_four_entry_points_are_exported_and_refuse_null_before_any_device_access(lib):
    from mbd_hip import _capi
    for name in NAMES:
        assert name in _capi.EXPORTS and hasattr(lib, name), name
    rec = _capi.MpcSigma(sigma_cold=1.0, sigma_warm=1.0, gain=0.0)
    out = (C.c_float * 4)()
    for call, what in ((lambda: lib.mbd_plan_set_mpc_sigma(None, C.byref(rec)), b"plan"),
                       (lambda: lib.mbd_plan_peek_mpc_sigma(None, out), b"plan"),
                       (lambda: lib.mbd_sweep_set_mpc_sigma(None, C.byref(rec)), b"sweep"),
                       (lambda: lib.mbd_sweep_peek_mpc_sigma(None, 0, out), b"sweep")):
        assert call() == _capi.MBD_ERR_INVALID
        assert what in lib.mbd_last_error() and b"NULL" in lib.mbd_last_error()


def test_the_records_own_refusals_name_the_field(lib):
    from mbd_hip import _capi

    def check(method, cold=1.0, warm=1.0, gain=0.0, reserved=None):
        rec = _capi.MpcSigma(sigma_cold=cold, sigma_warm=warm, gain=gain)
        if reserved is not None:
            rec.reserved[reserved] = 1
        return _capi.debug_check_mpc_sigma(rec, method), lib.mbd_last_error()
    for method in (1, 2, 3):
        assert check(method)[0] == _capi.MBD_OK
        assert check(method, 0.7, 0.25)[0] == _capi.MBD_OK and check(method, 0.25, 0.7)[0] == _capi.MBD_OK
        for bad in (0.0, -1.0, np.inf, np.nan):
            for field in ("cold", "warm"):
                rc, msg = check(method, **{field: bad})
                assert rc == _capi.MBD_ERR_INVALID and b"sigma_" + field.encode() in msg, (method, field, bad, msg)
        for bad in (-0.5, np.inf, np.nan):
            rc, msg = check(method, gain=bad)
            assert rc == _capi.MBD_ERR_INVALID and b"gain" in msg, (method, bad, msg)
        rc, msg = check(method, reserved=4)
        assert rc == _capi.MBD_ERR_INVALID and b"reserved" in msg
    assert check(2, 0.6, 0.3, 100.0)[0] == _capi.MBD_OK and check(2, 0.5, 0.5, 2.0)[0] == _capi.MBD_OK
    for method in (1, 3):  # sigma never changes within a tick of mppi or cem
        rc, msg = check(method, 0.6, 0.3, 100.0)
        assert rc == _capi.MBD_ERR_INVALID and b"gain" in msg and b"update_method" in msg
    rc, msg = check(2, 0.3, 0.6, 2.0)
    assert rc == _capi.MBD_ERR_INVALID and b"sigma_warm" in msg and b"sigma_cold" in msg


@pytest.mark.parametrize("method", cases.METHODS)
def test_checker_tick0_under_sigma_cold_1_is_the_open_loop_refinement_loop(method):
    """oracle.planner.run_path_integral's loop (path_integral.py:111-127), restated call for call, from k_0 = split(key)[1]:
    tick 0's mean and sigma, bit for bit; a warm sigma of its own changes nothing in tick 0."""
    oe, orc = cases.oenv("hopper"), cases._orc()
    N = cases.N_OF["hopper"]
    s0, key = cases.start("hopper")
    r, mu, sigma = orc.split(key, 2, 1)[1], np.zeros((cases.H, oe.Nu), np.float32), np.float32(1.0)
    for _ in range(cases.ND - 1):
        keys = orc.split(r, 2, 1)
        r, ks = keys[0], keys[1]
        Y0s = orc.sample(ks, 1, N, cases.H, oe.Nu, 0, N, float(sigma), mu)
        rews = op.mean_h(orc, np.ascontiguousarray(oe.rollout(s0, Y0s)))
        mu, sigma, _, _ = orc.pi_update(op.PI_METHODS[method], rews, Y0s, mu, float(sigma), cases.TEMP)
    for rec in (cases.PLAIN, (1.0, 0.25, 0.0)):
        ep = pic.episode(oe, s0, key, N, cases.H, cases.ND, cases.TEMP, 2, cases.K, 1, method, *rec)
        assert np.array_equal(ep["means"][0], mu)
        assert ep["sigmas"][0, 0] == np.float32(1.0) and ep["sigmas"][0, 1] == np.float32(sigma)
        assert ep["sigmas"][1, 0] == np.float32(rec[1])
    assert (np.float32(sigma) != 1.0) == (method == "cma-es")


@pytest.mark.parametrize("name,method,rec", [("hopper", "mppi", cases.RESET), ("hopper", "cma-es", cases.CARRY),
                                             ("hopper", "cem", cases.PLAIN), ("car2d", "cma-es", cases.CARRY)])
def test_checker_episode_is_a_prefix_of_a_longer_one(name, method, rec):
    short = cases.episode(name, method, 1, rec, T_=3)
    long = cases.episode(name, method, 1, rec)
    for k, v in short.items():
        assert v.tobytes() == long[k][: len(v)].tobytes(), k  # (by bytes: car2d's carry is NaN from tick 0 on)
    assert len(long["means"]) == cases.T and short["sigmas"].shape == (3, 2)


@pytest.mark.parametrize("method", cases.METHODS)
def test_the_plain_record_is_the_references_update_per_tick(method):
    """Record {1, 1, 0}: every tick starts at sigma = 1 from the shifted mean and runs path_integral.py:113-126 K times —
    written out by hand here, against the checker's episode."""
    oe, orc = cases.oenv("hopper"), cases._orc()
    N, E = cases.N_OF["hopper"], 2
    s, rng = cases.start("hopper")
    ep = cases.episode("hopper", method, E, cases.PLAIN)
    mu, n_it = np.zeros((cases.H, oe.Nu), np.float32), cases.ND - 1
    for t in range(cases.T):
        rng, r = orc.split(rng, 2, 1)
        sigma = 1.0
        for _ in range(n_it):
            r, ks = orc.split(r, 2, 1)
            Y0s = orc.sample(ks, 1, N, cases.H, oe.Nu, 0, N, sigma, mu)
            rews = op.mean_h(orc, np.ascontiguousarray(oe.rollout(s, Y0s)))
            mu, sigma, _, _ = orc.pi_update(op.PI_METHODS[method], rews, Y0s, mu, sigma, cases.TEMP)
        assert np.array_equal(ep["means"][t], mu), t
        assert ep["sigmas"][t, 0] == 1.0 and ep["sigmas"][t, 1] == np.float32(sigma)
        rew, s = mpc_checker.execute(oe, s, mu[:E])
        assert np.array_equal(ep["rewards"][t * E:(t + 1) * E], rew) and np.array_equal(ep["states"][t + 1], s)
        assert np.array_equal(ep["actions"][t * E:(t + 1) * E], mu[:E])
        mu, n_it = mpc_checker.shift(mu, E), cases.K


def test_the_kernels_boundary_function_on_the_host_is_the_checkers(lib):
    """mpc_pi_next_sigma — the text mpc_pi_sigma_kernel calls, compiled for the host — against the checker's three float32
    operations, by bits: NaN (both signs), infinities, zeros, the floor 1e-3 of cma-es, values either side of both clamps and on
    them, products that round, overflow and underflow; gain = 0 returns sigma_warm whatever comes in."""
    from mbd_hip import _capi
    f = np.float32
    nan_neg = np.array([0xFFC00000], np.uint32).view(f)[0]
    ends = [f(np.nan), nan_neg, f(np.inf), f(-np.inf), f(0.0), f(-0.0), f(1e-3), f(1e-45), f(1e-38), f(3e38), f(1.0), f(0.6), f(0.3)]
    for cold, warm, gain in ((0.6, 0.3, 100.0), (0.6, 0.3, 0.0), (1.0, 1.0, 0.0), (0.7, 0.25, 0.0), (0.25, 0.7, 0.0),
                             (0.5, 0.5, 2.0), (1.0, 1e-3, 1e-3), (3e38, 1e-38, 3e38), (1.0, 0.1, 1.0 / 3.0)):
        g, lo, hi = f(gain), f(warm), f(cold)
        grid = list(ends)
        if gain > 0:  # sigma_end whose product lands one ulp either side of each clamp, and on it
            for edge in (lo, hi):
                x = f(edge / g)
                for _ in range(3):
                    x = np.nextafter(x, f(-np.inf))
                for _ in range(7):
                    grid.append(f(x))
                    x = np.nextafter(x, f(np.inf))
        grid += list(np.linspace(0.0, 2.0 * cold / max(gain, 1e-3), 97).astype(f))
        grid = np.array(grid, f)
        got = _capi.debug_mpc_sigma_next(grid, cold, warm, gain)
        want = np.array([pic.next_sigma(x, cold, warm, gain) for x in grid], f)
        assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist(), (cold, warm, gain)
        nan_in = np.isnan(grid)
        if gain == 0:
            assert np.all(got == lo)
        else:
            assert np.isnan(got[nan_in]).all() and not np.isnan(got[~nan_in]).any()  # a NaN sigma stays NaN, nothing else becomes one
            assert np.all((got[~nan_in] >= lo) & (got[~nan_in] <= hi))
            assert (got == lo).any() and (got == hi).any() and ((got > lo) & (got < hi)).any() == (lo < hi)


@pytest.mark.parametrize("name", ["hopper", "humanoidrun"])
@pytest.mark.parametrize("E", [1, 2])
def test_the_gpu_cases_can_tell_their_records_apart(name, E):
    """What tests/test_gpu_mpc_pi.py runs, on the checker: the means under {1, 1, 0} differ from those under the case's record from
    tick 1 on (tick 0 under another sigma_cold too), so a library that ignored the record could not pass."""
    for method in cases.METHODS:
        plain = cases.episode(name, method, E, cases.PLAIN)
        recs = (cases.RESET,) + ((cases.CARRY,) if method == "cma-es" else ())
        for rec in recs:
            ep = cases.episode(name, method, E, rec)
            for t in range(cases.T):
                assert not np.array_equal(ep["means"][t], plain["means"][t]), (method, rec, t)
            assert np.isfinite(ep["means"]).all() and np.isfinite(ep["states"]).all() and np.isfinite(ep["sigmas"]).all()
        if method == "cma-es":
            a, b = cases.episode(name, method, E, cases.RESET), cases.episode(name, method, E, cases.CARRY)
            assert not np.array_equal(a["means"][0], b["means"][0]) and not np.array_equal(a["sigmas"], b["sigmas"])


def _branches(sigmas, rec):
    """Which branch of the clamp every boundary of an episode took: 'warm', 'range' or 'cold'."""
    cold, warm, gain = (np.float32(v) for v in rec)
    out = []
    for t in range(len(sigmas) - 1):
        x = np.float32(gain * sigmas[t, 1])
        out.append("warm" if x < warm else "cold" if x > cold else "range")
        assert sigmas[t + 1, 0] == pic.next_sigma(sigmas[t, 1], *rec)
    return out


@pytest.mark.parametrize("name,third", [("hopper", 0.549), ("humanoidrun", 0.504)])
def test_the_carry_case_reaches_all_three_branches_of_the_clamp(name, third):
    """cma-es under {0.6, 0.3, 100}: from reset(split(prng_key(5))[1]) with the episode key prng_key(6), boundaries 0, 1, 2 take
    the warm clamp, the product itself and the cold clamp — sigma starts 0.6, 0.3, 0.549 (humanoidrun 0.504), 0.6 — and all
    three methods stay finite over 7 ticks.  And for the inputs the GPU tests use (tests/mpc_pi_cases.py), E = 1 and 2: all
    three branches within their 5 ticks."""
    oe, orc = cases.oenv(name), cases._orc()
    s0 = oe.reset(orc.split(orc.prng_key(5), 2, 1)[1], 1)
    key = orc.prng_key(6)
    args = (oe, s0, key, cases.N_OF[name], cases.H, cases.ND, cases.TEMP, 7, cases.K, 1)
    ep = pic.episode(*args, "cma-es", *cases.CARRY)
    assert _branches(ep["sigmas"], cases.CARRY)[:3] == ["warm", "range", "cold"]
    starts = ep["sigmas"][:4, 0]
    assert starts[0] == np.float32(0.6) and starts[1] == np.float32(0.3) and starts[3] == np.float32(0.6)
    assert abs(float(starts[2]) - third) < 5e-4, starts[2]
    for method, rec in (("cma-es", cases.CARRY), ("mppi", (0.6, 0.3, 0.0)), ("cem", (0.6, 0.3, 0.0))):
        e = ep if method == "cma-es" else pic.episode(*args, method, *rec)
        for k, v in e.items():
            assert np.isfinite(v).all(), (method, k)
    for E in (1, 2):
        got = _branches(cases.episode(name, "cma-es", E, cases.CARRY)["sigmas"], cases.CARRY)
        assert {"warm", "range", "cold"} <= set(got), (E, got)


@pytest.mark.parametrize("method", ["mppi", "cma-es"])
def test_car2d_is_the_nan_case(method):
    """car2d's rewards tie at N = 64 and path_integral.py:123 has no zero-std guard: the weights, the mean and — for cma-es —
    sigma go NaN in tick 0.  Under the carry record the NaN sigma stays NaN across every boundary (neither clamp catches it)."""
    rec = cases.CARRY if method == "cma-es" else cases.RESET
    ep = cases.episode("car2d", method, 1, rec)
    assert np.isnan(ep["means"]).any()
    if method == "cma-es":
        assert ep["sigmas"][0, 0] == np.float32(0.6) and np.isnan(ep["sigmas"].reshape(-1)[1:]).all()
    else:
        assert np.array_equal(ep["sigmas"][:, 0], ep["sigmas"][:, 1])  # mppi leaves sigma alone


def test_session_restatement_is_the_episode():
    """tests/mpc_pi_checker.Session fed the episode's states returns its means and sigmas; reset_mean gives a cold tick."""
    name, method = "hopper", "cma-es"
    ep = cases.episode(name, method, 1, cases.CARRY)
    _, key = cases.start(name)
    ss = pic.Session(cases.oenv(name), key, cases.N_OF[name], cases.H, cases.ND, cases.TEMP, cases.K, 1, method, *cases.CARRY)
    for t in range(3):
        out = ss.tick(ep["states"][t])
        assert np.array_equal(out["mean"], ep["means"][t]) and tuple(out["sigma"]) == tuple(ep["sigmas"][t])
        assert ss.sigma == ep["sigmas"][t + 1, 0]
    ss.reset_mean()
    assert ss.sigma == np.float32(0.6) and ss.n_it == cases.ND - 1
