"""Path-integral episodes on the GPU (include/mbd_hip.h mbd_mpc_sigma; DESIGN.md section 1 "N12 path-integral episodes").  Every
comparison is np.array_equal, or by bytes where NaN is expected.  Sizes: N = 64 (humanoidrun 128), H = 20, Ndiffuse = 6, K = 2,
T = 5 (tests/mpc_pi_cases.py, whose checker episodes are computed once and shared).

  episodes        means, actions, rewards, states and sigmas against tests/mpc_pi_checker.py: hopper and humanoidrun x mppi,
                  cma-es, cem x E in {1, 2} under the records {1, 1, 0} and {0.7, 0.25, 0}; cma-es also under the carry record
                  {0.6, 0.3, 100}, which takes all three branches of the clamp (tests/test_mpc_pi.py holds that for these inputs)
  definition      tick 0 under sigma_cold = 1 is Plan.run(k_0); prefix; set, clear, set
  the NaN case    car2d cma-es: sigma goes NaN in tick 0 and stays NaN through the carry
  records         a plant (mismatch, action noise, a kick every 2nd tick), a delay D in {1, 2} with given rows0, a warm noise
                  shape with a 4-knot basis
  sweeps          P in {1, 3} equal the single plans' episodes; per-episode plants and a delay
  sessions        fed the episode's states: its means and rows; get_sigma between ticks; reset_mean
  refusals        what only a real handle decides
  command line    --update_method mppi --sigma_warm 0.25 equals the API call; --n_episodes 3 equals three single runs; --online;
                  examples/mbd_control.c --mppi
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mpc_pi_cases as cases
import mpc_pi_checker as pic
import noise_basis_checker as nbc
from conftest import ROOT
from test_gpu_noise_shape import _args, _env, _oenv, _state, shape_of

pytestmark = pytest.mark.gpu

_LOGS = ("means", "actions", "rewards", "states", "sigmas")
H, ND, K, T = cases.H, cases.ND, cases.K, cases.T
METHOD = {"mppi": 1, "cma-es": 2, "cem": 3}
PLANT = dict(act_std=0.1, kick_std=0.3, kick_every=2)
MISMATCH = dict(mass=1.3, friction=0.5, gear=0.8)


@pytest.fixture(scope="module")
def gpu(lib):
    from mbd_hip import _capi
    from mbd_hip.envs.base import prng_impl
    if _capi.device_count() < 1:
        pytest.fail("tests/test_gpu_mpc_pi.py needs a GPU")
    assert prng_impl() == 1  # (the layout tests/mpc_pi_cases.py computes its episodes under)
    return _capi


def _equal(a, b, what="", logs=_LOGS):
    for k in logs:
        x, y = np.asarray(a[k], np.float32), np.asarray(b[k], np.float32)
        assert x.size == y.size and np.array_equal(x.reshape(y.shape), y), f"{what}: {k} differ"


def _start(name):
    """The case's start state as the library's State and the episode key: the library's reset is held to the checker's."""
    from mbd_hip.planners.mpc import _reset_and_key
    env = _env(name)
    st, key = _reset_and_key(env, cases.SEED)
    s0, key0 = cases.start(name)
    assert np.array_equal(_state(env, st), s0) and np.array_equal(np.asarray(key, np.uint32), key0)
    return env, st, key0


def _plan(env, name, method, st, rec=None):
    from mbd_hip.planners.mbd_planner import Plan
    plan = Plan(env, _args(name, cases.N_OF[name], H, ND), update_method=METHOD[method])
    plan.set_state0(st)
    if rec is not None:
        plan.set_mpc_sigma(*rec)
    return plan


def _sweep(env, name, method, sts, rec=None):
    from mbd_hip.planners.mbd_planner import Sweep
    sw = Sweep(env, _args(name, cases.N_OF[name], H, ND), len(sts), update_method=METHOD[method])
    for k, st in enumerate(sts):
        sw.set_state0(k, st)
    if rec is not None:
        sw.set_mpc_sigma(*rec)
    return sw


# ---- episodes against the checker -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("E", [1, 2])
@pytest.mark.parametrize("method", cases.METHODS)
@pytest.mark.parametrize("name", ["hopper", "humanoidrun"])
def test_episode_matches_the_checker(gpu, name, method, E):
    env, st, key = _start(name)
    plan = _plan(env, name, method, st)
    for rec in (cases.PLAIN, cases.RESET) + ((cases.CARRY,) if method == "cma-es" else ()):
        plan.set_mpc_sigma(*rec)
        ep = plan.run_mpc(key, T, K, E)
        ref = cases.episode(name, method, E, rec)
        _equal(ep, ref, f"{name} {method} E={E} {rec}")
        assert ep["sigmas"].shape == (T, 2) and np.isfinite(ref["states"]).all()
        assert plan.get_sigma() == pic.next_sigma(ref["sigmas"][-1, 1], *rec)  # (what a tick T would start from)
    plan.close()


@pytest.mark.parametrize("method", cases.METHODS)
def test_tick_0_is_plan_run_and_episodes_are_prefixes(gpu, method):
    """With sigma_cold = 1: tick 0's mean and sigma are mbd_plan_run(k_0)'s.  An episode of 3 ticks is a prefix of one of 5 and
    that of one of 6 (the logs grow).  Set, clear, set: the refusal comes back and goes; run() is untouched by all of it."""
    name = "hopper"
    env, st, key = _start(name)
    plan = _plan(env, name, method, st)
    k0 = gpu.prng_split(key, 2, plan.cfg.prng_impl)[1]
    mu0, rm0, rf0, _ = plan.run(k0)
    sigma0 = np.float32(plan.get_sigma())
    rec = (1.0, 0.25, 0.0)
    plan.set_mpc_sigma(*rec)
    mid = plan.run_mpc(key, T, K, 1)
    assert np.array_equal(mid["means"][0], mu0[-1]) and mid["sigmas"][0, 0] == 1.0 and mid["sigmas"][0, 1] == sigma0
    short, long = plan.run_mpc(key, 3, K, 1), plan.run_mpc(key, T + 1, K, 1)
    for k in _LOGS:
        assert np.array_equal(short[k], mid[k][: len(short[k])]) and np.array_equal(mid[k], long[k][: len(mid[k])]), k
    plan.clear_mpc_sigma()
    with pytest.raises(gpu.MbdError, match="update_method") as e:
        plan.run_mpc(key, T, K, 1)
    assert e.value.code == gpu.MBD_ERR_UNSUPPORTED and "set_mpc_sigma" in str(e.value)
    plan.set_mpc_sigma(*rec)
    _equal(plan.run_mpc(key, T, K, 1), mid, "set, clear, set")
    mu1, rm1, rf1, _ = plan.run(k0)
    assert np.array_equal(mu1, mu0) and np.array_equal(rm1, rm0) and np.float32(rf1) == np.float32(rf0)
    plan.close()


def test_car2d_cma_es_sigma_goes_nan_and_stays_nan_through_the_carry(gpu):
    """car2d's rewards tie and path_integral.py:123 has no zero-std guard: sigma is NaN from tick 0's first update on, and
    neither clamp of the carry catches it.  By bytes: the sigmas against the checker's, and every log of an episode of 3 ticks
    against the first 3 ticks of one of 5.  The means against the checker's with a NaN equal to a NaN.  (Rewards and states are
    not held to the checker here: what car2d's rollout does with a NaN action — the kernel's clip keeps a bound, the checker's
    propagates it — is the rollout's business and older than episodes.)"""
    name, method, rec = "car2d", "cma-es", cases.CARRY
    env, st, key = _start(name)
    plan = _plan(env, name, method, st, rec)
    ep, short = plan.run_mpc(key, T, K, 1), plan.run_mpc(key, 3, K, 1)
    plan.close()
    ref = cases.episode(name, method, 1, rec)
    sig = ep["sigmas"].reshape(-1)
    print("car2d cma-es sigmas", ep["sigmas"].view(np.uint32).tolist(), "checker", ref["sigmas"].view(np.uint32).tolist())
    assert sig[0] == np.float32(0.6) and np.isnan(sig[1:]).all()
    assert ep["sigmas"].tobytes() == ref["sigmas"].tobytes()
    for k in _LOGS:
        assert short[k].tobytes() == ep[k][: len(short[k])].tobytes(), k
    assert np.isnan(ref["means"]).all() and np.array_equal(ep["means"], ref["means"], equal_nan=True)


# ---- records ------------------------------------------------------------------------------------------------------------------

def _rows0(D, E, Nu, seed=3):
    r = np.random.default_rng(seed).uniform(-1, 1, (D * E, Nu)).astype(np.float32)
    r[0, 0] = -0.0
    return r


@pytest.mark.parametrize("method,rec", [("mppi", cases.RESET), ("cma-es", cases.CARRY), ("cem", cases.RESET)])
@pytest.mark.parametrize("D", [0, 1, 2])
def test_plant_and_delay_records_compose(gpu, orc, method, rec, D):
    """A plant of mass 1.3, friction 0.5, gear 0.8 with action noise and a kick every 2nd tick (ticks 1 and 3 go through the
    boundary's kick variant), alone (D = 0) and under a delay record with given committed rows."""
    from mbd_hip.envs.base import RigidBodyEnv
    name, E = "hopper", 1
    env, st, key = _start(name)
    dkey = gpu.prng_key(11)
    plant = RigidBodyEnv(name, model=env.sys.scaled(**MISMATCH))
    plan = _plan(env, name, method, st, rec)
    plan.set_mpc_plant(env=plant, key=dkey, **PLANT)
    rows0 = _rows0(D, E, env.action_size) if D else None
    if D:
        plan.set_mpc_delay(D, rows0)
    ep = plan.run_mpc(key, T, K, E)
    plan.close()
    ref = pic.episode(_oenv(orc, env), _state(env, st), key, cases.N_OF[name], H, ND, cases.TEMP, T, K, E, method, *rec, D=D,
                      rows0=rows0, plant=_oenv(orc, plant), dkey=dkey, **PLANT)
    _equal(ep, ref, f"{method} D={D}", _LOGS + (("predicted",) if D else ()))
    assert not np.array_equal(ref["states"], cases.episode(name, method, E, rec)["states"])
    assert not np.array_equal(ref["actions"][-E:], ref["means"][T - 1 - D][:E])  # (the action noise)


@pytest.mark.parametrize("method,rec", [("mppi", cases.RESET), ("cma-es", cases.CARRY)])
def test_warm_noise_shape_and_basis_leave_tick_0_flat(gpu, orc, method, rec):
    name, E = "hopper", 1
    env, st, key = _start(name)
    g, W = shape_of(H, env.action_size), nbc.basis_of(H, 4)
    W[H // 2] = (0.5, -0.25, 1.25, 0.75)  # (no frozen row)
    plan = _plan(env, name, method, st, rec)
    flat = plan.run_mpc(key, T, K, E)
    plan.set_noise_shape(g, "warm")
    plan.set_noise_basis(W, "warm")
    ep = plan.run_mpc(key, T, K, E)
    plan.set_noise_basis(W, "always")
    always = plan.run_mpc(key, 2, K, E)
    plan.close()
    args = (_state(env, st), key, cases.N_OF[name], H, ND, cases.TEMP)
    checker = lambda e, *a, **kw: pic.episode(e, *a, method, *rec, **kw)  # noqa: E731
    ref = nbc.episode(checker, _oenv(orc, env), W, "warm", ND, *args, T, K, E, shape=g, shape_when="warm")
    _equal(ep, ref, f"{method} warm shape and basis")
    _equal(flat, cases.episode(name, method, E, rec), "flat")
    assert np.array_equal(ep["means"][0], flat["means"][0]) and not np.array_equal(ep["means"][1], flat["means"][1])
    ref = nbc.episode(checker, _oenv(orc, env), W, "always", ND, *args, 2, K, E, shape=g, shape_when="warm")
    _equal(always, ref, f"{method} basis always")
    assert not np.array_equal(always["means"][0], flat["means"][0])


# ---- sweeps -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("method,rec", [("mppi", cases.RESET), ("cma-es", cases.CARRY), ("cem", cases.PLAIN)])
def test_sweep_episodes_are_the_single_plans(gpu, method, rec, P):
    """Episode k of a sweep, from its own state and key at its own temperature, is the plan's episode bit for bit."""
    from dataclasses import replace
    from mbd_hip.planners.mbd_planner import Plan, Sweep
    name, E = "hopper", 2
    env, st, key = _start(name)
    sts = [st] + [env.reset(gpu.prng_key(20 + k)) for k in range(1, P)]
    keys = np.array([key] + [gpu.prng_key(30 + k) for k in range(1, P)], np.uint32)
    temps = [0.1, 0.5, 0.05][:P]
    a = _args(name, cases.N_OF[name], H, ND)
    sw = Sweep(env, a, P, temps=temps, update_method=METHOD[method])
    for k in range(P):
        sw.set_state0(k, sts[k])
    with pytest.raises(gpu.MbdError, match="update_method"):
        sw.run_mpc(keys, T, K, E)
    sw.set_mpc_sigma(*rec)
    got = sw.run_mpc(keys, T, K, E)
    sw.close()
    assert got["sigmas"].shape == (P, T, 2)
    _equal({k: got[k][0] for k in _LOGS}, cases.episode(name, method, E, rec), "episode 0 against the checker")
    for k in range(P):
        plan = Plan(env, replace(a, temp_sample=temps[k]), update_method=METHOD[method])
        plan.set_state0(sts[k])
        plan.set_mpc_sigma(*rec)
        _equal({f: got[f][k] for f in _LOGS}, plan.run_mpc(keys[k], T, K, E), f"episode {k}")
        plan.close()
    if P > 1:
        assert not np.array_equal(got["means"][0], got["means"][1])


def test_sweep_with_per_episode_plants_and_a_delay(gpu):
    from mbd_hip.envs.base import RigidBodyEnv
    name, method, rec, E, D, P = "hopper", "cma-es", cases.CARRY, 1, 1, 3
    env, st, key = _start(name)
    plant = RigidBodyEnv(name, model=env.sys.scaled(**MISMATCH))
    sts = [st] + [env.reset(gpu.prng_key(20 + k)) for k in range(1, P)]
    keys = np.array([key] + [gpu.prng_key(30 + k) for k in range(1, P)], np.uint32)
    rows0 = _rows0(D, E, env.action_size)
    recs = [dict(env=plant, key=gpu.prng_key(11), **PLANT), None, dict(env=None, key=gpu.prng_key(12), act_std=0.2)]
    sw = _sweep(env, name, method, sts, rec)
    sw.set_mpc_delay(D, rows0)
    for k, r in enumerate(recs):
        if r is not None:
            sw.set_mpc_plant(k, **r)
    got = sw.run_mpc(keys, T, K, E)
    sw.close()
    for k, r in enumerate(recs):
        plan = _plan(env, name, method, sts[k], rec)
        plan.set_mpc_delay(D, rows0)
        if r is not None:
            plan.set_mpc_plant(**r)
        _equal({f: got[f][k] for f in _LOGS + ("predicted",)}, plan.run_mpc(keys[k], T, K, E), f"episode {k}", _LOGS + ("predicted",))
        plan.close()


# ---- sessions -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method,rec", [("mppi", cases.RESET), ("cma-es", cases.CARRY)])
def test_session_fed_the_episodes_states_returns_its_means_and_rows(gpu, orc, method, rec):
    """... and mbd_plan_get_sigma between two ticks is the sigma the next one starts from; after reset_mean that is sigma_cold,
    and the tick that follows is the checker's cold tick from the session's key chain."""
    name, E = "hopper", 1
    env, st, key = _start(name)
    plan = _plan(env, name, method, st, rec)
    ep = plan.run_mpc(key, T + 1, K, E)
    _equal({k: ep[k][: len(v)] for k, v in cases.episode(name, method, E, rec).items()}, cases.episode(name, method, E, rec))
    ref = pic.Session(_oenv(orc, env), key, cases.N_OF[name], H, ND, cases.TEMP, K, E, method, *rec)
    with plan.mpc_open(key, K, E) as ss:
        assert np.float32(plan.get_sigma()) == np.float32(rec[0])
        for t in range(T):
            out = ss.tick(ep["states"][t])
            assert np.array_equal(out["mean"], ep["means"][t]) and np.array_equal(out["rows"], ep["actions"][t * E:(t + 1) * E]), t
            assert (out["flags"] & gpu.TICK_COLD != 0) == (t == 0)
            assert np.float32(plan.get_sigma()) == ep["sigmas"][t + 1, 0], t
            ref.tick(ep["states"][t])
        with pytest.raises(gpu.MbdError, match="session") as e:
            plan.set_mpc_sigma(*rec)
        assert e.value.code == gpu.MBD_ERR_STATE
        ss.reset_mean()
        ref.reset_mean()
        assert np.float32(plan.get_sigma()) == np.float32(rec[0])
        for t in (T, T - 1):  # a cold tick, then a warm one behind it
            out, want = ss.tick(ep["states"][t]), ref.tick(ep["states"][t])
            assert np.array_equal(out["mean"], want["mean"]) and np.array_equal(out["rows"], want["rows"]), t
            assert np.float32(plan.get_sigma()) == ref.sigma
            assert (out["flags"] & gpu.TICK_COLD != 0) == (t == T)
    _equal(plan.run_mpc(key, T + 1, K, E), ep, "an episode after the session")
    plan.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------

def test_refusals_that_need_a_handle(gpu):
    from mbd_hip.planners.mbd_planner import Plan
    lib = gpu.load()
    name = "hopper"
    env, st, key = _start(name)
    keyc = gpu.key_array(key)
    mc = gpu.MpcConfig(n_ticks=2, warm_steps=2, exec_steps=1)
    out = np.zeros((8, 2), np.float32)
    rec = gpu.MpcSigma(sigma_cold=1.0, sigma_warm=0.5, gain=0.0)
    # no record: the run and the open call, as before, now naming the set call
    for method in cases.METHODS:
        plan = _plan(env, name, method, st)
        for rc in (lib.mbd_plan_run_mpc(plan.h, C.byref(mc), keyc, None, None, None, None, None),
                   lib.mbd_plan_mpc_open(plan.h, C.byref(mc), keyc)):
            assert rc == gpu.MBD_ERR_UNSUPPORTED and b"update_method" in lib.mbd_last_error() and b"mbd_plan_set_mpc_sigma" in lib.mbd_last_error()
        # peek before a run, with and without a record
        assert lib.mbd_plan_peek_mpc_sigma(plan.h, gpu.np_ptr(out)) == gpu.MBD_ERR_STATE and b"no sigma record" in lib.mbd_last_error()
        assert lib.mbd_plan_set_mpc_sigma(plan.h, C.byref(rec)) == gpu.MBD_OK
        assert lib.mbd_plan_peek_mpc_sigma(plan.h, gpu.np_ptr(out)) == gpu.MBD_ERR_STATE and b"no episode" in lib.mbd_last_error()
        # gain > 0 is cma-es'
        carry = gpu.MpcSigma(sigma_cold=0.6, sigma_warm=0.3, gain=2.0)
        rc = lib.mbd_plan_set_mpc_sigma(plan.h, C.byref(carry))
        assert (rc == gpu.MBD_OK) == (method == "cma-es")
        if method != "cma-es":
            assert rc == gpu.MBD_ERR_INVALID and b"gain" in lib.mbd_last_error()
        # a refused record leaves the one in force: the run is accepted, the peek serves it, a set call forgets the log
        assert lib.mbd_plan_run_mpc(plan.h, C.byref(mc), keyc, None, None, None, None, None) == gpu.MBD_OK
        assert lib.mbd_plan_peek_mpc_sigma(plan.h, gpu.np_ptr(out)) == gpu.MBD_OK and out[0, 0] == np.float32(0.6 if method == "cma-es" else 1.0)
        assert lib.mbd_plan_set_mpc_sigma(plan.h, C.byref(rec)) == gpu.MBD_OK
        assert lib.mbd_plan_peek_mpc_sigma(plan.h, gpu.np_ptr(out)) == gpu.MBD_ERR_STATE
        # sharded plans and ensembles stay refused
        plan.close()
    # a record on an MBD plan or sweep
    mbd = Plan(env, _args(name, 64, H, ND))
    assert lib.mbd_plan_set_mpc_sigma(mbd.h, C.byref(rec)) == gpu.MBD_ERR_STATE and b"not a path-integral plan" in lib.mbd_last_error()
    assert lib.mbd_plan_set_mpc_sigma(mbd.h, None) == gpu.MBD_ERR_STATE
    assert lib.mbd_plan_run_mpc(mbd.h, C.byref(mc), keyc, None, None, None, None, None) == gpu.MBD_OK
    mbd.close()
    sharded = Plan(env, _args(name, 64, H, ND), shard_begin=0, shard_count=32, update_method=1)
    assert lib.mbd_plan_set_mpc_sigma(sharded.h, C.byref(rec)) == gpu.MBD_OK
    assert lib.mbd_plan_run_mpc(sharded.h, C.byref(mc), keyc, None, None, None, None, None) == gpu.MBD_ERR_STATE and b"shard" in lib.mbd_last_error()
    sharded.close()
    from mbd_hip.planners.mbd_planner import Sweep
    sw0 = Sweep(env, _args(name, 64, H, ND), 2)
    assert lib.mbd_sweep_set_mpc_sigma(sw0.h, C.byref(rec)) == gpu.MBD_ERR_STATE and b"not a path-integral sweep" in lib.mbd_last_error()
    sw0.close()
    # sweeps: sessions stay refused, record or not; peek before a run and outside the episodes
    sw = _sweep(env, name, "mppi", [st, st])
    keys = np.array([key, key], np.uint32)
    for with_rec in (False, True):
        if with_rec:
            assert lib.mbd_sweep_set_mpc_sigma(sw.h, C.byref(rec)) == gpu.MBD_OK
        assert lib.mbd_sweep_mpc_open(sw.h, C.byref(mc), gpu.np_ptr(keys)) == gpu.MBD_ERR_UNSUPPORTED
        assert b"update_method" in lib.mbd_last_error()
        assert lib.mbd_sweep_peek_mpc_sigma(sw.h, 0, gpu.np_ptr(out)) == gpu.MBD_ERR_STATE
    assert lib.mbd_sweep_set_mpc_sigma(sw.h, C.byref(gpu.MpcSigma(sigma_cold=0.6, sigma_warm=0.3, gain=2.0))) == gpu.MBD_ERR_INVALID
    assert lib.mbd_sweep_run_mpc(sw.h, C.byref(mc), gpu.np_ptr(keys), None, None, None, None, None) == gpu.MBD_OK
    assert lib.mbd_sweep_peek_mpc_sigma(sw.h, 1, gpu.np_ptr(out)) == gpu.MBD_OK and out[1, 0] == 0.5
    assert lib.mbd_sweep_peek_mpc_sigma(sw.h, 2, gpu.np_ptr(out)) == gpu.MBD_ERR_INVALID
    sw.close()


# ---- command line -------------------------------------------------------------------------------------------------------------

def _cli(tmp_path, *flags):
    pkg = os.path.join(ROOT, "model-based-diffusion_amd")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([pkg, ROOT, os.environ.get("PYTHONPATH", "")]))
    return subprocess.run([sys.executable, "-m", "mbd_hip.planners.mpc", "--env_name", "hopper", "--disable_recommended_params",
                           "--seed", str(cases.SEED), "--Nsample", "64", "--Hsample", str(H), "--Ndiffuse", str(ND), "--n_ticks",
                           str(T), "--warm_steps", str(K), *flags], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)


def test_command_line(gpu, tmp_path):
    """--update_method mppi --sigma_warm 0.25 is the API call (the checker's episode of the same record); --n_episodes 3 is three
    single runs; --online with --n_episodes ends with the library's refusal."""
    from dataclasses import replace
    from mbd_hip.planners.mpc import run_mpc
    rec = (1.0, 0.25, 0.0)
    out = _cli(tmp_path, "--update_method", "mppi", "--sigma_warm", "0.25")
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["update_method"] == "mppi" and res["sigma_warm"] == 0.25 and res["sigma_cold"] == 1.0 and res["sigma_gain"] == 0.0
    ep = np.load(os.path.join(tmp_path, "results", "hopper", "mpc_episode.npz"))
    ref = cases.episode("hopper", "mppi", 1, rec)
    _equal(ep, ref, "command line")
    assert np.float32(res["episode_reward"]) == np.float32(ref["rewards"].mean())
    a = _args("hopper", 64, H, ND, seed=cases.SEED, n_ticks=T, warm_steps=K, update_method="mppi", sigma_warm=0.25)
    rew, det = run_mpc(a, return_details=True)
    _equal(det, ref, "run_mpc")
    out = _cli(tmp_path, "--update_method", "mppi", "--sigma_warm", "0.25", "--n_episodes", "3")
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    ep = np.load(os.path.join(tmp_path, "results", "hopper", "mpc_episode.npz"))
    assert res["n_episodes"] == 3 and ep["sigmas"].shape == (3, T, 2)
    _equal({k: ep[k][0] for k in _LOGS}, ref, "episode 0 of the batch")
    for k in (1, 2):
        _, det = run_mpc(replace(a, seed=cases.SEED + k), return_details=True)
        _equal({f: ep[f][k] for f in _LOGS}, det, f"episode {k} of the batch")
    out = _cli(tmp_path, "--update_method", "mppi", "--sigma_warm", "0.25", "--online")  # the same episode through a session
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    ep = np.load(os.path.join(tmp_path, "results", "hopper", "mpc_episode.npz"))
    assert res["online"] is True and res["update_method"] == "mppi"
    _equal(ep, ref, "online", ("means", "actions", "rewards", "states"))
    out = _cli(tmp_path, "--update_method", "mppi", "--n_episodes", "3", "--online")
    assert out.returncode != 0 and "update_method" in out.stderr and "sessions of sweeps" in out.stderr


def test_c_caller_drives_an_mppi_session(gpu, tmp_path):
    """examples/mbd_control.c --mppi from plain C: the rewards of its 5 ticks are those of the Python session on the same plan —
    record {1, 0.25, 0}, seed 0's reset and key, the rows executed with mbd_env_step."""
    libdir = os.path.join(ROOT, "model-based-diffusion_amd", "lib")
    exe = str(tmp_path / "mbd_control")
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "mbd_control.c"),
                    "-o", exe, "-L", libdir, "-lmbd_hip", f"-Wl,-rpath,{libdir}", "-lm"], check=True)
    out = subprocess.run([exe, "hopper", "64", str(H), str(ND), str(K), str(T), "0", "--mppi"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    ticks = [ln.split() for ln in out.stdout.strip().splitlines() if ln.startswith("tick ")]
    assert [int(t[7]) for t in ticks] == [4] + [0] * (T - 1)
    env = _env("hopper")
    rng_episode, rng_reset = gpu.prng_split(gpu.prng_key(0), 2, 1)
    st = env.reset(rng_reset)
    plan = _plan(env, "hopper", "mppi", st, (1.0, 0.25, 0.0))
    ep = plan.run_mpc(rng_episode, T, K, 1)  # (nothing disturbed, the plan's env executes: the session's episode)
    plan.close()
    assert [np.float32(float(t[3])) for t in ticks] == [np.float32(r) for r in ep["rewards"]]
