"""Receding-horizon episodes planned ahead of the plant, on the GPU (include/mbd_hip.h mbd_mpc_delay; DESIGN.md section 1 "N9
delay").  Every comparison is np.array_equal.

  episodes        actions, rewards, states, means and predicted states against tests/mpc_delay_checker.py: hopper (planar, two
                  spheres per foot) E in {1, 2}, D in {1, 2, 3}; humanoidrun at N = 128 (the 16-lane 3-D kernel) D in {1, 2};
                  car2d D = 2 — each with rows0 = NULL and with random committed rows, without and with a plant record
  records         an ensemble (the prediction keeps the plan's env), a warm noise shape with a 4-knot basis
  definition      the D = 1 shift identity and predicted[t] == states[t + 1].  The shifted episode is TWO RUNS OF THE LIBRARY
                  compared with each other — the delayed one and the undelayed one from its s_1 — not a comparison with the
                  checker: it pins the definition, not parity (the episodes above hold both runs to the checker).
  properties      prefix, set-then-clear, the levers
  sweeps          P in {1, 3} episodes equal the single plans'; a plant that diverges in the middle episode
  refusals        what only a real handle decides: a non-finite row, n_rows against the run's D * exec_steps, peek before a run
  command line    --delay_ticks equals the API call; --n_episodes 4 equals four single runs
"""
import ctypes as C
import json
import os
import subprocess
import sys
from dataclasses import replace

import numpy as np
import pytest

import containment_inputs as ci
import ensemble_checker
import mpc_delay_checker as mdc
import noise_basis_checker as nbc
from conftest import ROOT
from test_gpu_noise_shape import _args, _env, _oenv, _state, shape_of

pytestmark = pytest.mark.gpu

_LOGS = ("means", "actions", "rewards", "states", "predicted")
N, H, ND, K, T = 64, 20, 6, 2, 5  # the sizes of the episodes against the checker
PLANT = dict(act_std=0.1, kick_std=0.3, kick_every=2)
MISMATCH = dict(mass=1.3, friction=0.5, gear=0.8)


@pytest.fixture(scope="module")
def gpu(lib):
    from mbd_hip import _capi
    if _capi.device_count() < 1:
        pytest.fail("tests/test_gpu_mpc_delay.py needs a GPU")
    return _capi


def _equal(a, b, what="", logs=_LOGS):
    for k in logs:
        x, y = np.asarray(a[k], np.float32), np.asarray(b[k], np.float32)
        assert x.size == y.size and np.array_equal(x.reshape(y.shape), y), f"{what}: {k} differ"


def _rows0(D, E, Nu, seed=3):
    """Finite random committed rows in [-1, 1], one of them a negative zero."""
    r = np.random.default_rng(seed).uniform(-1, 1, (D * E, Nu)).astype(np.float32)
    r[0, 0] = -0.0
    return r


def _plan(env, name, n, st, h=H, nd=ND):
    from mbd_hip.planners.mbd_planner import Plan
    plan = Plan(env, _args(name, n, h, nd))
    plan.set_state0(st)
    return plan


def _plant_of(env, name):
    """(plant env or None, the record's settings): the issue's mismatch and disturbances; car2d has no body to scale and no
    link to kick, so its record carries the action noise only."""
    from mbd_hip.envs.base import RigidBodyEnv
    if name == "car2d":
        return None, dict(act_std=PLANT["act_std"])
    return RigidBodyEnv(name, model=env.sys.scaled(**MISMATCH)), dict(PLANT)


# ---- episodes against the checker -------------------------------------------------------------------------------------------

_CASES = [("hopper", N, E, D) for E in (1, 2) for D in (1, 2, 3)] + [("humanoidrun", 128, 1, 1), ("humanoidrun", 128, 1, 2),
                                                                     ("car2d", N, 1, 2)]


@pytest.mark.parametrize("with_plant", [False, True], ids=["nominal", "plant"])
@pytest.mark.parametrize("name,n,E,D", _CASES)
def test_episode_matches_the_checker(gpu, orc, name, n, E, D, with_plant):
    """With the plant record (mass 1.3, friction 0.5, gear 0.8, act_std 0.1, kick_std 0.3 every 2nd tick) the queue keeps the
    undisturbed rows, the shift takes the undisturbed mean, and ticks 1 and 3 go through the boundary's kick variant."""
    from mbd_hip.envs.base import prng_impl
    env = _env(name)
    st, key, dkey = env.reset(gpu.prng_key(5)), gpu.prng_key(6), gpu.prng_key(11)
    plant, rec = _plant_of(env, name) if with_plant else (None, None)
    plan = _plan(env, name, n, st)
    if with_plant:
        plan.set_mpc_plant(env=plant, key=dkey, **rec)
    kw = dict(plant=None if plant is None else _oenv(orc, plant), dkey=dkey, **rec) if with_plant else {}
    for rows0 in (None, _rows0(D, E, env.action_size)):
        plan.set_mpc_delay(D, rows0)
        ep = plan.run_mpc(key, T, K, E)
        ref = mdc.episode(_oenv(orc, env), _state(env, st), key, n, H, ND, 0.1, T, K, E, D, rows0=rows0, impl=prng_impl(), **kw)
        _equal(ep, ref, f"{name} E={E} D={D} rows0={'given' if rows0 is not None else 'NULL'}")
        assert ep["predicted"].shape == (T, ref["states"].shape[1]) and np.isfinite(ref["states"]).all()
        if with_plant:
            assert not np.array_equal(ref["actions"][-E:], ref["means"][T - 1 - D][:E])  # (the action noise)
            assert not np.array_equal(ref["predicted"][0], ref["states"][D])  # (the plan's env is not the plant)
        else:
            assert np.array_equal(ref["actions"][-E:], ref["means"][T - 1 - D][:E])
        if rows0 is not None and not with_plant:
            assert ep["actions"][: D * E].tobytes() == rows0.tobytes()
    plan.close()


@pytest.mark.parametrize("risk", ["mean", "min"])
def test_ensemble_episode_predicts_with_the_plans_env(gpu, orc, risk):
    """M = 2 (the plan's env and one of mass 1.3, gear 0.8), D = 1: the candidates are scored over the members, the prediction
    is one rollout of the plan's own env."""
    from mbd_hip.envs.base import RigidBodyEnv, prng_impl
    name, E, D = "hopper", 1, 1
    env = _env(name)
    member = RigidBodyEnv(name, model=env.sys.scaled(mass=1.3, gear=0.8))
    st, key = env.reset(gpu.prng_key(5)), gpu.prng_key(6)
    plan = _plan(env, name, N, st)
    plan.set_ensemble([None, member], risk)
    plan.set_mpc_delay(D)
    ep = plan.run_mpc(key, T, K, E)
    plan.close()
    oenv = _oenv(orc, env)
    ee = ensemble_checker.EnsembleEnv(oenv, [None, _oenv(orc, member)], risk)
    ref = mdc.episode(ee, _state(env, st), key, N, H, ND, 0.1, T, K, E, D, plant=oenv, impl=prng_impl())
    _equal(ep, ref, f"ensemble {risk}")
    assert np.array_equal(ep["predicted"], ep["states"][1:])  # (D = 1, nothing disturbed, the plan's env executes)


def test_warm_noise_shape_and_basis_leave_tick_0_flat(gpu, orc):
    """A noise shape and a 4-knot basis, both under MBD_NOISE_WARM_TICKS, D = 1: tick 0 is the flat, white plan from shat_0."""
    from mbd_hip.envs.base import prng_impl
    name, E, D = "hopper", 1, 1
    env = _env(name)
    st, key = env.reset(gpu.prng_key(5)), gpu.prng_key(6)
    g, W = shape_of(H, env.action_size), nbc.basis_of(H, 4)
    W[H // 2] = (0.5, -0.25, 1.25, 0.75)  # (no frozen row)
    plan = _plan(env, name, N, st)
    plan.set_mpc_delay(D)
    flat = plan.run_mpc(key, T, K, E)
    plan.set_noise_shape(g, "warm")
    plan.set_noise_basis(W, "warm")
    ep = plan.run_mpc(key, T, K, E)
    plan.close()
    checker = lambda e, *a, **kw: mdc.episode(e, *a, D, **kw)  # noqa: E731
    ref = nbc.episode(checker, _oenv(orc, env), W, "warm", ND, _state(env, st), key, N, H, ND, 0.1, T, K, E, shape=g,
                      shape_when="warm", impl=prng_impl())
    _equal(ep, ref, "warm shape and basis")
    assert np.array_equal(ep["means"][0], flat["means"][0]) and not np.array_equal(ep["means"][1], flat["means"][1])


# ---- the definition and the properties --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,n,E", [("hopper", N, 2), ("humanoidrun", 128, 1), ("car2d", N, 1)])
def test_d1_is_the_undelayed_episode_shifted_by_one_tick(gpu, name, n, E):
    """TWO RUNS OF THE LIBRARY against each other, no checker: the delayed episode of T + 1 ticks from s_0 and the undelayed
    one of T ticks from the delayed one's s_1, same key.  Also with a plant record that disturbs nothing (plant NULL, stds 0)."""
    env = _env(name)
    st, key = env.reset(gpu.prng_key(5)), gpu.prng_key(6)
    rows0 = _rows0(1, E, env.action_size)
    plan = _plan(env, name, n, st)
    plan.set_mpc_delay(1, rows0)
    d = plan.run_mpc(key, T + 1, K, E)
    plan.set_mpc_plant(key=gpu.prng_key(123), kick_every=2)
    _equal(plan.run_mpc(key, T + 1, K, E), d, "a record that disturbs nothing")
    plan.close()
    assert np.array_equal(d["predicted"], d["states"][1:])
    assert d["actions"][:E].tobytes() == rows0.tobytes()
    from mbd_hip.envs.base import State
    und = _plan(env, name, n, State(d["states"][1], None, np.float32(0), np.float32(0), {}))
    u = und.run_mpc(key, T, K, E)
    und.close()
    assert "predicted" not in u
    assert np.array_equal(d["means"][:T], u["means"]) and np.array_equal(d["states"][1:], u["states"])
    assert np.array_equal(d["actions"][E:], u["actions"]) and np.array_equal(d["rewards"][E:], u["rewards"])


@pytest.mark.parametrize("D", [1, 3])
def test_prefix_and_cleared_record(gpu, D):
    """T = 3 is a prefix of T = 4; tick 0's mean is Plan.run(k_0) of a plan whose state0 is shat_0; set then clear gives the plan
    that never had a record — its episode, and a following Plan.run equals a fresh plan's."""
    from mbd_hip.envs.base import State
    name, E = "hopper", 2
    env = _env(name)
    st, key = env.reset(gpu.prng_key(5)), gpu.prng_key(6)
    fresh = _plan(env, name, N, st)
    nominal = fresh.run_mpc(key, 4, K, E)
    want_run = fresh.run(key)
    fresh.close()
    plan = _plan(env, name, N, st)
    plan.set_mpc_delay(D, _rows0(D, E, env.action_size))
    long, short = plan.run_mpc(key, 4, K, E), plan.run_mpc(key, 3, K, E)
    for k in _LOGS:
        assert np.array_equal(short[k], long[k][: len(short[k])]), k
    assert not np.array_equal(long["states"][1:], nominal["states"][1:])
    during = plan.run(key)  # (run ignores the record)
    plan.clear_mpc_delay()
    cleared = plan.run_mpc(key, 4, K, E)
    assert "predicted" not in cleared
    _equal(cleared, nominal, "after clear", _LOGS[:4])
    after = plan.run(key)
    for got in (during, after):
        for x, y in zip(got[:3], want_run[:3]):
            assert np.array_equal(np.asarray(x, np.float32), np.asarray(y, np.float32))
    with pytest.raises(gpu.MbdError) as e:
        np_out = np.zeros((4, long["predicted"].shape[1]), np.float32)
        gpu.check(plan.lib.mbd_plan_peek_mpc_predicted(plan.h, gpu.np_ptr(np_out)))
    assert e.value.code == gpu.MBD_ERR_STATE
    plan.close()
    cold = _plan(env, name, N, State(long["predicted"][0], None, np.float32(0), np.float32(0), {}))
    mu = cold.run(gpu.prng_split(key, 2, cold.cfg.prng_impl)[1])[0]
    cold.close()
    assert np.array_equal(long["means"][0], mu[-1])


@pytest.mark.parametrize("lever", ["MBD_NO_PREFETCH", "MBD_NO_LAZY"])
def test_delayed_episode_is_the_same_under_the_levers(gpu, levers, lever):
    from mbd_hip.envs.base import RigidBodyEnv
    name, E, D = "hopper", 2, 2

    def episode():
        env = _env(name)
        plant = RigidBodyEnv(name, model=env.sys.scaled(**MISMATCH))
        plan = _plan(env, name, N, env.reset(gpu.prng_key(5)))  # (after the lever: MBD_NO_LAZY acts on plans created from then on)
        plan.set_mpc_plant(env=plant, key=gpu.prng_key(9), **PLANT)
        plan.set_mpc_delay(D, _rows0(D, E, env.action_size))
        out = plan.run_mpc(gpu.prng_key(6), T, K, E)
        plan.close()
        return out
    ref = episode()
    levers(**{lever: 1})
    _equal(episode(), ref, lever)


# ---- sweeps -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,n", [("hopper", N), ("humanoidrun", 128)])
@pytest.mark.parametrize("P", [1, 3])
def test_batch_equals_the_single_episodes(gpu, name, n, P):
    """Seeds, temperatures and per-episode plant records of two different plants (the last episode: none): episode k of the
    sweep equals Plan.run_mpc on a plan of its own with the same delay record."""
    from mbd_hip.envs.base import RigidBodyEnv
    from mbd_hip.planners.mbd_planner import Plan, Sweep
    env, E, D = _env(name), 1, 2
    plants = [RigidBodyEnv(name, model=env.sys.scaled(mass=1.3)), RigidBodyEnv(name, model=env.sys.scaled(friction=0.5, gear=0.8))]
    recs = [dict(env=plants[0], key=gpu.prng_key(300), **PLANT), dict(env=plants[1], key=gpu.prng_key(301), act_std=0.2), None][:P]
    if P == 1:
        recs = [recs[0]]
    temps = [0.1, 0.3, 0.05][:P]
    keys = np.array([gpu.prng_key(100 + k) for k in range(P)], np.uint32)
    states = [env.reset(gpu.prng_key(k)) for k in range(P)]
    rows0 = _rows0(D, E, env.action_size)
    a = _args(name, n, H, ND)
    sw = Sweep(env, a, P, temps=temps)
    sw.set_mpc_delay(D, rows0)
    for k in range(P):
        sw.set_state0(k, states[k])
        if recs[k] is not None:
            sw.set_mpc_plant(k, **recs[k])
    batch = sw.run_mpc(keys, T, K, E)
    sw.clear_mpc_delay()
    assert "predicted" not in sw.run_mpc(keys, 2, K, E)
    sw.close()
    assert batch["predicted"].shape == (P, T, batch["states"].shape[2])
    for k in range(P):
        plan = Plan(env, replace(a, temp_sample=temps[k]))
        plan.set_state0(states[k])
        plan.set_mpc_delay(D, rows0)
        if recs[k] is not None:
            plan.set_mpc_plant(**recs[k])
        one = plan.run_mpc(keys[k], T, K, E)
        plan.close()
        _equal({f: batch[f][k] for f in _LOGS}, one, f"episode {k} of {P}")


def test_an_episode_whose_plant_diverges_stays_alone_in_the_prediction_launch(gpu, orc):
    """P = 3 hopper episodes, D = 1, the middle one on the plant with the 1e30 gear (tests/containment_inputs.py).  Tick 0 feeds it
    the committed zeros (0 * 1e30 = 0); tick 1 feeds it a planned row and its state overflows; from tick 2 on its prediction —
    one wavefront of the launch that predicts all three episodes — starts from that state.  Its states and predictions are
    non-finite wherever the checker's are, and equal the checker's before; the two other episodes keep their single-plan bits."""
    from mbd_hip.envs.base import RigidBodyEnv, prng_impl
    from mbd_hip.planners.mbd_planner import Plan, Sweep
    name, n, h, nd, P, E, D, T_ = "hopper", 33, ci.SWEEP_H, ci.SWEEP_ND, 3, 1, 1, 4
    env = _env(name)
    bad = RigidBodyEnv(name, model=ci.poison_model(env.sys))
    a = _args(name, n, h, nd)
    keys = np.array([gpu.prng_key(70 + k) for k in range(P)], np.uint32)
    states = [env.reset(gpu.prng_key(20 + k)) for k in range(P)]
    sw = Sweep(env, a, P)
    sw.set_mpc_delay(D)
    for k in range(P):
        sw.set_state0(k, states[k])
    sw.set_mpc_plant(1, env=bad, key=gpu.prng_key(7))
    got = sw.run_mpc(keys, T_, K, E)
    sw.close()
    for k in (0, 2):
        plan = Plan(env, a)
        plan.set_state0(states[k])
        plan.set_mpc_delay(D)
        one = plan.run_mpc(keys[k], T_, K, E)
        plan.close()
        for f in _LOGS:
            assert np.isfinite(one[f]).all(), f"episode {k} alone: {f}"
        _equal({f: got[f][k] for f in _LOGS}, one, f"episode {k}")
    ref = mdc.episode(_oenv(orc, env), _state(env, states[1]), keys[1], n, h, nd, 0.1, T_, K, E, D, plant=_oenv(orc, bad),
                      dkey=gpu.prng_key(7), impl=prng_impl())
    assert np.isfinite(ref["states"][:2]).all() and not np.isfinite(ref["states"][2]).all()
    assert not np.isfinite(ref["predicted"][2]).all(), "the checker's prediction from the overflowed state must be non-finite"
    for f in ("states", "predicted"):
        x = got[f][1]
        assert not np.isfinite(x[~np.isfinite(ref[f])]).any(), f
    assert np.array_equal(got["states"][1][:2], ref["states"][:2]) and np.array_equal(got["predicted"][1][:2], ref["predicted"][:2])
    assert np.array_equal(got["means"][1][:2], ref["means"][:2])


# ---- refusals that need a real handle ---------------------------------------------------------------------------------------

def test_refusals_on_a_plan_and_on_a_sweep(gpu):
    from mbd_hip.planners.mbd_planner import Plan, Sweep
    lib = gpu.load()
    name, E = "hopper", 2
    env = _env(name)
    a = _args(name, N, H, ND)
    plan, sweep = Plan(env, a), Sweep(env, a, 2)
    st, key = env.reset(gpu.prng_key(5)), gpu.prng_key(6)
    plan.set_state0(st)
    for k in range(2):
        sweep.set_state0(k, st)
    keys = np.array([key, key], np.uint32)
    out = np.zeros((2, T, 64), np.float32)
    for obj, setter, peek in ((plan, lib.mbd_plan_set_mpc_delay, lib.mbd_plan_peek_mpc_predicted),
                              (sweep, lib.mbd_sweep_set_mpc_delay, lib.mbd_sweep_peek_mpc_predicted)):
        run = (lambda T_, E_: plan.run_mpc(key, T_, K, E_)) if obj is plan else (lambda T_, E_: sweep.run_mpc(keys, T_, K, E_))
        assert peek(obj.h, gpu.np_ptr(out)) == gpu.MBD_ERR_STATE and b"no delay record" in lib.mbd_last_error()
        obj.set_mpc_delay(2, _rows0(2, E, env.action_size))
        assert peek(obj.h, gpu.np_ptr(out)) == gpu.MBD_ERR_STATE and b"with the record yet" in lib.mbd_last_error()
        ref = run(3, E)
        # a refused record changes nothing: the one set first is still there
        for bad in (np.nan, np.inf, -np.inf):
            r = _rows0(2, E, env.action_size)
            r[3, 1] = bad
            rec = gpu.MpcDelay()
            rec.delay_ticks, rec.n_rows, rec.rows0 = 2, 4, r.ctypes.data_as(C.POINTER(C.c_float))
            assert setter(obj.h, C.byref(rec)) == gpu.MBD_ERR_INVALID and b"rows0[3][1]" in lib.mbd_last_error()
        with pytest.raises(gpu.MbdError):
            obj.set_mpc_delay(9)
        again = run(3, E)
        _equal(again, ref, "after refused records")
        # the run call: n_rows = 4 is D * exec_steps for E = 2 only
        for E_bad in (1, 3):
            with pytest.raises(gpu.MbdError) as e:
                run(3, E_bad)
            assert e.value.code == gpu.MBD_ERR_INVALID and "n_rows=4" in str(e.value)
        # rows0 = NULL serves every exec_steps
        obj.set_mpc_delay(2)
        for E_ok in (1, 3):
            assert run(2, E_ok)["predicted"].shape[-2] == 2
    plan.close()
    sweep.close()


# ---- the command line -------------------------------------------------------------------------------------------------------

def _cli(tmp_path, *extra):
    pkg = os.path.join(ROOT, "model-based-diffusion_amd")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([pkg, ROOT, os.environ.get("PYTHONPATH", "")]))
    out = subprocess.run([sys.executable, "-m", "mbd_hip.planners.mpc", "--env_name", "hopper", "--disable_recommended_params",
                          "--Nsample", "128", "--Hsample", "20", "--Ndiffuse", "10", "--n_ticks", "6", "--warm_steps", "3",
                          "--exec_steps", "2", *extra], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1]), np.load(os.path.join(tmp_path, "results", "hopper", "mpc_episode.npz"))


@pytest.mark.parametrize("P", [1, 4])
def test_command_line(gpu, tmp_path, P):
    """--delay_ticks 2 at N = 128, H = 20, Nd = 10, T = 6: the saved episode equals run_mpc's of the same arguments, and the
    episodes of --n_episodes 4 equal the four single runs."""
    from mbd_hip.planners.mpc import MpcArgs, run_mpc
    res, saved = _cli(tmp_path, "--delay_ticks", "2", "--plant_mass", "1.3", *(("--n_episodes", str(P)) if P > 1 else ()))
    assert res["delay_ticks"] == 2 and res["plant_mass"] == 1.3 and np.isfinite(res["episode_reward"])
    if P > 1:
        assert res["n_episodes"] == P
    a = MpcArgs(env_name="hopper", disable_recommended_params=True, Nsample=128, Hsample=20, Ndiffuse=10, n_ticks=6, warm_steps=3,
                exec_steps=2, delay_ticks=2, plant_mass=1.3, not_render=True)
    for k in range(P):
        rew, det = run_mpc(replace(a, seed=k), return_details=True)
        assert det["delay_ticks"] == 2 and det["predicted"].shape[0] == 6
        for f in _LOGS:
            x = saved[f][k] if P > 1 else saved[f]
            assert np.array_equal(x, det[f]), (k, f)
        if P == 1:
            assert np.float32(res["episode_reward"]) == np.float32(rew)
        else:
            assert np.float32(res["episode_rewards"][k]) == np.float32(rew)
    assert not saved["actions"].reshape(-1, 12, 3)[0][:4].any()  # (the committed zeros of the first D ticks)
