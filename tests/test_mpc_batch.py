"""Batched receding-horizon episodes (include/mbd_hip.h mbd_sweep_run_mpc, mbd_hip.planners.mpc.run_mpc_batch): P episodes of
one env in lockstep, episode k being the single episode of DESIGN.md section 1 "N5" bit for bit.

Without a GPU: the entry point is exported and refuses NULL arguments before touching a device, and run_mpc_batch refuses
argument lists that are no batch before touching an env.  With a GPU (-m gpu): every episode of a batch bit for bit against the
checker's restatement (tests/mpc_checker.py) — what parity rests on — then, at the sizes the checker is too slow for, against the
library's own single episodes (a self-comparison), the structure of a batch, the test levers, the refusals and the command line."""
import ctypes as C
import json
import os
import subprocess
import sys
from dataclasses import replace

import numpy as np
import pytest

import mpc_checker
from conftest import ROOT


def _args(name, N, H=50, Nd=20, K=4, E=1, T=4, seed=0, temp=0.1):
    from mbd_hip.planners.mpc import MpcArgs
    return MpcArgs(seed=seed, env_name=name, Nsample=N, Hsample=H, Ndiffuse=Nd, temp_sample=temp, n_ticks=T, warm_steps=K,
                   exec_steps=E, disable_recommended_params=True, not_render=True)


# ---- without a GPU ------------------------------------------------------------------------------------------------------

def test_sweep_run_mpc_is_exported_and_refuses_null_arguments_before_any_device_access(lib):
    from mbd_hip import _capi
    assert "mbd_sweep_run_mpc" in _capi.EXPORTS and hasattr(lib, "mbd_sweep_run_mpc")
    mc = _capi.MpcConfig(n_ticks=2, warm_steps=1, exec_steps=1)
    keys = (C.c_uint32 * 4)(0, 42, 0, 43)
    stand_in = C.create_string_buffer(1 << 16)  # a non-NULL handle the call must not reach: its config or keys is NULL
    for args, field in (((None, C.byref(mc), keys), b"sweep"), ((stand_in, None, keys), b"config"),
                        ((stand_in, C.byref(mc), None), b"keys")):
        assert lib.mbd_sweep_run_mpc(*args, None, None, None, None, None) == _capi.MBD_ERR_INVALID
        assert field in lib.mbd_last_error()


def test_run_mpc_batch_refuses_what_is_no_batch_before_any_env_or_device(monkeypatch):
    """Lists that differ in Hsample or env_name, 33 episodes and car2d: ValueError naming the field, decided from the arguments
    alone — creating an env (the first thing that needs the library and a device) is made to fail the test."""
    from mbd_hip.planners import mpc

    def no_env(*a, **k):
        raise AssertionError("run_mpc_batch reached get_env")
    monkeypatch.setattr(mpc, "get_env", no_env)
    a = _args("hopper", 64, H=20, Nd=6)
    with pytest.raises(ValueError, match="Hsample"):
        mpc.run_mpc_batch([a, replace(a, seed=1, Hsample=21)])
    with pytest.raises(ValueError, match="env_name"):
        mpc.run_mpc_batch([a, replace(a, seed=1, env_name="halfcheetah")])
    with pytest.raises(ValueError, match="33 episodes"):
        mpc.run_mpc_batch([replace(a, seed=s) for s in range(33)])
    with pytest.raises(ValueError, match="env_name='car2d'"):
        mpc.run_mpc_batch([replace(a, seed=s, env_name="car2d") for s in range(2)])
    with pytest.raises(ValueError, match="n_ticks"):
        mpc.run_mpc_batch([a, replace(a, seed=1, n_ticks=5)])
    with pytest.raises(ValueError, match="Nsample"):
        mpc.run_mpc_batch([replace(a, seed=s, Nsample=16384) for s in range(2)])


# ---- on the GPU ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu(lib):
    from mbd_hip import _capi
    if _capi.device_count() < 1:
        pytest.fail("GPU tests need a visible MI355X; the product has no CPU fallback")
    return _capi


_LOGS = ("means", "actions", "rewards", "states")


def _same_episode(got, ref, what=""):
    T = len(ref["means"])
    first = next((t for t in range(T) if not np.array_equal(got["means"][t], ref["means"][t])), None)
    assert first is None, f"{what}: the means differ from tick {first} on"
    for k in ("actions", "rewards", "states"):
        g = np.asarray(got[k], np.float32).reshape(np.asarray(ref[k]).shape)
        assert np.array_equal(g, ref[k]), f"{what}: {k} differ"


def _episode_of(batch, k):
    return {f: batch[f][k] for f in _LOGS}


def _sweep_choice(env, a, P):
    """The rollout launch the library picks for a diffusion step of the batch (include/mbd_hip_debug.h)."""
    import torch
    from mbd_hip import _capi
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    return _capi.debug_rollout_choice(env.sys.to_struct(), n_cus, P * a.Nsample, a.Hsample, a.Nsample)


def _batch_against_checker(orc, arg_list):
    from mbd_hip.envs import get_env
    from mbd_hip.envs.base import prng_impl
    from mbd_hip.planners.mpc import run_mpc_batch
    from test_gpu_parity import _oenv
    rews, dets = run_mpc_batch(arg_list, return_details=True)
    oe = _oenv(orc, get_env(arg_list[0].env_name))
    assert len(rews) == len(dets) == len(arg_list)
    for k, (a, det) in enumerate(zip(arg_list, dets)):
        ref = mpc_checker.episode(oe, np.asarray(det["state_init"].pipeline_state, np.float32), det["key"], a.Nsample,
                                  a.Hsample, a.Ndiffuse, a.temp_sample, a.n_ticks, a.warm_steps, a.exec_steps, impl=prng_impl())
        _same_episode(det, ref, f"{a.env_name} episode {k}")
        assert np.float32(rews[k]) == np.float32(ref["rewards"].mean())
        assert det["states"].shape == (a.n_ticks + 1, ref["states"].shape[1])
        assert not np.array_equal(ref["states"][0], ref["states"][-1])
    return dets


@pytest.mark.gpu
@pytest.mark.parametrize("name,P,N,E", [("humanoidrun", 8, 1024, 1), ("hopper", 4, 512, 2), ("halfcheetah", 3, 256, 1),
                                        ("ant", 2, 256, 1)])
def test_batch_matches_the_checker(gpu, orc_omp, name, P, N, E):
    """Cases A-D: every episode of a batch — its own seed, hence its own reset state and key — against the checker's episode
    from that state, key and temperature: means, actions, rewards and states of all T = 4 ticks (H = 50, Nd = 20, K = 4), bit
    for bit.  humanoidrun's P N = 8192 candidates go through the two-candidates-per-lane kernel: asserted, not assumed."""
    from mbd_hip.envs import get_env
    arg_list = [_args(name, N, E=E, seed=3 + k) for k in range(P)]
    if name == "humanoidrun":
        assert "rollout_pk2_kernel" in _sweep_choice(get_env(name), arg_list[0], P)["name"]
    dets = _batch_against_checker(orc_omp, arg_list)
    assert len({np.asarray(d["states"][0]).tobytes() for d in dets}) == P  # (different seeds: different start states)


@pytest.mark.gpu
def test_batch_of_temperatures_matches_the_checker(gpu, orc_omp):
    """Case E: one seed at three temperatures — the episodes share the start state and the key and still differ."""
    dets = _batch_against_checker(orc_omp, [_args("humanoidrun", 256, temp=t) for t in (0.05, 0.1, 0.4)])
    assert len({np.asarray(d["means"]).tobytes() for d in dets}) == 3
    assert len({np.asarray(d["states"][0]).tobytes() for d in dets}) == 1


def _batch_and_singles(gpu, env, a, P, T, K, E=1, temps=None):
    """A batch on a Sweep, and each of its episodes on a Plan of its own from the same state, key and temperature."""
    from mbd_hip.planners.mbd_planner import Plan, Sweep
    keys = np.array([gpu.prng_key(100 + k) for k in range(P)], np.uint32)
    states = [env.reset(gpu.prng_key(k)) for k in range(P)]
    sw = Sweep(env, a, P, temps=temps)
    for k in range(P):
        sw.set_state0(k, states[k])
    batch = sw.run_mpc(keys, T, K, E)
    sw.close()
    assert batch["means"].shape == (P, T, a.Hsample, env.action_size) and batch["actions"].shape == (P, T * E, env.action_size)
    assert batch["rewards"].shape == (P, T * E) and batch["states"].shape[:2] == (P, T + 1) and batch["seconds"] > 0
    for k in range(P):
        plan = Plan(env, a if temps is None else replace(a, temp_sample=float(temps[k])))
        plan.set_state0(states[k])
        single = plan.run_mpc(keys[k], T, K, E)
        plan.close()
        _same_episode(_episode_of(batch, k), single, f"episode {k} of {P}")
    return batch


@pytest.mark.gpu
@pytest.mark.parametrize("P,N,Nd,K,T", [(8, 1024, 100, 20, 6), (32, 128, 12, 3, 4), (1, 256, 12, 3, 4)])
def test_batch_equals_the_single_episodes(gpu, P, N, Nd, K, T):
    """A SELF-COMPARISON of the library (parity rests on test_batch_matches_the_checker): at the metric's sizes, with the most
    episodes a sweep takes and with one, episode k of a batch equals Plan.run_mpc from the same state, key and temperature."""
    from mbd_hip.envs import get_env
    env = get_env("humanoidrun")
    temps = None if P != 32 else np.linspace(0.05, 0.5, 32).astype(np.float32)
    batch = _batch_and_singles(gpu, env, _args("humanoidrun", N, Nd=Nd), P, T, K, temps=temps)
    if P > 1:
        assert not np.array_equal(batch["means"][0], batch["means"][1])


@pytest.mark.gpu
@pytest.mark.parametrize("name,bits", [("ant", 8 | 128), ("hopper", 4 | 8 | 16 | 32)])
def test_batch_on_the_general_instantiations_equals_the_single_episodes(gpu, name, bits):
    """A SELF-COMPARISON: models with a specification word of their own (a 3-D and a planar one) run on the general
    instantiations, in a batch as in single episodes."""
    from test_gpu_parity import _spec_env
    env = _spec_env(name, bits)
    _batch_and_singles(gpu, env, _args(name, 48, H=12, Nd=6), 3, 4, 2, E=2)


@pytest.mark.gpu
def test_batch_logs_grow_after_their_first_use(gpu):
    """P = 2: a batch of T = 3 and then one of T = 7 on the same sweep — the sweep's logs grow behind their first use.  The
    short batch is a prefix of the long one per episode, and the long one equals the same 7 ticks on a fresh sweep."""
    from mbd_hip.envs import get_env
    from mbd_hip.planners.mbd_planner import Sweep
    P, K, E = 2, 3, 2
    a = _args("humanoidrun", 256, Nd=12)
    env = get_env("humanoidrun")
    keys = np.array([gpu.prng_key(30 + k) for k in range(P)], np.uint32)
    states = [env.reset(gpu.prng_key(5 + k)) for k in range(P)]

    def sweep():
        sw = Sweep(env, a, P)
        for k in range(P):
            sw.set_state0(k, states[k])
        return sw
    sw = sweep()
    short = sw.run_mpc(keys, 3, K, E)
    long = sw.run_mpc(keys, 7, K, E)
    sw.close()
    fresh = sweep()
    ref = fresh.run_mpc(keys, 7, K, E)
    fresh.close()
    for f in _LOGS:
        assert short[f].shape[1] < long[f].shape[1] and np.array_equal(short[f], long[f][:, : short[f].shape[1]]), f
        assert np.array_equal(long[f], ref[f]), f
    assert not np.array_equal(long["means"][0], long["means"][1])


@pytest.mark.gpu
def test_batch_structure(gpu):
    """A batch of T = 3 is a prefix of the same batch with T = 6; means[k][0] is the last mean of Sweep.run from
    split(keys[k])[1]; after a batch Sweep.run equals a fresh sweep's (the start states came back); reordering the episodes
    permutes the outputs and changes no bit."""
    from mbd_hip.envs import get_env
    from mbd_hip.planners.mbd_planner import Sweep
    P, K, E = 4, 3, 2
    a = _args("humanoidrun", 256, Nd=12)
    env = get_env("humanoidrun")
    keys = np.array([gpu.prng_key(20 + k) for k in range(P)], np.uint32)
    states = [env.reset(gpu.prng_key(k)) for k in range(P)]
    temps = np.array([0.1, 0.2, 0.05, 0.3], np.float32)

    def sweep(order):
        sw = Sweep(env, a, P, temps=temps[order])
        for j, k in enumerate(order):
            sw.set_state0(j, states[k])
        return sw
    ident = np.arange(P)
    sw = sweep(ident)
    long = sw.run_mpc(keys, 6, K, E)
    short = sw.run_mpc(keys, 3, K, E)
    for f in _LOGS:
        assert np.array_equal(short[f], long[f][:, : short[f].shape[1]]), f
    for k in range(P):
        assert np.array_equal(long["states"][k][0], np.asarray(states[k].pipeline_state, np.float32).reshape(-1))
    after = sw.run(keys)
    fresh = sweep(ident)
    ref = fresh.run(keys)
    for x, y in zip(after[:3], ref[:3]):
        assert np.array_equal(x, y)
    k0 = np.array([gpu.prng_split(keys[k], 2, fresh.cfg.prng_impl)[1] for k in range(P)], np.uint32)
    mu0 = fresh.run(k0)[0]
    assert np.array_equal(long["means"][:, 0], mu0[:, -1])
    sw.close()
    fresh.close()
    order = np.array([2, 0, 3, 1])
    perm = sweep(order)
    moved = perm.run_mpc(keys[order], 6, K, E)
    perm.close()
    for f in _LOGS:
        assert np.array_equal(moved[f], long[f][order]), f
    assert not np.array_equal(long["means"][0], long["means"][1])


@pytest.mark.gpu
@pytest.mark.parametrize("name,N,lever,values", [("humanoidrun", 1024, "MBD_WMEAN_V", (1, 2, 4)), ("humanoidrun", 1024, "MBD_PK2", (0, 1)),
                                                 ("humanoidrun", 256, "MBD_PK2", (0, 1)), ("ant", 256, "MBD_PK2", (0, 1)),
                                                 ("hopper", 512, "MBD_CPW", (0, 1, 2)), ("humanoidrun", 256, "MBD_NO_DPP", (1,)),
                                                 ("hopper", 512, "MBD_NO_DPP", (1,)), ("humanoidrun", 256, "MBD_NO_FUSED_NOISE", (1,)),
                                                 ("hopper", 512, "MBD_NO_FUSED_NOISE", (1,))])
def test_batch_is_the_same_under_every_lever(gpu, levers, name, N, lever, values):
    """The batch with no lever set against the batch under each value of the lever (the fixture sets every lever back)."""
    from mbd_hip.envs import get_env
    from mbd_hip.planners.mbd_planner import Sweep
    P = 8 if N == 1024 else 3
    a = _args(name, N, Nd=10)
    keys = np.array([gpu.prng_key(40 + k) for k in range(P)], np.uint32)
    states = [get_env(name).reset(gpu.prng_key(k)) for k in range(P)]

    def batch():
        env = get_env(name)  # (after the lever: MBD_NO_DPP acts on envs created from then on)
        sw = Sweep(env, a, P)
        for k in range(P):
            sw.set_state0(k, states[k])
        out = sw.run_mpc(keys, 4, 3, 1)
        sw.close()
        return out
    ref = batch()
    for v in values:
        levers(**{lever: v})
        got = batch()
        for f in _LOGS:
            assert np.array_equal(got[f], ref[f]), (lever, v, f)
    levers(**{lever: -1})


@pytest.mark.gpu
def test_refusals(gpu):
    from mbd_hip import _capi
    from mbd_hip.envs import get_env
    from mbd_hip.planners.mbd_planner import Sweep
    lib = _capi.load()
    env = get_env("hopper")
    a = _args("hopper", 64, H=10, Nd=5)
    P = 2
    keys = (C.c_uint32 * (2 * P))(0, 1, 0, 2)

    def run(sw, **kw):
        mc = _capi.MpcConfig(n_ticks=2, warm_steps=2, exec_steps=1)
        for k, v in kw.items():
            if k == "reserved":
                mc.reserved[v] = 1
            else:
                setattr(mc, k, v)
        return lib.mbd_sweep_run_mpc(sw.h, C.byref(mc), keys, None, None, None, None, None), lib.mbd_last_error()
    sw = Sweep(env, a, P)
    for k in range(P):
        sw.set_state0(k, env.reset(gpu.prng_key(k)))
    assert run(sw)[0] == _capi.MBD_OK
    for kw, field in (({"n_ticks": 0}, b"n_ticks"), ({"warm_steps": 0}, b"warm_steps"), ({"warm_steps": 5}, b"warm_steps"),
                      ({"exec_steps": 0}, b"exec_steps"), ({"exec_steps": 10}, b"exec_steps"), ({"reserved": 4}, b"reserved")):
        rc, msg = run(sw, **kw)
        assert rc == _capi.MBD_ERR_INVALID and field in msg, (kw, msg)
    assert run(sw, n_ticks=1, warm_steps=1)[0] == _capi.MBD_OK  # (the bounds themselves)
    assert run(sw, warm_steps=4, exec_steps=9)[0] == _capi.MBD_OK
    sw.close()
    pi = Sweep(env, a, P, update_method=1)
    rc, msg = run(pi)
    assert rc == _capi.MBD_ERR_UNSUPPORTED and b"update_method" in msg
    pi.close()
    track = get_env("humanoidtrack")
    d = _args("humanoidtrack", 16, H=50, Nd=5)
    d.enable_demo = True
    demo = Sweep(track, d, P)
    rc, msg = run(demo)
    assert rc == _capi.MBD_ERR_UNSUPPORTED and b"enable_demo" in msg
    demo.close()


def _cli(tmp_path, *extra):
    pkg = os.path.join(ROOT, "model-based-diffusion_amd")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([pkg, ROOT, os.environ.get("PYTHONPATH", "")]))
    out = subprocess.run([sys.executable, "-m", "mbd_hip.planners.mpc", "--env_name", "hopper", "--disable_recommended_params",
                          "--Nsample", "128", "--Hsample", "20", "--Ndiffuse", "10", "--n_ticks", "4", "--warm_steps", "3",
                          "--exec_steps", "2", *extra], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1]), np.load(os.path.join(tmp_path, "results", "hopper", "mpc_episode.npz"))


_SINGLE_KEYS = {"env", "Nsample", "Hsample", "Ndiffuse", "n_ticks", "warm_steps", "exec_steps", "ms_per_tick", "ticks_per_s",
                "ms_per_diffusion_step", "open_loop_ms_per_diffusion_step", "boundary_ms_per_tick", "real_time_factor",
                "episode_reward"}


@pytest.mark.gpu
def test_command_line(gpu, tmp_path):
    res, ep = _cli(tmp_path, "--n_episodes", "3")
    for k in _SINGLE_KEYS | {"n_episodes", "episode_rewards", "episode_reward_mean", "episode_reward_std", "episode_ticks_per_s",
                             "sequential_episode_seconds"}:
        assert k in res, k
    assert res["env"] == "hopper" and res["n_ticks"] == 4 and res["n_episodes"] == 3 and res["ms_per_tick"] > 0
    assert len(res["episode_rewards"]) == 3 and np.isfinite(res["episode_rewards"]).all()
    assert np.isclose(res["episode_reward_mean"], np.mean(res["episode_rewards"]))
    assert np.isclose(res["episode_reward_std"], np.std(res["episode_rewards"]))
    assert np.isclose(res["episode_ticks_per_s"], 3 * res["ticks_per_s"]) and res["sequential_episode_seconds"] > 0
    assert np.isfinite(res["open_loop_ms_per_diffusion_step"]) and np.isfinite(res["boundary_ms_per_tick"])
    assert ep["actions"].shape == (3, 8, 3) and ep["rewards"].shape == (3, 8) and ep["states"].shape[:2] == (3, 5)
    assert ep["means"].shape == (3, 4, 20, 3)


@pytest.mark.gpu
def test_command_line_with_one_episode_is_the_single_path(gpu, tmp_path):
    res, ep = _cli(tmp_path, "--n_episodes", "1")
    assert set(res) == _SINGLE_KEYS
    assert ep["actions"].shape == (8, 3) and ep["rewards"].shape == (8,) and ep["states"].shape[0] == 5
    assert ep["means"].shape == (4, 20, 3)


@pytest.mark.gpu
def test_run_mpc_batch_of_one_is_run_mpc(gpu):
    from mbd_hip.planners.mpc import run_mpc, run_mpc_batch
    a = _args("hopper", 128, H=20, Nd=10, K=3, E=2, seed=5)
    rew, det = run_mpc(replace(a), return_details=True)
    rews, dets = run_mpc_batch([replace(a)], return_details=True)
    assert len(rews) == 1 and np.float32(rews[0]) == np.float32(rew)
    _same_episode(dets[0], det, "a batch of one")
    assert np.array_equal(dets[0]["key"], det["key"])
