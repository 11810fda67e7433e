"""Receding-horizon episodes (include/mbd_hip.h mbd_plan_run_mpc, mbd_hip.planners.mpc).

Without a GPU: the entry point is exported and refuses NULL arguments before touching a device, and the checker's
restatement (tests/mpc_checker.py) keeps the semantics' consequences — tick 0 is the cold plan, episodes are prefixes of
longer ones, the shift is the definition.  With a GPU (-m gpu): whole episodes bit for bit against that restatement, the
episode against the library's own open-loop runs, the test levers, the refusals and the command line."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mpc_checker
from conftest import ROOT, load_model


def _oenv_cpu(orc, name):
    from oracle.planner import OracleEnv
    if name == "car2d":
        return OracleEnv(orc, "car2d")
    m = load_model(name)
    return OracleEnv(orc, name, m.to_struct(), init_q=m.init_q)


# ---- without a GPU ------------------------------------------------------------------------------------------------------

def test_run_mpc_is_exported_and_refuses_null_arguments_before_any_device_access(lib):
    from mbd_hip import _capi
    assert "mbd_plan_run_mpc" in _capi.EXPORTS and hasattr(lib, "mbd_plan_run_mpc")
    mc = _capi.MpcConfig(n_ticks=2, warm_steps=1, exec_steps=1)
    key = _capi.key_array([0, 42])
    stand_in = C.create_string_buffer(1 << 16)  # a non-NULL handle the call must not reach: its config or key is NULL
    for args, field in (((None, C.byref(mc), key), b"plan"), ((stand_in, None, key), b"config"),
                        ((stand_in, C.byref(mc), None), b"key")):
        assert lib.mbd_plan_run_mpc(*args, None, None, None, None, None) == _capi.MBD_ERR_INVALID
        assert field in lib.mbd_last_error()


def test_checker_tick0_is_the_cold_reverse_loop(orc):
    """Tick 0 of an episode is oracle.planner's reverse loop (mbd_planner.py:138-148) from k_0 = split(key)[1], bit for bit."""
    from oracle import planner as op
    oe = _oenv_cpu(orc, "hopper")
    N, H, Nd, temp = 32, 12, 8, 0.1
    s0 = oe.reset(orc.split(orc.prng_key(5), 2, 1)[1], 1)
    key = orc.prng_key(9)
    ep = mpc_checker.episode(oe, s0, key, N, H, Nd, temp, T=2, K=3, E=1)
    r, Y = orc.split(key, 2, 1)[1], np.zeros((H, oe.Nu), np.float32)
    sched = orc.schedule(1e-4, 1e-2, Nd)
    for i in range(Nd - 1, 0, -1):
        r, Y, _, _ = op.reverse_once(orc, oe, s0, i, r, Y, sched, N, H, temp, 1)
    assert np.array_equal(ep["means"][0], Y)
    assert np.array_equal(ep["actions"][:1], Y[:1]) and np.array_equal(ep["states"][0], s0.reshape(-1))
    s1, r0 = orc.env_step(oe.ms, s0, Y[0])  # the executed row through the env's step
    assert np.array_equal(ep["states"][1], s1.reshape(-1)) and np.float32(ep["rewards"][0]) == np.float32(r0)
    assert not np.array_equal(ep["means"][1], ep["means"][0])


@pytest.mark.parametrize("name", ["hopper", "car2d"])
def test_checker_episode_is_a_prefix_of_a_longer_one(orc, name):
    oe = _oenv_cpu(orc, name)
    N, H, Nd, K, E = 16, 10, 6, 2, 2
    s0 = oe.reset(orc.split(orc.prng_key(1), 2, 1)[1], 1)
    key = orc.prng_key(4)
    short = mpc_checker.episode(oe, s0, key, N, H, Nd, 0.1, T=3, K=K, E=E)
    long = mpc_checker.episode(oe, s0, key, N, H, Nd, 0.1, T=6, K=K, E=E)
    assert short["actions"].shape == (3 * E, oe.Nu) and short["states"].shape[0] == 4
    for k, v in short.items():
        assert np.array_equal(v, long[k][: len(v)]), k


def test_checker_shift_is_the_definition():
    H, Nu = 7, 3
    M = np.arange(H * Nu, dtype=np.float32).reshape(H, Nu) + 1
    for E in (1, H - 1):
        got = mpc_checker.shift(M, E)
        want = np.array([[M[h + E, u] if h < H - E else 0.0 for u in range(Nu)] for h in range(H)], np.float32)
        assert np.array_equal(got, want), E
    assert np.array_equal(mpc_checker.shift(M, H - 1)[0], M[-1])


# ---- on the GPU ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu(lib):
    from mbd_hip import _capi
    if _capi.device_count() < 1:
        pytest.fail("GPU tests need a visible MI355X; the product has no CPU fallback")
    return _capi


def _args(name, N, H=50, Nd=20, K=4, E=1, T=6, seed=0, temp=0.1):
    from mbd_hip.planners.mpc import MpcArgs
    return MpcArgs(seed=seed, env_name=name, Nsample=N, Hsample=H, Ndiffuse=Nd, temp_sample=temp, n_ticks=T, warm_steps=K,
                   exec_steps=E, disable_recommended_params=True, not_render=True)


def _same_episode(got, ref, what=""):
    T = len(ref["means"])
    first = next((t for t in range(T) if not np.array_equal(got["means"][t], ref["means"][t])), None)
    assert first is None, f"{what}: the means differ from tick {first} on"
    for k in ("actions", "rewards", "states"):
        g = np.asarray(got[k], np.float32).reshape(ref[k].shape)
        assert np.array_equal(g, ref[k]), f"{what}: {k} differ"


def _against_checker(orc, a):
    from mbd_hip.envs import get_env
    from mbd_hip.envs.base import prng_impl
    from mbd_hip.planners.mpc import run_mpc
    from test_gpu_parity import _oenv
    rew, det = run_mpc(a, return_details=True)
    env = get_env(a.env_name)
    ref = mpc_checker.episode(_oenv(orc, env), np.asarray(det["state_init"].pipeline_state, np.float32), det["key"],
                              a.Nsample, a.Hsample, a.Ndiffuse, a.temp_sample, a.n_ticks, a.warm_steps, a.exec_steps,
                              impl=prng_impl())
    _same_episode(det, ref, a.env_name)
    assert np.float32(rew) == np.float32(ref["rewards"].mean())
    assert det["states"].shape == (a.n_ticks + 1, ref["states"].shape[1])
    assert not np.array_equal(ref["states"][0], ref["states"][-1])


@pytest.mark.gpu
@pytest.mark.parametrize("name,N,E", [("humanoidrun", 256, 1), ("hopper", 512, 2), ("halfcheetah", 256, 1), ("ant", 256, 1),
                                      ("car2d", 256, 1)])
def test_episode_matches_the_checker(gpu, orc_omp, name, N, E):
    """humanoidrun N=256, H=50, Nd=20, K=4, E=1, T=6 and the other envs at those settings: actions, rewards, states and
    means of the whole episode, bit for bit."""
    _against_checker(orc_omp, _args(name, N, E=E, seed=3))


@pytest.mark.gpu
@pytest.mark.parametrize("N,Nd,K,T", [(1024, 100, 20, 12), (4096, 10, 3, 4)])
def test_episode_matches_the_checker_at_full_size(gpu, orc_omp, N, Nd, K, T):
    """The metric's plan size in closed loop (its rollouts leave CUs idle: the next step's normals ride in them across tick
    boundaries), and a plan that fills the chip (they come from the second stream)."""
    _against_checker(orc_omp, _args("humanoidrun", N, Nd=Nd, K=K, T=T, seed=1))


@pytest.mark.gpu
@pytest.mark.parametrize("N", [256, 4096])
def test_episode_against_the_open_loop_runs(gpu, N):
    """Self-comparisons of the library: tick 0 is mbd_plan_run(k_0)'s last mean; an episode of 3 ticks is a prefix of one of 6;
    after an episode the plan's mbd_plan_run equals a fresh plan's (its state0 is untouched).  N = 256: the episode of 6 ticks
    is a prefix of one of 9 run after both on the same plan — the plan's logs grow after their first use."""
    from mbd_hip.envs import get_env
    from mbd_hip.planners.mbd_planner import Plan
    a = _args("humanoidrun", N, Nd=12, K=3)
    env = get_env("humanoidrun")
    st = env.reset(gpu.prng_key(7))
    key = gpu.prng_key(8)
    plan = Plan(env, a)
    plan.set_state0(st)
    long = plan.run_mpc(key, 6, 3, 2)
    short = plan.run_mpc(key, 3, 3, 2)
    for k in ("actions", "rewards", "states", "means"):
        assert np.array_equal(short[k], long[k][: len(short[k])]), k
    assert np.array_equal(long["states"][0], np.asarray(st.pipeline_state, np.float32).reshape(-1))
    if N == 256:
        longer = plan.run_mpc(key, 9, 3, 2)
        for k in ("actions", "rewards", "states", "means"):
            assert len(longer[k]) > len(long[k]) and np.array_equal(long[k], longer[k][: len(long[k])]), k
    mu_after, rm_after, rf_after, _ = plan.run(key)
    fresh = Plan(env, a)
    fresh.set_state0(st)
    mu, rm, rf, _ = fresh.run(key)
    assert np.array_equal(mu_after, mu) and np.array_equal(rm_after, rm) and np.float32(rf_after) == np.float32(rf)
    mu0, _, _, _ = fresh.run(gpu.prng_split(key, 2, fresh.cfg.prng_impl)[1])
    assert np.array_equal(long["means"][0], mu0[-1])
    plan.close()
    fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1024, 4096])
@pytest.mark.parametrize("lever", ["MBD_NO_PREFETCH", "MBD_NO_FUSED_NOISE", "MBD_NO_FUSED_SCORE", "MBD_NO_LAZY"])
def test_episode_is_the_same_under_every_lever(gpu, levers, lever, N):
    from mbd_hip.envs import get_env
    from mbd_hip.planners.mbd_planner import Plan
    a = _args("humanoidrun", N, Nd=10, K=3)
    env = get_env("humanoidrun")
    st = env.reset(gpu.prng_key(2))
    key = gpu.prng_key(6)

    def episode():
        plan = Plan(env, a)  # (after the lever: MBD_NO_LAZY acts on plans created from then on)
        plan.set_state0(st)
        out = plan.run_mpc(key, 5, 3, 1)
        plan.close()
        return out
    ref = episode()
    levers(**{lever: 1})
    _same_episode(episode(), ref, lever)


@pytest.mark.gpu
def test_refusals(gpu):
    from mbd_hip import _capi
    from mbd_hip.envs import get_env
    from mbd_hip.planners.mbd_planner import Plan
    lib = _capi.load()
    env = get_env("hopper")
    a = _args("hopper", 64, H=10, Nd=5)
    plan = Plan(env, a)
    key = _capi.key_array([0, 1])

    def run(p, **kw):
        mc = _capi.MpcConfig(n_ticks=2, warm_steps=2, exec_steps=1)
        for k, v in kw.items():
            if k == "reserved":
                mc.reserved[v] = 1
            else:
                setattr(mc, k, v)
        return lib.mbd_plan_run_mpc(p.h, C.byref(mc), key, None, None, None, None, None), lib.mbd_last_error()
    assert run(plan)[0] == _capi.MBD_OK
    for kw, field in (({"n_ticks": 0}, b"n_ticks"), ({"warm_steps": 0}, b"warm_steps"), ({"warm_steps": 5}, b"warm_steps"),
                      ({"exec_steps": 0}, b"exec_steps"), ({"exec_steps": 10}, b"exec_steps"), ({"reserved": 4}, b"reserved")):
        rc, msg = run(plan, **kw)
        assert rc == _capi.MBD_ERR_INVALID and field in msg, (kw, msg)
    assert run(plan, warm_steps=4, exec_steps=9)[0] == _capi.MBD_OK  # (the bounds themselves)
    rc, msg = run(Plan(env, a, update_method=1))
    assert rc == _capi.MBD_ERR_UNSUPPORTED and b"update_method" in msg
    rc, msg = run(Plan(env, a, shard_begin=0, shard_count=32))
    assert rc == _capi.MBD_ERR_STATE and b"shard" in msg
    car = get_env("car2d")
    demo = _args("car2d", 16, H=50, Nd=5)
    demo.enable_demo = True
    rc, msg = run(Plan(car, demo))
    assert rc == _capi.MBD_ERR_UNSUPPORTED and b"enable_demo" in msg
    plan.close()


@pytest.mark.gpu
def test_command_line(gpu, tmp_path):
    pkg = os.path.join(ROOT, "model-based-diffusion_amd")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([pkg, ROOT, os.environ.get("PYTHONPATH", "")]))
    out = subprocess.run([sys.executable, "-m", "mbd_hip.planners.mpc", "--env_name", "hopper", "--disable_recommended_params",
                          "--Nsample", "128", "--Hsample", "20", "--Ndiffuse", "10", "--n_ticks", "4", "--warm_steps", "3",
                          "--exec_steps", "2"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    for k in ("env", "Nsample", "Hsample", "Ndiffuse", "n_ticks", "warm_steps", "exec_steps", "ms_per_tick", "ticks_per_s",
              "ms_per_diffusion_step", "real_time_factor", "episode_reward"):
        assert k in res, k
    assert res["env"] == "hopper" and res["n_ticks"] == 4 and res["ms_per_tick"] > 0 and np.isfinite(res["episode_reward"])
    ep = np.load(os.path.join(tmp_path, "results", "hopper", "mpc_episode.npz"))
    assert ep["actions"].shape == (8, 3) and ep["states"].shape[0] == 5
