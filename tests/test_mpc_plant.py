"""Receding-horizon episodes on a perturbed, disturbed plant (include/mbd_hip.h mbd_mpc_plant, mbd_plan_set_mpc_plant,
mbd_sweep_set_mpc_plant; mbd_hip.model.Model.scaled; mbd_hip.planners.mpc's plant settings; DESIGN.md section 1 "N5 plant").

Without a GPU: the two setters are exported and refuse a NULL handle before touching a device, the ctypes record has the
header's layout, Model.scaled scales what it says and nothing else, and the checker's restatement (tests/mpc_plant_checker.py)
keeps the semantics' consequences — a record without disturbances is no record, episodes are prefixes of longer ones, tick 0
does not see the record, kicks come every kick_every-th tick and leave a planar model's y alone.  With a GPU (-m gpu): whole
episodes bit for bit against that restatement, identity against the episode without a record, batched = single, the test
levers, the refusals and the command line.  Every comparison is np.array_equal."""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
from dataclasses import replace

import numpy as np
import pytest

import mpc_checker
import mpc_plant_checker
from conftest import ROOT, load_model

# the perturbation and the disturbances of the issue's item 4
MISMATCH = dict(mass=1.3, friction=0.5, gear=0.8)
DISTURB = dict(act_std=0.3, kick_std=0.5, kick_every=3)
_LOGS = ("means", "actions", "rewards", "states")


def _oenv_cpu(orc, name, **scale):
    from oracle.planner import OracleEnv
    if name == "car2d":
        return OracleEnv(orc, "car2d")
    m = load_model(name).scaled(**scale)
    return OracleEnv(orc, name, m.to_struct(), init_q=m.init_q)


def _reset(orc, oe, seed):
    return np.asarray(oe.reset(orc.split(orc.prng_key(seed), 2, 1)[1], 1), np.float32)


def _equal(a, b, what=""):
    for k in _LOGS:
        x, y = np.asarray(a[k], np.float32), np.asarray(b[k], np.float32)
        assert x.size == y.size and np.array_equal(x.reshape(y.shape), y), f"{what}: {k} differ"


# ---- without a GPU ------------------------------------------------------------------------------------------------------

def test_setters_are_exported_and_refuse_null_handles_before_any_device_access(lib):
    from mbd_hip import _capi
    for name in ("mbd_plan_set_mpc_plant", "mbd_sweep_set_mpc_plant"):
        assert name in _capi.EXPORTS and hasattr(lib, name), name
    rec = _capi.MpcPlant(act_std=0.1, kick_every=1)
    assert lib.mbd_plan_set_mpc_plant(None, C.byref(rec)) == _capi.MBD_ERR_INVALID
    assert b"plan" in lib.mbd_last_error()
    assert lib.mbd_sweep_set_mpc_plant(None, 0, C.byref(rec)) == _capi.MBD_ERR_INVALID
    assert b"sweep" in lib.mbd_last_error()
    stand_in = C.create_string_buffer(1 << 16)  # a zeroed stand-in for a sweep of no episodes: every k is out of range
    for k in (0, -1, 32):
        assert lib.mbd_sweep_set_mpc_plant(stand_in, k, C.byref(rec)) == _capi.MBD_ERR_INVALID
        assert b"k=" in lib.mbd_last_error()


def test_the_ctypes_record_has_the_headers_layout(tmp_path):
    from mbd_hip import _capi
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a C compiler is what builds the checker as well"
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mbd_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(mbd_mpc_plant), offsetof(mbd_mpc_plant, plant), '
                   'offsetof(mbd_mpc_plant, key), offsetof(mbd_mpc_plant, act_std), offsetof(mbd_mpc_plant, kick_std), '
                   'offsetof(mbd_mpc_plant, kick_every), offsetof(mbd_mpc_plant, reserved)); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    P = _capi.MpcPlant
    assert got == [C.sizeof(P), P.plant.offset, P.key.offset, P.act_std.offset, P.kick_std.offset, P.kick_every.offset,
                   P.reserved.offset]


def test_model_scaled(orc):
    m = load_model("hopper")
    same = m.scaled()
    assert bytes(same.to_struct()) == bytes(m.to_struct())
    assert set(same.fields) == set(m.fields)
    for k, v in m.fields.items():
        assert np.array_equal(np.asarray(same.fields[k]), np.asarray(v)), k
    heavy = m.scaled(mass=2)
    assert np.array_equal(heavy.fields["inv_mass"], np.asarray(m.fields["inv_mass"], np.float32) / np.float32(2))
    assert np.array_equal(heavy.fields["inv_inertia"], np.asarray(m.fields["inv_inertia"], np.float32) / np.float32(2))
    assert np.asarray(heavy.fields["inv_inertia"]).any()
    for k, v in m.fields.items():
        if k not in ("inv_mass", "inv_inertia"):
            assert np.array_equal(np.asarray(heavy.fields[k]), np.asarray(v)), k
    other = m.scaled(friction=0.5, gear=0.8)
    assert np.float32(other.fields["friction"]) == np.float32(m.fields["friction"]) * np.float32(0.5)
    assert np.array_equal(other.fields["act_gear"], np.asarray(m.fields["act_gear"], np.float32) * np.float32(0.8))
    for k, v in m.fields.items():
        if k not in ("friction", "act_gear"):
            assert np.array_equal(np.asarray(other.fields[k]), np.asarray(v)), k
    assert (heavy.link_names, heavy.actuator_names, heavy.env_name) == (m.link_names, m.actuator_names, m.env_name)
    with pytest.raises(ValueError, match="mass"):
        m.scaled(mass=0)
    # the scaled model is a model: the checker's forward kinematics and one env step on it are finite, and it is another system
    full = m.scaled(**MISMATCH)
    s0 = orc.forward(full.to_struct(), full.init_q, np.zeros(full.qd_size(), np.float32))
    assert np.array_equal(s0, orc.forward(m.to_struct(), m.init_q, np.zeros(m.qd_size(), np.float32)))
    a = np.full(m.act_size(), 0.7, np.float32)
    s1, r1 = orc.env_step(full.to_struct(), s0, a)
    s1n, _ = orc.env_step(m.to_struct(), s0, a)
    assert np.isfinite(s1).all() and np.isfinite(r1) and not np.array_equal(s1, s1n)


@pytest.mark.parametrize("name", ["hopper", "car2d"])
def test_checker_record_without_disturbances_is_no_record(orc, name):
    """plant = the env itself or a second OracleEnv of the same model, stds 0, any key: mpc_checker.episode's four outputs."""
    oe = _oenv_cpu(orc, name)
    N, H, Nd, K, E, T = 16, 10, 6, 2, 2, 4
    s0 = _reset(orc, oe, 1)
    key = orc.prng_key(4)
    ref = mpc_checker.episode(oe, s0, key, N, H, Nd, 0.1, T, K, E)
    for plant, dkey in ((None, (0, 0)), (oe, orc.prng_key(77)), (_oenv_cpu(orc, name), orc.prng_key(5))):
        got = mpc_plant_checker.episode(oe, s0, key, N, H, Nd, 0.1, T, K, E, plant=plant, dkey=dkey)
        _equal(got, ref, name)
    # kick_every alone switches nothing on
    _equal(mpc_plant_checker.episode(oe, s0, key, N, H, Nd, 0.1, T, K, E, kick_every=2), ref, name)


@pytest.mark.parametrize("seed", [0, 1])
def test_checker_disturbed_episode(orc_omp, seed):
    """hopper with the mismatch and the disturbances of the issue: T ticks are a prefix of T + 3; tick 0's mean does not depend
    on the record; every state from tick 1 on differs from the nominal episode's and is finite; with kick_every = 3 the states
    of ticks 1 and 2 are the plant's rollout of the logged rows and tick 3's is that plus a kick."""
    orc = orc_omp
    oe, plant = _oenv_cpu(orc, "hopper"), _oenv_cpu(orc, "hopper", **MISMATCH)
    N, H, Nd, K, E, Nu = 128, 20, 16, 4, 1, 3
    s0 = _reset(orc, oe, seed)
    key, dkey = orc.prng_key(10 + seed), orc.prng_key(20 + seed)
    run = lambda T, **kw: mpc_plant_checker.episode(oe, s0, key, N, H, Nd, 0.1, T, K, E, **kw)  # noqa: E731
    long = run(9, plant=plant, dkey=dkey, **DISTURB)
    short = run(6, plant=plant, dkey=dkey, **DISTURB)
    for k, v in short.items():
        assert np.array_equal(v, long[k][: len(v)]), k
    nominal = mpc_checker.episode(oe, s0, key, N, H, Nd, 0.1, 9, K, E)
    assert np.array_equal(long["means"][0], nominal["means"][0])
    assert np.array_equal(long["states"][0], nominal["states"][0])
    assert np.isfinite(long["states"]).all() and np.isfinite(long["rewards"]).all()
    for t in range(1, 10):
        assert not np.array_equal(long["states"][t], nominal["states"][t]), t
    assert not np.array_equal(long["actions"][0], long["means"][0][:E])  # (the action noise)
    dk = dkey
    for t in range(9):
        rew, s = mpc_checker.execute(plant, long["states"][t], long["actions"][t * E:(t + 1) * E])
        assert np.array_equal(rew, long["rewards"][t * E:(t + 1) * E])
        dk, eps = mpc_plant_checker.disturbances(orc, dk, E, Nu, 1)
        assert eps.shape == (E * Nu + 3,)
        assert np.array_equal(long["actions"][t * E:(t + 1) * E],
                              long["means"][t][:E] + (np.float32(0.3) * eps[: E * Nu]).reshape(E, Nu))
        if (t + 1) % 3:
            assert np.array_equal(s, long["states"][t + 1]), t
        else:
            assert not np.array_equal(s, long["states"][t + 1]), t
            s[7] += np.float32(0.5) * eps[E * Nu]
            s[9] += np.float32(0.5) * eps[E * Nu + 2]
            assert np.array_equal(s, long["states"][t + 1]), t
    # another disturbance key is another episode; the same one the same
    assert not np.array_equal(run(3, plant=plant, dkey=orc.prng_key(99), **DISTURB)["states"], long["states"][:4])


@pytest.mark.parametrize("name,moved", [("hopper", (True, False, True)), ("humanoidrun", (True, True, True))])
def test_checker_kick_leaves_a_planar_models_y_alone(orc, name, moved):
    oe = _oenv_cpu(orc, name)
    N, H, Nd, K, E = 8, 6, 3, 1, 1
    s0 = _reset(orc, oe, 2)
    ep = mpc_plant_checker.episode(oe, s0, orc.prng_key(1), N, H, Nd, 0.1, 1, K, E, dkey=orc.prng_key(3), kick_std=0.5)
    _, s1 = mpc_checker.execute(oe, s0, ep["actions"][:E])
    got = ep["states"][1]
    assert [bool(got[7 + j] != s1[7 + j]) for j in range(3)] == list(moved)
    rest = np.ones(got.size, bool)
    rest[7:10] = False
    assert np.array_equal(got[rest], s1[rest])
    assert np.array_equal(ep["actions"][:E], ep["means"][0][:E])  # (no action noise asked for)


def test_batch_arguments_may_differ_in_the_plant_settings(monkeypatch):
    """_check_batch lets the plant settings differ between the episodes of a batch, and still nothing else."""
    from mbd_hip.planners import mpc
    a = mpc.MpcArgs(env_name="hopper", Nsample=64, Hsample=20, Ndiffuse=6, n_ticks=3, warm_steps=2,
                    disable_recommended_params=True, not_render=True)
    assert not mpc._has_plant(a) and mpc._has_plant(replace(a, act_noise_std=0.1)) and mpc._has_plant(replace(a, disturb_seed=1))
    mpc._check_batch([a, replace(a, seed=1, plant_mass=1.3, plant_friction=0.5, plant_gear=0.8, act_noise_std=0.2, kick_std=0.1,
                                 kick_every=2, disturb_seed=7)])
    with pytest.raises(ValueError, match="Hsample"):
        mpc._check_batch([a, replace(a, plant_mass=1.3, Hsample=21)])


# ---- on the GPU ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu(lib):
    from mbd_hip import _capi
    if _capi.device_count() < 1:
        pytest.fail("GPU tests need a visible MI355X; the product has no CPU fallback")
    return _capi


def _args(name, N, H=50, Nd=20, K=4, E=1, T=6, seed=0, temp=0.1, **kw):
    from mbd_hip.planners.mpc import MpcArgs
    return MpcArgs(seed=seed, env_name=name, Nsample=N, Hsample=H, Ndiffuse=Nd, temp_sample=temp, n_ticks=T, warm_steps=K,
                   exec_steps=E, disable_recommended_params=True, not_render=True, **kw)


def _full(name, N, **kw):
    """The issue's settings: every mismatch and every disturbance at once (car2d: the action noise only)."""
    if name == "car2d":
        return _args(name, N, act_noise_std=0.3, disturb_seed=11, **kw)
    return _args(name, N, plant_mass=1.3, plant_friction=0.5, plant_gear=0.8, act_noise_std=0.3, kick_std=0.5, kick_every=3,
                 disturb_seed=11, **kw)


def _plant_env(env, a):
    from mbd_hip.envs.base import RigidBodyEnv
    if (a.plant_mass, a.plant_friction, a.plant_gear) == (1.0, 1.0, 1.0):
        return None
    return RigidBodyEnv(a.env_name, model=env.sys.scaled(a.plant_mass, a.plant_friction, a.plant_gear))


def _checker_episode(orc, env, a, det):
    from mbd_hip import _capi
    from mbd_hip.envs.base import prng_impl
    from test_gpu_parity import _oenv
    plant = _plant_env(env, a)
    return mpc_plant_checker.episode(
        _oenv(orc, env), np.asarray(det["state_init"].pipeline_state, np.float32), det["key"], a.Nsample, a.Hsample, a.Ndiffuse,
        a.temp_sample, a.n_ticks, a.warm_steps, a.exec_steps, plant=None if plant is None else _oenv(orc, plant),
        dkey=_capi.prng_key(a.disturb_seed), act_std=a.act_noise_std, kick_std=a.kick_std, kick_every=a.kick_every,
        impl=prng_impl())


def _against_checker(orc, a):
    from mbd_hip.envs import get_env
    from mbd_hip.planners.mpc import run_mpc
    rew, det = run_mpc(replace(a), return_details=True)
    ref = _checker_episode(orc, get_env(a.env_name), a, det)
    _equal(det, ref, a.env_name)
    assert np.float32(rew) == np.float32(ref["rewards"].mean())
    assert det["plant_mass"] == a.plant_mass and det["act_noise_std"] == a.act_noise_std
    E = a.exec_steps
    assert not np.array_equal(ref["actions"][:E], ref["means"][0][:E])  # (the episode was disturbed)
    return det, ref


@pytest.mark.gpu
@pytest.mark.parametrize("name,N,E", [("humanoidrun", 256, 1), ("hopper", 512, 2), ("halfcheetah", 256, 1), ("ant", 256, 1),
                                      ("car2d", 256, 1)])
def test_disturbed_episode_matches_the_checker(gpu, orc_omp, name, N, E):
    """The grid of test_mpc.py's test_episode_matches_the_checker (H=50, Nd=20, K=4, T=6) with mass 1.3, friction 0.5, gear 0.8,
    act_std 0.3, kick_std 0.5 every 3 ticks (car2d: act_std only): actions, rewards, states and means, bit for bit.  hopper's
    E Nu + 3 = 9 and ant's 11 are odd counts of normals."""
    det, ref = _against_checker(orc_omp, _full(name, N, E=E, seed=3))
    assert ref["states"].shape[0] == 7 and np.isfinite(ref["states"]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("N,Nd,K,T", [(1024, 100, 20, 12), (4096, 10, 3, 4)])
def test_disturbed_episode_matches_the_checker_at_full_size(gpu, orc_omp, N, Nd, K, T):
    """The metric's plan size (the next step's normals ride in the rollouts' spare workgroups across tick boundaries) and a plan
    that fills the chip (they come from the second stream)."""
    _against_checker(orc_omp, _full("humanoidrun", N, Nd=Nd, K=K, T=T, seed=1))


@pytest.mark.gpu
@pytest.mark.parametrize("name,N", [("humanoidrun", 256), ("hopper", 512), ("car2d", 256)])
def test_record_without_disturbances_is_no_record(gpu, name, N):
    """A record with zeros — plant NULL, or a second env of the same name — gives the episode without a record (which
    tests/test_mpc.py holds to the checker), any key; after clear again; and an episode with a record leaves the plan as an
    episode without one does: Plan.run equals a fresh plan's."""
    from mbd_hip.envs import get_env
    from mbd_hip.planners.mbd_planner import Plan
    a = _args(name, N, Nd=12, K=3)
    env = get_env(name)
    st = env.reset(gpu.prng_key(7))
    key = gpu.prng_key(8)
    plan = Plan(env, a)
    plan.set_state0(st)
    ref = plan.run_mpc(key, 5, 3, 2)
    plan.set_mpc_plant(key=gpu.prng_key(123))
    _equal(plan.run_mpc(key, 5, 3, 2), ref, "plant NULL")
    plan.set_mpc_plant(env=get_env(name), key=gpu.prng_key(5), kick_every=2)
    _equal(plan.run_mpc(key, 5, 3, 2), ref, "a second env")
    plan.set_mpc_plant(act_std=0.2, key=gpu.prng_key(5))
    noisy = plan.run_mpc(key, 5, 3, 2)
    assert np.array_equal(noisy["means"][0], ref["means"][0]) and not np.array_equal(noisy["actions"], ref["actions"])
    assert not np.array_equal(noisy["states"][1], ref["states"][1])
    short = plan.run_mpc(key, 3, 3, 2)
    for k in _LOGS:
        assert np.array_equal(short[k], noisy[k][: len(short[k])]), k
    after = plan.run(key)  # (run ignores the record; the plan's state0 came back)
    plan.clear_mpc_plant()
    _equal(plan.run_mpc(key, 5, 3, 2), ref, "after clear")
    fresh = Plan(env, a)
    fresh.set_state0(st)
    want = fresh.run(key)
    for x, y in zip(after[:3], want[:3]):
        assert np.array_equal(np.asarray(x, np.float32), np.asarray(y, np.float32))
    mu0 = fresh.run(gpu.prng_split(key, 2, fresh.cfg.prng_impl)[1])[0]
    assert np.array_equal(noisy["means"][0], mu0[-1])
    plan.close()
    fresh.close()


@pytest.mark.gpu
def test_the_disturbed_episodes_buffers_grow_after_their_first_use(gpu):
    """hopper with action noise and a kick every second tick: 3 ticks of one executed row, then 7 ticks of two on the same
    plan — the log of the executed rows and the tick's normals both grow behind their first use.  Each episode equals the
    one a fresh plan runs."""
    from mbd_hip.envs import get_env
    from mbd_hip.planners.mbd_planner import Plan
    a = _args("hopper", 256, Nd=12, K=3)
    env = get_env("hopper")
    st = env.reset(gpu.prng_key(7))
    key = gpu.prng_key(8)
    rec = dict(act_std=0.3, kick_std=0.5, kick_every=2, key=gpu.prng_key(5))

    def plan():
        p = Plan(env, a)
        p.set_state0(st)
        p.set_mpc_plant(**rec)
        return p
    grown = plan()
    episodes = [grown.run_mpc(key, 3, 3, 1), grown.run_mpc(key, 7, 3, 2)]
    grown.close()
    for got, (T, E) in zip(episodes, ((3, 1), (7, 2))):
        fresh = plan()
        _equal(got, fresh.run_mpc(key, T, 3, E), f"T={T} E={E}")
        fresh.close()
        assert got["states"].shape[0] == T + 1 and not np.array_equal(got["actions"][:E], got["means"][0][:E])
    assert episodes[1]["actions"].size > episodes[0]["actions"].size


def _records(gpu, env, P):
    """Three distinct plants in the order A, A, B, none, C, C, A, B: runs of equal handles, a gap, different keys and stds."""
    from mbd_hip.envs.base import RigidBodyEnv
    plants = dict(A=RigidBodyEnv(env.env_name, model=env.sys.scaled(mass=1.3)),
                  B=RigidBodyEnv(env.env_name, model=env.sys.scaled(friction=0.5, gear=0.8)),
                  C=RigidBodyEnv(env.env_name, model=env.sys.scaled(**MISMATCH)))
    recs = []
    for k, which in enumerate("AAB.CCAB"[:P]):
        if which == ".":
            recs.append(None)
        else:
            recs.append(dict(env=plants[which], key=gpu.prng_key(300 + k), act_std=(0.0, 0.3, 0.1)[k % 3],
                             kick_std=(0.5, 0.0, 0.2, 0.4)[k % 4], kick_every=1 + k % 3))
    return recs


@pytest.mark.gpu
@pytest.mark.parametrize("name,N", [("humanoidrun", 256), ("hopper", 512)])
@pytest.mark.parametrize("P", [1, 3, 8])
def test_batch_equals_the_single_episodes(gpu, name, N, P):
    """Episode k of a sweep with record k equals Plan.run_mpc on a plan of its own with that record (held to the checker by
    test_disturbed_episode_matches_the_checker), whatever the other episodes carry."""
    from mbd_hip.envs import get_env
    from mbd_hip.planners.mbd_planner import Plan, Sweep
    a = _args(name, N, Nd=12)
    env = get_env(name)
    T, K, E = 6, 3, 2
    recs = _records(gpu, env, P)
    keys = np.array([gpu.prng_key(100 + k) for k in range(P)], np.uint32)
    states = [env.reset(gpu.prng_key(k)) for k in range(P)]
    sw = Sweep(env, a, P)
    for k in range(P):
        sw.set_state0(k, states[k])
        if recs[k] is not None:
            sw.set_mpc_plant(k, **recs[k])
    batch = sw.run_mpc(keys, T, K, E)
    after = sw.run(keys)  # (run ignores the records; the start states are untouched)
    singles = []
    for k in range(P):
        plan = Plan(env, a)
        plan.set_state0(states[k])
        if recs[k] is not None:
            plan.set_mpc_plant(**recs[k])
        singles.append(plan.run_mpc(keys[k], T, K, E))
        plan.close()
        _equal({f: batch[f][k] for f in _LOGS}, singles[k], f"episode {k} of {P}")
    for k in range(P):
        sw.clear_mpc_plant(k)
    cleared = sw.run_mpc(keys, T, K, E)
    sw.close()
    fresh = Sweep(env, a, P)
    for k in range(P):
        fresh.set_state0(k, states[k])
    want = fresh.run(keys)
    for x, y in zip(after[:3], want[:3]):
        assert np.array_equal(x, y)
    nominal = fresh.run_mpc(keys, T, K, E)
    fresh.close()
    for f in _LOGS:
        assert np.array_equal(cleared[f], nominal[f]), f
    if P > 3:
        _equal({f: batch[f][3] for f in _LOGS}, {f: nominal[f][3] for f in _LOGS}, "the episode without a record")
    assert not np.array_equal(batch["states"][0][1:], nominal["states"][0][1:])


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1024, 4096])
@pytest.mark.parametrize("lever", ["MBD_NO_PREFETCH", "MBD_NO_FUSED_NOISE", "MBD_NO_FUSED_SCORE", "MBD_NO_LAZY"])
def test_disturbed_episode_is_the_same_under_every_lever(gpu, levers, lever, N):
    from mbd_hip.envs import get_env
    from mbd_hip.envs.base import RigidBodyEnv
    from mbd_hip.planners.mbd_planner import Plan
    a = _args("humanoidrun", N, Nd=10, K=3)
    st = get_env("humanoidrun").reset(gpu.prng_key(2))
    key = gpu.prng_key(6)

    def episode():
        env = get_env("humanoidrun")
        plant = RigidBodyEnv("humanoidrun", model=env.sys.scaled(**MISMATCH))
        plan = Plan(env, a)  # (after the lever: MBD_NO_LAZY acts on plans created from then on)
        plan.set_state0(st)
        plan.set_mpc_plant(env=plant, key=gpu.prng_key(9), **DISTURB)
        out = plan.run_mpc(key, 6, 3, 1)
        plan.close()
        return out
    ref = episode()
    levers(**{lever: 1})
    _equal(episode(), ref, lever)


def _one_actuator_fewer(m):
    """A copy of the model without its last actuator."""
    from mbd_hip.model import Model
    f = dict(m.fields)
    f["n_act"] = int(f["n_act"]) - 1
    for k in ("act_link", "act_slot", "act_gear", "act_lo", "act_hi"):
        f[k] = np.asarray(f[k])[: f["n_act"]].copy()
    return Model(f, m.link_names, m.actuator_names[: f["n_act"]], m.env_name)


def _not_planar(m):
    """A copy of a planar model with MBD_FLAG_PLANAR cleared: the same system through the general 3-D arithmetic."""
    from mbd_hip.model import FLAG_PLANAR, Model
    f = dict(m.fields)
    f["flags"] = int(f["flags"]) & ~FLAG_PLANAR
    return Model(f, m.link_names, m.actuator_names, m.env_name)


def test_the_mismatched_models_of_the_refusals_are_models(orc):
    """The two models test_refusals builds its action_size and planar cases from step on the checker like any model."""
    m = load_model("hopper")
    for other in (_one_actuator_fewer(m), _not_planar(m)):
        s0 = orc.forward(other.to_struct(), other.init_q, np.zeros(other.qd_size(), np.float32))
        s1, r1 = orc.env_step(other.to_struct(), s0, np.full(other.act_size(), 0.5, np.float32))
        assert np.isfinite(s1).all() and np.isfinite(r1)
        assert other.n_links == m.n_links


@pytest.mark.gpu
def test_refusals(gpu):
    from mbd_hip import _capi
    from mbd_hip.envs import get_env
    from mbd_hip.envs.base import RigidBodyEnv
    from mbd_hip.planners.mbd_planner import Plan, Sweep
    lib = _capi.load()
    env = get_env("hopper")
    a = _args("hopper", 64, H=10, Nd=5)
    plan, sweep = Plan(env, a), Sweep(env, a, 2)

    def rec(plant=None, **kw):
        r = _capi.MpcPlant(kick_every=1)
        r.plant = None if plant is None else plant.handle
        for k, v in kw.items():
            if k == "reserved":
                r.reserved[v] = 1
            else:
                setattr(r, k, v)
        return r

    def both(r):
        out = []
        for call in (lambda: lib.mbd_plan_set_mpc_plant(plan.h, C.byref(r)), lambda: lib.mbd_sweep_set_mpc_plant(sweep.h, 1, C.byref(r))):
            out.append((call(), lib.mbd_last_error()))
        return out
    for rc, _ in both(rec(act_std=0.5, kick_std=0.5, kick_every=4)):
        assert rc == _capi.MBD_OK
    for kw, field in (({"act_std": -0.1}, b"act_std"), ({"act_std": float("nan")}, b"act_std"), ({"act_std": float("inf")}, b"act_std"),
                      ({"kick_std": -1.0}, b"kick_std"), ({"kick_std": float("nan")}, b"kick_std"), ({"kick_every": 0}, b"kick_every"),
                      ({"kick_every": -3}, b"kick_every"), ({"reserved": 0}, b"reserved"), ({"reserved": 2}, b"reserved")):
        for rc, msg in both(rec(**kw)):
            assert rc == _capi.MBD_ERR_INVALID and field in msg, (kw, msg)
    # another topology: walker2d's seven links against hopper's four
    walker, car = get_env("walker2d"), get_env("car2d")  # (kept alive: a record does not own its plant)
    for rc, msg in both(rec(walker)):
        assert rc == _capi.MBD_ERR_INVALID and b"n_links" in msg, msg
    for rc, msg in both(rec(car)):
        assert rc == _capi.MBD_ERR_INVALID and b"n_links" in msg, msg
    # the same links, one actuator fewer; and the same model without the planar flag (a 3-D simulation of it).  n_links stands
    # for state_size too (13 floats per link, car2d: none); another device would need a second GPU and is not exercised here.
    fewer, flat = _one_actuator_fewer(env.sys), _not_planar(env.sys)
    assert fewer.act_size() == env.action_size - 1 and fewer.n_links == env.sys.n_links
    plant_fewer, plant_3d = RigidBodyEnv("hopper", model=fewer), RigidBodyEnv("hopper", model=flat)
    for rc, msg in both(rec(plant_fewer)):
        assert rc == _capi.MBD_ERR_INVALID and b"action_size" in msg, msg
    for rc, msg in both(rec(plant_3d)):
        assert rc == _capi.MBD_ERR_INVALID and b"planar" in msg, msg
    # k out of range
    for k in (-1, 2):
        r = rec()
        assert lib.mbd_sweep_set_mpc_plant(sweep.h, k, C.byref(r)) == _capi.MBD_ERR_INVALID and b"k=" in lib.mbd_last_error()
    # kicks need a root that translates freely in its plane: hopper, walker2d, halfcheetah, ant, the humanoids do
    for name, ok in (("hopper", True), ("walker2d", True), ("halfcheetah", True), ("ant", True), ("humanoidrun", True),
                     ("cartpole", False), ("car2d", False)):
        e, second = get_env(name), get_env(name)
        p = Plan(e, _args(name, 16, H=10, Nd=5))
        for r in (rec(kick_std=0.5), rec(second, kick_std=0.5)):
            rc, msg = lib.mbd_plan_set_mpc_plant(p.h, C.byref(r)), lib.mbd_last_error()
            if ok:
                assert rc == _capi.MBD_OK, (name, msg)
            else:
                assert rc == _capi.MBD_ERR_UNSUPPORTED and b"kick_std" in msg, (name, msg)
        r = rec(act_std=0.5)  # the action noise works for every env
        assert lib.mbd_plan_set_mpc_plant(p.h, C.byref(r)) == _capi.MBD_OK
        assert lib.mbd_plan_set_mpc_plant(p.h, None) == _capi.MBD_OK
        p.close()
    # a refused record changes nothing: the one set first is still there
    key = gpu.prng_key(1)
    plan.set_state0(env.reset(gpu.prng_key(0)))
    plan.set_mpc_plant(act_std=0.4, key=gpu.prng_key(2))
    ref = plan.run_mpc(key, 3, 2, 1)
    with pytest.raises(_capi.MbdError):
        plan.set_mpc_plant(act_std=-1.0)
    _equal(plan.run_mpc(key, 3, 2, 1), ref, "after a refused record")
    # the run calls' own refusals are untouched by a record
    mc = _capi.MpcConfig(n_ticks=0, warm_steps=2, exec_steps=1)
    assert lib.mbd_plan_run_mpc(plan.h, C.byref(mc), _capi.key_array(key), None, None, None, None, None) == _capi.MBD_ERR_INVALID
    assert b"n_ticks" in lib.mbd_last_error()
    plant = RigidBodyEnv("hopper", model=env.sys.scaled(mass=1.3))
    pi = Plan(env, a, update_method=1)
    pi.set_mpc_plant(env=plant)
    mc = _capi.MpcConfig(n_ticks=2, warm_steps=2, exec_steps=1)
    assert lib.mbd_plan_run_mpc(pi.h, C.byref(mc), _capi.key_array(key), None, None, None, None, None) == _capi.MBD_ERR_UNSUPPORTED
    assert b"update_method" in lib.mbd_last_error()
    pi.close()
    plan.close()
    sweep.close()


def _cli(tmp_path, *extra):
    pkg = os.path.join(ROOT, "model-based-diffusion_amd")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([pkg, ROOT, os.environ.get("PYTHONPATH", "")]))
    out = subprocess.run([sys.executable, "-m", "mbd_hip.planners.mpc", "--env_name", "hopper", "--disable_recommended_params",
                          "--Nsample", "128", "--Hsample", "20", "--Ndiffuse", "10", "--n_ticks", "6", "--warm_steps", "3",
                          "--exec_steps", "2", *extra], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1]), np.load(os.path.join(tmp_path, "results", "hopper", "mpc_episode.npz"))


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 4])
def test_command_line(gpu, tmp_path, P):
    res, ep = _cli(tmp_path, "--plant_mass", "1.3", "--act_noise_std", "0.2", *(("--n_episodes", str(P)) if P > 1 else ()))
    for k in ("plant_mass", "plant_friction", "plant_gear", "act_noise_std", "kick_std", "kick_every", "disturb_seed",
              "episode_reward", "nominal_episode_reward", "ms_per_tick"):
        assert k in res, k
    assert res["plant_mass"] == 1.3 and res["act_noise_std"] == 0.2 and res["plant_gear"] == 1.0 and res["kick_every"] == 1
    assert np.isfinite(res["episode_reward"]) and np.isfinite(res["nominal_episode_reward"])
    assert res["episode_reward"] != res["nominal_episode_reward"]
    if P > 1:
        assert res["n_episodes"] == P
        assert ep["actions"].shape == (P, 12, 3) and ep["states"].shape[:2] == (P, 7)
    else:
        assert ep["actions"].shape == (12, 3) and ep["states"].shape[0] == 7
    assert not np.array_equal(ep["actions"].reshape(-1, 12, 3)[0][:2], ep["means"].reshape(-1, 6, 20, 3)[0][0][:2])
