"""Sessions on the GPU (include/mbd_hip.h mbd_plan_mpc_open; DESIGN.md section 1 "N11 session"): an episode the caller drives one
tick per call.  Every comparison is np.array_equal, plus tobytes where a negative zero matters.

  replay           a session fed the states of Plan.run_mpc returns that episode's means and rows: hopper, humanoidrun (N = 128),
                   car2d, E in {1, 2}; under a delay record, D in {1, 2, 3}, rows0 NULL and given (one -0.0 in it), also the heads
                   and the predicted states
  caller = plant   a session whose rows the test executes on a scaled env equals the episode under a plant record naming that env
                   (stds 0), on the GPU and in tests/mpc_plant_checker.py
  foreign states   a state from another reset at tick 2: tests/mpc_online_checker.py, and not the replay from there on
  records          noise shape + basis (warm), ensemble (mean, min), humanoidtrack under a demo record with period 20
  asynchronous     submit, host work, collect == tick; a tick in flight, nothing in flight, the tick after max_ticks
  reset_mean       tick t equals tick 0 of a fresh session at the advanced key (the checker computes it); flagged COLD
  containment      a NaN root velocity at tick 1 is flagged; reset_mean and a healthy state give a checker-equal tick again
  while open       every other call of the handle is refused and works again after close; run_mpc before == after
  command line     --online writes the batch run's fields with equal contents; the C example runs

  sweeps           P in {2, 8} sessions in lockstep equal P single sessions, per-episode temperatures and a delay record included;
                   P = 3 with a NaN state and reset_mean in the middle episode: the other two keep a single session's bits throughout,
                   the middle one a single session's that is fed and reset alike (a tick whose episodes differ in length)
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mpc_online_checker as moc
import mpc_plant_checker
import noise_basis_checker as nbc
from conftest import ROOT
from test_gpu_noise_shape import _args, _env, _oenv, _state, shape_of

pytestmark = pytest.mark.gpu

N, H, ND, K, T = 64, 20, 6, 2, 5  # tests/test_gpu_mpc_delay.py's sizes
MISMATCH = dict(mass=1.3, friction=0.5, gear=0.8)


@pytest.fixture(scope="module")
def gpu(lib):
    from mbd_hip import _capi
    if _capi.device_count() < 1:
        pytest.fail("tests/test_gpu_mpc_online.py needs a GPU")
    return _capi


def _plan(env, name, n, st, h=H, nd=ND, **kw):
    from mbd_hip.planners.mbd_planner import Plan
    plan = Plan(env, _args(name, n, h, nd, **kw))
    plan.set_state0(st)
    return plan


def _rows0(D, E, Nu, seed=3):
    """Finite random committed rows in [-1, 1], one of them a negative zero."""
    r = np.random.default_rng(seed).uniform(-1, 1, (D * E, Nu)).astype(np.float32)
    r[0, 0] = -0.0
    return r


def _session(plan, key, states, E, n_ticks=None, reset_at=(), max_ticks=None):
    """The ticks of a session fed ``states``, as a dict of stacked arrays (and the list of flags)."""
    outs = []
    with plan.mpc_open(key, K, E, max_ticks) as s:
        for t in range(len(states) if n_ticks is None else n_ticks):
            if t in reset_at:
                s.reset_mean()
            outs.append(s.tick(states[t]))
    assert [o["tick"] for o in outs] == list(range(len(outs)))
    assert all(o["seconds"] > 0 for o in outs)
    pred = None if outs[0]["predicted"] is None else np.stack([o["predicted"] for o in outs])
    return dict(means=np.stack([o["mean"] for o in outs]), rows=np.stack([o["rows"] for o in outs]),
                heads=np.stack([o["head"] for o in outs]), predicted=pred, flags=[o["flags"] for o in outs],
                rew_mean=[o["rew_mean"] for o in outs])


# ---- replay -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("E", [1, 2])
@pytest.mark.parametrize("name,n", [("hopper", N), ("humanoidrun", 128), ("car2d", N)])
def test_replay_of_an_episode(gpu, name, n, E):
    env = _env(name)
    st, key = env.reset(gpu.prng_key(5)), gpu.prng_key(6)
    plan = _plan(env, name, n, st)
    ep = plan.run_mpc(key, T, K, E)
    got = _session(plan, key, ep["states"][:T], E)
    again = plan.run_mpc(key, T, K, E)
    from mbd_hip.envs.base import prng_impl
    mu, rew_means, _, _ = plan.run(gpu.prng_split(key, 2, prng_impl())[1])  # (tick 0 is Plan.run(k_0): its last step's mean reward)
    plan.close()
    assert np.array_equal(mu[-1], got["means"][0]) and np.float32(got["rew_mean"][0]).tobytes() == rew_means[-1].tobytes()
    assert np.isfinite(ep["means"]).all() and ep["means"].any()
    assert got["means"].tobytes() == ep["means"].tobytes()
    assert got["rows"].reshape(T * E, -1).tobytes() == ep["actions"].tobytes()
    assert got["heads"].tobytes() == got["rows"].tobytes() and got["predicted"] is None
    assert got["flags"] == [gpu.TICK_COLD] + [0] * (T - 1)
    for k in ("means", "actions", "rewards", "states"):  # (the handle runs episodes again after the session, same bits)
        assert again[k].tobytes() == ep[k].tobytes(), k


@pytest.mark.parametrize("name,n,E,D", [("hopper", N, 2, 1), ("hopper", N, 2, 2), ("hopper", N, 1, 3), ("humanoidrun", 128, 1, 2),
                                        ("car2d", N, 1, 2)])
def test_replay_of_a_delayed_episode(gpu, name, n, E, D):
    env = _env(name)
    st, key = env.reset(gpu.prng_key(5)), gpu.prng_key(6)
    plan = _plan(env, name, n, st)
    for rows0 in (None, _rows0(D, E, env.action_size)):
        plan.set_mpc_delay(D, rows0)
        ep = plan.run_mpc(key, T, K, E)
        got = _session(plan, key, ep["states"][:T], E)
        what = f"{name} E={E} D={D} rows0={'given' if rows0 is not None else 'NULL'}"
        assert got["means"].tobytes() == ep["means"].tobytes(), what
        assert got["heads"].reshape(T * E, -1).tobytes() == ep["actions"].tobytes(), what  # (the committed -0.0 included)
        assert got["predicted"].tobytes() == ep["predicted"].tobytes(), what
        assert got["rows"].tobytes() == np.ascontiguousarray(ep["means"][:, :E]).tobytes(), what
        if rows0 is not None:
            assert got["heads"].reshape(T * E, -1)[: D * E].tobytes() == rows0.tobytes()
    plan.close()


# ---- the caller is the plant ------------------------------------------------------------------------------------------------

def test_the_caller_is_the_plant(gpu, orc):
    from mbd_hip.envs.base import RigidBodyEnv, State, prng_impl
    name, E = "hopper", 2
    env = _env(name)
    plant = RigidBodyEnv(name, model=env.sys.scaled(**MISMATCH))
    st, key = env.reset(gpu.prng_key(5)), gpu.prng_key(6)
    plan = _plan(env, name, N, st)
    plan.set_mpc_plant(env=plant, key=gpu.prng_key(11))  # (both stds 0)
    ep = plan.run_mpc(key, T, K, E)
    with pytest.raises(gpu.MbdError, match="the caller is the plant") as e:
        plan.mpc_open(key, K, E)
    assert e.value.code == gpu.MBD_ERR_STATE
    plan.clear_mpc_plant()
    s = _state(env, st)
    means, actions, states = [], [], [s]
    with plan.mpc_open(key, K, E) as session:
        for _ in range(T):
            out = session.tick(s)
            _, fin = plant.rollout(State(s, None, np.float32(0), np.float32(0), {}), out["rows"][None], want_final=True)
            s = fin[0].cpu().numpy().reshape(-1)
            means.append(out["mean"]); actions.append(out["rows"]); states.append(s)
    plan.close()
    got = dict(means=np.stack(means), actions=np.concatenate(actions), states=np.stack(states))
    ref = mpc_plant_checker.episode(_oenv(orc, env), _state(env, st), key, N, H, ND, 0.1, T, K, E, plant=_oenv(orc, plant),
                                    impl=prng_impl())
    for k in got:
        assert np.array_equal(got[k], ep[k]), f"{k}: the session and the episode under the plant record differ"
        assert np.array_equal(got[k], ref[k]), f"{k}: the session and the checker differ"
    assert np.isfinite(ref["states"]).all()


# ---- foreign states ---------------------------------------------------------------------------------------------------------

def test_a_foreign_state_at_tick_2(gpu, orc):
    from mbd_hip.envs.base import prng_impl
    name, E = "hopper", 1
    env = _env(name)
    st, key = env.reset(gpu.prng_key(5)), gpu.prng_key(6)
    plan = _plan(env, name, N, st)
    ep = plan.run_mpc(key, T, K, E)
    states = ep["states"][:T].copy()
    states[2] = _state(env, env.reset(gpu.prng_key(77)))
    got = _session(plan, key, states, E)
    plan.close()
    ref = moc.session(_oenv(orc, env), key, states, N, H, ND, 0.1, K, E, impl=prng_impl())
    assert np.isfinite(ref["means"]).all()
    assert np.array_equal(got["means"], ref["means"]) and got["rows"].tobytes() == ref["rows"].tobytes()
    assert np.array_equal(got["means"][:2], ep["means"][:2])
    for t in range(2, T):
        assert not np.array_equal(got["means"][t], ep["means"][t]), t


# ---- records ----------------------------------------------------------------------------------------------------------------

def test_replay_under_a_warm_noise_shape_and_basis(gpu):
    name, E = "hopper", 1
    env = _env(name)
    st, key = env.reset(gpu.prng_key(5)), gpu.prng_key(6)
    g, W = shape_of(H, env.action_size), nbc.basis_of(H, 4)
    W[H // 2] = (0.5, -0.25, 1.25, 0.75)  # (no frozen row)
    plan = _plan(env, name, N, st)
    flat = plan.run_mpc(key, T, K, E)
    plan.set_noise_shape(g, "warm")
    plan.set_noise_basis(W, "warm")
    ep = plan.run_mpc(key, T, K, E)
    got = _session(plan, key, ep["states"][:T], E)
    plan.close()
    assert np.array_equal(got["means"], ep["means"])
    assert np.array_equal(ep["means"][0], flat["means"][0]) and not np.array_equal(ep["means"][1], flat["means"][1])


@pytest.mark.parametrize("risk", ["mean", "min"])
def test_replay_under_an_ensemble(gpu, risk):
    from mbd_hip.envs.base import RigidBodyEnv
    name, E = "hopper", 1
    env = _env(name)
    member = RigidBodyEnv(name, model=env.sys.scaled(mass=1.3, gear=0.8))
    st, key = env.reset(gpu.prng_key(5)), gpu.prng_key(6)
    plan = _plan(env, name, N, st)
    alone = plan.run_mpc(key, T, K, E)
    plan.set_ensemble([None, member], risk)
    ep = plan.run_mpc(key, T, K, E)
    got = _session(plan, key, ep["states"][:T], E)
    plan.close()
    assert np.array_equal(got["means"], ep["means"]) and not np.array_equal(ep["means"], alone["means"])


def test_replay_under_a_demo_record_with_period_20(gpu):
    """humanoidtrack, enable_demo, the env's clip extended with period 20: every tick's window is built by the tick's own launch
    and is the one the batch episode's table holds."""
    from mbd_hip.planners.mpc import cycle_clip
    name, E, Td = "humanoidtrack", 2, 4
    env = _env(name)
    st, key = env.reset(gpu.prng_key(5)), gpu.prng_key(6)
    clip = cycle_clip(np.asarray(env.xref, np.float32), 3 + Td * E + 50, 20)
    plan = _plan(env, name, N, st, h=50, enable_demo=True)
    with pytest.raises(gpu.MbdError, match="enable_demo") as e:  # (a demo plan without a record has no clock: run_mpc's refusal)
        plan.mpc_open(key, K, E)
    assert e.value.code == gpu.MBD_ERR_UNSUPPORTED
    plan.set_mpc_demo(clip, start_row=3)
    ep = plan.run_mpc(key, Td, K, E)
    got = _session(plan, key, ep["states"][:Td], E)
    # a start row past the clip's end: every window holds the last row, in the episode's table and in the ticks' own launches
    # (the clip is played backwards, so that its last row is where the system starts and the means are finite: held on the
    # forward clip's last row, metres ahead, every candidate's distance would be clipped alike and the means would be NaN, which
    # compares nothing — the reason tests/mpc_demo_checker.py's "held" case reverses its clip too)
    plan.set_mpc_demo(np.ascontiguousarray(clip[:, ::-1]), start_row=clip.shape[1] + 5)
    late = plan.run_mpc(key, 2, K, E)
    got_late = _session(plan, key, late["states"][:2], E)
    plan.close()
    assert np.isfinite(ep["means"]).all()
    assert np.array_equal(got["means"], ep["means"]) and np.array_equal(got["rows"].reshape(Td * E, -1), ep["actions"])
    assert np.isfinite(late["means"]).all()
    assert np.array_equal(got_late["means"], late["means"]) and not np.array_equal(late["means"][1], ep["means"][1])


# ---- asynchronous use -------------------------------------------------------------------------------------------------------

def test_submit_then_collect_and_the_refusals(gpu):
    name, E = "hopper", 1
    env = _env(name)
    st, key = env.reset(gpu.prng_key(5)), gpu.prng_key(6)
    plan = _plan(env, name, N, st)
    ep = plan.run_mpc(key, 3, K, E)

    def state_error(call, text):
        with pytest.raises(gpu.MbdError, match=text) as e:
            call()
        assert e.value.code == gpu.MBD_ERR_STATE

    with plan.mpc_open(key, K, E, max_ticks=3) as s:
        state_error(s.collect, "no tick is in flight")
        state_error(lambda: plan.mpc_open(key, K, E), "a session is open")
        for t in range(3):
            s.submit(ep["states"][t])
            state_error(lambda: s.submit(ep["states"][t]), "a tick is in flight")
            state_error(s.reset_mean, "a tick is in flight")
            host_work = float(np.linalg.norm(np.arange(1 << 16, dtype=np.float64)))  # (the host is free meanwhile)
            out = s.collect()
            assert host_work > 0 and out["tick"] == t and np.array_equal(out["mean"], ep["means"][t])
            state_error(s.collect, "no tick is in flight")
        state_error(lambda: s.tick(ep["states"][0]), "n_ticks=3")
    state_error(s.collect, "no session is open")
    with plan.mpc_open(key, K, E) as s:  # (a tick left in flight is dropped by close)
        s.submit(ep["states"][0])
    assert np.array_equal(plan.run_mpc(key, 3, K, E)["means"], ep["means"])
    plan.close()


# ---- reset_mean and containment ---------------------------------------------------------------------------------------------

def _advanced(gpu, key, t):
    from mbd_hip.envs.base import prng_impl
    rng = np.asarray(key, np.uint32)
    for _ in range(t):
        rng = gpu.prng_split(rng, 2, prng_impl())[0]
    return rng


@pytest.mark.parametrize("D", [0, 2])
def test_reset_mean_gives_tick_0_of_a_fresh_session_at_the_advanced_key(gpu, orc, D):
    from mbd_hip.envs.base import prng_impl
    name, E, t = "hopper", 1, 3
    env = _env(name)
    st, key = env.reset(gpu.prng_key(5)), gpu.prng_key(6)
    plan = _plan(env, name, N, st)
    rows0 = _rows0(D, E, env.action_size) if D else None
    if D:
        plan.set_mpc_delay(D, rows0)
    ep = plan.run_mpc(key, T, K, E)
    states = ep["states"][:T]
    got = _session(plan, key, states, E, reset_at=(t,))
    plan.close()
    assert got["flags"] == [gpu.TICK_COLD if k in (0, t) else 0 for k in range(T)]
    assert np.array_equal(got["means"][:t], ep["means"][:t]) and not np.array_equal(got["means"][t], ep["means"][t])
    oenv = _oenv(orc, env)
    ref = moc.session(oenv, key, states, N, H, ND, 0.1, K, E, D, rows0=rows0, reset_at=(t,), impl=prng_impl())
    assert np.isfinite(ref["means"]).all() and np.array_equal(got["means"], ref["means"])
    assert got["heads"].tobytes() == ref["heads"].tobytes()  # (the queue is left as it is)
    if not D:  # tick 0 of a fresh session whose key is the chain advanced t times
        fresh = moc.Session(oenv, _advanced(gpu, key, t), N, H, ND, 0.1, K, E, impl=prng_impl()).tick(states[t])
        assert fresh["cold"] and np.array_equal(fresh["mean"], got["means"][t])


def test_a_nan_state_is_flagged_and_reset_mean_recovers(gpu, orc):
    from mbd_hip.envs.base import prng_impl
    name, E = "hopper", 1
    env = _env(name)
    st, key = env.reset(gpu.prng_key(5)), gpu.prng_key(6)
    plan = _plan(env, name, N, st)
    ep = plan.run_mpc(key, T, K, E)
    bad = ep["states"][1].copy()
    bad[gpu_link_vel()] = np.nan  # (link 0's linear velocity)
    outs = []
    with plan.mpc_open(key, K, E) as s:
        outs.append(s.tick(ep["states"][0]))
        outs.append(s.tick(bad))
        s.reset_mean()
        outs.append(s.tick(ep["states"][2]))
        outs.append(s.tick(ep["states"][3]))
    plan.close()
    assert outs[0]["flags"] == gpu.TICK_COLD and np.array_equal(outs[0]["mean"], ep["means"][0])
    assert outs[1]["flags"] & gpu.TICK_STATE_NONFINITE
    # the tick ran, and containment is the episode's: every candidate starts from the NaN state, so every reward, every weight and
    # with them every element of the mean is NaN — its first rows included, which the device's reduction has to have seen
    assert np.isnan(outs[1]["mean"]).all() and np.isnan(outs[1]["rows"]).all()
    assert outs[1]["flags"] & gpu.TICK_ROWS_NONFINITE
    assert all(not (o["flags"] & gpu.TICK_ROWS_NONFINITE) for k, o in enumerate(outs) if k != 1)
    oenv = _oenv(orc, env)
    fresh = moc.Session(oenv, _advanced(gpu, key, 2), N, H, ND, 0.1, K, E, impl=prng_impl())
    for t in (2, 3):
        want = fresh.tick(ep["states"][t])
        assert outs[t]["flags"] == (gpu.TICK_COLD if t == 2 else 0)
        assert np.isfinite(outs[t]["mean"]).all() and np.array_equal(outs[t]["mean"], want["mean"]), t


def gpu_link_vel():
    """MBD_LINK_VEL of include/mbd_hip.h: where link 0's linear velocity starts inside a state."""
    import re
    text = open(os.path.join(ROOT, "include", "mbd_hip.h")).read()
    return int(re.search(r"#define MBD_LINK_VEL (\d+)", text).group(1))


# ---- sweeps ------------------------------------------------------------------------------------------------------------------

def _single(env, name, st, key, temp, states, E, D=0, rows0=None, reset_at=(), n=N):
    """The ticks of ONE plan's session at temperature ``temp`` fed ``states`` (list of dicts)."""
    from mbd_hip.planners.mbd_planner import Plan
    plan = Plan(env, _args(name, n, H, ND, **{}) if temp is None else _targs(name, n, temp))
    plan.set_state0(st)
    if D:
        plan.set_mpc_delay(D, rows0)
    outs = []
    with plan.mpc_open(key, K, E) as s:
        for t, x in enumerate(states):
            if t in reset_at:
                s.reset_mean()
            outs.append(s.tick(x))
    plan.close()
    return outs


def _targs(name, n, temp):
    from dataclasses import replace
    return replace(_args(name, n, H, ND), temp_sample=float(temp))


@pytest.mark.parametrize("P,D", [(2, 0), (2, 2), (8, 0), (8, 1)])
def test_sweep_sessions_equal_single_sessions(gpu, P, D):
    """Episode k has its own key, start state, temperature and fed states (episode k's own batch episode's); with D a delay record
    with committed rows, one -0.0 in them."""
    from mbd_hip.planners.mbd_planner import Sweep
    name, E = "hopper", 2
    env = _env(name)
    temps = [0.1 + 0.05 * k for k in range(P)]
    sts = [env.reset(gpu.prng_key(20 + k)) for k in range(P)]
    keys = np.stack([gpu.prng_key(40 + k) for k in range(P)])
    rows0 = _rows0(D, E, env.action_size) if D else None
    sweep = Sweep(env, _args(name, N, H, ND), P, temps=temps)
    for k in range(P):
        sweep.set_state0(k, sts[k])
    if D:
        sweep.set_mpc_delay(D, rows0)
    ep = sweep.run_mpc(keys, T, K, E)
    assert np.isfinite(ep["means"]).all()
    outs = []
    with sweep.mpc_open(keys, K, E) as s:
        for t in range(T):
            outs.append(s.tick(np.ascontiguousarray(ep["states"][:, t])))
    again = sweep.run_mpc(keys, T, K, E)
    sweep.close()
    for k in range(P):
        one = _single(env, name, sts[k], keys[k], temps[k], ep["states"][k, :T], E, D, rows0)
        for t in range(T):
            for f in ("mean", "rows", "head") + (("predicted",) if D else ()):
                assert outs[t][f][k].tobytes() == one[t][f].tobytes(), (k, t, f)
            assert int(outs[t]["flags"][k]) == one[t]["flags"] == (gpu.TICK_COLD if t == 0 else 0)
            assert np.float32(outs[t]["rew_mean"][k]).tobytes() == np.float32(one[t]["rew_mean"]).tobytes()
            assert np.array_equal(outs[t]["mean"][k], ep["means"][k, t])  # (and the batch episode's: the replay)
    assert not np.array_equal(outs[1]["mean"][0], outs[1]["mean"][1])
    for f in ("means", "actions", "rewards", "states"):
        assert again[f].tobytes() == ep[f].tobytes(), f


def test_sweep_contains_a_nan_episode_and_its_reset(gpu):
    """P = 3: episode 1 is fed a NaN root velocity at tick 1 and reset in front of tick 2, where its tick is cold (Ndiffuse-1 steps)
    and the others' are warm (K steps).  Episodes 0 and 2 keep the bits of single sessions throughout; episode 1 equals a single
    session fed and reset alike in its finite ticks."""
    from mbd_hip.planners.mbd_planner import Sweep
    name, E, P = "hopper", 1, 3
    env = _env(name)
    sts = [env.reset(gpu.prng_key(20 + k)) for k in range(P)]
    keys = np.stack([gpu.prng_key(40 + k) for k in range(P)])
    sweep = Sweep(env, _args(name, N, H, ND), P)
    for k in range(P):
        sweep.set_state0(k, sts[k])
    ep = sweep.run_mpc(keys, T, K, E)
    fed = np.ascontiguousarray(ep["states"][:, :T]).copy()
    fed[1, 1, gpu_link_vel()] = np.nan
    outs = []
    with sweep.mpc_open(keys, K, E) as s:
        with pytest.raises(gpu.MbdError, match="outside") as e:
            s.reset_mean(3)
        assert e.value.code == gpu.MBD_ERR_INVALID
        for t in range(T):
            if t == 2:
                s.reset_mean(1)
            outs.append(s.tick(np.ascontiguousarray(fed[:, t])))
    sweep.close()
    for k in range(P):
        one = _single(env, name, sts[k], keys[k], None, fed[k], E, reset_at=(2,) if k == 1 else ())
        for t in range(T):
            assert int(outs[t]["flags"][k]) == one[t]["flags"], (k, t)
            if k == 1 and t == 1:
                assert np.isnan(outs[t]["mean"][k]).all() and int(outs[t]["flags"][k]) == gpu.TICK_STATE_NONFINITE | gpu.TICK_ROWS_NONFINITE
                continue
            assert np.isfinite(one[t]["mean"]).all(), (k, t)
            assert outs[t]["mean"][k].tobytes() == one[t]["mean"].tobytes(), (k, t)
            assert outs[t]["rows"][k].tobytes() == one[t]["rows"].tobytes(), (k, t)
    assert int(outs[2]["flags"][1]) == gpu.TICK_COLD and int(outs[2]["flags"][0]) == 0
    for k in (0, 2):  # (untouched by their neighbour: the batch episode's means)
        assert np.array_equal(np.stack([o["mean"][k] for o in outs]), ep["means"][k])


def test_sweep_refuses_other_calls_while_a_session_is_open(gpu):
    from mbd_hip.planners.mbd_planner import Sweep
    name, E, P = "hopper", 1, 2
    env = _env(name)
    st = env.reset(gpu.prng_key(5))
    keys = np.stack([gpu.prng_key(40 + k) for k in range(P)])
    g = shape_of(H, env.action_size)
    sweep = Sweep(env, _args(name, N, H, ND), P)
    for k in range(P):
        sweep.set_state0(k, st)
    before = sweep.run_mpc(keys, 3, K, E)
    calls = {"run": lambda: sweep.run(keys), "run_mpc": lambda: sweep.run_mpc(keys, 3, K, E), "set_state0": lambda: sweep.set_state0(0, st),
             "set_mpc_plant": lambda: sweep.set_mpc_plant(0), "clear_mpc_plant": lambda: sweep.clear_mpc_plant(0),
             "set_noise_shape": lambda: sweep.set_noise_shape(g), "clear_noise_shape": sweep.clear_noise_shape,
             "set_noise_basis": lambda: sweep.set_noise_basis(nbc.basis_of(H, 4)), "set_mpc_delay": lambda: sweep.set_mpc_delay(1),
             "clear_mpc_delay": sweep.clear_mpc_delay, "clear_mpc_demo": sweep.clear_mpc_demo,
             "mpc_open": lambda: sweep.mpc_open(keys, K, E)}
    with sweep.mpc_open(keys, K, E, max_ticks=1) as s:
        for what, call in calls.items():
            with pytest.raises(gpu.MbdError, match="a session is open") as e:
                call()
            assert e.value.code == gpu.MBD_ERR_STATE, what
        s.submit(np.ascontiguousarray(before["states"][:, 0]))
        for call, text in ((lambda: s.submit(before["states"][:, 0].copy()), "a tick is in flight"), (lambda: s.reset_mean(0), "a tick is in flight")):
            with pytest.raises(gpu.MbdError, match=text) as e:
                call()
            assert e.value.code == gpu.MBD_ERR_STATE
        out = s.collect()
        for call, text in ((s.collect, "no tick is in flight"), (lambda: s.tick(before["states"][:, 0].copy()), "n_ticks=1")):
            with pytest.raises(gpu.MbdError, match=text) as e:
                call()
            assert e.value.code == gpu.MBD_ERR_STATE
    assert np.array_equal(out["mean"], before["means"][:, 0])
    sweep.set_mpc_plant(0)  # (they work again; and a plant record refuses the session)
    with pytest.raises(gpu.MbdError, match="the caller is the plant") as e:
        sweep.mpc_open(keys, K, E)
    assert e.value.code == gpu.MBD_ERR_STATE
    sweep.clear_mpc_plant(0)
    assert np.array_equal(sweep.run_mpc(keys, 3, K, E)["means"], before["means"])
    with sweep.mpc_open(keys, K, E):  # (destroy closes an open session)
        sweep.close()


# ---- while a session is open ------------------------------------------------------------------------------------------------

def test_other_calls_are_refused_while_a_session_is_open(gpu):
    from mbd_hip.envs.base import RigidBodyEnv
    name, E = "hopper", 1
    env = _env(name)
    member = RigidBodyEnv(name, model=env.sys.scaled(mass=1.2))
    st, key = env.reset(gpu.prng_key(5)), gpu.prng_key(6)
    plan = _plan(env, name, N, st)
    before = plan.run_mpc(key, 3, K, E)
    g, W = shape_of(H, env.action_size), nbc.basis_of(H, 4)
    dummy = np.zeros(H * env.action_size + 8, np.float32)
    d, k2 = gpu.np_ptr(dummy), gpu.key_array(key)
    lib = plan.lib
    calls = {
        "run": lambda: plan.run(key), "run_mpc": lambda: plan.run_mpc(key, 3, K, E), "eval": lambda: plan.eval(before["means"][0]),
        "set_state0": lambda: plan.set_state0(st), "set_mpc_plant": lambda: plan.set_mpc_plant(env=member),
        "clear_mpc_plant": plan.clear_mpc_plant, "set_ensemble": lambda: plan.set_ensemble([None, member]),
        "clear_ensemble": plan.clear_ensemble, "set_noise_shape": lambda: plan.set_noise_shape(g),
        "clear_noise_shape": plan.clear_noise_shape, "set_noise_basis": lambda: plan.set_noise_basis(W),
        "clear_noise_basis": lambda: plan.set_noise_basis(None), "set_mpc_delay": lambda: plan.set_mpc_delay(1),
        "clear_mpc_delay": plan.clear_mpc_delay, "clear_mpc_demo": plan.clear_mpc_demo,
        "reverse_once": lambda: gpu.check(lib.mbd_plan_reverse_once(plan.h, 1, k2, d, d, None)),
        "sample_rollout": lambda: gpu.check(lib.mbd_plan_sample_rollout(plan.h, 1, k2, d, d, None, None)),
        "score_update": lambda: gpu.check(lib.mbd_plan_score_update(plan.h, 1, k2, d, d, None, d, d, None)),
    }
    with plan.mpc_open(key, K, E) as s:
        first = s.tick(before["states"][0])
        for what, call in calls.items():
            with pytest.raises(gpu.MbdError, match="a session is open") as e:
                call()
            assert e.value.code == gpu.MBD_ERR_STATE, what
        second = s.tick(before["states"][1])  # (the refused calls touched nothing)
    assert np.array_equal(first["mean"], before["means"][0]) and np.array_equal(second["mean"], before["means"][1])
    assert not dummy.any()
    after = plan.run_mpc(key, 3, K, E)
    for k in ("means", "actions", "rewards", "states"):
        assert after[k].tobytes() == before[k].tobytes(), k
    plan.set_state0(st)  # (they work again)
    plan.set_noise_shape(g)
    plan.clear_noise_shape()
    plan.set_mpc_delay(1)
    plan.clear_mpc_delay()
    assert np.array_equal(plan.run_mpc(key, 3, K, E)["means"], before["means"])
    with plan.mpc_open(key, K, E):  # (destroy closes an open session)
        plan.close()


# ---- the command line and the C example -------------------------------------------------------------------------------------

def test_command_line_online_equals_the_batch_run(gpu, tmp_path):
    """hopper N = 128, H = 20, Ndiffuse = 10, T = 6, K = 3 on a plant of mass 1.3, planned one tick ahead: --online saves the
    fields of the batch run with equal contents."""
    from mbd_hip.planners.mpc import MpcArgs, run_mpc
    pkg = os.path.join(ROOT, "model-based-diffusion_amd")
    envv = dict(os.environ, PYTHONPATH=os.pathsep.join([pkg, ROOT, os.environ.get("PYTHONPATH", "")]))
    argv = ["--env_name", "hopper", "--disable_recommended_params", "--Nsample", "128", "--Hsample", "20", "--Ndiffuse", "10", "--n_ticks", "6",
            "--warm_steps", "3", "--exec_steps", "2", "--plant_mass", "1.3", "--delay_ticks", "1"]
    out = subprocess.run([sys.executable, "-m", "mbd_hip.planners.mpc", *argv, "--online"], cwd=tmp_path, env=envv, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    saved = np.load(os.path.join(tmp_path, "results", "hopper", "mpc_episode.npz"))
    a = MpcArgs(env_name="hopper", disable_recommended_params=True, Nsample=128, Hsample=20, Ndiffuse=10, n_ticks=6, warm_steps=3,
                exec_steps=2, plant_mass=1.3, delay_ticks=1, not_render=True)
    rew, det = run_mpc(a, return_details=True)
    assert sorted(saved.files) == ["actions", "means", "predicted", "rewards", "states"]
    for f in saved.files:
        assert saved[f].shape == det[f].shape and np.array_equal(saved[f], det[f]), f
    assert res["online"] is True and np.float32(res["episode_reward"]) == np.float32(rew)
    assert res["ms_per_tick"] > 0 and res["warm_tick_ms_min"] <= res["warm_tick_ms_median"] <= res["warm_tick_ms_max"]
    refused = subprocess.run([sys.executable, "-m", "mbd_hip.planners.mpc", *argv, "--online", "--act_noise_std", "0.1"], cwd=tmp_path,
                             env=envv, capture_output=True, text=True, timeout=300)
    assert refused.returncode != 0 and "act_noise_std" in refused.stderr


@pytest.mark.parametrize("D", [0, 1])
def test_c_caller_drives_a_session(gpu, tmp_path, D):
    """examples/mbd_control.c from plain C: 6 ticks on hopper, finite rewards, tick 0 flagged cold (4) and no other flag."""
    libdir = os.path.join(ROOT, "model-based-diffusion_amd", "lib")
    exe = str(tmp_path / "mbd_control")
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "mbd_control.c"),
                    "-o", exe, "-L", libdir, "-lmbd_hip", f"-Wl,-rpath,{libdir}", "-lm"], check=True)
    out = subprocess.run([exe, "hopper", "64", "20", "6", "2", "6", str(D)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    ticks = [ln.split() for ln in lines if ln.startswith("tick ")]
    assert [int(t[1]) for t in ticks] == list(range(6)) and [int(t[7]) for t in ticks] == [4, 0, 0, 0, 0, 0]
    assert all(np.isfinite(float(t[3])) for t in ticks) and lines[-1].startswith("mean_reward ")
