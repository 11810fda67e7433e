"""-m gpu: the value record (include/mbd_hip.h mbd_value; DESIGN.md section 1 "N16 value") against the checker's restatement,
tests/value_checker.py.  Every comparison is by bit pattern (NaNs canonicalised where a row may hold one: value_checker.canon).

  the kernel alone   mbd_plan_eval_value over B = 1..40 and 257 rows, every net shape, both activations, REL_XY on and off, hopper,
                     humanoidrun and car2d, under every tile size of the launch (the lever MBD_VALUE_TILE) and the default
  identity           a record set and cleared, an all-zero net
  to the checker     whole plans and episodes: hopper, humanoidrun (one and two candidates per lane), car2d, mppi, cma-es, an
                     objective record in front, a demo plan
  closed loop        a session fed an episode's states, a sweep of three plans, two unequal shards, a pick record's returns
  containment        candidates that diverge on the 1e30 gear beside healthy ones (then dropped by a weighting record), a
                     diverged plan of a sweep
  refusals           an ensemble and a value record, in both orders
  the command line   python -m mbd_hip.planners.mpc --value"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import containment_inputs as ci
import mpc_pick_checker as pick_checker
import objective_checker as oc
import value_checker as vc
import value_inputs as vi
import weighting_checker as wc
import weighting_combined_inputs as wci
import weighting_inputs as wi
from conftest import ROOT
from oracle import planner as op
from state_inputs import same_bits
from test_objective import gpu_record

pytestmark = pytest.mark.gpu

_LOGS = ("means", "actions", "rewards", "states")
ND, T, K = 6, 3, 2
PLANS = [("hopper", 70, 7), ("humanoidrun", 40, 5), ("car2d", 33, 6)]


@pytest.fixture(scope="module")
def gpu(lib):
    from mbd_hip import _capi
    if _capi.device_count() < 1:
        pytest.fail("tests/test_gpu_value.py needs a GPU")
    return _capi


@functools.lru_cache(maxsize=None)
def _env(name):
    from mbd_hip.envs import get_env
    return get_env(name)


def _oenv(orc, env):
    if env.__class__.__name__ == "Car2d":
        return op.OracleEnv(orc, "car2d", xref=env.xref, rew_xref=env.rew_xref)
    return op.OracleEnv(orc, env.env_name, env.sys.to_struct(), xref=env.xref, rew_xref=env.rew_xref, init_q=env.sys.init_q)


def _args(name, N, H, Nd=ND, **kw):
    from mbd_hip.planners.mpc import MpcArgs
    return MpcArgs(env_name=name, Nsample=N, Hsample=H, Ndiffuse=Nd, temp_sample=0.1, disable_recommended_params=True,
                   not_render=True, **kw)


def _state(st):
    return np.asarray(st.pipeline_state, np.float32).reshape(-1)


def _equal(a, b, what=""):
    for k in _LOGS:
        x, y = np.asarray(a[k], np.float32), np.asarray(b[k], np.float32)
        assert x.size == y.size, f"{what}: {k} sizes"
        same_bits(x.reshape(y.shape), y, f"{what}: {k} differ")


def _impl():
    from mbd_hip.envs.base import prng_impl
    return prng_impl()


def _net(name, shape="S-65-64-1", act=None, scale=0.37):
    """The net of a plan test: tanh and REL_XY on the rigid-body envs, relu on car2d."""
    rigid = name != "car2d"
    return vi.net(name, shape, act or ("tanh" if rigid else "relu"), rel_xy=rigid, scale=scale)


def _plan(gpu, name, N, H, net=None, seed=3, Nd=ND, **plan_kw):
    from mbd_hip.planners.mbd_planner import Plan
    env = _env(name)
    plan = Plan(env, _args(name, N, H, Nd), **plan_kw)
    st = env.reset(gpu.prng_key(seed))
    plan.set_state0(st)
    if net is not None:
        plan.set_value(net.value_net())
    return env, plan, st


# ---- the kernel alone -----------------------------------------------------------------------------------------------------------
_KERNEL = [(e, a, r) for e in vi.ENVS for a in ("relu", "tanh") for r in ((False, True) if e != "car2d" else (False,))]


@pytest.mark.parametrize("name,act,rel", _KERNEL, ids=[f"{e}-{a}-{'rel' if r else 'abs'}" for e, a, r in _KERNEL])
def test_eval_value_against_the_checker(gpu, orc, levers, name, act, rel):
    """Every shape of value_inputs.SHAPES; B = 1..40 and 257 so that every remainder against every tile occurs; the rows with NaN,
    both infinities and -0 among them, and every other row with the bits it has when those rows are healthy."""
    env, plan, _ = _plan(gpu, name, 8, 3)
    states, healthy = vi.states(name), vi.healthy_states(name)
    plain = np.array([b for b in range(vi.ROWS) if b not in vi.SPECIAL])
    try:
        for shape in vi.SHAPES:
            net = vi.net(name, shape, act, rel)
            want = vc.canon(vc.value(orc, net, states))
            plan.set_value(net.value_net())
            for tile in (4, 8, 16, -1):
                levers(MBD_VALUE_TILE=tile)
                for B in (list(range(1, 41)) if tile > 0 else []) + [vi.ROWS]:
                    got = plan.eval_value(states[:B])
                    same_bits(vc.canon(got), want[:B], f"{name} {shape} {act} rel={rel} tile={tile} B={B}")
                clean = plan.eval_value(healthy)
                assert np.isfinite(clean).all()
                same_bits(got[plain], clean[plain], f"{name} {shape} tile={tile}: the neighbours of the non-finite rows")
    finally:
        plan.close()


def test_peek_eval_and_set_states(gpu):
    env, plan, st = _plan(gpu, "hopper", 33, 4)
    lib = plan.lib
    x = vi.healthy_states("hopper")[:4]
    assert lib.mbd_plan_peek_value(plan.h, None) == gpu.MBD_ERR_STATE and b"no value record" in lib.mbd_last_error()
    with pytest.raises(gpu.MbdError, match="no value record"):
        plan.eval_value(x)
    net = _net("hopper")
    plan.set_value(net.value_net())
    assert lib.mbd_plan_peek_value(plan.h, None) == gpu.MBD_ERR_STATE and b"no diffusion step" in lib.mbd_last_error()
    plan.run(gpu.prng_key(1))
    assert plan.peek_value().shape == (33,)
    for mutate, field in ((lambda r: setattr(r, "n_in", 13), "n_in"), (lambda r: r.width.__setitem__(0, 300), r"width\[0\]"),
                          (lambda r: setattr(r, "scale", float("nan")), "scale")):
        vn = net.value_net()
        rec = vn.record()
        mutate(rec)
        import ctypes as C
        assert lib.mbd_plan_set_value(plan.h, C.byref(rec)) == gpu.MBD_ERR_INVALID
        import re
        assert re.search(field, lib.mbd_last_error().decode())
    plan.peek_value()  # (a refused call leaves the record)
    assert lib.mbd_plan_eval_value(plan.h, None, 1, None) == gpu.MBD_ERR_INVALID
    out = np.zeros(1, np.float32)
    assert lib.mbd_plan_eval_value(plan.h, x.ctypes.data, 0, out.ctypes.data) == gpu.MBD_ERR_INVALID
    p2 = _plan(gpu, "car2d", 8, 3)[1]
    with pytest.raises(gpu.MbdError, match="REL_XY") as e:
        p2.set_value(vi.net("car2d", "S-1", rel_xy=True).value_net())
    assert e.value.code == gpu.MBD_ERR_UNSUPPORTED
    p2.close()
    with plan.mpc_open(gpu.prng_key(2), K) as s:
        with pytest.raises(gpu.MbdError, match="session is open"):
            plan.set_value(net.value_net())
        s.tick(_state(st))
    plan.set_value(None)
    assert lib.mbd_plan_peek_value(plan.h, None) == gpu.MBD_ERR_STATE
    plan.close()


# ---- identity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,N,H", PLANS[:2])
def test_records_that_change_nothing(gpu, name, N, H):
    env, plan, st = _plan(gpu, name, N, H)
    key = gpu.prng_key(8)
    ref_run = plan.run(key)
    ref_ep = plan.run_mpc(key, T, K, 2)

    def same(what):
        got = plan.run(key)
        for x, y in zip(got[:3], ref_run[:3]):
            same_bits(np.asarray(x, np.float32), np.asarray(y, np.float32), f"{name} {what}: run")
        _equal(plan.run_mpc(key, T, K, 2), ref_ep, f"{name} {what}")

    net = _net(name)
    zero = vc.Net([np.zeros_like(w) for w in net.W], [np.zeros_like(b) for b in net.b], net.act, net.center, net.in_scale, net.rel_xy, 1.0)
    plan.set_value(zero.value_net())
    same("an all-zero net")
    same_bits(plan.peek_value(), np.zeros(N, np.float32), "V of the all-zero net")
    plan.set_value(net.value_net())
    assert not np.array_equal(plan.run(key)[0], ref_run[0])
    plan.set_value(None)
    same("a record set, then cleared")
    plan.close()


# ---- whole plans and episodes to the checker ------------------------------------------------------------------------------------
_FAMILIES = PLANS + [("humanoidrun-pk2", 40, 5)]


@pytest.mark.parametrize("case,N,H", _FAMILIES, ids=[c[0] for c in _FAMILIES])
def test_plan_and_episode_match_the_checker(gpu, orc, levers, case, N, H):
    name = case.split("-")[0]
    if case.endswith("pk2"):
        levers(MBD_PK2=1)  # the two-candidates-per-lane rollouts
    net = _net(name)
    env, plan, st = _plan(gpu, name, N, H, net, seed=5)
    oenv, s0, key = _oenv(orc, env), _state(st), gpu.prng_key(6)
    ve = vc.ValueEnv(oenv, net)
    mu, rm, rf, _ = plan.run(key)
    want = oc.plan(orc, oenv, oc.Record(), s0, key, N, H, ND, 0.1, _impl(), env=ve)
    same_bits(mu, want["mu_0ts"], f"{case}: means")
    same_bits(rm, want["rew_means"], f"{case}: mean rewards")
    same_bits(np.float32(rf), np.float32(want["rew_final"]), f"{case}: the final reward is the env's own")
    same_bits(plan.peek_value(), ve.last[1], f"{case}: V of the last step")
    assert np.isfinite(ve.last[1]).all() and np.ptp(ve.last[1]) > 0
    # one step through the phase call: the rewards buffer holds rews + scale * V
    import torch
    i = ND - 2
    Ybar = (np.random.default_rng(N + H).normal(size=(H, env.action_size)) * 0.3).astype(np.float32)
    d_Y, d_r = torch.tensor(Ybar.reshape(-1), device="cuda"), torch.full((N,), float("nan"), device="cuda")
    gpu.check(plan.lib.mbd_plan_sample_rollout(plan.h, i, gpu.key_array(gpu.prng_key(10 + N)), d_Y.data_ptr(), d_r.data_ptr(), None, None))
    torch.cuda.synchronize()
    Y0s, rewss, _ = plan.peek()
    V = vc.value(orc, net, vc.final_states(oenv, s0, Y0s))
    same_bits(plan.peek_value(), V, f"{case}: V of one step")
    same_bits(d_r.cpu().numpy(), vc.add(op.mean_h(orc, rewss), net.scale, V), f"{case}: the rewards of one step")
    for E in (1, 2):
        ep = plan.run_mpc(key, T, K, E)
        ref = oc.episode(oenv, oc.Record(), s0, key, N, H, ND, 0.1, T, K, E, env=ve, prev=oc.Prev(), impl=_impl())
        _equal(ep, ref, f"{case} E={E}")
    same_bits(plan.peek_value(), ve.last[1], f"{case}: V of the episode's last step")
    plan.close()


@pytest.mark.parametrize("method", ["mppi", "cma-es"])
def test_path_integral_plan_and_episode_match_the_checker(gpu, orc, method):
    from mbd_hip.planners import path_integral
    from mbd_hip.planners.mbd_planner import Plan
    name, N, H, Nr, E = "hopper", 70, 7, 5, 2
    env = _env(name)
    net = _net(name)
    args = path_integral.Args(env_name=name, Nsample=N, Hsample=H, Nrefine=Nr, temp_sample=0.1, disable_recommended_params=True)
    plan = Plan(env, args, update_method=op.PI_METHODS[method])
    st, key = env.reset(gpu.prng_key(3)), gpu.prng_key(4)
    plan.set_state0(st)
    plan.set_value(net.value_net())
    oenv, s0 = _oenv(orc, env), _state(st)
    ve = vc.ValueEnv(oenv, net)
    mu = plan.run(key)[0]
    want = oc.pi_plan(orc, ve, oc.Record(), s0, key, N, H, Nr, 0.1, method, _impl())  # (an empty objective record changes nothing)
    same_bits(mu, want["mu_0ts"], f"{method}: means")
    same_bits(plan.peek_value(), ve.last[1], f"{method}: V")
    sig = (1.0, 0.5, 0.0) if method == "mppi" else (1.0, 0.25, 2.0)
    plan.set_mpc_sigma(*sig)
    ep = plan.run_mpc(key, T, K, E)
    ref = oc.episode(oenv, oc.Record(), s0, key, N, H, Nr, 0.1, T, K, E, method=method, sigma=sig, env=ve, prev=oc.Prev(), impl=_impl())
    _equal(ep, ref, f"{method} episode")
    plan.close()


@pytest.mark.parametrize("name,N,H", PLANS[:2])
def test_the_value_launch_follows_the_objectives(gpu, orc, name, N, H):
    """An objective record with row weights rebuilds the reward from the per-step rewards: were the value launch in front of it,
    V would be lost.  The checker adds scale * V to ret - cost."""
    env = _env(name)
    rec, net, E = gpu_record(H, env.action_size), _net(name), 2
    env, plan, st = _plan(gpu, name, N, H, net, seed=5)
    plan.set_objective(**rec.kwargs())
    oenv, s0, key = _oenv(orc, env), _state(st), gpu.prng_key(6)
    prev = oc.Prev(rec.prev0)
    inner = oc.ObjectiveEnv(oenv, rec, prev)
    ve = vc.ValueEnv(inner, net)
    ep = plan.run_mpc(key, T, K, E)
    ref = oc.episode(oenv, rec, s0, key, N, H, ND, 0.1, T, K, E, env=ve, prev=prev, impl=_impl())
    _equal(ep, ref, f"{name}: objective, then value")
    ret, cost = plan.peek_objective()
    same_bits(ret, inner.last[1], "ret")
    same_bits(cost, inner.last[2], "cost")
    same_bits(plan.peek_value(), ve.last[1], "V")
    plan.set_value(None)
    assert not np.array_equal(plan.run_mpc(key, T, K, E)["means"], ep["means"])
    plan.close()


def test_demo_plan_blends_on_the_rewards_the_record_leaves(gpu, orc_omp):
    from mbd_hip.planners.mbd_planner import Plan
    orc = orc_omp
    name, N, H, Nd = "humanoidtrack", 33, 50, 4
    env = _env(name)
    net = _net(name, "S-3-1")
    plan = Plan(env, _args(name, N, H, Nd, enable_demo=True))
    st, key = env.reset(gpu.prng_key(3)), gpu.prng_key(4)
    plan.set_state0(st)
    base = plan.run(key)[0]
    plan.set_value(net.value_net())
    mu, rm, rf, _ = plan.run(key)
    oenv = _oenv(orc, env)
    ve = vc.ValueEnv(oenv, net)
    want = oc.plan(orc, oenv, oc.Record(), _state(st), key, N, H, Nd, 0.1, _impl(), enable_demo=True, env=ve)
    same_bits(mu, want["mu_0ts"], "demo plan: means")
    same_bits(rm, want["rew_means"], "demo plan: mean rewards")
    same_bits(plan.peek_value(), ve.last[1], "demo plan: V")
    assert not np.array_equal(mu, base)
    plan.close()


# ---- closed loop ------------------------------------------------------------------------------------------------------------------
def test_session_is_the_episode(gpu):
    name, N, H, E = "hopper", 70, 7, 2
    env, plan, st = _plan(gpu, name, N, H, _net(name), seed=5)
    key = gpu.prng_key(6)
    ep = plan.run_mpc(key, T, K, E)
    with plan.mpc_open(key, K, E) as s:
        means = np.stack([s.tick(ep["states"][t])["mean"] for t in range(T)])
    same_bits(means, ep["means"], "a session fed the episode's states")
    plan.close()


@pytest.mark.parametrize("um", [0, 1], ids=["mbd", "mppi"])
def test_sweep_of_three_is_the_single_plans(gpu, um):
    from mbd_hip.planners import path_integral
    from mbd_hip.planners.mbd_planner import Plan, Sweep
    name, N, H, E, P = "hopper", 70, 7, 2, 3
    env = _env(name)
    net = _net(name)
    a = _args(name, N, H) if um == 0 else path_integral.Args(env_name=name, Nsample=N, Hsample=H, Nrefine=ND, temp_sample=0.1,
                                                              disable_recommended_params=True)
    keys = np.array([gpu.prng_key(60 + k) for k in range(P)], np.uint32)
    states = [env.reset(gpu.prng_key(k)) for k in range(P)]
    sw = Sweep(env, a, P, update_method=um)
    for k in range(P):
        sw.set_state0(k, states[k])
    flat = sw.run(keys)[0]
    sw.set_value(net.value_net())
    if um:
        sw.set_mpc_sigma(1.0, 0.5, 0.0)
    mu = sw.run(keys)[0]
    sw.set_mpc_pick()
    ep = sw.run_mpc(keys, T, K, E)
    sess = None
    if um == 0:
        with sw.mpc_open(keys, K, E) as s:
            sess = np.stack([s.tick(ep["states"][:, t])["mean"] for t in range(T)], axis=1)
    sw.clear_mpc_pick()
    sw.set_value(None)
    same_bits(sw.run(keys)[0], flat, "a cleared record")
    sw.close()
    assert not np.array_equal(mu, flat)
    for k in range(P):
        p = Plan(env, a, update_method=um)
        p.set_state0(states[k])
        p.set_value(net.value_net())
        if um:
            p.set_mpc_sigma(1.0, 0.5, 0.0)
        same_bits(mu[k], p.run(keys[k])[0], f"plan {k}: open loop")
        p.set_mpc_pick()
        one = p.run_mpc(keys[k], T, K, E)
        _equal({f: ep[f][k] for f in _LOGS}, one, f"episode {k}")
        same_bits(ep["pick"][k]["rets"], one["pick"]["rets"], f"episode {k}: the pick's returns")
        if sess is not None:
            same_bits(sess[k], ep["means"][k], f"session {k}")
        p.close()


def test_two_unequal_shards_give_the_unsharded_rewards(gpu):
    import torch
    from mbd_hip.planners.mbd_planner import Plan
    for name, N, H in (("humanoidrun", 40, 5), ("car2d", 33, 6)):
        env = _env(name)
        Nu = env.action_size
        net = _net(name)
        st = env.reset(gpu.prng_key(3))
        i = ND - 2
        Ybar = (np.random.default_rng(1).normal(size=(H, Nu)) * 0.3).astype(np.float32)
        d_Y = torch.tensor(Ybar.reshape(-1), device="cuda")
        key = gpu.key_array(gpu.prng_key(12))
        out = {}
        for tag, (b, c) in (("all", (0, N)), ("lo", (0, 27)), ("hi", (27, N - 27))):
            plan = Plan(env, _args(name, N, H), shard_begin=b, shard_count=c)
            plan.set_state0(st)
            plan.set_value(net.value_net())
            d_r = torch.full((c,), float("nan"), device="cuda")
            gpu.check(plan.lib.mbd_plan_sample_rollout(plan.h, i, key, d_Y.data_ptr(), d_r.data_ptr(), None, None))
            torch.cuda.synchronize()
            out[tag] = (d_r.cpu().numpy(), plan.peek_value())
            plan.close()
        for j, what in enumerate(("rews", "V")):
            same_bits(np.concatenate([out["lo"][j], out["hi"][j]]), out["all"][j], f"{name}: {what}")
        assert np.isfinite(out["all"][0]).all() and np.ptp(out["all"][1]) > 0


@pytest.mark.parametrize("name,N,H", [("hopper", 70, 7), ("car2d", 33, 6)])
def test_pick_returns_include_the_value(gpu, orc, name, N, H):
    """A pick record's three logged returns are the checker's rollouts of the three slots with scale * V of their final states."""
    net, E = _net(name), 2
    env, plan, st = _plan(gpu, name, N, H, net, seed=5)
    plan.set_mpc_pick()
    oenv, s0, key = _oenv(orc, env), _state(st), gpu.prng_key(6)
    ep = plan.run_mpc(key, T, K, E)
    ref = pick_checker.episode(vc.ValueEnv(oenv, net), s0, key, N, H, ND, 0.1, T, K, E, 7, impl=_impl(), plant=oenv)
    _equal(ep, ref, f"{name}: pick")
    same_bits(ep["pick"]["rets"], ref["rets"], "the three returns")
    assert np.array_equal(ep["pick"]["choice"], ref["choice"]) and np.array_equal(ep["pick"]["best"], ref["best"])
    plain = pick_checker.episode(oenv, s0, key, N, H, ND, 0.1, 1, K, E, 7, impl=_impl())
    assert not np.array_equal(plain["rets"][0], ref["rets"][0])
    plan.close()


# ---- containment ------------------------------------------------------------------------------------------------------------------
def test_diverged_candidates_stay_in_their_rows_and_a_weighting_record_drops_them(gpu, orc):
    """weighting_combined_inputs' one-step launch: the hopper whose actuator 0 has a gear of 1e30 under the noise shape of 3e-5 on
    that column — some candidates diverge from finite inputs, some do not.  The healthy rows hold the checker's rews + scale * V bit
    for bit, a diverged row is finite nowhere the checker's is not; then the score under a rejecting weighting record gives the
    checker's weights of that buffer and a finite mean."""
    import torch
    from mbd_hip.envs.base import RigidBodyEnv, State
    from mbd_hip.planners.mbd_planner import Plan
    c = wci.STEP
    N, i, H = c["N"], c["i"], wci.H
    ref = wci.divergence_step(orc, 0, _impl())
    bad = wci.models()[1]
    env = RigidBodyEnv(wci.NAME, model=bad)
    net = vi.net("hopper", "S-65-64-1", "relu", rel_xy=True, scale=0.37)
    plan = Plan(env, _args(wci.NAME, N, H, c["Nd"]))
    plan.set_state0(State(np.asarray(ref["s0"], np.float32), None, np.float32(0.0), np.float32(0.0), {}))
    plan.set_noise_shape(wci.shape(plan.Nu))
    plan.set_value(net.value_net())
    ks = gpu.key_array(gpu.prng_key(c["key_seed"]))
    d_mu = torch.tensor(ref["mu"].reshape(-1), device="cuda")
    d_r = torch.full((N,), 7.0, device="cuda")
    gpu.check(plan.lib.mbd_plan_sample_rollout(plan.h, i, ks, d_mu.data_ptr(), d_r.data_ptr(), None, None))
    torch.cuda.synchronize()
    rews, V = d_r.cpu().numpy(), plan.peek_value()
    same_bits(plan.peek()[0], ref["Y0s"], "the candidates")
    oe = wci.oenv(orc, bad)
    fin = vc.final_states(oe, ref["s0"], ref["Y0s"])
    want_v = vc.value(orc, net, fin)
    want = vc.add(ref["rews"], net.scale, want_v)
    ok = np.isfinite(ref["rews"]) & np.isfinite(fin).all(axis=1)
    print(f"healthy {int(ok.sum())} of {N}; finite V {int(np.isfinite(V).sum())}")
    assert 0 < ok.sum() < N
    same_bits(V[ok], want_v[ok], "healthy rows: V")
    same_bits(rews[ok], want[ok], "healthy rows: rews")
    assert not (np.isfinite(V) & ~np.isfinite(want_v)).any() and not (np.isfinite(rews) & ~np.isfinite(want)).any()
    same_bits(vc.canon(V), vc.canon(want_v), "every row: V")
    same_bits(vc.canon(rews), vc.canon(want), "every row: rews")
    plan.set_weighting(**wi.REJECT.kwargs())
    out, rm = torch.full((H * plan.Nu,), 7.0, device="cuda"), torch.zeros(1, device="cuda")
    gpu.check(plan.lib.mbd_plan_score_update(plan.h, i, ks, d_mu.data_ptr(), d_r.data_ptr(), None, out.data_ptr(), rm.data_ptr(), None))
    torch.cuda.synchronize()
    res = wc.weigh(orc, rews, wci.TEMP, wi.REJECT)
    w = plan.peek()[2]
    same_bits(w, res["weights"], "weights under the rejecting record")
    assert res["kept"] == int(np.isfinite(rews).sum()) and (w[~np.isfinite(rews)].view(np.uint32) == 0).all()
    assert np.isfinite(out.cpu().numpy()).all()
    plan.close()


def test_a_diverged_plan_of_a_sweep_stays_alone(gpu):
    from mbd_hip.envs import get_env
    from mbd_hip.envs.base import State
    from mbd_hip.planners.mbd_planner import Args, Plan, Sweep
    name, kernel, N, _ = ci.SWEEPS[0]
    env = get_env(name)
    H, P = ci.SWEEP_H, ci.SWEEP_P
    a = Args(env_name=name, Nsample=N, Hsample=H, Ndiffuse=ci.SWEEP_ND, temp_sample=0.1, disable_recommended_params=True, not_render=True)
    sts = [env.reset(gpu.prng_key(20 + k)) for k in range(P)]
    S = np.asarray(sts[0].pipeline_state, np.float32).size
    rng = np.random.default_rng(S)
    net = vc.Net([(rng.normal(size=(33, S)) * 0.2).astype(np.float32), (rng.normal(size=(1, 33)) * 0.3).astype(np.float32)],
                 [np.zeros(33, np.float32), np.zeros(1, np.float32)], "tanh", rel_xy=True, scale=0.37)
    s = np.asarray(sts[1].pipeline_state, np.float32)
    sts[1] = State(ci.poison_state(s.reshape(-1, 13)).reshape(s.shape), None, np.float32(0), np.float32(0), {})
    keys = np.stack([gpu.prng_key(40 + k) for k in range(P)])
    sw = Sweep(env, a, P)
    for k in range(P):
        sw.set_state0(k, sts[k])
    sw.set_value(net.value_net())
    mu, rm, rf, _ = sw.run(keys)
    sw.close()
    assert not np.isfinite(rm[1]).any()
    for k in (0, 2):
        p = Plan(env, a)
        p.set_state0(sts[k])
        base = p.run(keys[k])[0]
        p.set_value(net.value_net())
        mu1, rm1, _, _ = p.run(keys[k])
        p.close()
        assert np.isfinite(mu1).all() and np.isfinite(rm1).all() and not np.array_equal(mu1, base)
        same_bits(mu[k], mu1, f"plan {k}: means")
        same_bits(rm[k], rm1, f"plan {k}: mean rewards")


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_ensemble_and_value_refuse_each_other(gpu):
    from mbd_hip.envs.base import RigidBodyEnv
    name = "hopper"
    env = _env(name)
    member = RigidBodyEnv(name, model=env.sys.scaled(mass=1.3))
    net = _net(name)
    env, plan, st = _plan(gpu, name, 64, 7, net)
    with pytest.raises(gpu.MbdError, match="value record") as e:
        plan.set_ensemble([None, member], "mean")
    assert e.value.code == gpu.MBD_ERR_STATE
    plan.run(gpu.prng_key(1))  # (the refused call left no ensemble behind)
    plan.peek_value()
    plan.set_value(None)
    plan.set_ensemble([None, member], "mean")
    with pytest.raises(gpu.MbdError, match="ensemble record") as e:
        plan.set_value(net.value_net())
    assert e.value.code == gpu.MBD_ERR_STATE
    plan.run(gpu.prng_key(1))
    plan.peek_ensemble()
    plan.close()


def test_c_caller_sets_a_linear_value(gpu, tmp_path):
    """examples/mbd_control.c --value from plain C: the rewards of its ticks are those of the Python session under the same record —
    one layer, V = z of link 0, scale 1 / H, seed 0's reset and key, rejection on — and differ from the run without it."""
    libdir = os.path.join(ROOT, "model-based-diffusion_amd", "lib")
    exe = str(tmp_path / "mbd_control")
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "mbd_control.c"),
                    "-o", exe, "-L", libdir, "-lmbd_hip", f"-Wl,-rpath,{libdir}", "-lm"], check=True)
    name, N, H, Tc = "hopper", 64, 7, 5

    def rewards(*extra):
        out = subprocess.run([exe, name, str(N), str(H), str(ND), str(K), str(Tc), "0", *extra], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        return [np.float32(float(ln.split()[3])) for ln in out.stdout.strip().splitlines() if ln.startswith("tick ")]

    got, plain = rewards("--value"), rewards()
    from mbd_hip.planners.mbd_planner import Plan
    from mbd_hip.planners.value import ValueNet
    env = _env(name)
    rng_episode, rng_reset = gpu.prng_split(gpu.prng_key(0), 2, 1)
    plan = Plan(env, _args(name, N, H))
    plan.set_state0(env.reset(rng_reset))
    w = np.zeros((1, env._state_size), np.float32)
    w[0, 2] = 1.0
    plan.set_value(ValueNet([w], [np.zeros(1, np.float32)], scale=1.0 / H))
    plan.set_weighting(reject_nonfinite=True)
    ep = plan.run_mpc(rng_episode, Tc, K, 1)
    plan.close()
    assert got == [np.float32(r) for r in ep["rewards"]] and got != plain


# ---- the command line -------------------------------------------------------------------------------------------------------------
def test_command_line(gpu, orc, tmp_path):
    """--value at the sizes of tests/test_mpc_batch.py::_cli: the JSON line gains value and value_scale and nothing else, and the
    episode's means are the plan's under the same record with scale = value_scale / Hsample."""
    from test_mpc_batch import _SINGLE_KEYS, _cli
    net = _net("hopper", "S-3-1", scale=1.0)
    path = str(tmp_path / "v.npz")
    net.value_net().save(path)
    res, ep = _cli(tmp_path, "--seed", "2", "--value", path, "--value_scale", "2.5")
    assert set(res) == _SINGLE_KEYS | {"value", "value_scale"} and (res["value"], res["value_scale"]) == (path, 2.5)
    from mbd_hip.planners.mbd_planner import Plan
    from mbd_hip.planners.mpc import _reset_and_key
    from mbd_hip.planners.value import terminal_scale
    env = _env("hopper")
    st, key = _reset_and_key(env, 2)
    plan = Plan(env, _args("hopper", 128, 20, 10))
    plan.set_state0(st)
    plan.set_value(net.value_net(), terminal_scale(2.5, 20))
    want = plan.run_mpc(key, 4, 3, 2)
    plan.set_value(None)
    flat = plan.run_mpc(key, 4, 3, 2)
    plan.close()
    same_bits(ep["means"], want["means"], "the command line's means")
    assert not np.array_equal(flat["means"], want["means"])
