"""-m gpu: the zone record (include/mbd_hip.h mbd_zones; DESIGN.md section 1 "N20 zones") against the checker plus the numpy
restatement tests/zones_checker.py.  Comparison rule: finite values by bit pattern, non-finite ones by class, the NaNs of a clearance
as the canonical pattern.

  the kernel alone   mbd_debug_zones_step on the table of tests/zones_inputs.py — B in {1, 5}, H in {1, 50, 64, 65}, K in {1, 3, 8},
                     Z in {1, 16} — and at B = 37 and B = 1024
  to the checker     one diffusion step and whole plans: humanoidrun tracked [0, last, 5] (N 64 and 37, H 50 and 7) and ant tracked
                     [8, 0, 4] (N 16), under MBD and mppi; once each beside an objective, a value, a weighting and an elite record
  identity           a record whose every weight is 0, a record set and cleared
  closed loop        an episode (T = 3, K = 2, E = 2) with its log of the executed steps, a session fed its states, update_zones
                     between two ticks, a sweep of three temperatures with its lockstep episodes and its session
  refusals           the env, the plan and the records a zone record does not go with; the plant's tracked links at the run call
  the command line   mpc.py --zones --zone_links, alone, with --online and with --n_episodes"""
import functools
import types

import numpy as np
import pytest

import objective_checker as oc
import zones_checker as zc
import zones_inputs as zi
from oracle import planner as op
from state_inputs import same_bits

pytestmark = pytest.mark.gpu

F32 = np.float32
ND, T, K, E = zi.ND, 3, 2, 2
_LOGS = ("means", "actions", "rewards", "states")


@pytest.fixture(scope="module")
def gpu(lib):
    from mbd_hip import _capi
    if _capi.device_count() < 1:
        pytest.fail("tests/test_gpu_zones.py needs a GPU")
    return _capi


def _impl():
    from mbd_hip.envs.base import prng_impl
    return prng_impl()


def _links(name, links):
    from conftest import load_model
    n = load_model(name).n_links
    return tuple(n - 1 if l == "last" else int(l) for l in links)


@functools.lru_cache(maxsize=None)
def _env(name, links):
    from mbd_hip.envs import get_env
    return get_env(name, track=_links(name, links))


@functools.lru_cache(maxsize=None)
def _placed(orc, name, links, N, H):
    """(model, s0, zones, resolved zones) of a whole-plan case: the reference is computed once and left unchanged."""
    m = zi.plan_model(name, links)
    s0 = np.ascontiguousarray(orc.forward(m.to_struct(), m.init_q, np.zeros(m.qd_size(), F32)), F32).reshape(-1)
    zones, _ = zi.place(orc, m, s0, N, H)
    return m, s0, zones


def _oenv(orc, env):
    return op.OracleEnv(orc, env.env_name, env.sys.to_struct(), xref=env.xref, rew_xref=env.rew_xref, init_q=env.sys.init_q)


def _args(name, N, H, um=0, temp=0.1):
    if um:
        from mbd_hip.planners import path_integral
        return path_integral.Args(env_name=name, Nsample=N, Hsample=H, Nrefine=ND, temp_sample=temp, disable_recommended_params=True)
    from mbd_hip.planners.mpc import MpcArgs
    return MpcArgs(env_name=name, Nsample=N, Hsample=H, Ndiffuse=ND, temp_sample=temp, disable_recommended_params=True, not_render=True)


def _plan(env, name, N, H, s0, zones=None, um=0, temp=0.1, **kw):
    from mbd_hip.planners.mbd_planner import Plan
    plan = Plan(env, _args(name, N, H, um, temp), update_method=um, **kw)
    plan.set_state0(types.SimpleNamespace(pipeline_state=s0))
    if zones is not None:
        plan.set_zones(zones)
    return plan


def _equal(a, b, what=""):
    for k in _LOGS:
        x, y = np.asarray(a[k], F32), np.asarray(b[k], F32)
        assert x.size == y.size, f"{what}: {k} sizes"
        same_bits(x.reshape(y.shape), y, f"{what}: {k} differ")


# ---- the kernel alone -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H", [(B, H) for B in (1, 5) for H in (1, 50, 64, 65)])
def test_kernel_matches_the_checker(gpu, B, H):
    for Kt in (1, 3, 8):
        for Z in (1, 16):
            zones, xpos, rews = zi.crafted(B, H, Kt, Z)
            rec = gpu.zones_record(zones, Kt)
            got = gpu.debug_zones_step(rec, xpos, rews)
            zc.same_launch(got, zc.launch(zones, xpos, rews), f"B={B} H={H} K={Kt} Z={Z}")
            host = gpu.debug_zones_host(rec, xpos, rews)
            zc.same_launch(got, host, f"B={B} H={H} K={Kt} Z={Z}: the device against the host text")


@pytest.mark.parametrize("B", [37, 1024])
def test_kernel_over_many_workgroups(gpu, B):
    """Rows that are no multiple of the workgroup's four, and 256 workgroups: 37 crafted rows, tiled with a row-dependent shift."""
    H, Kt, Z = 50, 3, 16
    zones, x37, r37 = zi.crafted(37, H, Kt, Z)
    reps = (B + 36) // 37
    xpos = np.tile(x37, (reps, 1, 1, 1))[:B].copy()
    xpos += (np.arange(B, dtype=F32) // 37 * F32(0.0078125))[:, None, None, None]
    rews = np.tile(r37, reps)[:B].copy()
    got = gpu.debug_zones_step(gpu.zones_record(zones, Kt), xpos, rews)
    zc.same_launch(got, zc.launch(zones, xpos, rews), f"B={B}")
    # without rewards the launch stores pen and clr alone
    alone = gpu.debug_zones_step(gpu.zones_record(zones, Kt), xpos)
    assert "rews" not in alone
    zc.same(alone["pen"], got["pen"], "pen without rews")


# ---- one step and whole plans to the checker ------------------------------------------------------------------------------------
@pytest.mark.parametrize("um", [0, 1], ids=["mbd", "mppi"])
@pytest.mark.parametrize("name,links,N,H", zi.PLANS, ids=[f"{p[0]}-N{p[2]}-H{p[3]}" for p in zi.PLANS])
def test_plan_and_step_match_the_checker(gpu, orc, name, links, N, H, um):
    m, s0, zones = _placed(orc, name, links, N, H)
    env = _env(name, links)
    assert bytes(env.sys.to_struct()) == bytes(m.to_struct()), "get_env(track=...) is Model.tracked of the built-in model"
    plan = _plan(env, name, N, H, s0, zones, um)
    oenv, key = _oenv(orc, env), gpu.prng_key(6)
    ze = zc.ZoneEnv(oenv, zones)
    ze.log = []
    what = f"{name} N={N} H={H} um={um}"
    out = plan.run(key)
    if um == 0:
        want = oc.plan(orc, oenv, oc.Record(), s0, key, N, H, ND, 0.1, _impl(), env=ze)
        same_bits(out[1], want["rew_means"], f"{what}: mean rewards")
        same_bits(F32(out[2]), F32(want["rew_final"]), f"{what}: the final reward is the env's own")
    else:
        want = oc.pi_plan(orc, ze, oc.Record(), s0, key, N, H, ND, 0.1, "mppi", _impl())
    same_bits(out[0], want["mu_0ts"], f"{what}: means")
    pk = plan.peek_zones()
    zc.same(pk["pen"], ze.last["pen"], f"{what}: pen of the last step")
    zc.same_clr(pk["clr"], ze.last["clr"], f"{what}: clr of the last step")
    # (the first step draws the widest candidates: there the record bites, as the census of the case says; the last may not)
    assert (ze.log[0]["pen"] != 0).any(), f"{what}: the record bites"
    if um == 0:  # one step through the phase call: the rewards buffer holds rews - pen
        import torch
        Ybar = (np.random.default_rng(N + H).normal(size=(H, env.action_size)) * 0.3).astype(F32)
        d_Y, d_r = torch.tensor(Ybar.reshape(-1), device="cuda"), torch.full((N,), float("nan"), device="cuda")
        gpu.check(plan.lib.mbd_plan_sample_rollout(plan.h, ND - 2, gpu.key_array(gpu.prng_key(10 + N)), d_Y.data_ptr(), d_r.data_ptr(), None, None))
        torch.cuda.synchronize()
        Y0s, rewss, _ = plan.peek()
        ref_rewss, xpos = orc.rollout(m.to_struct(), s0, np.ascontiguousarray(Y0s, F32), want_xpos=True)
        same_bits(rewss, ref_rewss, f"{what}: rewss is not touched")
        ref = zc.launch(zones, xpos, op.mean_h(orc, np.ascontiguousarray(ref_rewss, F32)))
        zc.same(d_r.cpu().numpy(), ref["rews"], f"{what}: the rewards of one step")
        pk = plan.peek_zones()
        zc.same(pk["pen"], ref["pen"], f"{what}: pen of one step")
        zc.same_clr(pk["clr"], ref["clr"], f"{what}: clr of one step")
    plan.close()


_BESIDE = ("objective", "value", "weighting", "elites")


@pytest.mark.parametrize("other", _BESIDE)
def test_beside_another_record(gpu, orc, other):
    """The launch sits behind the objective's and in front of the value's; the weighting and the elite selection read the rewards
    it wrote."""
    name, links, N, H = zi.PLANS[1]  # humanoidrun, 64 candidates, 7 rows
    m, s0, zones = _placed(orc, name, links, N, H)
    env = _env(name, links)
    plan = _plan(env, name, N, H, s0, zones)
    oenv, key = _oenv(orc, env), gpu.prng_key(7)
    if other == "objective":
        from test_objective import gpu_record
        rec = gpu_record(H, env.action_size)
        plan.set_objective(**rec.kwargs())
        inner = oc.ObjectiveEnv(oenv, rec, oc.Prev(rec.prev0))
        ze = zc.ZoneEnv(inner, zones)
        want = oc.plan(orc, oenv, rec, s0, key, N, H, ND, 0.1, _impl(), env=ze)
    elif other == "value":
        import value_checker as vc
        import value_inputs as vi
        net = vi.net(name, "S-65-64-1", "tanh", rel_xy=True, scale=0.37)
        plan.set_value(net.value_net())
        ze = zc.ZoneEnv(oenv, zones)
        ve = vc.ValueEnv(ze, net)
        want = oc.plan(orc, oenv, oc.Record(), s0, key, N, H, ND, 0.1, _impl(), env=ve)
    elif other == "weighting":
        import weighting_checker as wc
        wrec = wc.Record(reject_nonfinite=True, ess_frac=0.5, temp_min=0.01, temp_max=10.0, iters=12)
        plan.set_weighting(reject_nonfinite=True, ess_frac=0.5, temp_min=0.01, temp_max=10.0, iters=12)
        ze = zc.ZoneEnv(oenv, zones)
        want = wc.run(orc, ze, s0, key, N, H, ND, 0.1, wrec, _impl())
    else:
        import elites_checker as ec
        plan.set_elites(4, nominal=True, carry=False)
        ze = zc.ZoneEnv(oenv, zones)
        want = ec.run(orc, ze, s0, key, N, H, ND, 0.1, ec.State(ec.Record(4, True, False), H, env.action_size, True), impl=_impl())
    mu, rm = plan.run(key)[:2]
    same_bits(mu, want["mu_0ts"], f"beside {other}: means")
    same_bits(rm, want["rew_means"], f"beside {other}: mean rewards")
    zc.same(plan.peek_zones()["pen"], ze.last["pen"], f"beside {other}: pen")
    plan.clear_zones()
    assert not np.array_equal(plan.run(key)[0], mu), f"beside {other}: the zone record changes the plan"
    plan.close()


# ---- identity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("um", [0, 1], ids=["mbd", "mppi"])
def test_records_that_change_nothing(gpu, orc, um):
    name, links, N, H = zi.PLANS[3]  # humanoidrun, 37 candidates, 7 rows
    m, s0, zones = _placed(orc, name, links, N, H)
    plan = _plan(_env(name, links), name, N, H, s0, None, um)
    key = gpu.prng_key(8)
    if um:
        plan.set_mpc_sigma(1.0, 0.5, 0.0)
    ref_run, ref_ep = plan.run(key), plan.run_mpc(key, T, K, E)

    def same(what):
        got = plan.run(key)
        for x, y in zip(got[:3], ref_run[:3]):
            same_bits(np.asarray(x, F32), np.asarray(y, F32), f"{what}: run")
        _equal(plan.run_mpc(key, T, K, E), ref_ep, what)

    plan.set_zones([dict(z, weight=0.0) for z in zones])
    same("every weight 0")
    assert not zc.bits(plan.peek_zones()["pen"]).any(), "every weight 0: pen is +0"
    plan.set_zones(zones)
    assert not np.array_equal(plan.run(key)[0], ref_run[0])
    plan.clear_zones()
    same("a record set, then cleared")
    plan.close()


# ---- closed loop ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,links,N,H", [zi.PLANS[3], zi.PLANS[5]], ids=["humanoidrun", "ant"])
def test_episode_session_and_update(gpu, orc, name, links, N, H):
    m, s0, zones = _placed(orc, name, links, N, H)
    env = _env(name, links)
    plan = _plan(env, name, N, H, s0, zones)
    oenv, key = _oenv(orc, env), gpu.prng_key(9)
    ep = plan.run_mpc(key, T, K, E)
    ze = zc.ZoneEnv(oenv, zones)
    ref = oc.episode(oenv, oc.Record(), s0, key, N, H, ND, 0.1, T, K, E, env=ze, prev=oc.Prev(), impl=_impl())
    _equal(ep, ref, f"{name}: the episode")
    pen, clr = zc.executed(orc, m.to_struct(), zones, ep["states"], ep["actions"], E)
    assert ep["zone_pen"].shape == (T * E,) and ep["zone_clear"].shape == (T * E,)
    zc.same(ep["zone_pen"], pen, f"{name}: zone_pen of the executed steps")
    zc.same_clr(ep["zone_clear"], clr, f"{name}: zone_clear of the executed steps")
    # a session fed the episode's states returns its means
    with plan.mpc_open(key, K, E) as s:
        means = np.stack([s.tick(ep["states"][t])["mean"] for t in range(T)])
    same_bits(means, ep["means"], f"{name}: a session fed the episode's states")
    # update_zones between two ticks: the episode replayed with the second table from that tick
    second = [dict(z, center=[c + 0.05 for c in z["center"]], weight=2.0 * z["weight"] + 1.0) for z in zones]
    import mpc_online_checker as online
    sess = online.Session(zc.ZoneEnv(oenv, zones), key, N, H, ND, 0.1, K, E, impl=_impl())
    want = []
    for t in range(T):
        if t == 1:
            sess.oenv.zones = second
        want.append(sess.tick(ep["states"][t])["mean"])
    with plan.mpc_open(key, K, E) as s:
        got = [s.tick(ep["states"][0])["mean"]]
        s.submit(ep["states"][1])
        with pytest.raises(gpu.MbdError, match="in flight") as e:
            s.update_zones(second)
        assert e.value.code == gpu.MBD_ERR_STATE
        s.collect()
    with plan.mpc_open(key, K, E) as s:
        got = [s.tick(ep["states"][0])["mean"]]
        s.update_zones(second)
        got += [s.tick(ep["states"][t])["mean"] for t in range(1, T)]
        with pytest.raises(gpu.MbdError, match="session is open"):
            plan.set_zones(zones)
    same_bits(np.stack(got), np.stack(want), f"{name}: update_zones between two ticks")
    assert not np.array_equal(got[1], ep["means"][1]), "the second table moves the plan"
    plan.close()


def test_sweep_of_three_temperatures_is_the_single_plans(gpu, orc):
    from mbd_hip.planners.mbd_planner import Sweep
    name, links, N, H = zi.PLANS[3]
    P, temps = 3, (0.05, 0.1, 0.3)
    m, s0, zones = _placed(orc, name, links, N, H)
    env = _env(name, links)
    keys = np.array([gpu.prng_key(60 + k) for k in range(P)], np.uint32)
    st = types.SimpleNamespace(pipeline_state=s0)
    sw = Sweep(env, _args(name, N, H), P, temps=temps)
    for k in range(P):
        sw.set_state0(k, st)
    sw.set_zones(zones)
    mu, rm, rf, _ = sw.run(keys)
    peeks = [sw.peek_zones(k) for k in range(P)]
    eps = sw.run_mpc(keys, T, K, E)
    with sw.mpc_open(keys, K, E) as s:
        sess = np.stack([s.tick(eps["states"][:, t])["mean"] for t in range(T)], axis=1)  # [P, T, H, Nu]
    sw.close()
    for k in range(P):
        plan = _plan(env, name, N, H, s0, zones, temp=temps[k])
        one = plan.run(keys[k])
        same_bits(mu[k], one[0], f"plan {k}: means")
        same_bits(rm[k], one[1], f"plan {k}: mean rewards")
        pk = plan.peek_zones()
        zc.same(peeks[k]["pen"], pk["pen"], f"plan {k}: pen")
        zc.same_clr(peeks[k]["clr"], pk["clr"], f"plan {k}: clr")
        ep = plan.run_mpc(keys[k], T, K, E)
        _equal({f: eps[f][k] for f in _LOGS}, ep, f"episode {k}")
        zc.same(eps["zone_pen"][k], ep["zone_pen"], f"episode {k}: zone_pen")
        zc.same_clr(eps["zone_clear"][k], ep["zone_clear"], f"episode {k}: zone_clear")
        same_bits(sess[k], ep["means"], f"episode {k}: the sweep's session")
        plan.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_handles(gpu, orc):
    from mbd_hip.envs import get_env
    from mbd_hip.envs.base import RigidBodyEnv
    from mbd_hip.planners.mbd_planner import Plan, Sweep
    name, links, N, H = zi.PLANS[3]
    m, s0, zones = _placed(orc, name, links, N, H)
    env = _env(name, links)
    U, S, I = gpu.MBD_ERR_UNSUPPORTED, gpu.MBD_ERR_STATE, gpu.MBD_ERR_INVALID

    def refused(call, code, word):
        with pytest.raises((gpu.MbdError, ValueError), match=word) as e:
            call()
        assert getattr(e.value, "code", code) == code, (word, e.value)

    # the env: car2d, a model that tracks nothing
    for other in ("car2d", "humanoidrun"):
        e2 = get_env(other)
        p2 = Plan(e2, _args(other, 8, 4))
        rec = gpu.zones_record(zones, 3)
        import ctypes as C
        assert p2.lib.mbd_plan_set_zones(p2.h, C.byref(rec)) == U
        assert (b"car2d" if other == "car2d" else b"tracks no link") in p2.lib.mbd_last_error()
        p2.close()
    plan = _plan(env, name, N, H, s0)
    refused(lambda: plan.set_zones([dict(zones[0], links=0b1000)]), I, "n_track=3")
    refused(plan.peek_zones, S, "no zone record")
    refused(lambda: plan.update_zones(zones), S, "no zone record")
    # the records a zone record does not go with, in both orders
    for set_other, clear_other, word in ((lambda: plan.set_togo(2, 1), plan.clear_togo, "to-go"),
                                         (lambda: plan.set_mpc_pick(), plan.clear_mpc_pick, "pick"),
                                         (lambda: plan.set_ensemble([env, env]), plan.clear_ensemble, "ensemble")):
        set_other()
        refused(lambda: plan.set_zones(zones), U, word)
        clear_other()
        plan.set_zones(zones)
        refused(set_other, U, "zone record")
        plan.clear_zones()
    plan.set_zones(zones)
    refused(plan.peek_zones, S, "no diffusion step")
    with pytest.raises(gpu.MbdError, match="no episode") as e:
        gpu.check(plan.lib.mbd_plan_peek_mpc_zones(plan.h, None, None))
    assert e.value.code == S
    # at the run call: a plant whose tracked links differ
    plant = RigidBodyEnv(name, model=m.tracked([0, 1, 5]).scaled(mass=1.1))
    plan.set_mpc_plant(env=plant)
    refused(lambda: plan.run_mpc(gpu.prng_key(1), T, K, E), I, r"track_link\[1\]")
    plan.set_mpc_plant(env=RigidBodyEnv(name, model=m.scaled(mass=1.1)))
    assert plan.run_mpc(gpu.prng_key(1), T, K, E)["zone_pen"].shape == (T * E,)
    plan.close()
    # the plan: sharded, a demo plan
    sharded = Plan(env, _args(name, N, H), shard_begin=0, shard_count=N // 2)
    refused(lambda: sharded.set_zones(zones), S, "shard")
    sharded.close()
    track = get_env("humanoidtrack")
    from mbd_hip.planners.mpc import MpcArgs
    demo = Plan(track, MpcArgs(env_name="humanoidtrack", Nsample=8, Hsample=50, Ndiffuse=ND, enable_demo=True, disable_recommended_params=True))
    refused(lambda: demo.set_zones([dict(zones[0], links=1)]), U, "enable_demo")
    demo.close()
    sw = Sweep(env, _args(name, N, H), 2)
    sw.set_togo(2, 1)
    refused(lambda: sw.set_zones(zones), U, "to-go")
    sw.clear_togo()
    sw.set_zones(zones)
    refused(lambda: sw.set_togo(2, 1), U, "zone record")
    refused(lambda: sw.set_mpc_pick(), U, "zone record")
    refused(lambda: sw.peek_zones(2), I, "k=2")
    sw.close()


# ---- the command line -------------------------------------------------------------------------------------------------------------
def test_the_command_line(gpu, capsys):
    from mbd_hip.planners import mpc
    argv = ["--env_name", "humanoidrun", "--Nsample", "32", "--Hsample", "8", "--Ndiffuse", str(ND), "--n_ticks", str(T), "--warm_steps", str(K),
            "--exec_steps", str(E), "--disable_recommended_params", "--not_render", "--zone_links", "torso,5",
            "--zones", "out:0.3,0,1.2:0.2:0.3:5;goal:6,0,1.2:0.2:6:1:xy:torso"]
    res = mpc._main(argv)
    for f in ("zone_pen_mean", "zone_clear_min", "zone_hits", "zones", "zone_links"):
        assert f in res, f
    assert res["zone_pen_mean"] > 0 and np.isfinite(res["zone_clear_min"]) and res["zone_hits"] >= 0
    online = mpc._main(argv + ["--online"])
    assert online["zone_pen_mean"] == res["zone_pen_mean"] and online["zone_clear_min"] == res["zone_clear_min"], "the same episode"
    batch = mpc._main(argv + ["--n_episodes", "2"])
    assert batch["zone_hits"] >= res["zone_hits"] and "zone_pen_mean" in batch
    capsys.readouterr()
    plain = mpc._main(argv[:-4])
    assert not any(f.startswith("zone") for f in plain), "without the flags the line is what it was"


def test_c_caller_moves_a_goal_between_ticks(gpu, tmp_path):
    """examples/mbd_control.c --zones from plain C: a retracked humanoidrun, a pillar and a goal moved with mbd_plan_update_zones
    before every tick of the open session; every tick's line carries a finite mean penalty and a finite clearance."""
    import os
    import subprocess

    from conftest import ROOT
    libdir = os.path.join(ROOT, "model-based-diffusion_amd", "lib")
    exe = str(tmp_path / "mbd_control")
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "mbd_control.c"),
                    "-o", exe, "-L", libdir, "-lmbd_hip", f"-Wl,-rpath,{libdir}", "-lm"], check=True)
    out = subprocess.run([exe, "humanoidrun", "64", "10", "4", "2", "4", "--zones"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    ticks = [ln.split() for ln in out.stdout.strip().splitlines() if ln.startswith("tick ")]
    assert [int(t[1]) for t in ticks] == list(range(4))
    for t in ticks:
        pen, clr = float(t[t.index("pen") + 1]), float(t[t.index("clear") + 1])
        assert np.isfinite(pen) and pen > 0 and np.isfinite(clr), t
