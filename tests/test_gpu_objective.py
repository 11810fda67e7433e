"""-m gpu: the objective record (include/mbd_hip.h mbd_objective; DESIGN.md section 1 "N13 objective") against the checker's
restatement, tests/objective_checker.py.  Every comparison is by bit pattern or np.array_equal: the contract fixes every rounding.

  the kernel alone   one step, then peek_objective against the checker on peek()'s own Y0s and rewss: hopper, ant, humanoidrun
                     (lazy normals), car2d (materialised) at sizes where N is no multiple of the 2 or 8 candidates a wavefront or a
                     workgroup holds and Nu does not divide 32; with prev0 and without; H = 1; N = 1
  identity           no record, the NULL / zero record, all-ones weights, a record set and cleared: whole plans and episodes
  to the checker     whole plans and episodes: hopper, humanoidrun, car2d, an mppi and a cma-es plan; tick 0, prefixes
  prev across ticks  delay records, a plant with action noise, a session fed the episode's states, reset_mean
  composition        noise shape and basis, a demo plan and a demo episode, ensembles (one launch and M launches, both risks), sweeps and their
                     sessions, two unequal shards through the phase calls
  containment        a diverged member of an ensemble, a diverged plan of a sweep
  the command line   python -m mbd_hip.planners.mpc --discount --rate_cost

The records and the sizes of the kernel test come from tests/test_objective.py, which holds the checker to telling them apart."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import containment_inputs as ci
import ensemble_checker
import noise_basis_checker as nbc
import objective_checker as oc
from conftest import ROOT
from oracle import planner as op
from state_inputs import same_bits
from test_objective import GPU_SIZES, gpu_record

pytestmark = pytest.mark.gpu

_LOGS = ("means", "actions", "rewards", "states")
ND, T, K = 6, 3, 2


@pytest.fixture(scope="module")
def gpu(lib):
    from mbd_hip import _capi
    if _capi.device_count() < 1:
        pytest.fail("tests/test_gpu_objective.py needs a GPU")
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


def _plan(name, N, H, rec=None, seed=3, Nd=ND, **plan_kw):
    from mbd_hip.planners.mbd_planner import Plan
    env = _env(name)
    plan = Plan(env, _args(name, N, H, Nd), **plan_kw)
    st = env.reset(_capi().prng_key(seed))
    plan.set_state0(st)
    if rec is not None:
        plan.set_objective(**rec.kwargs())
    return env, plan, st


def _capi():
    from mbd_hip import _capi as c
    return c


def _same_last(plan, last, what):
    ret, cost = plan.peek_objective()
    same_bits(ret, last[1], f"{what}: ret of the last step")
    same_bits(cost, last[2], f"{what}: cost of the last step")


# ---- the kernel alone -------------------------------------------------------------------------------------------------------
_KERNEL = [(n,) + GPU_SIZES[n] for n in sorted(GPU_SIZES)] + [("hopper", 33, 1, 3), ("hopper", 1, 7, 3), ("humanoidrun", 9, 1, 17)]


@pytest.mark.parametrize("with_prev", [True, False], ids=["prev0", "noprev"])
@pytest.mark.parametrize("name,N,H,Nu", _KERNEL, ids=[f"{c[0]}-N{c[1]}-H{c[2]}" for c in _KERNEL])
def test_one_step_against_the_checker(gpu, orc, name, N, H, Nu, with_prev):
    """One diffusion step from a mean that is not zero.  ret and cost are the checker's on the step's own candidates and per-step
    rewards; the weights and the new mean are the checker's score update of ret - cost, so the rewards buffer holds exactly that."""
    import torch
    rec = gpu_record(H, Nu, prev0=with_prev)
    env, plan, st = _plan(name, N, H, rec)
    assert env.action_size == Nu
    i = ND - 2
    Ybar = (np.random.default_rng(N + H).normal(size=(H, Nu)) * 0.3).astype(np.float32)
    d_Y, d_rm = torch.tensor(Ybar.reshape(-1), device="cuda"), torch.zeros(1, device="cuda")
    key = gpu.key_array(gpu.prng_key(10 + N))
    gpu.check(plan.lib.mbd_plan_reverse_once(plan.h, i, key, d_Y.data_ptr(), d_rm.data_ptr(), None))
    torch.cuda.synchronize()
    Y0s, rewss, w = plan.peek()
    ret, cost = plan.peek_objective()
    plan.close()
    what = f"{name} N={N} H={H}"
    rews, want_ret, want_cost = oc.step(rewss, op.mean_h(orc, rewss), Y0s, rec, oc.clip(rec.prev0))
    print(f"{what}: ret {ret[:3]} cost {cost[:3]} (checker {want_ret[:3]} {want_cost[:3]})")
    same_bits(ret, want_ret, f"{what}: ret")
    same_bits(cost, want_cost, f"{what}: cost")
    assert np.isfinite(cost).all() and (cost > 0).all()
    a, ab, _ = orc.schedule(1e-4, 1e-2, ND)
    Ybar_im1, weights, rew_mean = orc.score_update(rews, Y0s, Ybar, float(a[i]), float(ab[i]), float(ab[i - 1]), 0.1, lp_demo=None,
                                                   rew_xref=env.rew_xref, literal=True)
    same_bits(w, weights, f"{what}: weights")
    same_bits(d_Y.cpu().numpy().reshape(H, Nu), Ybar_im1, f"{what}: the new mean")
    same_bits(np.float32(d_rm.item()), np.float32(rew_mean), f"{what}: rew_mean")


def test_peek_and_set_states(gpu):
    env, plan, st = _plan("hopper", 33, 4)
    lib = plan.lib
    assert lib.mbd_plan_peek_objective(plan.h, None, None) == gpu.MBD_ERR_STATE and b"no objective record" in lib.mbd_last_error()
    rec = gpu_record(4, 3)
    plan.set_objective(**rec.kwargs())
    assert lib.mbd_plan_peek_objective(plan.h, None, None) == gpu.MBD_ERR_STATE and b"no diffusion step" in lib.mbd_last_error()
    plan.run(gpu.prng_key(1))
    plan.peek_objective()
    for kw, field in ((dict(row_weight=np.ones(5)), "rows=5"), (dict(act_weight=np.ones(4)), "cols=4"),
                      (dict(row_weight=[1, 1, -1, 1]), "row_weight[2]"), (dict(prev0=[0, np.nan, 0]), "prev0[1]")):
        with pytest.raises(gpu.MbdError, match=field.replace("[", r"\[").replace("]", r"\]")):
            plan.set_objective(**kw)
    plan.peek_objective()  # (a refused call leaves the record)
    with plan.mpc_open(gpu.prng_key(2), K) as s:
        with pytest.raises(gpu.MbdError, match="session is open"):
            plan.set_objective(rate=1.0)
        s.tick(_state(st))
    plan.clear_objective()
    assert lib.mbd_plan_peek_objective(plan.h, None, None) == gpu.MBD_ERR_STATE
    plan.close()


# ---- identity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,N,H", [("hopper", 70, 7), ("humanoidrun", 40, 5)])
def test_records_that_change_nothing(gpu, name, N, H):
    env, plan, st = _plan(name, N, H)
    key = gpu.prng_key(8)
    ref_run = plan.run(key)
    ref_eps = [plan.run_mpc(key, T, K, E) for E in (1, 2)]

    def same(what):
        got = plan.run(key)
        for x, y in zip(got[:3], ref_run[:3]):
            same_bits(np.asarray(x, np.float32), np.asarray(y, np.float32), f"{name} {what}: run")
        for E, ref in zip((1, 2), ref_eps):
            _equal(plan.run_mpc(key, T, K, E), ref, f"{name} {what} E={E}")

    plan.set_objective()  # NULL weights, zero costs
    same("NULL / zero record")
    plan.set_objective(row_weight=np.ones(H, np.float32), prev0=np.full(env.action_size, 0.5, np.float32))
    same("all-ones weights")
    plan.set_objective(**gpu_record(H, env.action_size).kwargs())
    assert not np.array_equal(plan.run(key)[0], ref_run[0])
    plan.clear_objective()
    same("a record set, then cleared")
    plan.close()


# ---- whole plans and episodes to the checker ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,N,H", [("hopper", 70, 7), ("humanoidrun", 40, 5), ("car2d", 33, 6)])
def test_plan_and_episode_match_the_checker(gpu, orc, name, N, H):
    env = _env(name)
    rec = gpu_record(H, env.action_size)
    env, plan, st = _plan(name, N, H, rec, seed=5)
    oenv, s0, key = _oenv(orc, env), _state(st), gpu.prng_key(6)
    mu, rm, rf, _ = plan.run(key)
    want = oc.plan(orc, oenv, rec, s0, key, N, H, ND, 0.1, _impl())
    same_bits(mu, want["mu_0ts"], f"{name}: means")
    same_bits(rm, want["rew_means"], f"{name}: mean rewards")
    same_bits(np.float32(rf), np.float32(want["rew_final"]), f"{name}: the final reward is the env's own")
    _same_last(plan, want["last"], name)
    k0 = gpu.prng_split(key, 2, plan.cfg.prng_impl)[1]
    mu0 = plan.run(k0)[0]
    for E in (1, 2):
        ep, short = plan.run_mpc(key, T, K, E), plan.run_mpc(key, T - 1, K, E)
        ref = oc.episode(oenv, rec, s0, key, N, H, ND, 0.1, T, K, E, impl=_impl())
        _equal(ep, ref, f"{name} E={E}")
        for k in _LOGS:
            assert np.array_equal(short[k], ep[k][: len(short[k])]), k
        same_bits(ep["means"][0], mu0[-1], f"{name}: tick 0 is mbd_plan_run(k_0) under the record")
    ep = plan.run_mpc(key, T, K, 2)
    _same_last(plan, ref["last"], f"{name}: the episode's last step")
    # the record matters in every tick: without prev0 tick 0 differs, and the later ticks (whose prev is the episode's own) too
    plan.set_objective(**dict(rec.kwargs(), prev0=None))
    other = plan.run_mpc(key, T, K, 2)
    assert not np.array_equal(other["means"][0], ep["means"][0])
    plan.close()


@pytest.mark.parametrize("method", ["mppi", "cma-es"])
def test_path_integral_plan_and_episode_match_the_checker(gpu, orc, method):
    from mbd_hip.planners import path_integral
    from mbd_hip.planners.mbd_planner import Plan
    name, N, H, Nr, E = "hopper", 70, 7, 5, 2
    env = _env(name)
    rec = gpu_record(H, env.action_size)
    args = path_integral.Args(env_name=name, Nsample=N, Hsample=H, Nrefine=Nr, temp_sample=0.1, disable_recommended_params=True)
    plan = Plan(env, args, update_method=op.PI_METHODS[method])
    st, key = env.reset(gpu.prng_key(3)), gpu.prng_key(4)
    plan.set_state0(st)
    plan.set_objective(**rec.kwargs())
    oenv, s0 = _oenv(orc, env), _state(st)
    mu = plan.run(key)[0]
    want = oc.pi_plan(orc, oenv, rec, s0, key, N, H, Nr, 0.1, method, _impl())
    same_bits(mu, want["mu_0ts"], f"{method}: means")
    _same_last(plan, want["last"], method)
    sig = (1.0, 0.5, 0.0) if method == "mppi" else (1.0, 0.25, 2.0)
    plan.set_mpc_sigma(*sig)
    ep = plan.run_mpc(key, T, K, E)
    ref = oc.episode(oenv, rec, s0, key, N, H, Nr, 0.1, T, K, E, method=method, sigma=sig, impl=_impl())
    _equal(ep, ref, f"{method} episode")
    _same_last(plan, ref["last"], f"{method} episode")
    plan.close()


# ---- prev across ticks ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,given", [(1, True), (1, False), (2, True), (2, False)])
def test_delay_record_sets_the_first_previous_action(gpu, orc, D, given):
    """The first tick's prev is the clipped last row of the committed queue — rows0 (one value outside the clip), or zeros —,
    whatever prev0 says; afterwards clip(M_{t-1}[E-1]), the last row committed, as without a delay."""
    name, N, H, E = "hopper", 70, 7, 2
    env = _env(name)
    rec = gpu_record(H, env.action_size)
    env, plan, st = _plan(name, N, H, rec, seed=5)
    rows0 = None
    if given:
        rows0 = (np.random.default_rng(D).normal(size=(D * E, env.action_size)) * 0.5).astype(np.float32)
        rows0[-1, 1] = -1.75
    plan.set_mpc_delay(D, rows0)
    key = gpu.prng_key(6)
    ep = plan.run_mpc(key, T, K, E)
    ref = oc.episode(_oenv(orc, env), rec, _state(st), key, N, H, ND, 0.1, T, K, E, D=D, rows0=rows0, impl=_impl())
    _equal(ep, ref, f"D={D} rows0 {'given' if given else 'NULL'}")
    _same_last(plan, ref["last"], f"D={D}")
    plan.close()


def test_plant_noise_does_not_enter_the_previous_action(gpu, orc):
    """act_std > 0 on a heavier plant: prev is the commanded row clip(M_{t-1}[E-1]), not the disturbed one the plant was fed."""
    from mbd_hip.envs.base import RigidBodyEnv
    name, N, H, E = "hopper", 70, 7, 2
    env = _env(name)
    plant = RigidBodyEnv(name, model=env.sys.scaled(mass=1.3))
    rec = gpu_record(H, env.action_size)
    env, plan, st = _plan(name, N, H, rec, seed=5)
    key, dkey = gpu.prng_key(6), gpu.prng_key(11)
    plan.set_mpc_plant(env=plant, key=dkey, act_std=0.3)
    ep = plan.run_mpc(key, T, K, E)
    ref = oc.episode(_oenv(orc, env), rec, _state(st), key, N, H, ND, 0.1, T, K, E, plant=_oenv(orc, plant), dkey=dkey, act_std=0.3,
                     impl=_impl())
    _equal(ep, ref, "plant")
    assert not np.array_equal(ref["actions"][:E], ref["means"][0][:E])
    plan.close()


@pytest.mark.parametrize("D", [0, 1])
def test_session_is_the_episode_and_reset_mean_keeps_prev(gpu, orc, D):
    name, N, H, E = "hopper", 70, 7, 2
    env = _env(name)
    rec = gpu_record(H, env.action_size)
    env, plan, st = _plan(name, N, H, rec, seed=5)
    if D:
        plan.set_mpc_delay(D)
    key = gpu.prng_key(6)
    ep = plan.run_mpc(key, T, K, E)
    with plan.mpc_open(key, K, E) as s:
        means = np.stack([s.tick(ep["states"][t])["mean"] for t in range(T)])
    same_bits(means, ep["means"], f"D={D}: a session fed the episode's states")
    # reset_mean in front of tick 2: a cold tick whose previous action is still clip(M_1[E-1]) (the checker's reset_at)
    ref = oc.episode(_oenv(orc, env), rec, _state(st), key, N, H, ND, 0.1, T, K, E, D=D, reset_at=(2,), impl=_impl())
    with plan.mpc_open(key, K, E) as s:
        got = []
        for t in range(T):
            if t == 2:
                s.reset_mean()
            got.append(s.tick(ref["states"][t])["mean"])
    same_bits(np.stack(got), ref["means"], f"D={D}: reset_mean keeps prev")
    assert not np.array_equal(ref["means"][2], ep["means"][2])
    same_bits(plan.run_mpc(key, T, K, E)["means"], ep["means"], "an episode after the sessions")
    plan.close()


# ---- composition ----------------------------------------------------------------------------------------------------------------
def test_the_cost_is_taken_on_the_shaped_candidates(gpu, orc):
    """A noise shape (always) and a noise basis (warm ticks) together, humanoidrun (lazy normals): the checker's ObjectiveEnv sees
    the candidates its shaped sampler made."""
    name, N, H, E = "humanoidrun", 40, 5, 1
    env = _env(name)
    Nu = env.action_size
    rec = gpu_record(H, Nu)
    env, plan, st = _plan(name, N, H, rec, seed=5)
    g = (0.5 + np.arange(H * Nu, dtype=np.float64) / (H * Nu)).astype(np.float32).reshape(H, Nu)
    g[H // 2] = 0.0
    W = nbc.basis_of(H, 3)
    plan.set_noise_shape(g, "always")
    plan.set_noise_basis(W, "warm")
    key = gpu.prng_key(6)
    ep = plan.run_mpc(key, T, K, E)
    oenv = _oenv(orc, env)

    ref = nbc.episode(lambda e, *a, **kw: _episode_on(e, rec, *a, **kw), oenv, W, "warm", ND, _state(st), key, N, H, ND, 0.1, T, K, E,
                      shape=g, shape_when="always")
    _equal(ep, ref, "shape + basis")
    flat = oc.episode(oenv, rec, _state(st), key, N, H, ND, 0.1, T, K, E, impl=_impl())
    assert not np.array_equal(flat["means"], ref["means"])
    plan.close()


def _episode_on(env_like, rec, *a, **kw):
    """oc.episode on an env another checker has wrapped (its ``orc`` samples under a shape or a basis)."""
    e = oc.ObjectiveEnv(env_like, rec)
    return oc.episode(env_like, rec, *a, env=e, prev=e.prev, impl=_impl(), **kw)


def test_demo_plan_blends_on_the_shaped_rewards(gpu, orc_omp):
    """humanoidtrack with demos: the log-densities are untouched and the blend runs on ret - cost (a whole plan; H = 50)."""
    from mbd_hip.planners.mbd_planner import Plan
    orc = orc_omp
    name, N, H, Nd = "humanoidtrack", 33, 50, 4
    env = _env(name)
    rec = gpu_record(H, env.action_size)
    rec.row_weight = oc.f32(0.96) ** np.arange(H, dtype=np.float32)
    plan = Plan(env, _args(name, N, H, Nd, enable_demo=True))
    st, key = env.reset(gpu.prng_key(3)), gpu.prng_key(4)
    plan.set_state0(st)
    base = plan.run(key)[0]
    plan.set_objective(**rec.kwargs())
    mu, rm, rf, _ = plan.run(key)
    want = oc.plan(orc, _oenv(orc, env), rec, _state(st), key, N, H, Nd, 0.1, _impl(), enable_demo=True)
    same_bits(mu, want["mu_0ts"], "demo plan: means")
    same_bits(rm, want["rew_means"], "demo plan: mean rewards")
    _same_last(plan, want["last"], "demo plan")
    assert not np.array_equal(mu, base)
    plan.close()


def test_demo_episode_blends_on_the_shaped_rewards(gpu, orc_omp):
    """A humanoidtrack demo EPISODE (T = 3, K = 2, E = 2, the synthetic clip of tests/mpc_demo_checker.py from row 2): every tick
    plans under its own window of the clip — the demo record's d_xref —, the log-densities are untouched, the blend runs on the
    shaped rewards, and the previous action moves from tick to tick.  As a plan and as episode 0 and 1 of a sweep."""
    import mpc_demo_checker as mdc
    from mbd_hip.planners.mbd_planner import Plan, Sweep
    orc = orc_omp
    name, N, H, Nd, E, c0, rew_xref = "humanoidtrack", 33, 50, 4, 2, 2, 1.0
    env = _env(name)
    oenv = _oenv(orc, env)
    clip = mdc.extended(oenv.xref)
    rec = gpu_record(H, env.action_size)
    rec.row_weight = oc.f32(0.96) ** np.arange(H, dtype=np.float32)
    a = _args(name, N, H, Nd, enable_demo=True)
    sts = [env.reset(gpu.prng_key(5 + k)) for k in range(2)]
    keys = np.array([gpu.prng_key(6), gpu.prng_key(16)], np.uint32)
    plan = Plan(env, a)
    plan.set_state0(sts[0])
    plan.set_mpc_demo(clip, c0, rew_xref)
    base = plan.run_mpc(keys[0], T, K, E)
    plan.set_objective(**rec.kwargs())
    ep = plan.run_mpc(keys[0], T, K, E)
    ref = oc.demo_episode(oenv, rec, clip, c0, rew_xref, _state(sts[0]), keys[0], N, H, Nd, 0.1, T, K, E, impl=_impl())
    _equal(ep, ref, "demo episode")
    _same_last(plan, ref["last"], "demo episode")
    assert np.isfinite(ref["means"]).all() and not np.array_equal(ep["means"], base["means"])
    same_bits(ep["demo_windows"], mdc.windows(clip, c0, T, E), "the windows are the clock's")
    plan.set_state0(sts[1])
    ep1 = plan.run_mpc(keys[1], T, K, E)
    plan.close()
    sw = Sweep(env, a, 2)
    for k in range(2):
        sw.set_state0(k, sts[k])
    sw.set_mpc_demo(clip, c0, rew_xref)
    sw.set_objective(**rec.kwargs())
    got = sw.run_mpc(keys, T, K, E)
    sw.close()
    for k, one in enumerate((ep, ep1)):
        _equal({f: got[f][k] for f in _LOGS}, one, f"sweep demo episode {k}")


@pytest.mark.parametrize("N,risk", [(64, "mean"), (64, "min"), (40, "mean"), (40, "min")])
def test_ensemble_members_are_shaped_then_combined(gpu, orc, N, risk):
    """M = 2 on hopper: N = 64 is one rollout launch over M N rows, N = 40 M launches; the objective runs over the M N rows with
    the candidate b % N, and ensemble_reduce_kernel combines the shaped returns."""
    from mbd_hip.envs.base import RigidBodyEnv
    name, H, E = "hopper", 7, 1
    env = _env(name)
    member = RigidBodyEnv(name, model=env.sys.scaled(mass=1.3, gear=0.8))
    rec = gpu_record(H, env.action_size)
    env, plan, st = _plan(name, N, H, rec, seed=5)
    plan.set_ensemble([None, member], risk)
    key = gpu.prng_key(6)
    ep = plan.run_mpc(key, T, K, E)
    ret, cost = plan.peek_objective()
    rm, comb = plan.peek_ensemble()
    oenv, omember = _oenv(orc, env), _oenv(orc, member)
    prev = oc.Prev(rec.prev0)
    members = [oc.ObjectiveEnv(oenv, rec, prev), oc.ObjectiveEnv(omember, rec, prev)]
    ee = ensemble_checker.EnsembleEnv(oenv, members, risk)
    ref = oc.episode(oenv, rec, _state(st), key, N, H, ND, 0.1, T, K, E, env=ee, prev=prev, impl=_impl())
    _equal(ep, ref, f"ensemble N={N} {risk}")
    assert ret.shape == (2, N)
    for m in range(2):
        same_bits(ret[m], members[m].last[1], f"member {m}: ret")
        same_bits(rm[m], members[m].last[0], f"member {m}: the shaped return the combination reads")
    same_bits(cost, members[0].last[2], "cost")
    same_bits(comb, ensemble_checker.combine(np.stack([members[0].last[0], members[1].last[0]]), risk), "combined")
    plan.close()


@pytest.mark.parametrize("um", [0, 1], ids=["mbd", "mppi"])
def test_sweep_is_the_single_plans(gpu, um):
    """P = 2 on hopper: mbd_sweep_run, mbd_sweep_run_mpc (with a delay record: the queue's last row is the first prev) and, for MBD
    sweeps, the sweep's session equal the single plans under the same record; peek_objective per plan."""
    from mbd_hip.planners import path_integral
    from mbd_hip.planners.mbd_planner import Plan, Sweep
    name, N, H, E, P = "hopper", 70, 7, 2, 2
    env = _env(name)
    rec = gpu_record(H, env.action_size)
    a = _args(name, N, H) if um == 0 else path_integral.Args(env_name=name, Nsample=N, Hsample=H, Nrefine=ND, temp_sample=0.1,
                                                              disable_recommended_params=True)
    keys = np.array([gpu.prng_key(60 + k) for k in range(P)], np.uint32)
    states = [env.reset(gpu.prng_key(k)) for k in range(P)]
    rows0 = (np.random.default_rng(2).normal(size=(E, env.action_size)) * 0.5).astype(np.float32)
    sw = Sweep(env, a, P, update_method=um)
    for k in range(P):
        sw.set_state0(k, states[k])
    flat = sw.run(keys)[0]
    sw.set_objective(**rec.kwargs())
    if um:
        sw.set_mpc_sigma(1.0, 0.5, 0.0)
    mu = sw.run(keys)[0]
    peeks = [sw.peek_objective(k) for k in range(P)]
    ep = sw.run_mpc(keys, T, K, E)
    sw.set_mpc_delay(1, rows0)
    epd = sw.run_mpc(keys, T, K, E)
    sw.clear_mpc_delay()
    sess = None
    if um == 0:
        with sw.mpc_open(keys, K, E) as s:
            sess = np.stack([s.tick(ep["states"][:, t])["mean"] for t in range(T)], axis=1)
    sw.clear_objective()
    same_bits(sw.run(keys)[0], flat, "a cleared record")
    sw.close()
    assert not np.array_equal(mu, flat)
    for k in range(P):
        p = Plan(env, a, update_method=um)
        p.set_state0(states[k])
        p.set_objective(**rec.kwargs())
        if um:
            p.set_mpc_sigma(1.0, 0.5, 0.0)
        same_bits(mu[k], p.run(keys[k])[0], f"plan {k}: open loop")
        for got, want in zip(peeks[k], p.peek_objective()):
            same_bits(got, want, f"plan {k}: peek_objective")
        _equal({f: ep[f][k] for f in _LOGS}, p.run_mpc(keys[k], T, K, E), f"episode {k}")
        if sess is not None:
            same_bits(sess[k], ep["means"][k], f"session {k}")
        p.set_mpc_delay(1, rows0)
        _equal({f: epd[f][k] for f in _LOGS}, p.run_mpc(keys[k], T, K, E), f"delayed episode {k}")
        p.close()


def test_two_unequal_shards_give_the_unsharded_rewards(gpu):
    """humanoidrun (lazy normals) and car2d (materialised candidates) — both forms take the shard's row offset —: shards [0, 27)
    and [27, N) through the phase calls in one process against the unsharded plan's rewards, and their peeks against its."""
    import torch
    from mbd_hip.planners.mbd_planner import Plan
    for name, N, H in (("humanoidrun", 40, 5), ("car2d", 33, 6)):
        env = _env(name)
        Nu = env.action_size
        rec = gpu_record(H, Nu)
        st = env.reset(gpu.prng_key(3))
        i = ND - 2
        Ybar = (np.random.default_rng(1).normal(size=(H, Nu)) * 0.3).astype(np.float32)
        d_Y = torch.tensor(Ybar.reshape(-1), device="cuda")
        key = gpu.key_array(gpu.prng_key(12))
        out = {}
        for tag, (b, c) in (("all", (0, N)), ("lo", (0, 27)), ("hi", (27, N - 27))):
            plan = Plan(env, _args(name, N, H), shard_begin=b, shard_count=c)
            plan.set_state0(st)
            plan.set_objective(**rec.kwargs())
            d_r = torch.full((c,), float("nan"), device="cuda")
            gpu.check(plan.lib.mbd_plan_sample_rollout(plan.h, i, key, d_Y.data_ptr(), d_r.data_ptr(), None, None))
            torch.cuda.synchronize()
            out[tag] = (d_r.cpu().numpy(),) + plan.peek_objective()
            plan.close()
        for j, what in enumerate(("rews", "ret", "cost")):
            same_bits(np.concatenate([out["lo"][j], out["hi"][j]]), out["all"][j], f"{name}: {what}")
        assert np.isfinite(out["all"][0]).all()


# ---- containment ----------------------------------------------------------------------------------------------------------------
def test_a_diverged_member_stays_in_its_rows(gpu, orc):
    """tests/containment_inputs.py's poisoned model (one actuator's gear at 1e30) as member 1 of an ensemble of halfcheetah, N = 33:
    every row of member 1 diverges, and row 32 of member 0 shares a wavefront of the objective launch with row 0 of member 1.  The
    healthy rows keep the checker's bits — ret, cost and the rewards the combination reads —, the diverged rows are not finite."""
    import torch
    from mbd_hip.envs.base import RigidBodyEnv
    name, N, H = "halfcheetah", 33, ci.H
    m = ci.model(name)[0]
    env = RigidBodyEnv(name, model=m)
    bad = RigidBodyEnv(name, model=ci.poison_model(m))
    from mbd_hip.planners.mbd_planner import Plan
    rec = gpu_record(H, env.action_size)
    plan = Plan(env, _args(name, N, H))
    st = env.reset(gpu.prng_key(3))
    plan.set_state0(st)
    plan.set_objective(**rec.kwargs())
    plan.set_ensemble([None, bad], "mean")
    i = ND - 2
    Ybar = np.full((H, env.action_size), 0.2, np.float32)
    d_Y, d_rm = torch.tensor(Ybar.reshape(-1), device="cuda"), torch.zeros(1, device="cuda")
    gpu.check(plan.lib.mbd_plan_reverse_once(plan.h, i, gpu.key_array(gpu.prng_key(5)), d_Y.data_ptr(), d_rm.data_ptr(), None))
    torch.cuda.synchronize()
    Y0s, rewss0, _ = plan.peek()
    ret, cost = plan.peek_objective()
    members, comb = plan.peek_ensemble()
    plan.close()
    assert np.isfinite(rewss0).all()
    want = oc.step(rewss0, op.mean_h(orc, rewss0), Y0s, rec, oc.clip(rec.prev0))
    same_bits(ret[0], want[1], "healthy rows: ret")
    same_bits(cost, want[2], "cost")
    same_bits(members[0], want[0], "healthy rows: rews")
    assert not np.isfinite(ret[1]).any() and not np.isfinite(members[1]).any() and not np.isfinite(comb).any()


def test_a_diverged_plan_of_a_sweep_stays_alone(gpu):
    """containment_inputs.SWEEPS' first case (halfcheetah, N = 33: plans share wavefronts) with plan 1 started from the poisoned
    state, under a record with both costs: plans 0 and 2 keep the single plan's bits, plan 1's mean rewards are not finite."""
    from mbd_hip.envs import get_env
    from mbd_hip.planners.mbd_planner import Args, Plan, Sweep
    name, kernel, N, _ = ci.SWEEPS[0]
    env = get_env(name)
    H, P = ci.SWEEP_H, ci.SWEEP_P
    a = Args(env_name=name, Nsample=N, Hsample=H, Ndiffuse=ci.SWEEP_ND, temp_sample=0.1, disable_recommended_params=True, not_render=True)
    rec = gpu_record(H, env.action_size)
    from mbd_hip.envs.base import State
    sts = [env.reset(gpu.prng_key(20 + k)) for k in range(P)]
    s = np.asarray(sts[1].pipeline_state, np.float32)
    sts[1] = State(ci.poison_state(s.reshape(-1, 13)).reshape(s.shape), None, np.float32(0), np.float32(0), {})
    keys = np.stack([gpu.prng_key(40 + k) for k in range(P)])
    sw = Sweep(env, a, P)
    for k in range(P):
        sw.set_state0(k, sts[k])
    sw.set_objective(**rec.kwargs())
    mu, rm, rf, _ = sw.run(keys)
    sw.close()
    assert not np.isfinite(rm[1]).any()
    for k in (0, 2):
        p = Plan(env, a)
        p.set_state0(sts[k])
        p.set_objective(**rec.kwargs())
        mu1, rm1, _, _ = p.run(keys[k])
        p.close()
        assert np.isfinite(mu1).all() and np.isfinite(rm1).all()
        same_bits(mu[k], mu1, f"plan {k}: means")
        same_bits(rm[k], rm1, f"plan {k}: mean rewards")


# ---- the command line -----------------------------------------------------------------------------------------------------------
def test_command_line(gpu, orc, tmp_path):
    """python -m mbd_hip.planners.mpc --discount --rate_cost at the small hopper size: its episode's means are the checker's."""
    from mbd_hip.planners.mpc import action_rate, discount_weights
    name, N, H, E = "hopper", 70, 7, 1
    cmd = [sys.executable, "-m", "mbd_hip.planners.mpc", "--env_name", name, "--Nsample", str(N), "--Hsample", str(H), "--Ndiffuse", str(ND),
           "--temp_sample", "0.1", "--disable_recommended_params", "--n_ticks", str(T), "--warm_steps", str(K), "--exec_steps", str(E),
           "--seed", "2", "--discount", "0.9", "--rate_cost", "0.25"]
    envv = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "model-based-diffusion_amd")]))
    res = subprocess.run(cmd, cwd=tmp_path, env=envv, check=True, capture_output=True, text=True, timeout=300)
    line = json.loads(res.stdout.strip().splitlines()[-1])
    saved = np.load(tmp_path / "results" / name / "mpc_episode.npz")
    assert (line["discount"], line["rate_cost"], line["effort_cost"]) == (0.9, 0.25, 0.0)
    assert line["action_rate"] == pytest.approx(action_rate(saved["actions"]))
    from mbd_hip.planners.mpc import _reset_and_key
    env = _env(name)
    st, key = _reset_and_key(env, 2)
    rec = oc.Record(row_weight=discount_weights(H, 0.9), rate=0.25)
    ref = oc.episode(_oenv(orc, env), rec, _state(st), key, N, H, ND, 0.1, T, K, E, impl=_impl())
    same_bits(saved["means"], ref["means"], "the command line's means")
    same_bits(saved["rewards"], ref["rewards"], "the command line's rewards are the env's own")


def test_c_caller_sets_a_rate_cost(gpu, tmp_path):
    """examples/mbd_control.c --rate_cost from plain C: the rewards of its ticks are those of the Python episode under the same
    record — rate cost 0.5, prev0 zeros (the actuators at rest), seed 0's reset and key — and differ from the run without it."""
    libdir = os.path.join(ROOT, "model-based-diffusion_amd", "lib")
    exe = str(tmp_path / "mbd_control")
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "mbd_control.c"),
                    "-o", exe, "-L", libdir, "-lmbd_hip", f"-Wl,-rpath,{libdir}", "-lm"], check=True)
    name, N, H, Tc = "hopper", 64, 7, 5

    def rewards(*extra):
        out = subprocess.run([exe, name, str(N), str(H), str(ND), str(K), str(Tc), "0", *extra], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        return [np.float32(float(ln.split()[3])) for ln in out.stdout.strip().splitlines() if ln.startswith("tick ")]

    got, plain = rewards("--rate_cost", "0.5"), rewards()
    from mbd_hip.planners.mbd_planner import Plan
    env = _env(name)
    rng_episode, rng_reset = gpu.prng_split(gpu.prng_key(0), 2, 1)
    plan = Plan(env, _args(name, N, H))
    plan.set_state0(env.reset(rng_reset))
    plan.set_objective(rate=0.5, prev0=np.zeros(env.action_size, np.float32))
    ep = plan.run_mpc(rng_episode, Tc, K, 1)
    plan.close()
    assert got == [np.float32(r) for r in ep["rewards"]] and got != plain
