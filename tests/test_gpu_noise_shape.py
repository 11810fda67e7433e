"""-m gpu: noise shapes (include/mbd_hip.h mbd_noise_shape; DESIGN.md section 1 "N7 noise shape") against the checker's
restatement, tests/noise_shape_checker.py.  Every comparison is by bit pattern or np.array_equal.

  every sampler form   the small cases of tests/sampler_inputs.py — whole tensor, three ranges, one range, noise_kernel + shift,
                       the noise workgroups of a rollout launch and their second-stream form — in both threefry layouts, through
                       the entry points of tests/test_gpu_sampler.py, under a shape with a distinct value per (h, a), one zero
                       row and values above 1: peek()[0], element by element; the sweeps' batched kernels at the sizes of
                       sampler_inputs.SWEEPS against the plans run alone under the same shape; the two index widths of the
                       shaped loops on their own
  all ones             no shape at all: whole plans and whole episodes, both modes
  whole plans          hopper (planar family), humanoidrun (3-D), car2d, an mppi and a cma-es plan, with the last step's Y0s
  episodes             both modes, E = 1 and 2: tick 0, prefixes, and all four logs against the checker
  plant, ensemble      the disturbance normals stay unshaped; the M N launch's noise workgroups carry the shape
  sweep                P = 2 episodes = two single-plan episodes
  stale prefetch       a set call between two steps discards the normals prepared ahead; so does a clear
"""
import functools
from dataclasses import replace

import numpy as np
import pytest

import ensemble_checker
import mpc_checker
import mpc_plant_checker
import noise_shape_checker as nsc
import sampler_inputs as sx
from oracle import planner as op
from state_inputs import same_bits
from test_gpu_sampler import KEY_SEED, _Sampler

pytestmark = pytest.mark.gpu

_LOGS = ("means", "actions", "rewards", "states")


@pytest.fixture(scope="module")
def gpu(lib):
    from mbd_hip import _capi
    if _capi.device_count() < 1:
        pytest.fail("tests/test_gpu_noise_shape.py needs a GPU")
    return _capi


@functools.lru_cache(maxsize=None)
def _env(name):
    from mbd_hip.envs import get_env
    return get_env(name)


def _oenv(orc, env):
    if env.__class__.__name__ == "Car2d":
        return op.OracleEnv(orc, "car2d", xref=env.xref, rew_xref=env.rew_xref)
    return op.OracleEnv(orc, env.env_name, env.sys.to_struct(), xref=env.xref, rew_xref=env.rew_xref, init_q=env.sys.init_q)


def shape_of(H, Nu):
    """A distinct value per (h, a) in [0.5, 1.5) — above and below 1 — and, from two rows on, one row of zeros."""
    g = (0.5 + np.arange(H * Nu, dtype=np.float64) / (H * Nu)).astype(np.float32).reshape(H, Nu)
    if H >= 2:
        g[H // 2] = 0.0
    else:
        g[0, 0] = 1.75
    assert np.unique(g[g > 0]).size == (g > 0).sum() and (g > 1).any()
    return g


def _args(name, N, H, Nd, **kw):
    from mbd_hip.planners.mpc import MpcArgs
    return MpcArgs(env_name=name, Nsample=N, Hsample=H, Ndiffuse=Nd, temp_sample=0.1, disable_recommended_params=True,
                   not_render=True, **kw)


def _state(env, st):
    return np.asarray(st.pipeline_state, np.float32).reshape(-1)


def _equal(a, b, what=""):
    for k in _LOGS:
        x, y = np.asarray(a[k], np.float32), np.asarray(b[k], np.float32)
        assert x.size == y.size and np.array_equal(x.reshape(y.shape), y), f"{what}: {k} differ"


# ---- every sampler form ---------------------------------------------------------------------------------------------------

def _compare(s, orc, g, key, sigma, Ybar, what):
    c = s.c
    s.torch.cuda.synchronize()
    Y0s = s.plan.peek()[0]
    ref = nsc.ShapedOracle(orc, g).sample(key, c.layout, c.N, c.H, s.Nu, 0, c.N, float(sigma), Ybar.reshape(c.H, s.Nu))
    same_bits(Y0s, ref, what)
    if c.H >= 2:  # the zero row is frozen at the clipped mean
        row = np.clip(Ybar.reshape(c.H, s.Nu)[c.H // 2], np.float32(-1), np.float32(1))
        assert np.array_equal(Y0s[:, c.H // 2, :], np.broadcast_to(row, (c.N, s.Nu))), what
    if c.total > 4:
        flat = orc.sample(key, c.layout, c.N, c.H, s.Nu, 0, c.N, float(sigma), Ybar.reshape(c.H, s.Nu))
        assert not np.array_equal(Y0s, flat), f"{what}: the shape changed nothing"


_STEP = [c for c in sx.cases(large=False) if c.form != "fused"]
_FUSED = sx.cases("fused")


@pytest.mark.parametrize("c", _STEP, ids=[c.id for c in _STEP])
def test_sampler_forms_under_a_shape(gpu, orc, c, monkeypatch, levers):
    """sample_kernel in its whole-tensor form and both range forms (sigma from the host and from the device), noise_kernel +
    shift_kernel: one step in the plain setting and one in the saturating setting of tests/test_gpu_sampler.py."""
    s = _Sampler(gpu, orc, c, monkeypatch, levers)
    try:
        g = shape_of(c.H, s.Nu)
        s.plan.set_noise_shape(g)
        key = gpu.prng_key(KEY_SEED + c.N)
        for saturating in (False, True):
            i, sigma = s.sigma(saturating)
            Ybar = s.ybar(saturating, seed=c.N)
            s.sample_rollout(i, key, Ybar)
            _compare(s, orc, g, key, sigma, Ybar, f"{c.id} {'saturating' if saturating else 'plain'}")
            key = gpu.prng_key(KEY_SEED + c.N + 7)
    finally:
        s.close()


@pytest.mark.parametrize("c", _FUSED, ids=[c.id for c in _FUSED])
def test_prefetched_normals_under_a_shape(gpu, orc, c, monkeypatch, levers):
    """The next step's normals generated beside the rollout — by the launch's noise workgroups, plain and XCD-pinned, or by
    noise_kernel on the second stream — carry the shape: key B is declared, a step runs with key A, the step after it asks for
    key B and its candidates are the checker's, every element."""
    s = _Sampler(gpu, orc, c, monkeypatch, levers)
    try:
        g = shape_of(c.H, s.Nu)
        s.plan.set_noise_shape(g)
        i = sx.I_LARGE
        A, B = gpu.prng_key(KEY_SEED + c.N + 3), gpu.prng_key(KEY_SEED + c.N + 4)
        s.prefetch(B)
        d_Y = s.sample_rollout(i, A, s.ybar(True, seed=3))
        s.score_update(i, A, d_Y)
        Ybar = s.ybar(True, seed=4)
        s.sample_rollout(i - 1, B, Ybar)
        _compare(s, orc, g, B, np.float32(s.sched[2][i - 1]), Ybar, c.id)
    finally:
        s.close()


@pytest.mark.parametrize("layout", sx.LAYOUTS, ids=["legacy", "part"])
@pytest.mark.parametrize("name,N,H,steps,kind", sx.SWEEPS, ids=[f"{s[4]}-{s[0]}-N{s[1]}" for s in sx.SWEEPS])
def test_batched_samplers_under_a_shape(gpu, name, N, H, steps, kind, layout, monkeypatch):
    """noise_batch_kernel (MBD sweeps) and sample_batch_kernel (path-integral sweeps) above their grid cap — the shaped loops
    stride — as ONE sweep under a shape against the same plans run alone under it (whose launches are held to the checker above)."""
    monkeypatch.setenv("MBD_THREEFRY_PARTITIONABLE", str(layout))
    from mbd_hip.planners import path_integral
    from mbd_hip.planners.mbd_planner import Args, Plan, Sweep
    env, P = _env(name), 2
    if kind == "mbd":
        um, args = 0, Args(env_name=name, Nsample=N, Hsample=H, Ndiffuse=steps + 1, temp_sample=0.1, disable_recommended_params=True,
                           not_render=True)
    else:
        um, args = 1, path_integral.Args(env_name=name, Nsample=N, Hsample=H, Nrefine=steps + 1, temp_sample=0.1,
                                         disable_recommended_params=True)
    g = shape_of(H, env.action_size)
    keys = np.array([gpu.prng_key(50 + k) for k in range(P)], np.uint32)
    states = [env.reset(gpu.prng_key(k)) for k in range(P)]
    sw = Sweep(env, args, P, update_method=um)
    for k in range(P):
        sw.set_state0(k, states[k])
    flat = sw.run(keys)[0]
    sw.set_noise_shape(g)
    mu, rm, rf, _ = sw.run(keys)
    sw.clear_noise_shape()
    again = sw.run(keys)[0]
    sw.close()
    assert np.isfinite(mu).all() and not np.array_equal(mu, flat) and np.array_equal(again, flat)
    for k in range(P):
        p = Plan(env, args, update_method=um)
        p.set_state0(states[k])
        p.set_noise_shape(g)
        mu1, rm1, rf1, _ = p.run(keys[k])
        p.close()
        same_bits(mu[k], mu1, f"{name} {kind} plan {k}: means")
        same_bits(rm[k], rm1, f"{name} {kind} plan {k}: mean rewards")
        same_bits(np.float32(rf[k]), np.float32(rf1), f"{name} {kind} plan {k}: final reward")


@pytest.mark.parametrize("layout", sx.LAYOUTS, ids=["legacy", "part"])
@pytest.mark.parametrize("wide", [False, True], ids=["idx32", "idx64"])
@pytest.mark.parametrize("N,HNu,blocks", [(1, 1, 1), (3, 1, 1), (37, 7, 1), (101, 33, 3), (257, 1, 1), (64, 170, 5), (513, 3, 2)])
def test_shaped_loops_in_both_index_widths(gpu, orc, N, HNu, blocks, wide, layout):
    """noise_fill's shaped loops on their own: the residue that advances by stride mod HNu instead of a division per element,
    with the 32-bit indices the library takes below 2^32 elements and the 64-bit ones it takes beyond — rows coprime to the
    stride, odd totals whose `half` falls inside a row, fewer threads than thread-items (the loops wrap), HNu above and below
    the stride's residue.  z = eps * g against the checker's, every element."""
    g = shape_of(1, HNu).reshape(-1) if HNu < 2 else shape_of(HNu, 1).reshape(-1)
    key = gpu.prng_key(900 + N)
    z = gpu.debug_noise_shaped(key, layout, N, HNu, g, wide, blocks)
    _, want = nsc.ShapedOracle(orc, g.reshape(HNu, 1)).sample(key, layout, N, HNu, 1, 0, N, 1.0, np.zeros((HNu, 1), np.float32),
                                                             want_eps=True)
    same_bits(z, want.reshape(N, HNu), f"N={N} HNu={HNu} blocks={blocks} wide={wide}")


# ---- all ones ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["hopper", "humanoidrun"])
def test_all_ones_is_no_shape(gpu, name):
    from mbd_hip.planners.mbd_planner import Plan
    env = _env(name)
    a = _args(name, 128, 6, 6)
    plan = Plan(env, a)
    plan.set_state0(env.reset(gpu.prng_key(7)))
    key = gpu.prng_key(8)
    ref_run, ref_ep = plan.run(key), plan.run_mpc(key, 3, 2, 1)
    ones = np.ones((6, env.action_size), np.float32)
    for when in ("always", "warm"):
        plan.set_noise_shape(ones, when)
        got = plan.run(key)
        for x, y in zip(got[:3], ref_run[:3]):
            assert np.array_equal(np.asarray(x, np.float32), np.asarray(y, np.float32)), (name, when)
        _equal(plan.run_mpc(key, 3, 2, 1), ref_ep, f"{name} {when}")
    plan.set_noise_shape(shape_of(6, env.action_size))
    assert not np.array_equal(plan.run(key)[0], ref_run[0])
    plan.clear_noise_shape()
    assert np.array_equal(plan.run(key)[0], ref_run[0])
    plan.close()


# ---- whole plans ---------------------------------------------------------------------------------------------------------

def _checker_plan(orc, oenv, g, s0, key, N, H, Nd, temp, impl):
    sched = orc.schedule(1e-4, 1e-2, Nd)
    r, Ybar = np.asarray(key, np.uint32), np.zeros((H, oenv.Nu), np.float32)
    mus, rms, det = [], [], None
    for i in range(Nd - 1, 0, -1):
        r, Ybar, rm, det = nsc.reverse_once(orc, oenv, g, s0, i, r, Ybar, sched, N, H, temp, impl)
        mus.append(Ybar)
        rms.append(rm)
    rew_final = op.mean_h(orc, np.ascontiguousarray(oenv.rollout(s0, Ybar[None])))[0]
    return np.stack(mus), np.array(rms, np.float32), rew_final, det


@pytest.mark.parametrize("name,N,H", [("hopper", 96, 6), ("humanoidrun", 128, 5), ("car2d", 100, 6)])
def test_whole_plan_matches_the_checker(gpu, orc, name, N, H):
    from mbd_hip.envs.base import prng_impl
    from mbd_hip.planners.mbd_planner import Plan
    env, Nd = _env(name), 6
    a = _args(name, N, H, Nd)
    st, key = env.reset(gpu.prng_key(3)), gpu.prng_key(4)
    g = shape_of(H, env.action_size)
    plan = Plan(env, a)
    plan.set_state0(st)
    plan.set_noise_shape(g)
    mu, rm, rf, _ = plan.run(key)
    Y0s, rewss, w = plan.peek()
    plan.close()
    want = _checker_plan(orc, _oenv(orc, env), g, _state(env, st), key, N, H, Nd, 0.1, prng_impl())
    same_bits(mu, want[0], f"{name}: means")
    same_bits(rm, want[1], f"{name}: mean rewards")
    same_bits(np.float32(rf), np.float32(want[2]), f"{name}: final reward")
    same_bits(Y0s, want[3]["Y0s"], f"{name}: the last step's candidates")
    same_bits(w, want[3]["weights"], f"{name}: the last step's weights")


@pytest.mark.parametrize("method", ["mppi", "cma-es"])
def test_path_integral_plan_matches_the_checker(gpu, orc, method):
    from mbd_hip.envs.base import prng_impl
    from mbd_hip.planners import path_integral
    from mbd_hip.planners.mbd_planner import Plan
    name, N, H, Nr = "hopper", 96, 6, 5
    env = _env(name)
    oenv, impl = _oenv(orc, env), prng_impl()
    args = path_integral.Args(env_name=name, Nsample=N, Hsample=H, Nrefine=Nr, temp_sample=0.1, disable_recommended_params=True)
    st, key = env.reset(gpu.prng_key(3)), gpu.prng_key(4)
    g = shape_of(H, env.action_size)
    plan = Plan(env, args, update_method=op.PI_METHODS[method])
    plan.set_state0(st)
    plan.set_noise_shape(g)
    mu_gpu, rm_gpu, _, _ = plan.run(key)
    Y0s_gpu = plan.peek()[0]
    sigma_gpu = plan.get_sigma()
    plan.close()
    so, s0 = nsc.ShapedOracle(orc, g), _state(env, st)
    r, mu, sigma = np.asarray(key, np.uint32), np.zeros((H, env.action_size), np.float32), np.float32(1.0)
    for t in range(Nr - 1, 0, -1):
        keys = orc.split(r, 2, impl)
        r, ks = keys[0], keys[1]
        Y0s = so.sample(ks, impl, N, H, env.action_size, 0, N, float(sigma), mu)
        rews = op.mean_h(orc, np.ascontiguousarray(oenv.rollout(s0, Y0s)))
        mu, sigma, _, rm = orc.pi_update(op.PI_METHODS[method], rews, Y0s, mu, float(sigma), 0.1)
        same_bits(mu_gpu[Nr - 1 - t], mu, f"{method}: mean of step {t}")
        same_bits(np.float32(rm_gpu[Nr - 1 - t]), np.float32(rm), f"{method}: mean reward of step {t}")
    same_bits(Y0s_gpu, Y0s, f"{method}: the last step's candidates")
    same_bits(np.float32(sigma_gpu), np.float32(sigma), f"{method}: sigma")


# ---- episodes ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,N,H", [("hopper", 64, 6), ("humanoidrun", 128, 5), ("car2d", 64, 6)])
@pytest.mark.parametrize("E", [1, 2])
@pytest.mark.parametrize("when", ["always", "warm"])
def test_episode_matches_the_checker(gpu, orc, name, N, H, E, when):
    """T = 3, K = 2.  The warm mode's tick 0 is mbd_plan_run(k_0); in both modes T = 2 is a prefix of T = 3 and means,
    actions, rewards and states equal the checker episode's."""
    from mbd_hip.envs.base import prng_impl
    from mbd_hip.planners.mbd_planner import Plan
    env, Nd, T, K = _env(name), 6, 3, 2
    a = _args(name, N, H, Nd)
    st, key = env.reset(gpu.prng_key(5)), gpu.prng_key(6)
    g = shape_of(H, env.action_size)
    plan = Plan(env, a)
    plan.set_state0(st)
    k0 = gpu.prng_split(key, 2, plan.cfg.prng_impl)[1]
    flat_mu0 = plan.run(k0)[0]
    plan.set_noise_shape(g, when)
    ep = plan.run_mpc(key, T, K, E)
    short = plan.run_mpc(key, T - 1, K, E)
    mu0 = plan.run(k0)[0]
    plan.close()
    for k in _LOGS:
        assert np.array_equal(short[k], ep[k][: len(short[k])]), k
    assert np.array_equal(ep["means"][0], mu0[-1])
    assert np.array_equal(mu0, flat_mu0) == (when == "warm")
    ref = nsc.episode(mpc_checker.episode, _oenv(orc, env), g, when, Nd, _state(env, st), key, N, H, Nd, 0.1, T, K, E,
                      impl=prng_impl())
    _equal(ep, ref, f"{name} {when} E={E}")
    assert np.isfinite(ref["states"]).all()


def test_plant_disturbances_stay_unshaped(gpu, orc):
    """hopper with action noise and a kick every second tick, a heavier plant, and a warm-tick shape: the executed rows are
    M_t[0:E] + act_std * eps with the UNSHAPED normals of the disturbance chain — the checker's ``orc.normal``."""
    from mbd_hip.envs.base import RigidBodyEnv, prng_impl
    from mbd_hip.planners.mbd_planner import Plan
    name, N, H, Nd, T, K, E = "hopper", 64, 6, 6, 3, 2, 2
    env = _env(name)
    plant = RigidBodyEnv(name, model=env.sys.scaled(mass=1.3))
    st, key, dkey = env.reset(gpu.prng_key(5)), gpu.prng_key(6), gpu.prng_key(11)
    g = shape_of(H, env.action_size)
    g[:E] = 3.0  # (the executed rows' own shape: what a shaped disturbance would be scaled by)
    for when in ("always", "warm"):
        plan = Plan(env, _args(name, N, H, Nd))
        plan.set_state0(st)
        plan.set_mpc_plant(env=plant, key=dkey, act_std=0.3, kick_std=0.5, kick_every=2)
        plan.set_noise_shape(g, when)
        ep = plan.run_mpc(key, T, K, E)
        plan.close()
        ref = nsc.episode(mpc_plant_checker.episode, _oenv(orc, env), g, when, Nd, _state(env, st), key, N, H, Nd, 0.1, T, K, E,
                          plant=_oenv(orc, plant), dkey=dkey, act_std=0.3, kick_std=0.5, kick_every=2, impl=prng_impl())
        _equal(ep, ref, f"plant {when}")
        assert not np.array_equal(ref["actions"][:E], ref["means"][0][:E])


def test_ensemble_episode_matches_the_checker(gpu, orc):
    """M = 2: the rollout launch over M N candidates carries the next step's shaped normals; episodes in both modes."""
    from mbd_hip.envs.base import RigidBodyEnv
    from mbd_hip.planners.mbd_planner import Plan
    name, N, H, Nd, T, K, E = "hopper", 64, 6, 6, 3, 2, 1
    env = _env(name)
    member = RigidBodyEnv(name, model=env.sys.scaled(mass=1.3, gear=0.8))
    st, key = env.reset(gpu.prng_key(5)), gpu.prng_key(6)
    g = shape_of(H, env.action_size)
    oenv, omember = _oenv(orc, env), _oenv(orc, member)
    for when, risk in (("always", "mean"), ("warm", "min")):
        plan = Plan(env, _args(name, N, H, Nd))
        plan.set_state0(st)
        plan.set_ensemble([None, member], risk)
        plan.set_noise_shape(g, when)
        ep = plan.run_mpc(key, T, K, E)
        plan.close()
        ref = nsc.episode(lambda e, *a, **kw: ensemble_checker.episode(e, [None, omember], risk, *a, **kw), oenv, g, when, Nd,
                          _state(env, st), key, N, H, Nd, 0.1, T, K, E)
        _equal(ep, ref, f"ensemble {when} {risk}")


@pytest.mark.parametrize("when", ["always", "warm"])
def test_sweep_episode_is_the_single_plans(gpu, when):
    from mbd_hip.planners.mbd_planner import Plan, Sweep
    name, N, H, Nd, T, K, E, P = "hopper", 64, 6, 6, 3, 2, 2, 2
    env = _env(name)
    a = _args(name, N, H, Nd)
    g = shape_of(H, env.action_size)
    keys = np.array([gpu.prng_key(60 + k) for k in range(P)], np.uint32)
    states = [env.reset(gpu.prng_key(k)) for k in range(P)]
    sw = Sweep(env, a, P)
    for k in range(P):
        sw.set_state0(k, states[k])
    flat = sw.run_mpc(keys, T, K, E)
    sw.set_noise_shape(g, when)
    ep = sw.run_mpc(keys, T, K, E)
    mu = sw.run(keys)[0]
    sw.close()
    assert not np.array_equal(ep["means"], flat["means"])
    assert np.array_equal(ep["means"][:, 0], flat["means"][:, 0]) == (when == "warm")
    for k in range(P):
        p = Plan(env, a)
        p.set_state0(states[k])
        p.set_noise_shape(g, when)
        one = p.run_mpc(keys[k], T, K, E)
        mu1 = p.run(keys[k])[0]
        p.close()
        _equal({f: ep[f][k] for f in _LOGS}, one, f"episode {k} {when}")
        same_bits(mu[k], mu1, f"open loop, plan {k} {when}")


# ---- the set call --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,N,H", [("humanoidrun", 128, 5), ("hopper", 64, 6), ("humanoidrun", 4608, 4)])
def test_set_call_discards_normals_prepared_ahead(gpu, orc_omp, name, N, H):
    """mbd_plan_reverse_once declares the next step's key, whose normals are generated beside its rollout (in the launch's
    spare workgroups; N = 4608 fills the chip: on the second stream).  A set call between two steps: the second step equals
    the checker under the NEW setting; then a clear between the second and the third: the third is flat again."""
    import torch
    from mbd_hip.envs.base import prng_impl
    from mbd_hip.planners.mbd_planner import Plan
    orc = orc_omp
    env, Nd = _env(name), 6
    impl = prng_impl()
    plan = Plan(env, _args(name, N, H, Nd))
    st = env.reset(gpu.prng_key(9))
    plan.set_state0(st)
    g = shape_of(H, env.action_size)
    d_Y, d_rm = torch.zeros(H * env.action_size, device="cuda"), torch.zeros(1, device="cuda")
    key = (gpu.key_array(gpu.prng_key(10)))
    oenv, s0, sched = _oenv(orc, env), _state(env, st), orc.schedule(1e-4, 1e-2, Nd)
    r, Ybar = np.asarray(gpu.prng_key(10), np.uint32), np.zeros((H, env.action_size), np.float32)
    for i, setting in ((Nd - 1, None), (Nd - 2, g), (Nd - 3, None), (Nd - 4, g)):
        if i < Nd - 1:  # between two steps: the previous step prepared this step's normals under the previous setting
            if setting is None:
                plan.clear_noise_shape()
            else:
                plan.set_noise_shape(setting)
        gpu.check(plan.lib.mbd_plan_reverse_once(plan.h, i, key, d_Y.data_ptr(), d_rm.data_ptr(), None))
        torch.cuda.synchronize()
        r, Ybar, rm, det = nsc.reverse_once(orc, oenv, setting, s0, i, r, Ybar, sched, N, H, 0.1, impl)
        same_bits(plan.peek()[0], det["Y0s"], f"{name}: candidates of step {i}")
        same_bits(d_Y.cpu().numpy().reshape(H, -1), Ybar, f"{name}: mean after step {i}")
        assert np.array_equal(np.array([key[0], key[1]], np.uint32), r)
    plan.close()


def test_refusals_on_a_plan(gpu):
    """What only a real handle decides: rows against Hsample, cols against action_size; a refused call leaves the setting."""
    import ctypes as C
    from mbd_hip.planners.mbd_planner import Plan, Sweep
    env = _env("hopper")
    a = _args("hopper", 64, 6, 6)
    plan, sweep = Plan(env, a), Sweep(env, a, 2)
    lib = plan.lib
    for setter, h in ((lib.mbd_plan_set_noise_shape, plan.h), (lib.mbd_sweep_set_noise_shape, sweep.h)):
        for shape, field in (((5, 3), b"rows=5"), ((7, 3), b"rows=7"), ((6, 2), b"cols=2"), ((6, 4), b"cols=4")):
            gg = np.ones(shape, np.float32)
            rec = gpu.NoiseShape()
            rec.scale = gg.ctypes.data_as(C.POINTER(C.c_float))
            rec.rows, rec.cols = shape
            assert setter(h, C.byref(rec)) == gpu.MBD_ERR_INVALID and field in lib.mbd_last_error(), lib.mbd_last_error()
    with pytest.raises(ValueError):
        plan.set_noise_shape(np.ones((6, 3), np.float32), when="sometimes")
    plan.set_noise_shape(np.array([1.0, 0.5, 2.0], np.float32))  # (one value per actuator broadcasts over the rows)
    sweep.set_noise_shape(np.ones((6, 1), np.float32), "warm")
    plan.close()
    sweep.close()
