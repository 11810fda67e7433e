"""-m gpu: noise bases (include/mbd_hip.h mbd_noise_basis; DESIGN.md section 1 "N8 noise basis") against the checker's
restatement, tests/noise_basis_checker.py.  Bit for bit (same_bits / np.array_equal) unless said otherwise.

  kernel alone      knot_noise_kernel through mbd_debug_knot_noise: both threefry layouts, with and without a shape, on 1 and 3
                    workgroups (the column loop strides), a dense W with negative values, values above 1, a zero row, a zero
                    column and scattered exact zeros
  identity          n_knots = Hsample, W = I: the plan without a basis, in value
  whole plans       hopper, humanoidrun, car2d, an mppi and a cma-es plan under 3 knots, with the last step's candidates
  episodes          both modes, E = 1 and 2; with a plant (the disturbances stay white); with an ensemble; a basis and a shape
                    with different `when`
  sweeps            episodes and open-loop runs equal the single plans'; the batched kernels above their grid cap
  set, then clear   between two steps of a plan that had prepared the next normals: fused -> second stream and back
  sharded           the phase calls of a sharded plan on one device equal the unsharded step
  refusals          what only a real handle decides
"""
import ctypes as C

import numpy as np
import pytest

import ensemble_checker
import mpc_checker
import mpc_plant_checker
import noise_basis_checker as nbc
import sampler_inputs as sx
from oracle import planner as op
from state_inputs import same_bits
from noise_basis_checker import basis_of
from test_gpu_noise_shape import _args, _env, _equal, _oenv, _state, shape_of

pytestmark = pytest.mark.gpu

_LOGS = ("means", "actions", "rewards", "states")


@pytest.fixture(scope="module")
def gpu(lib):
    from mbd_hip import _capi
    if _capi.device_count() < 1:
        pytest.fail("tests/test_gpu_noise_basis.py needs a GPU")
    return _capi


def knots3(H):
    """The 3-knot basis of the whole-plan tests: signed, rows of different norms, exact zeros among the weights."""
    W = basis_of(H, 3)
    W[H // 2] = (0.5, -0.25, 1.25)  # (no frozen row: every row of a whole plan explores)
    return W


# ---- the kernel alone --------------------------------------------------------------------------------------------------------

_SIZES = [(1, 1, 1, 1), (3, 4, 1, 2), (37, 7, 3, 3), (5, 16, 2, 16), (101, 11, 3, 5), (257, 5, 1, 16), (64, 50, 17, 10), (513, 6, 3, 4)]


@pytest.mark.parametrize("layout", sx.LAYOUTS, ids=["legacy", "part"])
@pytest.mark.parametrize("shaped", [False, True], ids=["noshape", "shape"])
@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("N,H,Nu,K", _SIZES, ids=["-".join(map(str, s)) for s in _SIZES])
def test_knot_kernel_alone(gpu, orc, N, H, Nu, K, blocks, shaped, layout):
    """z [N][H][Nu] of knot_noise_kernel against the checker's, every element; (37, 7, 3, 3) has an odd knot tensor, whose last
    threefry block of the legacy layout is padded; one workgroup holds 64 columns, so all but the smallest sizes stride."""
    W = basis_of(H, K)
    g = shape_of(H, Nu) if shaped else None
    key = gpu.prng_key(700 + N)
    z = gpu.debug_knot_noise(key, layout, N, H, Nu, W, g, blocks)
    _, want = nbc.BasisOracle(orc, W, g).sample(key, layout, N, H, Nu, 0, N, 1.0, np.zeros((H, Nu), np.float32), want_eps=True)
    same_bits(z, want, f"N={N} H={H} Nu={Nu} K={K} blocks={blocks}")
    if H >= 3:  # the zero row: z = +0 by bit pattern, under a shape as well
        assert not z[:, H // 2, :].view(np.uint32).any()


# ---- identity ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["hopper", "humanoidrun"])
def test_identity_basis_is_no_basis_in_value(gpu, name):
    from mbd_hip.planners.mbd_planner import Plan
    env, H = _env(name), 6
    plan = Plan(env, _args(name, 128, H, 6))
    plan.set_state0(env.reset(gpu.prng_key(7)))
    key = gpu.prng_key(8)
    ref = plan.run(key)
    plan.set_noise_basis(np.eye(H, dtype=np.float32))
    got = plan.run(key)
    for x, y in zip(got[:3], ref[:3]):
        assert np.array_equal(np.asarray(x, np.float32), np.asarray(y, np.float32)), name  # (==: the sign of a zero may differ)
    plan.set_noise_basis(knots3(H))
    assert not np.array_equal(plan.run(key)[0], ref[0])
    plan.set_noise_basis(None)
    assert np.array_equal(plan.run(key)[0], ref[0])
    plan.close()


# ---- whole plans ---------------------------------------------------------------------------------------------------------------

def _checker_plan(orc, oenv, W, s0, key, N, H, Nd, temp, impl):
    sched = orc.schedule(1e-4, 1e-2, Nd)
    r, Ybar = np.asarray(key, np.uint32), np.zeros((H, oenv.Nu), np.float32)
    mus, rms, det = [], [], None
    for i in range(Nd - 1, 0, -1):
        r, Ybar, rm, det = nbc.reverse_once(orc, oenv, W, s0, i, r, Ybar, sched, N, H, temp, impl)
        mus.append(Ybar)
        rms.append(rm)
    rew_final = op.mean_h(orc, np.ascontiguousarray(oenv.rollout(s0, Ybar[None])))[0]
    return np.stack(mus), np.array(rms, np.float32), rew_final, det


@pytest.mark.parametrize("name,N,H", [("hopper", 96, 6), ("humanoidrun", 128, 5), ("car2d", 100, 6)])
def test_whole_plan_matches_the_checker(gpu, orc, name, N, H):
    from mbd_hip.envs.base import prng_impl
    from mbd_hip.planners.mbd_planner import Plan
    env, Nd = _env(name), 6
    st, key = env.reset(gpu.prng_key(3)), gpu.prng_key(4)
    W = knots3(H)
    plan = Plan(env, _args(name, N, H, Nd))
    plan.set_state0(st)
    plan.set_noise_basis(W)
    mu, rm, rf, _ = plan.run(key)
    Y0s, rewss, w = plan.peek()
    plan.close()
    want = _checker_plan(orc, _oenv(orc, env), W, _state(env, st), key, N, H, Nd, 0.1, prng_impl())
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
    W = knots3(H)
    plan = Plan(env, args, update_method=op.PI_METHODS[method])
    plan.set_state0(st)
    plan.set_noise_basis(W)
    mu_gpu, rm_gpu, _, _ = plan.run(key)
    Y0s_gpu = plan.peek()[0]
    sigma_gpu = plan.get_sigma()
    plan.close()
    bo, s0 = nbc.BasisOracle(orc, W), _state(env, st)
    r, mu, sigma = np.asarray(key, np.uint32), np.zeros((H, env.action_size), np.float32), np.float32(1.0)
    for t in range(Nr - 1, 0, -1):
        keys = orc.split(r, 2, impl)
        r, ks = keys[0], keys[1]
        Y0s = bo.sample(ks, impl, N, H, env.action_size, 0, N, float(sigma), mu)
        rews = op.mean_h(orc, np.ascontiguousarray(oenv.rollout(s0, Y0s)))
        mu, sigma, _, rm = orc.pi_update(op.PI_METHODS[method], rews, Y0s, mu, float(sigma), 0.1)
        same_bits(mu_gpu[Nr - 1 - t], mu, f"{method}: mean of step {t}")
        same_bits(np.float32(rm_gpu[Nr - 1 - t]), np.float32(rm), f"{method}: mean reward of step {t}")
    same_bits(Y0s_gpu, Y0s, f"{method}: the last step's candidates")
    same_bits(np.float32(sigma_gpu), np.float32(sigma), f"{method}: sigma")


# ---- episodes ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,N,H", [("hopper", 64, 6), ("humanoidrun", 128, 5), ("car2d", 64, 6)])
@pytest.mark.parametrize("E", [1, 2])
@pytest.mark.parametrize("when", ["always", "warm"])
def test_episode_matches_the_checker(gpu, orc, name, N, H, E, when):
    """T = 3, K = 2.  The warm mode's tick 0 is mbd_plan_run(k_0); in both modes T = 2 is a prefix of T = 3 and means, actions,
    rewards and states equal the checker episode's."""
    from mbd_hip.envs.base import prng_impl
    from mbd_hip.planners.mbd_planner import Plan
    env, Nd, T, K = _env(name), 6, 3, 2
    st, key = env.reset(gpu.prng_key(5)), gpu.prng_key(6)
    W = knots3(H)
    plan = Plan(env, _args(name, N, H, Nd))
    plan.set_state0(st)
    k0 = gpu.prng_split(key, 2, plan.cfg.prng_impl)[1]
    flat_mu0 = plan.run(k0)[0]
    plan.set_noise_basis(W, when)
    ep = plan.run_mpc(key, T, K, E)
    short = plan.run_mpc(key, T - 1, K, E)
    mu0 = plan.run(k0)[0]
    plan.close()
    for k in _LOGS:
        assert np.array_equal(short[k], ep[k][: len(short[k])]), k
    assert np.array_equal(ep["means"][0], mu0[-1])
    assert np.array_equal(mu0, flat_mu0) == (when == "warm")
    ref = nbc.episode(mpc_checker.episode, _oenv(orc, env), W, when, Nd, _state(env, st), key, N, H, Nd, 0.1, T, K, E,
                      impl=prng_impl())
    _equal(ep, ref, f"{name} {when} E={E}")
    assert np.isfinite(ref["states"]).all()


def test_plant_disturbances_stay_white(gpu, orc):
    """hopper with action noise and a kick every second tick on a heavier plant: the executed rows are M_t[0:E] + act_std * eps
    with the disturbance chain's own normals — E Nu + 3 white ones per tick, the checker's ``orc.normal`` — under either mode."""
    from mbd_hip.envs.base import RigidBodyEnv, prng_impl
    from mbd_hip.planners.mbd_planner import Plan
    name, N, H, Nd, T, K, E = "hopper", 64, 6, 6, 3, 2, 2
    env = _env(name)
    plant = RigidBodyEnv(name, model=env.sys.scaled(mass=1.3))
    st, key, dkey = env.reset(gpu.prng_key(5)), gpu.prng_key(6), gpu.prng_key(11)
    W = knots3(H)
    for when in ("always", "warm"):
        plan = Plan(env, _args(name, N, H, Nd))
        plan.set_state0(st)
        plan.set_mpc_plant(env=plant, key=dkey, act_std=0.3, kick_std=0.5, kick_every=2)
        plan.set_noise_basis(W, when)
        ep = plan.run_mpc(key, T, K, E)
        plan.close()
        ref = nbc.episode(mpc_plant_checker.episode, _oenv(orc, env), W, when, Nd, _state(env, st), key, N, H, Nd, 0.1, T, K, E,
                          plant=_oenv(orc, plant), dkey=dkey, act_std=0.3, kick_std=0.5, kick_every=2, impl=prng_impl())
        _equal(ep, ref, f"plant {when}")
        assert not np.array_equal(ref["actions"][:E], ref["means"][0][:E])


def test_ensemble_episode_matches_the_checker(gpu, orc):
    """M = 2: the launch over M N candidates reads the correlated normals; its noise job goes to the second stream."""
    from mbd_hip.envs.base import RigidBodyEnv
    from mbd_hip.planners.mbd_planner import Plan
    name, N, H, Nd, T, K, E = "hopper", 64, 6, 6, 3, 2, 1
    env = _env(name)
    member = RigidBodyEnv(name, model=env.sys.scaled(mass=1.3, gear=0.8))
    st, key = env.reset(gpu.prng_key(5)), gpu.prng_key(6)
    W = knots3(H)
    oenv, omember = _oenv(orc, env), _oenv(orc, member)
    for when, risk in (("always", "mean"), ("warm", "min")):
        plan = Plan(env, _args(name, N, H, Nd))
        plan.set_state0(st)
        plan.set_ensemble([None, member], risk)
        plan.set_noise_basis(W, when)
        ep = plan.run_mpc(key, T, K, E)
        plan.close()
        ref = nbc.episode(lambda e, *a, **kw: ensemble_checker.episode(e, [None, omember], risk, *a, **kw), oenv, W, when, Nd,
                          _state(env, st), key, N, H, Nd, 0.1, T, K, E)
        _equal(ep, ref, f"ensemble {when} {risk}")


@pytest.mark.parametrize("name,N,H", [("hopper", 64, 6), ("humanoidrun", 128, 5)])
@pytest.mark.parametrize("when,shape_when", [("always", "warm"), ("warm", "always")])
def test_basis_and_shape_with_different_when(gpu, orc, name, N, H, when, shape_when):
    """A plan carries both settings, each with its own `when`: tick 0 sees only the one that is always in force."""
    from mbd_hip.envs.base import prng_impl
    from mbd_hip.planners.mbd_planner import Plan
    env, Nd, T, K, E = _env(name), 6, 3, 2, 1
    st, key = env.reset(gpu.prng_key(5)), gpu.prng_key(6)
    W, g = knots3(H), shape_of(H, env.action_size)
    plan = Plan(env, _args(name, N, H, Nd))
    plan.set_state0(st)
    plan.set_noise_shape(g, shape_when)
    plan.set_noise_basis(W, when)
    ep = plan.run_mpc(key, T, K, E)
    plan.close()
    ref = nbc.episode(mpc_checker.episode, _oenv(orc, env), W, when, Nd, _state(env, st), key, N, H, Nd, 0.1, T, K, E,
                      shape=g, shape_when=shape_when, impl=prng_impl())
    _equal(ep, ref, f"{name} basis {when}, shape {shape_when}")


# ---- sweeps --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("when", ["always", "warm"])
def test_sweep_episode_is_the_single_plans(gpu, when):
    from mbd_hip.planners.mbd_planner import Plan, Sweep
    name, N, H, Nd, T, K, E, P = "hopper", 64, 6, 6, 3, 2, 2, 2
    env = _env(name)
    a = _args(name, N, H, Nd)
    W = knots3(H)
    keys = np.array([gpu.prng_key(60 + k) for k in range(P)], np.uint32)
    states = [env.reset(gpu.prng_key(k)) for k in range(P)]
    sw = Sweep(env, a, P)
    for k in range(P):
        sw.set_state0(k, states[k])
    flat = sw.run_mpc(keys, T, K, E)
    sw.set_noise_basis(W, when)
    ep = sw.run_mpc(keys, T, K, E)
    mu = sw.run(keys)[0]
    sw.close()
    assert not np.array_equal(ep["means"], flat["means"])
    assert np.array_equal(ep["means"][:, 0], flat["means"][:, 0]) == (when == "warm")
    for k in range(P):
        p = Plan(env, a)
        p.set_state0(states[k])
        p.set_noise_basis(W, when)
        one = p.run_mpc(keys[k], T, K, E)
        mu1 = p.run(keys[k])[0]
        p.close()
        _equal({f: ep[f][k] for f in _LOGS}, one, f"episode {k} {when}")
        same_bits(mu[k], mu1, f"open loop, plan {k} {when}")


@pytest.mark.parametrize("layout", sx.LAYOUTS, ids=["legacy", "part"])
@pytest.mark.parametrize("name,N,H,steps,kind", sx.SWEEPS, ids=[f"{s[4]}-{s[0]}-N{s[1]}" for s in sx.SWEEPS])
def test_batched_kernels_under_a_basis(gpu, name, N, H, steps, kind, layout, monkeypatch):
    """knot_noise_batch_kernel as ONE sweep against the same plans run alone (whose launches are held to the checker above):
    humanoidrun N = 4096 has 69 632 columns a plan, above the 1024 x 64 the batched launch gives one — its column loop strides;
    the path-integral sweep adds shift_batch_kernel above its 4096 x 256."""
    monkeypatch.setenv("MBD_THREEFRY_PARTITIONABLE", str(layout))
    from mbd_hip.planners import path_integral
    from mbd_hip.planners.mbd_planner import Args, Plan, Sweep
    from mbd_hip.planners.mpc import knot_basis
    env, P = _env(name), 2
    if kind == "mbd":
        um, args = 0, Args(env_name=name, Nsample=N, Hsample=H, Ndiffuse=steps + 1, temp_sample=0.1, disable_recommended_params=True,
                           not_render=True)
    else:
        um, args = 1, path_integral.Args(env_name=name, Nsample=N, Hsample=H, Nrefine=steps + 1, temp_sample=0.1,
                                         disable_recommended_params=True)
    W = knot_basis(H, 10, "linear")
    keys = np.array([gpu.prng_key(50 + k) for k in range(P)], np.uint32)
    states = [env.reset(gpu.prng_key(k)) for k in range(P)]
    sw = Sweep(env, args, P, update_method=um)
    for k in range(P):
        sw.set_state0(k, states[k])
    flat = sw.run(keys)[0]
    sw.set_noise_basis(W)
    mu, rm, rf, _ = sw.run(keys)
    sw.set_noise_basis(None)
    again = sw.run(keys)[0]
    sw.close()
    assert np.isfinite(mu).all() and not np.array_equal(mu, flat) and np.array_equal(again, flat)
    for k in range(P):
        p = Plan(env, args, update_method=um)
        p.set_state0(states[k])
        p.set_noise_basis(W)
        mu1, rm1, rf1, _ = p.run(keys[k])
        p.close()
        same_bits(mu[k], mu1, f"{name} {kind} plan {k}: means")
        same_bits(rm[k], rm1, f"{name} {kind} plan {k}: mean rewards")
        same_bits(np.float32(rf[k]), np.float32(rf1), f"{name} {kind} plan {k}: final reward")


# ---- the set call --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,N,H", [("humanoidrun", 128, 5), ("humanoidrun", 4608, 4)])
def test_set_then_clear_between_two_steps(gpu, orc_omp, name, N, H):
    """mbd_plan_reverse_once declares the next step's key, whose normals are generated beside its rollout — N = 128: in the
    launch's spare workgroups while the plan is flat, on the second stream under a basis, so the settings below switch between
    the two and back; N = 4608 fills the chip: the second stream either way.  A set call between two steps: the step equals
    the checker under the NEW setting, whatever was prepared under the old one."""
    import torch
    from mbd_hip.envs.base import prng_impl
    from mbd_hip.planners.mbd_planner import Plan
    orc = orc_omp
    env, Nd = _env(name), 7
    impl = prng_impl()
    plan = Plan(env, _args(name, N, H, Nd))
    st = env.reset(gpu.prng_key(9))
    plan.set_state0(st)
    W, W2 = knots3(H), basis_of(H, 2)
    d_Y, d_rm = torch.zeros(H * env.action_size, device="cuda"), torch.zeros(1, device="cuda")
    key = (gpu.key_array(gpu.prng_key(10)))
    oenv, s0, sched = _oenv(orc, env), _state(env, st), orc.schedule(1e-4, 1e-2, Nd)
    r, Ybar = np.asarray(gpu.prng_key(10), np.uint32), np.zeros((H, env.action_size), np.float32)
    previous = None
    for i, setting in ((Nd - 1, None), (Nd - 2, W), (Nd - 3, W), (Nd - 4, None), (Nd - 5, W2), (Nd - 6, W2)):
        # between two steps: the previous step prepared this step's normals under the previous setting.  (No call where the
        # setting stays: that step consumes the normals knot_noise_kernel prepared on the second stream)
        if i < Nd - 1 and setting is not previous:
            plan.set_noise_basis(setting)
        previous = setting
        gpu.check(plan.lib.mbd_plan_reverse_once(plan.h, i, key, d_Y.data_ptr(), d_rm.data_ptr(), None))
        torch.cuda.synchronize()
        r, Ybar, rm, det = nbc.reverse_once(orc, oenv, setting, s0, i, r, Ybar, sched, N, H, 0.1, impl)
        same_bits(plan.peek()[0], det["Y0s"], f"{name}: candidates of step {i}")
        same_bits(d_Y.cpu().numpy().reshape(H, -1), Ybar, f"{name}: mean after step {i}")
        assert np.array_equal(np.array([key[0], key[1]], np.uint32), r)
    plan.close()


# ---- sharded phase calls -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,N,H,um", [("hopper", 96, 6, 0), ("car2d", 100, 6, 0), ("hopper", 96, 6, 1)],
                         ids=["lazy", "car2d", "mppi"])
def test_sharded_phase_calls_equal_the_unsharded_step(gpu, orc, name, N, H, um):
    """shard_begin / shard_count on one device: every rank forms all N candidates (a materialised plan samples the whole tensor
    on the caller's stream under a basis — N >= 5 shard_count would otherwise split it over two streams) and rolls out its own
    rows; candidates and the shard's rewards equal the unsharded step's and the checker's."""
    import torch
    from mbd_hip.envs.base import prng_impl
    from mbd_hip.planners import path_integral
    from mbd_hip.planners.mbd_planner import Plan
    env, Nd, i = _env(name), 6, 3
    if um:
        args = path_integral.Args(env_name=name, Nsample=N, Hsample=H, Nrefine=Nd, temp_sample=0.1, disable_recommended_params=True)
    else:
        args = _args(name, N, H, Nd)
    st, key = env.reset(gpu.prng_key(3)), gpu.prng_key(31)
    W = knots3(H)
    Ybar = (np.random.default_rng(2).normal(size=(H, env.action_size)) * 0.2).astype(np.float32)
    d_Y = torch.tensor(Ybar.reshape(-1), device="cuda")
    got = {}
    for begin, count in ((0, N), (0, 16), (32, 16), (N - 7, 7)):
        plan = Plan(env, args, shard_begin=begin, shard_count=count, update_method=um)
        plan.set_state0(st)
        plan.set_noise_basis(W)
        loc = torch.zeros(count, device="cuda")
        gpu.check(plan.lib.mbd_plan_sample_rollout(plan.h, i, gpu.key_array(key), d_Y.data_ptr(), loc.data_ptr(), None, None))
        torch.cuda.synchronize()
        got[(begin, count)] = (plan.peek()[0], loc.cpu().numpy())
        sigma = 1.0 if um else float(plan.schedule()[2][i])
        plan.close()
    ref = nbc.BasisOracle(orc, W).sample(key, prng_impl(), N, H, env.action_size, 0, N, sigma, Ybar)
    whole_Y, whole_r = got[(0, N)]
    same_bits(whole_Y, ref, f"{name}: the unsharded step's candidates")
    for (begin, count), (Y, rews) in got.items():
        same_bits(Y, whole_Y, f"{name}: candidates of shard [{begin}, +{count})")
        same_bits(rews, whole_r[begin:begin + count], f"{name}: rewards of shard [{begin}, +{count})")


# ---- refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals_on_a_plan_and_on_a_sweep(gpu):
    """What needs a real handle: a non-finite entry anywhere in [Hsample][n_knots] (and only there), each message naming the
    field; a refused call leaves the setting in force."""
    from mbd_hip.planners.mbd_planner import Plan, Sweep
    env, H = _env("hopper"), 6
    a = _args("hopper", 64, H, 6)
    plan, sweep = Plan(env, a), Sweep(env, a, 2)
    plan.set_state0(env.reset(gpu.prng_key(1)))
    lib = plan.lib

    def record(W, n_knots=None, when=0):
        W = np.ascontiguousarray(W, np.float32)
        rec = gpu.NoiseBasis()
        rec.basis = W.ctypes.data_as(C.POINTER(C.c_float))
        rec.n_knots, rec.when = (W.shape[1] if n_knots is None else n_knots), when
        return rec, W

    key = gpu.prng_key(2)
    plan.set_noise_basis(knots3(H))
    before = plan.run(key)[0]
    for setter, h in ((lib.mbd_plan_set_noise_basis, plan.h), (lib.mbd_sweep_set_noise_basis, sweep.h)):
        for bad in (np.nan, np.inf, -np.inf):
            W = np.ones((H, 3), np.float32)
            W[4, 1] = bad
            rec, keep = record(W)
            assert setter(h, C.byref(rec)) == gpu.MBD_ERR_INVALID and b"basis[4][1]" in lib.mbd_last_error(), lib.mbd_last_error()
        for k in (0, 17):
            rec, keep = record(np.ones((H, 17), np.float32), n_knots=k)
            assert setter(h, C.byref(rec)) == gpu.MBD_ERR_INVALID and b"n_knots=%d" % k in lib.mbd_last_error()
        rec, keep = record(np.ones((H, 3), np.float32), when=2)
        assert setter(h, C.byref(rec)) == gpu.MBD_ERR_INVALID and b"when=2" in lib.mbd_last_error()
        rec, keep = record(np.ones((H, 3), np.float32))
        rec.basis = None
        assert setter(h, C.byref(rec)) == gpu.MBD_ERR_INVALID and b"basis is NULL" in lib.mbd_last_error()
    with pytest.raises(ValueError):
        plan.set_noise_basis(np.ones((H, 3), np.float32), when="sometimes")
    with pytest.raises(ValueError):
        plan.set_noise_basis(np.ones((H + 1, 3), np.float32))
    assert np.array_equal(plan.run(key)[0], before)
    for setter, h in ((lib.mbd_plan_set_noise_basis, plan.h), (lib.mbd_sweep_set_noise_basis, sweep.h)):
        W = np.full((H + 1, 16), -3.0, np.float32)  # negative values and 16 knots are fine; the row beyond Hsample is not read
        W[H] = np.nan
        rec, keep = record(W)
        assert setter(h, C.byref(rec)) == gpu.MBD_OK
    assert not np.array_equal(plan.run(key)[0], before)
    plan.close()
    sweep.close()
