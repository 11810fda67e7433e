"""-m gpu: the HIP path (through the C ABI) against the CPU oracle on the same seeded inputs.

The numerical contract makes every comparison BIT-EXACT (np.array_equal), far inside the 1e-5 relative
tolerance the north star asks for — which is the only way to get a meaningful comparison through 350
chaotic contact-rich substeps (tests/test_oracle_physics.py::test_chaos_amplification)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import load_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(lib):
    from mbd_hip import _capi
    if _capi.device_count() < 1:
        pytest.fail("GPU tests need a visible MI355X; the product has no CPU fallback")
    return _capi


def _oenv(orc, env):
    from oracle.planner import OracleEnv
    if env.__class__.__name__ == "Car2d":
        return OracleEnv(orc, "car2d", xref=env.xref, rew_xref=env.rew_xref)
    return OracleEnv(orc, env.env_name, env.sys.to_struct(), xref=env.xref, rew_xref=env.rew_xref,
                     init_q=env.sys.init_q)


def test_library_loaded_is_in_tree(gpu):
    import os
    path = os.path.realpath(gpu.LIB_PATH)
    assert path.endswith("model-based-diffusion_amd/lib/libmbd_hip.so")
    with open("/proc/self/maps") as f:
        assert any("libmbd_hip.so" in line for line in f), "native library not mapped"


@pytest.mark.parametrize("impl", [0, 1])
def test_prng_split_and_reset(gpu, orc, impl, monkeypatch):
    monkeypatch.setenv("MBD_THREEFRY_PARTITIONABLE", str(impl))
    from mbd_hip.envs import get_env
    key = gpu.prng_key(7)
    assert np.array_equal(key, orc.prng_key(7))
    for num in (2, 3):
        assert np.array_equal(gpu.prng_split(key, num, impl), orc.split(key, num, impl))
    for name in ("humanoidrun", "hopper", "halfcheetah", "humanoidtrack", "walker2d", "humanoidstandup",
                 "cartpole", "ant", "car2d"):
        env = get_env(name)
        st = env.reset(key)
        ref = _oenv(orc, env).reset(key, impl)
        assert np.array_equal(np.asarray(st.pipeline_state).reshape(-1), ref.reshape(-1)), name


@pytest.mark.parametrize("impl,seed,want", [(0, 42, [0.18693547, -1.2806505, -1.5593132]),
                                            (1, 42, [-0.028304616, None, None])])
def test_sample_kernel_reproduces_published_jax_normals(gpu, orc, impl, seed, want, monkeypatch):
    """The device noise generator (sample_kernel: threefry -> bits -> uniform -> erf_inv) against normal
    draws printed in JAX's documentation (sources: tests/test_oracle_prng.py). Y0s = 0 + 0.5 * eps is exact
    in f32, so the published eps must come back bit for bit; entries the docs do not show are checked
    against the oracle."""
    import torch
    monkeypatch.setenv("MBD_THREEFRY_PARTITIONABLE", str(impl))
    from mbd_hip.envs import get_env
    from mbd_hip.planners.path_integral import Args
    from mbd_hip.planners.mbd_planner import Plan
    env = get_env("hopper")  # Nu = 3: eps has shape (1, 1, 3), the same counters as shape (3,)
    plan = Plan(env, Args(env_name="hopper", Nsample=1, Hsample=1, Nrefine=2), update_method=1)
    plan.set_state0(env.reset(gpu.prng_key(0)))
    plan.set_sigma(0.5)
    key = gpu.prng_key(seed)
    Ybar, loc = torch.zeros(3, device="cuda"), torch.zeros(1, device="cuda")
    gpu.check(plan.lib.mbd_plan_sample_rollout(plan.h, 1, gpu.key_array(key), Ybar.data_ptr(), loc.data_ptr(),
                                               None, None))
    torch.cuda.synchronize()
    eps = plan.peek()[0].reshape(3) * np.float32(2.0)
    plan.close()
    ref = orc.normal(key, (3,), impl)
    assert np.array_equal(eps, ref)
    for got, w in zip(eps, want):
        if w is not None:
            assert got == np.float32(w)


@pytest.mark.parametrize("name,B,H,sigma", [("humanoidrun", 96, 50, 0.6), ("humanoidrun", 1, 3, 0.3),
                                            ("humanoidtrack", 64, 50, 0.4), ("hopper", 80, 50, 0.5),
                                            ("halfcheetah", 72, 50, 0.5), ("walker2d", 40, 50, 0.5),
                                            ("humanoidstandup", 36, 50, 0.5), ("cartpole", 200, 50, 0.8),
                                            ("ant", 44, 50, 0.5), ("car2d", 128, 30, 0.5),
                                            ("car2d", 3, 50, 1.0)])
def test_rollout_bitexact(gpu, orc, name, B, H, sigma):
    _rollout_bitexact(gpu, orc, name, B, H, sigma)


@pytest.mark.parametrize("name,B,H,sigma", [("humanoidrun", 40, 50, 0.6), ("humanoidstandup", 20, 30, 0.5),
                                            ("hopper", 48, 50, 0.5), ("halfcheetah", 24, 50, 0.5),
                                            ("walker2d", 24, 30, 0.5), ("ant", 20, 50, 0.5), ("cartpole", 64, 50, 0.8)])
def test_rollout_bitexact_shuffle_fallback(gpu, orc, name, B, H, sigma, monkeypatch, levers):
    """Every built-in tree fits a DPP family, so the ds_bpermute exchange — the path an arbitrary MJCF tree
    takes — is forced with MBD_NO_DPP=1 (read when the env is created) and held to the same bit-exact bar."""
    levers(MBD_NO_DPP=1)
    _rollout_bitexact(gpu, orc, name, B, H, sigma)


@pytest.mark.parametrize("name,B,H,sigma", [("humanoidrun", 24, 20, 0.6), ("humanoidtrack", 16, 20, 0.4),
                                            ("humanoidstandup", 12, 20, 0.5), ("hopper", 48, 50, 0.5),
                                            ("halfcheetah", 24, 50, 0.5), ("walker2d", 24, 30, 0.5),
                                            ("cartpole", 64, 50, 0.8)])
def test_rollout_bitexact_general_instantiations(gpu, orc, name, B, H, sigma, monkeypatch, levers):
    """The built-in models run instantiations with their switches, reward kind and n_frames as compile-time constants;
    a model that differs in any of them (another MJCF, another n_frames) runs the general instantiation of the same
    kernel.  Forced here for the built-in models (switches read per launch) and held to the same bar."""
    for k in ("MBD_NO_PLANAR_FLAGS", "MBD_NO_REWARD_CONST", "MBD_NO_NFR_CONST"):
        levers(**{k: 1})
    _rollout_bitexact(gpu, orc, name, B, H, sigma)
    levers(MBD_NO_PLANAR_FLAGS=-1)  # (n_frames at run time under the compile-time switches)
    levers(MBD_NO_REWARD_CONST=-1)
    _rollout_bitexact(gpu, orc, name, B, H, sigma)


@pytest.mark.parametrize("name,nf,B,H", [("humanoidrun", 1, 12, 20), ("humanoidrun", 4, 12, 12), ("humanoidrun", 9, 8, 8),
                                         ("humanoidstandup", 3, 8, 10), ("hopper", 7, 32, 20), ("hopper", 21, 16, 10),
                                         ("halfcheetah", 5, 16, 20), ("cartpole", 3, 32, 20), ("walker2d", 1, 16, 20)])
def test_rollout_bitexact_other_n_frames(gpu, orc, name, nf, B, H):
    """n_frames is a compile-time constant of the instantiations the built-in models run (NFR); a model with another
    value — odd, 1, larger than any built-in — takes the run-time loops (pairs / fours plus a remainder)."""
    from conftest import load_model
    from mbd_hip.envs.base import RigidBodyEnv
    m = load_model(name)
    m.fields["n_frames"] = nf
    env = RigidBodyEnv(name, model=m)
    st = env.reset(gpu.prng_key(5))
    rng = np.random.default_rng(nf * 100 + B)
    us = np.clip(rng.normal(size=(B, H, env.action_size)) * 0.5, -1.3, 1.3).astype(np.float32)
    want = env.xref is not None
    out = env.rollout(st, us, want_xpos=want)
    ref = _oenv(orc, env).rollout(np.asarray(st.pipeline_state, np.float32), us, want_xpos=want)
    got = (out[0] if want else out).cpu().numpy()
    assert np.isfinite(got).all() and np.array_equal(got, ref[0] if want else ref), f"{name} n_frames={nf}"


@pytest.mark.parametrize("no_dpp", [False, True])
def test_custom_mjcf_model_on_the_general_kernels(gpu, orc, no_dpp, monkeypatch, levers):
    """A model only a custom MJCF file produces (tests/custom_models.py: full inertia tensors, 1/2/3-dof hinges with
    springs and dampers, a slide + hinge joint, four children on the root, two colliders on one link) through
    mjcf.load -> mbd_env_create_model -> the general 3-D instantiation, rollouts and one planning step, bit for bit."""
    from custom_models import CRAB
    from test_oracle_physics import _compile
    from mbd_hip.envs.base import RigidBodyEnv
    if no_dpp:
        levers(MBD_NO_DPP=1)
    m = _compile(CRAB, env_name="hopper", n_frames=3, reset_noise=0.02, reward_params=(1.0, 0.5))
    F = m.fields
    assert F["iso_inertia"] == 0 and np.abs(F["inv_inertia"][:m.n_links, 3:]).max() > 1.0  # (not even diagonal)
    assert F["n_slide"].max() == 1 and F["n_rot"].max() == 3 and np.bincount(F["parent"][1:m.n_links]).max() == 4
    env = RigidBodyEnv("hopper", model=m)
    st = env.reset(gpu.prng_key(11))
    rng = np.random.default_rng(4)
    us = np.clip(rng.normal(size=(37, 25, env.action_size)) * 0.6, -1.3, 1.3).astype(np.float32)
    got = env.rollout(st, us).cpu().numpy()
    ref = _oenv(orc, env).rollout(np.asarray(st.pipeline_state, np.float32), us)
    assert np.isfinite(got).all() and np.ptp(got) > 1e-3
    assert np.array_equal(got, ref), f"max |d| = {np.abs(got - ref).max()}"
    _one_step(gpu, orc, "hopper", 96, 12, 20, 0.1, 1, False, i=12, env=env)


@pytest.mark.parametrize("seed", range(16))
def test_random_models_on_the_general_kernels(gpu, orc, seed, levers):
    """Fuzz (tests/random_models.py): random link trees — 1 / 2 / 3-dof hinges, slide + hinge joints, fused bodies, up to four
    children and two colliders on a link, both inertia classes, springs, dampers, restitution — through mjcf.load ->
    mbd_env_create_model -> whichever general instantiation the library picks (every third seed with the DPP layouts off):
    rollouts long enough to hit the ground (90 control steps) and one planning step, bit for bit."""
    from random_models import stable_random_model
    from test_random_models import _comp
    from mbd_hip.envs.base import RigidBodyEnv
    if seed % 3 == 2:
        levers(MBD_NO_DPP=1)
    _, m = stable_random_model(seed, _comp)
    env = RigidBodyEnv("hopper", model=m)
    st = env.reset(gpu.prng_key(seed))
    rng = np.random.default_rng(seed)
    us = np.clip(rng.normal(size=(37, 90, env.action_size)) * 0.6, -1.3, 1.3).astype(np.float32)
    got = env.rollout(st, us).cpu().numpy()
    ref = _oenv(orc, env).rollout(np.asarray(st.pipeline_state, np.float32), us)
    assert np.isfinite(got).all() and np.ptp(got) > 1e-4
    assert np.array_equal(got, ref), f"seed {seed}: max |d| = {np.abs(got - ref).max()}"
    _one_step(gpu, orc, "hopper", 64, 10, 20, 0.1, 1, False, i=10, env=env)


def test_custom_model_with_three_colliders_on_a_link(gpu, orc):
    """A fused body hands its spheres to its parent's link: three to five colliders on a link outside the humanoids' shape
    run through the general instantiation of the specification switches (five collider slots, zero flag word = the default
    specification), bit for bit; more than five are refused by name."""
    from random_models import random_mjcf, stable_random_model
    from test_random_models import _comp
    from mbd_hip.envs.base import RigidBodyEnv
    found = 0
    for seed in range(16, 200):
        _, m = stable_random_model(seed, _comp)
        F = m.fields
        most = int(np.bincount(np.asarray(F["col_link"][:int(F["n_col"])]), minlength=m.n_links).max())
        if most < 3:
            continue
        assert most <= 5
        env = RigidBodyEnv("hopper", model=m)
        st = env.reset(gpu.prng_key(seed))
        us = np.clip(np.random.default_rng(seed).normal(size=(21, 90, env.action_size)) * 0.6, -1.3, 1.3).astype(np.float32)
        got = env.rollout(st, us).cpu().numpy()
        ref = _oenv(orc, env).rollout(np.asarray(st.pipeline_state, np.float32), us)
        assert np.array_equal(got, ref), f"seed {seed}: max |d| = {np.abs(got - ref).max()}"
        found += 1
        if found == 3:
            break
    assert found == 3
    six = random_mjcf(0, max_bodies=3, kinds=("h1",), probs=(1,)).replace(
        "</body>", "".join(f'<geom type="sphere" pos="0 {0.02 * k} 0" size="0.03" contype="1" conaffinity="1"/>' for k in range(6)) + "</body>", 1)
    with pytest.raises(Exception, match="colliders"):
        RigidBodyEnv("hopper", model=_comp(six))


@pytest.mark.parametrize("planar", [None, False])
@pytest.mark.parametrize("seed", range(8))
def test_random_planar_models(gpu, orc, seed, planar):
    """Fuzz, planar variant: random planar trees of 3..10 links (4-, 8- and 16-lane candidate groups) through the planar
    kernels (planar=None) and, compiled planar=False, through the general 3-D axisymmetric / full-tensor instantiations."""
    from random_models import stable_random_model
    from test_random_models import _comp
    from mbd_hip.envs.base import RigidBodyEnv
    _, m = stable_random_model(seed, lambda x: _comp(x, env_name="halfcheetah", planar=planar), planar=True, max_bodies=10)
    assert bool(int(m.fields["flags"]) & 2) == (planar is None)
    env = RigidBodyEnv("halfcheetah", model=m)
    st = env.reset(gpu.prng_key(seed))
    us = np.clip(np.random.default_rng(seed).normal(size=(29, 90, env.action_size)) * 0.6, -1.3, 1.3).astype(np.float32)
    got = env.rollout(st, us).cpu().numpy()
    ref = _oenv(orc, env).rollout(np.asarray(st.pipeline_state, np.float32), us)
    assert np.isfinite(got).all() and np.array_equal(got, ref), f"seed {seed}: max |d| = {np.abs(got - ref).max()}"
    _one_step(gpu, orc, "halfcheetah", 48, 8, 20, 0.4, 1, False, i=10, env=env)


@pytest.mark.parametrize("planar", [None, False])
def test_custom_planar_model_sixteen_lane_groups(gpu, orc, planar):
    """tests/custom_models.py TRIPOD: a planar model of ten links — a 16-lane candidate group, which no built-in planar
    model needs — with joint springs, a limited root slide and restitution all at once (the planar kernel's run-time
    switches), as the planar restatement (MBD_FLAG_PLANAR) and, compiled with planar=False, through the 3-D
    arithmetic of the general axisymmetric 16-lane instantiation.  Each against the checker's matching arithmetic."""
    from custom_models import TRIPOD
    from test_oracle_physics import _compile
    from mbd_hip.envs.base import RigidBodyEnv
    m = _compile(TRIPOD, env_name="halfcheetah", n_frames=6, reset_noise=0.05, reward_params=(1.0, 0.1), planar=planar)
    assert m.n_links == 10 and bool(m.fields["flags"] & 2) == (planar is None)
    env = RigidBodyEnv("halfcheetah", model=m)
    st = env.reset(gpu.prng_key(2))
    rng = np.random.default_rng(9)
    us = np.clip(rng.normal(size=(29, 30, env.action_size)) * 0.6, -1.3, 1.3).astype(np.float32)
    got = env.rollout(st, us).cpu().numpy()
    ref = _oenv(orc, env).rollout(np.asarray(st.pipeline_state, np.float32), us)
    assert np.isfinite(got).all() and np.ptp(got) > 1e-3
    assert np.array_equal(got, ref), f"max |d| = {np.abs(got - ref).max()}"
    _one_step(gpu, orc, "halfcheetah", 80, 10, 20, 0.4, 1, False, i=10, env=env)


def _rollout_bitexact(gpu, orc, name, B, H, sigma):
    """Rewards (and tracked positions where the env has a demo) of a rollout from a reset state, by BIT PATTERN
    (state_inputs.same_bits: -0.0 is not +0.0) against the checker's."""
    from state_inputs import same_bits
    from mbd_hip.envs import get_env
    env = get_env(name)
    st = env.reset(gpu.prng_key(3))
    rng = np.random.default_rng(B * 1000 + H)
    us = np.clip(rng.normal(size=(B, H, env.action_size)) * sigma, -1.3, 1.3).astype(np.float32)
    want = env.xref is not None
    out = env.rollout(st, us, want_xpos=want)
    oe = _oenv(orc, env)
    ref = oe.rollout(np.asarray(st.pipeline_state, np.float32), us, want_xpos=want)
    if want:
        same_bits(out[0].cpu().numpy(), ref[0], f"{name}: rewards")
        same_bits(out[1].cpu().numpy(), ref[1], f"{name}: tracked positions")
    else:
        got = out.cpu().numpy()
        assert np.isfinite(got).all()
        same_bits(got, ref, f"{name}: rewards (max |d| = {np.abs(got - ref).max()})")


@pytest.mark.parametrize("name", ["humanoidrun", "hopper", "halfcheetah", "cartpole", "car2d"])
def test_env_step_matches_oracle(gpu, orc, name):
    from mbd_hip.envs import get_env
    env = get_env(name)
    st = env.reset(gpu.prng_key(11))
    rng = np.random.default_rng(5)
    ms = None if name == "car2d" else env.sys.to_struct()
    s_ref = np.asarray(st.pipeline_state, np.float32)
    for t in range(5):
        a = rng.uniform(-1, 1, env.action_size).astype(np.float32)
        st = env.step(st, a)
        if name == "car2d":
            s_ref, r_ref = orc.car2d_step(s_ref, a)
        else:
            s_ref, r_ref = orc.env_step(ms, s_ref, a)
        assert np.array_equal(np.asarray(st.pipeline_state), s_ref.reshape(np.asarray(st.pipeline_state).shape))
        assert np.float32(st.reward) == np.float32(r_ref)


def _one_step(gpu, orc, name, N, H, Nd, temp, impl, demo, i=None, env=None, state0=None):
    """One diffusion step of a plan against the checker's, by bit pattern.  state0: a pipeline state to plan from instead of
    the reset state (Plan.set_state0 only reads state.pipeline_state)."""
    from state_inputs import same_bits
    from mbd_hip.envs import get_env
    from mbd_hip.planners.mbd_planner import Args, Plan
    from oracle import planner as op
    import torch
    env = get_env(name) if env is None else env
    args = Args(env_name=name, Nsample=N, Hsample=H, Ndiffuse=Nd, temp_sample=temp, enable_demo=demo,
                disable_recommended_params=True, not_render=True)
    key = gpu.prng_key(1)
    rng, rng_reset = gpu.prng_split(key, 2, impl)
    st = env.reset(rng_reset)
    if state0 is not None:
        st = st.replace(pipeline_state=np.asarray(state0, np.float32).reshape(np.asarray(st.pipeline_state).shape))
    plan = Plan(env, args)
    plan.set_state0(st)
    i = Nd - 1 if i is None else i
    g = np.random.default_rng(0)
    Ybar = (g.normal(size=(H, env.action_size)) * 0.2).astype(np.float32)
    d_Y = torch.tensor(Ybar.reshape(-1), device="cuda")
    d_rm = torch.zeros(1, device="cuda")
    k = (C.c_uint32 * 2)(int(rng[0]), int(rng[1]))
    gpu.check(plan.lib.mbd_plan_reverse_once(plan.h, i, k, d_Y.data_ptr(), d_rm.data_ptr(), None))
    torch.cuda.synchronize()
    Y0s, rewss, w = plan.peek()
    oe = _oenv(orc, env)
    sched = orc.schedule(args.beta0, args.betaT, Nd)
    r2, Y_ref, rm_ref, det = op.reverse_once(orc, oe, np.asarray(st.pipeline_state, np.float32), i, rng, Ybar, sched,
                                             N, H, temp, impl, enable_demo=demo)
    assert np.array_equal(np.array([k[0], k[1]], np.uint32), r2)
    same_bits(Y0s, det["Y0s"], "sampled candidates")
    same_bits(rewss, det["rewss"], "rollout rewards")
    same_bits(w, det["weights"], "softmax weights")
    same_bits(np.float32(d_rm.item()), np.float32(rm_ref), "mean reward")
    same_bits(d_Y.cpu().numpy().reshape(H, -1), Y_ref, "Ybar_{i-1}")
    assert abs(float(w.sum()) - 1.0) < 1e-5
    plan.close()


@pytest.mark.parametrize("name,H,demo", [("car2d", 7, False), ("car2d", 50, True), ("hopper", 11, False)])
@pytest.mark.parametrize("N", [1, 3, 63, 64, 65, 1000, 1024, 1025, 2500, 4096, 5003, 12288, 12289, 20011, 40001])
def test_score_update_ragged_sizes(gpu, orc, name, H, demo, N):
    """mbd_plan_score_update on its own, at candidate counts around every boundary of its kernels (score + weighted
    mean in one launch of 16-output x 64-group tiles while the weights fit 48 KB of LDS — 12 288 candidates; beyond,
    one 1024-thread score workgroup with logp0 in LDS up to 36 864 candidates and in a global scratch above, and the
    row-major two-kernel weighted mean): resident candidates from the sampler,
    SYNTHETIC rewards (ties, outliers) and demo log-densities, against the oracle bit for bit — weights, Ybar_{i-1},
    mean reward."""
    import torch
    from mbd_hip.envs import get_env
    from mbd_hip.planners.mbd_planner import Args, Plan
    env = get_env(name)
    args = Args(env_name=name, Nsample=N, Hsample=H, Ndiffuse=30, temp_sample=0.2, enable_demo=demo,
                disable_recommended_params=True, not_render=True)
    plan = Plan(env, args)
    plan.set_state0(env.reset(gpu.prng_key(3)))
    Nu, i = env.action_size, 17
    g = np.random.default_rng(N)
    Ybar = (g.normal(size=H * Nu) * 0.3).astype(np.float32)
    d_Y, loc = torch.tensor(Ybar, device="cuda"), torch.zeros(N, device="cuda")
    d_lp = torch.zeros(N, device="cuda") if demo else None
    ks = gpu.key_array(gpu.prng_key(N + 11))
    gpu.check(plan.lib.mbd_plan_sample_rollout(plan.h, i, ks, d_Y.data_ptr(), loc.data_ptr(),
                                               d_lp.data_ptr() if demo else None, None))
    torch.cuda.synchronize()
    Y0s = plan.peek()[0]
    a, ab, _ = plan.schedule()
    for case in range(3):
        rews = g.normal(size=N).astype(np.float32)
        if case == 1:
            rews[:] = np.float32(0.25)  # zero spread: the 1e-4 guard (mbd_planner.py:112)
        if case == 2 and N > 2:
            rews[N // 2] = 40.0
            rews[: N // 3] = rews[0]
        lp = (g.normal(size=N) * 3 - 2).astype(np.float32) if demo else None
        if demo and case == 1:
            continue  # a constant logp0 blend has zero spread and no guard at :125 (NaN in the reference too)
        d_r = torch.tensor(rews, device="cuda")
        d_l = torch.tensor(lp, device="cuda") if demo else None
        out, rm = torch.zeros(H * Nu, device="cuda"), torch.zeros(1, device="cuda")
        gpu.check(plan.lib.mbd_plan_score_update(plan.h, i, ks, d_Y.data_ptr(), d_r.data_ptr(),
                                                 d_l.data_ptr() if demo else None, out.data_ptr(), rm.data_ptr(), None))
        torch.cuda.synchronize()
        ref, w_ref, m_ref = orc.score_update(rews, Y0s, Ybar, float(a[i]), float(ab[i]), float(ab[i - 1]), 0.2,
                                             lp_demo=lp, rew_xref=float(env.rew_xref) if demo else 0.0)
        w = plan.peek()[2]
        # (a single candidate with demo has zero spread at :125: NaN here, in the oracle and in the reference)
        assert np.array_equal(w, w_ref, equal_nan=True), (N, case)
        assert np.array_equal(out.cpu().numpy(), ref, equal_nan=True), (N, case)
        assert np.float32(rm.item()) == np.float32(m_ref)
    plan.close()


@pytest.mark.parametrize("impl", [0, 1])
def test_reverse_once_humanoidrun(gpu, orc, impl, monkeypatch):
    monkeypatch.setenv("MBD_THREEFRY_PARTITIONABLE", str(impl))
    _one_step(gpu, orc, "humanoidrun", 192, 50, 100, 0.1, impl, False)


def test_reverse_once_hopper(gpu, orc):
    _one_step(gpu, orc, "hopper", 512, 50, 100, 0.1, 1, False, i=40)


def test_reverse_once_walker2d_and_standup(gpu, orc):
    _one_step(gpu, orc, "walker2d", 128, 50, 100, 0.1, 1, False, i=60)
    _one_step(gpu, orc, "humanoidstandup", 96, 50, 100, 0.1, 1, False, i=90)
    _one_step(gpu, orc, "cartpole", 256, 50, 100, 0.1, 1, False, i=95)
    _one_step(gpu, orc, "ant", 128, 50, 100, 0.1, 1, False, i=70)


def test_reverse_once_halfcheetah(gpu, orc):
    _one_step(gpu, orc, "halfcheetah", 256, 50, 100, 0.4, 1, False, i=70)


def test_reverse_once_humanoidtrack_demo(gpu, orc):
    _one_step(gpu, orc, "humanoidtrack", 128, 50, 100, 0.1, 1, True)


def test_reverse_once_car2d_demo(gpu, orc):
    _one_step(gpu, orc, "car2d", 128, 50, 50, 0.1, 1, True, i=20)


def test_run_diffusion_car2d_config1_end_to_end(gpu, orc):
    """BASELINE config 1: car2d, N=128, H=30, 50 diffusion steps — the whole run, bit for bit."""
    from mbd_hip.planners.mbd_planner import Args, run_diffusion
    from mbd_hip.envs import get_env
    from oracle import planner as op
    args = Args(seed=0, env_name="car2d", Nsample=128, Hsample=30, Ndiffuse=50, temp_sample=0.1,
                disable_recommended_params=True, not_render=True)
    rew, det = run_diffusion(args, return_details=True)
    env = get_env("car2d")
    ref = op.run_diffusion(orc, _oenv(orc, env), 0, 128, 30, 50, 0.1)
    assert np.array_equal(det["mu_0ts"], ref["mu_0ts"])
    assert np.array_equal(det["rew_means"], ref["rew_means"])
    assert np.float32(rew) == np.float32(ref["rew_final"])


def test_run_diffusion_humanoidrun_end_to_end_short(gpu, orc):
    """humanoidrun, N=64, H=20, 12 diffusion steps end to end, bit for bit (the oracle needs ~2 s)."""
    from mbd_hip.planners.mbd_planner import Args, run_diffusion
    from mbd_hip.envs import get_env
    from oracle import planner as op
    args = Args(seed=3, env_name="humanoidrun", Nsample=64, Hsample=20, Ndiffuse=12, temp_sample=0.1,
                disable_recommended_params=True, not_render=True)
    rew, det = run_diffusion(args, return_details=True)
    env = get_env("humanoidrun")
    ref = op.run_diffusion(orc, _oenv(orc, env), 3, 64, 20, 12, 0.1)
    assert np.array_equal(det["mu_0ts"], ref["mu_0ts"])
    assert np.float32(rew) == np.float32(ref["rew_final"])


@pytest.mark.parametrize("name,N,H,Nd,temp,demo,seed", [
    ("humanoidrun", 1024, 50, 100, 0.1, False, 0),       # the metric's plan (what bench.py's `parity` compares, seed 0)
    ("hopper", 512, 50, 100, 0.1, False, 1),             # BASELINE config 2
    ("halfcheetah", 1024, 50, 100, 0.4, False, 2),       # config 3
    ("humanoidtrack", 2048, 50, 100, 0.1, True, 3),      # config 5's plan on one GPU
    ("humanoidrun", 4096, 50, 40, 0.1, False, 4),        # config 4's size, 39 steps
    # round 6, the row-(f) envs at their reference sizes: walker2d (one candidate per wavefront + contact early-out), ant (the
    # reference's default env_name), humanoidstandup (helper lanes, five colliders on the torso, averaged)
    ("walker2d", 1024, 50, 16, 0.1, False, 5), ("ant", 1024, 50, 10, 0.1, False, 6), ("humanoidstandup", 1024, 50, 10, 0.1, False, 7),
    ("hopper", 2048, 50, 16, 0.1, False, 8)])            # (two candidates per wavefront)
def test_whole_runs_at_full_size_bitexact(gpu, orc_omp, name, N, H, Nd, temp, demo, seed):
    """WHOLE planning runs at the full size of the BASELINE configs, free-running (every step from the previous step's own
    result, mbd_planner.py:138-151) and the final evaluation (:179-180): the product's run_diffusion through the C ABI against
    the checker's (OpenMP over candidates: 1-10 s each) — reset state, mu_0ts of every step, every step's mean reward and
    rew_final, bit for bit.  (Round 4 held whole runs only at N = 64, H = 20 and full sizes only teacher-forced.)"""
    from mbd_hip.planners.mbd_planner import Args, run_diffusion
    from mbd_hip.envs import get_env
    from oracle import planner as op
    args = Args(seed=seed, env_name=name, Nsample=N, Hsample=H, Ndiffuse=Nd, temp_sample=temp, enable_demo=demo,
                disable_recommended_params=True, not_render=True)
    rew, det = run_diffusion(args, return_details=True)
    env = get_env(name)
    ref = op.run_diffusion(orc_omp, _oenv(orc_omp, env), seed, N, H, Nd, temp, enable_demo=demo)
    assert np.array_equal(np.asarray(det["state_init"].pipeline_state, np.float32).reshape(-1), ref["state_init"].reshape(-1))
    got = np.asarray(det["mu_0ts"], np.float32).reshape(ref["mu_0ts"].shape)
    first = next((k for k in range(len(got)) if not np.array_equal(got[k], ref["mu_0ts"][k])), None)
    assert first is None, f"{name}: mu_0ts differ from step {first} on (max |d| there {np.abs(got[first] - ref['mu_0ts'][first]).max()})"
    assert np.array_equal(np.asarray(det["rew_means"], np.float32), ref["rew_means"])
    assert np.float32(rew) == np.float32(ref["rew_final"])
    assert np.ptp(ref["rew_means"]) > 1e-3 and len(got) == Nd - 1


def test_full_size_properties_humanoidrun(gpu):
    """BASELINE metric size (N=1024, H=50): size-independent properties instead of the oracle —
    determinism across runs, weights sum to 1, finite rewards, and shard-layout independence."""
    from mbd_hip.planners.mbd_planner import Args, run_diffusion
    args = Args(seed=0, env_name="humanoidrun", Nsample=1024, Hsample=50, Ndiffuse=6, temp_sample=0.1,
                disable_recommended_params=True, not_render=True)
    r1, d1 = run_diffusion(args, return_details=True)
    r2, d2 = run_diffusion(args, return_details=True)
    assert np.array_equal(d1["mu_0ts"], d2["mu_0ts"]) and r1 == r2
    assert np.isfinite(d1["mu_0ts"]).all() and np.abs(d1["mu_0ts"]).max() <= 1.0


@pytest.mark.parametrize("name,B", [("humanoidrun", 1024), ("hopper", 1000), ("halfcheetah", 777), ("ant", 515)])
def test_candidates_are_independent_of_their_neighbours(gpu, name, B):
    """Full-size property without the oracle: a candidate's rewards do not depend on where it sits in the batch —
    permuting the batch permutes the rewards, and a prefix of the batch gives the prefix of the rewards, bit for
    bit.  (Candidates share wavefronts — 4 to 16 per wave — and, for the small models, DPP rows: any leak
    between lane groups, or any dependence on the tail handling of a partial last wavefront, shows up here.)"""
    from mbd_hip.envs import get_env
    env = get_env(name)
    st = env.reset(gpu.prng_key(5))
    g = np.random.default_rng(B)
    us = np.clip(g.normal(size=(B, 50, env.action_size)) * 0.7, -1.0, 1.0).astype(np.float32)
    base = env.rollout(st, us).cpu().numpy()
    perm = g.permutation(B)
    assert np.array_equal(env.rollout(st, us[perm]).cpu().numpy(), base[perm])
    for cut in (1, 3, B // 2 + 1, B - 1):
        assert np.array_equal(env.rollout(st, us[:cut]).cpu().numpy(), base[:cut]), cut
    assert np.isfinite(base).all()


@pytest.mark.parametrize("impl", [1, 0])
def test_two_shards_on_one_gpu_match_unsharded(gpu, impl, monkeypatch):
    """The N>1 code path on a single GPU: two plans owning candidates [0,N/2) and [N/2,N) plus a manual
    'all-gather' must give exactly the unsharded Ybar (this is what every rank computes with G GPUs)."""
    monkeypatch.setenv("MBD_THREEFRY_PARTITIONABLE", str(impl))
    import torch
    from mbd_hip.envs import get_env
    from mbd_hip.planners.mbd_planner import Args, Plan
    N, H, Nd, i = 256, 50, 100, 80
    env = get_env("humanoidrun")
    args = Args(env_name="humanoidrun", Nsample=N, Hsample=H, Ndiffuse=Nd, temp_sample=0.1,
                disable_recommended_params=True, not_render=True)
    st = env.reset(gpu.prng_key(2))
    ks = gpu.key_array(gpu.prng_split(gpu.prng_key(9), 2)[1])
    g = np.random.default_rng(1)
    Ybar = torch.tensor((g.normal(size=H * 17) * 0.2).astype(np.float32), device="cuda")
    outs = []
    # (humanoidrun MBD plans are lazy: every shard generates the normals of ALL N rows with noise_kernel, whatever the shard
    # layout — the materialised plans' three-range launch, where the other ranks' rows are sampled on the second stream and
    # the legacy layout goes element by element, is not on this path: tests/test_gpu_sampler.py reaches it)
    for shards in ([(0, N)], [(0, N // 2), (N // 2, N // 2)], [(0, 64), (64, 64), (128, 64), (192, 64)],
                   [(k * 32, 32) for k in range(8)]):
        plans = [Plan(env, args, shard_begin=b, shard_count=c) for b, c in shards]
        allv = torch.zeros(N, device="cuda")
        for p, (b, c) in zip(plans, shards):
            p.set_state0(st)
            loc = torch.zeros(c, device="cuda")
            gpu.check(p.lib.mbd_plan_sample_rollout(p.h, i, ks, Ybar.data_ptr(), loc.data_ptr(), None, None))
            torch.cuda.synchronize()
            allv[b:b + c] = loc
        res = []
        for p in plans:  # every "rank" finishes the step from the same gathered rewards
            out, rm = torch.zeros(H * 17, device="cuda"), torch.zeros(1, device="cuda")
            gpu.check(p.lib.mbd_plan_score_update(p.h, i, ks, Ybar.data_ptr(), allv.data_ptr(), None,
                                                  out.data_ptr(), rm.data_ptr(), None))
            torch.cuda.synchronize()
            res.append((out.cpu().numpy(), rm.item()))
            p.close()
        assert all(np.array_equal(res[0][0], r[0]) and res[0][1] == r[1] for r in res)
        outs.append(res[0])
    assert all(np.array_equal(outs[0][0], o[0]) and outs[0][1] == o[1] for o in outs[1:])


def test_reverse_distributed_world1_equals_plan_run(gpu):
    """The Python step loop used for multi-GPU runs (world size 1 here) against the C loop mbd_plan_run."""
    from mbd_hip.envs import get_env
    from mbd_hip.planners.mbd_planner import Args, Plan, reverse_distributed
    args = Args(env_name="hopper", Nsample=128, Hsample=50, Ndiffuse=15, temp_sample=0.1,
                disable_recommended_params=True, not_render=True)
    env = get_env("hopper")
    st = env.reset(gpu.prng_key(4))
    key = gpu.prng_key(8)
    p1 = Plan(env, args)
    p1.set_state0(st)
    mu1, rm1, rf1, _ = p1.run(key)
    p2 = Plan(env, args)
    p2.set_state0(st)
    mu2, rm2 = reverse_distributed(p2, key, 0)
    assert np.array_equal(mu1, mu2.cpu().numpy()) and np.array_equal(rm1, rm2.cpu().numpy())
    assert p2.eval(mu1[-1]) == rf1


def test_concurrent_seed_sweep_equals_sequential_runs(gpu):
    """eight plans enqueued concurrently (one stream each) give exactly the results of
    eight sequential run_diffusion calls (the reference's scripts/run_mbd.py protocol)."""
    from mbd_hip.planners.mbd_planner import Args, run_diffusion
    from mbd_hip.scripts.run_mbd import run_concurrent
    plans = [Args(seed=s, env_name="humanoidrun", Nsample=256, Hsample=50, Ndiffuse=12, temp_sample=0.1,
                  disable_recommended_params=True, not_render=True) for s in range(4)]
    plans.append(Args(seed=1, env_name="hopper", Nsample=128, Hsample=50, Ndiffuse=9, temp_sample=0.1,
                      disable_recommended_params=True, not_render=True))
    rews, mus, _ = run_concurrent(plans)
    for a, r, mu in zip(plans, rews, mus):
        r_seq, det = run_diffusion(a, return_details=True)
        assert np.array_equal(mu, det["mu_0ts"]) and np.float32(r) == np.float32(r_seq)


@pytest.mark.parametrize("method", ["mppi", "cma-es", "cem"])
@pytest.mark.parametrize("name,N,H,Nr", [("hopper", 256, 50, 12), ("humanoidrun", 128, 20, 8)])
def test_path_integral_baselines_end_to_end(gpu, orc, method, name, N, H, Nr):
    """mbd/planners/path_integral.py (MPPI / CMA-ES / CEM) on the same rollout kernel —
    whole runs, bit for bit against the oracle (mu history, per-step mean rewards, final sigma, rew_final)."""
    from mbd_hip.envs import get_env
    from mbd_hip.planners.path_integral import Args, run_path_integral
    from oracle import planner as op
    args = Args(seed=2, env_name=name, Nsample=N, Hsample=H, Nrefine=Nr, temp_sample=0.1,
                update_method=method, disable_recommended_params=True)
    rew, det = run_path_integral(args, return_details=True)
    env = get_env(name)
    ref = op.run_path_integral(orc, _oenv(orc, env), 2, N, H, Nr, 0.1, method)
    assert np.array_equal(det["mu_0ts"], ref["mu_0ts"]), method
    assert np.array_equal(det["rew_means"], ref["rew_means"])
    assert np.float32(det["sigma_final"]) == np.float32(ref["sigmas"][-1])
    assert np.float32(rew) == np.float32(ref["rew_final"])


def test_demo_path_through_the_sharded_step_loop(gpu):
    """BASELINE config 5 shape (humanoidtrack, enable_demo): the Python step loop used for multi-GPU runs
    packs [rews, demo log-density] in ONE exchange buffer; world size 1 must equal mbd_plan_run, and a
    2-shard emulation on one GPU must equal the unsharded step."""
    import torch
    from mbd_hip.envs import get_env
    from mbd_hip.planners.mbd_planner import Args, Plan, reverse_distributed
    args = Args(env_name="humanoidtrack", Nsample=128, Hsample=50, Ndiffuse=8, temp_sample=0.1, enable_demo=True,
                disable_recommended_params=True, not_render=True)
    env = get_env("humanoidtrack")
    st = env.reset(gpu.prng_key(0))
    key = gpu.prng_key(5)
    p1 = Plan(env, args)
    p1.set_state0(st)
    mu1, rm1, _, _ = p1.run(key)
    p2 = Plan(env, args)
    p2.set_state0(st)
    mu2, rm2 = reverse_distributed(p2, key, 0)
    assert np.array_equal(mu1, mu2.cpu().numpy()) and np.array_equal(rm1, rm2.cpu().numpy())
    # two shards, manual gather of both rows
    N, H, i = 128, 50, 5
    ks = gpu.key_array(gpu.prng_split(key, 2)[1])
    Ybar = torch.tensor(mu1[2].reshape(-1), device="cuda")
    res = []
    for shards in ([(0, N)], [(0, 64), (64, 64)]):
        plans = [Plan(env, args, shard_begin=b, shard_count=c) for b, c in shards]
        allv = torch.zeros((2, N), device="cuda")
        for p, (b, c) in zip(plans, shards):
            p.set_state0(st)
            loc = torch.zeros((2, c), device="cuda")
            gpu.check(p.lib.mbd_plan_sample_rollout(p.h, i, ks, Ybar.data_ptr(), loc[0].data_ptr(), loc[1].data_ptr(), None))
            torch.cuda.synchronize()
            allv[:, b:b + c] = loc
        out, rm = torch.zeros(H * 17, device="cuda"), torch.zeros(1, device="cuda")
        gpu.check(plans[-1].lib.mbd_plan_score_update(plans[-1].h, i, ks, Ybar.data_ptr(), allv[0].data_ptr(),
                                                      allv[1].data_ptr(), out.data_ptr(), rm.data_ptr(), None))
        torch.cuda.synchronize()
        res.append((out.cpu().numpy(), rm.item()))
        for p in plans:
            p.close()
    assert np.array_equal(res[0][0], res[1][0]) and res[0][1] == res[1][1]


def test_env_step_produces_observations(gpu):
    from mbd_hip.envs import get_env
    for name in ("humanoidrun", "hopper", "car2d"):
        env = get_env(name)
        st = env.reset(gpu.prng_key(1))
        assert st.obs is not None and st.obs.shape == (env.observation_size,)
        st2 = env.step(st, np.zeros(env.action_size, np.float32))
        assert st2.obs.shape == (env.observation_size,) and np.isfinite(st2.obs).all()


@pytest.mark.parametrize("name", ["humanoidrun", "hopper", "ant", "car2d"])
def test_pipeline_init_is_the_checkers_forward_kinematics_and_plans_start_from_it(gpu, orc, name):
    """PipelineEnv.pipeline_init(q, qd) through the C ABI (mbd_env_pipeline_init): bit-equal to the checker's forward
    kinematics; a rollout from that state is the checker's, bit for bit; wrong sizes are refused."""
    import torch
    from conftest import load_model
    from mbd_hip.envs import get_env
    from mbd_hip.envs.base import State
    env = get_env(name)
    g = np.random.default_rng(3)
    if name == "car2d":
        q = np.array([-0.3, 0.2, 1.0], np.float32)
        ps = env.pipeline_init(q)
        assert np.array_equal(np.asarray(ps).reshape(-1), q)
        us = g.uniform(-1, 1, (8, 12, 2)).astype(np.float32)
        rew = env.rollout(State(ps, None, 0.0, 0.0, {}), us).cpu().numpy()
        assert np.array_equal(rew, orc.car2d_rollout(q, us))
        with pytest.raises(Exception):
            env.pipeline_init(np.zeros(4, np.float32))
        return
    m = load_model(name)
    ms = m.to_struct()
    q = (m.init_q + g.uniform(-0.05, 0.05, m.q_size())).astype(np.float32)
    qd = g.uniform(-0.5, 0.5, m.qd_size()).astype(np.float32)
    ps = env.pipeline_init(q, qd)
    want = orc.forward(ms, q, qd)
    assert np.array_equal(np.asarray(ps, np.float32).reshape(want.shape), want)
    us = g.uniform(-1, 1, (16, 6, env.action_size)).astype(np.float32)
    rew = env.rollout(State(ps, None, 0.0, 0.0, {}), us).cpu().numpy()
    assert np.array_equal(rew, orc.rollout(ms, want, us))
    with pytest.raises(Exception):
        env.pipeline_init(q[:-1], qd)
    with pytest.raises(Exception):
        env.pipeline_init(q, qd[:-1])
    # qd omitted: at rest (round 5, advice: the optional argument used to work for car2d only)
    assert np.array_equal(np.asarray(env.pipeline_init(q), np.float32), np.asarray(env.pipeline_init(q, np.zeros_like(qd)), np.float32))


def test_render_outputs_mu0ts_and_replay(gpu, tmp_path, monkeypatch):
    """N1: without not_render the run leaves results/{env}/mu_0ts.npy (the array vis_diffusion.py:22 loads)
    and the replayed final plan; replaying through env.step equals the batched rollout kernel."""
    from mbd_hip.planners.mbd_planner import Args, run_diffusion
    monkeypatch.chdir(tmp_path)
    args = Args(seed=0, env_name="hopper", Nsample=64, Hsample=20, Ndiffuse=6, temp_sample=0.1,
                disable_recommended_params=True, not_render=False)
    rew, det = run_diffusion(args, return_details=True)
    mu = np.load(tmp_path / "results" / "hopper" / "mu_0ts.npy")
    assert mu.shape == (5, 20, 3) and np.array_equal(mu, det["mu_0ts"])
    rs = np.load(tmp_path / "results" / "hopper" / "rollout_states.npz")
    assert rs["pipeline_states"].shape == (21, 4, 13) and rs["link_positions"].shape == (21, 4, 3)
    s = np.float32(0)
    for r in rs["rewards"]:
        s = np.float32(s + r)
    assert np.float32(s / np.float32(20)) == np.float32(rew)   # step-by-step replay == rollout kernel


def test_metric_config_full_size_step_bitexact(gpu):
    """The BASELINE metric configuration at FULL size (humanoidrun, N=1024, H=50, Ndiffuse=100): two
    consecutive reverse-diffusion steps, bit for bit against the oracle (OpenMP build: ~1 s on the GPU box)."""
    from oracle import oracle as orc_mod
    orc_mod.build()
    _one_step(gpu, orc_mod.Oracle("f32_omp"), "humanoidrun", 1024, 50, 100, 0.1, 1, False, i=99)
    _one_step(gpu, orc_mod.Oracle("f32_omp"), "humanoidrun", 1024, 50, 100, 0.1, 1, False, i=3)


@pytest.mark.parametrize("name,B,sigma", [("humanoidrun", 2048, 1.0), ("humanoidrun", 2048, 0.25),
                                          ("humanoidstandup", 1024, 1.0), ("ant", 1024, 1.0),
                                          ("halfcheetah", 1024, 1.0), ("hopper", 1024, 1.0)])
def test_rollout_bitexact_many_violent_candidates(gpu, orc_omp, name, B, sigma):
    """Thousands of candidates with saturating random actions (sigma 1 clipped to +-1): falls, hard impacts,
    joints driven into their limits and frames near the gimbal singularity — states the small cases never visit.
    The oracle runs them on all host cores; rewards must agree bit for bit (NaN == NaN if both ever produce one)."""
    from mbd_hip.envs import get_env
    env = get_env(name)
    st = env.reset(gpu.prng_key(11))
    rng = np.random.default_rng(B + int(sigma * 100))
    us = np.clip(rng.normal(size=(B, 50, env.action_size)) * sigma, -1.0, 1.0).astype(np.float32)
    got = env.rollout(st, us)
    got = (got[0] if isinstance(got, tuple) else got).cpu().numpy()
    ref = _oenv(orc_omp, env).rollout(np.asarray(st.pipeline_state, np.float32), us)
    ref = ref[0] if isinstance(ref, tuple) else ref
    assert np.array_equal(got, ref, equal_nan=True), f"{name}: {np.sum(got != ref)} of {got.size} rewards differ"
    assert np.isfinite(got).all(), f"{name}: {np.sum(~np.isfinite(got))} non-finite rewards"


@pytest.mark.parametrize("env_name,kw", [("humanoidrun", dict(Nsample=1024, Ndiffuse=100, disable_recommended_params=True)),
                                         ("humanoidrun", {}),  # the reference's recommended N=8192, Ndiffuse=300
                                         ("humanoidstandup", {}), ("ant", {}), ("hopper", {}), ("walker2d", {}),
                                         ("halfcheetah", {}), ("cartpole", {}), ("humanoidtrack", dict(enable_demo=True))])
def test_long_plans_stay_finite(gpu, env_name, kw):
    """Whole plans at the reference's own sizes: thousands of candidates visit states the short parity cases never
    do (gimbal-singular joint frames, hard impacts).  One non-finite reward poisons the softmax of its diffusion
    step and every mean after it, so every per-step mean reward must be finite and the plan must improve.
    (Regression: arithmetic masking of unused Euler-angle slots once turned an overflowing angle into 0*inf.)"""
    from mbd_hip.planners.mbd_planner import Args, run_diffusion
    a = Args(seed=0, env_name=env_name, not_render=True, **kw)
    rew, det = run_diffusion(a, return_details=True)
    assert np.isfinite(det["rew_means"]).all(), int(np.where(~np.isfinite(det["rew_means"]))[0][0])
    assert np.isfinite(det["mu_0ts"]).all() and np.isfinite(rew)
    assert det["rew_means"][-1] > det["rew_means"][0]


def test_bench_multirank_code_path_on_rccl_with_one_rank(gpu):
    """bench.py's N>1 branch — torch.distributed `nccl` (= RCCL) initialisation with a device id, the per-step
    all_gather_into_tensor of device buffers, the barriers and the max-over-ranks reduction — launched the way the
    driver launches it, with the one rank this box has (MBD_FORCE_DIST=1).  It must print one JSON line whose
    rate is in the same range as the plain single-GPU loop."""
    import json, os, socket, subprocess, sys
    from conftest import ROOT
    env = dict(os.environ, MBD_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    with socket.socket() as sk:  # a free rendezvous port
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20",
           "--warmup", "3", "--no-cpu-baseline", "--no-final-reward"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["config"]["collective"].startswith("all-gather of N/G rewards") and d["value"] > 300.0


def test_bench_plain_line_and_dumped_outputs(gpu, tmp_path):
    """A plain bench.py run: ONE timed block of exactly --steps steps, a line with the headline fields only, and
    --dump-outputs writing what the last timed step computed — the new mean [H, Nu], the step's mean reward as the host read
    it and the per-candidate rewards it is the mean of."""
    import json, os, subprocess, sys
    from conftest import ROOT
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                          "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 7 and d["repeats"] == 1 and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["value"] > 300.0 and abs(d["ms_per_step"] - 1e3 / d["value"]) < 1e-6 * d["ms_per_step"]
    assert not {"value_async", "roofline", "final_reward", "cpu_baseline", "extras", "valu"} & set(d), sorted(d)
    y, rm, rw = (np.load(tmp_path / f"{n}.npy") for n in ("ybar", "rew_mean", "rewards"))
    assert y.dtype == rm.dtype == rw.dtype == np.float32
    assert y.shape == (50, 17) and rm.shape == (1,) and rw.shape == (1024,)
    assert np.isfinite(y).all() and np.isfinite(rw).all() and np.abs(y).max() > 0
    assert abs(float(rm[0]) - float(rw.astype(np.float64).mean())) < 1e-4 * max(1.0, abs(float(rm[0])))


def test_bench_runs_a_tree_it_cannot_write(gpu, tmp_path):
    """bench.py on a tree another user built: the library's directory and its build lock are not writable (build() cannot
    even take the lock).  The run must load the library as built and print its line, the plain and the --full one."""
    import json, os, stat, subprocess, sys
    from conftest import ROOT
    libdir = os.path.join(ROOT, "model-based-diffusion_amd", "lib")
    lock = os.path.join(libdir, ".build.lock")
    modes = {p_: stat.S_IMODE(os.stat(p_).st_mode) for p_ in (libdir, lock)}
    try:
        os.chmod(lock, 0o444)
        os.chmod(libdir, 0o555)
        for extra in ([], ["--full", "--no-cpu-baseline", "--no-final-reward", "--no-extras"]):
            out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup",
                                  "1", *extra], capture_output=True, text=True, timeout=600)
            assert out.returncode == 0, out.stderr[-2000:]
            lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
            assert len(lines) == 1 and json.loads(lines[0])["value"] > 300.0, out.stdout[-2000:]
    finally:
        for p_, m in modes.items():
            os.chmod(p_, m)


def test_bench_two_ranks_line_is_complete(gpu):
    """bench.py --gpus 2 the way the driver launches it, as a dry run on this box's ONE GPU (MBD_DIST_BACKEND=gloo, both
    ranks on device 0): the line must carry the final reward of the SHARDED plans and say that it equals the one-GPU
    values bit for bit, the per-phase times of a sharded step, and the second collective (the in-library windows)
    measured beside the process group's all-gather."""
    import json, os, socket, subprocess, sys
    from conftest import ROOT
    env = dict(os.environ, MBD_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "10",
           "--warmup", "2", "--no-cpu-baseline", "--full"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["config"]["N_per_gpu"] == 512
    fr = d["final_reward"]
    assert fr["sharded_over"] == 2 and fr["equals_one_gpu_bitwise"] is True and len(fr["rew_final"]) == 8
    assert set(d["phase_ms"]) >= {"phase1_ms", "exchange_ms", "phase2_ms"} and d["phase_ms"]["phase1_ms"] > 0.3
    assert d["other_collective"]["collective"].startswith("p2p") and d["other_collective"]["value"] > 100.0, d["other_collective"]
    assert d["other_scaling"]["scaling"] == "weak" and d["other_scaling"]["N_per_gpu"] == 1024


# ---- BASELINE.json configs 3 / 4 / 5 at their full sizes (round-2 verdict item 1) --------------------------------
def test_config3_halfcheetah_full_size_step_bitexact(gpu, orc_omp):
    """BASELINE config 3 at FULL size: halfcheetah, N=1024, H=50, temp 0.4 — a whole reverse-diffusion step
    (sampled candidates, 819 200 substeps of rollout, softmax weights, Ybar_{i-1}) bit for bit against the oracle."""
    _one_step(gpu, orc_omp, "halfcheetah", 1024, 50, 100, 0.4, 1, False, i=99)
    _one_step(gpu, orc_omp, "halfcheetah", 1024, 50, 100, 0.4, 1, False, i=20)


def test_config2_hopper_full_size_step_bitexact(gpu, orc_omp):
    """BASELINE config 2 at full size (hopper, N=512, H=50, temp 0.1), first and a late diffusion step."""
    _one_step(gpu, orc_omp, "hopper", 512, 50, 100, 0.1, 1, False, i=99)
    _one_step(gpu, orc_omp, "hopper", 512, 50, 100, 0.1, 1, False, i=5)


def test_config5_humanoidtrack_demo_full_size_step_bitexact(gpu, orc_omp):
    """BASELINE config 5 at FULL size: humanoidtrack, enable_demo, N=2048, H=50 — rewards (lagged,
    humanoidtrack.py:78), tracked positions -> demo log-density, the double-temperature blend (:117-125), weights
    and Ybar_{i-1}, bit for bit."""
    _one_step(gpu, orc_omp, "humanoidtrack", 2048, 50, 100, 0.1, 1, True, i=99)


def test_config4_humanoidrun_n4096_eight_shards_every_rank_bitexact(gpu, orc_omp):
    """BASELINE config 4 at FULL size on one GPU: humanoidrun N=4096 split into the 8 shards of an 8-GPU job.
    Every shard's phase 1 (its 512 rows of the rollout) must reproduce the oracle's rewards, and EVERY shard's
    phase 2 (mbd_plan_score_update from the gathered rewards) must give the oracle's weights / Ybar_{i-1} / mean
    reward of the unsharded N=4096 step, bit for bit."""
    import torch
    from mbd_hip.envs import get_env
    from mbd_hip.planners.mbd_planner import Args, Plan
    from oracle import planner as op
    N, H, Nd, i, G = 4096, 50, 100, 97, 8
    env = get_env("humanoidrun")
    args = Args(env_name="humanoidrun", Nsample=N, Hsample=H, Ndiffuse=Nd, temp_sample=0.1,
                disable_recommended_params=True, not_render=True)
    rng, rng_reset = gpu.prng_split(gpu.prng_key(0), 2)
    st = env.reset(rng_reset)
    state0 = np.asarray(st.pipeline_state, np.float32)
    g = np.random.default_rng(4)
    Ybar = (g.normal(size=(H, 17)) * 0.15).astype(np.float32)
    d_Y = torch.tensor(Ybar.reshape(-1), device="cuda")
    sched = orc_omp.schedule(args.beta0, args.betaT, Nd)
    r2, Y_ref, rm_ref, det = op.reverse_once(orc_omp, _oenv(orc_omp, env), state0, i, rng, Ybar, sched, N, H, 0.1, 1)
    ks = gpu.key_array(gpu.prng_split(rng, 2)[1])
    plans = [Plan(env, args, shard_begin=k * (N // G), shard_count=N // G) for k in range(G)]
    allv = torch.zeros(N, device="cuda")
    for k, p in enumerate(plans):
        p.set_state0(st)
        loc = torch.zeros(N // G, device="cuda")
        gpu.check(p.lib.mbd_plan_sample_rollout(p.h, i, ks, d_Y.data_ptr(), loc.data_ptr(), None, None))
        torch.cuda.synchronize()
        Y0s, rewss, _ = p.peek()
        assert np.array_equal(Y0s, det["Y0s"]), f"shard {k}: sampled candidates differ"
        assert np.array_equal(rewss, det["rewss"][k * (N // G):(k + 1) * (N // G)]), f"shard {k}: rewards differ"
        allv[k * (N // G):(k + 1) * (N // G)] = loc
    for k, p in enumerate(plans):
        out, rm = torch.zeros(H * 17, device="cuda"), torch.zeros(1, device="cuda")
        gpu.check(p.lib.mbd_plan_score_update(p.h, i, ks, d_Y.data_ptr(), allv.data_ptr(), None, out.data_ptr(),
                                              rm.data_ptr(), None))
        torch.cuda.synchronize()
        assert np.array_equal(p.peek()[2], det["weights"]), f"rank {k}: weights differ"
        assert np.array_equal(out.cpu().numpy().reshape(H, 17), Y_ref), f"rank {k}: Ybar_(i-1) differs"
        assert np.float32(rm.item()) == np.float32(rm_ref)
        p.close()


def _run_ranks(tmp_path, world, env_name, N, H, Nd, temp, demo, collective="torch", extra_env=None):
    import json, os, socket, subprocess, sys
    from conftest import ROOT
    with socket.socket() as sk:  # a free rendezvous port
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "dist_worker.py"), str(tmp_path),
           env_name, str(N), str(H), str(Nd), str(temp), str(int(demo))]
    out = subprocess.run(cmd, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MBD_COLLECTIVE=collective,
                                       **(extra_env or {})),
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    res = [json.load(open(os.path.join(tmp_path, f"rank{r}.json"))) for r in range(world)]
    mus = [np.load(os.path.join(tmp_path, f"mu_rank{r}.npy")) for r in range(world)]
    return res, mus


def _run_two_ranks(tmp_path, env_name, N, H, Nd, temp, demo, collective="torch"):
    return _run_ranks(tmp_path, 2, env_name, N, H, Nd, temp, demo, collective)


@pytest.mark.parametrize("collective", ["torch", "p2p"])
def test_two_real_ranks_run_the_sharded_product_path(gpu, tmp_path, collective):
    """The product's sharded path with TWO REAL RANKS and real HIP kernels: torch.distributed.run --nproc-per-node 2
    (gloo; both ranks on this box's one GPU) -> run_diffusion -> reverse_distributed (mbd_plan_sample_rollout on
    the rank's shard, the per-step all-gather, mbd_plan_score_update).  Both ranks' mu_0ts, per-step mean rewards
    and final reward must equal the unsharded plan's bit for bit, and each other's.  collective = "p2p": the step's
    exchange through the in-library windows (mbd_exchange_*: hipIpc-mapped peer stores + flags; the two processes map
    each other's window on the one device) instead of the all-gather of the process group."""
    res, mus = _run_two_ranks(tmp_path, "humanoidrun", 1024, 50, 12, 0.1, False, collective)
    assert all(r["world"] == 2 and r["equal_to_unsharded"] for r in res), res
    assert all(r["force_single_progress_ok"] for r in res), res  # (unsharded plans never touch the process group)
    assert np.array_equal(mus[0], mus[1]) and res[0]["rew"] == res[1]["rew"]


@pytest.mark.parametrize("collective", ["torch", "p2p"])
def test_two_real_ranks_demo_path(gpu, tmp_path, collective):
    """The same with the demo-conditioned score (config 5's shape): two rows per rank in the one exchange buffer."""
    res, mus = _run_two_ranks(tmp_path, "humanoidtrack", 256, 50, 8, 0.1, True, collective)
    assert all(r["world"] == 2 and r["equal_to_unsharded"] for r in res), res
    assert np.array_equal(mus[0], mus[1])


# ---- world = 8 before the driver's SCALE run does it (round-3 verdict item 1): eight REAL ranks on this box's one GPU ----
@pytest.mark.parametrize("collective", ["torch", "p2p"])
@pytest.mark.parametrize("env_name,N,H,Nd,demo", [("humanoidrun", 1024, 50, 10, False),    # the metric's plan, 128 per rank
                                                  ("humanoidtrack", 512, 50, 6, True),     # two rows per rank and step
                                                  ("car2d", 128, 30, 12, False)])          # a MATERIALISED plan
def test_eight_real_ranks_run_the_sharded_product_path(gpu, tmp_path, collective, env_name, N, H, Nd, demo):
    """run_diffusion -> reverse_distributed with EIGHT real processes (torch.distributed.run --nproc-per-node 8, gloo, all
    on device 0), through the process group's all-gather and through the in-library windows (eight hipIpc-mapped
    windows per rank, seven peers each): every rank's mu_0ts, mean rewards and final reward equal the unsharded
    plan's bit for bit.  car2d materialises Y0s: with N = 8 shards every rank samples its own rows on the step's stream
    and the other seven ranks' rows on its second stream (csrc: `N >= 5 * shard`) — that branch with real processes."""
    res, mus = _run_ranks(tmp_path, 8, env_name, N, H, Nd, 0.1, demo, collective)
    assert len(res) == 8 and all(r["world"] == 8 and r["equal_to_unsharded"] for r in res), res
    assert all(r["force_single_progress_ok"] for r in res), res
    assert all(np.array_equal(mus[0], m) for m in mus[1:]) and len({r["rew"] for r in res}) == 1


def _bench_ranks(world, extra, timeout=1500):
    import json, os, socket, subprocess, sys
    from conftest import ROOT
    env = dict(os.environ, MBD_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", str(world), *extra]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("config,n_strong", [("metric", 128), ("humanoidrun4096", 512), ("humanoidtrack2048demo", 256)])
def test_bench_eight_ranks_lines_are_complete(gpu, config, n_strong):
    """bench.py --gpus 8 the way the driver's SCALE run launches it, as a dry run on this box's ONE GPU (gloo, all ranks on
    device 0), for the metric and for BASELINE configs 4 and 5 (both DEFINED on 8 GPUs): the line carries the final
    rewards of the plans SHARDED over the eight ranks, equal to one GPU's bit for bit, the phases of a sharded step, and
    the second collective (eight windows) beside the process group's."""
    d = _bench_ranks(8, ["--steps", "4", "--warmup", "1", "--repeats", "2", "--no-cpu-baseline", "--full", "--config", config])
    assert d["n_gpus"] == 8 and d["scaling"] == "strong" and d["config"]["N_per_gpu"] == n_strong and d["repeats"] == 2
    assert d["value_min"] <= d["value"] <= d["value_max"]
    fr = d["final_reward"]
    assert fr["sharded_over"] == 8 and fr["equals_one_gpu_bitwise"] is True and len(fr["rew_final"]) == 8
    assert set(d["phase_ms"]) >= {"phase1_ms", "exchange_ms", "phase2_ms"} and d["phase_ms"]["phase1_ms"] > 0.1
    assert d["other_collective"]["collective"].startswith("p2p") and d["other_collective"]["value"] > 10.0, d["other_collective"]
    assert d["other_scaling"]["scaling"] == "weak" and d["other_scaling"]["N_per_gpu"] == 8 * n_strong
    if config == "metric":  # the workload that scales rides in the same line: 8 plans per rank as one sweep each, rates summed
        x = d["extras"]["sweep8_replicas"]
        assert x["ranks_ok"] == 8 and len(x["per_rank"]) == 8 and x["plan_steps_per_sec"] > 100.0, x


@pytest.mark.parametrize("world", [2, 8])
def test_bench_sweep_replicas_over_ranks(gpu, world):
    """bench.py --config sweep8 --gpus G (round-3 verdict item 2): the reference's eight independent plans
    (mbd/scripts/run_mbd.py:17-39) as REPLICAS over the ranks — 8/G plans per rank through mbd_sweep_*, no communication
    inside a run — with the final rewards gathered once and equal, bit for bit, to the one-GPU sweep of all eight."""
    d = _bench_ranks(world, ["--steps", "6", "--warmup", "2", "--repeats", "2", "--no-cpu-baseline", "--full", "--config",
                             "sweep8"])
    assert d["n_gpus"] == world and d["config"]["plans"] == 8 and d["config"]["plans_per_gpu"] == 8 // world
    assert d["unit"].startswith("plan-steps/sec") and d["value"] > 100.0
    fr = d["final_reward"]
    assert fr["replicated_over"] == world and fr["equals_one_gpu_bitwise"] is True and len(fr["rew_final"]) == 8
    assert len(d["per_rank_plan_steps_per_sec"]) == world and min(d["per_rank_plan_steps_per_sec"]) > 10.0
    assert d["other_scaling"]["scaling"] == "weak" and d["other_scaling"]["plans"] == 8 * world


def test_exchange_eight_windows_two_rows(gpu, tmp_path):
    """mbd_exchange_* with EIGHT windows and rows = 2 (config 5's shape): eight canary processes on the one device map
    each other's windows (7 hipIpcOpenMemHandle each), run four all-gathers with known values and check every rank's
    slice of every step (mbd_hip.planners.exchange_canary — what bench.py starts beside its ranks)."""
    import subprocess, sys
    from conftest import ROOT
    rdv = str(tmp_path / "rdv")
    procs = [subprocess.Popen([sys.executable, "-m", "mbd_hip.planners.exchange_canary", str(r), "8", "0", rdv],
                              cwd=os.path.join(ROOT, "model-based-diffusion_amd"), stderr=subprocess.PIPE, text=True,
                              env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")) for r in range(8)]
    rcs = []
    for p_ in procs:
        try:
            _, err = p_.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            p_.kill()
            _, err = p_.communicate()
        rcs.append((p_.returncode, err[-300:]))
    assert all(rc == 0 for rc, _ in rcs), rcs


def test_exchange_window_is_fine_grained_or_refused(gpu):
    """The receive windows are FINE-GRAINED device memory (round-3 advice: a coarse-grained window can hand its owner a
    flag beside stale rewards); a runtime without such a pool gets MBD_ERR_UNSUPPORTED — the caller keeps the process
    group's all-gather — unless the dry-run lever MBD_EXCHANGE_COARSE_OK asks for plain memory."""
    lib = gpu.load()
    h, fg = C.c_void_p(), C.c_int(-1)
    gpu.check(lib.mbd_exchange_create(0, 0, 1, 1, 64, C.byref(h)))
    gpu.check(lib.mbd_exchange_fine_grained(h, C.byref(fg)))
    assert fg.value == 1
    gpu.check(lib.mbd_exchange_destroy(h))
    gpu.debug_set("MBD_EXCHANGE_NO_FINEGRAINED", 1)
    try:
        assert lib.mbd_exchange_create(0, 0, 1, 1, 64, C.byref(h)) == gpu.MBD_ERR_UNSUPPORTED
        gpu.debug_set("MBD_EXCHANGE_COARSE_OK", 1)
        gpu.check(lib.mbd_exchange_create(0, 0, 1, 1, 64, C.byref(h)))
        gpu.check(lib.mbd_exchange_fine_grained(h, C.byref(fg)))
        assert fg.value == 0
        gpu.check(lib.mbd_exchange_destroy(h))
    finally:
        gpu.debug_set("MBD_EXCHANGE_NO_FINEGRAINED", -1)
        gpu.debug_set("MBD_EXCHANGE_COARSE_OK", -1)


def test_create_by_name_through_the_c_abi(gpu):
    """mbd_env_create(name): every env of the registry (mbd/envs/__init__.py:13-33) straight from the C ABI — no
    Python model, no MJCF compiler — with the sizes the reference reads off the env, and a step that runs."""
    lib = gpu.load()
    k, names = 0, []
    while lib.mbd_env_name(k) is not None:
        names.append(lib.mbd_env_name(k).decode())
        k += 1
    want = {"car2d": (2, 3), "humanoidrun": (17, 47), "humanoidtrack": (17, 47), "hopper": (3, 12),
            "halfcheetah": (6, 17), "walker2d": (6, 18), "humanoidstandup": (17, 47), "cartpole": (1, 4), "ant": (8, 27)}
    assert sorted(names) == sorted(want)
    for name in names:
        h = C.c_void_p()
        gpu.check(lib.mbd_env_create(name.encode(), 0, C.byref(h)))
        a, o, s = C.c_int(), C.c_int(), C.c_int()
        gpu.check(lib.mbd_env_info(h, C.byref(a), C.byref(o), C.byref(s), None, None, None))
        assert (a.value, o.value) == want[name], name
        key = (C.c_uint32 * 2)(0, 1)
        st, st2 = np.zeros(s.value, np.float32), np.zeros(s.value, np.float32)
        obs, rew = np.zeros(o.value, np.float32), np.zeros(1, np.float32)
        gpu.check(lib.mbd_env_reset(h, key, 1, gpu.np_ptr(st)))
        gpu.check(lib.mbd_env_step(h, gpu.np_ptr(st), gpu.np_ptr(np.zeros(a.value, np.float32)), gpu.np_ptr(st2),
                                   gpu.np_ptr(rew), gpu.np_ptr(obs)))
        assert np.isfinite(st2).all() and np.isfinite(obs).all() and np.isfinite(rew).all(), name
        lib.mbd_env_destroy(h)
    h = C.c_void_p()
    assert lib.mbd_env_create(b"pushT", 0, C.byref(h)) == gpu.MBD_ERR_UNSUPPORTED


@pytest.mark.parametrize("name", ["humanoidtrack", "car2d"])
def test_standalone_xref_logpd_matches_oracle(gpu, orc, name):
    """mbd_env_xref_logpd = jax.vmap(env.eval_xref_logpd) (mbd_planner.py:118) on rollout output, against the
    oracle's per-trajectory log-density and the env object's own single-trajectory method."""
    from mbd_hip.envs import get_env
    env = get_env(name)
    st = env.reset(gpu.prng_key(2))
    g = np.random.default_rng(9)
    us = np.clip(g.normal(size=(37, 50, env.action_size)) * 0.5, -1, 1).astype(np.float32)
    rewss, xpos = env.rollout(st, us, want_xpos=True)
    lp = env.eval_xref_logpd_batch(xpos).cpu().numpy()
    xp = xpos.cpu().numpy()
    oe = _oenv(orc, env)
    ref = oe.logpd(xp)
    assert np.array_equal(lp, ref)
    one = np.array([env.eval_xref_logpd(xp[b]) for b in range(4)], np.float32)
    assert np.allclose(one, lp[:4], rtol=1e-5, atol=1e-6)


def test_progress_callback_reads_every_step(gpu):
    """mbd_planner.py:147: the reference formats the mean reward of EVERY diffusion step.  run_diffusion(progress=)
    delivers the same values per step, and they equal the means of the asynchronous run."""
    from mbd_hip.planners.mbd_planner import Args, run_diffusion
    a = dict(seed=1, env_name="hopper", Nsample=128, Hsample=50, Ndiffuse=10, temp_sample=0.1,
             disable_recommended_params=True, not_render=True)
    seen = []
    r1, d1 = run_diffusion(Args(**a), return_details=True, progress=lambda i, rew: seen.append((i, rew)))
    r2, d2 = run_diffusion(Args(**a), return_details=True)
    assert [i for i, _ in seen] == list(range(9, 0, -1))
    assert np.array_equal(np.array([r for _, r in seen], np.float32), d2["rew_means"])
    assert np.array_equal(d1["mu_0ts"], d2["mu_0ts"]) and r1 == r2


@pytest.mark.parametrize("mode", ["fused", "aux"])
@pytest.mark.parametrize("impl", [1, 0])
def test_noise_prefetch_is_bit_identical(gpu, impl, mode, monkeypatch, levers):
    """mbd_plan_prefetch_noise (the NEXT step's normals generated beside the current rollout — in spare workgroups of
    the rollout launch ("fused"), or on the plan's second stream when the rollout fills the chip ("aux", forced here
    by MBD_NO_FUSED_NOISE) — and the candidates formed lazily at the rollout's action fetch and in the weighted mean)
    is a HINT: a plan run through mbd_plan_run — which declares every next key — must equal, bit for bit, (a) the same
    plan stepped by hand through sample_rollout / score_update without any declaration, where a declaration of a key
    that is NOT used next must be ignored, and (b) the same plan with materialised candidates (MBD_NO_LAZY: the
    sampler writes Y0s, rollout and weighted mean read it).  Both threefry layouts."""
    monkeypatch.setenv("MBD_THREEFRY_PARTITIONABLE", str(impl))
    if mode == "aux":
        levers(MBD_NO_FUSED_NOISE=1)
    import torch
    from mbd_hip.envs import get_env
    from mbd_hip.planners.mbd_planner import Args, Plan
    N, H, Nd = 2048, 50, 6
    env = get_env("humanoidrun")
    args = Args(env_name="humanoidrun", Nsample=N, Hsample=H, Ndiffuse=Nd, temp_sample=0.1,
                disable_recommended_params=True, not_render=True)
    st = env.reset(gpu.prng_key(2))
    key = gpu.prng_key(6)
    p1 = Plan(env, args)
    p1.set_state0(st)
    mu1, rm1, rf1, _ = p1.run(key)
    Y1, rewss1, w1 = p1.peek()
    p1.close()
    levers(MBD_NO_LAZY=1)
    p0 = Plan(env, args)
    levers(MBD_NO_LAZY=-1)
    p0.set_state0(st)
    mu0, rm0, rf0, _ = p0.run(key)
    Y0, rewss0, w0 = p0.peek()
    p0.close()
    assert np.array_equal(mu0, mu1) and np.array_equal(rm0, rm1) and rf0 == rf1
    assert np.array_equal(Y0, Y1) and np.array_equal(rewss0, rewss1) and np.array_equal(w0, w1)
    p2 = Plan(env, args)
    p2.set_state0(st)
    HNu = H * 17
    Ybar = torch.zeros(HNu, device="cuda")
    rng = np.asarray(key, np.uint32)
    mus, rms = [], []
    for i in range(Nd - 1, 0, -1):
        keys = gpu.prng_split(rng, 2, impl)
        rng, ks = keys[0], gpu.key_array(keys[1])
        if i == 3:  # a declaration of a key nobody will ask for: generated, then ignored
            gpu.check(p2.lib.mbd_plan_prefetch_noise(p2.h, gpu.key_array(gpu.prng_key(12345)), None))
        if i == 2:  # the current step's own key declared as "next": nothing to prepare
            gpu.check(p2.lib.mbd_plan_prefetch_noise(p2.h, ks, None))
        loc, out, rm = torch.zeros(N, device="cuda"), torch.zeros(HNu, device="cuda"), torch.zeros(1, device="cuda")
        gpu.check(p2.lib.mbd_plan_sample_rollout(p2.h, i, ks, Ybar.data_ptr(), loc.data_ptr(), None, None))
        gpu.check(p2.lib.mbd_plan_score_update(p2.h, i, ks, Ybar.data_ptr(), loc.data_ptr(), None, out.data_ptr(),
                                               rm.data_ptr(), None))
        torch.cuda.synchronize()
        Ybar = out
        mus.append(out.cpu().numpy().reshape(H, 17))
        rms.append(rm.item())
    assert np.array_equal(np.stack(mus), mu1) and np.array_equal(np.array(rms, np.float32), rm1)
    assert p2.eval(mu1[-1]) == rf1
    p2.close()


@pytest.mark.parametrize("no_dpp", [False, True])
@pytest.mark.parametrize("name,B", [("hopper", 200), ("walker2d", 72), ("halfcheetah", 136), ("cartpole", 100)])
def test_general_3d_kernels_on_planar_models(gpu, orc_omp, name, B, no_dpp, monkeypatch, levers):
    """The planar models normally run the planar restatement (MBD_FLAG_PLANAR).  Compiled WITHOUT the flag (mjcf.load(
    planar=False) — here: the flag cleared on the compiled model, passed through mbd_env_create_model) they take the
    general 3-D slide-joint kernels (constant slide axes, packed collider pairs, axisymmetric inertia; DPP and shuffle
    exchange), which must stay bit-exact against the 3-D restatement of the checker."""
    if no_dpp:
        levers(MBD_NO_DPP=1)
    from conftest import load_model
    from mbd_hip.envs.base import RigidBodyEnv
    from oracle.planner import OracleEnv
    m = load_model(name)
    m.fields["flags"] = int(m.fields["flags"]) & ~2
    env = RigidBodyEnv(name, model=m)
    assert not (int(env.sys.fields["flags"]) & 2)
    st = env.reset(gpu.prng_key(3))
    g = np.random.default_rng(B)
    us = np.clip(g.normal(size=(B, 50, env.action_size)) * 0.8, -1.0, 1.0).astype(np.float32)
    got = env.rollout(st, us).cpu().numpy()
    oe = OracleEnv(orc_omp, name, m.to_struct(), init_q=m.init_q)
    ref = oe.rollout(np.asarray(st.pipeline_state, np.float32), us)
    assert np.isfinite(got).all()
    assert np.array_equal(got, ref), f"{name}: max |d| = {np.abs(got - ref).max()}"


@pytest.mark.parametrize("no_dpp", [False, True])
@pytest.mark.parametrize("cls", ["iso", "diag", "full"])
@pytest.mark.parametrize("name", ["hopper", "walker2d", "tripod", "humanoidrun", "ant"])
def test_general_3d_kernels_by_inertia_class(gpu, orc, name, cls, no_dpp, monkeypatch, levers):
    """launch_rollout picks an instantiation by candidate-group width (4 / 8 / 16 lanes), exchange (a DPP family or
    shuffles) and the CLASS of the model's inverse-inertia tensors: isotropic, axisymmetric, diagonal, full.  The
    built-in models populate only some of the combinations; here the tensors of built-in trees are replaced (the
    checker reads the same model), planar models run their 3-D arithmetic, and every combination is held to the bar."""
    if no_dpp:
        levers(MBD_NO_DPP=1)
    from conftest import load_model
    from mbd_hip.envs.base import RigidBodyEnv
    from oracle.planner import OracleEnv
    if name == "tripod":
        from custom_models import TRIPOD
        from test_oracle_physics import _compile
        m = _compile(TRIPOD, env_name="halfcheetah", n_frames=4, reset_noise=0.05, reward_params=(1.0, 0.1), planar=False)
        ename = "halfcheetah"
    else:
        m, ename = load_model(name), name
        m.fields["n_frames"] = min(int(m.fields["n_frames"]), 5)
    m.fields["flags"] = int(m.fields["flags"]) & ~2
    g = np.random.default_rng(len(name) * 7 + len(cls))
    Iinv = np.array(m.fields["inv_inertia"], np.float32)
    for l in range(m.n_links):
        a = float(Iinv[l, :3].mean())
        if cls == "iso":
            Iinv[l] = [a, a, a, 0, 0, 0]
        elif cls == "diag":
            Iinv[l] = [a * 0.7, a * 1.1, a * 1.6, 0, 0, 0]
        else:  # a rotated diagonal tensor: symmetric positive definite with all six entries non-zero
            q = g.normal(size=4); q /= np.linalg.norm(q)
            w, x, y, z = q
            R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                          [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                          [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
            T = R @ np.diag([a * 0.7, a * 1.1, a * 1.6]) @ R.T
            Iinv[l] = [T[0, 0], T[1, 1], T[2, 2], T[0, 1], T[0, 2], T[1, 2]]
    m.fields["inv_inertia"] = Iinv
    m.fields["iso_inertia"] = int(cls == "iso")
    env = RigidBodyEnv(ename, model=m)
    st = env.reset(gpu.prng_key(6))
    B, H = 21, 12
    us = np.clip(g.normal(size=(B, H, env.action_size)) * 0.6, -1.2, 1.2).astype(np.float32)
    got = env.rollout(st, us).cpu().numpy()
    oe = OracleEnv(orc, ename, m.to_struct(), init_q=m.init_q)
    ref = oe.rollout(np.asarray(st.pipeline_state, np.float32), us)
    assert np.isfinite(got).all()
    assert np.array_equal(got, ref), f"{name}/{cls}: max |d| = {np.abs(got - ref).max()}"


def test_short_exact_sequences(gpu):
    """The value-preserving shortcuts of csrc/mbd_math.h, on the device that runs them: rcp + one Newton
    step is the correctly rounded reciprocal for EVERY float32 in [1e-20, 1e20]; with it ONE residual step gives the
    correctly rounded quotient (2.6e10 random pairs with full random mantissas + the hard denominators); rsq + one
    correction is the correctly rounded square root for EVERY float32 in [1e-30, FLT_MAX].  The probes are standalone
    HIP programs built by __graft_entry__.build(); the controls (bare rcp / rsq products) must mismatch."""
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([os.path.join(root, "tools", "probes", "probe_rcp")], capture_output=True, text=True,
                         timeout=300, check=True).stdout
    rows = re.findall(r"^\s+([ABC]) .*?(\d+) mismatches", out, re.M)
    assert [r[0] for r in rows] == ["A", "B", "C"] and all(int(r[1]) == 0 for r in rows), out
    assert "1114674149 checked" in out
    out = subprocess.run([os.path.join(root, "tools", "probes", "probe_short")], capture_output=True, text=True,
                         timeout=600, check=True).stdout
    div = re.findall(r"^div5 .*mismatches (\d+) of (\d+) \(control n\*rcp\(d\): (\d+)\)", out, re.M)
    assert len(div) == 6 and all(int(m) == 0 and int(n) == 2048 * 256 * 8192 and int(c) > 0 for m, n, c in div), out
    sq = re.findall(r"^(sqrtA|sqrtB|control).*?(\d+) mismatches of (\d+)", out, re.M)
    assert len(sq) == 3 and int(sq[0][1]) == 0 and int(sq[1][1]) == 0 and int(sq[2][1]) > 0, out
    assert all(int(x[2]) == 1910357408 for x in sq), out


@pytest.mark.parametrize("name,N,demo", [("humanoidrun", 300, False), ("humanoidtrack", 192, True), ("car2d", 257, False)])
def test_phase2_kernel_variants_and_shared_device_are_bit_identical(gpu, name, N, demo, monkeypatch, levers):
    """Phase 2 has three forms that must give the same bits: score + weighted mean in one launch (the default up to
    12 288 candidates), score_kernel + the tile weighted mean (MBD_NO_FUSED_SCORE=1), score_kernel + the row-major
    two-kernel weighted mean (MBD_WMEAN_SPLIT=1).  And a plan that shares its device with another live plan (it then
    generates its normals in front of each rollout instead of beside the previous one) equals the plan run alone."""
    from mbd_hip.envs import get_env
    from mbd_hip.planners.mbd_planner import Args, Plan
    env = get_env(name)
    args = Args(env_name=name, Nsample=N, Hsample=50, Ndiffuse=7, temp_sample=0.1, enable_demo=demo,
                disable_recommended_params=True, not_render=True)
    st = env.reset(gpu.prng_key(4))
    key = gpu.prng_key(9)

    def run(**envs):
        levers(**{k: int(v) for k, v in envs.items()})
        p = Plan(env, args)
        p.set_state0(st)
        out = p.run(key)[:3]
        w = p.peek()[2]
        p.close()
        levers(**{k: -1 for k in envs})
        return out, w

    (mu0, rm0, rf0), w0 = run()
    for envs in (dict(MBD_NO_FUSED_SCORE="1"), dict(MBD_WMEAN_SPLIT="1")):
        (mu, rm, rf), w = run(**envs)
        assert np.array_equal(mu, mu0) and np.array_equal(rm, rm0) and rf == rf0 and np.array_equal(w, w0), envs
    other = Plan(env, args)  # a second live plan on the device (plans no longer count each other: shares_device says it)
    other.set_state0(st)
    (mu, rm, rf), w = run()
    other.close()
    assert np.array_equal(mu, mu0) and np.array_equal(rm, rm0) and rf == rf0 and np.array_equal(w, w0)

@pytest.mark.parametrize("name,N,H", [("humanoidrun", 1024, 50), ("hopper", 333, 50), ("halfcheetah", 200, 17), ("car2d", 128, 30),
                                      ("humanoidrun", 4096, 50), ("humanoidrun", 8192, 50), ("halfcheetah", 2500, 17)])
def test_score_launch_layouts_are_bit_identical(gpu, name, N, H, levers):
    """Round 5: the single-plan score + weighted-mean launch is pinned to X of the 8 XCDs (MBD_WMEAN_XCDS; the library picks X
    from the tile count and the candidates' bytes) and the sweeps' batch launch gives a thread V outputs (MBD_WMEAN_V; default 2).
    Which workgroup computes which outputs never enters a value: whole plans and sweeps under every setting, bit for bit — odd
    output counts (halfcheetah H=17: 102 outputs, a partial last tile at every V) included."""
    from mbd_hip.envs import get_env
    from mbd_hip.planners.mbd_planner import Args, Plan
    from mbd_hip.scripts.run_mbd import run_concurrent
    env = get_env(name)
    args = Args(env_name=name, Nsample=N, Hsample=H, Ndiffuse=6, temp_sample=0.1, disable_recommended_params=True, not_render=True)
    st, key = env.reset(gpu.prng_key(2)), gpu.prng_key(11)

    def run():
        p = Plan(env, args)
        p.set_state0(st)
        out = p.run(key)[:3]
        p.close()
        return out
    mu0, rm0, rf0 = run()
    for x in (1, 2, 4, 8):
        levers(MBD_WMEAN_XCDS=x)
        mu, rm, rf = run()
        assert np.array_equal(mu, mu0) and np.array_equal(rm, rm0) and rf == rf0, x
    levers(MBD_WMEAN_XCDS=-1)
    for v in (1, 2):  # (round 6: outputs per thread of the single-plan launch; the library keeps 1 — 2 measured slower, no lighter)
        levers(MBD_WMEAN_V1=v)
        mu, rm, rf = run()
        assert np.array_equal(mu, mu0) and np.array_equal(rm, rm0) and rf == rf0, v
    levers(MBD_WMEAN_V1=-1)
    if name == "car2d" or N > 1024:
        return
    plans = [Args(seed=s, env_name=name, Nsample=min(N, 256), Hsample=H, Ndiffuse=5, temp_sample=0.1, disable_recommended_params=True,
                  not_render=True) for s in range(8)]
    base = None
    for v in (2, 1, 4):
        levers(MBD_WMEAN_V=v)
        rews, mus, _ = run_concurrent(plans, batched=True)
        if base is None:
            base = (rews, mus)
        assert np.array_equal(np.float32(rews), np.float32(base[0])) and all(np.array_equal(a, b) for a, b in zip(mus, base[1])), v
    levers(MBD_WMEAN_V=-1)


@pytest.mark.parametrize("name,B,H", [("hopper", 512, 20), ("halfcheetah", 200, 12), ("humanoidrun", 100, 10), ("cartpole", 64, 30), ("ant", 128, 8)])
def test_rollout_launch_pinned_to_one_xcd_is_bit_identical(gpu, orc_omp, name, B, H, levers):
    """Round 5: small rollout launches are made 8 x as long and only every 8th workgroup rolls out (they all land on one XCD; the
    others carry the noise or leave): MBD_ROLL_PIN = 0 / 1 — rewards bit for bit the checker's either way, and a whole plan
    (whose launches carry the next step's normals in the other workgroups) equal under both."""
    from mbd_hip.envs import get_env
    from mbd_hip.planners.mbd_planner import Args, Plan
    env = get_env(name)
    oe = _oenv(orc_omp, env)
    st = env.reset(gpu.prng_key(1))
    us = np.clip(np.random.default_rng(B).normal(size=(B, H, env.action_size)) * 0.5, -1.2, 1.2).astype(np.float32)
    ref = oe.rollout(np.asarray(st.pipeline_state, np.float32), us)
    outs = []
    for pin in (0, 1):
        levers(MBD_ROLL_PIN=pin)
        assert np.array_equal(env.rollout(st, us).cpu().numpy(), ref), pin
        p = Plan(env, Args(env_name=name, Nsample=B, Hsample=H, Ndiffuse=5, temp_sample=0.1, disable_recommended_params=True, not_render=True))
        p.set_state0(st)
        outs.append(p.run(gpu.prng_key(3))[:3])
        p.close()
    levers(MBD_ROLL_PIN=-1)
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and outs[0][2] == outs[1][2]


@pytest.mark.parametrize("name,B,H", [("hopper", 77, 50), ("hopper", 512, 10), ("halfcheetah", 61, 50), ("halfcheetah", 256, 16),
                                      ("walker2d", 45, 50)])
def test_candidates_per_wavefront_and_contact_early_out_are_bit_identical(gpu, orc_omp, name, B, H, levers):
    """Round 6: launches that would leave SIMDs idle put fewer candidates on a wavefront (RolloutParams::cpw) and take a
    wave-uniform early-out around the contact code of a substep in which no sphere of the wavefront is below the plane
    (mbd_planar.h, EO).  MBD_CPW = 0 (the filled wavefronts of rounds 1-5) / 1 / 2 / 4 / 8 / unset (the library's choice): rewards bit
    for bit the checker's under every value (ragged B: the last wavefront repeats candidates), and a whole plan equal under all."""
    from mbd_hip.envs import get_env
    from mbd_hip.planners.mbd_planner import Args, Plan
    env = get_env(name)
    oe = _oenv(orc_omp, env)
    st = env.reset(gpu.prng_key(2))
    us = np.clip(np.random.default_rng(B + H).normal(size=(B, H, env.action_size)) * 0.6, -1.2, 1.2).astype(np.float32)
    ref = oe.rollout(np.asarray(st.pipeline_state, np.float32), us)
    outs = []
    for cpw in (0, 1, 2, 4, 8, -1):
        levers(MBD_CPW=cpw)
        assert np.array_equal(env.rollout(st, us).cpu().numpy(), ref), cpw
        p = Plan(env, Args(env_name=name, Nsample=B, Hsample=min(H, 12), Ndiffuse=5, temp_sample=0.1, disable_recommended_params=True, not_render=True))
        p.set_state0(st)
        outs.append(p.run(gpu.prng_key(3))[:3])
        p.close()
    levers(MBD_CPW=-1)
    for o in outs[1:]:
        assert np.array_equal(outs[0][0], o[0]) and np.array_equal(outs[0][1], o[1]) and outs[0][2] == o[2]


@pytest.mark.parametrize("name,N,H,Nd,cpw", [("hopper", 96, 20, 6, 0), ("hopper", 96, 20, 6, 2), ("halfcheetah", 50, 16, 5, 0), ("halfcheetah", 50, 16, 5, 1)])
def test_sweep_under_every_candidates_per_wavefront(gpu, name, N, H, Nd, cpw, levers):
    """... and a sweep (several plans in one launch: candidate b belongs to plan b / N) equals its plans run alone whatever the lever says."""
    from mbd_hip.planners.mbd_planner import Args, run_diffusion
    from mbd_hip.scripts.run_mbd import run_concurrent
    plans = [Args(seed=s, env_name=name, Nsample=N, Hsample=H, Ndiffuse=Nd, temp_sample=0.1, disable_recommended_params=True, not_render=True)
             for s in range(3)]
    levers(MBD_CPW=cpw)
    rews, mus, _ = run_concurrent(plans, batched=True)
    levers(MBD_CPW=-1)
    for a, r, mu in zip(plans, rews, mus):
        r_seq, det = run_diffusion(a, return_details=True)
        assert np.array_equal(mu, det["mu_0ts"]), (name, a.seed)
        assert np.float32(r) == np.float32(r_seq)


@pytest.mark.parametrize("N,Nd", [(96, 6), (33, 4)])
def test_demo_log_density_accumulated_in_the_rollout_is_bit_identical(gpu, orc_omp, N, Nd, levers):
    """Round 6: humanoidtrack's demo plans get eval_xref_logpd (humanoidtrack.py:98-106) out of the rollout kernel itself
    (RolloutParams::lp: S_k accumulated on each tracked link's lane, one control step at a time) instead of writing x.pos
    [N,H,5,3] for logpd_track_kernel to read back.  MBD_NO_FUSED_LOGPD = 1 forces the two-launch form of rounds 1-5: the same plan
    bit for bit, a sweep of three plans too; and the accumulated values equal the checker's on the tracked positions the
    rollout API returns."""
    from mbd_hip.envs import get_env
    from mbd_hip.planners.mbd_planner import Args, Plan, run_diffusion
    from mbd_hip.scripts.run_mbd import run_concurrent
    env = get_env("humanoidtrack")
    st = env.reset(gpu.prng_key(4))
    outs, lps = [], []
    for off in (0, 1):
        levers(MBD_NO_FUSED_LOGPD=off)
        p = Plan(env, Args(env_name="humanoidtrack", Nsample=N, Hsample=50, Ndiffuse=Nd, temp_sample=0.1, enable_demo=True,
                           disable_recommended_params=True, not_render=True))
        p.set_state0(st)
        outs.append(p.run(gpu.prng_key(3))[:3])
        p.close()
        plans = [Args(seed=s, env_name="humanoidtrack", Nsample=N, Hsample=50, Ndiffuse=Nd, temp_sample=0.1, enable_demo=True,
                      disable_recommended_params=True, not_render=True) for s in range(3)]
        lps.append(run_concurrent(plans, batched=True)[:2])
    levers(MBD_NO_FUSED_LOGPD=-1)
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and outs[0][2] == outs[1][2]
    assert all(np.array_equal(a, b) for a, b in zip(lps[0][1], lps[1][1])) and list(lps[0][0]) == list(lps[1][0])
    # the standalone entry against the checker, in the new order of the sum
    us = np.clip(np.random.default_rng(N).normal(size=(N, 50, env.action_size)) * 0.4, -1, 1).astype(np.float32)
    _, xpos = env.rollout(st, us, want_xpos=True)
    got = env.eval_xref_logpd_batch(xpos).cpu().numpy()
    want = np.array([orc_omp.track_xref_logpd(x, env.xref) for x in xpos.cpu().numpy()], np.float32)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name,planar_expected", [("hopper", True), ("walker2d", True), ("halfcheetah", True)])
def test_collide_all_capsules_models_bitexact(gpu, orc_omp, name, planar_expected):
    """DESIGN.md §9's data-level switch `collide_all_capsules` (every capsule end of every link a sphere collider instead of the
    feet only): hopper and walker2d stay on the tuned planar kernels (two spheres per link, now on EVERY lane), the
    halfcheetah's torso carries four and runs the planar kernels' four-collider instantiation (MAXCOL = 4: the stages collider by
    collider) — rollouts and a short plan bit for bit the checker's."""
    from conftest import ROOT
    from mbd_hip import mjcf
    from mbd_hip.envs import specs
    from mbd_hip.envs.base import RigidBodyEnv
    from mbd_hip.planners.mbd_planner import Args, Plan
    from oracle.planner import OracleEnv
    spec = specs.SPECS[name]
    m = mjcf.load(os.path.join(ROOT, "model-based-diffusion_amd", "assets", spec["xml"]), env_name=name, n_frames=spec["n_frames"],
                  reset_noise=spec["reset_noise"], reward_params=spec.get("reward_params", ()), gear_override=spec.get("gear_override", ()),
                  collide_all_capsules=True, warn_unstable=False)
    assert bool(int(m.fields["flags"]) & 2) == planar_expected and int(m.fields["n_col"]) >= 8
    env = RigidBodyEnv(name, model=m)
    oe = OracleEnv(orc_omp, name, m.to_struct(), init_q=m.init_q)
    st = env.reset(gpu.prng_key(6))
    us = np.clip(np.random.default_rng(5).normal(size=(70, 50, env.action_size)) * 0.7, -1.2, 1.2).astype(np.float32)
    ref = oe.rollout(np.asarray(st.pipeline_state, np.float32), us)
    got = env.rollout(st, us).cpu().numpy()
    assert np.isfinite(got).all() and np.array_equal(got, ref)
    p = Plan(env, Args(env_name=name, Nsample=64, Hsample=20, Ndiffuse=5, temp_sample=0.1, disable_recommended_params=True, not_render=True))
    p.set_state0(st)
    mu = p.run(gpu.prng_key(3))[0]
    p.close()
    assert np.isfinite(mu).all()


@pytest.mark.parametrize("name", ["hopper", "walker2d", "halfcheetah", "cartpole"])
def test_speculated_renormalisation_reruns_the_control_step_exactly(gpu, orc, name, levers):
    """Round 6: the planar kernels no longer branch on the renormalisation's rare exact side (|n2 - 1| > 0.05: a link turning by
    more than 0.45 rad in ONE substep) — they use the series unconditionally, keep the largest |n2 - 1| of the control step and
    re-run a control step in which it exceeded the bound, from its saved start, with the exact side selected (pl_qupdate QM = 1 /
    2).  Here a hinge starts at 400 rad/s (0.8 ... 2 rad per substep): the first control steps take the re-run, later ones do
    not — rewards bit for bit the checker's (which branches per renormalisation), filled wavefronts and every early-out form."""
    from conftest import load_model
    from mbd_hip.envs import get_env
    from mbd_hip.envs.base import State
    env = get_env(name)
    m = load_model(name)
    ms = m.to_struct()
    q = m.init_q.copy()
    qd = np.zeros(m.qd_size(), np.float32)
    qd[-1] = 400.0
    ps = env.pipeline_init(q, qd)
    st0 = orc.forward(ms, q, qd)
    assert np.array_equal(np.asarray(ps, np.float32).reshape(st0.shape), st0)
    st1 = orc.substep(ms, st0, np.zeros(m.act_size(), np.float32))
    assert np.abs(st1[:, 10:13]).max() * float(m.fields["dt"]) > 0.45   # (the exact side is taken in the very first substep)
    us = np.clip(np.random.default_rng(7).normal(size=(37, 12, env.action_size)) * 0.5, -1, 1).astype(np.float32)
    ref = orc.rollout(ms, st0, us)
    assert np.isfinite(ref).all()
    for cpw in (-1, 0, 1, 2):
        levers(MBD_CPW=cpw)
        got = env.rollout(State(ps, None, 0.0, 0.0, {}), us).cpu().numpy()
        assert np.array_equal(got, ref), (name, cpw, np.abs(got - ref).max())
    levers(MBD_CPW=-1)


@pytest.mark.parametrize("which,no_dpp,general", [("hopper", 0, 0), ("hopper", 1, 0), ("halfcheetah", 0, 0), ("halfcheetah", 1, 0),
                                                  ("halfcheetah", 0, 1), ("tripod", 0, 0)])
def test_planar_links_with_three_or_four_colliders(gpu, orc_omp, which, no_dpp, general, levers):
    """Round 6: the planar kernels take up to FOUR sphere colliders per link (MAXCOL = 4: two packed pairs) — what
    collide_all_capsules gives the halfcheetah's torso.  Every instantiation of that form: 4-lane groups (the hopper with two more
    spheres on its foot and one more on its leg), 8-lane DPP / shuffle / run-time switches (the halfcheetah with every capsule
    colliding), 16-lane groups (the ten-link tripod with three spheres on one link); rollouts bit for bit the checker's."""
    from conftest import ROOT
    from custom_models import TRIPOD
    from test_oracle_physics import _compile
    from mbd_hip import mjcf
    from mbd_hip.envs import specs
    from mbd_hip.envs.base import RigidBodyEnv
    from oracle.planner import OracleEnv
    if no_dpp:
        levers(MBD_NO_DPP=1)
    if general:
        for k in ("MBD_NO_PLANAR_FLAGS", "MBD_NO_REWARD_CONST", "MBD_NO_NFR_CONST"):
            levers(**{k: 1})
    assets = os.path.join(ROOT, "model-based-diffusion_amd", "assets")
    if which == "halfcheetah":
        sp = specs.SPECS["halfcheetah"]
        m = mjcf.load(os.path.join(assets, sp["xml"]), env_name="halfcheetah", n_frames=sp["n_frames"], reset_noise=sp["reset_noise"],
                      reward_params=sp["reward_params"], gear_override=sp["gear_override"], collide_all_capsules=True, warn_unstable=False)
        name, want_max = "halfcheetah", 4
    elif which == "hopper":
        xml = open(os.path.join(assets, "hopper.xml")).read()
        xml = xml.replace('name="foot_geom" size="0.06" type="capsule"/>', 'name="foot_geom" size="0.06" type="capsule"/>'
                          '<geom contype="1" type="sphere" pos="0.06 0 0" size="0.07"/><geom contype="1" type="sphere" pos="0.2 0 0" size="0.065"/>')
        xml = xml.replace('name="leg_geom" size="0.04" type="capsule"/>', 'name="leg_geom" size="0.04" type="capsule" contype="1"/>'
                          '<geom contype="1" type="sphere" pos="0 0 -0.25" size="0.05"/>')
        assert xml.count('type="sphere"') == 3
        sp = specs.SPECS["hopper"]
        m = _compile(xml, env_name="hopper", n_frames=sp["n_frames"], reset_noise=sp["reset_noise"], reward_params=sp["reward_params"])
        name, want_max = "hopper", 4
    else:
        # (foot_a: its capsule's two end spheres plus one on the capsule's axis — the link stays diagonal in its own frame)
        xml = TRIPOD.replace('<geom contype="1" fromto="-0.05 0 0 0.15 0 0" size="0.05" type="capsule"/>',
                             '<geom contype="1" fromto="-0.05 0 0 0.15 0 0" size="0.05" type="capsule"/>'
                             '<geom contype="1" type="sphere" pos="0.05 0 0" size="0.06"/>')
        assert xml != TRIPOD
        m = _compile(xml, env_name="halfcheetah", n_frames=6, reset_noise=0.05, reward_params=(1.0, 0.1))
        name, want_max = "halfcheetah", 3
    cl = list(m.fields["col_link"][:int(m.fields["n_col"])])
    assert bool(int(m.fields["flags"]) & 2) and max(cl.count(l) for l in set(cl)) >= min(want_max, 3)
    env = RigidBodyEnv(name, model=m)
    oe = OracleEnv(orc_omp, name, m.to_struct(), init_q=m.init_q)
    st = env.reset(gpu.prng_key(8))
    us = np.clip(np.random.default_rng(11).normal(size=(53, 40, env.action_size)) * 0.7, -1.2, 1.2).astype(np.float32)
    ref = oe.rollout(np.asarray(st.pipeline_state, np.float32), us)
    got = env.rollout(st, us).cpu().numpy()
    assert np.isfinite(got).all() and np.ptp(got) > 1e-3 and np.array_equal(got, ref), np.abs(got - ref).max()


# ---- two candidates per lane (mbd_pk2.h) -----------------------------------------------------------------------------
@pytest.mark.parametrize("name,B,H,sigma", [("humanoidrun", 96, 50, 0.6), ("humanoidrun", 1, 3, 0.3),
                                            ("humanoidrun", 37, 20, 0.9), ("humanoidtrack", 64, 50, 0.4),
                                            ("humanoidtrack", 9, 12, 0.4), ("humanoidstandup", 36, 50, 0.5),
                                            ("ant", 44, 50, 0.5), ("ant", 7, 20, 0.9)])
def test_pk2_rollout_bitexact(gpu, orc, name, B, H, sigma, monkeypatch, levers):
    """rollout_pk2_kernel — a lane holds its link for the candidates (2k, 2k+1), all arithmetic as v_pk_*_f32 — forced
    with MBD_PK2=1 (launches pick it by themselves only above 4096 candidates) and held to the checker bit for bit,
    odd batch sizes (a half-filled last pair) included."""
    levers(MBD_PK2=1)
    _rollout_bitexact(gpu, orc, name, B, H, sigma)


@pytest.mark.parametrize("name,B,H", [("humanoidrun", 24, 20), ("humanoidtrack", 16, 20), ("humanoidstandup", 12, 20),
                                      ("ant", 20, 20)])
def test_pk2_general_instantiations(gpu, orc, name, B, H, monkeypatch, levers):
    levers(MBD_PK2=1)
    for k in ("MBD_NO_REWARD_CONST", "MBD_NO_NFR_CONST"):
        levers(**{k: 1})
    _rollout_bitexact(gpu, orc, name, B, H, 0.5)


@pytest.mark.parametrize("name,B", [("humanoidrun", 8192), ("humanoidtrack", 4100), ("humanoidstandup", 4099), ("ant", 4098)])
def test_pk2_is_bit_identical_to_the_one_candidate_kernel_at_scale(gpu, name, B, monkeypatch, levers):
    """What a launch of more than 4096 candidates runs by default, against the one-candidate-per-lane kernel on the same
    inputs: rewards, tracked positions and the final link states of every candidate."""
    import torch
    from mbd_hip.envs import get_env
    env = get_env(name)
    st = env.reset(gpu.prng_key(4))
    rng = np.random.default_rng(B)
    us = np.clip(rng.normal(size=(B, 50, env.action_size)) * 0.7, -1.3, 1.3).astype(np.float32)
    want = env.xref is not None
    res = {}
    for k in ("0", "auto"):
        if k == "auto":  # (humanoidstandup keeps one candidate per lane by default — helper lanes: forced here)
            levers(MBD_PK2=1 if name == "humanoidstandup" else -1)
        else:
            levers(MBD_PK2=k)
        out = env.rollout(st, us, want_xpos=want, want_final=True)
        res[k] = [o.cpu().numpy() for o in out]
    for a, b in zip(res["0"], res["auto"]):
        assert np.isfinite(a).all() and np.array_equal(a, b)


# ---- sweeps: several plans in one launch per step (mbd_sweep_*) ------------------------------------------------------
@pytest.mark.parametrize("name,N,H,Nd,demo,pk2", [("humanoidrun", 256, 50, 12, False, None), ("humanoidrun", 96, 20, 8, False, "1"),
                                                  ("humanoidrun", 33, 12, 6, False, "1"), ("humanoidtrack", 128, 50, 8, True, None),
                                                  ("humanoidtrack", 64, 50, 6, True, "1"), ("hopper", 96, 50, 10, False, None),
                                                  ("halfcheetah", 50, 30, 7, False, None), ("ant", 40, 20, 6, False, None),
                                                  ("ant", 64, 20, 6, False, "1")])
def test_sweep_equals_the_plans_run_alone(gpu, name, N, H, Nd, demo, pk2, monkeypatch, levers):
    """SURVEY §8(f) N3 as ONE batched launch per diffusion step (mbd/scripts/run_mbd.py:17-39): every plan of a
    seed sweep — its own key chain and start state — comes out of mbd_sweep_run exactly as out of run_diffusion on its
    own: mu_0ts, per-step mean rewards and the final reward, bit for bit.  pk2 = "1": the sweep's rollout through the
    two-candidates-per-lane kernel (an odd N falls back to the one-candidate kernel: a pair must not straddle two
    plans)."""
    from mbd_hip.planners.mbd_planner import Args, run_diffusion
    from mbd_hip.scripts.run_mbd import run_concurrent
    plans = [Args(seed=s, env_name=name, Nsample=N, Hsample=H, Ndiffuse=Nd, temp_sample=0.1, enable_demo=demo,
                  disable_recommended_params=True, not_render=True) for s in range(5)]
    if pk2 is not None:
        levers(MBD_PK2=pk2)
    rews, mus, _ = run_concurrent(plans, batched=True)
    levers(MBD_PK2=-1)
    for a, r, mu in zip(plans, rews, mus):
        r_seq, det = run_diffusion(a, return_details=True)
        assert np.array_equal(mu, det["mu_0ts"]), (name, a.seed)
        assert np.float32(r) == np.float32(r_seq)


@pytest.mark.parametrize("name,bits,um", [("ant", 8 | 128, 0), ("hopper", 4 | 8 | 16 | 32, 0), ("crab", 4 | 64, 0), ("ant", 4 | 16, 2),
                                          ("random3col", 0, 0)])
def test_sweeps_on_the_general_instantiations_equal_the_plans_run_alone(gpu, name, bits, um):
    """Sweeps of models that run on the general instantiation of the specification switches — switched built-in models
    (3-D and planar), a custom model, a path-integral sweep, and a random model with three colliders on a link (zero flag
    word) — against the same plans run one by one: mu_0ts, mean rewards, final rewards, bit for bit."""
    from mbd_hip.planners.mbd_planner import Args, Plan, Sweep
    from mbd_hip.planners import path_integral
    if name == "random3col":
        from random_models import stable_random_model
        from test_random_models import _comp
        from mbd_hip.envs.base import RigidBodyEnv
        for seed in range(16, 400):
            _, m = stable_random_model(seed, _comp)
            F = m.fields
            if int(np.bincount(np.asarray(F["col_link"][:int(F["n_col"])]), minlength=m.n_links).max()) >= 3:
                break
        env, env_name = RigidBodyEnv("hopper", model=m), "hopper"
    else:
        env = _spec_env(name, bits)
        env_name = {"crab": "hopper"}.get(name, name)
    P, N, H, Nd = 3, 48, 12, 5
    if um == 0:
        args = Args(env_name=env_name, Nsample=N, Hsample=H, Ndiffuse=Nd, temp_sample=0.1, disable_recommended_params=True, not_render=True)
    else:
        args = path_integral.Args(env_name=env_name, Nsample=N, Hsample=H, Nrefine=Nd, temp_sample=0.1, disable_recommended_params=True)
    keys = np.array([gpu.prng_key(10 + k) for k in range(P)], np.uint32)
    states = [env.reset(gpu.prng_key(k)) for k in range(P)]
    sw = Sweep(env, args, P, update_method=um)
    for k in range(P):
        sw.set_state0(k, states[k])
    mu, rm, rf, _ = sw.run(keys)
    sw.close()
    for k in range(P):
        p = Plan(env, args, update_method=um)
        p.set_state0(states[k])
        mu1, rm1, rf1, _ = p.run(keys[k])
        p.close()
        assert np.array_equal(mu[k], mu1) and np.array_equal(rm[k], rm1) and np.float32(rf[k]) == np.float32(rf1), (name, k)
    assert not np.array_equal(mu[0], mu[1])


def test_temperature_sweep_equals_the_plans_run_alone(gpu):
    """run_mbd.py:42-64: eight temperatures at seed 0 — one sweep whose plans differ in temp_sample only."""
    from mbd_hip.planners.mbd_planner import Args, run_diffusion
    from mbd_hip.scripts.run_mbd import run_concurrent, _batchable
    temps = [0.01, 0.03, 0.06, 0.1, 0.2, 0.4, 0.6, 0.8]
    plans = [Args(seed=0, env_name="humanoidrun", Nsample=128, Hsample=30, Ndiffuse=9, temp_sample=t,
                  disable_recommended_params=True, not_render=True) for t in temps]
    assert _batchable(plans)
    rews, mus, _ = run_concurrent(plans)
    assert len({np.asarray(m).tobytes() for m in mus}) == len(temps)  # (the temperature does change the plan)
    for a, r, mu in zip(plans, rews, mus):
        r_seq, det = run_diffusion(a, return_details=True)
        assert np.array_equal(mu, det["mu_0ts"]) and np.float32(r) == np.float32(r_seq)


@pytest.mark.parametrize("impl", [1, 0])
@pytest.mark.parametrize("method", ["mppi", "cma-es", "cem"])
@pytest.mark.parametrize("name,N,H,Nr", [("hopper", 256, 50, 10), ("humanoidrun", 128, 20, 8), ("ant", 33, 12, 6)])
def test_path_integral_sweep_equals_the_plans_run_alone(gpu, method, name, N, H, Nr, impl, monkeypatch):
    """Round-3 verdict item 7: the path-integral baselines' sweeps (mbd/scripts/run_mbd.py:22-26,46-50 over
    path_integral.py:111-127) as ONE mbd_sweep — one sampling launch, one rollout launch and the update rule's kernels
    over all plans per refinement step.  Five seeds with five temperatures: mu_0ts, per-step mean rewards, the carried
    sigma (cma-es) and the final reward of every plan equal path_integral.run_path_integral on that plan alone, bit for
    bit, in both threefry layouts."""
    monkeypatch.setenv("MBD_THREEFRY_PARTITIONABLE", str(impl))
    from mbd_hip.planners import path_integral
    from mbd_hip.scripts.run_mbd import run_path_integral_sweep
    temps = [0.05, 0.1, 0.2, 0.4, 0.8]
    plans = [path_integral.Args(seed=s, env_name=name, update_method=method, Nsample=N, Hsample=H, Nrefine=Nr,
                                temp_sample=temps[s], disable_recommended_params=True) for s in range(5)]
    rews, secs, det = run_path_integral_sweep(plans, return_details=True)
    assert det is not None and np.isfinite(det["mu_0ts"]).all()
    for k, a in enumerate(plans):
        r_seq, d = path_integral.run_path_integral(path_integral.Args(**vars(a)), return_details=True)
        assert np.array_equal(det["mu_0ts"][k], d["mu_0ts"]), (method, name, k)
        assert np.array_equal(det["rew_means"][k], d["rew_means"])
        assert np.float32(det["sigma_final"][k]) == np.float32(d["sigma_final"])
        assert np.float32(rews[k]) == np.float32(r_seq)
    assert len({np.asarray(m).tobytes() for m in det["mu_0ts"]}) == len(plans)  # (five different plans)


def test_run_multiple_seed_path_integral_is_one_sweep(gpu, capsys):
    """mbd_hip.scripts.run_mbd.run_multiple_seed(algo="path_integral") (run_mbd.py:17-39): eight seeds through ONE
    sweep, the rewards those of the eight plans run alone."""
    from mbd_hip.planners import path_integral
    from mbd_hip.scripts import run_mbd
    kw = dict(Nsample=64, Hsample=20, Nrefine=6, disable_recommended_params=True)
    rews, secs = run_mbd.run_multiple_seed(run_mbd.Args(algo="path_integral", update_method="cma-es", env_name="hopper"), **kw)
    assert len(rews) == 8 and "per plan" in capsys.readouterr().out
    for seed in (0, 7):
        r = path_integral.run_path_integral(path_integral.Args(seed=seed, env_name="hopper", update_method="cma-es", **kw))
        assert np.float32(r) == np.float32(rews[seed])


def test_sweep_rejects_what_it_does_not_batch(gpu):
    from mbd_hip.envs import get_env
    from mbd_hip.planners.mbd_planner import Args, Sweep
    env = get_env("humanoidrun")
    a = Args(env_name="humanoidrun", Nsample=16384, Hsample=10, Ndiffuse=4, disable_recommended_params=True)
    with pytest.raises(gpu.MbdError):
        Sweep(env, a, 2)  # plans that fill the chip on their own
    a.Nsample = 64
    with pytest.raises(gpu.MbdError):
        Sweep(env, a, 33)  # more than MBD_SWEEP_MAX_PLANS
    with pytest.raises(gpu.MbdError):
        Sweep(get_env("car2d"), Args(env_name="car2d", Nsample=64, Hsample=10, Ndiffuse=4), 2)


def test_exchange_single_rank_and_argument_checks(gpu):
    """mbd_exchange_* with a world of one (no peer to map): the gathered values are the local ones; bad arguments fail."""
    import torch
    lib = gpu.load()
    h = C.c_void_p()
    gpu.check(lib.mbd_exchange_create(0, 0, 1, 2, 96, C.byref(h)))
    local = torch.arange(192, dtype=torch.float32, device="cuda").reshape(2, 96).contiguous()
    out = C.c_void_p()
    for step in range(5):
        gpu.check(lib.mbd_exchange_all_gather(h, local.data_ptr(), C.byref(out), torch.cuda.current_stream().cuda_stream))
        got = torch.empty(192, dtype=torch.float32, device="cuda")
        C.cdll.LoadLibrary("libamdhip64.so").hipMemcpy(C.c_void_p(got.data_ptr()), out, 768, 3)
        assert torch.equal(got, local.reshape(-1) )
        local += 1.0
    gpu.check(lib.mbd_exchange_status(h))
    gpu.check(lib.mbd_exchange_destroy(h))
    assert lib.mbd_exchange_create(0, 3, 2, 1, 8, C.byref(h)) == gpu.MBD_ERR_INVALID
    assert lib.mbd_exchange_create(0, 0, 99, 1, 8, C.byref(h)) == gpu.MBD_ERR_INVALID


# ---- the fallback build (round-2 verdict item 7) -----------------------------------------------------------------------
_VARIANT_PROBE = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
from mbd_hip import _capi
from mbd_hip.envs import get_env
out = {}
for name, B, pk2 in (("humanoidrun", 24, -1), ("humanoidrun", 24, 1), ("humanoidstandup", 8, -1), ("ant", 12, -1),
                     ("hopper", 32, -1), ("halfcheetah", 16, -1), ("cartpole", 32, -1), ("car2d", 16, -1)):
    _capi.debug_set("MBD_PK2", pk2)
    env = get_env(name)
    st = env.reset(_capi.prng_key(5))
    us = np.clip(np.random.default_rng(B).normal(size=(B, 20, env.action_size)) * 0.6, -1.3, 1.3).astype(np.float32)
    out[f"{name}_{pk2}"] = env.rollout(st, us).cpu().numpy()
np.savez(sys.argv[3], lib=np.array(_capi.LIB_PATH if not __import__("os").environ.get("MBD_HIP_LIB") else __import__("os").environ["MBD_HIP_LIB"]), **out)
'''


def test_fallback_build_is_bit_identical(gpu, tmp_path):
    """The library is built through an assembly post-pass (hipcc -S, tools/fix_straddles.py, assembler, lld, bundler:
    __graft_entry__.build) that re-encodes instructions without changing the stream; a toolchain that breaks that
    pipeline gets the plain hipcc build instead.  build() also leaves that plain build under lib/variants/: here one
    rollout per kernel family (3-D DPP, two candidates per lane, five colliders, ant, three planar families, car2d)
    runs through BOTH libraries, each in its own process, and must agree bit for bit — and build_mode.txt must say
    that the library under test did take the assembly path (no silent fallback)."""
    import subprocess, sys
    from conftest import ROOT
    pkg = os.path.join(ROOT, "model-based-diffusion_amd")
    with open(os.path.join(pkg, "lib", "build_mode.txt")) as f:
        assert f.read().strip() == "assembly", "the library under test is a fallback build"
    plain = os.path.join(pkg, "lib", "variants", "libmbd_hip_plain.so")
    assert os.path.exists(plain), "build() leaves the plain build under lib/variants/"
    res = {}
    for tag, lib_path in (("main", None), ("plain", plain)):
        env = dict(os.environ)
        env.pop("MBD_HIP_LIB", None)
        if lib_path:
            env["MBD_HIP_LIB"] = lib_path
        out = str(tmp_path / f"{tag}.npz")
        r = subprocess.run([sys.executable, "-c", _VARIANT_PROBE, ROOT, pkg, out], env=env, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res[tag] = np.load(out)
    assert str(res["plain"]["lib"]).endswith("libmbd_hip_plain.so") and str(res["main"]["lib"]).endswith("libmbd_hip.so")
    keys = [k for k in res["main"].files if k != "lib"]
    assert len(keys) == 8
    for k in keys:
        assert np.isfinite(res["main"][k]).all() and np.array_equal(res["main"][k], res["plain"][k]), k


_AVG_PROBE = r"""
import os, sys
root, pkg, out, W = sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4])
for p in (root, pkg, os.path.join(root, "tests")):
    sys.path.insert(0, p)
import numpy as np
from conftest import load_model
from mbd_hip import _capi
from mbd_hip.envs.base import RigidBodyEnv
from mbd_hip.planners.mbd_planner import Args, Plan
res = {"lib": np.array(os.environ.get("MBD_HIP_LIB", "")), "tuned": np.array(_capi.load().mbd_tuned_spec())}
def model_of(name, bits):
    if name.endswith("CA"):  # collide_all_capsules: the halfcheetah's torso then carries FOUR spheres (mbd_planar.h MAXCOL = 4)
        from mbd_hip import mjcf
        from mbd_hip.envs import specs
        sp = specs.SPECS[name[:-2]]
        return mjcf.load(os.path.join(pkg, "assets", sp["xml"]), env_name=name[:-2], n_frames=sp["n_frames"], reset_noise=sp["reset_noise"],
                         reward_params=sp.get("reward_params", ()), gear_override=sp.get("gear_override", ()), collide_all_capsules=True,
                         warn_unstable=False, spec_flags=bits)
    return load_model(name).with_spec(bits)
for name, B, bits in (("hopper", 80, W), ("halfcheetah", 72, W), ("walker2d", 40, W), ("ant", 44, W), ("humanoidstandup", 36, W),
                      ("humanoidrun", 48, W), ("ant", 4200, W), ("hopper", 64, W ^ 4), ("humanoidstandup", 24, W ^ 4), ("hopper", 48, W ^ 16),
                      ("halfcheetahCA", 56, W), ("halfcheetahCA", 40, W ^ 4)):
    env = RigidBodyEnv(name.replace("CA", ""), model=model_of(name, bits))
    st = env.reset(_capi.prng_key(5))
    H = 50 if B < 1000 else 6
    us = np.clip(np.random.default_rng(B + bits).normal(size=(B, H, env.action_size)) * 0.5, -1.2, 1.2).astype(np.float32)
    res[f"{name}_{B}_{bits}_state"] = np.asarray(st.pipeline_state, np.float32)
    res[f"{name}_{B}_{bits}_us"] = us
    res[f"{name}_{B}_{bits}_rewss"] = env.rollout(st, us).cpu().numpy()
    if B < 1000:
        p = Plan(env, Args(env_name=name, Nsample=B, Hsample=12, Ndiffuse=4, temp_sample=0.1, disable_recommended_params=True, not_render=True))
        p.set_state0(st)
        res[f"{name}_{B}_{bits}_mu"] = p.run(_capi.prng_key(3))[0]
        p.close()
np.savez(out, **res)
"""


def _tuned_variants():
    """(file name, word) of the MBD_TUNED_SPEC builds to hold to the checker: the one build() keeps (word 0: summed contacts) and whatever
    `python tools/build_variant.py spec<word> -DMBD_TUNED_SPEC=<word>` left beside it."""
    import glob, re
    from conftest import ROOT
    out = [("libmbd_hip_sum.so", 0)]
    for f in sorted(glob.glob(os.path.join(ROOT, "model-based-diffusion_amd", "lib", "variants", "libmbd_hip_spec*.so"))):
        m = re.search(r"libmbd_hip_spec(\d+)\.so$", f)
        if m:
            out.append((os.path.basename(f), int(m.group(1))))
    return out


@pytest.mark.parametrize("lib_name,word", _tuned_variants())
def test_tuned_spec_variant_is_bit_exact_to_the_flagged_checker(gpu, orc_omp, tmp_path, lib_name, word):
    """Round 6: the tuned kernels compile a word of specification switches in, MBD_TUNED_SPEC — MBD_DEFAULT_SPEC =
    contact_avg (4) in the library, 0 (a link's contacts summed: rounds 1-5) in lib/variants/libmbd_hip_sum.so, which build()
    keeps beside it.  Under the variant a model carrying the variant's word runs the TUNED instantiations (planar packed pairs
    with their early-out, the humanoids', ant's, the helper-lane form, two candidates per lane at 4200 ant candidates, four
    colliders on a link) and must equal the checker run with that word, bit for bit; a model with another word (the default 4,
    word ^ 16) runs the general SPEC instantiations there and must equal the checker too.  The library under test answers 4.
    (Other words — gauss_seidel, friction_vel_bound, restitution_min and their unions — build the same way; a variant named
    libmbd_hip_spec<word>.so found beside it is held to the same bar: round 6 ran 60 = all four.)"""
    import subprocess, sys
    from conftest import ROOT, load_model
    from oracle.planner import OracleEnv
    pkg = os.path.join(ROOT, "model-based-diffusion_amd")
    assert gpu.load().mbd_tuned_spec() == 4
    avg = os.path.join(pkg, "lib", "variants", lib_name)
    assert os.path.exists(avg), "build() leaves the summed-contacts build under lib/variants/"
    env = dict(os.environ)
    env["MBD_HIP_LIB"] = avg
    out = str(tmp_path / "avg.npz")
    r = subprocess.run([sys.executable, "-c", _AVG_PROBE, ROOT, pkg, out, str(word)], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    res = np.load(out)
    assert str(res["lib"]).endswith(lib_name) and int(res["tuned"]) == word
    cases = sorted({k.rsplit("_", 1)[0] for k in res.files if k.endswith("_rewss")})
    assert len(cases) == 12
    for c in cases:
        name, B, bits = c.split("_")
        if name.endswith("CA"):
            from mbd_hip import mjcf
            from mbd_hip.envs import specs
            sp = specs.SPECS[name[:-2]]
            m = mjcf.load(os.path.join(pkg, "assets", sp["xml"]), env_name=name[:-2], n_frames=sp["n_frames"], reset_noise=sp["reset_noise"],
                          reward_params=sp.get("reward_params", ()), gear_override=sp.get("gear_override", ()), collide_all_capsules=True,
                          warn_unstable=False, spec_flags=int(bits))
            name = name[:-2]
        else:
            m = load_model(name).with_spec(int(bits))
        oe = OracleEnv(orc_omp, name, m.to_struct(), init_q=getattr(m, "init_q", None))
        ref = oe.rollout(res[c + "_state"], res[c + "_us"])
        assert np.isfinite(res[c + "_rewss"]).all() and np.array_equal(res[c + "_rewss"], ref), c


def test_exchange_reports_a_peer_that_never_arrives(gpu, tmp_path):
    """A rank whose peer never pushes: its waits end at their time limit (~2 s of the wall clock, once — the flag is
    sticky), mbd_exchange_status turns that into MBD_ERR_STATE, and the process returns instead of hanging."""
    import json, socket, subprocess, sys
    from conftest import ROOT
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "exchange_timeout_worker.py"), str(tmp_path)]
    out = subprocess.run(cmd, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    r0 = json.load(open(os.path.join(tmp_path, "xt_rank0.json")))
    assert r0["error"] is not None and "time limit" in r0["error"], r0
    assert 1.0 < r0["seconds"] < 8.0, r0  # one limit, not four


# ---- round 3's bench configs at their full sizes ---------------------------------------------------------------------
def test_humanoidrun8192_full_size_step_bitexact(gpu, orc_omp):
    """bench config humanoidrun8192 — the reference's own default N for humanoidrun (mbd_planner.py:54-60), the launch
    the two-candidates-per-lane kernel serves by default — one whole reverse-diffusion step against the checker:
    sampled candidates, 2.9 M pair-substeps of rollout, softmax weights, Ybar_{i-1}, bit for bit."""
    assert gpu.debug_get("MBD_PK2") == -1  # (the library decides: more than 4096 candidates)
    _one_step(gpu, orc_omp, "humanoidrun", 8192, 50, 100, 0.1, 1, False, i=99)
    _one_step(gpu, orc_omp, "humanoidrun", 8192, 50, 100, 0.1, 1, False, i=7)


def test_sweep8_full_size_equals_the_plans_run_alone(gpu):
    """bench config sweep8 at full size: the reference's 8-seed sweep (run_mbd.py:17-39) at the metric's sizes —
    8 plans x N=1024 x H=50 x 99 steps through ONE launch per step over 8192 candidates — against each plan's own
    run_diffusion: mu_0ts and the final reward, bit for bit."""
    from mbd_hip.planners.mbd_planner import Args, run_diffusion
    from mbd_hip.scripts.run_mbd import run_concurrent
    plans = [Args(seed=s, env_name="humanoidrun", Nsample=1024, Hsample=50, Ndiffuse=100, temp_sample=0.1,
                  disable_recommended_params=True, not_render=True) for s in range(8)]
    rews, mus, secs = run_concurrent(plans)
    assert secs < 0.5
    for a, r, mu in zip(plans, rews, mus):
        r_seq, det = run_diffusion(a, return_details=True)
        assert np.array_equal(mu, det["mu_0ts"]) and np.float32(r) == np.float32(r_seq), a.seed


def test_ant_default_sweep_shape_bitexact(gpu, orc_omp):
    """The reference's literal default sweep is ant (run_mbd.py:14; Nsample 2048): one step of such a plan against the
    checker through the two-candidates-per-lane ant kernel (forced: a single plan of 2048 would not pick it), and a
    3-plan sweep of them against the plans run alone."""
    from mbd_hip.planners.mbd_planner import Args, run_diffusion
    from mbd_hip.scripts.run_mbd import run_concurrent
    gpu.debug_set("MBD_PK2", 1)
    try:
        _one_step(gpu, orc_omp, "ant", 2048, 50, 100, 0.1, 1, False, i=99)
    finally:
        gpu.debug_set("MBD_PK2", -1)
    plans = [Args(seed=s, env_name="ant", Nsample=2048, Hsample=50, Ndiffuse=12, temp_sample=0.1,
                  disable_recommended_params=True, not_render=True) for s in range(3)]
    rews, mus, _ = run_concurrent(plans)  # 6144 candidates in one launch: two per lane by default
    for a, r, mu in zip(plans, rews, mus):
        r_seq, det = run_diffusion(a, return_details=True)
        assert np.array_equal(mu, det["mu_0ts"]) and np.float32(r) == np.float32(r_seq), a.seed


def test_c_caller_without_python(gpu, tmp_path):
    """examples/mbd_run.c — run_diffusion and the seed sweep from plain C through include/mbd_hip.h (envs by name, no
    Python, no MJCF compiler) — compiled with gcc against the in-tree library and run: every plan's final reward equals
    the Python shim's run_diffusion for the same seed bit for bit (%.9g round-trips a float32), alone and in the sweep."""
    import re, shutil, subprocess
    from conftest import ROOT
    from mbd_hip.planners.mbd_planner import Args, run_diffusion
    if shutil.which("gcc") is None:
        pytest.skip("no gcc on this box")
    exe = str(tmp_path / "mbd_run")
    libdir = os.path.join(ROOT, "model-based-diffusion_amd", "lib")
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "mbd_run.c"),
                    "-o", exe, "-L", libdir, "-lmbd_hip", f"-Wl,-rpath,{libdir}", "-lm"], check=True)
    out = subprocess.run([exe, "humanoidrun", "256", "20", "9", "0.1", "3"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    alone = {int(m.group(1)): np.float32(m.group(2)) for m in re.finditer(r"^seed (\d+) rew_final (\S+)", out.stdout, re.M)}
    swept = {int(m.group(1)): np.float32(m.group(2)) for m in re.finditer(r"^sweep seed (\d+) rew_final (\S+)", out.stdout, re.M)}
    assert sorted(alone) == [0, 1, 2] and sorted(swept) == [0, 1, 2]
    for seed in range(3):
        a = Args(seed=seed, env_name="humanoidrun", Nsample=256, Hsample=20, Ndiffuse=9, temp_sample=0.1,
                 disable_recommended_params=True, not_render=True)
        r = np.float32(run_diffusion(a))
        assert alone[seed] == r and swept[seed] == r, (seed, alone[seed], swept[seed], r)


@pytest.mark.parametrize("helpers", [True, False])
def test_humanoidstandup_helper_lanes(gpu, orc, helpers, levers):
    """humanoidstandup's torso carries five sphere colliders.  By default its colliders 2..4 run stage (4) — a Jacobi
    solve: every contact sees the pose of the stage's start — on two of the candidate's five idle lanes, which ride on
    the torso's pose and hand impulse, rotation, contact point, multiplier and flag back; the torso adds them in
    collider order with the loop's own operations (HELP instantiations: 1726 -> 1345 instructions per substep).  The
    lever MBD_NO_HELPERS=1 keeps every collider on the torso's lane.  Both against the checker, bit for bit: rollouts
    with saturated actions (all fifteen colliders touch the floor while the humanoid lies down) and a planning step."""
    levers(MBD_NO_HELPERS=0 if helpers else 1)
    _rollout_bitexact(gpu, orc, "humanoidstandup", 52, 50, 0.9)
    _rollout_bitexact(gpu, orc, "humanoidstandup", 3, 7, 0.2)
    _one_step(gpu, orc, "humanoidstandup", 96, 20, 30, 0.1, 1, False, i=29)
    levers(MBD_NO_REWARD_CONST=1, MBD_NO_NFR_CONST=1)   # the general instantiation of either form
    _rollout_bitexact(gpu, orc, "humanoidstandup", 12, 20, 0.5)


@pytest.mark.parametrize("mode", ["host_ahead", "host_in_step", "other_stream"])
def test_noise_ring_orderings_are_bit_identical(gpu, mode, levers):
    """Plans whose rollout fills the chip keep their normals in a ring of three buffers filled on a second stream (forced
    here on a small plan by MBD_NO_FUSED_NOISE): a caller that never waits (held one step behind the device through the
    progress word), one that synchronises after every step (the mark behind the weighted mean), and one that alternates
    the stream of its calls must all equal mbd_plan_run's own loop — Ybars, mean rewards, final reward — over enough steps
    for the ring to wrap several times."""
    levers(MBD_NO_FUSED_NOISE=1)
    import torch
    from mbd_hip.envs import get_env
    from mbd_hip.planners.mbd_planner import Args, Plan
    N, H, Nd = 1024, 20, 14
    env = get_env("humanoidrun")
    args = Args(env_name="humanoidrun", Nsample=N, Hsample=H, Ndiffuse=Nd, temp_sample=0.1,
                disable_recommended_params=True, not_render=True)
    st = env.reset(gpu.prng_key(2))
    key = gpu.prng_key(6)
    p1 = Plan(env, args)
    p1.set_state0(st)
    mu1, rm1, rf1, _ = p1.run(key)
    p1.close()
    p2 = Plan(env, args)
    p2.set_state0(st)
    HNu = H * 17
    side = torch.cuda.Stream()
    bufs = [torch.zeros(HNu, device="cuda") for _ in range(Nd)]
    rms = torch.zeros(Nd, device="cuda")
    loc = torch.zeros(N, device="cuda")
    torch.cuda.synchronize()
    rng = np.asarray(key, np.uint32)
    impl = int(p2.cfg.prng_impl)
    keys = gpu.prng_split(rng, 2, impl)
    for k, i in enumerate(range(Nd - 1, 0, -1)):
        rng, ks = keys[0], gpu.key_array(keys[1])
        keys = gpu.prng_split(rng, 2, impl)
        if i > 1:
            gpu.check(p2.lib.mbd_plan_prefetch_noise(p2.h, gpu.key_array(keys[1]), None))
        stream = side.cuda_stream if (mode == "other_stream" and k % 2) else None
        gpu.check(p2.lib.mbd_plan_sample_rollout(p2.h, i, ks, bufs[k].data_ptr(), loc.data_ptr(), None, stream))
        gpu.check(p2.lib.mbd_plan_score_update(p2.h, i, ks, bufs[k].data_ptr(), loc.data_ptr(), None, bufs[k + 1].data_ptr(),
                                               rms[k:].data_ptr(), stream))
        if mode == "host_in_step":
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    mus = np.stack([b.cpu().numpy().reshape(H, 17) for b in bufs[1:]])
    assert np.array_equal(mus, mu1) and np.array_equal(rms.cpu().numpy()[:Nd - 1], rm1), mode
    assert p2.eval(mu1[-1]) == rf1
    p2.close()


@pytest.mark.parametrize("pk2", [0, 1])
def test_ant_second_collider_skip_is_exact(gpu, orc, pk2, levers):
    """ant's rollout instantiations skip stage (6) of a link's SECOND collider (the ankle end of a lower leg's capsule)
    when no lane of the wavefront has it in contact (SKIP6, mbd_kernels.h / mbd_pk2.h).  From the standing start that
    slot is idle; here the ant is dropped flat on its belly with its legs spread, so that both ends of every lower leg
    touch the floor in some candidates and not in others: the kernel must equal the checker bit for bit through both
    sides of the test, one and two candidates per lane."""
    from mbd_hip.envs import get_env
    levers(MBD_PK2=pk2)
    env = get_env("ant")
    oe = _oenv(orc, env)
    m = env.sys
    q = np.array(m.init_q, np.float32).copy()
    q[2] = 0.07                      # torso 7 cm above the floor (standing: 0.55)
    q[7:] = 0.0                      # hips and ankles at zero: the lower legs level with the floor (outside the ankles'
                                     # range: the limit corrections then lift the ankle ends at candidate-dependent times)
    s0 = orc.forward(m.to_struct(), q, np.zeros(m.qd_size(), np.float32))
    # (the premise: in this pose the ankle-end spheres — every second collider — are at or below the floor)
    f = m.fields
    col_link, col_pos, col_rad = np.asarray(f["col_link"]), np.asarray(f["col_pos"], np.float32), np.asarray(f["col_radius"], np.float32)
    st = np.asarray(s0, np.float32).reshape(-1, 13)
    def rot(qw, v):
        w, x, y, z = qw
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        return R @ v
    low = [st[l, 0:3][2] + rot(st[l, 3:7], col_pos[k])[2] - col_rad[k] for k, l in enumerate(col_link)]
    assert min(low[1::2]) < 0.02, low
    B, H = 96, 30
    rng = np.random.default_rng(17)
    us = np.clip(rng.normal(size=(B, H, env.action_size)) * 0.8, -1.0, 1.0).astype(np.float32)
    from mbd_hip.envs.base import State
    state = env.reset(gpu.prng_key(3))
    state = state.replace(pipeline_state=np.asarray(s0, np.float32)) if hasattr(state, "replace") else State(np.asarray(s0, np.float32), state.obs, state.reward, state.done)
    got = env.rollout(state, us).cpu().numpy()
    ref = oe.rollout(np.asarray(s0, np.float32), us)
    assert np.isfinite(got).all() and np.array_equal(got, ref), np.abs(got - ref).max()


# ---- the specification switches (round-3 verdict item 3): checker and kernels honour every flag alike ---------------------
def _spec_env(name, bits, planar=None):
    """A built-in or custom model with the specification switches `bits` (mbd_model_flags) behind the C ABI."""
    from conftest import load_model
    from custom_models import CRAB, TRIPOD
    from test_oracle_physics import _compile
    from mbd_hip.envs.base import RigidBodyEnv
    if name == "crab":
        m, env_name = _compile(CRAB, env_name="hopper", n_frames=3, reset_noise=0.02, reward_params=(1.0, 0.5)), "hopper"
    elif name == "tripod":
        m, env_name = _compile(TRIPOD, env_name="halfcheetah", n_frames=6, reset_noise=0.05, reward_params=(1.0, 0.1),
                               planar=planar), "halfcheetah"
    else:
        m, env_name = load_model(name), name
        if planar is False:
            m.fields["flags"] = int(m.fields["flags"]) & ~2
    return RigidBodyEnv(env_name, model=m.with_spec(bits))


from state_inputs import SPEC_WORDS  # noqa: E402 — shared with the census (tests/state_census_worker.py)


@pytest.mark.parametrize("name,planar,bits", SPEC_WORDS)
def test_specification_switches_bitexact(gpu, orc, name, planar, bits):
    """Every specification switch (include/mbd_hip.h mbd_model_flags: contact_avg 4, contact6_gauss_seidel 8, friction_vel_bound
    16, restitution_min 32, euler_extrinsic 64, gyroscopic 128), alone and combined, on every inertia class of the 3-D SPEC
    instantiations (isotropic: the humanoids, ant; axisymmetric: hopper / walker2d / tripod compiled 3-D; full tensors:
    the crab) and on the planar SPEC instantiation: reset (forward kinematics under euler_extrinsic), rollouts and one
    planning step through the C ABI, bit for bit against the checker run with the same flag word."""
    env = _spec_env(name, bits, planar)
    assert int(env.sys.fields["flags"]) & 252 == bits
    st = env.reset(gpu.prng_key(7))
    oe = _oenv(orc, env)
    assert np.array_equal(np.asarray(st.pipeline_state, np.float32).reshape(-1),
                          np.asarray(oe.reset(gpu.prng_key(7), gpu_impl()), np.float32).reshape(-1))
    rng = np.random.default_rng(bits * 7 + len(name))
    B, H = 41, 30
    us = np.clip(rng.normal(size=(B, H, env.action_size)) * 0.5, -1.3, 1.3).astype(np.float32)
    want = env.xref is not None
    out = env.rollout(st, us, want_xpos=want)
    ref = oe.rollout(np.asarray(st.pipeline_state, np.float32), us, want_xpos=want)
    got = (out[0] if want else out).cpu().numpy()
    ref0 = ref[0] if want else ref
    assert np.isfinite(got).all() and np.ptp(got) > 1e-3
    assert np.array_equal(got, ref0), f"{name} flags={bits}: max |d| = {np.abs(got - ref0).max()}"
    if want:
        assert np.array_equal(out[1].cpu().numpy(), ref[1])


def gpu_impl():
    from mbd_hip.envs.base import prng_impl
    return prng_impl()


@pytest.mark.parametrize("name,bits", [("humanoidstandup", 8), ("hopper", 4 | 8 | 16)])
def test_specification_switches_change_results_and_plans_run(gpu, orc, name, bits):
    """The switches are not no-ops on the GPU either (a flagged model's rewards differ from the default's on the same
    actions), and a whole plan of a flagged model runs through mbd_plan_run, bit-exact per step against the checker."""
    env0, env1 = _spec_env(name, 0), _spec_env(name, bits)
    st = env0.reset(gpu.prng_key(3))
    rng = np.random.default_rng(5)
    us = np.clip(rng.normal(size=(64, 50, env0.action_size)) * 0.1, -1, 1).astype(np.float32)
    r0, r1 = env0.rollout(st, us).cpu().numpy(), env1.rollout(st, us).cpu().numpy()
    assert np.isfinite(r1).all() and not np.array_equal(r0, r1)
    _one_step(gpu, orc, name, 96, 20, 10, 0.1, 1, False, i=5, env=env1)
