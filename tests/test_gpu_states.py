"""-m gpu: the rollout kernels against the checker from start states across the whole state space (tests/state_inputs.py).

Every other GPU test starts from `env.reset`: the standing pose plus a few percent of noise.  Here every family of
state_inputs — random up to 3.2 rad / 30 rad/s, reached (fallen), joints at their limits, spheres on the plane, half turns,
non-unit quaternions, zero and 1e-30 velocities — goes through `env.rollout(..., want_final=True)` under each kernel family
the model can take, through `env.step`, and through the planner.  Rewards, tracked positions and FINAL STATES are compared
with the checker's by BIT PATTERN (state_inputs.same_bits): -0.0 is not +0.0.  tests/test_state_coverage.py shows on the CPU
that these cases reach every line and branch direction of the checker's step path."""
import functools

import numpy as np
import pytest

import state_inputs as si
from state_inputs import same_bits

pytestmark = pytest.mark.gpu

PLANAR = ("hopper", "walker2d", "halfcheetah", "cartpole")
HOT3D = ("humanoidrun", "humanoidtrack", "humanoidstandup", "ant")
# lever settings of each kernel family (conftest.levers; MBD_NO_DPP is read when the env is created)
KERNELS = {"default": {}, "no_dpp": dict(MBD_NO_DPP=1),
           "general": dict(MBD_NO_PLANAR_FLAGS=1, MBD_NO_REWARD_CONST=1, MBD_NO_NFR_CONST=1), "pk2": dict(MBD_PK2=1),
           "cpw0": dict(MBD_CPW=0), "cpw1": dict(MBD_CPW=1), "cpw2": dict(MBD_CPW=2), "cpw4": dict(MBD_CPW=4), "cpw8": dict(MBD_CPW=8)}
# the random and reached families go through every kernel family of a model; the others through the default choice and ALT: the
# one alternative whose code differs most for them (the two-candidate kernels' own renormalisation, contact and store; the
# filled-wavefront planar kernels without the contact early-out; the shuffle exchange for the custom trees)
WIDE = ("random", "reached")


def _matrix():
    out = []
    for n in HOT3D:
        out += [(n, k) for k in ("default", "no_dpp", "general", "pk2")]
    for n in PLANAR:
        out += [(n, k) for k in ("default", "no_dpp", "general", "cpw0", "cpw1", "cpw2", "cpw4", "cpw8")]
        out += [(n + "3d", "default"), (n + "3d", "no_dpp")]
    out += [(n, k) for n in ("tripod", "tripod_hi") for k in ("default", "no_dpp", "cpw0")]
    out += [(n, k) for n in ("crab", "tripod3d", "drop", "ant_unhealthy", "hopper3d_yaxis", "crab_xz", "crab_yz")
            for k in ("default", "no_dpp")]
    return out


def _alt(name):
    return "pk2" if name in HOT3D else "cpw0" if name in PLANAR + ("tripod", "tripod_hi") else "no_dpp"


@pytest.fixture(scope="module")
def gpu(lib):
    from mbd_hip import _capi
    if _capi.device_count() < 1:
        pytest.fail("tests/test_gpu_states.py needs a GPU")
    return _capi


def _env(name):
    """The env of a state_inputs model name: built-in names by name (the tuned instantiations), the rest from the model."""
    from mbd_hip.envs import get_env
    from mbd_hip.envs.base import RigidBodyEnv
    if name in si.BUILTIN:
        return get_env(name)
    m, env_name = si.model(name)
    return RigidBodyEnv(env_name, model=m)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """[(case, state, actions, checker's rewards, tracked positions, final states)] of a model, computed once."""
    from oracle.oracle import Oracle
    orc = Oracle("f32")
    m, _ = si.model(name)
    ms = m.to_struct()
    return [(case, s, us) + tuple(orc.rollout(ms, s, us, want_xpos=True, want_final=True)) for case, s, us in si.cases(orc, m, name=name)]


def _state(env, s):
    from mbd_hip.envs.base import State
    return State(np.asarray(s, np.float32), None, np.float32(0.0), np.float32(0.0), {})


def _compare_rollout(env, s, us, rew, xpos, fin, what):
    want = env.xref is not None
    out = env.rollout(_state(env, s), us, want_xpos=want, want_final=True)
    same_bits(out[0].cpu().numpy(), rew, f"{what}: rewards")
    if want:
        same_bits(out[1].cpu().numpy(), xpos, f"{what}: tracked positions")
    same_bits(out[-1].cpu().numpy(), fin, f"{what}: final states")


@pytest.mark.parametrize("name,kernel", _matrix())
def test_rollout_from_every_start_state(gpu, levers, name, kernel):
    """Rewards, tracked positions (where the env has a demo) and the final states [B][state] of an odd-B, short-H rollout
    from every case, bit pattern for bit pattern the checker's."""
    levers(**KERNELS[kernel])
    env = _env(name)
    fams = si.FAMILIES if kernel in ("default", _alt(name)) else WIDE
    n = 0
    for case, s, us, rew, xpos, fin in _reference(name):
        if case.split("/")[0] in fams:
            _compare_rollout(env, s, us, rew, xpos, fin, f"{name} [{kernel}] {case}")
            n += 1
    assert n >= 3 * si.N_RANDOM


def test_car2d_from_its_start_states(gpu, orc):
    from mbd_hip.envs import get_env
    env = get_env("car2d")
    for case, q, us in si.car2d_cases():
        rew, qs = orc.car2d_rollout(q, us, want_qs=True)
        out = env.rollout(_state(env, q), us, want_xpos=True, want_final=True)
        same_bits(out[0].cpu().numpy(), rew, f"{case}: rewards")
        same_bits(out[1].cpu().numpy(), qs, f"{case}: states along the way")
        same_bits(out[2].cpu().numpy(), qs[:, -1], f"{case}: final states")
        st = env.step(_state(env, q), us[0, 0])
        q1, r1 = orc.car2d_step(q, us[0, 0])
        same_bits(st.pipeline_state, q1, f"{case}: env.step state")
        same_bits(st.reward, r1, f"{case}: env.step reward")


@pytest.mark.parametrize("name", ["hopper", "walker2d", "halfcheetah", "tripod", "crab"])
def test_wavefronts_that_mix_contact_and_flight(gpu, orc, levers, name):
    """A launch takes one start state, so the candidates of a wavefront are told apart by their actions: from a state that
    hovers just above contact some push a sphere into the plane within the first control step and some do not.  The planar
    kernels' contact early-out is wave-uniform on "no sphere of this wavefront is below the plane", and an early-out
    wavefront holds candidates [w k, (w + 1) k) for k = candidates per wavefront.  So MBD_CPW is forced to 1, 2, 4 and 8
    besides unset and 0; the library says which kernel and which k each setting gives (mbd_debug_rollout_choice: k = 0 is
    the filled kernel without early-out); every DIFFERENT launch runs once; and for every launch with k >= 2 the checker
    must show a group of k consecutive candidates, aligned as the kernel groups them, that holds both kinds.  At least
    one such launch must exist for the hopper, the walker and the halfcheetah.  (Early-out instantiations
    exist for these three built-in models only, mbd_planar.hip: the tripod and the 3-D crab get one launch each, with the same mixed actions.  The humanoids and
    the ant touch down under every row of state_inputs.mixed_actions or under none.)"""
    m, _ = si.model(name)
    found = si.mixed_case(orc, m)
    assert found is not None, f"{name}: no hover height splits the first 64 candidates"
    gap, s, us = found
    t = si.touches(orc, m, s, us)
    assert t[:64].any() and not t[:64].all()
    rew, xpos, fin = orc.rollout(m.to_struct(), s, us, want_xpos=True, want_final=True)
    env = _env(name)
    seen, mixed_groups = set(), {}
    for lever in (-1, 0, 1, 2, 4, 8):
        levers(MBD_CPW=lever)
        choice = gpu.debug_rollout_choice(env.sys.to_struct(), 256, us.shape[0], us.shape[1])
        if (choice["name"], choice["cpw"]) in seen:
            continue  # (the same kernel with the same grouping as an earlier setting)
        seen.add((choice["name"], choice["cpw"]))
        k = choice["cpw"]
        if k >= 2:
            groups = t[: (t.size // k) * k].reshape(-1, k)
            n_mixed = int((groups.any(1) & ~groups.all(1)).sum())
            assert n_mixed > 0, f"{name}: no wavefront of {k} candidates holds both kinds"
            mixed_groups[k] = n_mixed
        _compare_rollout(env, s, us, rew, xpos, fin, f"{name} MBD_CPW={lever} ({k} per wavefront)")
    print(f"{name}: hovering {gap * 1e3:g} mm, {int(t.sum())} of {t.size} candidates touch down in the first control step; "
          f"{len(seen)} different launches; wavefronts holding both kinds, by candidates per wavefront: {mixed_groups}")
    if name in ("hopper", "walker2d", "halfcheetah"):
        assert mixed_groups, f"{name}: no early-out launch with two or more candidates per wavefront"
    else:  # (no early-out instantiation: whatever MBD_CPW says the launch is the same, and it ran once)
        assert len(seen) == 1


@pytest.mark.parametrize("name", si.BUILTIN + si.CUSTOM)
def test_env_step_from_every_start_state(gpu, orc, name):
    """env.step (B = 1, H = 1, host pointers) from every case: the next state and the reward against the checker's env_step,
    by bit pattern.  The observation is a CONSISTENCY check only, not a comparison with the checker, which has no
    observation path: step()'s obs must be what the library's own host-side observe() makes of the checker's next state —
    i.e. step() observes the state it returns.  (tests/test_host_obs.py holds observe() itself to the forward kinematics.)"""
    env = _env(name)
    ms = si.model(name)[0].to_struct()
    for case, s, us, *_ in _reference(name):
        a = us[0, 0]
        st = env.step(_state(env, s), a)
        s1, r1 = orc.env_step(ms, s, a)
        same_bits(st.pipeline_state, s1, f"{name} {case}: next state")
        same_bits(st.reward, r1, f"{name} {case}: reward")
        same_bits(st.obs, env.observe(s1), f"{name} {case}: observation")


def _reached(orc, name, which="reached/1"):
    m, _ = si.model(name)
    return dict(si.reached_states(orc, m))[which]


@pytest.mark.parametrize("name", si.BUILTIN + ("car2d",))
def test_planning_step_from_a_reached_state(gpu, orc, name):
    """One diffusion step of a plan whose state0 (Plan.set_state0) is where the robot ended up, against the checker's."""
    from test_gpu_parity import _one_step
    s0 = np.array([0.2, -0.45, 2.5], np.float32) if name == "car2d" else _reached(orc, name)
    _one_step(gpu, orc, name, 48, 8, 10, 0.1, 1, False, i=5, state0=s0)


@pytest.mark.parametrize("name,N", [("humanoidrun", 64), ("hopper", 96)])
def test_receding_horizon_episode_from_a_fallen_state(gpu, orc_omp, name, N):
    """A short closed-loop episode (mbd_plan_run_mpc) that starts where 100 control steps without actuation left the body
    (state_inputs "reached/unactuated": collapsed, hanging from its foot colliders): actions, rewards, states and means of
    every tick against tests/mpc_checker.py, by bit pattern."""
    import mpc_checker
    from mbd_hip.envs import get_env
    from mbd_hip.envs.base import prng_impl
    from mbd_hip.planners.mbd_planner import Args, Plan
    from test_gpu_parity import _oenv
    env = get_env(name)
    s0 = _reached(orc_omp, name, "reached/unactuated")
    H, Nd, T, K, E, temp = 12, 8, 3, 2, 1, 0.1
    plan = Plan(env, Args(env_name=name, Nsample=N, Hsample=H, Ndiffuse=Nd, temp_sample=temp, disable_recommended_params=True,
                          not_render=True))
    plan.set_state0(_state(env, s0))
    key = gpu.prng_key(5)
    got = plan.run_mpc(key, T, K, E)
    plan.close()
    ref = mpc_checker.episode(_oenv(orc_omp, env), s0, key, N, H, Nd, temp, T, K, E, impl=prng_impl())
    for k in ("means", "actions", "rewards", "states"):
        same_bits(got[k], ref[k], f"{name}: {k} of the episode")
    assert not np.array_equal(ref["states"][0], ref["states"][-1])
