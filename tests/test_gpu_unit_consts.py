"""-m gpu: the instantiations with the humanoids' unit inverse inertia compiled in (mbd_kernels.h unit_inertia_form) against the
checker and against their twins that read the inverse inertia from the lane records (rollout_kernel_rtib,
rollout_pk2_kernel_rtib), bit for bit.

humanoidrun and humanoidtrack, H = 2 control steps of the model's own n_frames.  One candidate per lane: B = 5, a full
wavefront and one that holds a single candidate; two per lane (lever MBD_PK2 = 1): B = 9, whose odd count leaves a pair
half filled.  Start states: the reset pose, and the states of tests/contact_pair_inputs.py with the shins in the floor
(rest_left, slide_left, both, deep) — the angular part of a contact impulse is where a link's inverse inertia enters.
Actions are seeded normals clipped to [-1, 1].  Rewards and final link states equal (a) the checker's and (b) the same call
under MBD_NO_UNIT_CONST = 1 by bit pattern.

An ensemble of the stock model and scaled(mass=1.25) — whose inverse inertia is 0.8 — in ONE launch must not run the unit
form on the scaled member: four candidates each, against the same plan with one launch per member (MBD_ENS_SPLIT = 1)."""
import functools

import numpy as np
import pytest

import contact_pair_inputs as cp
import state_inputs as si
from state_inputs import same_bits

pytestmark = pytest.mark.gpu

H = 2
STARTS = ("reset", "rest_left", "slide_left", "both", "deep")
HUMANOIDS = {"humanoidrun": "0, 7", "humanoidtrack": "3, 5"}
# form -> (B, levers of the launch, the instantiation's name with `{}` for "reward kind, n_frames")
FORMS = {"3d": (5, {}, "rollout_kernel<16, true, false, 3, 1, 1, -4, -6, 0, false, true, 3, false, false, {}, false, false, false>"),
         "pk2": (9, {"MBD_PK2": 1}, "rollout_pk2_kernel<1, {}, 1, 0>")}


@pytest.fixture(scope="module")
def gpu(lib):
    from mbd_hip import _capi
    if _capi.device_count() < 1:
        pytest.fail("tests/test_gpu_unit_consts.py needs a GPU")
    return _capi


def _actions(m, b, seed):
    rng = np.random.default_rng(si._seed("unit_consts", seed))
    return np.clip(rng.normal(size=(b, H, m.act_size())), -1.0, 1.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _reference(name, b):
    """[(start, q, qd, us, the checker's rewards, the checker's final states)] — computed once per model and size."""
    from oracle.oracle import Oracle
    orc = Oracle("f32")
    m, _ = si.model(name)
    ms = m.to_struct()
    zero = np.zeros(m.qd_size(), np.float32)
    starts = [("reset", m.init_q.astype(np.float32), zero)] + [(c, q, qd) for c, q, qd in cp.cases(name) if c in STARTS]
    assert tuple(s[0] for s in starts) == STARTS
    out = []
    for i, (start, q, qd) in enumerate(starts):
        us = _actions(m, b, i)
        rew, fin = orc.rollout(ms, orc.forward(ms, q, qd), us, want_final=True)
        out.append((start, q, qd, us, rew, fin))
    return out


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", sorted(HUMANOIDS))
def test_unit_form_against_the_checker_and_the_general_form(gpu, levers, name, form):
    from mbd_hip.envs import get_env
    from mbd_hip.envs.base import State
    b, launch_levers, kernel = FORMS[form]
    env = get_env(name)
    ms = env.sys.to_struct()
    levers(**launch_levers)

    def run(s0, us):
        out = env.rollout(State(np.asarray(s0, np.float32), None, np.float32(0.0), np.float32(0.0), {}), us, want_final=True)
        return out[0].cpu().numpy(), out[-1].cpu().numpy()

    for start, q, qd, us, rew, fin in _reference(name, b):
        what = f"{name} {form} {start} N={b} H={H}"
        s0 = env.pipeline_init(q, qd)
        levers(MBD_NO_UNIT_CONST=-1)
        choice = gpu.debug_rollout_choice(ms, 256, b, H)["name"]
        assert "mbd::" + kernel.format(HUMANOIDS[name]) in choice, choice
        got_rew, got_fin = run(s0, us)
        same_bits(got_rew, rew, f"{what}: rewards against the checker")
        same_bits(got_fin, fin, f"{what}: final states against the checker")
        levers(MBD_NO_UNIT_CONST=1)
        choice = gpu.debug_rollout_choice(ms, 256, b, H)["name"]
        assert "mbd::" + kernel.format(HUMANOIDS[name]).replace("kernel<", "kernel_rtib<") in choice, choice
        gen_rew, gen_fin = run(s0, us)
        same_bits(got_rew, gen_rew, f"{what}: rewards against the general form")
        same_bits(got_fin, gen_fin, f"{what}: final states against the general form")


@pytest.mark.parametrize("name", sorted(HUMANOIDS))
def test_one_launch_ensemble_with_a_scaled_member(gpu, levers, name):
    """The one launch runs ONE instantiation on every member's model: with a member whose inverse inertia is 0.8 it has to be
    the twin that reads it.  Against one launch per member, where the stock member runs the unit form and the scaled one the twin."""
    from mbd_hip.envs import get_env
    from mbd_hip.envs.base import RigidBodyEnv
    from mbd_hip.planners.mbd_planner import Args, Plan
    env = get_env(name)
    members = [None, RigidBodyEnv(name, model=env.sys.scaled(mass=1.25))]
    a = Args(env_name=name, Nsample=4, Hsample=H, Ndiffuse=3, temp_sample=0.1, disable_recommended_params=True, not_render=True)
    st, key = env.reset(gpu.prng_key(7)), gpu.prng_key(8)

    def run():
        plan = Plan(env, a)
        plan.set_state0(st)
        plan.set_ensemble(members, "mean")
        mu, rm, rf, _ = plan.run(key)
        out = [np.asarray(mu), np.asarray(rm), np.float32(rf)] + list(plan.peek()) + list(plan.peek_ensemble())
        plan.close()
        return out

    one = run()
    r_members = one[-2]
    assert not np.array_equal(r_members[0], r_members[1]), "the scaled member computes other rewards"
    levers(MBD_ENS_SPLIT=1)
    split = run()
    for k, (x, y) in enumerate(zip(one, split)):
        same_bits(x, y, f"{name}: output {k} of the one-launch ensemble against one launch per member")
