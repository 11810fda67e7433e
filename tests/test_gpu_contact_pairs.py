"""-m gpu: stage (4) of the one-collider humanoid kernels — contact detection, the position solve, its friction test — case by
case against the checker, bit for bit.

The start states are tests/contact_pair_inputs.py's (pipeline_init(q, qd) through the C ABI): both shin spheres in the air, one
resting (the stick side of the friction test), one sliding (the slip side), both in contact, one touching exactly
(penetration 0: inactive), one a single float below that, a start without tangential motion (ct2 == 0: the 1e-20 of the
denominator), and 2 cm of penetration.  tests/test_contact_pair_cases.py shows on the CPU that the checker reaches each
of them in the first substep.  A launch is one or two wavefronts (N = 4 fills one, N = 5 starts a second), H = 2 or 3; the
spheres sit on two links, so one wavefront holds the cases of both on different lanes, next to the lanes of the nine links
without a collider (whose collider offset is a zero vector: its rotation gives exact zeros of either sign).  Rewards and
final link states of mbd_env_rollout are compared with the checker's rollout(..., want_final=True) by bit pattern."""
import numpy as np
import pytest

import contact_pair_inputs as cp
from state_inputs import same_bits

pytestmark = pytest.mark.gpu

CASES = tuple(cp.EXPECT)


@pytest.fixture(scope="module")
def gpu(lib):
    from mbd_hip import _capi
    if _capi.device_count() < 1:
        pytest.fail("tests/test_gpu_contact_pairs.py needs a GPU")
    return _capi


def _env(name):
    from mbd_hip.envs import get_env
    from mbd_hip.envs.base import RigidBodyEnv
    if name in ("humanoidrun", "humanoidtrack"):
        return get_env(name)
    m, env_name = cp.variant(name)
    return RigidBodyEnv(env_name, model=m)


def _run_case(gpu, orc, name, env, case, b, h, kernel_args):
    from mbd_hip.envs.base import State
    m, _ = cp.variant(name)
    ms = m.to_struct()
    choice = gpu.debug_rollout_choice(ms, 256, b, h)["name"]
    assert f"rollout_kernel<16, true, false, 3, 1, 1, -4, -6, 0, false, true, 3, false, false, {kernel_args}," in choice, choice
    q, qd = next((q, qd) for c, q, qd in cp.cases(name) if c == case)
    s0 = env.pipeline_init(q, qd)
    want = orc.forward(ms, q, qd)  # (the state tests/test_contact_pair_cases.py classified)
    assert np.array_equal(np.asarray(s0, np.float32).reshape(want.shape), want), f"{name} {case}: pipeline_init"
    us = cp.actions(m, b, h)
    rew, fin = orc.rollout(ms, s0, us, want_final=True)
    out = env.rollout(State(np.asarray(s0, np.float32), None, np.float32(0.0), np.float32(0.0), {}), us, want_final=True)
    same_bits(out[0].cpu().numpy(), rew, f"{name} {case} N={b} H={h}: rewards")
    same_bits(out[-1].cpu().numpy(), fin, f"{name} {case} N={b} H={h}: final states")


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("name,kernel_args", [("humanoidrun", "0, 7"), ("humanoidtrack", "3, 5")])
def test_stage4_case_by_case(gpu, orc, name, kernel_args, case):
    """The compiled-in instantiations of the two built-in humanoids; N = 4 / H = 2 and N = 5 / H = 3 in turn."""
    b, h = ((4, 2), (5, 3))[CASES.index(case) % 2]
    _run_case(gpu, orc, name, _env(name), case, b, h, kernel_args)


def test_stage4_generic_instantiation(gpu, orc):
    """The humanoid with another reward kind: the instantiation without a compiled-in reward or substep count (RK = -1)."""
    env = _env("generic")
    for i, case in enumerate(CASES):
        b, h = ((5, 2), (4, 3))[i % 2]
        _run_case(gpu, orc, "generic", env, case, b, h, "-1, 0")


def test_stage4_five_substeps(gpu, orc):
    """humanoidrun with n_frames = 5: the substep loop with a run-time count."""
    env = _env("frames5")
    for i, case in enumerate(CASES):
        b, h = ((4, 2), (5, 3))[i % 2]
        _run_case(gpu, orc, "frames5", env, case, b, h, "-1, 0")
