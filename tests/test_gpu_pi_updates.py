"""-m gpu: the path-integral update kernels (update_method 1 / 2 / 3 = mppi / cma-es / cem) against the checker, by bit
pattern, at every size and reward shape of tests/pi_inputs.py.

Every other GPU test reaches these kernels through whole runs with organic rewards at N = 33, 128, 256: no exact tie between
weights, no N below ten, none around 64, 8192, 12 288 or 36 864 with std_guard = 0, no zero-spread rewards.  Here the update
step runs on its own: a path-integral `Plan`, `set_sigma`, `mbd_plan_sample_rollout` once to make the candidates resident,
then for every shape `mbd_plan_score_update` with the synthetic rewards uploaded, against `orc.pi_update` on the same arrays
— softmax weights, the new mean, the carried sigma, the mean reward.  The step under test ends at the update: nothing here
feeds a NaN mean to a rollout.

Comparisons are by bit pattern (state_inputs.same_bits).  The constant shapes and N = 1 (zero spread: NaN weights, DESIGN.md
numerics) are compared with equal_nan for mppi and cma-es — a NaN is a NaN, whatever its payload — and cem's mean, which is
finite there, bit for bit like everywhere else.
"""
import functools

import numpy as np
import pytest

import pi_inputs as pi
from state_inputs import same_bits

pytestmark = pytest.mark.gpu

# around every boundary: K = N below ten; one element per lane of the selection at 64; the score workgroup's 1024 threads;
# rewards in registers up to 8192; score + weighted mean in one launch up to 12 288; weights / logp0 in LDS up to 36 864
SIZES = (1, 2, 9, 10, 11, 63, 64, 65, 1000, 1024, 1025, 8192, 8193, 12288, 12289, 36864, 36865, 40001)
# H x Nu below 64 (one partial workgroup of the 64-output kernels), between 64 and 256, above 256 (two workgroups of the
# row-major weighted mean, six of the spread and cem mean kernels)
ENVS = (("cartpole", 7), ("hopper", 30), ("humanoidrun", 20))
SIGMA0 = 0.7


@pytest.fixture(scope="module")
def gpu(lib):
    from mbd_hip import _capi
    if _capi.device_count() < 1:
        pytest.fail("tests/test_gpu_pi_updates.py needs a GPU")
    return _capi


@functools.lru_cache(maxsize=None)
def _env(name):
    from mbd_hip.envs import get_env
    return get_env(name)


class _Step:
    """A path-integral plan of one temperature with resident candidates, ready for mbd_plan_score_update."""

    def __init__(self, gpu, name, H, N, method, temp):
        import torch
        from mbd_hip.planners.mbd_planner import Plan
        from mbd_hip.planners.path_integral import Args
        self.gpu, self.torch, self.method, self.temp = gpu, torch, method, temp
        env = _env(name)
        self.H, self.Nu, self.N, self.i = H, env.action_size, N, 3
        args = Args(env_name=name, Nsample=N, Hsample=H, Nrefine=8, temp_sample=temp, disable_recommended_params=True)
        self.plan = Plan(env, args, update_method=method)
        self.plan.set_state0(env.reset(gpu.prng_key(3)))
        self.plan.set_sigma(SIGMA0)
        g = np.random.default_rng([N, H, self.Nu])
        self.mu = (g.normal(size=(H, self.Nu)) * 0.3).astype(np.float32)
        self.d_mu = torch.tensor(self.mu.reshape(-1), device="cuda")
        self.ks = gpu.key_array(gpu.prng_key(N + 11))
        loc = torch.zeros(N, device="cuda")
        gpu.check(self.plan.lib.mbd_plan_sample_rollout(self.plan.h, self.i, self.ks, self.d_mu.data_ptr(), loc.data_ptr(), None, None))
        torch.cuda.synchronize()
        self.Y0s = self.plan.peek()[0]
        assert np.isfinite(self.Y0s).all() and np.abs(self.Y0s).max() <= 1.0

    def update(self, rews):
        """(new mean [H][Nu], sigma, weights [N], mean reward) of one update on the uploaded rewards."""
        torch = self.torch
        self.plan.set_sigma(SIGMA0)  # (cma-es updates it in place)
        d_r = torch.tensor(rews, device="cuda")
        out, rm = torch.full((self.H * self.Nu,), 7.0, device="cuda"), torch.zeros(1, device="cuda")
        self.gpu.check(self.plan.lib.mbd_plan_score_update(self.plan.h, self.i, self.ks, self.d_mu.data_ptr(), d_r.data_ptr(), None,
                                                           out.data_ptr(), rm.data_ptr(), None))
        torch.cuda.synchronize()
        return out.cpu().numpy().reshape(self.H, self.Nu), np.float32(self.plan.get_sigma()), self.plan.peek()[2], np.float32(rm.item())

    def close(self):
        self.plan.close()


def _compare(step, orc, name, rews, what):
    mu, sigma, w, rm = step.update(rews)
    mu_r, sigma_r, w_r, rm_r = orc.pi_update(step.method, rews, step.Y0s, step.mu, SIGMA0, step.temp)
    sigma_r, rm_r = np.float32(sigma_r), np.float32(rm_r)
    same_bits(rm, rm_r, f"{what}: mean reward")
    if name in pi.CONSTANT or step.N == 1:
        assert np.array_equal(w, w_r, equal_nan=True), f"{what}: weights"
        assert np.array_equal(sigma, sigma_r, equal_nan=True), f"{what}: sigma {sigma!r} against {sigma_r!r}"
        if step.method == 3:
            assert np.isfinite(mu_r).all(), what
            same_bits(mu, mu_r, f"{what}: cem mean")
        else:
            assert np.array_equal(mu, mu_r, equal_nan=True), f"{what}: mean"
    else:
        assert np.isfinite(w_r).all() and np.isfinite(mu_r).all() and np.isfinite(sigma_r), what
        same_bits(w, w_r, f"{what}: weights")
        same_bits(mu, mu_r, f"{what}: mean")
        same_bits(sigma, sigma_r, f"{what}: sigma")
    if step.method != 2:
        assert sigma == np.float32(SIGMA0), what


def _temps(N):
    return sorted({t for _, t, _ in pi.cases(N)})


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("name,H", ENVS)
@pytest.mark.parametrize("method", [1, 2, 3])
def test_pi_update_ragged_sizes(gpu, orc, method, name, H, N):
    """mbd_plan_score_update of a path-integral plan on its own — score_kernel / score_wmean_kernel with std_guard = 0, the
    row-major weighted mean, cma_spread_kernel, cma_sigma_kernel, cem_select_kernel, cem_mean_kernel — at candidate counts
    around every boundary of those kernels, three output counts H x Nu (7, 90, 340) and every reward shape and temperature
    of pi_inputs (exact ties within a lane and across lanes, underflowed weights, zero spread), against the checker bit for
    bit: weights, the new mean, sigma, the mean reward.  The N list is the same for all three envs: nothing is thinned (the
    whole matrix takes about ten seconds on the device)."""
    n = 0
    for temp in _temps(N):
        step = _Step(gpu, name, H, N, method, temp)
        try:
            for shape, t, rews in pi.cases(N):
                if t == temp:
                    _compare(step, orc, shape, rews, f"method {method} {name} N={N} {shape} temp={temp}")
                    n += 1
        finally:
            step.close()
    assert n == len(list(pi.cases(N)))


@pytest.mark.parametrize("N", [300, 8193])
@pytest.mark.parametrize("name,H", ENVS)
@pytest.mark.parametrize("method", [1, 2])
def test_pi_update_kernel_variants(gpu, orc, levers, method, name, H, N):
    """mppi and cma-es through the three forms of phase 2 — score + weighted mean in one launch (the default at these sizes),
    score_kernel + the tile weighted mean (MBD_NO_FUSED_SCORE=1, MBD_WMEAN_SPLIT=0), score_kernel + the row-major pair
    (MBD_WMEAN_SPLIT=1) — every shape, each against the checker bit for bit."""
    for temp in _temps(N):
        step = _Step(gpu, name, H, N, method, temp)
        try:
            for lv in (dict(MBD_NO_FUSED_SCORE=1), dict(MBD_WMEAN_SPLIT=0), dict(MBD_WMEAN_SPLIT=1),
                       dict(MBD_NO_FUSED_SCORE=1, MBD_WMEAN_SPLIT=0)):
                levers(**lv)
                for shape, t, rews in pi.cases(N):
                    if t == temp:
                        _compare(step, orc, shape, rews, f"method {method} {name} N={N} {shape} temp={temp} {lv}")
                levers(**{k: -1 for k in lv})
        finally:
            step.close()


@pytest.mark.parametrize("N", [1, 5, 10])
def test_pi_tiny_plans_whole_runs(gpu, orc, N):
    """cem with ten candidates or fewer (K = N; at N = 1 every weight of every step is NaN and the mean is Y0s[0]): whole runs
    of hopper, H = 12, Nrefine = 6, as a plan and as ONE sweep of three seeds (blockIdx.y > 0 of the selection and mean
    kernels), bit for bit against the checker's run.  mppi / cma-es at N = 1 are left out on purpose: their mean is NaN in
    the reference too, and what the rollout kernels do with NaN actions is not part of this work."""
    from mbd_hip.planners import path_integral
    from mbd_hip.scripts.run_mbd import run_path_integral_sweep
    from oracle import planner as op
    from oracle.planner import OracleEnv
    env = _env("hopper")
    oe = OracleEnv(orc, env.env_name, env.sys.to_struct(), xref=env.xref, rew_xref=env.rew_xref, init_q=env.sys.init_q)
    H, Nr, temp = 12, 6, 0.1
    plans = [path_integral.Args(seed=s, env_name="hopper", update_method="cem", Nsample=N, Hsample=H, Nrefine=Nr,
                                temp_sample=temp, disable_recommended_params=True) for s in (0, 1, 2)]
    refs = [op.run_path_integral(orc, oe, s, N, H, Nr, temp, "cem") for s in (0, 1, 2)]
    for a, ref in zip(plans, refs):
        assert np.isfinite(ref["mu_0ts"]).all() and np.isfinite(ref["rew_final"])
        rew, det = path_integral.run_path_integral(path_integral.Args(**vars(a)), return_details=True)
        same_bits(det["mu_0ts"], ref["mu_0ts"], f"plan N={N} seed={a.seed}: mu_0ts")
        same_bits(det["rew_means"], ref["rew_means"], f"plan N={N} seed={a.seed}: mean rewards")
        same_bits(np.float32(rew), np.float32(ref["rew_final"]), f"plan N={N} seed={a.seed}: final reward")
        assert np.float32(det["sigma_final"]) == np.float32(1.0)
    rews, _, det = run_path_integral_sweep(plans, return_details=True)
    assert det is not None  # (one sweep, not the plans in sequence)
    for k, ref in enumerate(refs):
        same_bits(det["mu_0ts"][k], ref["mu_0ts"], f"sweep N={N} plan {k}: mu_0ts")
        same_bits(det["rew_means"][k], ref["rew_means"], f"sweep N={N} plan {k}: mean rewards")
        same_bits(np.float32(rews[k]), np.float32(ref["rew_final"]), f"sweep N={N} plan {k}: final reward")
        assert np.float32(det["sigma_final"][k]) == np.float32(1.0)
