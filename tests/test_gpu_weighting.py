"""-m gpu: the weighting record on the device (include/mbd_hip.h mbd_weighting, DESIGN.md section 1 "N14 weighting") against the
checker (tests/weighting_checker.py) by bit pattern: weigh_kernel through the phase calls at every size and case of
tests/weighting_inputs.py under all four update methods, whole runs, sweeps against their plans run alone, closed loops and sessions,
and the set call's refusals."""
import functools

import numpy as np
import pytest

import weighting_checker as wc
import weighting_inputs as wi
from state_inputs import same_bits

pytestmark = pytest.mark.gpu

H = 4
TABLE = wi.table()


@pytest.fixture(scope="module")
def gpu(lib):
    from mbd_hip import _capi
    if _capi.device_count() < 1:
        pytest.fail("tests/test_gpu_weighting.py needs a GPU")
    return _capi


@functools.lru_cache(maxsize=None)
def _env(name):
    from mbd_hip.envs import get_env
    return get_env(name)


def _oenv(orc, env):
    from oracle import planner as op
    return op.OracleEnv(orc, env.env_name, env.sys.to_struct(), xref=env.xref, rew_xref=env.rew_xref, init_q=env.sys.init_q)


def _args(name, N, Nd, method=0, temp=0.1, **kw):
    if method:
        from mbd_hip.planners.path_integral import Args
        return Args(env_name=name, Nsample=N, Hsample=H, Nrefine=Nd, temp_sample=temp, disable_recommended_params=True, **kw)
    from mbd_hip.planners.mpc import MpcArgs
    return MpcArgs(env_name=name, Nsample=N, Hsample=H, Ndiffuse=Nd, temp_sample=temp, disable_recommended_params=True,
                   not_render=True, **kw)


def _impl():
    from mbd_hip.envs.base import prng_impl
    return prng_impl()


@functools.lru_cache(maxsize=None)
def _checked(orc, k):
    c = TABLE[k]
    return wc.weigh(orc, c.rews, c.temp, c.rec)


class _Step:
    """A plan with resident candidates, ready for mbd_plan_score_update on the caller's rewards (test_gpu_pi_updates._Step)."""

    def __init__(self, gpu, name, N, method):
        import torch
        from mbd_hip.planners.mbd_planner import Plan
        self.gpu, self.torch, self.method, self.N, self.i = gpu, torch, method, N, 3
        env = _env(name)
        self.Nu = env.action_size
        self.plan = Plan(env, _args(name, N, 8, method, temp=wi.TEMP), update_method=method)
        self.plan.set_state0(env.reset(gpu.prng_key(3)))
        self.sched = self.plan.schedule()
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
        """(new mean [H][Nu], weights [N], mean reward) of one score + update on the uploaded rewards."""
        torch = self.torch
        if self.method:
            self.plan.set_sigma(0.7)
        d_r = torch.tensor(rews, device="cuda")
        out, rm = torch.full((H * self.Nu,), 7.0, device="cuda"), torch.zeros(1, device="cuda")
        self.gpu.check(self.plan.lib.mbd_plan_score_update(self.plan.h, self.i, self.ks, self.d_mu.data_ptr(), d_r.data_ptr(), None,
                                                           out.data_ptr(), rm.data_ptr(), None))
        torch.cuda.synchronize()
        return out.cpu().numpy().reshape(H, self.Nu), self.plan.peek()[2], np.float32(rm.item())


@pytest.mark.parametrize("N", wi.SIZES)
@pytest.mark.parametrize("method", [0, 1, 2, 3])
def test_phase_calls_at_every_size(gpu, orc, method, N):
    """mbd_plan_sample_rollout once, then mbd_plan_score_update on every case's rewards (the caller's buffer, as the sharded path
    hands it over): the weights, the new mean, rew_mean and the log entry equal the checker fed the peeked candidates.  For the
    planted cases the same call without a record gives a non-finite mean — today's behaviour, the failure the record removes."""
    step = _Step(gpu, "hopper" if N <= 1025 else "cartpole", N, method)
    try:
        n = 0
        for k, c in enumerate(TABLE):
            if c.N != N:
                continue
            what = f"method {method} {c.id}"
            if c.name == "planted":
                step.plan.clear_weighting()
                mu, w, _ = step.update(c.rews)
                assert np.isnan(w).all(), f"{what}: without a record a planted reward should reach every weight"
                if method != 3:  # (cem's mean of ten candidates is finite whatever the weights: it then selects by index alone)
                    assert not np.isfinite(mu).any(), f"{what}: without a record a planted reward should reach the mean"
            step.plan.set_weighting(**c.rec.kwargs())
            mu, w, rm = step.update(c.rews)
            ref = _checked(orc, k)
            log = step.plan.peek_weighting()
            assert len(log["temp"]) == len(log["ess"]) == len(log["kept"]) == 1, what
            same_bits(w, ref["weights"], f"{what}: weights")
            same_bits(log["temp"][0], ref["temp"], f"{what}: logged temperature")
            same_bits(log["ess"][0], ref["ess"], f"{what}: logged ess")
            assert int(log["kept"][0]) == ref["kept"], what
            if ref["kept"] == 0:
                assert np.isnan(rm), what
            else:
                same_bits(rm, ref["rew_mean"], f"{what}: mean reward")
            mu_ref = wc.update(orc, method, ref["weights"], step.Y0s, step.mu, step.sched, step.i)
            if ref["kept"] or method == 3:
                assert np.isfinite(mu).all(), f"{what}: the mean is not finite"
            assert np.array_equal(mu, mu_ref, equal_nan=True), f"{what}: the new mean"
            n += 1
        assert n == len(wi.cases(N))
    finally:
        step.plan.close()


def test_whole_run_under_an_ess_target(gpu, orc):
    """mbd_plan_run, N = 96, Ndiffuse = 5, ess_frac = 0.25: the checker's run; four log entries, every T* inside the bracket."""
    from mbd_hip.planners.mbd_planner import Plan
    env, N, Nd = _env("cartpole"), 96, 5
    st = env.reset(gpu.prng_key(3))
    plan = Plan(env, _args("cartpole", N, Nd))
    try:
        plan.set_state0(st)
        plan.set_weighting(**wi.ESS.kwargs())
        key = gpu.prng_key(7)
        mu, rm, _, _ = plan.run(key)
        log = plan.peek_weighting()
        ref = wc.run(orc, _oenv(orc, env), np.asarray(st.pipeline_state, np.float32).reshape(-1), key, N, H, Nd, 0.1, wi.ESS, _impl())
        same_bits(mu, ref["mu_0ts"], "mu_0ts")
        same_bits(rm, ref["rew_means"], "mean rewards")
        assert len(log["temp"]) == Nd - 1
        for j, (T, ess, kept) in enumerate(ref["log"]):
            same_bits(log["temp"][j], T, f"step {j}: temperature")
            same_bits(log["ess"][j], ess, f"step {j}: ess")
            assert int(log["kept"][j]) == kept == N
            assert np.float32(wi.ESS.temp_min) <= log["temp"][j] <= np.float32(wi.ESS.temp_max)
    finally:
        plan.close()


@pytest.mark.parametrize("method", [0, 1, 2, 3])
@pytest.mark.parametrize("P", [3, 8])
def test_sweeps_equal_their_plans_alone(gpu, method, P):
    """P plans with distinct temperatures and one record in one sweep: plan k's run and log are the single plan's with that
    temperature and record, bit for bit (MBD, mppi, cma-es and cem; P = 8: the plan-to-XCD mapping)."""
    from mbd_hip.planners.mbd_planner import Plan, Sweep
    name = "hopper"
    env, N, Nd = _env(name), 80, 4
    temps = [0.05 + 0.1 * k for k in range(P)]
    keys = np.stack([gpu.prng_key(20 + k) for k in range(P)])
    states = [env.reset(gpu.prng_key(k)) for k in range(P)]
    sweep = Sweep(env, _args(name, N, Nd, method), P, temps=temps, update_method=method)
    try:
        for k in range(P):
            sweep.set_state0(k, states[k])
        sweep.set_weighting(**wi.ESS.kwargs())
        mu, rm, _, _ = sweep.run(keys)
        logs = [sweep.peek_weighting(k) for k in range(P)]
    finally:
        sweep.close()
    for k in range(P):
        plan = Plan(env, _args(name, N, Nd, method, temp=temps[k]), update_method=method)
        try:
            plan.set_state0(states[k])
            plan.set_weighting(**wi.ESS.kwargs())
            mu1, rm1, _, _ = plan.run(keys[k])
            log1 = plan.peek_weighting()
        finally:
            plan.close()
        same_bits(mu[k], mu1, f"plan {k}: mu_0ts")
        same_bits(rm[k], rm1, f"plan {k}: mean rewards")
        assert len(log1["temp"]) == Nd - 1
        for f in ("temp", "ess", "kept"):
            assert np.array_equal(logs[k][f], log1[f]), f"plan {k}: log {f}"


def test_closed_loop_and_sessions(gpu, orc):
    """A 3-tick episode under a record equals mpc_checker's episode with the checker in the score's place; a session fed that
    episode's states returns its means; so does a sweep's session; the log after a warm tick has warm_steps entries."""
    from mbd_hip.planners.mbd_planner import Plan, Sweep
    env, N, Nd, T, K, E = _env("cartpole"), 64, 5, 3, 2, 1
    st = env.reset(gpu.prng_key(3))
    s0 = np.asarray(st.pipeline_state, np.float32).reshape(-1)
    key = gpu.prng_key(5)
    plan = Plan(env, _args("cartpole", N, Nd))
    try:
        plan.set_state0(st)
        plan.set_weighting(**wi.ESS.kwargs())
        ep = plan.run_mpc(key, T, K, E)
        log = plan.peek_weighting()
        ref = wc.episode(_oenv(orc, env), s0, key, N, H, Nd, 0.1, T, K, E, wi.ESS, _impl())
        same_bits(ep["means"], ref["means"], "means")
        same_bits(ep["actions"], ref["actions"], "actions")
        same_bits(ep["states"], ref["states"], "states")
        assert len(log["temp"]) == K
        for j, (Ts, ess, kept) in enumerate(ref["log"][-1]):
            same_bits(log["temp"][j], Ts, f"last tick, step {j}: temperature")
            same_bits(log["ess"][j], ess, f"last tick, step {j}: ess")
            assert int(log["kept"][j]) == kept
        with plan.mpc_open(key, K, E) as s:
            means = np.stack([s.tick(ep["states"][t])["mean"] for t in range(T)])
            assert len(plan.peek_weighting()["temp"]) == K
        same_bits(means, ep["means"], "the session's means")
    finally:
        plan.close()
    P = 2
    sweep = Sweep(env, _args("cartpole", N, Nd), P)
    try:
        sweep.set_weighting(**wi.ESS.kwargs())
        with sweep.mpc_open(np.stack([key] * P), K, E) as s:
            means = np.stack([s.tick(np.stack([ep["states"][t]] * P))["mean"] for t in range(T)])
        for k in range(P):
            same_bits(means[:, k], ep["means"], f"the sweep session's means, episode {k}")
    finally:
        sweep.close()


def test_set_clear_and_refusals(gpu):
    """Set then clear leaves the next run's bits equal to a fresh plan's; an enable_demo plan is refused with MBD_ERR_UNSUPPORTED;
    setting a record with a session open gives MBD_ERR_STATE; the MBD_ERR_INVALID messages name the field."""
    import ctypes as C
    from mbd_hip.planners.mbd_planner import Plan
    env, N, Nd = _env("cartpole"), 64, 4
    st = env.reset(gpu.prng_key(3))
    key = gpu.prng_key(9)
    fresh = Plan(env, _args("cartpole", N, Nd))
    plan = Plan(env, _args("cartpole", N, Nd))
    try:
        fresh.set_state0(st)
        plan.set_state0(st)
        mu0, rm0, _, _ = fresh.run(key)
        plan.set_weighting(**wi.ESS.kwargs())
        mu1, _, _, _ = plan.run(key)
        assert not np.array_equal(mu1, mu0)  # (the record does something)
        plan.clear_weighting()
        mu2, rm2, _, _ = plan.run(key)
        same_bits(mu2, mu0, "after clear: mu_0ts")
        same_bits(rm2, rm0, "after clear: mean rewards")
        with pytest.raises(gpu.MbdError) as e:
            plan.peek_weighting()
        assert e.value.code == gpu.MBD_ERR_STATE
        # rejection alone, nothing dropped: the bits of the plan without a record
        plan.set_weighting(reject_nonfinite=True)
        mu3, rm3, _, _ = plan.run(key)
        same_bits(mu3, mu0, "rejection only: mu_0ts")
        same_bits(rm3, rm0, "rejection only: mean rewards")
        for kw, field in ((dict(reject_nonfinite=3), "reject_nonfinite"), (dict(ess_frac=2.0), "ess_frac"),
                          (dict(ess_frac=0.5, temp_min=-1.0, temp_max=1.0), "temp_min"),
                          (dict(ess_frac=0.5, temp_min=1.0, temp_max=0.5), "temp_max"),
                          (dict(ess_frac=0.5, temp_min=0.1, temp_max=1.0, iters=40), "iters")):
            with pytest.raises(gpu.MbdError) as e:
                plan.set_weighting(**kw)
            assert e.value.code == gpu.MBD_ERR_INVALID and field in str(e.value), (kw, str(e.value))
        rec = gpu.weighting_record()
        rec.reserved[0] = 5
        assert plan.lib.mbd_plan_set_weighting(plan.h, C.byref(rec)) == gpu.MBD_ERR_INVALID
        assert b"reserved[0]" in plan.lib.mbd_last_error()
        with plan.mpc_open(key, 1, 1):
            with pytest.raises(gpu.MbdError) as e:
                plan.set_weighting()
            assert e.value.code == gpu.MBD_ERR_STATE
    finally:
        plan.close()
        fresh.close()
    track = _env("humanoidtrack")
    from mbd_hip.planners.mbd_planner import Args
    demo = Plan(track, Args(env_name="humanoidtrack", Nsample=64, Hsample=50, Ndiffuse=3, enable_demo=True, disable_recommended_params=True,
                            not_render=True))
    try:
        with pytest.raises(gpu.MbdError) as e:
            demo.set_weighting()
        assert e.value.code == gpu.MBD_ERR_UNSUPPORTED
    finally:
        demo.close()


def test_the_python_layer_maps_every_field(gpu):
    """mpc.run_mpc, run_mpc_online and run_mpc_batch under the weighting flags against the Plan path with the record written out by
    hand: the same means bit for bit and the same log, so every flag reaches its field (a bracket or an iteration count that did not
    would move T*).  ``weighting_last_tick`` is the last tick's steps; the online episode's ``weighting`` has one entry per tick,
    each tick's last step."""
    from dataclasses import replace
    from mbd_hip.planners import mpc
    T, K, E = 3, 2, 1
    flags = dict(reject_nonfinite=True, ess_frac=0.3, temp_min=0.02, temp_max=5.0, ess_iters=7)
    rec = dict(reject_nonfinite=True, ess_frac=0.3, temp_min=0.02, temp_max=5.0, iters=7)
    base = replace(_args("cartpole", 64, 5), seed=2, n_ticks=T, warm_steps=K, exec_steps=E)
    args = replace(base, **flags)
    env, plan, state_init, key = mpc._setup(replace(base), 0)
    try:
        plan.set_weighting(**rec)
        ref = plan.run_mpc(key, T, K, E)
        ref_log = plan.peek_weighting()
        plan.set_weighting(**dict(rec, iters=6))  # (the episode can tell the fields apart: one bisection step fewer moves T*)
        plan.run_mpc(key, T, K, E)
        assert not np.array_equal(plan.peek_weighting()["temp"], ref_log["temp"])
        plan.set_weighting(**dict(rec, temp_max=4.0))
        plan.run_mpc(key, T, K, E)
        assert not np.array_equal(plan.peek_weighting()["temp"], ref_log["temp"])
    finally:
        plan.close()
    assert len(ref_log["temp"]) == K
    _, det = mpc.run_mpc(replace(args), return_details=True)
    same_bits(det["means"], ref["means"], "mpc.run_mpc: means")
    for f in ("temp", "ess", "kept"):
        assert np.array_equal(det["weighting_last_tick"][f], ref_log[f]), f"mpc.run_mpc: weighting_last_tick {f}"
    assert "weighting" not in det and det["ess_iters"] == 7 and det["temp_max"] == 5.0
    _, on = mpc.run_mpc_online(replace(args), return_details=True)
    same_bits(on["means"], ref["means"], "mpc.run_mpc_online: means")
    assert "weighting_last_tick" not in on and all(len(on["weighting"][f]) == T for f in ("temp", "ess", "kept"))
    for f in ("temp", "ess", "kept"):  # (the last tick's last step is the log's last entry)
        assert on["weighting"][f][-1] == ref_log[f][-1], f"mpc.run_mpc_online: weighting {f}"
    _, dets = mpc.run_mpc_batch([replace(args), replace(args, seed=3)], return_details=True)
    same_bits(dets[0]["means"], ref["means"], "mpc.run_mpc_batch: episode 0's means")
    assert dets[1]["ess_iters"] == 7 and dets[1]["temp_min"] == 0.02
    _, plain = mpc.run_mpc(replace(base), return_details=True)
    assert "weighting_last_tick" not in plain and "ess_frac" not in plain
