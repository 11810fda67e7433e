"""-m gpu: the adapt record on the device (include/mbd_hip.h mbd_adapt, DESIGN.md section 1 "N17 adapt") against the checker
(tests/adapt_checker.py) by bit pattern.

  the update alone   mbd_debug_adapt_step — the table kernel, adapt_spread_kernel, adapt_finish_kernel — at N in {1, 33, 64, 70,
                     1029, 4100} x HNu in {12, 21, 32, 85}: ragged tiles, empty and ragged groups, the unrolled rounds; lazy normals
                     with sigma from the host and values with sigma from a device scalar; weights with exact zeros, all equal, in
                     tied pairs, all on one candidate (skipped); a frozen column; HNu = 2100, beyond one chunk of the sum of S;
                     N = 12289 and 12300, beyond the weights the spread kernel stages in LDS (its other instantiation)
  whole plans        hopper, ant, humanoidrun, car2d at Ndiffuse = 6, MBD and mppi, with and without a noise shape, a noise basis,
                     a weighting record with an ESS target: mu_0ts, the table and the S log of every step; no step skipped
  identity           a_min = a_max = 1, and a record set and cleared: the bits of the plan without one
  episodes           T = 3, K = 2, E = 2: carry 0 and 1, a MBD_NOISE_WARM_TICKS shape, a delay record, a pick record, mppi; a session
                     fed the episode's states returns its means and tables; reset_mean resets the table
  phase calls        mbd_plan_reverse_once step by step, the shape set behind the record; after an episode under a warm-only shape
  composition        objective and plant records beside the record
  refusals           a sharded plan, an open session, cma-es, a demo plan"""
import functools

import numpy as np
import pytest

import adapt_cases as cases
import adapt_checker as ac
from state_inputs import same_bits
from test_adapt import BIG_N, HOST_HNU, KINDS, NU_OF, RULE, WIDE_HNU, assert_step, checked, step_case

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def gpu(lib):
    from mbd_hip import _capi
    if _capi.device_count() < 1:
        pytest.fail("tests/test_gpu_adapt.py needs a GPU")
    return _capi


@functools.lru_cache(maxsize=None)
def _env(name):
    from mbd_hip.envs import get_env
    return get_env(name)


def _oenv(orc, env):
    from oracle import planner as op
    if env.__class__.__name__ == "Car2d":
        return op.OracleEnv(orc, "car2d", xref=env.xref, rew_xref=env.rew_xref)
    return op.OracleEnv(orc, env.env_name, env.sys.to_struct(), xref=env.xref, rew_xref=env.rew_xref, init_q=env.sys.init_q)


def _impl():
    from mbd_hip.envs.base import prng_impl
    return prng_impl()


def _state(st):
    return np.asarray(st.pipeline_state, f32).reshape(-1)


def _plan(gpu, name, method=0, **plan_kw):
    """(env, plan, state0) of a case's sizes from reset(prng_key(3)), no record set."""
    from mbd_hip.planners.mbd_planner import Plan
    N, H, _ = cases.SIZES[name]
    env = _env(name)
    if method:
        from mbd_hip.planners.path_integral import Args
        args = Args(env_name=name, Nsample=N, Hsample=H, Nrefine=cases.ND, temp_sample=cases.TEMP, disable_recommended_params=True)
    else:
        from mbd_hip.planners.mpc import MpcArgs
        args = MpcArgs(env_name=name, Nsample=N, Hsample=H, Ndiffuse=cases.ND, temp_sample=cases.TEMP, disable_recommended_params=True,
                       not_render=True)
    plan = Plan(env, args, update_method=method, **plan_kw)
    st = env.reset(gpu.prng_key(3))
    plan.set_state0(st)
    return env, plan, _state(st)


def _start_from(plan, s0):
    """The plan's start state set to s0 [S] (a case whose start is not the reset state)."""
    import types
    plan.set_state0(types.SimpleNamespace(pipeline_state=np.ascontiguousarray(s0, f32)))


def _same_log(plan, ref, what, a_ref):
    log = plan.peek_adapt()
    assert log["count"] == len(ref["log"]) == len(log["ratio"]), what
    for j, (S, skipped) in enumerate(ref["log"]):
        same_bits(log["ratio"][j], S, f"{what}: S of step {j}")
        assert int(log["skipped"][j]) == int(skipped) == 0, f"{what}: step {j} skipped"
    same_bits(log["a"], a_ref, f"{what}: the table")


# ---- the update alone ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 33, 64, 70, 1029, 4100])
def test_the_update_alone(gpu, orc, N):
    """The three launches on uploaded arrays, every kind of weights, under a shape with a frozen column and without one."""
    skipped = 0
    for HNu in HOST_HNU + (32,):
        for lazy, on_device in ((True, False), (False, True)):
            for kind in KINDS:
                for with_shape in (True, False):
                    c = step_case(N, HNu, lazy, kind, with_shape)
                    ref = checked(orc, c)
                    what = f"N={N} HNu={HNu} lazy={lazy} {kind} shape={with_shape}"
                    got = gpu.debug_adapt_step(c["w"], c["cand"], c["ybar"], c["sigma"], lazy, c["a"], c["g"], RULE.rate, RULE.a_min,
                                               RULE.a_max, sigma_on_device=on_device)
                    assert_step(got, ref, what)
                    if kind == "one" or N == 1:
                        assert got[3] == 1, f"{what}: one candidate carries all weight"
                        same_bits(got[0], c["a"], f"{what}: a skipped step leaves a as it was")
                    if with_shape:
                        col = np.arange(HNu) % NU_OF[HNu] == 1
                        same_bits(got[0][col], c["a"][col], f"{what}: a frozen column keeps its a")
                        assert (got[1][col].view(np.uint32) << 1 == 0).all(), f"{what}: a frozen column stays frozen"
                    skipped += got[3]
    assert skipped >= 8


def test_the_update_beyond_one_chunk_of_the_sum(gpu, orc):
    """HNu = 2100 > 2048: adapt_finish_kernel's sum of S crosses LDS in two chunks, and adapt_table_kernel and the parallel passes
    take nine blocks of 256 elements; 132 tiles of the spread kernel."""
    for lazy, on_device in ((True, False), (False, True)):
        for kind in ("equal", "one"):
            c = step_case(33, WIDE_HNU, lazy, kind)
            got = gpu.debug_adapt_step(c["w"], c["cand"], c["ybar"], c["sigma"], lazy, c["a"], c["g"], RULE.rate, RULE.a_min, RULE.a_max,
                                       sigma_on_device=on_device)
            assert_step(got, checked(orc, c), f"HNu={WIDE_HNU} lazy={lazy} {kind}")
            assert got[3] == int(kind == "one")


@pytest.mark.parametrize("N", BIG_N)
def test_the_update_beyond_the_lds_window(gpu, orc, N):
    """More than 12288 candidates: adapt_spread_kernel<false>, whose threads read their weights from memory — one past the boundary
    (12289: one group has a candidate more than the others) and 12300 (ragged groups; every group enters the 32-row rounds)."""
    for HNu in (12, 21):
        for lazy, on_device in ((True, False), (False, True)):
            for kind in ("zeros", "equal"):
                c = step_case(N, HNu, lazy, kind)
                ref = checked(orc, c)
                got = gpu.debug_adapt_step(c["w"], c["cand"], c["ybar"], c["sigma"], lazy, c["a"], c["g"], RULE.rate, RULE.a_min,
                                           RULE.a_max, sigma_on_device=on_device)
                assert_step(got, ref, f"N={N} HNu={HNu} lazy={lazy} {kind}")
                assert got[3] == 0


# ---- whole plans -----------------------------------------------------------------------------------------------------------------
def _configure(plan, case):
    N, H, Nu = cases.SIZES[case.name]
    if getattr(case, "shape", False):
        plan.set_noise_shape(cases.plan_shape(H, Nu), case.shape if isinstance(case.shape, str) else "always")
    if getattr(case, "knots", 0):
        from noise_basis_checker import basis_of
        plan.set_noise_basis(basis_of(H, case.knots), "always")
    if getattr(case, "ess", False):
        plan.set_weighting(**case.wrec.kwargs())
    if getattr(case, "D", 0):
        plan.set_mpc_delay(case.D)
    if getattr(case, "pick", 0):
        plan.set_mpc_pick(True, True, True)
    if isinstance(case, cases.EpisodeCase) and case.method:
        plan.set_mpc_sigma(*cases.SIGMA)


@pytest.mark.parametrize("case", cases.PLAN_CASES, ids=[c.id for c in cases.PLAN_CASES])
def test_whole_plans(gpu, orc, case):
    """mbd_plan_run under the record: mu_0ts, the table behind the run and the S of every step; no step skipped."""
    env, plan, s0 = _plan(gpu, case.name, case.method)
    try:
        if case.state0 is not None:
            s0 = case.state0
            _start_from(plan, s0)
        _configure(plan, case)
        plan.set_adapt(**RULE.kwargs())
        key = gpu.prng_key(4)
        mu = plan.run(key)[0]
        ref = cases.plan_reference(orc, _oenv(orc, env), s0, key, case, _impl())
        same_bits(mu, ref["mu_0ts"], f"{case.id}: mu_0ts")
        _same_log(plan, ref, case.id, ref["tables"][-1].reshape(mu.shape[1:]))
        mu2 = plan.run(key)[0]  # (a second run starts from ones again)
        same_bits(mu2, mu, f"{case.id}: a second run")
    finally:
        plan.close()


# ---- identity --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,method,shape", [("hopper", 0, True), ("humanoidrun", 0, False), ("car2d", 0, True), ("hopper", 1, False)])
def test_identity(gpu, name, method, shape):
    """a_min = a_max = 1 keeps the bits of the plan without a record, run and episode; so does a record set and cleared; and a
    record that is free to move changes them."""
    env, plan, _ = _plan(gpu, name, method)
    N, H, Nu = cases.SIZES[name]
    try:
        if shape:
            plan.set_noise_shape(cases.plan_shape(H, Nu), "always")
        if method:
            plan.set_mpc_sigma(*cases.SIGMA)
        key = gpu.prng_key(4)
        mu0, rm0 = plan.run(key)[:2]
        ep0 = plan.run_mpc(key, cases.T, cases.K, cases.E)
        plan.set_adapt(0.5, 1.0, 1.0, True)
        mu1, rm1 = plan.run(key)[:2]
        same_bits(mu1, mu0, "a_min = a_max = 1: mu_0ts")
        same_bits(rm1, rm0, "a_min = a_max = 1: mean rewards")
        log = plan.peek_adapt()
        assert (log["a"] == 1).all() and log["count"] == cases.ND - 1 and not log["skipped"].any()
        ep1 = plan.run_mpc(key, cases.T, cases.K, cases.E)
        for k in ("means", "actions", "states", "rewards"):
            same_bits(ep1[k], ep0[k], f"a_min = a_max = 1: the episode's {k}")
        plan.set_adapt(**RULE.kwargs())
        assert not np.array_equal(plan.run(key)[0], mu0), "a record that may move changes the plan"
        plan.clear_adapt()
        mu2, rm2 = plan.run(key)[:2]
        same_bits(mu2, mu0, "set and cleared: mu_0ts")
        same_bits(rm2, rm0, "set and cleared: mean rewards")
        with pytest.raises(gpu.MbdError) as e:
            plan.peek_adapt()
        assert e.value.code == gpu.MBD_ERR_STATE
    finally:
        plan.close()


# ---- episodes and sessions ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.EPISODE_CASES, ids=[c.id for c in cases.EPISODE_CASES])
def test_episodes_and_sessions(gpu, orc, case):
    """mbd_plan_run_mpc under the record against the checker's episode: the logs, the table behind the last tick, the S of every
    step; then a session fed the episode's states: its means and the table behind every tick."""
    env, plan, s0 = _plan(gpu, case.name, case.method)
    T, K, E = cases.T, cases.K, cases.E
    try:
        _configure(plan, case)
        plan.set_adapt(**dict(RULE.kwargs(), carry=case.carry))
        key = gpu.prng_key(4)
        ep = plan.run_mpc(key, T, K, E)
        ref = cases.episode_reference(orc, _oenv(orc, env), s0, key, case, _impl())
        for k in ("means", "actions", "states", "rewards"):
            same_bits(ep[k], np.asarray(ref[k], f32).reshape(np.shape(ep[k])), f"{case.id}: {k}")
        _same_log(plan, ref, case.id, ref["tables"][-1])
        with plan.mpc_open(key, K, E) as s:
            for t in range(T):
                out = s.tick(ep["states"][t])
                same_bits(out["mean"], ep["means"][t], f"{case.id}: the session's mean of tick {t}")
                same_bits(plan.peek_adapt()["a"], ref["tables"][t], f"{case.id}: the session's table behind tick {t}")
            assert plan.peek_adapt()["count"] == len(ref["log"])
    finally:
        plan.close()


@pytest.mark.parametrize("method", [0, 1], ids=["mbd", "mppi"])
def test_reset_mean_resets_the_table(gpu, orc, method):
    """A session with reset_mean in front of its third tick against the checker's: the table is all ones right after the call, and
    the cold tick that follows, and its table, are the checker's."""
    case = cases.EpisodeCase(method=method, carry=True, shape="always")
    env, plan, s0 = _plan(gpu, case.name, method)
    N, H, Nu = cases.SIZES[case.name]
    try:
        _configure(plan, case)
        plan.set_adapt(**RULE.kwargs())
        key = gpu.prng_key(4)
        states = [s0, s0, s0]
        ref = ac.Session(_oenv(orc, env), key, N, H, cases.ND, cases.TEMP, cases.K, cases.E, cases.state_of(case),
                         method=1 if method else None, sigma=cases.SIGMA, impl=_impl())
        with plan.mpc_open(key, cases.K, cases.E) as s:
            for t, x in enumerate(states):
                if t == 2:
                    s.reset_mean()
                    ref.reset_mean()
                    assert (plan.peek_adapt()["a"] == 1).all(), "reset_mean: the table is all ones"
                out, want = s.tick(x), ref.tick(x)
                same_bits(out["mean"], want["mean"], f"tick {t}: mean")
                same_bits(plan.peek_adapt()["a"], want["a"], f"tick {t}: table")
        assert not any(sk for _, sk in ref.state.log)
    finally:
        plan.close()


# ---- the phase calls -------------------------------------------------------------------------------------------------------------
def _reverse_once(gpu, plan, i, key, d_ybar):
    """mbd_plan_reverse_once on the device mean d_ybar (in place) with the key array ``key`` (advanced); the new mean [H, Nu]."""
    import torch
    rm = torch.zeros(1, device="cuda")
    gpu.check(plan.lib.mbd_plan_reverse_once(plan.h, i, key, d_ybar.data_ptr(), rm.data_ptr(), None))
    torch.cuda.synchronize()
    return d_ybar.cpu().numpy().reshape(plan.H, plan.Nu)


@pytest.mark.parametrize("name", ["hopper", "car2d"])
def test_phase_calls_step_by_step(gpu, orc, name):
    """mbd_plan_reverse_once at i = 5, 4, 3 with a record — lazy (hopper) and materialised (car2d) —, the noise shape set BEHIND the
    record (mbd_plan_set_noise_shape forms G again): every mean, the key chain, the table and the log are the checker's; the table
    persists between the calls."""
    import torch
    env, plan, s0 = _plan(gpu, name)
    N, H, Nu = cases.SIZES[name]
    try:
        plan.set_adapt(**RULE.kwargs())
        g = cases.plan_shape(H, Nu)
        plan.set_noise_shape(g, "always")
        same_bits(plan.peek_adapt()["a"], np.ones((H, Nu), f32), "a new shape leaves the table alone")
        st = ac.State(RULE, H, Nu, g, g)
        sched = plan.schedule()
        key = gpu.key_array(gpu.prng_key(4))
        r, Ybar = np.asarray(gpu.prng_key(4), np.uint32), np.zeros((H, Nu), f32)
        d_ybar = torch.zeros(H * Nu, device="cuda")
        oenv = _oenv(orc, env)
        for i in (5, 4, 3):
            got = _reverse_once(gpu, plan, i, key, d_ybar)
            r, Ybar, _, _ = ac.reverse_once(orc, oenv, s0, i, r, Ybar, sched, N, H, cases.TEMP, _impl(), state=st)
            same_bits(got, Ybar, f"{name}: the mean behind step {i}")
            assert list(key) == [int(x) for x in r], f"{name}: the key behind step {i}"
            same_bits(plan.peek_adapt()["a"], st.a, f"{name}: the table behind step {i}")
        log = plan.peek_adapt()
        assert log["count"] == 3 and not log["skipped"].any()
        for j, (S, _) in enumerate(st.log):
            same_bits(log["ratio"][j], S, f"{name}: S of call {j}")
        plan.clear_noise_shape()  # (cleared behind the record: G = a from here on)
        st.g_always = st.g_warm = st.g = None
        st._form()
        got = _reverse_once(gpu, plan, 2, key, d_ybar)
        r, Ybar, _, _ = ac.reverse_once(orc, oenv, s0, 2, r, Ybar, sched, N, H, cases.TEMP, _impl(), state=st)
        same_bits(got, Ybar, f"{name}: the mean behind step 2, the shape cleared")
    finally:
        plan.close()


def test_phase_calls_behind_an_episode_sample_under_the_shape_in_force(gpu):
    """A MBD_NOISE_WARM_TICKS shape enters G in the warm ticks only: behind an episode, and behind a session, mbd_plan_reverse_once
    samples flat again — with a_min = a_max = 1 the bits of the same calls on a plan without a record."""
    import torch
    N, H, Nu = cases.SIZES["hopper"]
    outs = []
    for with_record in (False, True):
        env, plan, _ = _plan(gpu, "hopper")
        try:
            plan.set_noise_shape(cases.plan_shape(H, Nu), "warm")
            if with_record:
                plan.set_adapt(0.5, 1.0, 1.0, True)
            ep = plan.run_mpc(gpu.prng_key(4), cases.T, cases.K, cases.E)
            d_ybar = torch.zeros(H * Nu, device="cuda")
            a = _reverse_once(gpu, plan, 3, gpu.key_array(gpu.prng_key(6)), d_ybar).copy()
            with plan.mpc_open(gpu.prng_key(4), cases.K, cases.E) as s:
                for t in range(2):
                    s.tick(ep["states"][t])
            b = _reverse_once(gpu, plan, 2, gpu.key_array(gpu.prng_key(7)), d_ybar).copy()
            outs.append((ep["means"], a, b))
        finally:
            plan.close()
    for x, y, what in zip(outs[0], outs[1], ("the episode's means", "reverse_once behind the episode", "reverse_once behind the session")):
        same_bits(y, x, what)


# ---- composition -----------------------------------------------------------------------------------------------------------------
def test_objective_and_plant_records_beside_the_record(gpu):
    """An episode under an objective record and a plant record with action noise: with a_min = a_max = 1 the bits of the episode
    without an adapt record; with a record that may move, other and finite means, no step skipped, the frozen element's a = 1."""
    from test_objective import gpu_record
    N, H, Nu = cases.SIZES["hopper"]
    env, plan, _ = _plan(gpu, "hopper")
    try:
        plan.set_objective(**gpu_record(H, Nu).kwargs())
        plan.set_mpc_plant(None, gpu.prng_key(8), act_std=0.05)
        plan.set_noise_shape(cases.plan_shape(H, Nu), "always")
        key = gpu.prng_key(4)
        ep0 = plan.run_mpc(key, cases.T, cases.K, cases.E)
        plan.set_adapt(0.5, 1.0, 1.0, True)
        ep1 = plan.run_mpc(key, cases.T, cases.K, cases.E)
        for k in ("means", "actions", "states", "rewards"):
            same_bits(ep1[k], ep0[k], f"a_min = a_max = 1: {k}")
        plan.set_adapt(**RULE.kwargs())
        ep2 = plan.run_mpc(key, cases.T, cases.K, cases.E)
        log = plan.peek_adapt()
        assert np.isfinite(ep2["means"]).all() and not np.array_equal(ep2["means"], ep0["means"])
        assert log["count"] == (cases.ND - 1) + (cases.T - 1) * cases.K and not log["skipped"].any()
        assert not (log["a"] == 1).all()
    finally:
        plan.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_that_need_a_device(gpu):
    """A sharded plan and an open session: MBD_ERR_STATE; cma-es and a demo plan: MBD_ERR_UNSUPPORTED; with a record the prefetch
    call is accepted and does nothing."""
    import ctypes as C
    from mbd_hip.planners.mbd_planner import Args, Plan
    N, H, _ = cases.SIZES["hopper"]
    env, plan, _ = _plan(gpu, "hopper")
    try:
        with plan.mpc_open(gpu.prng_key(4), cases.K, cases.E):
            for call in (lambda: plan.set_adapt(**RULE.kwargs()), plan.clear_adapt):
                with pytest.raises(gpu.MbdError) as e:
                    call()
                assert e.value.code == gpu.MBD_ERR_STATE and "session" in str(e.value)
        plan.set_adapt(**RULE.kwargs())
        mu = plan.run(gpu.prng_key(4))[0]
        gpu.check(plan.lib.mbd_plan_prefetch_noise(plan.h, gpu.key_array(gpu.prng_key(9)), None))
        same_bits(plan.run(gpu.prng_key(4))[0], mu, "a declared key changes nothing")
        rec = gpu.adapt_record(0.5, 0.5, 2.0)
        rec.reserved[2] = 1
        assert plan.lib.mbd_plan_set_adapt(plan.h, C.byref(rec)) == gpu.MBD_ERR_INVALID and b"reserved[2]" in plan.lib.mbd_last_error()
        assert plan.peek_adapt()["count"] == cases.ND - 1  # (a refused set call leaves the record alone)
    finally:
        plan.close()
    env, shard, _ = _plan(gpu, "hopper", shard_begin=0, shard_count=N // 2)
    try:
        with pytest.raises(gpu.MbdError) as e:
            shard.set_adapt(**RULE.kwargs())
        assert e.value.code == gpu.MBD_ERR_STATE and "shard_count" in str(e.value)
    finally:
        shard.close()
    env, cma, _ = _plan(gpu, "hopper", method=2)
    try:
        with pytest.raises(gpu.MbdError) as e:
            cma.set_adapt(**RULE.kwargs())
        assert e.value.code == gpu.MBD_ERR_UNSUPPORTED and "update_method=2" in str(e.value)
    finally:
        cma.close()
    track = _env("humanoidtrack")
    demo = Plan(track, Args(env_name="humanoidtrack", Nsample=64, Hsample=50, Ndiffuse=3, enable_demo=True, disable_recommended_params=True,
                            not_render=True))
    try:
        with pytest.raises(gpu.MbdError) as e:
            demo.set_adapt(**RULE.kwargs())
        assert e.value.code == gpu.MBD_ERR_UNSUPPORTED and "enable_demo" in str(e.value)
    finally:
        demo.close()


def test_the_python_layer_maps_every_flag(gpu):
    """mpc.run_mpc and run_mpc_online under the adapt flags against the Plan path with the record written out by hand: the same
    means and the same table, so every flag reaches its field (the CPU tests show the checker tells the fields apart)."""
    from dataclasses import replace

    from mbd_hip.planners import mpc
    N, H, _ = cases.SIZES["hopper"]
    T, K, E = cases.T, cases.K, cases.E
    base = mpc.MpcArgs(env_name="hopper", Nsample=N, Hsample=H, Ndiffuse=cases.ND, temp_sample=cases.TEMP, disable_recommended_params=True,
                       not_render=True, seed=2, n_ticks=T, warm_steps=K, exec_steps=E)
    args = replace(base, adapt_rate=0.5, adapt_min=0.5, adapt_max=2.0, adapt_carry=True)
    env, plan, state_init, key = mpc._setup(replace(base), 0)
    try:
        plan.set_adapt(**RULE.kwargs())
        ref = plan.run_mpc(key, T, K, E)
        ref_log = plan.peek_adapt()
    finally:
        plan.close()
    _, det = mpc.run_mpc(replace(args), return_details=True)
    same_bits(det["means"], ref["means"], "mpc.run_mpc: means")
    same_bits(det["adapt"]["a"], ref_log["a"], "mpc.run_mpc: the table")
    same_bits(det["adapt"]["ratio"], ref_log["ratio"], "mpc.run_mpc: the log")
    assert det["adapt_rate"] == 0.5 and det["adapt_carry"] is True
    _, on = mpc.run_mpc_online(replace(args), return_details=True)
    same_bits(on["means"], ref["means"], "mpc.run_mpc_online: means")
    same_bits(on["adapt"]["a"], ref_log["a"], "mpc.run_mpc_online: the table")
    _, plain = mpc.run_mpc(replace(base), return_details=True)
    assert "adapt" not in plain and "adapt_rate" not in plain
