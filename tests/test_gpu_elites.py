"""-m gpu: the elite record on the device (include/mbd_hip.h mbd_elites, DESIGN.md section 1 "N18 elites") against the checker
(tests/elites_checker.py) by bit pattern.

  the launches alone  elite_inject_kernel and elite_select_kernel on uploaded arrays over the table of tests/elites_inputs.py: N in
                      {1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 8193, 12289} x k in {1, 5, 32}; all rewards equal, ties across the
                      wavefronts' and the workgroup's boundaries, +0 beside -0, planted non-finite entries, fewer finite entries
                      than k, none; lazy and materialised
  whole plans         hopper, ant, humanoidrun, car2d at Ndiffuse = 6, MBD and mppi, (n_elites, nominal) in {(3, 1), (1, 0), (0, 1),
                      (32, 1)}; a noise shape with a frozen element, a 3-knot basis, an ESS target, an adapt record beside
  other records       rejection on the hopper whose candidates really diverge, a two-member ensemble, an objective record with a
                      rate cost, a value record
  episodes            T = 3, K = 2, E = 2: both carry values, a delay record, pick mask 7, mppi under a sigma record, a plant of mass
                      1.3, car2d; a session fed the episode's states; reset_mean empties the elites
  phase calls         mbd_plan_reverse_once step by step against run
  identity            a record set and cleared: the bits of the plan without one
  refusals            a shard, an open session, cem, cma-es, a demo plan"""
import numpy as np
import pytest

import elites_checker as ec
import elites_inputs as inputs
from state_inputs import same_bits
from test_gpu_adapt import _env, _impl, _oenv, _plan, _reverse_once, _start_from

pytestmark = pytest.mark.gpu
f32 = np.float32
ND, TEMP, T, K, E = inputs.ND, inputs.TEMP, inputs.T, inputs.K, inputs.E


@pytest.fixture(scope="module")
def gpu(lib):
    from mbd_hip import _capi
    if _capi.device_count() < 1:
        pytest.fail("tests/test_gpu_elites.py needs a GPU")
    return _capi


def _same_elites(plan, ref, what):
    """The plan's elites and step log against the checker's state behind the same steps."""
    got = plan.peek_elites()
    assert got["count"] == len(ref["src"]), f"{what}: count {got['count']}, the checker {len(ref['src'])}"
    assert list(got["src"]) == list(ref["src"]), f"{what}: src"
    same_bits(got["R"], ref["R"], f"{what}: R")
    same_bits(got["E"], ref["E"], f"{what}: E")
    assert got["steps"] == len(ref["elog"]) == len(got["log_top"]), f"{what}: {got['steps']} steps, the checker {len(ref['elog'])}"
    for j, (count, kept, top) in enumerate(ref["elog"]):
        assert (int(got["log_count"][j]), int(got["log_kept"][j])) == (count, kept), f"{what}: step {j}: count and kept"
        same_bits(got["log_top"][j], top, f"{what}: step {j}: top")


# ---- the two launches alone --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", inputs.NS)
def test_the_two_launches_alone(gpu, N):
    """elite_inject_kernel, then elite_select_kernel over what it left, against the checker's step: every k and kind at this N, lazy
    and materialised; the sizes at which the record would be refused are refused."""
    cases = [c for c in inputs.table() if c["N"] == N]
    if N <= 2:
        bad = inputs.case(64, 1, "random", True)
        for call in (lambda: gpu.debug_elites_inject(bad["cand"][:N], bad["ybar"], bad["sigma"], True, None, 1, 1),
                     lambda: gpu.debug_elites_select(bad["rews"][:N], bad["cand"][:N], bad["ybar"], bad["sigma"], True, 1, 1)):
            with pytest.raises(gpu.MbdError) as e:
                call()
            assert e.value.code == gpu.MBD_ERR_INVALID and "must lie below N" in str(e.value)
    for c in cases:
        ref, rec, what = inputs.checked(c), c["rec"], inputs.what(c)
        cand = gpu.debug_elites_inject(c["cand"], c["ybar"], c["sigma"], c["lazy"], c["g"], rec.n_elites, int(rec.nominal), c["E_in"])
        same_bits(cand, ref["cand"], f"{what}: the candidates behind the injection")
        got = gpu.debug_elites_select(c["rews"], cand, c["ybar"], c["sigma"], c["lazy"], rec.n_elites, int(rec.nominal),
                                      count_in=len(c["E_in"]))
        inputs.assert_step(got, ref, what, same_bits, with_cand=False)


# ---- whole plans -----------------------------------------------------------------------------------------------------------------
def _configure(plan, case):
    N, H, Nu = inputs.SIZES[case.name]
    if case.shape:
        plan.set_noise_shape(inputs.ac_cases.plan_shape(H, Nu), "always")
    if getattr(case, "knots", 0):
        from noise_basis_checker import basis_of
        plan.set_noise_basis(basis_of(H, case.knots), "always")
    if getattr(case, "ess", False):
        plan.set_weighting(**case.wrec.kwargs())
    if getattr(case, "adapt", False):
        plan.set_adapt(**inputs.ac_cases.RULE.kwargs())
    if getattr(case, "D", 0):
        plan.set_mpc_delay(case.D)
    if getattr(case, "pick", 0):
        plan.set_mpc_pick(True, True, True)
    if isinstance(case, inputs.EpisodeCase) and case.method:
        plan.set_mpc_sigma(*inputs.SIGMA_REC)


@pytest.mark.parametrize("case", inputs.PLAN_CASES, ids=[c.id for c in inputs.PLAN_CASES])
def test_whole_plans(gpu, orc, case):
    """mbd_plan_run under the record: mu_0ts, the elites behind the run and the log of every step; the last step's candidates are
    the checker's, injected rows included.  (n_elites, nominal) = (32, 1) at 33 candidates is refused: 33 >= Nsample."""
    env, plan, s0 = _plan(gpu, case.name, case.method)
    N, H, Nu = inputs.SIZES[case.name]
    try:
        if case.state0 is not None:
            s0 = case.state0
            _start_from(plan, s0)
        _configure(plan, case)
        if case.record.n_elites + int(case.record.nominal) >= N:
            with pytest.raises(gpu.MbdError) as e:
                plan.set_elites(**case.record.kwargs())
            assert e.value.code == gpu.MBD_ERR_INVALID and f"Nsample={N}" in str(e.value)
            return
        plan.set_elites(**case.record.kwargs())
        key = gpu.prng_key(4)
        mu = plan.run(key)[0]
        ref = inputs.plan_reference(orc, _oenv(orc, env), s0, key, case, _impl())
        same_bits(mu, ref["mu_0ts"], f"{case.id}: mu_0ts")
        _same_elites(plan, ref, case.id)
        same_bits(plan.peek()[0], ref["details"][-1]["Y0s"], f"{case.id}: the last step's candidates")
        if case.adapt:
            same_bits(plan.peek_adapt()["a"], ref["table"], f"{case.id}: the adapt record's table")
        if case.record.n_elites and case.name == "car2d":  # (materialised: an elite is re-evaluated exactly and can stay)
            assert sum(k for _, k, _ in ref["elog"]) > 0, f"{case.id}: exact elites stay"
        mu2 = plan.run(key)[0]  # (a second run starts without elites again)
        same_bits(mu2, mu, f"{case.id}: a second run")
    finally:
        plan.close()


def test_a_frozen_elements_z_stays_zero(gpu, orc):
    """hopper under the shape with one frozen element: in the last step's normals, as mbd_plan_peek turns them into candidates, the
    frozen element of every row — injected or drawn — is Ybar_i's."""
    case = inputs.PlanCase("hopper", 0, "e3n", shape=True)
    env, plan, s0 = _plan(gpu, case.name, 0)
    N, H, Nu = inputs.SIZES[case.name]
    try:
        _configure(plan, case)
        plan.set_elites(**case.record.kwargs())
        key = gpu.prng_key(4)
        mu = plan.run(key)[0]
        Y = plan.peek()[0].reshape(N, H, Nu)
        ybar_last = mu[-2]  # (Ybar_1: what the last step sampled around)
        same_bits(Y[:, 1, Nu - 1], np.broadcast_to(ec.clip(ybar_last[1, Nu - 1]), (N,)).copy(), "the frozen element of every row")
        assert plan.peek_elites()["log_count"].tolist() == [3] * (ND - 1)
    finally:
        plan.close()


# ---- beside the other records -------------------------------------------------------------------------------------------------------
def test_rejection_on_the_hopper_whose_candidates_diverge(gpu, orc):
    """tests/weighting_combined_inputs.py's hopper with the 1e30 gear under its shape and a weighting record with rejection: in every
    step some candidates diverge, none of them is ever selected, and means, elites and log are the checker's."""
    import weighting_combined_inputs as wci
    import weighting_inputs as wi
    from noise_shape_checker import ShapedOracle
    from test_gpu_weighting_combined import _plan as _wplan
    c = wci.LOOP
    N, Nd, H = c["N"], c["Nd"], wci.H
    plan, s0 = _wplan(gpu, orc, 1, N, Nd, 0, c["state_seed"])
    try:
        g = wci.shape(plan.Nu)
        plan.set_noise_shape(g)
        plan.set_weighting(**wi.REJECT.kwargs())
        plan.set_elites(3, True, False)
        key = gpu.prng_key(c["key_seed"])
        mu = plan.run(key)[0]
        oe = wci.oenv(orc, wci.models()[1])
        st = ec.State(ec.Record(3, True, False), H, oe.Nu, True, g)
        ref = ec.run(ShapedOracle(orc, g), oe, s0, key, N, H, Nd, wci.TEMP, st, rec=wi.REJECT, impl=_impl())
        dropped = [int((~np.isfinite(s["rews"])).sum()) for s in st.steps]
        assert all(0 < d < N for d in dropped), dropped
        assert all(np.isfinite(s["rews"][s["src"]]).all() and len(s["src"]) == 3 for s in st.steps)
        same_bits(mu, ref["mu_0ts"], "rejection: mu_0ts")
        _same_elites(plan, dict(src=st.src, R=st.R, E=st.E, elog=st.log), "rejection")
    finally:
        plan.close()


def _other_record(gpu, orc, kind, env, plan, oenv):
    """Sets the record of ``kind`` on the plan; the checker's env for it."""
    import objective_checker as oc
    if kind == "ensemble":
        import ensemble_checker
        from mbd_hip.envs.base import RigidBodyEnv
        member = RigidBodyEnv(env.env_name, model=env.sys.scaled(mass=1.3, gear=0.8))
        plan.set_ensemble([None, member], "mean")
        return ensemble_checker.EnsembleEnv(oenv, [oenv, _oenv(orc, member)], "mean")
    if kind == "objective":
        prev0 = np.linspace(-0.5, 0.5, env.action_size).astype(f32)
        plan.set_objective(effort=0.05, rate=0.5, prev0=prev0)
        return oc.ObjectiveEnv(oenv, oc.Record(effort=0.05, rate=0.5, prev0=prev0))
    import value_checker as vc
    import value_inputs as vi
    net = vi.net(env.env_name, "S-65-64-1", "tanh", rel_xy=True, scale=0.37)
    plan.set_value(net.value_net())
    return vc.ValueEnv(oenv, net)


@pytest.mark.parametrize("kind", ["ensemble", "objective", "value"])
def test_beside_another_record(gpu, orc, kind):
    """hopper, MBD, (3, 1): the selection reads the rewards the score read — combined over two members, shaped by a rate cost, with
    a terminal value added — and the injected rows are rolled out and shaped like any other."""
    env, plan, s0 = _plan(gpu, "hopper", 0)
    N, H, Nu = inputs.SIZES["hopper"]
    try:
        oenv = _oenv(orc, env)
        cenv = _other_record(gpu, orc, kind, env, plan, oenv)
        plan.set_elites(3, True, False)
        key = gpu.prng_key(4)
        mu = plan.run(key)[0]
        st = ec.State(ec.Record(3, True, False), H, Nu, True)
        ref = ec.run(orc, cenv, s0, key, N, H, ND, TEMP, st, impl=_impl())
        same_bits(mu, ref["mu_0ts"], f"{kind}: mu_0ts")
        _same_elites(plan, dict(src=st.src, R=st.R, E=st.E, elog=st.log), kind)
        bare = ec.State(ec.Record(3, True, False), H, Nu, True)
        ec.run(orc, oenv, s0, key, N, H, ND, TEMP, bare, impl=_impl())
        assert [t for _, _, t in bare.log] != [t for _, _, t in st.log], f"{kind}: the record changes the rewards the selection reads"
    finally:
        plan.close()


# ---- episodes and sessions ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", inputs.EPISODE_CASES, ids=[c.id for c in inputs.EPISODE_CASES])
def test_episodes_and_sessions(gpu, orc, case):
    """mbd_plan_run_mpc under the record against the checker's episode: the logs, the elites behind the last tick and the log of
    every step; then a session fed the episode's states: its means, the elites behind every tick, the same log."""
    env, plan, s0 = _plan(gpu, case.name, case.method)
    try:
        _configure(plan, case)
        plant = None
        if case.plant:
            from mbd_hip.envs.base import RigidBodyEnv
            penv = RigidBodyEnv(case.name, model=env.sys.scaled(mass=case.plant))
            plan.set_mpc_plant(env=penv, key=gpu.prng_key(11), act_std=0.0, kick_std=0.0)
            plant = _oenv(orc, penv)
        plan.set_elites(**case.record.kwargs())
        key = gpu.prng_key(4)
        ep = plan.run_mpc(key, T, K, E)
        ref = inputs.episode_reference(orc, _oenv(orc, env), s0, key, case, _impl(), plant=plant)
        for k in ("means", "actions", "states", "rewards"):
            same_bits(ep[k], np.asarray(ref[k], f32).reshape(np.shape(ep[k])), f"{case.id}: {k}")
        _same_elites(plan, ref, case.id)
        counts = [c for c, _, _ in ref["elog"]]
        assert counts == [case.record.n_elites] * ((ND - 1) + (T - 1) * K)
        if case.carry and case.name != "car2d":  # (the first step of a warm tick injected the shifted elites: slots = 1 + 3)
            assert ref["steps"][ND - 1]["slots"] == 4
        if not case.carry:
            assert ref["steps"][ND - 1]["slots"] == 1
        if case.pick:
            assert [p for p in ref["picks"]], case.id
        if case.plant:
            plan.clear_mpc_plant()  # (in a session the caller is the plant)
        with plan.mpc_open(key, K, E) as s:
            for t in range(T):
                out = s.tick(ep["states"][t])
                same_bits(out["mean"], ep["means"][t], f"{case.id}: the session's mean of tick {t}")
                same_bits(plan.peek_elites()["E"], ref["elites"][t], f"{case.id}: the session's elites behind tick {t}")
            _same_elites(plan, ref, f"{case.id}: the session")
    finally:
        plan.close()


@pytest.mark.parametrize("method", [0, 1], ids=["mbd", "mppi"])
def test_reset_mean_empties_the_elites(gpu, orc, method):
    """A session with reset_mean in front of its third tick against the checker's: no elites right after the call, and the cold
    tick that follows, and its elites, are the checker's."""
    case = inputs.EpisodeCase(method=method, carry=True)
    env, plan, s0 = _plan(gpu, case.name, method)
    N, H, Nu = inputs.SIZES[case.name]
    try:
        _configure(plan, case)
        plan.set_elites(**case.record.kwargs())
        key = gpu.prng_key(4)
        ref = ec.Session(_oenv(orc, env), key, N, H, ND, TEMP, K, E, inputs.state_of(case, carry=True),
                         method=1 if method else None, sigma=inputs.SIGMA_REC, impl=_impl())
        with plan.mpc_open(key, K, E) as s:
            for t, x in enumerate([s0, s0, s0]):
                if t == 2:
                    assert plan.peek_elites()["count"] == 3
                    s.reset_mean()
                    ref.reset_mean()
                    assert plan.peek_elites()["count"] == 0, "reset_mean: no elites"
                out, want = s.tick(x), ref.tick(x)
                same_bits(out["mean"], want["mean"], f"tick {t}: mean")
                same_bits(plan.peek_elites()["E"], want["elites"], f"tick {t}: elites")
        assert ref.state.steps[ND - 1 + K]["slots"] == 1, "the cold tick's first step injected the nominal alone"
    finally:
        plan.close()


# ---- the phase calls -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hopper", "car2d"])
def test_phase_calls_against_run(gpu, orc, name):
    """mbd_plan_reverse_once at i = 5 .. 1 with a record — lazy (hopper) and materialised (car2d) — uses the state as it stands: from
    the empty state the set call leaves, the means and the elites behind every call are mbd_plan_run's and the checker's; the log
    appends."""
    import torch
    case = inputs.PlanCase(name, 0, "e3n")
    env, plan, s0 = _plan(gpu, name)
    N, H, Nu = inputs.SIZES[name]
    try:
        if case.state0 is not None:
            s0 = case.state0
            _start_from(plan, s0)
        plan.set_elites(**case.record.kwargs())
        k4 = gpu.prng_key(4)
        mu = plan.run(k4)[0]
        ref = inputs.plan_reference(orc, _oenv(orc, env), s0, k4, case, _impl())
        plan.set_elites(**case.record.kwargs())  # (the set call empties the elites and the log)
        assert plan.peek_elites()["count"] == 0 and plan.peek_elites()["steps"] == 0
        key = gpu.key_array(k4)
        d_ybar = torch.zeros(H * Nu, device="cuda")
        for n, i in enumerate(range(ND - 1, 0, -1)):
            got = _reverse_once(gpu, plan, i, key, d_ybar)
            same_bits(got, mu[n], f"{name}: the mean behind step {i}")
            same_bits(got, ref["mu_0ts"][n], f"{name}: the mean behind step {i} (checker)")
            pk = plan.peek_elites()
            same_bits(pk["E"], ref["steps"][n]["E"], f"{name}: the elites behind step {i}")
            assert pk["steps"] == n + 1 and int(pk["log_kept"][n]) == ref["elog"][n][1]
    finally:
        plan.close()


# ---- identity --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,method", [("hopper", 0), ("humanoidrun", 0), ("car2d", 0), ("hopper", 1)])
def test_a_cleared_record_gives_back_the_bits(gpu, name, method):
    """A record set, run and cleared: run and episode have the bits of the plan without one again — the ring's rewritten buffers are
    forgotten —, a record changes them, and peek without a record is refused."""
    env, plan, _ = _plan(gpu, name, method)
    try:
        if method:
            plan.set_mpc_sigma(*inputs.SIGMA_REC)
        key = gpu.prng_key(4)
        mu0, rm0 = plan.run(key)[:2]
        ep0 = plan.run_mpc(key, T, K, E)
        plan.set_elites(3, True, True)
        assert plan.has_elites
        mu1 = plan.run(key)[0]
        assert not np.array_equal(mu1, mu0), "a record changes the plan"
        ep1 = plan.run_mpc(key, T, K, E)
        assert not np.array_equal(ep1["means"], ep0["means"])
        plan.clear_elites()
        assert not plan.has_elites
        mu2, rm2 = plan.run(key)[:2]
        same_bits(mu2, mu0, "set and cleared: mu_0ts")
        same_bits(rm2, rm0, "set and cleared: mean rewards")
        ep2 = plan.run_mpc(key, T, K, E)
        for k in ("means", "actions", "states", "rewards"):
            same_bits(ep2[k], ep0[k], f"set and cleared: the episode's {k}")
        with pytest.raises(gpu.MbdError) as e:
            plan.peek_elites()
        assert e.value.code == gpu.MBD_ERR_STATE
    finally:
        plan.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_that_need_a_handle(gpu):
    """A sharded plan and an open session: MBD_ERR_STATE; cem, cma-es and a demo plan: MBD_ERR_UNSUPPORTED; a refused set call leaves
    the record alone; with a record the prefetch call is accepted and does nothing."""
    import ctypes as C
    from mbd_hip.planners.mbd_planner import Args, Plan
    N, H, _ = inputs.SIZES["hopper"]
    env, plan, _ = _plan(gpu, "hopper")
    try:
        with plan.mpc_open(gpu.prng_key(4), K, E):
            for call in (lambda: plan.set_elites(3, True, True), plan.clear_elites):
                with pytest.raises(gpu.MbdError) as e:
                    call()
                assert e.value.code == gpu.MBD_ERR_STATE and "session" in str(e.value)
        plan.set_elites(3, True, True)
        mu = plan.run(gpu.prng_key(4))[0]
        gpu.check(plan.lib.mbd_plan_prefetch_noise(plan.h, gpu.key_array(gpu.prng_key(9)), None))
        same_bits(plan.run(gpu.prng_key(4))[0], mu, "a declared key changes nothing")
        rec = gpu.elites_record(3, True, True)
        rec.reserved[2] = 1
        assert plan.lib.mbd_plan_set_elites(plan.h, C.byref(rec)) == gpu.MBD_ERR_INVALID and b"reserved[2]" in plan.lib.mbd_last_error()
        rec = gpu.elites_record(N - 1, True, True)
        assert plan.lib.mbd_plan_set_elites(plan.h, C.byref(rec)) == gpu.MBD_ERR_INVALID
        assert plan.peek_elites()["steps"] == ND - 1  # (a refused set call leaves the record alone)
    finally:
        plan.close()
    env, shard, _ = _plan(gpu, "hopper", shard_begin=0, shard_count=N // 2)
    try:
        with pytest.raises(gpu.MbdError) as e:
            shard.set_elites(3, True, True)
        assert e.value.code == gpu.MBD_ERR_STATE and "shard_count" in str(e.value)
    finally:
        shard.close()
    for method in (2, 3):
        env, pi, _ = _plan(gpu, "hopper", method=method)
        try:
            with pytest.raises(gpu.MbdError) as e:
                pi.set_elites(3, True, True)
            assert e.value.code == gpu.MBD_ERR_UNSUPPORTED and f"update_method={method}" in str(e.value)
        finally:
            pi.close()
    track = _env("humanoidtrack")
    demo = Plan(track, Args(env_name="humanoidtrack", Nsample=64, Hsample=50, Ndiffuse=3, enable_demo=True, disable_recommended_params=True,
                            not_render=True))
    try:
        with pytest.raises(gpu.MbdError) as e:
            demo.set_elites(3, True, True)
        assert e.value.code == gpu.MBD_ERR_UNSUPPORTED and "enable_demo" in str(e.value)
    finally:
        demo.close()


def test_the_python_layer_maps_every_flag(gpu):
    """mpc.run_mpc and run_mpc_online under the elite flags against the Plan path with the record written out by hand: the same
    means, elites and log, so every flag reaches its field."""
    from dataclasses import replace

    from mbd_hip.planners import mpc
    N, H, _ = inputs.SIZES["hopper"]
    base = mpc.MpcArgs(env_name="hopper", Nsample=N, Hsample=H, Ndiffuse=ND, temp_sample=TEMP, disable_recommended_params=True,
                       not_render=True, seed=2, n_ticks=T, warm_steps=K, exec_steps=E)
    args = replace(base, elites=3, elite_nominal=True, elite_carry=True)
    env, plan, state_init, key = mpc._setup(replace(base), 0)
    try:
        plan.set_elites(3, True, True)
        ref = plan.run_mpc(key, T, K, E)
        ref_log = plan.peek_elites()
        plan.set_elites(3, True, False)
        other = plan.run_mpc(key, T, K, E)
        assert not np.array_equal(other["means"], ref["means"]), "carry is told apart"
    finally:
        plan.close()
    _, det = mpc.run_mpc(replace(args), return_details=True)
    same_bits(det["means"], ref["means"], "mpc.run_mpc: means")
    same_bits(det["elite_log"]["E"], ref_log["E"], "mpc.run_mpc: the elites")
    same_bits(det["elite_log"]["log_top"], ref_log["log_top"], "mpc.run_mpc: the log")
    assert det["elites"] == 3 and det["elite_carry"] is True and det["elite_nominal"] is True
    _, on = mpc.run_mpc_online(replace(args), return_details=True)
    same_bits(on["means"], ref["means"], "mpc.run_mpc_online: means")
    same_bits(on["elite_log"]["log_top"], ref_log["log_top"], "mpc.run_mpc_online: the log")
    _, plain = mpc.run_mpc(replace(base), return_details=True)
    assert "elite_log" not in plain and "elites" not in plain and "elite_carry" not in plain
