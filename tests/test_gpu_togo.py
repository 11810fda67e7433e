"""-m gpu: the to-go record on the device (include/mbd_hip.h mbd_togo, DESIGN.md section 1 "N19 to-go") against the checker
(tests/togo_checker.py: numpy for layout and returns, the oracle's update once per group) by bit pattern, with a NaN where and only
where the checker has one.

  the update alone    mbd_debug_togo_step (togo_returns_kernel, togo_update_kernel) over N in {2, 63, 65, 1000, 1025, 2049} x (H, Nu)
                      in {(1, 1), (2, 3), (7, 17), (50, 17), (5, 24)} x (block, min_tail) in {(1, 1), (3, 1), (1, 4), (H, 1), (2, H)} x
                      the reward shapes; lazy and materialised candidates, MBD literal and identity, mppi
  G = 1               mbd_plan_run and run_mpc with block = H and with min_tail = H against the same handle after clear_togo
  whole plans         hopper, cartpole, humanoidrun, car2d at N = 64 and 130, H = 8, Ndiffuse = 6, blocks 1 and 3, MBD and mppi
  episodes, sessions  run_mpc with T = 4, K = 2, E = 1; a session fed the episode's states; reset_mean and the cold tick behind it
  other records       a noise shape with a frozen element, a noise basis, an mppi episode under a sigma record, a plant record with
                      act_std, a delay record, an elite record
  set, clear, set     between steps of one plan through the phase calls
  refusals            another record on the handle either way round, a shard, an open session, cem, cma-es, a demo plan"""
import functools

import numpy as np
import pytest

import togo_checker as tc
import togo_inputs as inputs
from state_inputs import same_bits

pytestmark = pytest.mark.gpu
f32 = np.float32
ND, H, TEMP, T, K, E = inputs.ND, inputs.H, inputs.TEMP, inputs.T, inputs.K, inputs.E


@pytest.fixture(scope="module")
def gpu(lib):
    from mbd_hip import _capi
    if _capi.device_count() < 1:
        pytest.fail("tests/test_gpu_togo.py needs a GPU")
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


def _plan(gpu, name, N, method=0, Hs=H, Nd=ND, state0=None, **plan_kw):
    """(env, plan, state0) from reset(prng_key(3)) or ``state0``, no record set."""
    import types

    from mbd_hip.planners.mbd_planner import Plan
    env = _env(name)
    if method:
        from mbd_hip.planners.path_integral import Args
        args = Args(env_name=name, Nsample=N, Hsample=Hs, Nrefine=Nd, temp_sample=TEMP, disable_recommended_params=True)
    else:
        from mbd_hip.planners.mpc import MpcArgs
        args = MpcArgs(env_name=name, Nsample=N, Hsample=Hs, Ndiffuse=Nd, temp_sample=TEMP, disable_recommended_params=True,
                       not_render=True)
    plan = Plan(env, args, update_method=method, **plan_kw)
    st = env.reset(gpu.prng_key(3))
    if state0 is not None:
        st = types.SimpleNamespace(pipeline_state=np.ascontiguousarray(state0, f32))
    plan.set_state0(st)
    return env, plan, np.asarray(st.pipeline_state, f32).reshape(-1)


def _same(got, ref, what):
    inputs.same(got, ref, what, same_bits)


def _same_peek(plan, step, what):
    """peek_togo's R and W against the checker's last step, and peek's weights against group 0's."""
    pk = plan.peek_togo()
    assert pk["R"].shape == step["R"].shape, f"{what}: {pk['R'].shape[0]} groups, the checker {step['R'].shape[0]}"
    _same(pk["R"], step["R"], f"{what}: R")
    _same(pk["W"], step["W"], f"{what}: W")
    _same(plan.peek()[2], step["W"][0], f"{what}: peek's weights are group 0's")


# ---- the update alone ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", inputs.SHAPES, ids=[f"H{h}-Nu{u}" for h, u in inputs.SHAPES])
@pytest.mark.parametrize("N", inputs.NS)
def test_the_update_alone(gpu, orc, N, shape):
    """The step's two launches on uploaded arrays against the checker's step: every layout and reward shape at this size.  Rows the
    checker has finite are finite and bit-equal; a non-finite late step leaves the later groups' rows finite."""
    Hs, Nu = shape
    for c in inputs.step_cases(N, Hs, Nu):
        ref, what = inputs.checked_step(orc, c), inputs.what(c)
        starts = tc.groups(Hs, c["block"], c["min_tail"])
        got = gpu.debug_togo_step(c["cand"], c["ybar"], c["rews"], c["rewss"], Nu, c["block"], c["min_tail"], c["lazy"], inputs.SIGMA,
                                  TEMP, c["method"] == 0, *inputs.ALPHAS, c["literal"], len(starts))
        _same(got["R"], ref["R"], f"{what}: R")
        _same(got["W"], ref["W"], f"{what}: W")
        _same(got["ybar"], ref["out"], f"{what}: Ybar_im1")
        _same(got["rew_mean"], ref["rew_mean"], f"{what}: the mean reward")
        if c["kind"] in ("nan_step_t", "inf_step0"):
            for j, s in enumerate(starts):
                if s > c["t"]:
                    end = starts[j + 1] if j + 1 < len(starts) else Hs
                    assert np.isfinite(got["ybar"][s:end]).all() and np.isfinite(got["W"][j]).all(), f"{what}: group {j} stays finite"
        if c["kind"] == "random" and len(starts) > 1 and N >= 63:  # (two candidates standardise to +-1 whatever their returns)
            assert not np.array_equal(got["W"][1], got["W"][0]), f"{what}: the groups' weights differ"


# ---- G = 1 is no record ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hopper", "humanoidrun"])
def test_one_group_is_no_record(gpu, name):
    """block = H and min_tail = H: mu_0ts, rew_means, peek and a three-tick episode are bit-equal to the same handle after
    clear_togo."""
    env, plan, _ = _plan(gpu, name, 64)
    key = gpu.prng_key(4)
    try:
        got = []
        for kw in (dict(block=H, min_tail=1), dict(block=1, min_tail=H), None):
            if kw is None:
                plan.clear_togo()
            else:
                plan.set_togo(**kw)
                assert plan.peek_togo()["starts"].tolist() == [0]
            mu, rm = plan.run(key)[:2]
            Y, rewss, w = plan.peek()
            ep = plan.run_mpc(key, 3, K, E)
            got.append(dict(mu=mu, rm=rm, Y=Y, rewss=rewss, w=w, means=ep["means"], states=ep["states"], actions=ep["actions"],
                            rewards=ep["rewards"]))
        for g, what in zip(got[:2], ("block = H", "min_tail = H")):
            for k, v in got[2].items():
                same_bits(g[k], v, f"{name}, {what}: {k}")
    finally:
        plan.close()


# ---- whole plans ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", inputs.PLAN_CASES, ids=[c.id for c in inputs.PLAN_CASES])
def test_whole_plans(gpu, orc, case):
    """mbd_plan_run under the record: mu_0ts, rew_means, the last step's R and W, and peek's weights, which are group 0's."""
    env, plan, s0 = _plan(gpu, case.name, case.N, case.method, state0=case.state0)
    try:
        plan.set_togo(case.block, 1)
        key = gpu.prng_key(4)
        mu, rm = plan.run(key)[:2]
        ref = inputs.plan_reference(_oenv(orc, env), s0, key, case, _impl())
        _same(mu, ref["mu_0ts"], f"{case.id}: mu_0ts")
        _same(rm, ref["rew_means"], f"{case.id}: rew_means")
        assert plan.peek_togo()["starts"].tolist() == tc.groups(H, case.block, 1).tolist()
        _same_peek(plan, ref["steps"][-1], case.id)
        if case.name != "car2d" or case.method == 1:  # (car2d's rewards from its reset state are all equal: every group's weights are)
            assert np.isfinite(ref["mu_0ts"]).all(), case.id
            W = ref["steps"][-1]["W"]
            assert not np.array_equal(W[1], W[0]), f"{case.id}: the groups' weights differ"
    finally:
        plan.close()


# ---- episodes and sessions ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", inputs.EPISODE_CASES, ids=[c.id for c in inputs.EPISODE_CASES])
def test_episodes_and_sessions(gpu, orc, case):
    """run_mpc against the checker's episode; a session fed that episode's states returns its means; reset_mean then gives a cold
    tick equal to tick 0 of a fresh episode from that state and key."""
    env, plan, s0 = _plan(gpu, case.name, case.N, case.method)
    try:
        if case.method:
            plan.set_mpc_sigma(*inputs.SIGMA_REC)
        plan.set_togo(case.block, 1)
        key = gpu.prng_key(4)
        ep = plan.run_mpc(key, T, K, E)
        ref = inputs.episode_reference(_oenv(orc, env), s0, key, case, _impl())
        for k in ("means", "actions", "states", "rewards"):
            _same(ep[k], np.asarray(ref[k], f32).reshape(np.shape(ep[k])), f"{case.id}: {k}")
        assert len(ref["steps"]) == (ND - 1) + (T - 1) * K
        _same_peek(plan, ref["steps"][-1], f"{case.id}: behind the episode")
        with plan.mpc_open(key, K, E) as s:
            for t in range(T):
                same_bits(s.tick(ep["states"][t])["mean"], ep["means"][t], f"{case.id}: the session's mean of tick {t}")
            s.reset_mean()
            x = ep["states"][2]
            cold = s.tick(x)["mean"]
        # tick 0 of a fresh episode from x under the key the session's fifth tick drew: the checker's session says which
        sess = tc.session(_oenv(orc, env), key, case.N, H, ND, TEMP, K, E, case.block, 1, case.method, inputs.SIGMA_REC, _impl())
        for t in range(T):
            sess.tick(ep["states"][t])
        sess.reset_mean()
        _same(cold, sess.tick(x)["mean"], f"{case.id}: the cold tick behind reset_mean")
    finally:
        plan.close()


# ---- beside other records ------------------------------------------------------------------------------------------------------------
def _shape(Nu):
    g = (0.75 + 0.5 * np.linspace(0, 1, H * Nu)).astype(f32).reshape(H, Nu)
    g[1, Nu - 1] = 0.0  # a frozen element
    return g


def test_beside_a_noise_shape_and_a_noise_basis(gpu, orc):
    """hopper, block 3: under a shape with a frozen element, and under a 3-knot basis, the plan is the checker's with the sampler's
    wrapper around the record's env."""
    from noise_basis_checker import basis_env, basis_of
    from noise_shape_checker import shaped_env
    env, plan, s0 = _plan(gpu, "hopper", 64)
    key = gpu.prng_key(4)
    try:
        plan.set_togo(3, 1)
        g = _shape(plan.Nu)
        plan.set_noise_shape(g, "always")
        ref = tc.run(_oenv(orc, env), s0, key, 64, H, ND, TEMP, 3, 1, 0, _impl(), wrap=lambda e: shaped_env(e, g))
        mu = plan.run(key)[0]
        _same(mu, ref["mu_0ts"], "shape: mu_0ts")
        _same_peek(plan, ref["steps"][-1], "shape")
        # (the frozen element's candidates all equal Ybar_i: every group's weights sum to 1, so the mean stays put up to rounding)
        plan.clear_noise_shape()
        W = basis_of(H, 3)
        plan.set_noise_basis(W, "always")
        ref = tc.run(_oenv(orc, env), s0, key, 64, H, ND, TEMP, 3, 1, 0, _impl(), wrap=lambda e: basis_env(e, W))
        _same(plan.run(key)[0], ref["mu_0ts"], "basis: mu_0ts")
        _same_peek(plan, ref["steps"][-1], "basis")
    finally:
        plan.close()


def test_beside_a_plant_and_a_delay_record(gpu, orc):
    """hopper, block 3: an episode on a plant of mass 1.3 with action noise, and an episode planned one tick ahead, against the plant
    and delay checkers over the record's env."""
    import mpc_delay_checker
    import mpc_plant_checker
    from mbd_hip.envs.base import RigidBodyEnv
    env, plan, s0 = _plan(gpu, "hopper", 64)
    key = gpu.prng_key(4)
    try:
        plan.set_togo(3, 1)
        penv = RigidBodyEnv("hopper", model=env.sys.scaled(mass=1.3))
        dkey = gpu.prng_key(11)
        plan.set_mpc_plant(env=penv, key=dkey, act_std=0.1)
        ep = plan.run_mpc(key, T, K, E)
        ref = tc.episode(_oenv(orc, env), s0, key, 64, H, ND, TEMP, T, K, E, 3, 1, checker_episode=mpc_plant_checker.episode,
                         plant=_oenv(orc, penv), dkey=dkey, act_std=0.1, impl=_impl())
        for k in ("means", "actions", "states", "rewards"):
            _same(ep[k], np.asarray(ref[k], f32).reshape(np.shape(ep[k])), f"plant: {k}")
        plan.clear_mpc_plant()
        plan.set_mpc_delay(1)
        ep = plan.run_mpc(key, T, K, E)
        ref = tc.episode(_oenv(orc, env), s0, key, 64, H, ND, TEMP, T, K, E, 3, 1, checker_episode=mpc_delay_checker.episode, D=1,
                         impl=_impl())
        for k in ("means", "actions", "states", "rewards", "predicted"):
            _same(ep[k], np.asarray(ref[k], f32).reshape(np.shape(ep[k])), f"delay: {k}")
    finally:
        plan.close()


def test_beside_an_elite_record(gpu, orc):
    """hopper, block 3, three elites and the nominal: the selection is the elite checker's on rews — not on a group's returns — and
    the rows injected are its rows; means, elites and the record's R and W are the composed checker's."""
    import elites_checker as ec
    from oracle import planner as op
    env, plan, s0 = _plan(gpu, "hopper", 64)
    key = gpu.prng_key(4)
    try:
        plan.set_togo(3, 1)
        plan.set_elites(3, True, False)
        mu = plan.run(key)[0]
        st = ec.State(ec.Record(3, True, False), H, plan.Nu, True, None)
        st.reset()

        def step(o, e, *a, **kw):  # (the injection behind the sampler, the record's update, the selection over rews)
            out = op.reverse_once(ec.ElitesOracle(o, st), e, *a, **kw)
            st.select(out[3]["rews"], out[3]["Y0s"])
            return out

        ref = tc.run(_oenv(orc, env), s0, key, 64, H, ND, TEMP, 3, 1, 0, _impl(), step=step)
        _same(mu, ref["mu_0ts"], "elites: mu_0ts")
        _same_peek(plan, ref["steps"][-1], "elites")
        pk = plan.peek_elites()
        assert list(pk["src"]) == list(st.src), "the selection reads rews"
        same_bits(pk["R"], st.R, "the elites' returns are entries of rews")
        same_bits(pk["E"], st.E, "the elites")
        same_bits(plan.peek()[0], ref["details"][-1]["Y0s"], "the last step's candidates, injected rows included")
    finally:
        plan.close()


# ---- set, clear, set again --------------------------------------------------------------------------------------------------------------
def _reverse_once(gpu, plan, i, key, d_ybar):
    """mbd_plan_reverse_once on the device mean d_ybar (in place) with the key array ``key`` (advanced); the new mean [H, Nu]."""
    import torch
    rm = torch.zeros(1, device="cuda")
    gpu.check(plan.lib.mbd_plan_reverse_once(plan.h, i, key, d_ybar.data_ptr(), rm.data_ptr(), None))
    torch.cuda.synchronize()
    return d_ybar.cpu().numpy().reshape(plan.H, plan.Nu)


@pytest.mark.parametrize("name", ["hopper", "car2d"])
def test_set_clear_set_between_steps(gpu, orc, name):
    """One plan stepped through the phase calls, lazy (hopper) and materialised (car2d): two steps with the record, two after
    clear_togo, one with it again.  Every step is the checker's from the mean it found, and the cleared stretch has the bits of a
    plan that never had a record, stepped from the same mean and keys."""
    import torch
    from oracle import planner as op
    N, Nd = 64, 7
    s0 = np.array(inputs.CAR2D_S0, f32) if name == "car2d" else None
    env, plan, s0 = _plan(gpu, name, N, Nd=Nd, state0=s0)
    env, bare, _ = _plan(gpu, name, N, Nd=Nd, state0=s0)
    oenv = _oenv(orc, env)
    tenv = tc.togo_env(oenv, 3, 1)
    sched = orc.schedule(1e-4, 1e-2, Nd)
    try:
        key = gpu.key_array(gpu.prng_key(4))
        d_ybar = torch.zeros(H * plan.Nu, device="cuda")
        r, Ybar = np.asarray(gpu.prng_key(4), np.uint32), np.zeros((H, plan.Nu), f32)
        for i, rec in zip(range(Nd - 1, 0, -1), (True, True, False, False, True, False)):
            if rec:
                plan.set_togo(3, 1)
            elif plan.has_togo:
                plan.clear_togo()
            e = tenv if rec else oenv
            before = d_ybar.clone()
            key_before = type(key)(*key)
            got = _reverse_once(gpu, plan, i, key, d_ybar)
            r, Ybar, _, _ = op.reverse_once(e.orc, e, s0, i, r, Ybar, sched, N, H, TEMP, _impl())
            _same(got, Ybar, f"{name}: step {i} {'with' if rec else 'without'} the record")
            if not rec:
                same_bits(_reverse_once(gpu, bare, i, key_before, before), got, f"{name}: step {i}: a plan that never had a record")
    finally:
        plan.close()
        bare.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_that_need_a_handle(gpu):
    """A plan holding an objective, value, weighting, adapt or ensemble record refuses the record, and a plan holding the record
    refuses those five, each naming the other; a shard and an open session: MBD_ERR_STATE; cem, cma-es and a demo plan:
    MBD_ERR_UNSUPPORTED; a refused set call leaves the record alone."""
    import ctypes as C

    import value_inputs as vi
    from mbd_hip.envs.base import RigidBodyEnv
    from mbd_hip.planners.mbd_planner import Args, Plan
    env, plan, _ = _plan(gpu, "hopper", 64)
    member = RigidBodyEnv("hopper", model=env.sys.scaled(mass=1.3))
    others = (("objective", lambda: plan.set_objective(effort=0.05), plan.clear_objective),
              ("value", lambda: plan.set_value(vi.net("hopper", "S-65-64-1", "tanh", rel_xy=True, scale=0.37).value_net()), lambda: plan.set_value(None)),
              ("weighting", lambda: plan.set_weighting(reject_nonfinite=True), plan.clear_weighting),
              ("adapt", lambda: plan.set_adapt(0.5, 0.5, 2.0), plan.clear_adapt),
              ("ensemble", lambda: plan.set_ensemble([None, member], "mean"), plan.clear_ensemble))
    try:
        for word, set_, clear in others:
            set_()
            with pytest.raises(gpu.MbdError) as e:
                plan.set_togo(3, 1)
            assert e.value.code == gpu.MBD_ERR_UNSUPPORTED and word in str(e.value), (word, str(e.value))
            clear()
            plan.set_togo(3, 1)
            with pytest.raises(gpu.MbdError) as e:
                set_()
            assert e.value.code == gpu.MBD_ERR_UNSUPPORTED and "to-go" in str(e.value), (word, str(e.value))
            plan.clear_togo()
        with plan.mpc_open(gpu.prng_key(4), K, E):
            for call in (lambda: plan.set_togo(3, 1), plan.clear_togo):
                with pytest.raises(gpu.MbdError) as e:
                    call()
                assert e.value.code == gpu.MBD_ERR_STATE and "session" in str(e.value)
        plan.set_togo(3, 1)
        mu = plan.run(gpu.prng_key(4))[0]
        rec = gpu.togo_record(3, H + 1)
        assert plan.lib.mbd_plan_set_togo(plan.h, C.byref(rec)) == gpu.MBD_ERR_INVALID and b"min_tail" in plan.lib.mbd_last_error()
        same_bits(plan.run(gpu.prng_key(4))[0], mu, "a refused set call leaves the record alone")
        plan.clear_togo()
        with pytest.raises(gpu.MbdError) as e:
            plan.peek_togo()
        assert e.value.code == gpu.MBD_ERR_STATE
    finally:
        plan.close()
    env, shard, _ = _plan(gpu, "hopper", 64, shard_begin=0, shard_count=32)
    try:
        with pytest.raises(gpu.MbdError) as e:
            shard.set_togo(3, 1)
        assert e.value.code == gpu.MBD_ERR_STATE and "shard_count" in str(e.value)
    finally:
        shard.close()
    for method in (2, 3):
        env, pi, _ = _plan(gpu, "hopper", 64, method=method)
        try:
            with pytest.raises(gpu.MbdError) as e:
                pi.set_togo(3, 1)
            assert e.value.code == gpu.MBD_ERR_UNSUPPORTED and f"update_method={method}" in str(e.value)
        finally:
            pi.close()
    track = _env("humanoidtrack")
    demo = Plan(track, Args(env_name="humanoidtrack", Nsample=64, Hsample=50, Ndiffuse=3, enable_demo=True, disable_recommended_params=True,
                            not_render=True))
    try:
        with pytest.raises(gpu.MbdError) as e:
            demo.set_togo(3, 1)
        assert e.value.code == gpu.MBD_ERR_UNSUPPORTED and "enable_demo" in str(e.value)
    finally:
        demo.close()


def test_the_python_layer_maps_every_flag(gpu):
    """mpc.run_mpc and run_mpc_online under the to-go flags against the Plan path with the record written out by hand."""
    from dataclasses import replace

    from mbd_hip.planners import mpc
    base = mpc.MpcArgs(env_name="hopper", Nsample=64, Hsample=H, Ndiffuse=ND, temp_sample=TEMP, disable_recommended_params=True,
                       not_render=True, seed=2, n_ticks=T, warm_steps=K, exec_steps=E)
    args = replace(base, togo_block=3, togo_min_tail=3)
    env, plan, state_init, key = mpc._setup(replace(base), 0)
    try:
        plan.set_togo(3, 3)
        ref = plan.run_mpc(key, T, K, E)
        pk = plan.peek_togo()
        plan.set_togo(3, 1)
        assert not np.array_equal(plan.run_mpc(key, T, K, E)["means"], ref["means"]), "min_tail is told apart"
    finally:
        plan.close()
    assert pk["starts"].tolist() == [0, 3]  # (row 6 has two rows ahead of it: no start under min_tail = 3)
    _, det = mpc.run_mpc(replace(args), return_details=True)
    same_bits(det["means"], ref["means"], "mpc.run_mpc: means")
    same_bits(det["togo"]["W"], pk["W"], "mpc.run_mpc: the last step's weights")
    assert det["togo_block"] == 3 and det["togo_min_tail"] == 3 and det["togo"]["starts"].tolist() == [0, 3]
    _, on = mpc.run_mpc_online(replace(args), return_details=True)
    same_bits(on["means"], ref["means"], "mpc.run_mpc_online: means")
    _, plain = mpc.run_mpc(replace(base), return_details=True)
    assert "togo" not in plain and "togo_block" not in plain
