"""-m gpu: the weighting record (include/mbd_hip.h mbd_weighting, DESIGN.md section 1 "N14 weighting") TOGETHER with the other records
and behind rollouts that really diverge, against the composed checker by bit pattern.  tests/test_gpu_weighting.py hands weigh_kernel
rewards a test uploaded, on plans with no other record; here the rewards come out of the objective kernel, the ensemble's reduction
and rollouts on a model that overflows, and what the weights feed is looked at as far as it goes: cma-es' sigma, cem's selection, the
non-lazy weighted mean, sigma carried through path-integral episodes, sessions and sweeps, warm ticks under a noise shape and basis,
a delay and a plant.  The cases, the records and the checker's compositions are tests/weighting_combined_inputs.py's;
tests/test_weighting.py asserts on the CPU that they take the branches and drop the candidates they are there for.

Every comparison is by bit pattern (state_inputs.same_bits) or np.array_equal; the one exception is named in
test_real_divergence_closed_loop's docstring."""
import functools

import numpy as np
import pytest

import mpc_pi_checker as pic
import weighting_checker as wc
import weighting_combined_inputs as wci
import weighting_inputs as wi
from state_inputs import same_bits
from test_gpu_weighting import _Step, _args, _checked, _env, _impl, TABLE

pytestmark = pytest.mark.gpu

H, T, K, E = wci.H, wci.T, wci.K, wci.E
_LOGS = ("means", "actions", "rewards", "states")


@pytest.fixture(scope="module")
def gpu(lib):
    from mbd_hip import _capi
    if _capi.device_count() < 1:
        pytest.fail("tests/test_gpu_weighting_combined.py needs a GPU")
    return _capi


def _state(s):
    from mbd_hip.envs.base import State
    return State(np.asarray(s, np.float32), None, np.float32(0.0), np.float32(0.0), {})


@functools.lru_cache(maxsize=None)
def _hopper(which):
    """The device envs of wci.models(): 0 the hopper, 1 the one with the 1e30 gear, 2 the heavier one."""
    from mbd_hip.envs.base import RigidBodyEnv
    return RigidBodyEnv(wci.NAME, model=wci.models()[which])


def _equal(a, b, what, logs=_LOGS):
    for k in logs:
        x, y = np.asarray(a[k], np.float32), np.asarray(b[k], np.float32)
        assert x.size == y.size, f"{what}: {k} sizes"
        same_bits(x.reshape(y.shape), y, f"{what}: {k}")


def _same_log(log, ref, what):
    """A peeked log (the last run's or the last tick's steps) against the checker's entries [(temp, ess, kept)]."""
    assert len(log["temp"]) == len(log["ess"]) == len(log["kept"]) == len(ref), f"{what}: {len(log['temp'])} entries, the checker has {len(ref)}"
    for j, (Ts, ess, kept) in enumerate(ref):
        same_bits(log["temp"][j], Ts, f"{what}, step {j}: temperature")
        same_bits(log["ess"][j], ess, f"{what}, step {j}: ess")
        assert int(log["kept"][j]) == kept, f"{what}, step {j}: kept {int(log['kept'][j])}, the checker {kept}"


def _plan(gpu, orc, which, N, Nd, method=0, seed=3):
    """(plan, s0) on the device env ``which`` from the checker's reset state of ``seed``."""
    from mbd_hip.planners.mbd_planner import Plan
    env = _hopper(which)
    plan = Plan(env, _args(wci.NAME, N, Nd, method, temp=wci.TEMP), update_method=method)
    s0 = wci.start(orc, wci.models()[which], seed, _impl())
    plan.set_state0(_state(s0))
    return plan, s0


def test_the_inputs_are_the_librarys(gpu, orc):
    """What tests/weighting_combined_inputs.py builds without the library is what the library builds: keys, the reset state, the
    discount weights."""
    from mbd_hip.planners.mpc import discount_weights
    for seed in (3, 5, 75):
        assert np.array_equal(np.asarray(gpu.prng_key(seed), np.uint32), np.asarray(orc.prng_key(seed), np.uint32))
    same_bits(wci.objective(3).row_weight, discount_weights(H, 0.9, terminal=2.0), "discount weights")
    env = _hopper(0)
    same_bits(np.asarray(env.reset(gpu.prng_key(3)).pipeline_state, np.float32).reshape(-1), wci.start(orc, wci.models()[0], 3, _impl()), "reset state")


# ---- 1. cma-es' sigma under a record ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 64, 65, 1025])
def test_cma_sigma_under_a_record(gpu, orc, N):
    """set_sigma(0.7), one mbd_plan_score_update under every case's record, then mbd_plan_get_sigma: cma_spread_kernel and
    cma_sigma_kernel on the weigh kernel's weights — +0 for dropped candidates — against ``wc.pi_update``'s sigma, bit for bit.
    ``all_dropped``: every weight +0, the spread +0, sigma at the 1e-3 floor; ``one_kept``: one weight of 1."""
    step = _Step(gpu, "hopper", N, 2)
    try:
        n = 0
        for k, c in enumerate(TABLE):
            if c.N != N:
                continue
            step.plan.set_weighting(**c.rec.kwargs())
            mu, w, _ = step.update(c.rews)
            sigma = np.float32(step.plan.get_sigma())
            ref = _checked(orc, k)
            mu_ref, sigma_ref = wc.pi_update(orc, 2, ref, step.Y0s, step.mu, 0.7)
            print(f"{c.id}: sigma {sigma!r}, the checker {sigma_ref!r}")
            same_bits(w, ref["weights"], f"{c.id}: weights")
            assert np.array_equal(mu, mu_ref, equal_nan=True), f"{c.id}: the new mean"
            same_bits(sigma, sigma_ref, f"{c.id}: sigma")
            assert np.isfinite(sigma) and sigma >= np.float32(1e-3), c.id
            if c.name == "all_dropped":
                assert sigma == np.float32(1e-3), c.id
            n += 1
        assert n == len(wi.cases(N))
    finally:
        step.plan.close()


# ---- 2. the non-lazy MBD step ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [64, 1025, 12289])
@pytest.mark.parametrize("name", ["hopper", "car2d"])
def test_non_lazy_mbd_step_under_a_record(gpu, orc, levers, name, N):
    """Method 0 with MATERIALISED candidates — the hopper under MBD_NO_LAZY=1, car2d (no model env: never lazy) —: the weighted mean
    of given weights with lazy = 0 and the literal score form, which no other test runs under a record (every other method-0 plan
    there is lazy).  Weights, mean reward, log and the new mean against ``wc.update(..., literal=True)``."""
    if name == "hopper":
        levers(MBD_NO_LAZY=1)  # (acts on plans created from now on)
    step = _Step(gpu, name, N, 0)
    try:
        n = 0
        for k, c in enumerate(TABLE):
            if c.N != N or c.name not in ("planted", "planted_ess", "bracket"):
                continue
            what = f"{name} {c.id}"
            step.plan.set_weighting(**c.rec.kwargs())
            mu, w, rm = step.update(c.rews)
            ref = _checked(orc, k)
            _same_log(step.plan.peek_weighting(), [(ref["temp"], ref["ess"], ref["kept"])], what)
            same_bits(w, ref["weights"], f"{what}: weights")
            same_bits(rm, ref["rew_mean"], f"{what}: mean reward")
            mu_ref = wc.update(orc, 0, ref["weights"], step.Y0s, step.mu, step.sched, step.i, literal=True)
            assert np.isfinite(mu_ref).all()
            same_bits(mu, mu_ref, f"{what}: the new mean")
            n += 1
        assert n == 3
    finally:
        step.plan.close()


# ---- 3. real divergence, one step --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1, 2, 3])
def test_real_divergence_one_step(gpu, orc, method):
    """mbd_plan_sample_rollout on the hopper whose actuator 0 has a gear of 1e30, under the noise shape of 3e-5 on that column
    (tests/weighting_combined_inputs.py: without it every candidate diverges, with zeros there none does).  The candidates and the
    rewards the rollout left are the checker's launch; 0 < kept < N on the device's own buffer.  Then mbd_plan_score_update on that
    buffer under wi.REJECT and wi.ESS: weights, mean reward, log, the new mean (and cma-es' sigma) equal the checker fed the PEEKED
    rewards and candidates, kept is the count of finite peeked rewards and the mean is finite; without a record it is not (cem's
    excepted: its mean of ten candidates is finite whatever the weights)."""
    import torch
    c = wci.STEP
    N, i = c["N"], c["i"]
    ref = wci.divergence_step(orc, method, _impl())
    plan, s0 = _plan(gpu, orc, 1, N, c["Nd"], method, c["state_seed"])
    try:
        same_bits(s0, ref["s0"], "the start state")
        Nu = plan.Nu
        plan.set_noise_shape(wci.shape(Nu))
        if method:
            plan.set_sigma(c["pi_sigma"])
        ks = gpu.key_array(gpu.prng_key(c["key_seed"]))
        d_mu = torch.tensor(ref["mu"].reshape(-1), device="cuda")
        d_r = torch.full((N,), 7.0, device="cuda")
        gpu.check(plan.lib.mbd_plan_sample_rollout(plan.h, i, ks, d_mu.data_ptr(), d_r.data_ptr(), None, None))
        torch.cuda.synchronize()
        Y0s = plan.peek()[0]
        rews = d_r.cpu().numpy()
        kept = int(np.isfinite(rews).sum())
        print(f"method {method}: kept {kept} of {N} (the checker's launch: {int(np.isfinite(ref['rews']).sum())})")
        assert 0 < kept < N
        same_bits(Y0s, ref["Y0s"], "the candidates")
        assert np.array_equal(np.isfinite(rews), np.isfinite(ref["rews"])), "which candidates diverge"
        same_bits(rews[np.isfinite(rews)], ref["rews"][np.isfinite(rews)], "the finite rewards")
        sched = plan.schedule()

        def update():
            if method:
                plan.set_sigma(0.7)
            out, rm = torch.full((H * Nu,), 7.0, device="cuda"), torch.zeros(1, device="cuda")
            gpu.check(plan.lib.mbd_plan_score_update(plan.h, i, ks, d_mu.data_ptr(), d_r.data_ptr(), None, out.data_ptr(), rm.data_ptr(), None))
            torch.cuda.synchronize()
            return out.cpu().numpy().reshape(H, Nu), plan.peek()[2], np.float32(rm.item())

        mu, w, _ = update()
        assert not np.isfinite(w).any(), "without a record a diverged candidate reaches every weight"
        if method != 3:
            assert not np.isfinite(mu).any(), "without a record a diverged candidate reaches the mean"
        for rec in (wi.REJECT, wi.ESS):
            what = f"method {method} ess_frac={rec.ess_frac}"
            plan.set_weighting(**rec.kwargs())
            mu, w, rm = update()
            res = wc.weigh(orc, rews, wci.TEMP, rec)
            assert res["kept"] == kept
            _same_log(plan.peek_weighting(), [(res["temp"], res["ess"], res["kept"])], what)
            same_bits(w, res["weights"], f"{what}: weights")
            same_bits(rm, res["rew_mean"], f"{what}: mean reward")
            assert (w[~np.isfinite(rews)].view(np.uint32) == 0).all()
            if method == 0:
                mu_ref = wc.update(orc, 0, res["weights"], Y0s, ref["mu"], sched, i)
            else:
                mu_ref, sigma_ref = wc.pi_update(orc, method, res, Y0s, ref["mu"], 0.7)
                same_bits(np.float32(plan.get_sigma()), sigma_ref, f"{what}: sigma")
            assert np.isfinite(mu).all(), f"{what}: the new mean is not finite"
            same_bits(mu, mu_ref, f"{what}: the new mean")
    finally:
        plan.close()


# ---- 4. real divergence, closed loop -----------------------------------------------------------------------------------------------
def test_real_divergence_closed_loop(gpu, orc):
    """A 3-tick mbd_plan_run_mpc planned AND executed on the hopper with the 1e30 gear, under the noise shape that is 3e-5 (not
    zero) on that column and wi.REJECT: every tick drops some candidates and keeps some (asserted of the checker's episode on the
    CPU as well), every mean and state is finite, and means, rows, rewards, states and the last tick's log are the checker's
    episode bit for bit.  The same episode without a record ends with non-finite means.

    THE COMPARISON RULE where the checker's values are not finite (the episode without a record only) is
    tests/test_gpu_containment.py's: values are compared by bit pattern where the checker's are finite, and by their isfinite
    pattern elsewhere — the primitives differ in the kind and payload of a non-finite by contract, never in whether one arrives."""
    c = wci.LOOP
    N, Nd = c["N"], c["Nd"]
    ref = wci.divergence_episode(orc, wi.REJECT, _impl())
    plan, s0 = _plan(gpu, orc, 1, N, Nd, 0, c["state_seed"])
    try:
        plan.set_noise_shape(wci.shape(plan.Nu))
        key = gpu.prng_key(c["key_seed"])
        plan.set_weighting(**wi.REJECT.kwargs())
        ep = plan.run_mpc(key, T, K, E)
        log = plan.peek_weighting()
        print("kept per tick (checker):", [[e[2] for e in tick] for tick in ref["log"]], "last tick (device):", log["kept"].tolist())
        assert np.isfinite(ref["means"]).all() and np.isfinite(ref["states"]).all()
        assert np.isfinite(ep["means"]).all() and np.isfinite(ep["states"]).all()
        _equal(ep, ref, "under the record")
        _same_log(log, ref["log"][-1], "the last tick")
        assert all(0 < kept < N for kept in log["kept"])
        plan.clear_weighting()
        bare = plan.run_mpc(key, T, K, E)
        assert not np.isfinite(bare["means"][-1]).any(), "without a record the episode's means end non-finite"
        from noise_shape_checker import shaped_env
        import mpc_checker
        oe = wci.oenv(orc, wci.models()[1])
        bare_ref = mpc_checker.episode(shaped_env(oe, wci.shape(oe.Nu)), s0, key, N, H, Nd, wci.TEMP, T, K, E, _impl())
        for k in ("means", "rewards"):
            x, y = np.asarray(bare[k], np.float32).reshape(-1), np.asarray(bare_ref[k], np.float32).reshape(-1)
            fin = np.isfinite(y)
            assert np.array_equal(np.isfinite(x), fin), f"without a record: which {k} are finite"
            same_bits(x[fin], y[fin], f"without a record: the finite {k}")
    finally:
        plan.close()


# ---- 5. an objective record in front ----------------------------------------------------------------------------------------------
def _objective_plan(gpu, orc, N, Nd, with_objective=True):
    plan, s0 = _plan(gpu, orc, 0, N, Nd)
    if with_objective:
        plan.set_objective(**wci.objective(plan.Nu).kwargs())
    return plan, s0


@pytest.mark.parametrize("rec", [wi.ESS, wci.FULL], ids=["ess", "target_kept"])
def test_objective_in_front_whole_run(gpu, orc, rec):
    """mbd_plan_run with a discount, a terminal weight, effort and rate costs, actuator weights and a prev0 under an ESS target:
    objective_kernel rewrites the rewards in place and the target acts on ret - cost.  Means, mean rewards and the log against
    ``wc.run`` on an ObjectiveEnv; under ``target_kept`` every step sits at temp_max."""
    N, Nd = 65, 5
    plan, s0 = _objective_plan(gpu, orc, N, Nd)
    try:
        plan.set_weighting(**rec.kwargs())
        mu, rm, _, _ = plan.run(gpu.prng_key(7))
        ref = wci.objective_run(orc, rec, True, N, Nd, _impl())
        same_bits(mu, ref["mu_0ts"], "means")
        same_bits(rm, ref["rew_means"], "mean rewards")
        _same_log(plan.peek_weighting(), ref["log"], "the run")
        bare = wci.objective_run(orc, rec, False, N, Nd, _impl())
        assert not np.array_equal(bare["mu_0ts"], ref["mu_0ts"])
    finally:
        plan.close()


def test_objective_in_front_episode_and_session(gpu, orc):
    """A 3-tick episode under the objective record and wi.ESS against ``objective_checker.episode`` over ``wc.reverse_once`` — the
    rate cost's previous action carried from tick to tick —, then a session fed that episode's states.  The logged temperatures
    differ from those of the same episode without the objective, in the checker and on the device: the composition was exercised."""
    N, Nd = 65, 5
    key = gpu.prng_key(5)
    plan, s0 = _objective_plan(gpu, orc, N, Nd)
    try:
        plan.set_weighting(**wi.ESS.kwargs())
        ep = plan.run_mpc(key, T, K, E)
        log = plan.peek_weighting()
        ref = wci.objective_episode(orc, wi.ESS, True, N, Nd, _impl())
        _equal(ep, ref, "episode")
        _same_log(log, ref["log"][-1], "the last tick")
        bare = wci.objective_episode(orc, wi.ESS, False, N, Nd, _impl())
        assert all(a[0] != b[0] for ta, tb in zip(ref["log"], bare["log"]) for a, b in zip(ta, tb))
        with plan.mpc_open(key, K, E) as s:
            means, logs = [], []
            for t in range(T):
                means.append(s.tick(ep["states"][t])["mean"])
                logs.append(plan.peek_weighting())
        same_bits(np.stack(means), ep["means"], "the session's means")
        for t in range(T):
            _same_log(logs[t], ref["log"][t], f"the session's tick {t}")
        plan.clear_objective()
        plan.run_mpc(key, T, K, E)
        _same_log(plan.peek_weighting(), bare["log"][-1], "without the objective, the last tick")
        assert not np.array_equal(plan.peek_weighting()["temp"], log["temp"])
    finally:
        plan.close()


def test_objective_in_front_delay_and_plant(gpu, orc):
    """D = 1 and a heavier plant with action noise (act_std = 0.05): the first previous action is the queue's last row, afterwards
    the commanded row whatever the plant adds; the tick plans from the predicted state; the log of a warm tick holds K entries."""
    N, Nd = 65, 5
    key, dkey = gpu.prng_key(5), gpu.prng_key(11)
    plan, s0 = _objective_plan(gpu, orc, N, Nd)
    try:
        plan.set_weighting(**wi.ESS.kwargs())
        plan.set_mpc_delay(1)
        plan.set_mpc_plant(env=_hopper(2), key=dkey, act_std=0.05)
        ep = plan.run_mpc(key, T, K, E)
        ref = wci.objective_episode(orc, wi.ESS, True, N, Nd, _impl(), D=1, plant=wci.models()[2], dkey=dkey, act_std=0.05)
        _equal(ep, ref, "delayed episode on a plant")
        _same_log(plan.peek_weighting(), ref["log"][-1], "the last tick")
        assert len(ref["log"][-1]) == K
        assert not np.array_equal(ref["actions"][:E], np.zeros_like(ref["actions"][:E]))  # (the plant's noise on the zero queue)
    finally:
        plan.close()


# ---- 6. an ensemble in front -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,bad,risk,with_objective", wci.ENSEMBLES,
                         ids=[f"N{c[0]}-bad{c[1]}-{c[2]}" + ("-objective" if c[3] else "") for c in wci.ENSEMBLES])
def test_ensemble_in_front(gpu, orc, N, bad, risk, with_objective):
    """M = 3 hopper members, member ``bad`` with the 1e30 gear, under the noise shape of 3e-5 on that column: the member diverges for
    some candidates, ensemble_reduce_kernel hands their non-finite combination to the weigh kernel (N = 33: one launch per member,
    N = 32: one launch), and the record drops exactly those.  One mbd_plan_reverse_once — weights, the new mean, the mean reward,
    the log; kept is the count of candidates whose combined reward is finite in the checker, and on the device — and a 3-tick episode,
    against the checker.  One parametrisation adds the objective record: with an ensemble that is another launch of the step."""
    import torch
    Nd = 5
    plan, s0 = _plan(gpu, orc, 0, N, Nd)
    try:
        plan.set_noise_shape(wci.shape(plan.Nu))
        which = [None, 2]
        which.insert(bad, 1)  # (wci.ensemble_members(bad): the plan's own env, the heavier hopper, the 1e30 gear at ``bad``)
        plan.set_ensemble([None if k is None else _hopper(k) for k in which], risk)
        if with_objective:
            plan.set_objective(**wci.objective(plan.Nu).kwargs())
        plan.set_weighting(**wi.ESS.kwargs())
        ref = wci.ensemble_step(orc, N, bad, risk, wi.ESS, with_objective, Nd, _impl())
        d_Y, d_rm = torch.tensor(ref["Ybar"].reshape(-1), device="cuda"), torch.zeros(1, device="cuda")
        gpu.check(plan.lib.mbd_plan_reverse_once(plan.h, Nd - 2, gpu.key_array(gpu.prng_key(10 + N)), d_Y.data_ptr(), d_rm.data_ptr(), None))
        torch.cuda.synchronize()
        Y0s, _, w = plan.peek()
        members, comb = plan.peek_ensemble()
        what = f"N={N} bad={bad} {risk}"
        kept = int(np.isfinite(ref["det"]["rews"]).sum())
        print(f"{what}: kept {kept}, temperature {ref['log'][0][0]!r}")
        assert 0 < kept < N and kept == ref["log"][0][2] == int(np.isfinite(comb).sum())
        same_bits(Y0s, ref["det"]["Y0s"], f"{what}: candidates")
        assert np.array_equal(np.isfinite(comb), np.isfinite(ref["det"]["rews"])), f"{what}: which combined rewards are finite"
        _same_log(plan.peek_weighting(), ref["log"], f"{what}: one step")
        same_bits(w, ref["det"]["weights"], f"{what}: weights")
        same_bits(np.float32(d_rm.item()), ref["rew_mean"], f"{what}: mean reward")
        same_bits(d_Y.cpu().numpy().reshape(H, plan.Nu), ref["out"], f"{what}: the new mean")
        key = gpu.prng_key(6)
        ep = plan.run_mpc(key, T, K, E)
        ref = wci.ensemble_episode(orc, N, bad, risk, wi.ESS, with_objective, Nd, _impl())
        assert np.isfinite(ep["means"]).all()
        _equal(ep, ref, f"{what}: episode")
        _same_log(plan.peek_weighting(), ref["log"][-1], f"{what}: the last tick")
    finally:
        plan.close()


# ---- 7. path-integral closed loops -------------------------------------------------------------------------------------------------
def _sigma_record(method):
    """set_mpc_sigma(cold = 1.0, warm = 0.5, gain = 0.9): the gain is cma-es' alone — the set call refuses one on mppi and cem plans,
    whose sigma never changes within a tick (asserted below) — so those two run the record with gain = 0."""
    return (1.0, 0.5, 0.9 if method == 2 else 0.0)


@pytest.mark.parametrize("method", [1, 2, 3], ids=["mppi", "cma-es", "cem"])
def test_path_integral_closed_loops(gpu, orc, method):
    """A sigma record and wi.ESS together: ``Plan.run_mpc`` against ``pic.episode(..., plan_tick=wc.plan_tick)`` — means, rows,
    rewards, states, sigmas [T, 2] and the last tick's log —; a session fed the states returns the same means, and
    mbd_plan_get_sigma between its ticks is what the next one starts from (cma-es: carried from the weigh kernel's weights by
    mpc_pi_sigma_kernel); ``Sweep.run_mpc`` with three temperatures and keys: every episode is its plan run alone, logs included."""
    from mbd_hip.planners.mbd_planner import Plan, Sweep
    N, Nd, P = 64, 5, 3
    sig = _sigma_record(method)
    key = gpu.prng_key(5)
    plan, s0 = _plan(gpu, orc, 0, N, Nd, method)
    try:
        if method != 2:
            with pytest.raises(gpu.MbdError) as e:
                plan.set_mpc_sigma(1.0, 0.5, 0.9)
            assert e.value.code == gpu.MBD_ERR_INVALID and "gain" in str(e.value)
        plan.set_mpc_sigma(*sig)
        plan.set_weighting(**wi.ESS.kwargs())
        ep = plan.run_mpc(key, T, K, E)
        log_ref = []
        tick = functools.partial(wc.plan_tick, rec=wi.ESS, log=log_ref)
        ref = pic.episode(wci.oenv(orc, wci.models()[0]), s0, key, N, H, Nd, wci.TEMP, T, K, E, method, *sig, impl=_impl(), plan_tick=tick)
        print(f"method {method}: sigmas {ep['sigmas'].tolist()}, the checker {ref['sigmas'].tolist()}")
        _equal(ep, ref, f"method {method}", _LOGS + ("sigmas",))
        _same_log(plan.peek_weighting(), wc.ticks_of(log_ref, Nd, K, T)[-1], f"method {method}: the last tick")
        if method == 2:
            assert len({float(x) for x in ref["sigmas"][:, 1]}) == T  # (the carried sigma moves)
        with plan.mpc_open(key, K, E) as s:
            for t in range(T):
                assert np.float32(plan.get_sigma()) == ref["sigmas"][t, 0], f"method {method}: the session's tick {t} starts from"
                same_bits(s.tick(ep["states"][t])["mean"], ep["means"][t], f"method {method}: the session's tick {t}")
            same_bits(np.float32(plan.get_sigma()), pic.next_sigma(ref["sigmas"][-1, 1], *sig), "what a further tick would start from")
    finally:
        plan.close()
    env = _hopper(0)
    temps = [0.05 + 0.1 * k for k in range(P)]
    keys = np.stack([gpu.prng_key(30 + k) for k in range(P)])
    states = [_state(wci.start(orc, wci.models()[0], k, _impl())) for k in range(P)]
    sweep = Sweep(env, _args(wci.NAME, N, Nd, method), P, temps=temps, update_method=method)
    try:
        for k in range(P):
            sweep.set_state0(k, states[k])
        sweep.set_mpc_sigma(*sig)
        sweep.set_weighting(**wi.ESS.kwargs())
        got = sweep.run_mpc(keys, T, K, E)
        logs = [sweep.peek_weighting(k) for k in range(P)]
    finally:
        sweep.close()
    for k in range(P):
        one = Plan(env, _args(wci.NAME, N, Nd, method, temp=temps[k]), update_method=method)
        try:
            one.set_state0(states[k])
            one.set_mpc_sigma(*sig)
            one.set_weighting(**wi.ESS.kwargs())
            alone = one.run_mpc(keys[k], T, K, E)
            log1 = one.peek_weighting()
        finally:
            one.close()
        _equal({f: got[f][k] for f in _LOGS + ("sigmas",)}, alone, f"method {method}, episode {k}", _LOGS + ("sigmas",))
        assert len(log1["temp"]) == K
        for f in ("temp", "ess", "kept"):
            assert np.array_equal(logs[k][f], log1[f]), f"method {method}, episode {k}: log {f}"


# ---- 8. noise shape and basis, plant, delay ----------------------------------------------------------------------------------------
def _compose(obj, Nu, k=None, dkey=None):
    g, W = wci.composed_tables(Nu)
    obj.set_noise_shape(g, "warm")
    obj.set_noise_basis(W, "always")
    obj.set_mpc_delay(1, wci.composed_rows0(Nu))
    plant = dict(env=_hopper(2), key=dkey, act_std=0.05, kick_std=0.02, kick_every=2)
    if k is None:
        obj.set_mpc_plant(**plant)
    else:
        obj.set_mpc_plant(k, **plant)


def test_noise_shape_basis_delay_and_plant_under_a_record(gpu, orc):
    """Warm ticks whose sampling differs from the cold tick's — a noise shape in force from tick 1 on, a knot basis in every step —,
    D = 1 (the ticks plan from the predicted state; the log holds K entries, not Ndiffuse - 1) and a heavier plant with action
    noise and a kick after every second tick, under wi.ESS: against the composed checker.  Then an MBD sweep of two such episodes
    (distinct keys and temperatures): each is its plan alone."""
    from mbd_hip.planners.mbd_planner import Plan, Sweep
    N, Nd = 48, 5
    key, dkey = gpu.prng_key(5), gpu.prng_key(11)
    plan, s0 = _plan(gpu, orc, 0, N, Nd)
    try:
        _compose(plan, plan.Nu, dkey=dkey)
        plan.set_weighting(**wi.ESS.kwargs())
        ep = plan.run_mpc(key, T, K, E)
        ref = wci.composed_episode(orc, wi.ESS, N, Nd, _impl())
        _equal(ep, ref, "composed episode")
        _same_log(plan.peek_weighting(), ref["log"][-1], "the last tick")
        assert len(ref["log"][-1]) == K and len(ref["log"][0]) == Nd - 1
    finally:
        plan.close()
    P, env = 2, _hopper(0)
    temps = [0.1, 0.3]
    keys = np.stack([key, gpu.prng_key(6)])
    sweep = Sweep(env, _args(wci.NAME, N, Nd), P, temps=temps)
    try:
        for k in range(P):
            sweep.set_state0(k, _state(s0))
        g, W = wci.composed_tables(env.action_size)
        sweep.set_noise_shape(g, "warm")
        sweep.set_noise_basis(W, "always")
        sweep.set_mpc_delay(1, wci.composed_rows0(env.action_size))
        for k in range(P):
            sweep.set_mpc_plant(k, env=_hopper(2), key=dkey, act_std=0.05, kick_std=0.02, kick_every=2)
        sweep.set_weighting(**wi.ESS.kwargs())
        got = sweep.run_mpc(keys, T, K, E)
        logs = [sweep.peek_weighting(k) for k in range(P)]
    finally:
        sweep.close()
    same_bits(got["means"][0], ep["means"], "episode 0 is the plan above")
    for k in range(P):
        one = Plan(env, _args(wci.NAME, N, Nd, temp=temps[k]))
        try:
            one.set_state0(_state(s0))
            _compose(one, one.Nu, dkey=dkey)
            one.set_weighting(**wi.ESS.kwargs())
            alone = one.run_mpc(keys[k], T, K, E)
            log1 = one.peek_weighting()
        finally:
            one.close()
        _equal({f: got[f][k] for f in _LOGS}, alone, f"episode {k}")
        for f in ("temp", "ess", "kept"):
            assert np.array_equal(logs[k][f], log1[f]), f"episode {k}: log {f}"


# ---- 9. cem with fewer than ten positive weights -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["few_positive", "one_kept", "all_dropped"])
def test_cem_ties_among_zero_weights(gpu, orc, case):
    """THE RULE, as it is: cem takes the ten largest weights, ties towards the HIGHER index, and a +0 is a +0 — a kept candidate
    whose weight underflowed ties with the dropped ones, so among +0 weights the higher index wins WHETHER THE CANDIDATE WAS KEPT OR
    DROPPED.  ``few_positive``: twelve kept, three positive weights; the other seven places go to the dropped candidates 63 .. 57,
    not to the nine kept ones at the low indices.  ``one_kept``: candidate 32 and the dropped 63 .. 55.  ``all_dropped``: 63 .. 54.
    The new mean is ``wc.cem_mean`` of those indices bit for bit — the sequential sum of ten distinct candidates in selection order,
    which another selection or order does not reproduce (asserted of the checker below); the library has no entry that returns
    cem_select_kernel's indices themselves."""
    N = 64
    rews, rec = wci.cem_ties(N)[case]
    step = _Step(gpu, "hopper", N, 3)
    try:
        step.plan.set_weighting(**rec.kwargs())
        mu, w, _ = step.update(rews)
        res = wc.weigh(orc, rews, wi.TEMP, rec)
        same_bits(w, res["weights"], f"{case}: weights")
        same_bits(mu, wc.cem_mean(res["weights"], step.Y0s).reshape(mu.shape), f"{case}: the new mean against wc.cem_mean")
        # ... and wc.cem_mean is the rule as the docstring states it, written out by hand
        idx = {"few_positive": [41, 20, 3] + list(range(63, 56, -1)), "one_kept": [32] + list(range(63, 54, -1)),
               "all_dropped": list(range(63, 53, -1))}[case]
        assert all(res["weights"][a] > res["weights"][b] or (res["weights"][a] == res["weights"][b] and a > b) for a, b in zip(idx, idx[1:]))
        assert all(res["weights"][n] <= res["weights"][idx[-1]] for n in range(N) if n not in idx)
        Y = step.Y0s.reshape(N, -1)
        acc = np.zeros(Y.shape[1], np.float32)
        for n in idx:
            acc = (acc + Y[n]).astype(np.float32)
        same_bits(mu, (acc / np.float32(10)).astype(np.float32).reshape(mu.shape), f"{case}: the new mean against the indices by hand")
        if case == "few_positive":  # (the selection that prefers kept candidates gives another mean: the test can tell)
            kept_first = [41, 20, 3] + [9, 8, 7, 6, 5, 4, 2]
            assert not np.array_equal(Y[kept_first].sum(axis=0), Y[idx].sum(axis=0))
            assert np.isfinite(rews[[0, 1, 2, 4, 5, 6, 7, 8, 9]]).all() and not np.isfinite(rews[57:]).any()
    finally:
        step.plan.close()


# ---- 10. a demo record and a weighting record ----------------------------------------------------------------------------------------
def test_demo_record_and_weighting_record_never_meet(gpu):
    """Today's answer, pinned: no plan can hold both records, in either order.  A demo record needs an enable_demo plan
    (mbd_plan_set_mpc_demo refuses every other plan with MBD_ERR_INVALID, naming enable_demo), and mbd_plan_set_weighting refuses
    every enable_demo plan with MBD_ERR_UNSUPPORTED, naming the demo — before and after a demo record is set; the refused call
    leaves the plan as it was."""
    import mpc_demo_checker as mdc
    from mbd_hip.planners.mbd_planner import Args, Plan
    track = _env("humanoidtrack")
    clip = mdc.extended(np.asarray(track.xref, np.float32))
    demo = Plan(track, Args(env_name="humanoidtrack", Nsample=33, Hsample=50, Ndiffuse=3, enable_demo=True, disable_recommended_params=True,
                            not_render=True))
    try:
        for order in ("weighting first", "demo first"):
            if order == "demo first":
                demo.set_mpc_demo(clip, 2, 1.0)
            with pytest.raises(gpu.MbdError) as e:
                demo.set_weighting(**wi.ESS.kwargs())
            assert e.value.code == gpu.MBD_ERR_UNSUPPORTED and "weighting record" in str(e.value) and "demo" in str(e.value), order
            with pytest.raises(gpu.MbdError) as e:
                demo.peek_weighting()
            assert e.value.code == gpu.MBD_ERR_STATE, order  # (no record was left behind)
            if order == "weighting first":
                demo.set_mpc_demo(clip, 2, 1.0)  # (the refused weighting record does not stand in a demo record's way)
                demo.clear_mpc_demo()
    finally:
        demo.close()
    plain = Plan(track, Args(env_name="humanoidtrack", Nsample=33, Hsample=50, Ndiffuse=3, disable_recommended_params=True, not_render=True))
    try:
        plain.set_weighting(**wi.ESS.kwargs())
        with pytest.raises(gpu.MbdError) as e:
            plain.set_mpc_demo(clip, 2, 1.0)
        assert e.value.code == gpu.MBD_ERR_INVALID and "demo record" in str(e.value) and "enable_demo=0" in str(e.value)
        plain.clear_weighting()
        with pytest.raises(gpu.MbdError) as e:
            plain.set_mpc_demo(clip, 2, 1.0)
        assert e.value.code == gpu.MBD_ERR_INVALID  # (the refusal is the plan's, with or without a weighting record)
    finally:
        plain.close()
