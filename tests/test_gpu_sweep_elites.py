"""-m gpu: the elite record in sweeps (include/mbd_hip.h mbd_sweep_set_elites, DESIGN.md section 1 "N18 elites") by bit pattern.

  the launches alone   elite_inject_batch_kernel and elite_select_batch_kernel through mbd_debug_sweep_elites_step against the checker
                       (tests/elites_checker.py) per plan: P in {1, 3, 8, 32} x N in {2, 63, 64, 65, 1023, 1024, 1025, 8193, 12288} x
                       k in {1, 5, 32}, with and without the nominal, lazy and materialised; every plan of a launch draws another
                       reward kind of tests/elites_inputs.py and another incoming count; a mask with some plans off, whose outputs
                       keep what they held
  sweeps and plans     hopper, N = 80, Ndiffuse = 4, P in {3, 8}, MBD and mppi: plan k of the sweep is the Plan alone, elites and log
                       included; under a noise shape and a 3-knot basis; beside an objective and a weighting record; beside a to-go
                       record
  isolation            one plan of three starts from a state whose candidates all diverge: the others keep their bits
  episodes, sessions   cartpole, T = 3, K = 2, E = 1, P = 3: carry on and off, a delay record, a pick record, mppi under a sigma record;
                       a session fed the episodes' states; a mixed tick after reset_mean(1)
  set, clear, refusals every refusal's code and the field or record its message names"""
import ctypes as C

import numpy as np
import pytest

import elites_checker as ec
import elites_inputs as inputs
import sweep_records_cases as sc
from state_inputs import same_bits
from test_gpu_noise_shape import _env

pytestmark = pytest.mark.gpu
f32 = np.float32
NS = (2, 63, 64, 65, 1023, 1024, 1025, 8193, 12288)  # (12289 stays a plan-only size: sweeps cap at 12288)
PS = (1, 3, 8, 32)
HNU = inputs.HNU
ONES = 0xffffffff


@pytest.fixture(scope="module")
def gpu(lib):
    from mbd_hip import _capi
    if _capi.device_count() < 1:
        pytest.fail("tests/test_gpu_sweep_elites.py needs a GPU")
    return _capi


# ---- the launches alone ------------------------------------------------------------------------------------------------------------
def _launch_inputs(P, N, k, lazy, seed):
    """P plans' rews, cand, ybar, E_in, count_in and the one shape: plan p draws kind p + seed of KINDS and count (p + seed) % (k + 1)."""
    rng = np.random.default_rng([P, N, k, int(lazy), seed])
    cand = rng.standard_normal((P, N, HNU)).astype(f32)
    if not lazy:
        cand = ec.clip(cand * f32(0.6))
    ybar = (rng.standard_normal((P, HNU)) * 0.4).astype(f32)
    ybar[:, 0] = f32(1.5)  # (outside the clip: the nominal of a materialised plan is clip(Ybar))
    g = (0.5 + rng.random(HNU)).astype(f32)
    g[2] = 0.0
    E_in = ec.clip(rng.standard_normal((P, k, HNU)) * 0.8)
    count = np.array([(p + seed) % (k + 1) for p in range(P)], np.int32)
    kinds = [inputs.KINDS[(p + seed) % len(inputs.KINDS)] for p in range(P)]
    rews = np.stack([inputs.rewards(N, kinds[p], seed=p) for p in range(P)])
    return rews, cand, ybar, g, E_in, count, kinds


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("N", NS)
def test_the_launches_alone(gpu, N):
    seed = 0
    for P in PS:
        mask = ONES if P == 1 else ONES & ~0b10 & ~(1 << (P - 1))  # (plans 1 and P - 1 off)
        for k in inputs.KS:
            for nominal in (0, 1):
                if k + nominal >= N:
                    continue
                for lazy in (True, False):
                    seed += 1
                    rews, cand, ybar, g, E_in, count, kinds = _launch_inputs(P, N, k, lazy, seed)
                    shape = g if seed % 2 else None
                    got = gpu.debug_sweep_elites_step(rews, cand, ybar, inputs.SIGMA, lazy, shape, k, nominal, E_in, count, mask)
                    rec = ec.Record(n_elites=k, nominal=bool(nominal), carry=False)
                    for p in range(P):
                        what = f"P={P} N={N} k={k} nominal={nominal} lazy={lazy} plan {p} ({kinds[p]}, count {count[p]})"
                        c = int(count[p])
                        if not (mask >> p) & 1:  # a plan left out: nothing of it is read or written
                            same_bits(got["cand"][p], cand[p], f"{what}: masked out: cand")
                            same_bits(got["E"][p, :c], E_in[p, :c], f"{what}: masked out: E")
                            assert (_bits(got["E"][p, c:]) == ONES).all() and (_bits(got["R"][p]) == ONES).all(), what
                            assert (got["src"][p] == -1).all() and got["count"][p] == c and got["kept"][p] == -1, what
                            assert _bits(got["top"][p:p + 1])[0] == ONES, what
                            continue
                        ref = ec.step(rews[p], cand[p], ybar[p], inputs.SIGMA, lazy, shape, rec, E_in[p, :c])
                        n = ref["count"]
                        same_bits(got["cand"][p], ref["cand"], f"{what}: the candidates behind the injection")
                        assert got["count"][p] == n and got["kept"][p] == ref["kept"], f"{what}: count {got['count'][p]} / {n}"
                        same_bits(got["top"][p], np.asarray(ref["top"], f32), f"{what}: top")
                        assert list(got["src"][p, :n]) == list(ref["src"]), f"{what}: src"
                        same_bits(got["R"][p, :n], ref["R"], f"{what}: R")
                        same_bits(got["E"][p, :n], ref["E"], f"{what}: E")
                        assert (_bits(got["R"][p, n:]) == ONES).all() and (got["src"][p, n:] == -1).all(), f"{what}: behind count'"
                        same_bits(got["E"][p, n:max(n, c)], E_in[p, n:max(n, c)], f"{what}: rows the selection did not reach")
                        assert (_bits(got["E"][p, max(n, c):]) == ONES).all(), f"{what}: E behind count' is untouched"


# ---- sweeps equal their plans alone ---------------------------------------------------------------------------------------------------
def _elites(h):
    h.set_elites(3, True, False)


def _both(h):
    h.set_elites(3, True, False)
    h.set_togo(**sc.TOGO)


@pytest.mark.parametrize("P", [3, 8])
@pytest.mark.parametrize("method", [0, 1], ids=["mbd", "mppi"])
@pytest.mark.parametrize("records", [_elites, _both], ids=["e3n", "e3n+togo"])
def test_sweeps_equal_their_plans_alone(gpu, P, method, records):
    sc.run_equals_plans(gpu, _env(sc.NAME), sc.args(sc.NAME, sc.N, sc.H, sc.ND), P, method, records, f"P={P} method={method}")


def test_under_a_noise_shape_and_a_basis(gpu):
    from noise_basis_checker import basis_of
    from test_gpu_noise_shape import shape_of
    env = _env(sc.NAME)

    def configure(h):
        h.set_noise_shape(shape_of(sc.H, env.action_size), "always")  # (a frozen row: an elite's normal there stays +0)
        h.set_noise_basis(basis_of(sc.H, 3), "always")
        _both(h)
    sc.run_equals_plans(gpu, env, sc.args(sc.NAME, sc.N, sc.H, sc.ND), 3, 0, configure, "shape and basis")


@pytest.mark.parametrize("kind", ["objective", "weighting"])
def test_beside_another_record(gpu, kind):
    env = _env(sc.NAME)
    prev0 = np.linspace(-0.5, 0.5, env.action_size).astype(f32)

    def configure(h):
        if kind == "objective":
            h.set_objective(effort=0.05, rate=0.5, prev0=prev0)
        else:
            h.set_weighting(reject_nonfinite=True, ess_frac=0.3, temp_min=0.01, temp_max=10.0)
        _elites(h)
    sc.run_equals_plans(gpu, env, sc.args(sc.NAME, sc.N, sc.H, sc.ND), 3, 0, configure, kind)


# ---- isolation ---------------------------------------------------------------------------------------------------------------------
def test_a_diverged_plan_stays_alone(gpu):
    """Plan 1 of three starts with the root's angular velocity at 3e38 (tests/containment_inputs.py): plans 0 and 2 keep the single
    plan's bits, and plan 1's count' is its finite count, the single plan's."""
    import containment_inputs as ci
    from mbd_hip.envs.base import State
    env, P = _env(sc.NAME), 3
    a = sc.args(sc.NAME, sc.N, sc.H, sc.ND)
    states, keys, temps = sc.inputs(gpu, env, P)
    s = np.asarray(states[1].pipeline_state, f32)
    states[1] = State(ci.poison_state(s.reshape(-1, 13)).reshape(s.shape), None, f32(0), f32(0), {})
    sw = sc.make_sweep(env, a, P, states, temps, 0, _both)
    try:
        mu, rm = sw.run(keys)[:2]
        for k in range(P):
            plan = sc.make_plan(env, a, states[k], temps[k], 0, _both)
            try:
                pmu, prm = plan.run(keys[k])[:2]
                if k != 1:
                    same_bits(mu[k], pmu, f"plan {k}: mu_0ts")
                    same_bits(rm[k], prm, f"plan {k}: mean rewards")
                    sc.same_records(sw, k, plan, f"plan {k}")
                    assert np.isfinite(mu[k]).all()
                else:
                    got, ref = sw.peek_elites(1), plan.peek_elites()
                    finite = int(np.isfinite(sw.peek_togo(1)["R"][0]).sum())  # (row 0: the rewards the score read)
                    assert finite < 3, "the poisoned plan's candidates diverge"
                    assert got["count"] == ref["count"] == finite, (got["count"], ref["count"], finite)
                    assert np.array_equal(got["log_count"], ref["log_count"])
            finally:
                plan.close()
    finally:
        sw.close()


# ---- episodes and sessions ---------------------------------------------------------------------------------------------------------
EPISODES = {"carry": dict(carry=True), "no_carry": dict(carry=False), "delay": dict(carry=True, D=1), "pick": dict(carry=True, pick=True),
            "mppi": dict(carry=True, method=1)}


def _episode_records(case):
    def configure(h):
        if case.get("D"):
            h.set_mpc_delay(case["D"])
        if case.get("pick"):
            h.set_mpc_pick(True, True, True)
        if case.get("method"):
            h.set_mpc_sigma(**sc.SIGMA)
        h.set_elites(3, True, case["carry"])
    return configure


@pytest.mark.parametrize("case", list(EPISODES), ids=list(EPISODES))
def test_episodes_and_sessions(gpu, case):
    """Sweep.run_mpc per episode equals Plan.run_mpc, elites and log included; a sweep's session fed those states returns the same
    means, elites and log (MBD: sessions of path-integral sweeps stay refused)."""
    c, e = EPISODES[case], sc.EP
    env, P, method = _env(e["name"]), e["P"], c.get("method", 0)
    a = sc.args(e["name"], e["N"], 20, e["Nd"])
    states, keys, temps = sc.inputs(gpu, env, P)
    configure = _episode_records(c)
    sw = sc.make_sweep(env, a, P, states, temps, method, configure)
    try:
        out = sw.run_mpc(keys, e["T"], e["K"], e["E"])
        peeks = [sw.peek_elites(k) for k in range(P)]
        for k in range(P):
            plan = sc.make_plan(env, a, states[k], temps[k], method, configure)
            try:
                ep = plan.run_mpc(keys[k], e["T"], e["K"], e["E"])
                sc.same_episode(out, k, ep, case)
                sc.same_elites(peeks[k], plan.peek_elites(), f"{case}: episode {k}")
                assert peeks[k]["steps"] == (e["Nd"] - 1) + (e["T"] - 1) * e["K"]
            finally:
                plan.close()
        if method:
            return
        with sw.mpc_open(keys, e["K"], e["E"]) as s:
            for t in range(e["T"]):
                o = s.tick(np.ascontiguousarray(out["states"][:, t]))
                same_bits(o["mean"], out["means"][:, t], f"{case}: the session's means of tick {t}")
            for k in range(P):
                sc.same_elites(sw.peek_elites(k), peeks[k], f"{case}: the session: episode {k}")
    finally:
        sw.close()


def test_a_mixed_tick(gpu):
    """reset_mean(1) after tick 1: episode 1's next tick is cold and runs Ndiffuse - 1 steps; episodes 0 and 2 idle through the steps
    above K and take no part in the record's launches there.  Episode 1 equals a single session with reset_mean, episodes 0 and 2
    ones without, elites, counts and logs included."""
    e = sc.EP
    env, P = _env(e["name"]), e["P"]
    a = sc.args(e["name"], e["N"], 20, e["Nd"])
    states, keys, temps = sc.inputs(gpu, env, P)
    configure = _episode_records(EPISODES["carry"])
    fed = [np.stack([np.asarray(env.reset(gpu.prng_key(60 + 3 * t + k)).pipeline_state, f32).reshape(-1) for k in range(P)])
           for t in range(e["T"])]
    sw = sc.make_sweep(env, a, P, states, temps, 0, configure)
    try:
        means = []
        with sw.mpc_open(keys, e["K"], e["E"]) as s:
            for t in range(e["T"]):
                if t == 2:
                    s.reset_mean(1)
                    assert sw.peek_elites(1)["count"] == 0 and sw.peek_elites(0)["count"] == 3, "reset_mean(1) empties episode 1's alone"
                means.append(s.tick(fed[t])["mean"])
            peeks = [sw.peek_elites(k) for k in range(P)]
        for k in range(P):
            plan = sc.make_plan(env, a, states[k], temps[k], 0, configure)
            try:
                with plan.mpc_open(keys[k], e["K"], e["E"]) as s:
                    for t in range(e["T"]):
                        if t == 2 and k == 1:
                            s.reset_mean()
                        same_bits(means[t][k], s.tick(fed[t][k])["mean"], f"tick {t}: episode {k}: mean")
                    sc.same_elites(peeks[k], plan.peek_elites(), f"episode {k}")
            finally:
                plan.close()
        assert peeks[1]["steps"] == 2 * (e["Nd"] - 1) + e["K"] and peeks[0]["steps"] == (e["Nd"] - 1) + 2 * e["K"]
    finally:
        sw.close()


# ---- set, clear and refusals ----------------------------------------------------------------------------------------------------------
def test_set_and_clear_give_back_the_bits(gpu):
    env, P = _env(sc.NAME), 3
    a = sc.args(sc.NAME, sc.N, sc.H, sc.ND)
    states, keys, temps = sc.inputs(gpu, env, P)
    sw = sc.make_sweep(env, a, P, states, temps, 0, lambda h: None)
    try:
        mu0, rm0 = sw.run(keys)[:2]
        ep0 = sw.run_mpc(keys, 3, 2, 1)
        sw.set_elites(3, True, True)
        assert sw.has_elites and sw.peek_elites(2)["count"] == 0
        assert not np.array_equal(sw.run(keys)[0], mu0), "a record changes the plans"
        assert not np.array_equal(sw.run_mpc(keys, 3, 2, 1)["means"], ep0["means"])
        sw.clear_elites()
        assert not sw.has_elites
        mu2, rm2 = sw.run(keys)[:2]
        same_bits(mu2, mu0, "set and cleared: mu_0ts")
        same_bits(rm2, rm0, "set and cleared: mean rewards")
        ep2 = sw.run_mpc(keys, 3, 2, 1)
        for k in ("means", "actions", "states", "rewards"):
            same_bits(ep2[k], ep0[k], f"set and cleared: the episodes' {k}")
        with pytest.raises(gpu.MbdError) as e:
            sw.peek_elites(0)
        assert e.value.code == gpu.MBD_ERR_STATE and "elite record" in str(e.value)
    finally:
        sw.close()


def test_refusals(gpu):
    from mbd_hip.planners.mbd_planner import Args, Sweep
    env = _env(sc.NAME)
    a = sc.args(sc.NAME, sc.N, sc.H, sc.ND)
    lib = gpu.load()
    sw = Sweep(env, a, 2)
    try:
        for rec, field in ((gpu.elites_record(33), "n_elites=33"), (gpu.elites_record(0, False), "n_elites=0")):
            assert lib.mbd_sweep_set_elites(sw.h, C.byref(rec)) == gpu.MBD_ERR_INVALID and field.encode() in lib.mbd_last_error(), field
        tiny = Sweep(env, sc.args(sc.NAME, 4, sc.H, sc.ND), 2)
        try:
            with pytest.raises(gpu.MbdError) as e:
                tiny.set_elites(3, True)  # (n_elites + nominal >= Nsample)
            assert e.value.code == gpu.MBD_ERR_INVALID and "Nsample=4" in str(e.value)
        finally:
            tiny.close()
        rec = gpu.elites_record(3, True, True)
        rec.reserved[2] = 1
        assert lib.mbd_sweep_set_elites(sw.h, C.byref(rec)) == gpu.MBD_ERR_INVALID and b"reserved[2]" in lib.mbd_last_error()
        sw.set_elites(3, True, True)
        for k in (-1, 2):
            with pytest.raises(gpu.MbdError) as e:
                sw.peek_elites(k)
            assert e.value.code == gpu.MBD_ERR_INVALID and f"k={k}" in str(e.value)
        with sw.mpc_open(np.stack([gpu.prng_key(1), gpu.prng_key(2)]), 2, 1):
            for call in (lambda: sw.set_elites(3, True, True), sw.clear_elites):
                with pytest.raises(gpu.MbdError) as e:
                    call()
                assert e.value.code == gpu.MBD_ERR_STATE and "session" in str(e.value)
    finally:
        sw.close()
    for method in (2, 3):
        pi = Sweep(env, a, 2, update_method=method)
        try:
            with pytest.raises(gpu.MbdError) as e:
                pi.set_elites(3, True, True)
            assert e.value.code == gpu.MBD_ERR_UNSUPPORTED and f"update_method={method}" in str(e.value)
        finally:
            pi.close()
    track = _env("humanoidtrack")
    demo = Sweep(track, Args(env_name="humanoidtrack", Nsample=64, Hsample=50, Ndiffuse=3, enable_demo=True, disable_recommended_params=True,
                             not_render=True), 2)
    try:
        with pytest.raises(gpu.MbdError) as e:
            demo.set_elites(3, True, True)
        assert e.value.code == gpu.MBD_ERR_UNSUPPORTED and "enable_demo" in str(e.value)
    finally:
        demo.close()


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------
def test_a_batch_of_episodes_honours_the_flags(gpu):
    """mpc.run_mpc_batch under --elites 3 --elite_nominal --elite_carry --togo_block 5: episode k is mpc.run_mpc of its arguments, the
    elites, their log and the to-go values included."""
    from dataclasses import replace

    from mbd_hip.planners import mpc
    e = sc.EP
    base = mpc.MpcArgs(env_name=e["name"], Nsample=e["N"], Hsample=20, Ndiffuse=e["Nd"], temp_sample=0.1, disable_recommended_params=True,
                       not_render=True, n_ticks=e["T"], warm_steps=e["K"], exec_steps=e["E"], elites=3, elite_nominal=True,
                       elite_carry=True, togo_block=5, togo_min_tail=3)
    arg_list = [replace(base, seed=2 + k, temp_sample=0.1 * (1 + k)) for k in range(3)]
    rewards, dets = mpc.run_mpc_batch([replace(a) for a in arg_list], return_details=True)
    for k, a in enumerate(arg_list):
        r, one = mpc.run_mpc(replace(a), return_details=True)
        assert r == rewards[k]
        same_bits(dets[k]["means"], one["means"], f"episode {k}: means")
        sc.same_elites(dets[k]["elite_log"], one["elite_log"], f"episode {k}")
        sc.same_togo(dets[k]["togo"], one["togo"], f"episode {k}")
        assert dets[k]["elites"] == 3 and dets[k]["elite_carry"] is True and dets[k]["togo_block"] == 5
