"""-m gpu: the to-go record in sweeps (include/mbd_hip.h mbd_sweep_set_togo, DESIGN.md section 1 "N19 to-go") by bit pattern, with a
NaN where and only where the reference has one.

  the launches alone   togo_returns_batch_kernel and togo_update_batch_kernel through mbd_debug_sweep_togo_step per plan: N in {1, 65,
                       1025, 12288} x the widths of tests/sweep_update_inputs.py and Nu = 1 with H in {15, 16, 17, 33} (partial last
                       tiles) x block in {1, 5, H - 1, H} x min_tail in {1, 10}; P in {1, 3, 8, 32} and the six modes (lazy or
                       materialised; MBD literal, MBD identity, mppi) rotate over them; a temperature per plan; one plan with a NaN in
                       one entry of rewss.  The reference is the checker (tests/togo_checker.py: the oracle's update once per group)
                       while a case's P G N H Nu stays below CHECKER_WORK; beyond, the single-plan launches mbd_debug_togo_step, which
                       tests/test_gpu_togo.py holds to that checker, once per plan at the plan's temperature
  sweeps and plans     hopper, N = 80, H = 50, Ndiffuse = 4, block 10 with min_tail 5, P in {3, 8}, MBD and mppi
  episodes, sessions   cartpole, T = 3, K = 2, E = 1, P = 3: MBD, a delay record, mppi under a sigma record; a session; a mixed tick
  set, clear, refusals every refusal's code and the field or record its message names, both ways round"""
import ctypes as C

import numpy as np
import pytest

import sweep_records_cases as sc
import sweep_update_inputs as sui
import togo_checker as tc
import togo_inputs as ti
from state_inputs import same_bits
from test_gpu_noise_shape import _env

pytestmark = pytest.mark.gpu
f32 = np.float32
NS = (1, 65, 1025, 12288)
PS = (1, 3, 8, 32)
# (H, Nu): the sweeps' widths H Nu = 7, 90, 340, and one actuator at horizons around the 16-element tile
NU = {"cartpole": 1, "hopper": 3, "humanoidrun": 17}
SHAPES = tuple((h, NU[n]) for n, h in sui.WIDTHS) + ((15, 1), (16, 1), (17, 1), (33, 1))
# the oracle runs one whole update per group: about six million candidate elements a second
CHECKER_WORK = 1_500_000


@pytest.fixture(scope="module")
def gpu(lib):
    from mbd_hip import _capi
    if _capi.device_count() < 1:
        pytest.fail("tests/test_gpu_sweep_togo.py needs a GPU")
    return _capi


def _same(got, ref, what):
    ti.same(got, ref, what, same_bits)


def _temps(P):
    return np.array([0.1 * (1 + p % 3) + 0.01 * p for p in range(P)], f32)


# ---- the launches alone ------------------------------------------------------------------------------------------------------------
def _cases(N, H, Nu, base):
    out = []
    for bi, block in enumerate((1, 5, H - 1, H)):
        for mi, mt in enumerate((1, 10)):
            r = base + bi + 2 * mi
            lazy, (method, literal) = ti.MODES[r % len(ti.MODES)]
            out.append(dict(P=PS[r % len(PS)], block=max(block, 1), min_tail=min(mt, H), lazy=lazy, method=method, literal=literal))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=[f"H{h}-Nu{u}" for h, u in SHAPES])
@pytest.mark.parametrize("N", NS)
def test_the_launches_alone(gpu, orc, N, shape):
    H, Nu = shape
    for c in _cases(N, H, Nu, NS.index(N) + SHAPES.index(shape)):
        P, block, mt, lazy, method, literal = c["P"], c["block"], c["min_tail"], c["lazy"], c["method"], c["literal"]
        what0 = f"N={N} H={H} Nu={Nu} P={P} block={block} min_tail={mt} lazy={lazy} method={method} literal={literal}"
        starts = tc.groups(H, block, mt)
        G, bad = len(starts), P // 2
        g = np.random.default_rng([N, H, Nu, P, block, mt])
        ybar = (g.normal(size=(P, H, Nu)) * 0.3).astype(f32)
        z = g.normal(size=(P, N, H, Nu)).astype(f32)
        cand = z if lazy else np.stack([ti.values(z[p], ti.SIGMA, ybar[p]) for p in range(P)])
        rr = [ti.rewards("nan_step_t" if p == bad else "random", N, H, 5 + p) for p in range(P)]
        rews, rewss, t_bad = np.stack([r[0] for r in rr]), np.stack([r[1] for r in rr]), rr[bad][2]
        temps = _temps(P)
        got = gpu.debug_sweep_togo_step(temps, cand, ybar, rews, rewss, Nu, block, mt, lazy, ti.SIGMA, method == 0, *ti.ALPHAS, literal, G)
        by_checker = P * G * N * H * Nu <= CHECKER_WORK
        for p in range(P):
            what = f"{what0}: plan {p}"
            if by_checker:
                Y = ti.values(cand[p], ti.SIGMA, ybar[p]) if lazy else cand[p]
                ref = tc.update(orc, method, rews[p], rewss[p], Y, ybar[p], starts, float(temps[p]), alphas=ti.ALPHAS, literal=literal,
                                sigma=ti.SIGMA)
                ref = dict(ybar=ref["out"], R=ref["R"], W=ref["W"], rew_mean=ref["rew_mean"])
            else:
                ref = gpu.debug_togo_step(cand[p], ybar[p], rews[p], rewss[p], Nu, block, mt, lazy, ti.SIGMA, float(temps[p]), method == 0,
                                          *ti.ALPHAS, literal, G)
            for name in ("R", "W", "ybar", "rew_mean"):
                _same(got[name][p], ref[name], f"{what}: {name}")
            if p != bad:
                assert np.isfinite(got["R"][p]).all(), f"{what}: another plan's NaN reached its returns"
                if not (method == 1 and N == 1):  # (mppi's standard deviation of one candidate is 0: NaN by the rule itself)
                    assert np.isfinite(got["W"][p]).all() and np.isfinite(got["ybar"][p]).all(), f"{what}: another plan's NaN reached it"
                continue
            for j, s in enumerate(starts):  # the NaN of step t_bad reaches exactly the groups that start at or below it
                assert np.isnan(got["R"][p, j, N // 2]) == (s <= t_bad), f"{what}: group {j} (s = {s}, t = {t_bad})"
                if s > t_bad and not (method == 1 and N == 1):
                    end = starts[j + 1] if j + 1 < G else H
                    assert np.isfinite(got["W"][p, j]).all() and np.isfinite(got["ybar"][p, s:end]).all(), f"{what}: group {j} stays finite"


# ---- sweeps equal their plans alone ---------------------------------------------------------------------------------------------------
def _togo(h):
    h.set_togo(**sc.TOGO)


@pytest.mark.parametrize("P", [3, 8])
@pytest.mark.parametrize("method", [0, 1], ids=["mbd", "mppi"])
def test_sweeps_equal_their_plans_alone(gpu, P, method):
    sc.run_equals_plans(gpu, _env(sc.NAME), sc.args(sc.NAME, sc.N, sc.H, sc.ND), P, method, _togo, f"P={P} method={method}")


# ---- episodes and sessions ---------------------------------------------------------------------------------------------------------
EPISODES = {"mbd": dict(), "delay": dict(D=1), "mppi": dict(method=1)}


def _episode_records(case):
    def configure(h):
        if case.get("D"):
            h.set_mpc_delay(case["D"])
        if case.get("method"):
            h.set_mpc_sigma(**sc.SIGMA)
        h.set_togo(5, 3)  # (H = 20: groups at rows 0, 5, 10, 15)
    return configure


@pytest.mark.parametrize("case", list(EPISODES), ids=list(EPISODES))
def test_episodes_and_sessions(gpu, case):
    c, e = EPISODES[case], sc.EP
    env, P, method = _env(e["name"]), e["P"], c.get("method", 0)
    a = sc.args(e["name"], e["N"], 20, e["Nd"])
    states, keys, temps = sc.inputs(gpu, env, P)
    configure = _episode_records(c)
    sw = sc.make_sweep(env, a, P, states, temps, method, configure)
    try:
        out = sw.run_mpc(keys, e["T"], e["K"], e["E"])
        peeks = [sw.peek_togo(k) for k in range(P)]
        for k in range(P):
            plan = sc.make_plan(env, a, states[k], temps[k], method, configure)
            try:
                sc.same_episode(out, k, plan.run_mpc(keys[k], e["T"], e["K"], e["E"]), case)
                sc.same_togo(peeks[k], plan.peek_togo(), f"{case}: episode {k}")
            finally:
                plan.close()
        if method:
            return
        with sw.mpc_open(keys, e["K"], e["E"]) as s:
            for t in range(e["T"]):
                o = s.tick(np.ascontiguousarray(out["states"][:, t]))
                same_bits(o["mean"], out["means"][:, t], f"{case}: the session's means of tick {t}")
            for k in range(P):
                sc.same_togo(sw.peek_togo(k), peeks[k], f"{case}: the session: episode {k}")
    finally:
        sw.close()


def test_a_mixed_tick(gpu):
    """reset_mean(1) after tick 1: every episode's means equal a single session's, episode 1's with the reset."""
    e = sc.EP
    env, P = _env(e["name"]), e["P"]
    a = sc.args(e["name"], e["N"], 20, e["Nd"])
    states, keys, temps = sc.inputs(gpu, env, P)
    configure = _episode_records(EPISODES["mbd"])
    fed = [np.stack([np.asarray(env.reset(gpu.prng_key(60 + 3 * t + k)).pipeline_state, f32).reshape(-1) for k in range(P)])
           for t in range(e["T"])]
    sw = sc.make_sweep(env, a, P, states, temps, 0, configure)
    try:
        means = []
        with sw.mpc_open(keys, e["K"], e["E"]) as s:
            for t in range(e["T"]):
                if t == 2:
                    s.reset_mean(1)
                means.append(s.tick(fed[t])["mean"])
            peeks = [sw.peek_togo(k) for k in range(P)]
        for k in range(P):
            plan = sc.make_plan(env, a, states[k], temps[k], 0, configure)
            try:
                with plan.mpc_open(keys[k], e["K"], e["E"]) as s:
                    for t in range(e["T"]):
                        if t == 2 and k == 1:
                            s.reset_mean()
                        same_bits(means[t][k], s.tick(fed[t][k])["mean"], f"tick {t}: episode {k}: mean")
                    sc.same_togo(peeks[k], plan.peek_togo(), f"episode {k}")
            finally:
                plan.close()
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
        sw.set_togo(**sc.TOGO)
        assert sw.has_togo and np.isnan(sw.peek_togo(1)["R"]).all(), "before the record's first step R is all-ones bits"
        assert not np.array_equal(sw.run(keys)[0], mu0), "a record changes the plans"
        assert sw.peek_togo(0)["starts"].tolist() == [0, 10, 20, 30, 40]
        sw.clear_togo()
        assert not sw.has_togo
        mu2, rm2 = sw.run(keys)[:2]
        same_bits(mu2, mu0, "set and cleared: mu_0ts")
        same_bits(rm2, rm0, "set and cleared: mean rewards")
        with pytest.raises(gpu.MbdError) as e:
            sw.peek_togo(0)
        assert e.value.code == gpu.MBD_ERR_STATE and "to-go record" in str(e.value)
    finally:
        sw.close()


def test_refusals(gpu):
    from mbd_hip.planners.mbd_planner import Args, Sweep
    import value_inputs as vi
    env = _env(sc.NAME)
    a = sc.args(sc.NAME, sc.N, sc.H, sc.ND)
    lib = gpu.load()
    sw = Sweep(env, a, 2)
    try:
        for rec, field in ((gpu.togo_record(0, 1), "block=0"), (gpu.togo_record(1, 0), "min_tail=0"), (gpu.togo_record(1, sc.H + 1), "min_tail=")):
            assert lib.mbd_sweep_set_togo(sw.h, C.byref(rec)) == gpu.MBD_ERR_INVALID and field.encode() in lib.mbd_last_error(), field
        # beside the sweep's objective, value or weighting record: either way round
        others = {"objective": (lambda: sw.set_objective(effort=0.05), sw.clear_objective),
                  "value": (lambda: sw.set_value(vi.net(sc.NAME, "S-65-64-1", "tanh", rel_xy=True, scale=0.37).value_net()), lambda: sw.set_value(None)),
                  "weighting": (lambda: sw.set_weighting(reject_nonfinite=True), sw.clear_weighting)}
        for name, (set_, clear) in others.items():
            set_()
            with pytest.raises(gpu.MbdError) as e:
                sw.set_togo(**sc.TOGO)
            assert e.value.code == gpu.MBD_ERR_UNSUPPORTED and f"{name} record" in str(e.value), name
            clear()
            sw.set_togo(**sc.TOGO)
            with pytest.raises(gpu.MbdError) as e:
                set_()
            assert e.value.code == gpu.MBD_ERR_UNSUPPORTED and f"{name} record" in str(e.value) and "to-go record" in str(e.value), name
            sw.clear_togo()
        sw.set_togo(**sc.TOGO)
        sw.set_elites(3, True, False)  # (the two compose)
        for k in (-1, 2):
            with pytest.raises(gpu.MbdError) as e:
                sw.peek_togo(k)
            assert e.value.code == gpu.MBD_ERR_INVALID and f"k={k}" in str(e.value)
        with sw.mpc_open(np.stack([gpu.prng_key(1), gpu.prng_key(2)]), 2, 1):
            for call in (lambda: sw.set_togo(**sc.TOGO), sw.clear_togo):
                with pytest.raises(gpu.MbdError) as e:
                    call()
                assert e.value.code == gpu.MBD_ERR_STATE and "session" in str(e.value)
    finally:
        sw.close()
    for method in (2, 3):
        pi = Sweep(env, a, 2, update_method=method)
        try:
            with pytest.raises(gpu.MbdError) as e:
                pi.set_togo(**sc.TOGO)
            assert e.value.code == gpu.MBD_ERR_UNSUPPORTED and f"update_method={method}" in str(e.value)
        finally:
            pi.close()
    track = _env("humanoidtrack")
    demo = Sweep(track, Args(env_name="humanoidtrack", Nsample=64, Hsample=50, Ndiffuse=3, enable_demo=True, disable_recommended_params=True,
                             not_render=True), 2)
    try:
        with pytest.raises(gpu.MbdError) as e:
            demo.set_togo(**sc.TOGO)
        assert e.value.code == gpu.MBD_ERR_UNSUPPORTED and "enable_demo" in str(e.value)
    finally:
        demo.close()
