"""The pick record on the GPU (include/mbd_hip.h mbd_mpc_pick; DESIGN.md section 1 "N15 pick").  Every comparison is by bit
pattern or np.array_equal.

  argmax alone    mbd_debug_pick_best at N in {1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 8193}, P in {1, 3}: where the maximum
                  lies, ties, signs, subnormals, non-finite entries, nothing finite
  episodes        actions, rewards, states, means and the log against tests/mpc_pick_checker.py: hopper, humanoidrun and car2d
                  under mask 7, masks 1, 3, 5, 6 on hopper, E = 2, a plant of mass 1.3, an objective record with a rate cost, the
                  all-three-choices episode
  mask MEAN       the episode of the same handle with the record cleared, by bytes — alone and under an objective record with a
                  rate cost, a delay record, and mppi / cma-es / cem with a sigma record
  sweeps          P in {3, 8} lockstep episodes equal their plans run alone, logs included; a path-integral sweep
  sessions        a session fed the episode's states returns its picks and logs; reset_mean; a sweep's session with P = 3
  refusals        set, clear, set again; demo, ensemble and open-session refusals with their codes
  Python layer    mpc.run_mpc, run_mpc_batch, run_mpc_online and the command line under --pick: the fields, the three paths' bits
  other records   against the checker by bytes: mppi, cma-es and cem under a sigma record, a delay record with D = 1, a weighting
                  record with rejection on the hopper whose candidates really diverge (best is never a dropped one), a sweep with
                  an objective record, a sweep's session in which one episode is reset"""
import ctypes as C

import numpy as np
import pytest

import mpc_pick_checker as pc
from test_gpu_noise_shape import _args, _env, _oenv, _state
from test_mpc_pick import ALL3

pytestmark = pytest.mark.gpu

N, H, ND, K, T = 64, 20, 6, 2, 5
_OUT = ("actions", "rewards", "states", "means")
SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 8193)


@pytest.fixture(scope="module")
def gpu(lib):
    from mbd_hip import _capi
    if _capi.device_count() < 1:
        pytest.fail("tests/test_gpu_mpc_pick.py needs a GPU")
    return _capi


def _same(a, b, what):
    x, y = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert x.dtype == y.dtype and x.size == y.size and x.tobytes() == y.tobytes(), what


def _equal(ep, ref, what, log=True):
    for k in _OUT:
        x, y = np.asarray(ep[k], np.float32), np.asarray(ref[k], np.float32)
        assert x.size == y.size and np.array_equal(x.reshape(y.shape), y), f"{what}: {k} differ"
    if log:
        lg = ep["pick"]
        assert np.array_equal(lg["choice"], ref["choice"]), f"{what}: choice {lg['choice']} != {ref['choice']}"
        assert np.array_equal(lg["best"], ref["best"]), f"{what}: best"
        _same(lg["rets"], ref["rets"], f"{what}: rets")


def _plan(env, name, n, st, h=H, nd=ND, temp=0.1, **kw):
    from mbd_hip.planners.mbd_planner import Plan
    a = _args(name, n, h, nd)
    a.temp_sample = temp
    plan = Plan(env, a, **kw)
    plan.set_state0(st)
    return plan


def _mask_kw(mask):
    return dict(mean=bool(mask & 1), prev=bool(mask & 2), best=bool(mask & 4))


# ---- the argmax alone ---------------------------------------------------------------------------------------------------------

def _argmax_cases(n):
    """(name, rews [n]) — every case the size admits."""
    rng = np.random.default_rng(n)
    base = rng.normal(size=n).astype(np.float32)
    nan, inf = np.float32("nan"), np.float32("inf")
    out = []

    def peak(at):
        r = base.copy()
        r[at] = 50.0
        return r

    for name, at in (("first", 0), ("last", n - 1), ("lane 63", 63), ("lane 64", 64), ("entry 1024", 1024)):
        if at < n:
            out.append((name, peak(at)))
    out.append(("all equal", np.full(n, -1.25, np.float32)))
    out.append(("all negative", -np.abs(base) - 1.0))
    if n > 70:
        r = peak(70)
        r[5] = 50.0
        out.append(("equal maxima in two waves", r))
    if n > 1024 + 7:
        r = peak(1024 + 7)
        r[7] = 50.0
        out.append(("equal maxima in one thread's stride", r))
        r = peak(7)
        r[1024 + 7] = np.nextafter(np.float32(50.0), np.float32(60.0))
        out.append(("the larger in the thread's second entry", r))
    if n >= 2:
        r = np.full(n, -1.0, np.float32)
        r[n - 1], r[n // 2] = 0.0, -0.0
        out.append(("+0 against -0", r))
        r = np.full(n, -1.0, np.float32)
        r[n - 1], r[n // 2] = -0.0, 0.0
        out.append(("-0 against +0", r))
    r = (base * np.float32(1e-41)).astype(np.float32)
    out.append(("subnormals", r))
    r = peak(n // 2)
    r[0] = nan
    for at, v in ((n // 2 - 1, inf), (n // 2 + 1, -inf), (n - 1, nan), (n // 3, inf)):
        if 0 <= at < n and at != n // 2:
            r[at] = v
    if n == 1:
        r[0] = 50.0
    out.append(("non-finite scattered", r))
    r = np.full(n, nan, np.float32)
    r[::2] = inf
    r[::3] = -inf
    out.append(("nothing finite", r))
    if n >= 3:
        r = np.full(n, inf, np.float32)
        r[n - 2] = -7.0
        out.append(("one finite among +inf", r))
    return out


@pytest.mark.parametrize("n", SIZES)
def test_argmax_alone(gpu, n):
    cases = _argmax_cases(n)
    for P in (1, 3):
        for j, (name, r) in enumerate(cases):
            rows = np.stack([cases[(j + k) % len(cases)][1] for k in range(P)])
            got = gpu.debug_pick_best(rows)
            want = np.array([pc.best_index(x) for x in rows], np.int32)
            assert np.array_equal(got, want), f"N={n} P={P} {name}: {got} != {want}"
    assert pc.best_index(cases[-1][1] if n < 3 else cases[-2][1]) == -1


# ---- episodes against the checker -----------------------------------------------------------------------------------------------

_EPISODES = [("hopper", N, 7, 1), ("humanoidrun", N, 7, 1), ("car2d", N, 7, 1), ("hopper", N, 1, 1), ("hopper", N, 3, 1),
             ("hopper", N, 5, 1), ("hopper", N, 6, 1), ("hopper", N, 7, 2)]


@pytest.mark.parametrize("name,n,mask,E", _EPISODES)
def test_episode_matches_the_checker(gpu, orc, name, n, mask, E):
    from mbd_hip.envs.base import prng_impl
    env = _env(name)
    st, key = env.reset(gpu.prng_key(5)), gpu.prng_key(6)
    plan = _plan(env, name, n, st)
    plan.set_mpc_pick(**_mask_kw(mask))
    ep = plan.run_mpc(key, T, K, E)
    ref = pc.episode(_oenv(orc, env), _state(env, st), key, n, H, ND, 0.1, T, K, E, mask, impl=prng_impl())
    _equal(ep, ref, f"{name} mask={mask} E={E}")
    for t in range(T):  # (the best candidate's return is the reward the last step's score read, bit for bit)
        r = ref["last_rews"][t]
        if ref["best"][t] >= 0:
            _same(ep["pick"]["rets"][t, 2], r[np.isfinite(r)].max(), f"tick {t}: ret[2]")
    plan.close()


def test_all_three_choices_episode(gpu, orc):
    """The small episode of tests/test_mpc_pick.py in which the mean, the incumbent and the best candidate are each picked."""
    from mbd_hip.envs.base import prng_impl
    if prng_impl() != 1:
        pytest.fail("the episode's inputs are stated for prng impl 1")
    env = _env("hopper")
    keys = gpu.prng_split(gpu.prng_key(0), 2, 1)
    st = env.reset(keys[1])
    c = ALL3
    plan = _plan(env, "hopper", c["N"], st, c["H"], c["Nd"], temp=c["temp"])
    plan.set_mpc_pick()
    ep = plan.run_mpc(keys[0], c["T"], c["K"], c["E"])
    ref = pc.episode(_oenv(orc, env), _state(env, st), keys[0], mask=7, impl=1, **c)
    assert set(ref["choice"].tolist()) == {0, 1, 2}
    _equal(ep, ref, "all three choices")
    plan.close()


def test_plant_of_mass_1_3(gpu, orc):
    """The pick evaluates on the planner's model; the rows run on the plant."""
    from mbd_hip.envs.base import RigidBodyEnv, prng_impl
    env = _env("hopper")
    plant = RigidBodyEnv("hopper", model=env.sys.scaled(mass=1.3))
    st, key = env.reset(gpu.prng_key(5)), gpu.prng_key(6)
    plan = _plan(env, "hopper", N, st)
    plan.set_mpc_plant(env=plant, key=gpu.prng_key(11), act_std=0.0, kick_std=0.0)
    plan.set_mpc_pick()
    ep = plan.run_mpc(key, T, K, 1)
    ref = pc.episode(_oenv(orc, env), _state(env, st), key, N, H, ND, 0.1, T, K, 1, 7, impl=prng_impl(), plant=_oenv(orc, plant))
    _equal(ep, ref, "plant")
    nominal = pc.episode(_oenv(orc, env), _state(env, st), key, N, H, ND, 0.1, T, K, 1, 7, impl=prng_impl())
    assert not np.array_equal(nominal["states"], ref["states"])
    plan.close()


def test_objective_record_with_a_rate_cost(gpu, orc):
    """The steps and the pick see the shaped returns, the pick's with the tick's previous action; the next tick's previous action is
    the PICKED plan's row E-1."""
    import objective_checker as oc
    from mbd_hip.envs.base import prng_impl
    env = _env("hopper")
    st, key = env.reset(gpu.prng_key(5)), gpu.prng_key(6)
    prev0 = np.linspace(-0.5, 0.5, env.action_size).astype(np.float32)
    plan = _plan(env, "hopper", N, st)
    plan.set_objective(effort=0.05, rate=0.5, prev0=prev0)
    plan.set_mpc_pick()
    ep = plan.run_mpc(key, T, K, 1)
    rec = oc.Record(effort=0.05, rate=0.5, prev0=prev0)
    ref = pc.episode(_oenv(orc, env), _state(env, st), key, N, H, ND, 0.1, T, K, 1, 7, impl=prng_impl(), objective=rec)
    _equal(ep, ref, "objective")
    assert (ref["choice"] != 0).any()  # (a tick whose pick is not the mean: prev followed it, or the later ticks would differ)
    plan.close()


@pytest.mark.parametrize("method", ["mppi", "cma-es", "cem"])
def test_path_integral_episode_matches_the_checker(gpu, orc, method):
    """A path-integral plan under a sigma record: slot 2 is a row of the last refinement's materialised candidates, ret[2] the
    largest reward of that refinement by bytes, and the next tick samples around the PICKED plan."""
    from mbd_hip.envs.base import prng_impl
    env = _env("hopper")
    st, key = env.reset(gpu.prng_key(5)), gpu.prng_key(6)
    sig = (1.0, 0.5, 0.0)
    plan = _plan(env, "hopper", N, st, update_method=_METHOD[method])
    plan.set_mpc_sigma(*sig)
    plan.set_mpc_pick()
    ep = plan.run_mpc(key, T, K, 1)
    ref = pc.episode(_oenv(orc, env), _state(env, st), key, N, H, ND, 0.1, T, K, 1, 7, impl=prng_impl(), method=method, sigma=sig)
    _equal(ep, ref, method)
    for t in range(T):
        _same(ep["pick"]["rets"][t, 2], ref["last_rews"][t].max(), f"{method} tick {t}: ret[2]")
    assert (ref["choice"] != 0).any()
    plan.close()


@pytest.mark.parametrize("given", [False, True], ids=["rows0 NULL", "rows0 given"])
def test_delay_record(gpu, orc, given):
    """D = 1: the tick plans, and the pick evaluates, from the predicted state; the picked plan's first rows join the queue."""
    from mbd_hip.envs.base import prng_impl
    env = _env("hopper")
    st, key = env.reset(gpu.prng_key(5)), gpu.prng_key(6)
    rows0 = np.random.default_rng(3).uniform(-1, 1, (1, env.action_size)).astype(np.float32) if given else None
    plan = _plan(env, "hopper", N, st)
    plan.set_mpc_delay(1, rows0)
    plan.set_mpc_pick()
    ep = plan.run_mpc(key, T, K, 1)
    ref = pc.episode(_oenv(orc, env), _state(env, st), key, N, H, ND, 0.1, T, K, 1, 7, impl=prng_impl(), D=1, rows0=rows0)
    _equal(ep, ref, "delay")
    _same(np.asarray(ep["predicted"], np.float32), ref["predicted"], "predicted states")
    assert np.array_equal(ep["actions"][1:], ep["means"][:-1, 0]) and (ref["choice"] != 0).any()
    for t in range(T):
        r = ref["last_rews"][t]
        _same(ep["pick"]["rets"][t, 2], r[np.isfinite(r)].max(), f"tick {t}: ret[2] from the predicted state")
    plan.close()


def test_weighting_with_real_divergence(gpu, orc):
    """Rejection on the hopper whose actuator 0 has a gear of 1e30 (tests/weighting_combined_inputs.py): candidates of every tick's
    last step really diverge, ``best`` is never one of them and ``rets[t, 2]`` is the largest finite reward."""
    import weighting_combined_inputs as wci
    import weighting_inputs as wi
    from mbd_hip.envs.base import prng_impl
    from test_gpu_weighting_combined import _plan as _wplan
    from test_mpc_pick import divergence_episode
    c = wci.LOOP
    ref = divergence_episode(orc, 7, prng_impl())
    plan, _ = _wplan(gpu, orc, 1, c["N"], c["Nd"], 0, c["state_seed"])
    try:
        plan.set_noise_shape(wci.shape(plan.Nu))
        plan.set_weighting(**wi.REJECT.kwargs())
        plan.set_mpc_pick()
        ep = plan.run_mpc(gpu.prng_key(c["key_seed"]), wci.T, wci.K, wci.E)
        _equal(ep, ref, "divergence")
        lg = ep["pick"]
        for t in range(wci.T):
            r = ref["last_rews"][t]
            fin = np.isfinite(r)
            assert 0 < fin.sum() < c["N"], f"tick {t}: {int(fin.sum())} finite rewards"
            assert fin[lg["best"][t]], f"tick {t}: best = {lg['best'][t]} is a dropped candidate"
            _same(lg["rets"][t, 2], r[fin].max(), f"tick {t}: ret[2]")
        assert np.isfinite(ep["means"]).all() and np.isfinite(lg["rets"]).all()
    finally:
        plan.close()


# ---- mask MEAN ----------------------------------------------------------------------------------------------------------------

def _records(plan, kind):
    if kind == "objective":
        plan.set_objective(effort=0.05, rate=0.5)
    elif kind == "delay":
        plan.set_mpc_delay(1)
    elif kind == "weighting":
        plan.set_weighting(reject_nonfinite=True)
    elif kind in ("mppi", "cma-es", "cem"):
        plan.set_mpc_sigma(cold=1.0, warm=0.5)


_METHOD = {"mppi": 1, "cma-es": 2, "cem": 3}


@pytest.mark.parametrize("kind", ["plain", "objective", "delay", "weighting", "mppi", "cma-es", "cem"])
def test_mask_mean_is_the_episode_without_the_record(gpu, orc, kind):
    from mbd_hip.envs.base import prng_impl
    env = _env("hopper")
    st, key = env.reset(gpu.prng_key(5)), gpu.prng_key(6)
    plan = _plan(env, "hopper", N, st, update_method=_METHOD.get(kind, 0))
    _records(plan, kind)
    plan.set_mpc_pick(mean=True, prev=False, best=False)
    with_rec = plan.run_mpc(key, T, K, 1)
    plan.clear_mpc_pick()
    without = plan.run_mpc(key, T, K, 1)
    assert "pick" not in without
    for k in _OUT:
        _same(with_rec[k], without[k], f"{kind}: {k}")
    lg = with_rec["pick"]
    assert (lg["choice"] == 0).all() and lg["rets"].shape == (T, 3) and np.isfinite(lg["rets"]).all()
    _same(lg["rets"][0, 1], lg["rets"][0, 0], "tick 0 has no incumbent: its slot holds the mean")
    if kind == "plain":
        ref = pc.episode(_oenv(orc, env), _state(env, st), key, N, H, ND, 0.1, T, K, 1, 1, impl=prng_impl())
        _same(lg["rets"][:, 0], ref["rets"][:, 0], "the executed plans' values")
    # under every record the full pick's episode runs, logs a best candidate, and never hands on a plan the model values less
    plan.set_mpc_pick()
    full = plan.run_mpc(key, T, K, 1)["pick"]
    assert (full["best"] >= 0).all() and (full["best"] < N).all()
    assert all(full["rets"][t, full["choice"][t]] >= full["rets"][t, 0] for t in range(T))
    plan.close()


# ---- sweeps ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P,method", [(3, 0), (8, 0), (3, 1)])
def test_sweep_episodes_equal_their_plans_alone(gpu, P, method):
    from mbd_hip.planners.mbd_planner import Sweep
    env = _env("hopper")
    states = [env.reset(gpu.prng_key(20 + k)) for k in range(P)]
    keys = np.stack([gpu.prng_key(40 + k) for k in range(P)])
    temps = [0.1 * (1 + k % 3) for k in range(P)]
    a = _args("hopper", N, H, ND)
    sweep = Sweep(env, a, P, temps=temps, update_method=method)
    for k in range(P):
        sweep.set_state0(k, states[k])
    if method:
        sweep.set_mpc_sigma(cold=1.0, warm=0.5)
    sweep.set_mpc_pick()
    out = sweep.run_mpc(keys, T, K, 1)
    seen = set()
    for k in range(P):
        plan = _plan(env, "hopper", N, states[k], temp=temps[k], update_method=method)
        if method:
            plan.set_mpc_sigma(cold=1.0, warm=0.5)
        plan.set_mpc_pick()
        ep = plan.run_mpc(keys[k], T, K, 1)
        for name in _OUT:
            _same(out[name][k], ep[name], f"episode {k}: {name}")
        for name in ("choice", "rets", "best"):
            _same(out["pick"][k][name], ep["pick"][name], f"episode {k}: {name}")
        seen |= set(ep["pick"]["choice"].tolist())
        plan.close()
    assert len(seen) >= 2
    sweep.close()


# ---- sessions -------------------------------------------------------------------------------------------------------------------

def test_session_returns_the_episode(gpu, orc):
    from mbd_hip.envs.base import prng_impl
    env = _env("hopper")
    st, key = env.reset(gpu.prng_key(5)), gpu.prng_key(6)
    plan = _plan(env, "hopper", N, st)
    plan.set_mpc_pick()
    ep = plan.run_mpc(key, T, K, 1)
    with plan.mpc_open(key, K, 1) as s:
        assert s.pick is None
        for t in range(T):
            o = s.tick(ep["states"][t])
            _same(o["mean"], ep["means"][t], f"tick {t}: mean")
            _same(o["rows"], ep["actions"][t:t + 1], f"tick {t}: rows")
            assert s.pick["choice"] == ep["pick"]["choice"][t] and s.pick["best"] == ep["pick"]["best"][t]
            _same(s.pick["rets"], ep["pick"]["rets"][t], f"tick {t}: rets")
        lg = plan.peek_mpc_pick()
        for name in ("choice", "rets", "best"):
            _same(lg[name], ep["pick"][name], name)
        _same(plan.peek_mpc_pick(2)["choice"], ep["pick"]["choice"][-2:], "the most recent two ticks")
    # reset_mean: the tick is cold, slot 1 absent for that one tick — the checker's episode with a reset in front of tick 2
    ref = pc.episode(_oenv(orc, env), _state(env, st), key, N, H, ND, 0.1, T, K, 1, 7, impl=prng_impl(), reset_at=(2,))
    with plan.mpc_open(key, K, 1) as s:
        for t in range(T):
            if t == 2:
                s.reset_mean()
            o = s.tick(ref["states"][t])
            _same(o["mean"], ref["means"][t], f"reset: tick {t}: mean")
        lg = plan.peek_mpc_pick()
        assert np.array_equal(lg["choice"], ref["choice"]) and np.array_equal(lg["best"], ref["best"])
        _same(lg["rets"], ref["rets"], "reset: rets")
        _same(lg["rets"][2, 1], lg["rets"][2, 0], "the reset tick has no incumbent")
        assert lg["choice"][2] != 1
    plan.close()


def test_sweep_session(gpu):
    from mbd_hip.planners.mbd_planner import Sweep
    P = 3
    env = _env("hopper")
    states = [env.reset(gpu.prng_key(20 + k)) for k in range(P)]
    keys = np.stack([gpu.prng_key(40 + k) for k in range(P)])
    sweep = Sweep(env, _args("hopper", N, H, ND), P)
    for k in range(P):
        sweep.set_state0(k, states[k])
    sweep.set_mpc_pick()
    out = sweep.run_mpc(keys, T, K, 1)
    with sweep.mpc_open(keys, K, 1) as s:
        for t in range(T):
            o = s.tick(np.ascontiguousarray(out["states"][:, t]))
            _same(o["mean"], out["means"][:, t], f"tick {t}: means")
            _same(s.pick["choice"], np.array([out["pick"][k]["choice"][t] for k in range(P)], np.int32), f"tick {t}: choice")
            _same(s.pick["rets"], np.stack([out["pick"][k]["rets"][t] for k in range(P)]), f"tick {t}: rets")
    sweep.close()


def test_sweep_session_with_one_episode_reset(gpu, orc):
    """reset_mean(1) in front of tick 2: episode 1's tick is cold — no incumbent, Ndiffuse-1 steps — while episodes 0 and 2 idle
    through the steps above K inside the same launches; every episode equals the checker's, the reset one with its reset."""
    from mbd_hip.envs.base import prng_impl
    from mbd_hip.planners.mbd_planner import Sweep
    P = 3
    env = _env("hopper")
    states = [env.reset(gpu.prng_key(20 + k)) for k in range(P)]
    keys = np.stack([gpu.prng_key(40 + k) for k in range(P)])
    refs = [pc.episode(_oenv(orc, env), _state(env, states[k]), keys[k], N, H, ND, 0.1, T, K, 1, 7, impl=prng_impl(),
                       reset_at=(2,) if k == 1 else ()) for k in range(P)]
    sweep = Sweep(env, _args("hopper", N, H, ND), P)
    sweep.set_mpc_pick()
    with sweep.mpc_open(keys, K, 1) as s:
        for t in range(T):
            if t == 2:
                s.reset_mean(1)
            o = s.tick(np.stack([refs[k]["states"][t] for k in range(P)]))
            for k in range(P):
                _same(o["mean"][k], refs[k]["means"][t], f"tick {t} episode {k}: mean")
                assert s.pick["choice"][k] == refs[k]["choice"][t] and s.pick["best"][k] == refs[k]["best"][t], (t, k)
                _same(s.pick["rets"][k], refs[k]["rets"][t], f"tick {t} episode {k}: rets")
        assert s.pick["choice"][1] is not None and refs[1]["choice"][2] != 1
        _same(sweep.peek_mpc_pick(1)["rets"][2, 1], refs[1]["rets"][2, 0], "the reset tick has no incumbent")
    sweep.close()


def test_sweep_with_an_objective_record(gpu, orc):
    """An objective record, a sweep and a pick together: the objective launch over the 3 P slots, every episode's previous action
    following its own pick — each episode against the checker and against its plan alone."""
    import objective_checker as oc
    from mbd_hip.envs.base import prng_impl
    from mbd_hip.planners.mbd_planner import Sweep
    P = 3
    env = _env("hopper")
    states = [env.reset(gpu.prng_key(20 + k)) for k in range(P)]
    keys = np.stack([gpu.prng_key(40 + k) for k in range(P)])
    prev0 = np.linspace(-0.5, 0.5, env.action_size).astype(np.float32)
    rec = oc.Record(effort=0.05, rate=0.5, prev0=prev0)
    sweep = Sweep(env, _args("hopper", N, H, ND), P)
    for k in range(P):
        sweep.set_state0(k, states[k])
    sweep.set_objective(effort=0.05, rate=0.5, prev0=prev0)
    sweep.set_mpc_pick()
    out = sweep.run_mpc(keys, T, K, 1)
    for k in range(P):
        ref = pc.episode(_oenv(orc, env), _state(env, states[k]), keys[k], N, H, ND, 0.1, T, K, 1, 7, impl=prng_impl(), objective=rec)
        _equal({n: out[n][k] for n in _OUT} | {"pick": out["pick"][k]}, ref, f"episode {k}")
    sweep.close()


# ---- refusals and clearing -----------------------------------------------------------------------------------------------------

def test_refusals_and_clearing(gpu):
    from mbd_hip.envs.base import RigidBodyEnv
    env = _env("hopper")
    st, key = env.reset(gpu.prng_key(5)), gpu.prng_key(6)
    plan = _plan(env, "hopper", N, st)
    with pytest.raises(gpu.MbdError) as e:
        plan.peek_mpc_pick()
    assert e.value.code == gpu.MBD_ERR_STATE
    plan.set_mpc_pick()
    a = plan.run_mpc(key, 3, K, 1)
    plan.clear_mpc_pick()
    plan.set_mpc_pick()
    b = plan.run_mpc(key, 3, K, 1)
    for k in _OUT:
        _same(a[k], b[k], k)
    with pytest.raises(gpu.MbdError) as e:
        plan.set_mpc_pick(mean=False, prev=False, best=False)
    assert e.value.code == gpu.MBD_ERR_INVALID and "candidates" in str(e.value)
    # an ensemble on a plan with a pick record, and a pick record on a plan with an ensemble
    member = RigidBodyEnv("hopper", model=env.sys.scaled(mass=1.1))
    with pytest.raises(gpu.MbdError) as e:
        plan.set_ensemble([None, member], "mean")
    assert e.value.code == gpu.MBD_ERR_UNSUPPORTED and "pick" in str(e.value)
    plan.clear_mpc_pick()
    plan.set_ensemble([None, member], "mean")
    with pytest.raises(gpu.MbdError) as e:
        plan.set_mpc_pick()
    assert e.value.code == gpu.MBD_ERR_UNSUPPORTED and "ensemble" in str(e.value)
    plan.clear_ensemble()
    plan.set_mpc_pick()
    with plan.mpc_open(key, K, 1):
        with pytest.raises(gpu.MbdError) as e:
            plan.set_mpc_pick()
        assert e.value.code == gpu.MBD_ERR_STATE and "session" in str(e.value)
    plan.close()
    # a demo plan
    tenv = _env("humanoidtrack")
    from mbd_hip.planners.mbd_planner import Plan
    da = _args("humanoidtrack", N, 50, ND, enable_demo=True)
    dplan = Plan(tenv, da)
    with pytest.raises(gpu.MbdError) as e:
        dplan.set_mpc_pick()
    assert e.value.code == gpu.MBD_ERR_UNSUPPORTED and "enable_demo" in str(e.value)
    dplan.close()


# ---- the Python layer -----------------------------------------------------------------------------------------------------------

def test_python_layer_and_command_line_paths(gpu):
    """``--pick`` through mpc.run_mpc, the batch and ``--online``: every field of the log arrives, the three paths agree bit for
    bit, and the report carries the shares."""
    from dataclasses import replace
    from mbd_hip.planners import mpc
    a = replace(_args("hopper", N, H, ND), n_ticks=T, warm_steps=K, pick="mean,prev,best")
    assert mpc._pick_of(a) == dict(mean=True, prev=True, best=True)
    assert mpc._pick_of(replace(a, pick="best, mean")) == dict(mean=True, prev=False, best=True)
    for bad in ("none", "mean,worst", ","):
        with pytest.raises(ValueError, match="pick"):
            mpc._pick_of(replace(a, pick=bad))
    _, one = mpc.run_mpc(a, return_details=True)
    lg = one["pick"]
    assert lg["choice"].shape == (T,) and lg["rets"].shape == (T, 3) and lg["best"].shape == (T,)
    assert lg["choice"].dtype == np.int32 and lg["rets"].dtype == np.float32 and one["pick"] is lg
    _, plain = mpc.run_mpc(replace(a, pick=""), return_details=True)
    assert "pick" not in plain
    _, mean_only = mpc.run_mpc(replace(a, pick="mean"), return_details=True)
    for k in _OUT:
        _same(mean_only[k], plain[k], f"--pick mean: {k}")
    _, batch = mpc.run_mpc_batch([replace(a, seed=s) for s in (0, 1, 2)], return_details=True)
    _, online = mpc.run_mpc_online(a, return_details=True)
    for name in ("choice", "rets", "best"):
        _same(batch[0]["pick"][name], lg[name], f"batch: {name}")
        _same(online["pick"][name], lg[name], f"online: {name}")
    _same(batch[0]["means"], one["means"], "batch: means")
    _same(online["means"], one["means"], "online: means")
    rep = mpc._pick_log([d["pick"] for d in batch])
    assert abs(sum(rep["share"].values()) - 1.0) < 1e-6 and set(rep["share"]) == {"mean", "prev", "best"}
    res = mpc._main(["--env_name", "hopper", "--disable_recommended_params", "--not_render", "--Nsample", str(N), "--Hsample", str(H),
                     "--Ndiffuse", str(ND), "--n_ticks", str(T), "--warm_steps", str(K), "--pick", "prev,best"])
    assert res["pick"] == "prev,best" and res["pick_log"]["share"]["mean"] <= 1.0


def test_c_example_with_pick(gpu, tmp_path):
    """examples/mbd_control.c --pick from plain C: every tick's line carries a choice in {0, 1, 2} and the finite value of the plan
    handed on; without the flag the lines are what they always were; --mppi and --pick are accepted in either order."""
    import os
    import subprocess
    from conftest import ROOT
    libdir = os.path.join(ROOT, "model-based-diffusion_amd", "lib")
    exe = str(tmp_path / "mbd_control")
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "mbd_control.c"),
                    "-o", exe, "-L", libdir, "-lmbd_hip", f"-Wl,-rpath,{libdir}", "-lm"], check=True)

    def ticks(*extra):
        out = subprocess.run([exe, "hopper", "64", str(H), str(ND), str(K), str(T), "0", *extra], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        return [ln.split() for ln in out.stdout.strip().splitlines() if ln.startswith("tick ")]

    plain, picked = ticks(), ticks("--pick")
    assert len(plain) == len(picked) == T and all(len(t) == 8 for t in plain)
    for t in picked:
        assert len(t) == 12 and t[8] == "choice" and int(t[9]) in (0, 1, 2) and t[10] == "value" and np.isfinite(float(t[11]))
    assert int(picked[0][9]) != 1  # (tick 0 has no incumbent)
    a, b = ticks("--mppi", "--pick"), ticks("--pick", "--mppi")
    assert [t[:4] + t[8:] for t in a] == [t[:4] + t[8:] for t in b] and len(a[0]) == 12
