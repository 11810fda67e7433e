"""Episodes that follow a demonstration on the episode's clock, on the GPU (include/mbd_hip.h mbd_mpc_demo; DESIGN.md section 1
"N10 demo clock").  Every comparison is np.array_equal except ``track_err`` (float64 numpy on the checker's tracked positions,
rtol 1e-6: three products, two sums and one square root in f32 stay under 4 ulp = 4.8e-7 relative; exact where it is 0).
The sizes: N = 64, Nd = 6, K = 2, H = 50; the checker's episodes are tests/mpc_demo_checker.py's cases, the ones
tests/test_mpc_demo.py proves able to tell a moving window from a frozen one.

  episodes        means, actions, rewards, states and demo_windows against the checker: humanoidtrack (the instantiation that
                  accumulates the log-density itself), the same under MBD_NO_FUSED_LOGPD (logpd_track_kernel through the window
                  pointer) and car2d — each in both shapes: T = 3, E = 3, c0 = 2 (windows from rows 2, 5, 8, the last one clamped
                  at row 56) and T = 2, E = 1, c0 = 60 (every window held on the last row)
  definition      tick 0 under the env's own demo is Plan.run of the demo plan; T ticks are a prefix of T + 1, logs included
  untouched       episodes of plans without enable_demo (humanoidrun, humanoidtrack) still equal tests/mpc_checker.py
  records         a delay record (D = 1, E = 2, T = 3: the windows start at (t + 1) E); a plant record (mismatched body, action
                  noise, kicks: track_err is taken from the plant's positions)
  sweeps          P = 2 episodes with different seeds and one record equal the single plans', peeks included
  refusals        every refusal of the record by code and field; a demo plan without a record; the peek before an episode; a
                  plant with other tracked links or none, on a plan and on either episode of a sweep; demos with a path-integral
                  update refused at creation
  open loop       Plan.run and Sweep.run ignore a record that differs from the env's demo
  command line    --demo_clip env --demo_period equals the API call
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mpc_checker
import mpc_demo_checker as mdc
from conftest import ROOT
from test_gpu_noise_shape import _env, _oenv

pytestmark = pytest.mark.gpu

_LOGS = ("means", "actions", "rewards", "states", "demo_windows")


@pytest.fixture(scope="module")
def gpu(lib):
    from mbd_hip import _capi
    if _capi.device_count() < 1:
        pytest.fail("tests/test_gpu_mpc_demo.py needs a GPU")
    return _capi


def _args(name, demo=True, **kw):
    from mbd_hip.planners.mpc import MpcArgs
    return MpcArgs(env_name=name, Nsample=mdc.N, Hsample=mdc.ROWS, Ndiffuse=mdc.ND, temp_sample=mdc.TEMP, enable_demo=demo,
                   disable_recommended_params=True, not_render=True, **kw)


def _state(s):
    from mbd_hip.envs.base import State
    return State(np.ascontiguousarray(s, np.float32), None, np.float32(0), np.float32(0), {})


def _plan(env, name, s, demo=True):
    from mbd_hip.planners.mbd_planner import Plan
    plan = Plan(env, _args(name, demo))
    plan.set_state0(_state(s))
    return plan


def _equal(got, ref, what, logs=_LOGS):
    for k in logs:
        x, y = np.asarray(got[k], np.float32), np.asarray(ref[k], np.float32)
        assert x.size == y.size and np.array_equal(x.reshape(y.shape), y), f"{what}: {k} differ"


def _track_err_close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    zero = ref == 0
    assert np.array_equal(got[zero], ref[zero]), what
    worst = np.abs(got[~zero] - ref[~zero]) / ref[~zero]
    print(f"{what}: track_err worst relative error {worst.max() if worst.size else 0.0:.3g} over {worst.size} values")
    assert (worst <= 1e-6).all(), f"{what}: track_err off by {worst.max():.3g} relative"


def _run_case(orc, env, name, variant, plan=None):
    """(the library's episode, the checker's, the case's settings) of a case of tests/mpc_demo_checker.py"""
    ref, info = mdc.case(orc, name, variant)
    own = plan is None
    if own:
        plan = _plan(env, name, info["state0"])
    plan.set_mpc_demo(info["clip"], info["c0"], info["rew_xref"])
    ep = plan.run_mpc(info["key"], info["T"], mdc.WARM, info["E"])
    if own:
        plan.close()
    return ep, ref, info


# ---- episodes against the checker -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["moving", "held"])
@pytest.mark.parametrize("name,unfused", [("humanoidtrack", False), ("humanoidtrack", True), ("car2d", False)],
                         ids=["humanoidtrack", "humanoidtrack-unfused", "car2d"])
def test_episode_matches_the_checker(gpu, orc_omp, levers, name, unfused, shape):
    env = _env(name)
    if name == "humanoidtrack":
        levers(MBD_NO_FUSED_LOGPD=int(unfused))
        choice = gpu.debug_rollout_choice(env.sys.to_struct(), 256, mdc.N, mdc.ROWS, has_xref=True)
        assert bool(choice["fuses_logpd"]) == (not unfused), choice
    ep, ref, info = _run_case(orc_omp, env, name, shape)
    what = f"{name} {shape}{' unfused' if unfused else ''}"
    _equal(ep, ref, what)
    _track_err_close(ep["track_err"], ref["track_err"], what)
    T, E, c0 = mdc.SHAPES[shape]
    clip = mdc.as_tracks(info["clip"])
    assert ep["demo_windows"].shape == (T, clip.shape[0], mdc.ROWS, clip.shape[2]) and ep["track_err"].shape == (T * E, clip.shape[0])
    if shape == "moving":  # rows 2, 5, 8; the last window reaches row 57 and is clamped at 56
        for t in range(T):
            assert np.array_equal(ep["demo_windows"][t][:, 0], clip[:, c0 + t * E])
        assert np.array_equal(ep["demo_windows"][2][:, 48:], clip[:, [56, 56]])
    else:
        assert np.array_equal(ep["demo_windows"], np.broadcast_to(clip[None, :, -1:], ep["demo_windows"].shape))


# ---- the definition and the properties --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["humanoidtrack", "car2d"])
def test_tick0_under_the_envs_own_demo_is_the_open_loop_demo_plan(gpu, orc_omp, name):
    env = _env(name)
    _, info = mdc.case(orc_omp, name, "moving")
    plan = _plan(env, name, info["state0"])
    plan.set_mpc_demo(env.xref, 0)  # (rew_xref: the env's)
    ep = plan.run_mpc(info["key"], 1, mdc.WARM, 3)
    from mbd_hip.envs.base import prng_impl
    mu, _, _, _ = plan.run(gpu.prng_split(info["key"], 2, prng_impl())[1])
    plan.close()
    assert np.array_equal(ep["means"][0], mu[-1])
    assert np.array_equal(ep["demo_windows"][0], mdc.as_tracks(env.xref))


def test_an_episode_is_a_prefix_of_a_longer_one(gpu, orc_omp):
    name = "humanoidtrack"
    _, info = mdc.case(orc_omp, name, "moving")
    plan = _plan(_env(name), name, info["state0"])
    plan.set_mpc_demo(info["clip"], info["c0"], info["rew_xref"])
    short = plan.run_mpc(info["key"], 2, mdc.WARM, 3)
    long = plan.run_mpc(info["key"], 3, mdc.WARM, 3)
    plan.close()
    for k in _LOGS + ("track_err",):
        assert np.array_equal(short[k], long[k][: len(short[k])]), k
    assert not np.array_equal(long["means"][2], long["means"][1])


@pytest.mark.parametrize("name", ["humanoidrun", "humanoidtrack"])
def test_plans_without_demos_are_untouched(gpu, orc_omp, name):
    """A plan without enable_demo carries no record: its episode is still tests/mpc_checker.py's, bit for bit, and its result
    has no demo logs."""
    from mbd_hip.envs.base import prng_impl
    env = _env(name)
    st, key = env.reset(gpu.prng_key(mdc.SEED_RESET)), gpu.prng_key(mdc.SEED_KEY)
    s = np.asarray(st.pipeline_state, np.float32).reshape(-1)
    plan = _plan(env, name, s, demo=False)
    ep = plan.run_mpc(key, 3, mdc.WARM, 3)
    plan.close()
    ref = mpc_checker.episode(_oenv(orc_omp, env), s, key, mdc.N, mdc.ROWS, mdc.ND, mdc.TEMP, 3, mdc.WARM, 3, impl=prng_impl())
    _equal(ep, ref, name, logs=("means", "actions", "rewards", "states"))
    assert "track_err" not in ep and "demo_windows" not in ep


# ---- with the other records -------------------------------------------------------------------------------------------------

def test_delay_record_moves_the_windows_ahead(gpu, orc_omp):
    name = "humanoidtrack"
    env = _env(name)
    ref, info = mdc.case(orc_omp, name, "delay")
    T, E, D = mdc.DELAY
    plan = _plan(env, name, info["state0"])
    plan.set_mpc_delay(D)
    ep, _, _ = _run_case(orc_omp, env, name, "delay", plan)
    plan.close()
    _equal(ep, ref, "delay", logs=_LOGS + ("predicted",))
    _track_err_close(ep["track_err"], ref["track_err"], "delay")
    clip = mdc.as_tracks(info["clip"])
    for t in range(T):
        assert np.array_equal(ep["demo_windows"][t][:, 0], clip[:, info["c0"] + (t + D) * E])


def test_plant_record_tracks_the_plants_positions(gpu, orc_omp):
    from mbd_hip.envs.base import RigidBodyEnv
    name = "humanoidtrack"
    env = _env(name)
    plant = RigidBodyEnv(name, model=env.sys.scaled(**mdc.MISMATCH))
    ref, info = mdc.case(orc_omp, name, "plant")
    nominal, _ = mdc.case(orc_omp, name, "moving")
    plan = _plan(env, name, info["state0"])
    plan.set_mpc_plant(env=plant, key=info["dkey"], **mdc.PLANT)
    ep, _, _ = _run_case(orc_omp, env, name, "plant", plan)
    plan.close()
    _equal(ep, ref, "plant")
    _track_err_close(ep["track_err"], ref["track_err"], "plant")
    assert not np.array_equal(ref["xpos"], nominal["xpos"]) and not np.array_equal(ref["track_err"], nominal["track_err"])


def test_sweep_episodes_equal_the_single_plans(gpu, orc_omp):
    from mbd_hip.planners.mbd_planner import Sweep
    name, P = "humanoidtrack", 2
    env = _env(name)
    _, info = mdc.case(orc_omp, name, "moving")
    T, E, c0 = mdc.SHAPES["moving"]
    keys = np.stack([gpu.prng_key(mdc.SEED_KEY + 10 * k) for k in range(P)])
    states = [np.asarray(env.reset(gpu.prng_key(mdc.SEED_RESET + k)).pipeline_state, np.float32).reshape(-1) for k in range(P)]
    sweep = Sweep(env, _args(name), P)
    for k in range(P):
        sweep.set_state0(k, _state(states[k]))
    sweep.set_mpc_demo(info["clip"], c0, info["rew_xref"])
    batch = sweep.run_mpc(keys, T, mdc.WARM, E)
    sweep.close()
    singles = []
    for k in range(P):
        plan = _plan(env, name, states[k])
        plan.set_mpc_demo(info["clip"], c0, info["rew_xref"])
        singles.append(plan.run_mpc(keys[k], T, mdc.WARM, E))
        plan.close()
        for log in ("means", "actions", "rewards", "states", "track_err"):
            assert np.array_equal(batch[log][k], singles[k][log]), (k, log)
        assert np.array_equal(batch["demo_windows"], singles[k]["demo_windows"])
    assert not np.array_equal(singles[0]["means"], singles[1]["means"])


# ---- refusals ---------------------------------------------------------------------------------------------------------------

def test_refusals(gpu):
    from mbd_hip.envs.base import RigidBodyEnv
    from mbd_hip.model import Model
    from mbd_hip.planners.mbd_planner import Plan, Sweep
    lib = gpu.load()
    name = "humanoidtrack"
    env = _env(name)
    s = np.asarray(env.reset(gpu.prng_key(1)).pipeline_state, np.float32).reshape(-1)
    plan = _plan(env, name, s)
    sweep = Sweep(env, _args(name), 2)
    clip = np.ascontiguousarray(mdc.extended(env.xref), np.float32)
    key = gpu.key_array([0, 1])
    mc = gpu.MpcConfig(n_ticks=2, warm_steps=2, exec_steps=1)

    def rec(**kw):
        r = gpu.MpcDemo(clip=clip.ctypes.data_as(C.POINTER(C.c_float)), n_rows=clip.shape[1], start_row=0, rew_xref=1.0)
        for k, v in kw.items():
            if k == "reserved":
                r.reserved[v] = 1
            else:
                setattr(r, k, v)
        return r

    def run(p):
        return lib.mbd_plan_run_mpc(p.h, C.byref(mc), key, None, None, None, None, None), lib.mbd_last_error()

    # a demo plan without a record stays refused, and there is nothing to peek
    rc, msg = run(plan)
    assert rc == gpu.MBD_ERR_UNSUPPORTED and b"enable_demo" in msg, msg
    assert lib.mbd_plan_peek_mpc_track(plan.h, None, None) == gpu.MBD_ERR_STATE
    bad = clip.copy()
    bad[2, 5, 1] = np.nan
    nan_rec = rec()
    nan_rec.clip = bad.ctypes.data_as(C.POINTER(C.c_float))
    cases = [(rec(clip=None), b"clip"), (rec(n_rows=0), b"n_rows"), (rec(start_row=-1), b"start_row"), (nan_rec, b"clip[2][5][1]"),
             (rec(rew_xref=float("inf")), b"rew_xref"), (rec(rew_xref=float("nan")), b"rew_xref"), (rec(reserved=2), b"reserved")]
    for set_, h in ((lib.mbd_plan_set_mpc_demo, plan.h), (lib.mbd_sweep_set_mpc_demo, sweep.h)):
        for r, field in cases:
            assert set_(h, C.byref(r)) == gpu.MBD_ERR_INVALID and field in lib.mbd_last_error(), (field, lib.mbd_last_error())
    rc, msg = run(plan)  # (a refused record sets nothing)
    assert rc == gpu.MBD_ERR_UNSUPPORTED and b"enable_demo" in msg
    # a plan that does not use demos; an env without a demo
    for make, h_of, set_ in ((lambda e, n: _plan(e, n, s if n == name else np.asarray(e.reset(gpu.prng_key(1)).pipeline_state, np.float32).reshape(-1), demo=False),
                              lambda p: p.h, lib.mbd_plan_set_mpc_demo),
                             (lambda e, n: Sweep(e, _args(n, demo=False), 2), lambda w: w.h, lib.mbd_sweep_set_mpc_demo)):
        no_demo = make(env, name)
        assert set_(h_of(no_demo), C.byref(rec())) == gpu.MBD_ERR_INVALID and b"does not use demos" in lib.mbd_last_error()
        no_demo.close()
        run_env = _env("humanoidrun")
        no_xref = make(run_env, "humanoidrun")
        assert set_(h_of(no_xref), C.byref(rec())) == gpu.MBD_ERR_INVALID and b"xref" in lib.mbd_last_error()
        no_xref.close()
    # with a record: the peek before an episode; then an episode; cleared, the plan is refused again
    plan.set_mpc_demo(clip, 0)
    assert lib.mbd_plan_peek_mpc_track(plan.h, None, None) == gpu.MBD_ERR_STATE and b"episode" in lib.mbd_last_error()
    assert run(plan)[0] == gpu.MBD_OK and lib.mbd_plan_peek_mpc_track(plan.h, None, None) == gpu.MBD_OK
    sweep.set_mpc_demo(clip, 0)
    assert lib.mbd_sweep_peek_mpc_track(sweep.h, 0, None, None) == gpu.MBD_ERR_STATE
    assert lib.mbd_sweep_peek_mpc_track(sweep.h, 2, None, None) == gpu.MBD_ERR_INVALID
    # a plant that tracks other links
    f = dict(env.sys.fields)
    f["track_link"] = np.asarray(f["track_link"])[::-1].copy()
    other = RigidBodyEnv(name, model=Model(f, env.sys.link_names, env.sys.actuator_names, name))
    plan.set_mpc_plant(env=other)
    rc, msg = run(plan)
    assert rc == gpu.MBD_ERR_INVALID and b"track_link" in msg, msg
    plan.clear_mpc_plant()
    plan.clear_mpc_demo()
    rc, msg = run(plan)
    assert rc == gpu.MBD_ERR_UNSUPPORTED and b"enable_demo" in msg
    assert lib.mbd_plan_peek_mpc_track(plan.h, None, None) == gpu.MBD_ERR_STATE
    # the ensemble's refusal of demo plans stays
    with pytest.raises(gpu.MbdError, match="enable_demo"):
        plan.set_ensemble([None, None])
    plan.close()
    sweep.close()


def test_plant_refusals_and_path_integral_handles(gpu):
    """The other refusals around a record.  A plant whose n_track differs (humanoidrun: the same body, no tracked links) or whose
    tracked links differ is refused at the run call, by a plan and — through the per-episode loop — by a sweep, whichever episode
    carries it.  A handle that carries demos AND a path-integral update cannot be made at all: mbd_plan_create and
    mbd_sweep_create refuse it (MBD_ERR_INVALID), so no record ever reaches the path-integral score path; the run call's
    update_method refusal stays behind the enable_demo one for handles without demos."""
    from mbd_hip.envs.base import RigidBodyEnv
    from mbd_hip.model import Model
    from mbd_hip.planners.mbd_planner import Plan, Sweep
    lib = gpu.load()
    name = "humanoidtrack"
    env = _env(name)
    for make in (lambda: Plan(env, _args(name), update_method=1), lambda: Sweep(env, _args(name), 2, update_method=1)):
        with pytest.raises(gpu.MbdError, match="do not use demos") as e:
            make()
        assert e.value.code == gpu.MBD_ERR_INVALID
    s = np.asarray(env.reset(gpu.prng_key(1)).pipeline_state, np.float32).reshape(-1)
    clip = np.ascontiguousarray(mdc.extended(env.xref), np.float32)
    mc = gpu.MpcConfig(n_ticks=2, warm_steps=2, exec_steps=1)
    keys = np.stack([gpu.prng_key(k) for k in range(2)])
    f = dict(env.sys.fields)
    f["track_link"] = np.asarray(f["track_link"])[::-1].copy()
    other_links = RigidBodyEnv(name, model=Model(f, env.sys.link_names, env.sys.actuator_names, name))
    no_tracks = _env("humanoidrun")
    plan = _plan(env, name, s)
    plan.set_mpc_demo(clip, 0)
    sweep = Sweep(env, _args(name), 2)
    for k in range(2):
        sweep.set_state0(k, _state(s))
    sweep.set_mpc_demo(clip, 0)

    def run_plan():
        return lib.mbd_plan_run_mpc(plan.h, C.byref(mc), gpu.key_array(keys[0]), None, None, None, None, None), lib.mbd_last_error()

    def run_sweep():
        return lib.mbd_sweep_run_mpc(sweep.h, C.byref(mc), gpu.np_ptr(keys), None, None, None, None, None), lib.mbd_last_error()

    for plant, field in ((no_tracks, b"n_track"), (other_links, b"track_link")):
        plan.set_mpc_plant(env=plant)
        rc, msg = run_plan()
        assert rc == gpu.MBD_ERR_INVALID and field in msg, msg
        plan.clear_mpc_plant()
        for k in range(2):  # (whichever episode carries the plant)
            sweep.set_mpc_plant(k, env=plant)
            rc, msg = run_sweep()
            assert rc == gpu.MBD_ERR_INVALID and field in msg, (k, msg)
            sweep.clear_mpc_plant(k)
    assert run_plan()[0] == gpu.MBD_OK and run_sweep()[0] == gpu.MBD_OK
    plan.set_mpc_plant(env=RigidBodyEnv(name, model=env.sys.scaled(mass=1.2)))  # (the same tracked links: accepted)
    assert run_plan()[0] == gpu.MBD_OK
    plan.clear_mpc_demo()
    sweep.clear_mpc_demo()
    for rc, msg in (run_plan(), run_sweep()):  # (without a record: as before)
        assert rc == gpu.MBD_ERR_UNSUPPORTED and b"enable_demo" in msg, msg
    plan.close()
    sweep.close()


def test_open_loop_runs_ignore_the_record(gpu, orc_omp):
    """mbd_plan_run and mbd_sweep_run with a record that is NOT the env's demo — the synthetic clip from row 7, another reward
    level — give the bits they give without one."""
    from mbd_hip.planners.mbd_planner import Sweep
    name = "humanoidtrack"
    env = _env(name)
    _, info = mdc.case(orc_omp, name, "moving")
    keys = np.stack([gpu.prng_key(mdc.SEED_KEY + k) for k in range(2)])
    plan = _plan(env, name, info["state0"])
    sweep = Sweep(env, _args(name), 2)
    for k in range(2):
        sweep.set_state0(k, _state(info["state0"]))
    before = plan.run(keys[0])[:3], sweep.run(keys)[:3]
    plan.set_mpc_demo(info["clip"], 7, 0.25)
    sweep.set_mpc_demo(info["clip"], 7, 0.25)
    ep = plan.run_mpc(keys[0], 2, mdc.WARM, 1)  # (an episode under the record in between: it leaves nothing behind either)
    after = plan.run(keys[0])[:3], sweep.run(keys)[:3]
    plan.set_mpc_demo(env.xref, 0)
    own = plan.run_mpc(keys[0], 2, mdc.WARM, 1)
    plan.close()
    sweep.close()
    for b, a in zip(before, after):
        for x, y in zip(b, a):
            assert np.array_equal(np.asarray(x), np.asarray(y))
    assert not np.array_equal(ep["means"][0], own["means"][0])  # (the record is one an episode can tell from the env's demo)


# ---- the command line -------------------------------------------------------------------------------------------------------

def test_command_line(gpu, tmp_path):
    from mbd_hip.planners.mpc import run_mpc
    flags = dict(n_ticks=3, warm_steps=mdc.WARM, exec_steps=3, demo_clip="env", demo_start=2, demo_period=20)
    _, det = run_mpc(_args("humanoidtrack", **flags), return_details=True)
    assert det["demo_windows"].shape == (3, 5, 50, 3) and det["demo_period"] == 20
    pkg = os.path.join(ROOT, "model-based-diffusion_amd")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([pkg, ROOT, os.environ.get("PYTHONPATH", "")]))
    argv = ["--env_name", "humanoidtrack", "--disable_recommended_params", "--enable_demo", "--Nsample", str(mdc.N), "--Hsample", "50",
            "--Ndiffuse", str(mdc.ND), "--temp_sample", str(mdc.TEMP)] + [x for k, v in flags.items() for x in (f"--{k}", str(v))]
    out = subprocess.run([sys.executable, "-m", "mbd_hip.planners.mpc"] + argv, cwd=tmp_path, env=env, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["demo_clip"] == "env" and res["demo_start"] == 2 and res["demo_period"] == 20
    assert np.float32(res["track_err_mean"]) == np.float32(det["track_err"].mean())
    assert np.float32(res["episode_reward"]) == np.float32(det["rewards"].mean())
    saved = np.load(os.path.join(tmp_path, "results", "humanoidtrack", "mpc_episode.npz"))
    assert np.array_equal(saved["track_err"], det["track_err"]) and np.array_equal(saved["demo_windows"], det["demo_windows"])
    alone = subprocess.run([sys.executable, "-m", "mbd_hip.planners.mpc"] + argv[: argv.index("--demo_clip")] + ["--n_ticks", "2"],
                           cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert alone.returncode != 0 and "enable_demo" in alone.stderr  # (--enable_demo alone stays refused)
