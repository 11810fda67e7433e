"""-m gpu: tracked links and demo log-densities beyond humanoidtrack's own five (tests/track_inputs.py), every comparison with
the checker by BIT PATTERN (state_inputs.same_bits).

  positions      every row of track_inputs.ROWS under every form it lists — the tuned defaults, MBD_NO_HELPERS, MBD_PK2,
                 MBD_NO_DPP, the run-time reward / n_frames / inertia forms, the specification-switch instantiation, lane groups
                 of 4, 8 and 16 — with the instantiation asserted through mbd_debug_rollout_choice: rewards, positions and final
                 states of mbd_env_rollout at B = 1, 5 (and 37), H = 7, from the reset pose and from a reached state, sentinels
                 behind every output, and the positions' last row against the link origins of the device's own final state
  logpd_track    mbd_env_xref_logpd at K = 1 ... 8, B = 1, 2, 257 on crafted positions: distances of exactly 0, one float to either
                 side of 0.5, squares that overflow, underflow and land on subnormals, an infinite coordinate, a NaN in one
                 candidate only, and the sum-order candidate
  logpd_car2d    the same in the plane at B = 1, 63, 64, 65, 129
  demo plans     N = 33, H = 50, Nd = 4 on retracked models against oracle.planner.reverse_once: humanoidtrack at K = 1, 5, 8 with
                 the log-density accumulated in the rollout and through logpd_track_kernel, humanoidrun, ant under MBD_PK2, the
                 crab, an 8-lane model; a sweep of three such plans
  demo record    one episode of humanoidrun at K = 2 whose second window clamps at the clip's end, against tests/mpc_demo_checker.py
  refusals       check_model's four with a device present; a position pointer on an env without tracked links
"""
import ctypes as C
import functools

import numpy as np
import pytest

import mpc_demo_checker as mdc
import state_inputs as si
import track_inputs as ti
from conftest import load_model
from state_inputs import same_bits

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-12345.678)
PAD = 64
H = 7


@pytest.fixture(scope="module")
def gpu(lib):
    from mbd_hip import _capi
    if _capi.device_count() < 1:
        pytest.fail("tests/test_gpu_tracks.py needs a GPU")
    return _capi


def _state(s):
    from mbd_hip.envs.base import State
    return State(np.ascontiguousarray(s, np.float32), None, np.float32(0), np.float32(0), {})


def _orc():
    from oracle.oracle import Oracle
    return Oracle("f32")


def _padded(n, dev):
    import torch
    return torch.full((n + PAD,), float(SENTINEL), dtype=torch.float32, device=dev)


def _split(t, n, what):
    """(the first n floats, asserting that the floats behind them, PAD or more, still hold the sentinel)"""
    a = t.cpu().numpy()
    assert a.size >= n + PAD
    same_bits(a[n:], np.full(a.size - n, SENTINEL), f"{what}: the floats behind the buffer")
    return a[:n]


def _rollout(env, s0, us, K, what, spare=0):
    """mbd_env_rollout into buffers with PAD sentinel floats behind each (the position buffer: PAD + spare): (rewards [B, H],
    xpos [B, H, K, 3], final [B, S])"""
    import torch
    from mbd_hip import _capi
    dev = torch.device("cuda", env.device)
    us_t = torch.as_tensor(us, dtype=torch.float32, device=dev).contiguous()
    B, Hh, _ = us_t.shape
    st = torch.as_tensor(np.ascontiguousarray(s0, np.float32).reshape(-1), device=dev)
    S = st.numel()
    rew, xpos, fin = _padded(B * Hh, dev), _padded(B * Hh * K * 3 + spare, dev), _padded(B * S, dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    _capi.check(env._lib.mbd_env_rollout(env.handle, st.data_ptr(), us_t.data_ptr(), B, Hh, rew.data_ptr(), xpos.data_ptr(),
                                         fin.data_ptr(), stream))
    torch.cuda.synchronize(dev)
    return (_split(rew, B * Hh, f"{what}: rewards").reshape(B, Hh), _split(xpos, B * Hh * K * 3, f"{what}: positions").reshape(B, Hh, K, 3),
            _split(fin, B * S, f"{what}: final states").reshape(B, S))


# ---- 1. positions from every family -----------------------------------------------------------------------------------------
B_ALL = 37


@functools.lru_cache(maxsize=None)
def _reference(model, links, word):
    """(model, env name, links, [(state name, state, actions [37], the checker's rewards, positions, final states)]) of a table
    row with the flag word changed by `word`, computed once."""
    orc = _orc()
    m, env_name, ls = ti.row_model(model, links)
    if word:
        m = m.with_spec(int(m.fields.get("flags", 0)) ^ word)
    ms = m.to_struct()
    out = []
    for what, s in (("reset pose", si.init_state(orc, m)), ("reached/1", dict(si.reached_states(orc, m))["reached/1"])):
        us = si.actions(m, si._seed("tracks", model, what), b=B_ALL, h=H)
        out.append((what, s, us) + tuple(orc.rollout(ms, s, us, want_xpos=True, want_final=True)))
    return m, env_name, ls, out


def _rows_of(B):
    """candidates of the 37 a launch of B takes: a clipped-normal row; with five the rows of zeros, of -0.0 and at a limit too"""
    return {1: [0], 5: [0, 1, B_ALL - 5, B_ALL - 4, B_ALL - 2], B_ALL: list(range(B_ALL))}[B]


def _origin64(m, state, l):
    s = np.asarray(state, np.float64).reshape(-1, 13)
    return s[l, :3] - si._rot64(s[l, 3:7], np.asarray(m.fields["com"], np.float64)[l])


CASES = [(row, model, links, form) for row, model, links, forms in ti.ROWS for form in forms]


@pytest.mark.parametrize("row,model,links,form", CASES, ids=[f"{c[0]}-{c[3]}" for c in CASES])
def test_positions_from_every_family(gpu, orc, levers, row, model, links, form):
    from mbd_hip.envs.base import RigidBodyEnv
    lev, word = ti.FORMS[form]
    m, env_name, ls, ref = _reference(model, links, word)
    K = len(ls)
    levers(**lev)  # (before the env: MBD_NO_DPP is read at creation)
    xref = ti.make_xref(orc, m, ref[0][1], 1)
    env = RigidBodyEnv(env_name, model=m, xref=xref, rew_xref=1.0)
    assert np.array_equal(env.xref, xref) and env.rew_xref == 1.0
    Bs = (1, 5, B_ALL) if model in ti.BUILTIN else (1, 5)
    for B in Bs:
        choice = gpu.debug_rollout_choice(m.to_struct(), 256, B, H, has_xref=True)
        assert ti.reaches(choice, model, form, m) is None, ti.reaches(choice, model, form, m)
        assert choice["cpw"] == 0 and not choice["fuses_logpd"], choice  # (a filled launch; H != 50: nothing accumulates)
        for what, s, us, rew, xpos, fin in ref:
            idx = _rows_of(B)
            tag = f"{row} [{form}] B={B} from the {what}"
            assert np.isfinite(xpos[idx]).all() and np.isfinite(fin[idx]).all(), tag
            g_rew, g_xpos, g_fin = _rollout(env, s, us[idx], K, tag)
            same_bits(g_rew, rew[idx], f"{tag}: rewards")
            same_bits(g_xpos, xpos[idx], f"{tag}: tracked positions")
            same_bits(g_fin, fin[idx], f"{tag}: final states")
            for b in range(len(idx)):  # the device's own output: the last row is where its final state has the links
                for k, l in enumerate(ls):
                    assert np.abs(g_xpos[b, H - 1, k] - _origin64(m, g_fin[b], l)).max() <= 1e-6, (tag, b, k)


# ---- 2. logpd_track_kernel alone --------------------------------------------------------------------------------------------
def _logpd(lib, handle, x, B, dev_index=0):
    """mbd_env_xref_logpd of host positions x ([B, 50, ...]) with PAD sentinels behind lp[B]"""
    import torch
    from mbd_hip import _capi
    dev = torch.device("cuda", dev_index)
    xt = torch.as_tensor(np.ascontiguousarray(x, np.float32), device=dev)
    out = _padded(B, dev)
    _capi.check(lib.mbd_env_xref_logpd(handle, xt.data_ptr(), B, 50, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize(dev)
    return _split(out, B, f"log-densities of {B} candidates")


@pytest.mark.parametrize("K", range(1, ti.MAX_TRACK + 1))
def test_logpd_track_kernel_alone_at_every_k(gpu, orc, K):
    from mbd_hip.envs.base import RigidBodyEnv
    m = ti.tracked(load_model("humanoidrun"), list(range(10, 10 - K, -1)))
    xref0 = ti.make_xref(orc, m, si.init_state(orc, m), K)
    xref, _ = ti.crafted(xref0, 1, K)
    env = RigidBodyEnv("humanoidrun", model=m, xref=xref, rew_xref=0.5)
    for B in (1, 2, 257):
        xr, xpos = ti.crafted(xref0, B, K)
        assert np.array_equal(xr, xref)
        assert min(ti.census(ti.terms64(xpos, xref))) > 0
        want = np.array([orc.track_xref_logpd(x, xref) for x in xpos], np.float32)
        assert np.isfinite(want).all()
        same_bits(_logpd(env._lib, env.handle, xpos, B), want, f"K={K} B={B}")
    # a NaN in ONE candidate: the others keep their bits, and that candidate is NaN exactly where the checker's is
    _, xpos = ti.crafted(xref0, 5, K)
    clean = np.array([orc.track_xref_logpd(x, xref) for x in xpos], np.float32)
    for t, k, ax in ((0, 0, 0), (49, K - 1, 2), (17, K // 2, 1)):
        x = xpos.copy()
        x[2, t, k, ax] = np.nan
        got = _logpd(env._lib, env.handle, x, 5)
        want = np.array([orc.track_xref_logpd(c, xref) for c in x], np.float32)
        keep = [0, 1, 3, 4]
        same_bits(got[keep], clean[keep], f"K={K}: the candidates beside the NaN")
        assert np.isnan(got[2]) == np.isnan(want[2]), (K, t, k, got[2], want[2])
        if not np.isnan(want[2]):
            same_bits(got[2], want[2], f"K={K}: the candidate with the NaN")


# ---- 3. logpd_car2d_kernel alone --------------------------------------------------------------------------------------------
def test_logpd_car2d_kernel_alone(gpu, orc, lib):
    import os

    from conftest import ROOT
    xref0 = np.load(os.path.join(ROOT, "model-based-diffusion_amd", "assets", "compiled", "car2d_xref.npy")).astype(np.float32)
    xref, _ = ti.crafted_car2d(xref0, 1, 0)
    h = C.c_void_p()
    gpu.check(lib.mbd_env_create_car2d(0, xref.ctypes.data_as(C.c_void_p), C.byref(h)))
    try:
        for B in (1, 63, 64, 65, 129):
            xr, qs = ti.crafted_car2d(xref0, B, B)
            assert np.array_equal(xr, xref) and min(ti.census(ti.terms64_car2d(qs, xref))) > 0
            want = np.array([orc.car2d_xref_logpd(q, xref) for q in qs], np.float32)
            assert np.isfinite(want).all()
            same_bits(_logpd(lib, h, qs, B), want, f"car2d B={B}")
        _, qs = ti.crafted_car2d(xref0, 5, 1)
        clean = np.array([orc.car2d_xref_logpd(q, xref) for q in qs], np.float32)
        qs[2, 31, 1] = np.nan
        got = _logpd(lib, h, qs, 5)
        want2 = orc.car2d_xref_logpd(qs[2], xref)
        same_bits(got[[0, 1, 3, 4]], clean[[0, 1, 3, 4]], "car2d: the candidates beside the NaN")
        assert np.isnan(got[2]) == np.isnan(want2), (got[2], want2)
    finally:
        lib.mbd_env_destroy(h)


# ---- 4. demo plans on custom tracked models ---------------------------------------------------------------------------------
N, ND, TEMP = 33, 4, 0.1
# (id, model, links, levers, whether the rollout accumulates the log-density itself)
PLANS = [
    ("humanoidtrack-k1-fused", "humanoidtrack", (0,), dict(MBD_NO_FUSED_LOGPD=0), True),
    ("humanoidtrack-k1-unfused", "humanoidtrack", (0,), dict(MBD_NO_FUSED_LOGPD=1), False),
    ("humanoidtrack-k5-fused", "humanoidtrack", (4, 6, 3, 5, 0), dict(MBD_NO_FUSED_LOGPD=0), True),
    ("humanoidtrack-k5-unfused", "humanoidtrack", (4, 6, 3, 5, 0), dict(MBD_NO_FUSED_LOGPD=1), False),
    ("humanoidtrack-k8-fused", "humanoidtrack", (9, 0, 5, 3, 6, 4, 1, 10), dict(MBD_NO_FUSED_LOGPD=0), True),
    ("humanoidtrack-k8-unfused", "humanoidtrack", (9, 0, 5, 3, 6, 4, 1, 10), dict(MBD_NO_FUSED_LOGPD=1), False),
    ("humanoidrun-k3", "humanoidrun", ("last", 0, 5), {}, False),  # (no tracking reward: never accumulated)
    ("ant-k3-pk2", "ant", (8, 0, 4), dict(MBD_PK2=1), False),
    ("crab-k2", "crab", None, {}, False),          # (lane groups of 16: the crab has ten links)
    ("small6_0-k3", "small6_0", ("last", 0, 2), {}, False),  # (lane groups of 8)
]


def _plan_args(env_name):
    from mbd_hip.planners.mbd_planner import Args
    return Args(env_name=env_name, Nsample=N, Hsample=50, Ndiffuse=ND, temp_sample=TEMP, enable_demo=True,
                disable_recommended_params=True, not_render=True)


def _checker_plan(orc, oenv, s0, key):
    """Plan.run's reverse loop by oracle.planner.reverse_once with the demo on: (mu_0ts, rew_means, the steps' details)"""
    from mbd_hip.envs.base import prng_impl
    from oracle import planner as op
    sched = orc.schedule(1e-4, 1e-2, ND)
    Ybar, r = np.zeros((50, oenv.Nu), np.float32), np.asarray(key, np.uint32)
    mus, rms, dets = [], [], []
    for i in range(ND - 1, 0, -1):
        r, Ybar, rm, det = op.reverse_once(orc, oenv, s0, i, r, Ybar, sched, N, 50, TEMP, prng_impl(), enable_demo=True)
        mus.append(Ybar)
        rms.append(rm)
        dets.append(det)
    return np.stack(mus), np.array(rms, np.float32), dets


def _demo_env(orc, model, links, seed=2):
    from mbd_hip.envs.base import RigidBodyEnv
    from oracle.planner import OracleEnv
    m, env_name, ls = ti.row_model(model, links)
    s0 = si.init_state(orc, m)
    xref = ti.make_xref(orc, m, s0, seed)
    env = RigidBodyEnv(env_name, model=m, xref=xref, rew_xref=1.0)
    oenv = OracleEnv(orc, env_name, m.to_struct(), xref=xref, rew_xref=1.0, init_q=m.init_q)
    return m, env_name, env, oenv, s0


@pytest.mark.parametrize("case,model,links,lev,fused", PLANS, ids=[p[0] for p in PLANS])
def test_demo_plans_on_custom_tracked_models(gpu, orc_omp, levers, case, model, links, lev, fused):
    from mbd_hip.planners.mbd_planner import Plan
    orc = orc_omp
    levers(**lev)
    m, env_name, env, oenv, s0 = _demo_env(orc, model, links)
    choice = gpu.debug_rollout_choice(m.to_struct(), 256, N, 50, has_xref=True)
    assert bool(choice["fuses_logpd"]) == fused, choice
    if "MBD_PK2" in lev:
        assert "rollout_pk2_kernel" in choice["name"], choice
    key = gpu.prng_key(9)
    plan = Plan(env, _plan_args(env_name))
    plan.set_state0(_state(s0))
    mu, rm, _, _ = plan.run(key)
    plan.close()
    mu_ref, rm_ref, dets = _checker_plan(orc, oenv, s0, key)
    z, i, s = ti.census(ti.terms64(dets[0]["xpos"], oenv.xref))
    assert i > 0 and s > 0, (case, z, i, s)  # distances on both sides of the clip
    assert np.ptp(dets[0]["lp"]) > 0
    same_bits(mu, mu_ref, f"{case}: mu_0ts")
    same_bits(rm, rm_ref, f"{case}: rew_means")


@pytest.mark.parametrize("model,links,lev,fused", [("humanoidtrack", (9, 0, 5, 3, 6, 4, 1, 10), dict(MBD_NO_FUSED_LOGPD=0), True),
                                                   ("humanoidtrack", (0,), dict(MBD_NO_FUSED_LOGPD=1), False),
                                                   ("humanoidrun", ("last", 0, 5), {}, False)],
                         ids=["humanoidtrack-k8-fused", "humanoidtrack-k1-unfused", "humanoidrun-k3"])
def test_a_sweep_of_three_demo_plans_equals_its_plans_run_alone(gpu, orc, levers, model, links, lev, fused):
    from mbd_hip.planners.mbd_planner import Plan, Sweep
    levers(**lev)
    m, env_name, env, oenv, s0 = _demo_env(orc, model, links)
    choice = gpu.debug_rollout_choice(m.to_struct(), 256, 3 * N, 50, sweep_plan_N=N, has_xref=True)
    assert bool(choice["fuses_logpd"]) == fused, choice
    reached = dict(si.reached_states(orc, m))
    states = [s0, reached["reached/1"], reached["reached/2"]]
    keys = np.array([gpu.prng_key(20 + k) for k in range(3)], np.uint32)
    args = _plan_args(env_name)
    sw = Sweep(env, args, 3)
    for k in range(3):
        sw.set_state0(k, _state(states[k]))
    mu, rm, rf, _ = sw.run(keys)
    sw.close()
    for k in range(3):
        p = Plan(env, args)
        p.set_state0(_state(states[k]))
        mu1, rm1, rf1, _ = p.run(keys[k])
        p.close()
        same_bits(mu[k], mu1, f"plan {k}: mu_0ts")
        same_bits(rm[k], rm1, f"plan {k}: rew_means")
        same_bits(rf[k], rf1, f"plan {k}: final reward")
    assert not np.array_equal(mu[0], mu[1])


# ---- 5. a demo record on a custom tracked model -----------------------------------------------------------------------------
def test_demo_record_on_a_custom_tracked_model(gpu, orc_omp):
    """humanoidrun tracking its last link and its torso, T = 2, E = 2, c0 = 7 under a 57-row clip: tick 0's window ends on row
    56, the clip's last; tick 1's (rows 9 ... 58) is clamped there."""
    from mbd_hip.envs.base import RigidBodyEnv, prng_impl
    from mbd_hip.planners.mbd_planner import Plan
    orc = orc_omp
    m = ti.tracked(load_model("humanoidrun"), [10, 0])
    s0 = np.ascontiguousarray(si.init_state(orc, m), np.float32).reshape(-1)
    xref = ti.make_xref(orc, m, s0.reshape(-1, 13), 5, offset=0.3)
    rew_xref, T, E, c0, WARM = 0.75, 2, 2, 7, 2
    oenv = mdc.oracle_env(orc, "humanoidrun", custom=(m, xref), rew_xref=rew_xref)
    clip = mdc.extended(xref)
    assert clip.shape == (2, 57, 3)
    key = orc.prng_key(6)
    ref = mdc.episode(oenv, clip, c0, rew_xref, s0, key, N, 50, ND, TEMP, T, WARM, E, impl=prng_impl())
    assert np.array_equal(ref["demo_windows"][0][:, -1], clip[:, 56]) and not np.array_equal(ref["demo_windows"][0][:, -2], clip[:, 56])
    assert np.array_equal(ref["demo_windows"][1][:, 47:], clip[:, [56, 56, 56]])
    env = RigidBodyEnv("humanoidrun", model=m, xref=xref, rew_xref=rew_xref)
    plan = Plan(env, _plan_args("humanoidrun"))
    plan.set_state0(_state(s0))
    plan.set_mpc_demo(clip, c0, rew_xref)
    ep = plan.run_mpc(key, T, WARM, E)
    plan.close()
    for k in ("means", "actions", "states", "demo_windows", "rewards"):
        same_bits(ep[k], ref[k], f"demo record: {k}")
    assert ep["track_err"].shape == (T * E, 2)
    got, want = np.asarray(ep["track_err"], np.float64), ref["track_err"]
    assert (want > 0).all()
    worst = (np.abs(got - want) / want).max()
    print(f"track_err: worst relative error {worst:.3g}")
    assert worst <= 1e-6


# ---- 6. the refusals, with a device present ---------------------------------------------------------------------------------
def test_refusals_with_a_device_present(gpu, lib):
    from test_tracks import REFUSALS, _create, _struct
    for case, kw, field in REFUSALS:
        rc, msg = _create(lib, _struct(**kw), np.zeros((ti.MAX_TRACK, 50, 3), np.float32))
        assert rc == gpu.MBD_ERR_INVALID and field in msg, (case, rc, msg)


@pytest.mark.parametrize("name", ["humanoidrun", "hopper"])
def test_a_position_pointer_on_an_env_without_tracked_links_is_left_alone(gpu, orc, name):
    """K = 0: mbd_env_rollout with a position buffer writes none of it (3-D and planar kernels), and rewards and final states
    are the checker's."""
    from mbd_hip.envs import get_env
    env = get_env(name)
    m = load_model(name)
    assert int(m.fields["n_track"]) == 0
    s0 = si.init_state(orc, m)
    us = si.actions(m, 3, b=9, h=H)
    rew, fin = orc.rollout(m.to_struct(), s0, us, want_final=True)
    # (K = 0: nothing of the position buffer belongs to the rollout — room for one tracked link, all sentinels)
    g_rew, g_xpos, g_fin = _rollout(env, s0, us, 0, name, spare=us.shape[0] * H * 3)
    assert g_xpos.size == 0
    same_bits(g_rew, rew, f"{name}: rewards")
    same_bits(g_fin, fin, f"{name}: final states")
