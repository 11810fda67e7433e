"""Planning over an ensemble of perturbed models on the GPU (include/mbd_hip.h mbd_ensemble, mbd_plan_set_ensemble,
mbd_plan_peek_ensemble; DESIGN.md section 1 "N6 ensemble"), bit for bit against tests/ensemble_checker.py: the per-member
rewards of every kernel family against mbd_env_rollout on the member's env and against the checker, single steps and whole
plans under both risk modes, episodes with and without a plant record, the identities (no record = the parent, M = 1 = no
record, clear restores, prefixes, tick 0), the launch levers, and every refusal with its code and field name.  Every
comparison is np.array_equal."""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest

import ensemble_checker as ec
from conftest import load_model

pytestmark = pytest.mark.gpu

SCALES = [dict(mass=0.8, friction=1.3, gear=1.1), dict(mass=1.25, friction=0.7, gear=0.9), dict(mass=1.5, friction=1.0, gear=1.2)]


@pytest.fixture(scope="module")
def gpu(lib):
    from mbd_hip import _capi
    if _capi.device_count() < 1:
        pytest.fail("GPU tests need a visible MI355X; the product has no CPU fallback")
    return _capi


def _args(name, N, H=20, Nd=4, temp=0.1):
    from mbd_hip.planners.mbd_planner import Args
    return Args(env_name=name, Nsample=N, Hsample=H, Ndiffuse=Nd, temp_sample=temp, disable_recommended_params=True,
                not_render=True)


def _env(name, model=None):
    from mbd_hip.envs import get_env
    from mbd_hip.envs.base import RigidBodyEnv
    return get_env(name) if model is None else RigidBodyEnv(name, model=model)


def _members(env, scales=SCALES):
    """The plan's own env (NULL) and one env per scale."""
    return [None] + [_env(env.env_name, env.sys.scaled(**s)) for s in scales]


def _oenvs(orc, env, members):
    from test_gpu_parity import _oenv
    return _oenv(orc, env), [None if m is None else _oenv(orc, m) for m in members]


def _check_plan(gpu, orc, env, members, risk, N, H, Nd, seed=1, want_choice=None):
    """A whole mbd_plan_run with the record against the checker's plan, and the last step's peeked data: r_m against
    mbd_env_rollout on member m's env for the peeked Y0s and against the checker; the combined rewards; the weights."""
    from mbd_hip.planners.mbd_planner import Plan
    a = _args(env.env_name, N, H, Nd)
    st = env.reset(gpu.prng_key(seed))
    key = gpu.prng_key(100 + seed)
    plan = Plan(env, a)
    plan.set_state0(st)
    plan.set_ensemble(members, risk)
    if want_choice is not None:
        ch = gpu.debug_rollout_choice(env.sys.to_struct(), 256, len(members) * N, H, sweep_plan_N=N)
        assert want_choice in ch["name"], ch
    mu, rm, rf, _ = plan.run(key)
    Y0s, rewss, w = plan.peek()
    r_m, rews = plan.peek_ensemble()
    oe, oms = _oenvs(orc, env, members)
    s0 = np.asarray(st.pipeline_state, np.float32)
    ref = ec.plan(orc, oe, oms, risk, s0, key, N, H, Nd, a.temp_sample, impl=plan.cfg.prng_impl)
    assert np.array_equal(mu, ref["mu_0ts"]) and np.array_equal(rm, ref["rew_means"]) and np.float32(rf) == ref["rew_final"]
    # the last step (i = 1) again, from the plan's own Ybar_1, spelled out by the checker
    sched = orc.schedule(a.beta0, a.betaT, Nd)
    r = key
    for _ in range(Nd - 2):
        r = orc.split(r, 2, plan.cfg.prng_impl)[0]
    Ybar1 = mu[-2] if Nd > 2 else np.zeros((H, env.action_size), np.float32)
    _, Y, _, d = ec.step(orc, oe, oms, risk, s0, 1, r, Ybar1, sched, N, H, a.temp_sample, impl=plan.cfg.prng_impl)
    assert np.array_equal(Y0s, d["Y0s"]) and np.array_equal(r_m, d["r_members"]) and np.array_equal(rews, d["rews"])
    assert np.array_equal(w, d["weights"]) and np.array_equal(Y, mu[-1])
    for m, me in enumerate(members):
        got = (env if me is None else me).rollout(st, Y0s).cpu().numpy()
        assert np.array_equal(r_m[m], ec.op.mean_h(orc, got)), f"member {m}"
        if m == 0:
            assert np.array_equal(rewss, got)  # (mbd_plan_peek's rewss is member 0's)
    assert not np.array_equal(r_m[0], r_m[1])
    plan.close()
    return mu, rm


@pytest.mark.parametrize("risk", ["mean", "min"])
@pytest.mark.parametrize("name,N", [("hopper", 256), ("halfcheetah", 128)])
def test_planar_families(gpu, orc_omp, name, N, risk):
    env = _env(name)
    _check_plan(gpu, orc_omp, env, _members(env), risk, N, 20, 4)


@pytest.mark.parametrize("N,risk", [(256, "mean"), (256, "min"), (1024, "mean")])
def test_humanoid_one_candidate_per_lane_group(gpu, orc_omp, N, risk):
    env = _env("humanoidrun")
    _check_plan(gpu, orc_omp, env, _members(env), risk, N, 20, 4, want_choice="rollout_kernel")


def test_two_candidates_per_lane(gpu, orc_omp):
    """M N = 4 x 2048 = 8192 humanoid candidates: choose_rollout sends the launch to the two-per-lane kernel."""
    env = _env("humanoidrun")
    _check_plan(gpu, orc_omp, env, _members(env), "min", 2048, 8, 3, want_choice="pk2")


def test_general_spec_instantiation(gpu, orc_omp):
    """A model off the build's word of specification switches (friction_vel_bound set) runs the general SPEC instantiations."""
    m = load_model("humanoidrun")
    m.fields["flags"] = int(m.fields["flags"]) | 16
    env = _env("humanoidrun", m)
    _check_plan(gpu, orc_omp, env, _members(env, SCALES[:2]), "mean", 128, 10, 3, want_choice="rollout_kernel")


def test_members_launched_one_by_one_when_a_wavefront_would_straddle(gpu, orc_omp):
    """N = 100 is no multiple of the hopper's candidates per wavefront: one launch per member, same bits."""
    env = _env("hopper")
    _check_plan(gpu, orc_omp, env, _members(env, SCALES[:2]), "mean", 100, 10, 3)


def _run_all(plan, key):
    mu, rm, rf, _ = plan.run(key)
    return [np.asarray(mu), np.asarray(rm), np.float32(rf)]


@pytest.mark.parametrize("name,N", [("humanoidrun", 256), ("hopper", 512)])
def test_identities(gpu, name, N):
    """No record = a fresh plan (the parent's launches); M = 1 with a NULL member or a second env of the same model = no
    record, under either risk; clearing a record restores the plan without one."""
    from mbd_hip.planners.mbd_planner import Plan
    env = _env(name)
    a = _args(name, N, 20, 8)
    st, key = env.reset(gpu.prng_key(3)), gpu.prng_key(4)
    plan = Plan(env, a)
    plan.set_state0(st)
    ref = _run_all(plan, key)
    for members, risk in (([None], "mean"), ([None], "min"), ([_env(name)], "mean"), ([env], "min")):
        plan.set_ensemble(members, risk)
        got = _run_all(plan, key)
        assert all(np.array_equal(x, y) for x, y in zip(got, ref)), (risk,)
    members = _members(env)
    plan.set_ensemble(members, "min")
    other = _run_all(plan, key)
    assert not np.array_equal(other[0], ref[0])
    plan.set_ensemble(members[::-1], "min")  # MIN does not depend on the members' order
    assert all(np.array_equal(x, y) for x, y in zip(_run_all(plan, key)[:2], other[:2]))
    plan.clear_ensemble()
    assert all(np.array_equal(x, y) for x, y in zip(_run_all(plan, key), ref))
    fresh = Plan(env, a)
    fresh.set_state0(st)
    assert all(np.array_equal(x, y) for x, y in zip(_run_all(fresh, key), ref))
    plan.close()
    fresh.close()


@pytest.mark.parametrize("name,N", [("hopper", 256), ("humanoidrun", 256)])
def test_levers_give_the_same_bits(gpu, levers, name, N):
    """Noise prefetch on and off, cpw forced, the XCD pin asked for, the two-per-lane kernel forced, one launch per member."""
    from mbd_hip.planners.mbd_planner import Plan
    env = _env(name)
    members = _members(env)
    a = _args(name, N, 20, 8)
    st, key = env.reset(gpu.prng_key(5)), gpu.prng_key(6)

    def run():
        plan = Plan(env, a)
        plan.set_state0(st)
        plan.set_ensemble(members, "mean")
        out = _run_all(plan, key) + list(plan.peek_ensemble())
        plan.close()
        return out
    ref = run()
    # (MBD_ROLL_PIN = 1 is a no-op by design: the pin is a single-plan form and an ensemble launch is never pinned — the
    # lever must still change nothing; MBD_CPW = 1 is the hopper's own choice at this size, 2 and 0 are not)
    for kw in (dict(MBD_NO_PREFETCH=1), dict(MBD_NO_FUSED_NOISE=1), dict(MBD_CPW=1), dict(MBD_CPW=2), dict(MBD_CPW=0), dict(MBD_ROLL_PIN=1),
               dict(MBD_PK2=1), dict(MBD_ENS_SPLIT=1), dict(MBD_NO_LAZY=1)):
        levers(**kw)
        got = run()
        assert all(np.array_equal(x, y) for x, y in zip(got, ref)), kw
        levers(**{k: -1 for k in kw})


@pytest.mark.parametrize("risk", ["mean", "min"])
def test_the_two_phase_calls_read_the_record(gpu, orc_omp, risk):
    """mbd_plan_sample_rollout called directly: d_rews_local receives the COMBINED rewards; mbd_plan_score_update, handed
    those, gives the checker's Ybar_{i-1}, weights and mean reward."""
    import torch
    from mbd_hip.planners.mbd_planner import Plan
    env = _env("hopper")
    members = _members(env)
    N, H, Nd = 256, 20, 6
    a = _args("hopper", N, H, Nd)
    st, key = env.reset(gpu.prng_key(12)), gpu.prng_key(13)
    plan = Plan(env, a)
    plan.set_state0(st)
    plan.set_ensemble(members, risk)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    Ybar_h = (0.1 * orc_omp.normal(orc_omp.prng_key(2), (H, env.action_size), 1)).astype(np.float32)
    Ybar = torch.as_tensor(Ybar_h, device=dev).contiguous()
    local, out, mean = (torch.zeros(n, dtype=torch.float32, device=dev) for n in (N, H * env.action_size, 1))
    impl, i = plan.cfg.prng_impl, 3
    ks = gpu.key_array(gpu.prng_split(key, 2, impl)[1])
    gpu.check(plan.lib.mbd_plan_sample_rollout(plan.h, i, ks, Ybar.data_ptr(), local.data_ptr(), None, stream))
    torch.cuda.synchronize(dev)
    oe, oms = _oenvs(orc_omp, env, members)
    sched = orc_omp.schedule(a.beta0, a.betaT, Nd)
    _, Y, rm, d = ec.step(orc_omp, oe, oms, risk, np.asarray(st.pipeline_state, np.float32), i, key, Ybar_h, sched, N, H,
                          a.temp_sample, impl=impl)
    assert np.array_equal(local.cpu().numpy(), d["rews"])
    r_m, rews = plan.peek_ensemble()
    assert np.array_equal(r_m, d["r_members"]) and np.array_equal(rews, d["rews"])
    gpu.check(plan.lib.mbd_plan_score_update(plan.h, i, ks, Ybar.data_ptr(), local.data_ptr(), None, out.data_ptr(),
                                             mean.data_ptr(), stream))
    torch.cuda.synchronize(dev)
    assert np.array_equal(out.cpu().numpy().reshape(H, -1), Y) and np.float32(mean.item()) == np.float32(rm)
    assert np.array_equal(plan.peek()[2], d["weights"])
    plan.close()


_LOGS = ("means", "actions", "rewards", "states")


@pytest.mark.parametrize("name,N,risk,plant", [("hopper", 256, "mean", False), ("hopper", 256, "min", True),
                                               ("humanoidrun", 256, "min", False), ("humanoidrun", 256, "mean", True)])
def test_episodes(gpu, orc_omp, name, N, risk, plant):
    """mbd_plan_run_mpc with an ensemble, and with an ensemble plus a plant record with noise and kicks: the four logs against
    the checker; T ticks are a prefix of T + 2; tick 0's mean is mbd_plan_run(k_0) with the same record."""
    from mbd_hip.planners.mbd_planner import Plan
    from test_gpu_parity import _oenv
    env = _env(name)
    members = _members(env, SCALES[:2])
    H, Nd, K, E, T = 20, 8, 3, 2, 4
    a = _args(name, N, H, Nd)
    st, key = env.reset(gpu.prng_key(7)), gpu.prng_key(8)
    plan = Plan(env, a)
    plan.set_state0(st)
    plan.set_ensemble(members, risk)
    kw, penv = {}, None
    if plant:
        penv = _env(name, env.sys.scaled(mass=1.3, friction=0.5, gear=0.8))
        kw = dict(dkey=gpu.prng_key(11), act_std=0.3, kick_std=0.5, kick_every=3)
        plan.set_mpc_plant(env=penv, key=kw["dkey"], act_std=0.3, kick_std=0.5, kick_every=3)
    ep = plan.run_mpc(key, T, K, E)
    oe, oms = _oenvs(orc_omp, env, members)
    ref = ec.episode(oe, oms, risk, np.asarray(st.pipeline_state, np.float32), key, N, H, Nd, a.temp_sample, T, K, E,
                     plant=None if penv is None else _oenv(orc_omp, penv), impl=plan.cfg.prng_impl, **kw)
    for k in _LOGS:
        assert np.array_equal(np.asarray(ep[k]).reshape(ref[k].shape), ref[k]), k
    longer = plan.run_mpc(key, T + 2, K, E)
    for k in _LOGS:
        assert np.array_equal(ep[k], longer[k][: len(ep[k])]), k
    mu0 = plan.run(gpu.prng_split(key, 2, plan.cfg.prng_impl)[1])[0]
    assert np.array_equal(ep["means"][0], mu0[-1])
    plan.close()


def test_mpc_front_end_reports_the_ensemble(gpu):
    from mbd_hip.planners.mpc import MpcArgs, run_mpc
    a = MpcArgs(env_name="hopper", Nsample=128, Hsample=20, Ndiffuse=6, n_ticks=3, warm_steps=2, disable_recommended_params=True,
                not_render=True, ens_mass="0.8,1,1.25", ens_friction="0.7", ens_risk="min", plant_mass=1.25)
    rew, det = run_mpc(replace(a), return_details=True)
    assert det["ens_risk"] == "min" and det["ensemble"] == [dict(mass=0.8, friction=0.7, gear=1.0), dict(mass=1.0, friction=0.7, gear=1.0),
                                                            dict(mass=1.25, friction=0.7, gear=1.0)]
    nominal, det0 = run_mpc(replace(a, ens_mass="", ens_friction="", ens_risk="mean"), return_details=True)
    assert "ensemble" not in det0 and not np.array_equal(det["means"], det0["means"]) and np.isfinite(rew)


def test_run_diffusion_takes_an_ensemble(gpu):
    from mbd_hip.planners.mbd_planner import run_diffusion
    a = _args("hopper", 128, 20, 6)
    env = _env("hopper")
    base, d0 = run_diffusion(replace(a), return_details=True)
    same, d1 = run_diffusion(replace(a), return_details=True, ensemble=[None])
    assert np.array_equal(d0["mu_0ts"], d1["mu_0ts"]) and base == same
    _, d2 = run_diffusion(replace(a), return_details=True, ensemble=dict(envs=_members(env), risk="min"))
    assert not np.array_equal(d0["mu_0ts"], d2["mu_0ts"])


# ---- refusals: at the set call, before any launch, naming the field -------------------------------------------------------

def _refused(gpu, plan, rec, code, field):
    rc = plan.lib.mbd_plan_set_ensemble(plan.h, C.byref(rec))
    msg = plan.lib.mbd_last_error().decode()
    assert rc == code and field in msg, (rc, msg)


def _rec(gpu, members=(None,), risk=0):
    rec = gpu.Ensemble()
    for m, e in enumerate(members):
        rec.members[m] = None if e is None else e.handle
    rec.n_members, rec.risk = len(members), risk
    rec.keep_alive = list(members)  # (a record does not own its members: the envs must outlive the call that reads them)
    return rec


def test_refusals(gpu):
    from mbd_hip.planners.mbd_planner import Plan
    env = _env("hopper")
    a = _args("hopper", 64, 10, 4)
    plan = Plan(env, a)
    plan.set_state0(env.reset(gpu.prng_key(0)))
    key = gpu.prng_key(1)
    ref = _run_all(plan, key)
    INV, UNS, STA = gpu.MBD_ERR_INVALID, gpu.MBD_ERR_UNSUPPORTED, gpu.MBD_ERR_STATE
    for n in (0, -1, 9):
        rec = _rec(gpu)
        rec.n_members = n
        _refused(gpu, plan, rec, INV, "n_members")
    _refused(gpu, plan, _rec(gpu, risk=2), INV, "risk")
    _refused(gpu, plan, _rec(gpu, risk=-1), INV, "risk")
    rec = _rec(gpu)
    rec.reserved[5] = 1
    _refused(gpu, plan, rec, INV, "reserved[5]")
    with pytest.raises(ValueError, match="risk"):
        plan.set_ensemble([None], "cvar")
    with pytest.raises(ValueError, match="members"):
        plan.set_ensemble([None] * 9)
    # members of another topology or another launch
    _refused(gpu, plan, _rec(gpu, (None, _env("halfcheetah"))), INV, "n_links")
    _refused(gpu, plan, _rec(gpu, (None, _env("car2d"))), INV, "no model")
    # one edited copy of the hopper per field (another topology needs no other robot).  Where two checks would fire, the
    # message asserted is the one that fires FIRST in check_ensemble's order (n_links, action_size, planar flag, spec word,
    # reward_kind, n_frames, n_col, ..., col_link, parent, n_rot, n_slide, actuators, then the wave-uniform switches
    # slide_limits, max_children, max_rot, any_stiff, has_weld, then the lane tables and the rest of the shape): a second
    # child on link 1 also raises max_children, a weld also sets has_weld, a second hinge dof also raises max_rot — all three
    # are stopped at the tree tables, which come first.

    def set_(k, v):
        return lambda f: f.__setitem__(k, v)

    def at(k, idx, v):
        def edit(f):
            a = np.array(f[k])
            a[idx] = v
            f[k] = a
        return edit
    cases = (("n_frames", set_("n_frames", 18)),
             ("flags", lambda f: f.__setitem__("flags", int(f["flags"]) | 16)),
             ("planar flag", lambda f: f.__setitem__("flags", int(f["flags"]) & ~2)),
             ("any_stiff", lambda f: f.__setitem__("rot_stiff", np.asarray(f["rot_stiff"], np.float32) + np.float32(5))),
             ("action_size", set_("n_act", 2)),                 # the last actuator dropped
             ("col_link", at("col_link", 0, 2)),                # a collider moved to another link (max_col follows)
             ("n_col", set_("n_col", 1)),                       # a collider removed
             ("parent", at("parent", 3, 1)),                    # the foot hung on the thigh: the tree (max_children, lane tables follow)
             ("n_rot", at("n_rot", 3, 0)),                      # the foot joint a weld (has_weld follows)
             ("n_slide", at("n_slide", 0, 1)),                  # the root loses a slide dof (max_slide follows)
             ("slide_limits", at("slide_lo", (0, 0), -5.0)))    # a finite range on a root slide
    for field, edit in cases:
        m = load_model("hopper")
        edit(m.fields)
        _refused(gpu, plan, _rec(gpu, (None, _env("hopper", m))), INV, field)
    # max_rot, max_children and has_weld alone cannot differ while the tree tables agree (they are functions of parent and
    # n_rot): their lines are reached only behind a tree check, asserted above.  The lane tables can: an env created under
    # MBD_NO_DPP keeps the shuffle exchange for the same tree.
    gpu.debug_set("MBD_NO_DPP", 1)
    try:
        shuffled = _env("hopper", load_model("hopper"))
    finally:
        gpu.debug_set("MBD_NO_DPP", -1)
    _refused(gpu, plan, _rec(gpu, (None, shuffled)), INV, "dpp_family (lane table)")
    # (a member on another device needs a second GPU: not exercised here)
    hm = load_model("humanoidrun")
    henv = _env("humanoidrun")
    hplan = Plan(henv, _args("humanoidrun", 64, 10, 4))
    hm.fields["reward_kind"] = 4  # (humanoidstandup's reward on the same body)
    _refused(gpu, hplan, _rec(gpu, (_env("humanoidrun", hm),)), INV, "reward_kind")
    hplan.close()
    # everything Model.scaled produces is accepted
    plan.set_ensemble([_env("hopper", env.sys.scaled(mass=2.0, friction=0.3, gear=0.5)), None, env], "min")
    plan.clear_ensemble()
    # plans an ensemble cannot score
    for kw, code, field in ((dict(update_method=1), UNS, "update_method"), (dict(shard_begin=0, shard_count=32), STA, "shard_count")):
        p2 = Plan(env, a, **kw)
        _refused(gpu, p2, _rec(gpu), code, field)
        p2.close()
    tenv = _env("humanoidtrack")
    p3 = Plan(tenv, replace(_args("humanoidtrack", 64, 50, 4), enable_demo=True))
    _refused(gpu, p3, _rec(gpu), UNS, "enable_demo")
    p3.close()
    cenv = _env("car2d")
    p4 = Plan(cenv, _args("car2d", 64, 10, 4))
    _refused(gpu, p4, _rec(gpu), UNS, "no model")
    p4.close()
    # peeking without a record, or before a step with one
    out = np.zeros(64, np.float32)
    assert plan.lib.mbd_plan_peek_ensemble(plan.h, gpu.np_ptr(out), gpu.np_ptr(out)) == STA
    plan.set_ensemble([None, None])
    assert plan.lib.mbd_plan_peek_ensemble(plan.h, gpu.np_ptr(out), gpu.np_ptr(out)) == STA
    plan.clear_ensemble()
    # no refusal left anything behind: the plan is the parent's
    assert all(np.array_equal(x, y) for x, y in zip(_run_all(plan, key), ref))
    plan.close()
