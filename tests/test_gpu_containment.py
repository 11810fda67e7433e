"""-m gpu: a candidate that leaves the finite numbers stays alone (tests/containment_inputs.py).

Every other GPU test holds the kernels to the checker where every number stays finite.  Here some candidates of a launch, one
plan of a sweep, one episode of a batch, one member of an ensemble DIVERGE — from legal, finite inputs — and everything else
must keep its bits: (a) `env.rollout` under every kernel family, the healthy candidates against the checker AND against the same
launch with every poisoned candidate replaced by its healthy twin (the device against itself), the poisoned ones against the
checker up to the row where they are poisoned and NON-FINITE wherever the checker is ("a diverged candidate is never hidden";
NaN payloads and the kind of non-finite are not compared: the primitives differ there by contract); (b) the healthy plans of a
sweep against `Plan.run` alone — among them a humanoidtrack demo sweep, the one way to the rollout that accumulates the demo
log-density itself, held to the checker's plan as well; (c) the healthy episodes of a batch against `Plan.run_mpc` alone; (d) the healthy members of an
ensemble against plain plans, and the reduction of the device's own member rows against tests/ensemble_checker.py (synthetic
member rewards cannot be uploaded: mbd_plan_score_update takes combined rewards only); (e) zeros of either sign at the childless
links, where the confined exchange adds a +0.0f that the checker does not.  Comparisons
are by bit pattern (state_inputs.same_bits).  tests/test_containment_cases.py shows on the CPU that the cases diverge as claimed
and share the lanes they claim.

What the cases found with the kernels of the commit before this module: the halfcheetah's default launch, every filled planar
launch and the LPS 4 / 8 layouts of the 3-D kernel passed a diverged candidate on to the candidates sharing its 16-lane DPP
row (the exchange discarded the neighbour's lanes by a product with a 0/1 mask: NaN * 0 = NaN), and so did a sweep whose plan
size is no multiple of the candidates per row."""

import numpy as np
import pytest

import containment_inputs as ci
import ensemble_checker as ec
from state_inputs import same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(lib):
    from mbd_hip import _capi
    if _capi.device_count() < 1:
        pytest.fail("tests/test_gpu_containment.py needs a GPU")
    return _capi


def _state(s):
    from mbd_hip.envs.base import State
    return State(np.asarray(s, np.float32), None, np.float32(0.0), np.float32(0.0), {})


def _env(name, m):
    from mbd_hip.envs.base import RigidBodyEnv
    return RigidBodyEnv(name, model=m)


def _rollout(env, s0, us):
    """(rewards [B][H], tracked positions or None, final states [B][...]) of env.rollout as numpy arrays."""
    want = env.xref is not None
    out = env.rollout(_state(s0), us, want_xpos=want, want_final=True)
    return out[0].cpu().numpy(), (out[1].cpu().numpy() if want else None), out[-1].cpu().numpy()


# ---- (a) env.rollout ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kernel", ci.rollout_matrix())
def test_a_diverged_candidate_stays_alone(gpu, levers, name, kernel):
    ref = ci.reference(name)
    levers(**ci.KERNELS[kernel])
    choice = gpu.debug_rollout_choice(ref["model"].to_struct(), 256, ref["B"], ci.H)
    if kernel == "pk2":
        assert "pk2" in choice["name"]
    if kernel == "no_unit":
        assert "rtib" in choice["name"]
    env = _env(ref["env_name"], ref["model"])
    B, us, s0 = ref["B"], ref["us"], ref["s0"]
    twins = _rollout(env, s0, us)  # the launch with every candidate healthy
    for what, got, want in zip(("rewards", "tracked positions", "final states"), twins, ref["twin"]):
        if got is not None:
            same_bits(got, want, f"{name} [{kernel}] all healthy: {what}")
    for pattern in ci.PATTERNS:
        mask = ci.poisoned(pattern, B, ref["lps"])
        got = _rollout(env, s0, ci.poison_actions(us, mask))
        want = ci.expected(ref, mask)
        tag = f"{name} [{kernel}] {pattern} ({choice['name'].split('(')[0]}, cpw {choice['cpw']})"
        for what, g, w, t in zip(("rewards", "tracked positions", "final states"), got, want, twins):
            if g is None:
                continue
            g, w, t = (np.asarray(x).reshape(B, -1) for x in (g, w, t))
            same_bits(g[~mask], w[~mask], f"{tag}: healthy candidates' {what} against the checker")
            same_bits(g[~mask], t[~mask], f"{tag}: healthy candidates' {what} against the launch of their healthy twins")
            if what != "final states":  # the rows before the poison
                per_row = g.shape[1] // ci.H
                same_bits(g[mask][:, :ci.T0 * per_row], w[mask][:, :ci.T0 * per_row], f"{tag}: poisoned candidates' {what} before T0")
            if what != "tracked positions":  # never hidden
                hidden = ~np.isfinite(w[mask]) & np.isfinite(g[mask])
                assert not hidden.any(), f"{tag}: {int(hidden.sum())} non-finite {what} of the checker are finite on the device"


# ---- (b) sweeps -----------------------------------------------------------------------------------------------------------------
def _args(name, N, H=ci.SWEEP_H, Nd=ci.SWEEP_ND, demo=False):
    from mbd_hip.planners.mbd_planner import Args
    return Args(env_name=name, Nsample=N, Hsample=H, Ndiffuse=Nd, temp_sample=0.1, enable_demo=demo, disable_recommended_params=True,
                not_render=True)


def _start_states(gpu, env, P, poisoned_plan=1):
    """P reset states (different seeds), plan `poisoned_plan`'s with the root spinning at 3e38 rad/s."""
    sts = [env.reset(gpu.prng_key(20 + k)) for k in range(P)]
    if poisoned_plan is not None:
        s = np.asarray(sts[poisoned_plan].pipeline_state, np.float32)
        sts[poisoned_plan] = _state(ci.poison_state(s.reshape(-1, 13)).reshape(s.shape))
    return sts


def _sweep_against_plans(gpu, env, args, update_method=0, sts=None):
    from mbd_hip.planners.mbd_planner import Plan, Sweep
    P = ci.SWEEP_P
    sts = _start_states(gpu, env, P) if sts is None else sts
    keys = np.stack([gpu.prng_key(40 + k) for k in range(P)])
    sw = Sweep(env, args, P, update_method=update_method)
    for k in range(P):
        sw.set_state0(k, sts[k])
    mu, rm, rf, _ = sw.run(keys)
    sw.close()
    for k in (0, 2):
        plan = Plan(env, args, update_method=update_method)
        plan.set_state0(sts[k])
        mu1, rm1, rf1, _ = plan.run(keys[k])
        plan.close()
        assert np.isfinite(mu1).all() and np.isfinite(rm1).all()
        same_bits(mu[k], mu1, f"plan {k}: mu_0ts")
        same_bits(rm[k], rm1, f"plan {k}: rew_means")
        same_bits(rf[k], np.float32(rf1), f"plan {k}: rew_final")
    return mu, rm, rf


@pytest.mark.parametrize("name,kernel,N,claim", ci.SWEEPS)
def test_a_diverged_plan_of_a_sweep_stays_alone(gpu, levers, name, kernel, N, claim):
    from mbd_hip.envs import get_env
    levers(**ci.KERNELS[kernel])
    mu, rm, rf = _sweep_against_plans(gpu, get_env(name), _args(name, N))
    assert not np.isfinite(rm[1]).any(), "plan 1 starts from the diverging state: its mean rewards are not finite"


def test_a_diverged_plan_of_a_demo_sweep_leaves_the_fused_log_density_alone(gpu, orc):
    """The instantiation that accumulates the demo log-density in the rollout itself (RolloutParams::lp, mbd_hot3d.hip) next to a
    diverged neighbour.  No env.rollout reaches it (it needs the demo's 50 rows, an env with the demo and a plan that asks for
    the density; tests/test_containment_cases.py asserts both), so: a humanoidtrack demo sweep, plan 1 from the diverging
    state.  The log-densities enter every weight, so a healthy plan's means carry them: plans 0 and 2 equal `Plan.run` alone,
    and plan 0 equals the CHECKER's plan — its rollouts, its eval_xref_logpd of their tracked positions, its score — step by
    step from the same key."""
    from mbd_hip.envs import get_env
    from oracle import planner as op
    name, N, H, Nd = ci.DEMO_SWEEP
    env = get_env(name)
    choice = gpu.debug_rollout_choice(env.sys.to_struct(), 256, ci.SWEEP_P * N, H, sweep_plan_N=N, has_xref=True)
    assert choice["fuses_logpd"], choice
    sts = _start_states(gpu, env, ci.SWEEP_P)
    mu, rm, rf = _sweep_against_plans(gpu, env, _args(name, N, H, Nd, demo=True), sts=sts)
    assert not np.isfinite(rm[1]).any(), "plan 1 starts from the diverging state: its mean rewards are not finite"
    oenv = op.OracleEnv(orc, name, env.sys.to_struct(), xref=env.xref, rew_xref=env.rew_xref, init_q=env.sys.init_q)
    s0 = np.asarray(sts[0].pipeline_state, np.float32).reshape(-1, 13)
    sched = orc.schedule(1e-4, 1e-2, Nd)
    r, Ybar = gpu.prng_key(40), np.zeros((H, env.action_size), np.float32)
    for step, i in enumerate(range(Nd - 1, 0, -1)):
        r, Ybar, mean, det = op.reverse_once(orc, oenv, s0, i, r, Ybar, sched, N, H, 0.1, 1, enable_demo=True)
        assert np.isfinite(det["lp"]).all()
        same_bits(mu[0][step], Ybar, f"plan 0, step {step}: mu_0ts against the checker's plan")
        same_bits(rm[0][step], np.float32(mean), f"plan 0, step {step}: rew_means against the checker's plan")


def test_a_diverged_plan_of_a_cem_sweep_stays_alone_and_goes_on(gpu):
    """The path-integral baseline cem ranks NaN last and goes on: the poisoned plan's mean stays finite — every
    reward of its candidates is non-finite, the selection takes candidates N-1 ... N-10 — and its neighbours keep their bits."""
    from mbd_hip.envs import get_env
    from mbd_hip.planners.path_integral import Args
    a = Args(env_name="halfcheetah", Nsample=33, Hsample=ci.SWEEP_H, Nrefine=ci.SWEEP_ND, temp_sample=0.1,
             disable_recommended_params=True, update_method="cem")
    mu, rm, rf = _sweep_against_plans(gpu, get_env("halfcheetah"), a, update_method=3)
    assert np.isfinite(mu[1]).all()
    assert not np.isfinite(rm[1]).any()


# ---- (c) batched episodes -------------------------------------------------------------------------------------------------------
_LOGS = ("actions", "rewards", "states", "means")


def _episodes_against_plans(env, args, sts, keys, T=3, K=2, shape=None, plant=None):
    from mbd_hip.planners.mbd_planner import Plan, Sweep
    P = ci.SWEEP_P
    sw = Sweep(env, args, P)
    for k in range(P):
        sw.set_state0(k, sts[k])
    if shape is not None:
        sw.set_noise_shape(shape)
    if plant is not None:
        sw.set_mpc_plant(1, **plant)
    got = sw.run_mpc(keys, T, K)
    sw.close()
    for k in (0, 2):
        plan = Plan(env, args)
        plan.set_state0(sts[k])
        if shape is not None:
            plan.set_noise_shape(shape)
        one = plan.run_mpc(keys[k], T, K)
        plan.close()
        for f in _LOGS:
            assert np.isfinite(one[f]).all(), f"episode {k} alone: {f}"
            same_bits(got[f][k], one[f], f"episode {k}: {f}")
    return got


@pytest.mark.parametrize("name", ["halfcheetah", "hopper"])
def test_an_episode_that_starts_diverging_stays_alone(gpu, name):
    from mbd_hip.envs import get_env
    env = get_env(name)
    keys = np.stack([gpu.prng_key(60 + k) for k in range(ci.SWEEP_P)])
    got = _episodes_against_plans(env, _args(name, 33), _start_states(gpu, env, ci.SWEEP_P), keys)
    assert not np.isfinite(got["rewards"][1]).any() and not np.isfinite(got["states"][1][1:]).all(axis=1).any()


@pytest.mark.parametrize("name", ["halfcheetah", "hopper"])
def test_an_episode_whose_plant_diverges_stays_alone(gpu, name):
    """The three episodes plan and execute on the model with the 1e30 gear; a noise shape of 0 on that actuator keeps every
    candidate and every mean at exactly 0 there (the gear is never felt), and episode 1's plant record adds normal noise to the
    EXECUTED actions (act_std > 0): its executed step diverges, in the one launch that executes all three episodes' rows."""
    pm = ci.poison_model(ci.model(name)[0])
    env = _env(name, pm)
    shape = np.ones((ci.SWEEP_H, env.action_size), np.float32)
    shape[:, 0] = 0.0
    keys = np.stack([gpu.prng_key(70 + k) for k in range(ci.SWEEP_P)])
    sts = _start_states(gpu, env, ci.SWEEP_P, poisoned_plan=None)
    got = _episodes_against_plans(env, _args(name, 33), sts, keys, shape=shape, plant=dict(env=None, key=gpu.prng_key(7), act_std=0.25))
    assert got["actions"][1][0, 0] != 0.0 and np.isfinite(got["actions"][1][0]).all()
    assert not np.isfinite(got["states"][1][1]).all(), "episode 1's first executed step must diverge"


# ---- (d) ensembles --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("risk", ["mean", "min"])
@pytest.mark.parametrize("name,N", [("hopper", 33), ("humanoidrun", 33), ("hopper", 32), ("humanoidrun", 32)])
@pytest.mark.parametrize("bad", [0, 1, 2])
def test_a_diverged_member_of_an_ensemble_is_the_worst_case_and_stays_alone(gpu, orc, name, N, risk, bad):
    """(N = 33: one launch per member; N = 32: the three members in ONE launch, wavefront by wavefront.)
    M = 3, member `bad` (the first, the middle or the last one — in the first, a reduction that starts from member 0 and
    keeps the smaller by `b < a ? b : a` would hide the NaN) with the 1e30 gear (the plan's candidates are not 0 in that column:
    every one of its rollouts diverges).  The other two: the rewards of plain rollouts of the peeked candidates on their
    models; member `bad`: non-finite; the combined
    rewards: tests/ensemble_checker.combine of the device's own member rows (NaN where it says NaN, bits elsewhere)."""
    from mbd_hip.envs import get_env
    from mbd_hip.planners.mbd_planner import Plan
    env = get_env(name)
    m = ci.model(name)[0]
    members = [None, _env(name, env.sys.scaled(mass=1.25, friction=0.7, gear=0.9))]
    members.insert(bad, _env(name, ci.poison_model(m)))
    H, Nd = ci.SWEEP_H, 3
    st = env.reset(gpu.prng_key(11))
    plan = Plan(env, _args(name, N, H, Nd))
    plan.set_state0(st)
    plan.set_ensemble(members, risk)
    plan.run(gpu.prng_key(12))
    Y0s, _, _ = plan.peek()
    r_m, rews = plan.peek_ensemble()
    plan.close()
    assert (Y0s[:, :, 0] != 0).any(axis=1).all()
    for k in sorted({0, 1, 2} - {bad}):
        alone = (env if members[k] is None else members[k]).rollout(st, Y0s).cpu().numpy()
        same_bits(r_m[k], ec.op.mean_h(orc, alone), f"{name} {risk}: member {k}")
        assert np.isfinite(r_m[k]).all()
    assert not np.isfinite(r_m[bad]).any(), "the poisoned member diverges under every candidate"
    want = ec.combine(r_m, risk)
    assert np.array_equal(np.isnan(rews), np.isnan(want))
    same_bits(rews[~np.isnan(want)], want[~np.isnan(want)], f"{name} {risk}: the combined rewards")
    assert not np.isfinite(rews).any(), "a diverged member is the worst case, never hidden"


# ---- the sign of a zero ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kernel", ci.ZERO_SIGN_MODELS)
def test_a_childless_link_whose_own_share_is_a_negative_zero(gpu, orc, levers, name, kernel):
    """containment_inputs.zero_sign_cases: the confined exchange adds +0.0f for a child slot a link does not have (the
    checker adds nothing), which turns an own contribution of -0.0f into +0.0f; rewards and final states must still be the
    checker's bit for bit, signs of zeros included, in the layouts with several candidates per row."""
    levers(**ci.KERNELS[kernel])
    m, env_name = ci.model(name)
    env = _env(env_name, m)
    for tag, s, us in ci.zero_sign_cases(orc, m):
        want = orc.rollout(m.to_struct(), s, us, want_final=True)
        got = env.rollout(_state(s), us, want_final=True)
        same_bits(got[0].cpu().numpy(), want[0], f"{name} [{kernel}] {tag}: rewards")
        same_bits(got[-1].cpu().numpy().reshape(want[-1].shape), want[-1], f"{name} [{kernel}] {tag}: final states")
