"""What tests/test_gpu_sweep_elites.py and tests/test_gpu_sweep_togo.py share: a sweep under a record beside the plans it must
equal, each plan created from the sweep's config with temps[k], holding the same records, run with keys[k] from state k; and the
comparisons of the records' peek outputs.  Every comparison is by bit pattern.  The expected values are the single ``Plan``'s, which
tests/test_gpu_elites.py and tests/test_gpu_togo.py hold to the numpy checkers; the batch code is never its own reference."""
import numpy as np

from state_inputs import same_bits

NAME, N, H, ND = "hopper", 80, 50, 4      # sweeps equal their plans alone
E3N = dict(n_elites=3, nominal=True)      # the record `e3n` of tests/elites_inputs.py
TOGO = dict(block=10, min_tail=5)         # at H = 50: G = 5 groups
EP = dict(name="cartpole", N=64, Nd=5, T=3, K=2, E=1, P=3)
SIGMA = dict(cold=1.0, warm=0.5)
_OUT = ("actions", "rewards", "states", "means")


def args(name, n, h, nd):
    from mbd_hip.planners.mpc import MpcArgs
    return MpcArgs(env_name=name, Nsample=n, Hsample=h, Ndiffuse=nd, temp_sample=0.1, disable_recommended_params=True, not_render=True)


def inputs(gpu, env, P):
    """(start states, keys [P, 2], temps): distinct per plan."""
    states = [env.reset(gpu.prng_key(20 + k)) for k in range(P)]
    keys = np.stack([gpu.prng_key(40 + k) for k in range(P)])
    temps = [0.1 * (1 + k % 3) + 0.01 * k for k in range(P)]
    return states, keys, temps


def make_sweep(env, a, P, states, temps, method, configure):
    from mbd_hip.planners.mbd_planner import Sweep
    sw = Sweep(env, a, P, temps=temps, update_method=method)
    for k in range(P):
        sw.set_state0(k, states[k])
    configure(sw)
    return sw


def make_plan(env, a, state, temp, method, configure):
    from dataclasses import replace

    from mbd_hip.planners.mbd_planner import Plan
    plan = Plan(env, replace(a, temp_sample=float(np.float32(temp))), update_method=method)
    plan.set_state0(state)
    configure(plan)
    return plan


def same_elites(got, ref, what):
    assert got["count"] == ref["count"] and got["steps"] == ref["steps"], f"{what}: count {got['count']} / {ref['count']}, steps {got['steps']} / {ref['steps']}"
    assert list(got["src"]) == list(ref["src"]), f"{what}: src"
    for k in ("E", "R", "log_top"):
        same_bits(got[k], ref[k], f"{what}: {k}")
    for k in ("log_count", "log_kept"):
        assert np.array_equal(got[k], ref[k]), f"{what}: {k}"


def same_togo(got, ref, what):
    assert np.array_equal(got["starts"], ref["starts"]), f"{what}: starts"
    for k in ("R", "W"):
        same_bits(got[k], ref[k], f"{what}: {k}")


def same_records(sw, k, plan, what):
    if plan.has_elites:
        same_elites(sw.peek_elites(k), plan.peek_elites(), what)
    if plan.has_togo:
        same_togo(sw.peek_togo(k), plan.peek_togo(), what)


def run_equals_plans(gpu, env, a, P, method, configure, what, skip=()):
    """``Sweep.run`` under ``configure`` against ``Plan.run`` per plan: means, mean rewards and the records' peeks."""
    states, keys, temps = inputs(gpu, env, P)
    sw = make_sweep(env, a, P, states, temps, method, configure)
    try:
        mu, rm = sw.run(keys)[:2]
        for k in range(P):
            if k in skip:
                continue
            plan = make_plan(env, a, states[k], temps[k], method, configure)
            try:
                pmu, prm = plan.run(keys[k])[:2]
                same_bits(mu[k], pmu, f"{what}: plan {k}: mu_0ts")
                same_bits(rm[k], prm, f"{what}: plan {k}: mean rewards")
                same_records(sw, k, plan, f"{what}: plan {k}")
            finally:
                plan.close()
    finally:
        sw.close()


def same_episode(out, k, ep, what):
    for name in _OUT:
        same_bits(out[name][k], ep[name], f"{what}: episode {k}: {name}")
