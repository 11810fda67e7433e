"""The checker's restatement of the pick record (include/mbd_hip.h mbd_mpc_pick, DESIGN.md section 1 "N15 pick") in numpy, on the
existing building blocks: oracle.planner.reverse_once for the diffusion steps and mean_h for a rollout's return, mpc_checker.shift
and mpc_checker.execute for the boundary, objective_checker.ObjectiveEnv for an objective record, mpc_delay_checker.queue_of for a
delay record, mpc_pi_checker.plan_tick and next_sigma for the path-integral methods, and any stand-in for reverse_once
(weighting_checker's for a weighting record)."""
from __future__ import annotations

import numpy as np

from mpc_checker import execute, shift
from oracle import planner as op

f32 = np.float32
MEAN, PREV, BEST = 1, 2, 4


def best_index(rews) -> int:
    """n*: the lowest index among the maxima of the finite entries (+0 and -0 tie), -1 when none is finite."""
    r = np.asarray(rews, f32)
    ok = np.isfinite(r)
    if not ok.any():
        return -1
    m = r[ok].max()
    return int(np.flatnonzero(ok & (r == m))[0])


def choose(rets, mask, present) -> int:
    """The contract's choice among the three slots: enabled, present, finite, strictly greater takes over; none: 0."""
    c = -1
    for k in range(3):
        if (mask >> k) & 1 and present[k] and np.isfinite(rets[k]) and (c < 0 or rets[k] > rets[c]):
            c = k
    return max(c, 0)


def pick(oenv, s, M, B, cold, rews, Y0s, mask):
    """One tick's pick: (P_t, choice, rets [3], best, slots [3, H, Nu]) from the tick's result M, the Ybar B it started from,
    the rewards and candidates of its last step, evaluated on ``oenv`` from ``s``."""
    best = best_index(rews)
    slots = np.stack([M, M if cold else B, M if best < 0 else Y0s[best]]).astype(f32)
    rets = op.mean_h(oenv.orc, np.ascontiguousarray(oenv.rollout(s, slots), f32))
    c = choose(rets, mask, (True, not cold, best >= 0))
    return slots[c].copy(), c, rets, best, slots


def episode(oenv, state0, key, N, H, Nd, temp, T, K, E, mask, impl=1, plant=None, reset_at=(), objective=None, D=0, rows0=None,
            method=None, sigma=(1.0, 1.0, 0.0), reverse_once=None, beta0=1e-4, betaT=1e-2):
    """mpc_checker.episode with a pick record of ``mask`` (None: no record — the picked plan is the mean and nothing is logged).
    ``plant``: the env that executes the rows (the pick evaluates on ``oenv``, the planner's model).  ``reset_at``: ticks whose
    plan is a cold one (a session's reset_mean).  ``objective``: an objective_checker.Record — the steps and the pick then see the
    shaped returns, the pick's with the tick's previous action, and the next tick's previous action is clip(P_t[E-1]): it follows
    the pick.  ``D`` > 0: a delay record (mpc_delay_checker.queue_of; ``rows0`` as there) — the tick plans, and the pick evaluates,
    from the state the plan's env predicts the committed queue reaches; the rows executed are the queue's head and P_t[:E] joins its
    tail.  ``method``: "mppi", "cma-es" or "cem" under a sigma record ``sigma`` = (cold, warm, gain) — mpc_pi_checker.plan_tick for
    the refinements, slot 2 a row of the last refinement's materialised candidates, mpc_pi_checker.next_sigma across the boundary.
    ``reverse_once``: a stand-in for oracle.planner.reverse_once with its signature (a weighting record: functools.partial(
    weighting_checker.reverse_once, rec=...)); ``oenv`` may be noise_shape_checker.shaped_env's.  Returns dict(actions, rewards,
    states, means, choice [T], rets [T, 3], best [T], slot1 [T, H, Nu], last_rews [T, N]; predicted [T, S] with a delay)."""
    import mpc_pi_checker as pic
    from mpc_delay_checker import queue_of
    orc = oenv.orc
    Nu = oenv.Nu
    penv = oenv  # the plan's env as it is: the prediction of a delay record runs on it
    plant = oenv if plant is None else plant
    step = reverse_once or op.reverse_once
    if objective is not None:  # (the planner's env returns ret - cost; the rows run on the env itself)
        import objective_checker as oc
        oenv = oc.ObjectiveEnv(oenv, objective)
    sched = orc.schedule(beta0, betaT, Nd)
    rng = np.asarray(key, np.uint32)
    s = np.ascontiguousarray(state0, f32).reshape(-1)
    C = queue_of(rows0, D, E, Nu) if D > 0 else None
    Ybar, cold, sig = np.zeros((H, Nu), f32), True, f32(sigma[0])
    out = {k: [] for k in ("actions", "rewards", "means", "choice", "rets", "best", "slot1", "last_rews", "predicted")}
    states = [s]
    for t in range(T):
        if t in reset_at:
            Ybar, cold, sig = np.zeros((H, Nu), f32), True, f32(sigma[0])
        keys = orc.split(rng, 2, impl)
        rng, r = keys[0], keys[1]
        s_plan = s
        if D > 0:
            _, s_plan = execute(penv, s, C.reshape(D * E, Nu))
            s_plan = np.asarray(s_plan, f32).reshape(-1)
            out["predicted"].append(s_plan)
        B, d = Ybar, {}
        n_it = Nd - 1 if cold else K
        if method is None:
            for i in range(n_it, 0, -1):
                r, Ybar, _, d = step(orc, oenv, s_plan, i, r, Ybar, sched, N, H, temp, impl)
        else:  # (the update rule is mpc_pi_checker's own; the stand-in only looks at what the last refinement was handed)
            def upd(orc_, m, rews, Y0s, mu, sg, T0):
                d.update(rews=np.asarray(rews, f32), Y0s=Y0s)
                return pic.orc_update(orc_, m, rews, Y0s, mu, sg, T0)
            _, Ybar, sig_end = pic.plan_tick(oenv, s_plan, r, Ybar, sig, n_it, N, H, temp, method, impl, update=upd)
            sig = pic.next_sigma(sig_end, *sigma)
        M = Ybar
        if mask is not None:
            M, c, rets, best, slots = pick(oenv, s_plan, M, B, cold, d["rews"], d["Y0s"], mask)
            out["choice"].append(c)
            out["rets"].append(rets)
            out["best"].append(best)
            out["slot1"].append(slots[1])
        out["last_rews"].append(np.asarray(d["rews"], f32))
        if objective is not None:
            oenv.prev.value = oc.clip(M[E - 1])
        rows = np.array(C[0] if D > 0 else M[:E], f32)
        rew, s = execute(plant, s, rows)
        s = np.asarray(s, f32).reshape(-1)
        out["actions"].append(rows)
        out["rewards"].append(rew)
        out["means"].append(M)
        states.append(s)
        if D > 0:
            C = np.concatenate([C[1:], M[:E][None]]).astype(f32)
        Ybar, cold = shift(M, E), False
    res = dict(actions=np.concatenate(out["actions"]), rewards=np.concatenate(out["rewards"]), states=np.stack(states),
               means=np.stack(out["means"]), last_rews=np.stack(out["last_rews"]))
    if mask is not None:
        res.update(choice=np.array(out["choice"], np.int32), rets=np.stack(out["rets"]).astype(f32),
                   best=np.array(out["best"], np.int32), slot1=np.stack(out["slot1"]))
    if D > 0:
        res["predicted"] = np.stack(out["predicted"])
    return res
