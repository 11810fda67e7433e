"""The checker's restatement of the elite record (include/mbd_hip.h mbd_elites, DESIGN.md section 1 "N18 elites") in numpy float32,
every operation spelled out and rounded: how a diffusion step overwrites its first candidates with the step's mean and the elites
the previous step left (``State.inject``), and how it takes its own best candidates over (``State.select``).  There is no sum in
either: the selection is a sort of the finite rewards by (descending value, ascending index) — Python's, not the kernels' rounds —
and gathers.

``State`` is the elites as a plan carries them through runs, ticks and sessions; ``ElitesOracle`` wraps an oracle — the plain one, a
noise_shape_checker.ShapedOracle, a noise_basis_checker.BasisOracle, an adapt_checker.AdaptOracle — so that ``sample`` injects behind
the inner sampler; ``reverse_once`` and ``plan_tick`` are weighting_checker's with the selection (and, with ``adapt``, an adapt
record's update) behind them, so that ``run``, ``pi_run``, ``episode`` and the sessions of the existing checkers run on top."""
from __future__ import annotations

import copy
from dataclasses import dataclass

import numpy as np

import weighting_checker as wc

f32 = np.float32
QNAN = np.array([0x7fc00000], np.uint32).view(f32)[0]
MAX_ELITES = 32


@dataclass(frozen=True)
class Record:
    """mbd_elites."""
    n_elites: int = 3
    nominal: bool = True
    carry: bool = False

    def kwargs(self):
        return dict(n_elites=self.n_elites, nominal=self.nominal, carry=self.carry)


def finite(r):
    """pick_finite: the exponent bits are not all ones."""
    return (np.ascontiguousarray(r, f32).view(np.uint32) & np.uint32(0x7f800000)) != np.uint32(0x7f800000)


def before(v, i, bv, bi) -> bool:
    """pick_before on two present entries: the larger value, among equal values (+0 == -0) the lower index."""
    return bool(v > bv or (v == bv and i < bi))


def order(rews, k):
    """The first k finite entries of ``rews`` in the order: a list of indices."""
    r = np.ascontiguousarray(rews, f32).reshape(-1)
    idx = [int(i) for i in np.flatnonzero(finite(r))]
    idx.sort(key=lambda i: (-float(r[i]), i))  # (-(-0.0) == 0.0 == -(+0.0): the zeros tie, the index decides)
    return idx[:max(int(k), 0)]


def clip(y):
    with np.errstate(all="ignore"):
        return np.ascontiguousarray(np.clip(np.asarray(y, f32), f32(-1), f32(1)), f32)


def values(z, sigma, ybar):
    """What the consumers of a lazy plan's normals form: clip((z * sigma) + Ybar, -1, 1), two roundings."""
    with np.errstate(all="ignore"):
        y = (np.asarray(z, f32) * f32(sigma)).astype(f32)
        return clip((y + np.asarray(ybar, f32).reshape(1, -1)).astype(f32))


class State:
    """The elites as a plan carries them.  ``lazy``: the plan keeps normals, not candidates (the MBD update on a rigid-body env).
    ``g``: the shape the steps' samplers are handed — None, an array [HNu], or a callable that returns one of the two at the time
    of the step (an adapt record's G).  ``E`` [count, HNu], ``R``, ``src``; ``log``: one (count', kept, top) per selection;
    ``steps``: per step dict(slots, src, R, E) — what the step injected into and selected."""

    def __init__(self, rec: Record, H, Nu, lazy, g=None):
        assert 0 <= rec.n_elites <= MAX_ELITES and rec.n_elites + int(rec.nominal) > 0
        self.rec, self.H, self.Nu, self.lazy, self.g = rec, H, Nu, bool(lazy), g
        self.log, self.steps = [], []
        self.slots = 0
        self.reset()

    def reset(self):
        """count = 0: the set call, a run, a cold tick, reset_mean, a tick without carry."""
        self.E = np.zeros((0, self.H * self.Nu), f32)
        self.R, self.src = np.zeros(0, f32), np.zeros(0, np.int32)

    @property
    def count(self):
        return self.E.shape[0]

    def shape(self):
        g = self.g() if callable(self.g) else self.g
        return None if g is None else np.ascontiguousarray(g, f32).reshape(-1)

    def tick(self, cold, E_steps):
        """The launch in front of a tick's first step."""
        if cold or not self.rec.carry:
            self.reset()
            return
        sh = E_steps * self.Nu
        if self.count:
            self.E = np.concatenate([self.E[:, sh:], np.zeros((self.count, sh), f32)], axis=1).astype(f32)

    def inject(self, Y0s, z, ybar, sigma):
        """(Y0s', z') [N, HNu] behind the injection into the sampler's candidates and normals."""
        N = np.shape(Y0s)[0]
        Y = np.ascontiguousarray(Y0s, f32).reshape(N, -1).copy()
        zz = np.ascontiguousarray(z, f32).reshape(N, -1).copy()
        yb = np.asarray(ybar, f32).reshape(-1)
        nom, cnt = int(self.rec.nominal), self.count
        slots = nom + cnt
        assert slots < N
        if self.lazy:
            g = self.shape()
            if nom:
                zz[0] = f32(0)
            with np.errstate(all="ignore"):
                for j in range(cnt):
                    q = ((self.E[j] - yb).astype(f32) / f32(sigma)).astype(f32)
                    zz[nom + j] = q if g is None else np.where(g == 0, f32(0), q).astype(f32)
            Y[:slots] = values(zz[:slots], sigma, yb)
        else:  # (a materialised plan keeps no normals: the rows' z is left as drawn and means nothing)
            if nom:
                Y[0] = clip(yb)
            Y[nom:slots] = self.E
        self.slots = slots
        return Y, zz

    def select(self, rews, Y0s):
        """The selection over the rewards the score read and the candidates as mbd_plan_peek forms them; the log entry."""
        Y = np.ascontiguousarray(Y0s, f32).reshape(np.shape(Y0s)[0], -1)
        r = np.ascontiguousarray(rews, f32).reshape(-1)
        src = order(r, self.rec.n_elites)
        self.src = np.array(src, np.int32)
        self.R = r[src].astype(f32) if src else np.zeros(0, f32)
        self.E = Y[src].copy() if src else np.zeros((0, Y.shape[1]), f32)
        entry = (len(src), int(sum(1 for i in src if i < self.slots)), self.R[0] if src else QNAN)
        self.log.append(entry)
        self.steps.append(dict(slots=self.slots, src=self.src.copy(), R=self.R.copy(), E=self.E.copy(), rews=r.copy()))
        return entry


def step(rews, cand, ybar, sigma, lazy, g, rec: Record, E_in=None):
    """One step on given arrays, as mbd_debug_elites_host takes them: ``cand`` [N, HNu] values, or with ``lazy`` normals; ``E_in``
    [count, HNu] the elites the step finds.  dict(cand [N, HNu] behind the injection, E, R, src, count, kept, top)."""
    cand = np.ascontiguousarray(cand, f32)
    N, HNu = cand.shape
    st = State(rec, 1, HNu, lazy, g)
    if E_in is not None and len(E_in):
        st.E = np.ascontiguousarray(E_in, f32).reshape(-1, HNu)
    if lazy:
        Y, z = st.inject(values(cand, sigma, ybar), cand, ybar, sigma)
        Y = values(z, sigma, ybar)  # (every row as the consumers form it from the normals behind the injection)
        out = z
    else:
        Y, _ = st.inject(cand, cand, ybar, sigma)
        out = Y
    count, kept, top = st.select(rews, Y)
    return dict(cand=out, E=st.E, R=st.R, src=st.src, count=count, kept=kept, top=top)


class ElitesOracle:
    """An oracle whose ``sample`` injects the state's rows behind the inner sampler; everything else is the oracle's."""

    def __init__(self, orc, state: State):
        self._orc, self.state = orc, state

    def __getattr__(self, name):
        return getattr(self._orc, name)

    def sample(self, key, impl, N, H, Nu, begin, count, sigma, Ybar, want_eps=False):
        assert begin == 0 and count == N, "an elite record's plans are unsharded"
        Y0s, z = self._orc.sample(key, impl, N, H, Nu, begin, count, sigma, Ybar, want_eps=True)
        Y, zz = self.state.inject(Y0s, z, Ybar, sigma)
        Y, zz = Y.reshape(N, H, Nu), zz.reshape(N, H, Nu)
        return (Y, zz) if want_eps else Y


def elites_env(oenv, state: State):
    """A copy of the env whose ``orc`` injects the state's rows."""
    e = copy.copy(oenv)
    e.orc = ElitesOracle(oenv.orc, state)
    return e


def _inner(orc, state: State, adapt):
    """The oracle the injection stands behind: ``orc`` itself, or under an adapt record its sampler, whose G is the shape."""
    if adapt is None:
        return orc
    import adapt_checker as ac
    state.g = adapt.G  # (the table the step samples under: the update behind the step replaces it)
    return ac.AdaptOracle(getattr(orc, "_orc", orc), adapt)


def reverse_once(orc, env, state0, i, rng, Ybar_i, sched, N, H, T0, impl=1, enable_demo=False, literal=True, timers=None, *,
                 state: State, rec: wc.Record = wc.Record(reject_nonfinite=False), log=None, adapt=None):
    """weighting_checker.reverse_once (the score without a record where ``rec`` is its default) with the injection behind the
    sampler and the selection behind the update.  ``adapt``: an adapt_checker.State — the step then samples under its table and
    updates it as well.  ``functools.partial(reverse_once, state=...)`` stands wherever a checker takes a ``reverse_once``."""
    out = wc.reverse_once(ElitesOracle(_inner(orc, state, adapt), state), env, state0, i, rng, Ybar_i, sched, N, H, T0, impl,
                          enable_demo, literal, timers, rec=rec, log=log)
    d = out[3]
    if adapt is not None:
        adapt.step(getattr(orc, "_orc", orc), d["weights"], d["Y0s"], Ybar_i, f32(sched[2][i]))
    state.select(d["rews"], d["Y0s"])
    return out


def run(orc, env, state0, key, N, H, Nd, T0, state: State, rec: wc.Record = wc.Record(reject_nonfinite=False), impl=1, beta0=1e-4,
        betaT=1e-2, adapt=None):
    """mbd_plan_run's loop under the record: dict(mu_0ts, rew_means, log (a weighting record's), details (every step's))."""
    sched = orc.schedule(beta0, betaT, Nd)
    state.reset()
    if adapt is not None:
        adapt.reset()
    r, Ybar = np.asarray(key, np.uint32), np.zeros((H, env.Nu), f32)
    mus, rms, log, details = [], [], [], []
    for i in range(Nd - 1, 0, -1):
        r, Ybar, rm, d = reverse_once(orc, env, state0, i, r, Ybar, sched, N, H, T0, impl, state=state, rec=rec, log=log, adapt=adapt)
        mus.append(Ybar)
        rms.append(rm)
        details.append(d)
    return dict(mu_0ts=np.stack(mus), rew_means=np.array(rms, f32), log=log, details=details)


def plan_tick(oenv, s_plan, r, mu, sigma, n_it, N, H, temp, method, impl=1, *, state: State,
              rec: wc.Record = wc.Record(reject_nonfinite=False), log=None, adapt=None, details=None):
    """mpc_pi_checker.plan_tick for an mppi plan with the injection behind every refinement's sampler and the selection behind its
    update (the candidates are materialised: no sigma enters either)."""
    import mpc_pi_checker as pic
    base = getattr(oenv.orc, "_orc", oenv.orc) if adapt is not None else oenv.orc
    env = copy.copy(oenv)

    class _Orc(ElitesOracle):
        def sample(self, *a, **kw):  # (the inner sampler is looked up at every refinement: an adapt record's table moves)
            self._orc = _inner(oenv.orc, state, adapt)
            return ElitesOracle.sample(self, *a, **kw)

    env.orc = _Orc(oenv.orc, state)

    def upd(orc, m, rews, Y0s, mu_t, sig, T0):
        res = wc.weigh(base, rews, T0, rec)
        if log is not None:
            log.append((res["temp"], res["ess"], res["kept"]))
        out = wc.pi_update(base, m, res, Y0s, mu_t, sig)
        if adapt is not None:
            adapt.step(base, res["weights"], Y0s, mu_t, f32(sig))
        state.select(rews, Y0s)
        if details is not None:
            details.append(dict(rews=np.asarray(rews, f32), Y0s=Y0s, weights=res["weights"]))
        return out

    return pic.plan_tick(env, s_plan, r, mu, sigma, n_it, N, H, temp, method, impl, update=upd)


def pi_run(oenv, state0, key, N, H, Nd, temp, method, state: State, impl=1, rec: wc.Record = wc.Record(reject_nonfinite=False),
           adapt=None):
    """mbd_plan_run of an mppi plan under the record: dict(mu_0ts [Nd-1, H, Nu], details)."""
    state.reset()
    if adapt is not None:
        adapt.reset()
    r, mu, sigma = np.asarray(key, np.uint32), np.zeros((H, oenv.Nu), f32), f32(1.0)
    mus, details = [], []
    for _ in range(Nd - 1):
        r, mu, sigma = plan_tick(oenv, state0, r, mu, sigma, 1, N, H, temp, method, impl, state=state, rec=rec, adapt=adapt,
                                 details=details)
        mus.append(mu)
    return dict(mu_0ts=np.stack(mus), details=details)


class Session:
    """mpc_online_checker.Session (an MBD plan's; ``method`` None) or mpc_pi_checker.Session (mppi under a sigma record) with the
    elites carried across ticks: in front of every tick the state's ``tick``, ``reset_mean`` empties them as well.  ``tick`` returns
    the inner session's dict plus ``elites`` [count, H, Nu], the elites behind the tick."""

    def __init__(self, oenv, key, N, H, Nd, temp, K, E, state: State, D=0, rows0=None, method=None, sigma=(1.0, 1.0, 0.0), impl=1,
                 rec: wc.Record = wc.Record(reject_nonfinite=False)):
        import functools

        import mpc_online_checker as online
        import mpc_pi_checker as pic
        self.state, self.E = state, E
        if method is None:
            self.inner = online.Session(oenv, key, N, H, Nd, temp, K, E, D, rows0, impl=impl,
                                        reverse_once=functools.partial(reverse_once, state=state, rec=rec))
        else:
            self.inner = pic.Session(oenv, key, N, H, Nd, temp, K, E, method, *sigma, impl=impl,
                                     plan_tick=functools.partial(plan_tick, state=state, rec=rec))
        self.cold = True
        state.reset()

    def reset_mean(self):
        self.inner.reset_mean()
        self.cold = True
        self.state.reset()

    def tick(self, x):
        self.state.tick(self.cold, self.E)
        out = dict(self.inner.tick(x))
        self.cold = False
        out["elites"] = self.state.E.reshape(-1, self.state.H, self.state.Nu).copy()
        return out


def episode(oenv, state0, key, N, H, Nd, temp, T, K, E, state: State, D=0, rows0=None, method=None, sigma=(1.0, 1.0, 0.0), impl=1,
            rec: wc.Record = wc.Record(reject_nonfinite=False), pick_mask=None, plant=None):
    """A closed-loop episode of T ticks under the record: the session above fed the states ``plant`` (None: the env itself) reaches
    by executing each tick's rows (the queue's head under a delay record).  ``pick_mask``: a pick record (mpc_pick_checker.pick on
    the tick's result; MBD plans without a delay) — its best candidate may be an elite.  Returns dict(actions, rewards, states,
    means, elites — per tick [count, H, Nu] —, picks — per tick (choice, best))."""
    import mpc_pick_checker as pk
    from mpc_checker import execute, shift
    sess = Session(oenv, key, N, H, Nd, temp, K, E, state, D, rows0, method, sigma, impl, rec)
    s = np.ascontiguousarray(state0, f32).reshape(-1)
    actions, rewards, states, means, elites, picks = [], [], [s], [], [], []
    if pick_mask is not None:
        assert method is None and D == 0
        last = {}
        inner_step = sess.inner.reverse_once

        def step_(*a, **kw):
            out = inner_step(*a, **kw)
            last.update(out[3])
            return out
        sess.inner.reverse_once = step_
    for t in range(T):
        cold = sess.cold
        B = sess.inner.Ybar if method is None else None
        o = sess.tick(s)
        M = o["mean"]
        if pick_mask is not None:
            M, c, _, best, _ = pk.pick(oenv, s, M, B, cold, last["rews"], last["Y0s"], pick_mask)
            picks.append((c, best))
            sess.inner.Ybar = shift(M, E)
        rows = np.array(o.get("head", o["rows"]) if pick_mask is None else M[:E], f32)
        rew, s = execute(oenv if plant is None else plant, s, rows)
        s = np.asarray(s, f32).reshape(-1)
        actions.append(rows)
        rewards.append(rew)
        states.append(s)
        means.append(M)
        elites.append(o["elites"])
    return dict(actions=np.concatenate(actions), rewards=np.concatenate(rewards), states=np.stack(states), means=np.stack(means),
                elites=elites, picks=picks)
