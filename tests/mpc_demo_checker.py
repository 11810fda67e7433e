"""The checker's restatement of a receding-horizon episode that follows a demonstration on the episode's clock (include/mbd_hip.h
mbd_mpc_demo, DESIGN.md section 1 "N10 demo clock"): tests/mpc_delay_checker.py's episode — committed queue, plant, disturbances
and kick included, D = 0 being the episode without a queue — whose diffusion steps are oracle.planner.reverse_once with
``enable_demo`` on an OracleEnv whose ``xref`` and ``rew_xref`` are replaced per tick by a numpy restatement of the window
formula, and whose executed rows keep the tracked positions (``execute_tracked``: mpc_checker.execute's rollout, asked for them
too).  ``track_err`` is float64 numpy on those positions."""
from __future__ import annotations

import numpy as np

from mpc_checker import shift
from mpc_delay_checker import queue_of
from mpc_plant_checker import disturbances, kick, rows_of
from oracle import planner as op

ROWS = 50  # csrc/mbd_kernels.h kXrefRows


def as_tracks(clip):
    """The clip as [K, L, C] float32: a car2d clip [L, 2] is one track."""
    c = np.ascontiguousarray(clip, np.float32)
    return c[None] if c.ndim == 2 else c


def window(clip, c0, t, E, D=0):
    """window_t[k][h] = clip[k][min(c0 + (t + D) E + h, L - 1)], h = 0 .. 49 — [K, 50, C] (python integers: no overflow)."""
    c = as_tracks(clip)
    L = c.shape[1]
    rows = [min(int(c0) + (int(t) + int(D)) * int(E) + h, L - 1) for h in range(ROWS)]
    return np.ascontiguousarray(c[:, rows])


def windows(clip, c0, T, E, D=0):
    return np.stack([window(clip, c0, t, E, D) for t in range(T)])


def extended(xref, extra=7, drift=1e-4):
    """The synthetic clip of the tests, all rows distinct: xref's rows plus ``extra`` rows continued at the velocity of its last
    moving pair of rows (the envs' demos end — and start — on held rows, whose own velocity is 0), and, to tell the held rows
    apart as well, row r moved by r * ``drift`` along x.  float64, cast once.  [K, L0 + extra, C] (a car2d demo [L0, 2] stays 2-D)."""
    x = np.asarray(xref, np.float32)
    flat = x.ndim == 2
    x = as_tracks(x).astype(np.float64)
    step = np.diff(x, axis=1)
    moving = np.nonzero(np.abs(step).sum(axis=(0, 2)))[0]
    v = step[:, moving[-1]] if len(moving) else np.zeros_like(x[:, 0])
    more = x[:, -1][:, None] + np.arange(1, extra + 1)[None, :, None] * v[:, None]
    out = np.concatenate([x, more], axis=1)
    out[:, :, 0] += drift * np.arange(out.shape[1])[None, :]
    out = out.astype(np.float32)
    for k in range(out.shape[0]):
        assert len({r.tobytes() for r in out[k]}) == out.shape[1], "the clip's rows are not distinct"
    return np.ascontiguousarray(out[0] if flat else out)


def windowed(oenv, win, rew_xref):
    """``oenv`` with the demo replaced by one tick's window [K, 50, C] and the record's reward level."""
    xref = win[0] if oenv.name == "car2d" else win
    return op.OracleEnv(oenv.orc, oenv.name, oenv.ms, xref=np.ascontiguousarray(xref, np.float32), rew_xref=float(rew_xref),
                        init_q=oenv.init_q)


def execute_tracked(oenv, s, rows):
    """mpc_checker.execute with the tracked positions kept: rewards [E], the state after the rows, positions [E, K, 3] (car2d:
    its qs — x, y, theta — as one track)."""
    us = np.ascontiguousarray(rows, np.float32)[None]
    if oenv.name == "car2d":
        rewss, qs = oenv.orc.car2d_rollout(s, us, want_qs=True)
        return rewss[0], qs[0, -1].copy(), qs[0][:, None, :].copy()
    rewss, xpos, fin = oenv.orc.rollout(oenv.ms, s, us, want_xpos=True, want_final=True)
    return rewss[0], fin[0].reshape(-1), xpos[0]


def track_err(xpos, clip, c0):
    """float64: err[n][k] = |xpos[n][k][:C] - clip[k][min(c0 + n, L - 1)]| for the executed control steps n."""
    c = as_tracks(clip).astype(np.float64)
    K, L, C = c.shape
    x = np.asarray(xpos, np.float64)
    out = np.zeros((x.shape[0], K))
    for n in range(x.shape[0]):
        d = x[n, :, :C] - c[:, min(int(c0) + n, L - 1)]
        out[n] = np.sqrt((d * d).sum(axis=-1))
    return out


def episode(oenv, clip, c0, rew_xref, state0, key, N, H, Nd, temp, T, K, E, D=0, rows0=None, plant=None, dkey=(0, 0), act_std=0.0,
            kick_std=0.0, kick_every=1, impl=1, beta0=1e-4, betaT=1e-2, frozen=False):
    """A closed-loop episode of T ticks under the demo record (clip, c0, rew_xref), planned with ``oenv`` D ticks ahead (0: no
    queue) and executed on ``plant`` (None: oenv itself).  ``frozen``: every tick plans under tick 0's window — what an
    implementation without a clock would do.  Returns dict(actions, rewards, states, means, demo_windows [T, K, 50, C],
    xpos [T*E, K, 3], track_err [T*E, K] (float64) and, with D > 0, predicted [T, S])."""
    orc = oenv.orc
    plant = oenv if plant is None else plant
    Nu = oenv.Nu
    assert H == ROWS
    sched = orc.schedule(beta0, betaT, Nd)
    rng, dk = np.asarray(key, np.uint32), np.asarray(dkey, np.uint32)
    s = np.ascontiguousarray(state0, np.float32).reshape(-1)
    W = windows(clip, c0, T, E, D)
    C = queue_of(rows0, D, E, Nu) if D else None
    Ybar, i_start = np.zeros((H, Nu), np.float32), Nd - 1
    actions, rewards, states, means, predicted, xposs = [], [], [s], [], [], []
    for t in range(T):
        keys = orc.split(rng, 2, impl)
        rng, r = keys[0], keys[1]  # rng, k_t = split(rng)
        shat = s
        if D:
            _, shat, _ = execute_tracked(oenv, s, C.reshape(D * E, Nu))  # the PLAN's env over the undisturbed queue
            shat = np.asarray(shat, np.float32).reshape(-1)
        wenv = windowed(oenv, W[0 if frozen else t], rew_xref)
        for i in range(i_start, 0, -1):
            r, Ybar, _, _ = op.reverse_once(orc, wenv, shat, i, r, Ybar, sched, N, H, temp, impl, enable_demo=True)
        M = Ybar
        dk, eps = disturbances(orc, dk, E, Nu, impl)
        rows = rows_of(C[0] if D else M, E, eps, act_std)
        rew, s, xpos = execute_tracked(plant, s, rows)
        if kick_std > 0 and (t + 1) % kick_every == 0:
            s = kick(plant, s, (np.float32(kick_std) * eps[E * Nu:].astype(np.float32)).astype(np.float32))
        actions.append(rows)
        rewards.append(rew)
        states.append(s)
        means.append(M)
        predicted.append(shat)
        xposs.append(xpos)
        if D:
            C = np.concatenate([C[1:], M[:E][None]]).astype(np.float32)  # (copied: -0.0 stays -0.0)
        Ybar, i_start = shift(M, E), K
    xp = np.concatenate(xposs)
    out = dict(actions=np.concatenate(actions), rewards=np.concatenate(rewards), states=np.stack(states), means=np.stack(means),
               demo_windows=W, xpos=xp, track_err=track_err(xp, clip, c0))
    if D:
        out["predicted"] = np.stack(predicted)
    return out


# ---- the cases the CPU tests prove able to tell and the GPU tests run --------------------------------------------------------
# (T, E, L = 50 + 7, c0): windows that start at rows 2, 5, 8 and reach past the clip's end; windows held on the last row
ND, WARM, N = 6, 2, 64
SHAPES = {"moving": (3, 3, 2), "held": (2, 1, 60)}
TEMP = 0.1
# plant record of the plant case: a heavier, weaker body, action noise and a kick after every second tick
PLANT = dict(act_std=0.1, kick_std=0.3, kick_every=2)
MISMATCH = dict(mass=1.3, friction=0.5, gear=0.8)
DELAY = (3, 2, 1)  # T, E, D of the delay case
SEED_RESET, SEED_KEY, SEED_DISTURB = 5, 6, 11


REW_XREF = {"humanoidtrack": 1.0, "car2d": 0.75}  # the records' reward level (humanoidtrack.py:44; car2d: any finite value does)


def oracle_env(orc, name, custom=None, rew_xref=None):
    """The OracleEnv of ``name`` with its demo, from the compiled assets — no device.  ``custom``: (model, xref) of a
    caller-compiled tracked model (a mbd_hip.model.Model and its demonstration [n_track, 50, 3]) under that env name, with
    ``rew_xref`` as its reward level."""
    import os

    from conftest import ROOT, load_model
    if custom is not None:
        m, xref = custom
        assert np.shape(xref) == (int(m.fields["n_track"]), ROWS, 3), np.shape(xref)
        return op.OracleEnv(orc, name, m.to_struct(), xref=np.ascontiguousarray(xref, np.float32),
                            rew_xref=float(REW_XREF.get(name, 0.0) if rew_xref is None else rew_xref), init_q=m.init_q)
    compiled = os.path.join(ROOT, "model-based-diffusion_amd", "assets", "compiled")
    if name == "car2d":
        return op.OracleEnv(orc, "car2d", xref=np.load(os.path.join(compiled, "car2d_xref.npy")).astype(np.float32),
                            rew_xref=REW_XREF[name])
    m = load_model(name)
    return op.OracleEnv(orc, name, m.to_struct(), xref=np.load(os.path.join(compiled, "jog_xref.npy")).astype(np.float32),
                        rew_xref=REW_XREF[name], init_q=m.init_q)


def plant_env(orc, name):
    """The mismatched plant of the plant case (no demo of its own: it only executes)."""
    from conftest import load_model
    m = load_model(name).scaled(**MISMATCH)
    return op.OracleEnv(orc, name, m.to_struct(), init_q=m.init_q)


_CACHE = {}


def case(orc, name, variant, frozen=False):
    """The checker's episode of a test case, computed once per process and left unchanged: ``variant`` is a key of SHAPES, or
    "delay" (D = 1, E = 2, T = 3, c0 = 2) or "plant" (SHAPES["moving"] on the mismatched, disturbed plant); "held" follows
    the clip played backwards.  Returns
    (episode dict, dict(clip, c0, rew_xref, state0, key, dkey, T, E, D))."""
    from mbd_hip.envs.base import prng_impl
    k = (name, variant, frozen)
    if k in _CACHE:
        return _CACHE[k]
    oenv = oracle_env(orc, name)
    clip = extended(oenv.xref)
    if variant == "held":
        # every window is the clip's LAST row: under the clip as it is that row lies metres ahead of the system, every candidate's
        # distance is clipped alike, the blended log-densities have no spread and the reference's unguarded division (:125) makes
        # every mean NaN — which compares nothing.  Played backwards the clip ends where the system starts.
        clip = np.ascontiguousarray(as_tracks(clip)[:, ::-1][0] if clip.ndim == 2 else clip[:, ::-1])
    impl = prng_impl()
    state0 = np.ascontiguousarray(oenv.reset(orc.prng_key(SEED_RESET), impl), np.float32).reshape(-1)
    key, dkey = orc.prng_key(SEED_KEY), orc.prng_key(SEED_DISTURB)
    D, kw = 0, {}
    if variant == "delay":
        T, E, D = DELAY
        c0 = 2
    else:
        T, E, c0 = SHAPES["moving" if variant == "plant" else variant]
    if variant == "plant":
        kw = dict(plant=plant_env(orc, name), dkey=dkey, **PLANT)
    ep = episode(oenv, clip, c0, REW_XREF[name], state0, key, N, ROWS, ND, TEMP, T, WARM, E, D=D, impl=impl, frozen=frozen, **kw)
    _CACHE[k] = (ep, dict(clip=clip, c0=c0, rew_xref=REW_XREF[name], state0=state0, key=key, dkey=dkey, T=T, E=E, D=D))
    return _CACHE[k]
