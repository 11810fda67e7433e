"""The checker's restatement of the value record (include/mbd_hip.h mbd_value, DESIGN.md section 1 "N16 value"): what a diffusion
step adds to the rewards buffer behind the rollout (and the objective record), in numpy float32 with every operation spelled out and
rounded.  The two operations numpy does not have come from the oracle's primitives (``orc.sp_eval``), the way weighting_checker
takes them: ``exp_``, and the fused multiply-add as dot((a, 1, 0), (b, c, 0)) = fma(a, b, fma(1, c, 0 * 0)) = fma(a, b, c) — exact
except for c = -0, which that form turns into +0; there fma(a, b, -0) is the rounded product itself (x + -0 = x for every x) and is
taken as such.  ``value`` is vectorised over rows and outputs and loops over k, the order the contract fixes.

``ValueEnv`` hands the rewards the record leaves to the existing checkers as a one-column array, in the manner of
objective_checker.ObjectiveEnv, which it may wrap (the value launch follows the objective's)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

f32 = np.float32
LINK = 13


@dataclass
class Net:
    """mbd_value: W[l] [width, inputs], b[l] [width], act "relu" / "tanh", center / in_scale [n_in] or None, rel_xy, scale."""
    W: list
    b: list
    act: str = "relu"
    center: object = None
    in_scale: object = None
    rel_xy: bool = False
    scale: float = 1.0

    def value_net(self):
        """The ``mbd_hip.planners.value.ValueNet`` of the same fields (what ``Plan.set_value`` takes)."""
        from mbd_hip.planners.value import ValueNet
        return ValueNet(self.W, self.b, self.act, self.center, self.in_scale, self.rel_xy, self.scale)


def fma(orc, a, b, c):
    a, b, c = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32))
    rows = np.zeros((a.size, 6), f32)
    rows[:, 0], rows[:, 1], rows[:, 3], rows[:, 4] = a.reshape(-1), 1.0, b.reshape(-1), c.reshape(-1)
    out = orc.sp_eval("dot", rows).reshape(a.shape)
    with np.errstate(all="ignore"):
        return np.where((c == 0) & np.signbit(c), (a * b).astype(f32), out).astype(f32)


def relu(a):
    with np.errstate(all="ignore"):
        return np.where(a > 0, a, np.where(a <= 0, f32(0), a)).astype(f32)


def tanh(orc, a):
    with np.errstate(all="ignore"):
        aa = np.abs(a).astype(f32)
        m = np.where(aa < f32(44), aa, f32(44)).astype(f32)
        t = orc.sp_eval("exp_", (f32(-2) * m).astype(f32).reshape(-1)).reshape(a.shape).astype(f32)
        y = ((f32(1) - t).astype(f32) / (f32(1) + t).astype(f32)).astype(f32)
        return np.where(np.isnan(a), a, np.copysign(y, a)).astype(f32)


def inputs(net: Net, states):
    """x_0 [B, n_in]."""
    s = np.array(states, f32).reshape(len(states), -1)
    n_in = s.shape[1]
    with np.errstate(all="ignore"):
        if net.rel_xy:
            x0, y0 = s[:, 0].copy(), s[:, 1].copy()
            for l in range(n_in // LINK):
                s[:, LINK * l] = (s[:, LINK * l] - x0).astype(f32)
                s[:, LINK * l + 1] = (s[:, LINK * l + 1] - y0).astype(f32)
        center = np.zeros(n_in, f32) if net.center is None else np.asarray(net.center, f32)
        in_scale = np.ones(n_in, f32) if net.in_scale is None else np.asarray(net.in_scale, f32)
        return ((s - center).astype(f32) * in_scale).astype(f32)


def value(orc, net: Net, states, want_pre=False):
    """V [B] of ``states`` [B, n_in]; with ``want_pre`` also the hidden layers' pre-activations, a list of [B, width]."""
    x = inputs(net, states)
    pre = []
    n = len(net.W)
    for l in range(n):
        W, b = np.asarray(net.W[l], f32), np.asarray(net.b[l], f32)
        a = np.broadcast_to(b, (x.shape[0], W.shape[0])).astype(f32)
        for k in range(W.shape[1]):
            a = fma(orc, W[None, :, k], x[:, k, None], a)
        if l + 1 < n:
            pre.append(a)
            x = tanh(orc, a) if net.act == "tanh" else relu(a)
    V = a[:, 0]
    return (V, pre) if want_pre else V


def add(rews, scale, V):
    """rews + (scale * V): a product, then a sum."""
    with np.errstate(all="ignore"):
        return (np.asarray(rews, f32) + (f32(scale) * np.asarray(V, f32)).astype(f32)).astype(f32)


def canon(a):
    """``a`` with every NaN replaced by one NaN: which NaN an operation makes (its sign, its payload) is the processor's, not the
    contract's — everything else, infinities and the signs of zeros included, is compared by bits."""
    a = np.array(a, f32)
    a[np.isnan(a)] = f32(np.nan)
    return a


def _base(env):
    """The OracleEnv at the bottom of a stack of wrappers."""
    while hasattr(env, "oenv"):
        env = env.oenv
    return env


def final_states(env, state0, us):
    """The final states [B, state_size] of the candidates' rollouts on the env's model."""
    base = _base(env)
    us = np.ascontiguousarray(us, f32)
    if base.name == "car2d":
        return base.orc.car2d_rollout(state0, us, want_qs=True)[1][:, -1].reshape(us.shape[0], -1)
    return base.orc.rollout(base.ms, state0, us, want_final=True)[1].reshape(us.shape[0], -1)


class ValueEnv:
    """An OracleEnv (or a wrapper of one: an ObjectiveEnv, a windowed demo env) whose ``rollout`` returns every candidate's reward
    with scale * V of its final state added, as a one-column [B, 1] array — the checkers' mean over that column is the entry
    itself.  ``last``: (rews' [B], V [B], rews [B] before the record) of the last rollout."""

    def __init__(self, oenv, net: Net):
        self.oenv, self.net = oenv, net
        self.last = None

    def __getattr__(self, name):
        return getattr(self.oenv, name)

    def rollout(self, state0, us, want_xpos=False):
        from oracle import planner as op
        orc = _base(self.oenv).orc
        out = self.oenv.rollout(state0, us, want_xpos=True) if want_xpos else self.oenv.rollout(state0, us)
        rewss = np.ascontiguousarray(out[0] if want_xpos else out, f32)
        rews = op.mean_h(orc, rewss)
        V = value(orc, self.net, final_states(self.oenv, state0, us))
        self.last = (add(rews, self.net.scale, V), V, rews)
        shaped = self.last[0][:, None]
        return (shaped, out[1]) if want_xpos else shaped
