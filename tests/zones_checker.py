"""The zone record (include/mbd_hip.h mbd_zones; DESIGN.md section 1 "N20 zones") restated in numpy float32, operation by operation
as the contract has it — the way tests/track_inputs.py::terms32 restates the demo log-density.  It works on the checker's positions
and rewards as they stand: `launch(zones, xpos, rews)` is one zone launch, `ZoneEnv` wraps an OracleEnv (or a wrapper of one) so that
the checkers' planning loops plan under the record.  numpy only; nothing here touches a device or the library.

A zone is a dict(kind 0 keep-out / 1 goal, links bit mask or None: every slot, center [3], scale [3], radius, margin, weight) — what
mbd_hip.planners.mpc.zone builds, with links resolved to a mask (`resolved`).

Comparison rule (`same`): finite values by bit pattern; non-finite values by class (NaN where NaN, same-signed inf); the NaNs of
clr as the canonical pattern 0x7fc00000 (`same_clr`)."""
import numpy as np

F32 = np.float32
KEEP_OUT, GOAL = 0, 1
CANON_NAN = np.array([0x7fc00000], np.uint32).view(F32)[0]


def resolved(zones, K):
    """The zones with ``links`` as a bit mask over K track slots (None: all; a list of slots: their bits)."""
    out = []
    for z in zones:
        links = z.get("links")
        if links is None:
            mask = (1 << K) - 1
        elif isinstance(links, (int, np.integer)):
            mask = int(links)
        else:
            mask = sum(1 << int(l) for l in links)
        out.append(dict(z, links=mask))
    return out


def distance(x, z):
    """d of one zone at positions x [..., 3]: e_i = (x_i - c_i) * s_i, q = (e_0 e_0 + e_1 e_1) + e_2 e_2, d = sqrt(q)."""
    x = np.asarray(x, F32)
    c, s = np.asarray(z["center"], F32), np.asarray(z["scale"], F32)
    with np.errstate(all="ignore"):
        e = [((x[..., i] - c[i]).astype(F32) * s[i]).astype(F32) for i in range(3)]
        q = [(v * v).astype(F32) for v in e]
        return np.sqrt(((q[0] + q[1]).astype(F32) + q[2]).astype(F32)).astype(F32)


def clip_v(u):
    """fclip_nan(u, 0, 1): two selects, so a NaN stays a NaN (and -0 stays -0)."""
    return np.where(u < 0, F32(0), np.where(u > 1, F32(1), u)).astype(F32)


def term(d, z):
    """(term, v) of one zone at distances d: u, v = clip(u, 0, 1), term = w * (v * v)."""
    r, m, w = F32(z["radius"]), F32(z["margin"]), F32(z["weight"])
    with np.errstate(all="ignore"):
        if int(z["kind"]) == GOAL:
            u = ((d - r).astype(F32) / m).astype(F32)
        else:
            u = ((F32(r + m) - d).astype(F32) / m).astype(F32)
        v = clip_v(u)
        return (w * (v * v).astype(F32)).astype(F32), v


def nan_min(a, b):
    """The minimum in which a NaN wins, elementwise."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    with np.errstate(all="ignore"):
        return np.where(np.isnan(a) | np.isnan(b), F32(np.nan), np.minimum(a, b)).astype(F32)


def canon(a):
    """``a`` with every NaN replaced by the canonical quiet NaN the contract stores."""
    a = np.array(a, F32)
    a[np.isnan(a)] = CANON_NAN
    return a


def steps(zones, xpos):
    """(s_t, clr_t) [..., H] of positions xpos [..., H, K, 3]: s_t from +0, the terms added with slot k outer and zone z inner where
    bit k of the zone's links is set — a pair outside the mask contributes no operation —; clr_t the minimum of d - r over the
    step's keep-out terms, +inf where there are none, a NaN winning."""
    xpos = np.asarray(xpos, F32)
    K = xpos.shape[-2]
    s = np.zeros(xpos.shape[:-2], F32)
    c = np.full(xpos.shape[:-2], np.inf, F32)
    with np.errstate(all="ignore"):
        for k in range(K):
            for z in zones:
                if not (int(z["links"]) >> k) & 1:
                    continue
                d = distance(xpos[..., k, :], z)
                s = (s + term(d, z)[0]).astype(F32)
                if int(z["kind"]) == KEEP_OUT:
                    c = nan_min(c, (d - F32(z["radius"])).astype(F32))
    return s, c


def launch(zones, xpos, rews=None):
    """One zone launch over xpos [B, H, K, 3] and rews [B]: dict(rews, pen, clr [B], step_pen, step_clr [B, H]) — pen from +0 adds
    s_t in ascending t, then ONE division by float(H); rews - pen; clr the minimum over t; the NaNs of clr and step_clr canonical."""
    xpos = np.asarray(xpos, F32)
    B, H = xpos.shape[:2]
    s, c = steps(zones, xpos)
    pen, clr = np.zeros(B, F32), np.full(B, np.inf, F32)
    with np.errstate(all="ignore"):
        for t in range(H):
            pen = (pen + s[:, t]).astype(F32)
            clr = nan_min(clr, c[:, t])
        pen = (pen / F32(H)).astype(F32)
        out = dict(pen=pen, clr=canon(clr), step_pen=s, step_clr=canon(c))
        if rews is not None:
            out["rews"] = (np.asarray(rews, F32) - pen).astype(F32)
    return out


def classes(zones, xpos):
    """v of every (candidate, step, slot, zone) term inside the masks, as one flat array: the census' population."""
    xpos = np.asarray(xpos, F32)
    vs = []
    for k in range(xpos.shape[-2]):
        for z in zones:
            if (int(z["links"]) >> k) & 1:
                vs.append(term(distance(xpos[..., k, :], z), z)[1].reshape(-1))
    return np.concatenate(vs)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same(got, ref, what=""):
    """The comparison rule: finite values by bit pattern, non-finite ones by class."""
    g, r = np.asarray(got, F32).reshape(-1), np.asarray(ref, F32).reshape(-1)
    assert g.size == r.size, f"{what}: {g.size} values against {r.size}"
    fin = np.isfinite(r)
    bad = np.flatnonzero(np.where(fin, bits(g) != bits(r), ~((np.isnan(g) & np.isnan(r)) | ((g == r) & ~np.isfinite(g)))))
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {g.size} values differ, first at flat index {i}: {g[i]!r} (0x{bits(g)[i]:08x}) "
                             f"against {r[i]!r} (0x{bits(r)[i]:08x})")


def same_clr(got, ref, what=""):
    """Clearances: every value by bit pattern, NaNs included — the contract stores the canonical NaN."""
    g, r = bits(np.asarray(got, F32)).reshape(-1), bits(canon(ref)).reshape(-1)
    assert g.size == r.size, f"{what}: {g.size} values against {r.size}"
    bad = np.flatnonzero(g != r)
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {g.size} clearances differ, first at flat index {i}: 0x{g[i]:08x} against 0x{r[i]:08x}")


def same_launch(got, ref, what=""):
    """Every output of a launch (dicts as `launch` returns them) under the comparison rule."""
    for k in ("rews", "pen", "step_pen"):
        if k in ref:
            same(got[k], ref[k], f"{what}: {k}")
    for k in ("clr", "step_clr"):
        same_clr(got[k], ref[k], f"{what}: {k}")


class ZoneEnv:
    """An OracleEnv (or a wrapper of one: an ObjectiveEnv) whose ``rollout`` returns every candidate's reward less the record's
    penalty of the tracked positions of its own rollout, as a one-column [B, 1] array — the checkers' mean over that column is the
    entry itself.  ``zones``: resolved zones; replace the attribute to move them between ticks (mbd_plan_update_zones).  ``last``:
    the `launch` dict of the last rollout; ``log``: every rollout's, when it is a list."""

    def __init__(self, oenv, zones):
        self.oenv, self.zones = oenv, zones
        self.last, self.log = None, None

    def __getattr__(self, name):
        return getattr(self.oenv, name)

    def rollout(self, state0, us, want_xpos=False):
        from oracle import planner as op
        env = self.oenv
        while hasattr(env, "oenv"):
            env = env.oenv
        rewss, xpos = self.oenv.rollout(state0, us, want_xpos=True)
        rewss = np.ascontiguousarray(rewss, F32)
        self.last = launch(self.zones, xpos, op.mean_h(env.orc, rewss))
        if self.log is not None:
            self.log.append(self.last)
        shaped = self.last["rews"][:, None]
        return (shaped, xpos) if want_xpos else shaped


def executed(orc, ms, zones, states, actions, E):
    """(zone_pen, zone_clear) [T E] of an episode's executed steps, restated from its logs: tick t's E rows rolled out on the
    checker from the logged state s_t, their tracked positions through `steps`."""
    states, actions = np.asarray(states, F32), np.asarray(actions, F32)
    T = states.shape[0] - 1
    pen, clr = [], []
    for t in range(T):
        us = np.ascontiguousarray(actions[t * E:(t + 1) * E][None])
        _, xpos = orc.rollout(ms, np.ascontiguousarray(states[t]), us, want_xpos=True)
        s, c = steps(zones, xpos[0])
        pen.append(s)
        clr.append(canon(c))
    return np.concatenate(pen), np.concatenate(clr)
