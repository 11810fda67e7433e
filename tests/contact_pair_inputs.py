"""Start states of the one-collider humanoids (humanoidrun, humanoidtrack: one sphere at the end of each shin) that put every
case of stage (4) — contact detection, the position solve and its friction test — in front of the rollout kernels, and the
checker-side census that says which case a state reaches (tests/test_contact_pair_cases.py on the CPU;
tests/test_gpu_contact_pairs.py runs the same states on the GPU).

A state is pipeline_init(q, qd).  The census replays stage (4) of a substep from the checker's stage dump
(orc_substep_stages: the poses before the step and after stage (3)) with the checker's own primitives (orc_sp_eval) and
exact fused multiply-adds, and is held to the dump's poses after stage (4) bit for bit — so its flags (active, stick /
slip), its penetration and its tangential motion are the checker's, not an estimate of them."""
import ctypes as C
import functools
from fractions import Fraction

import numpy as np

import state_inputs as si

F = np.float32
RIGHT, LEFT = 0, 1  # collider slots: the right shin's sphere, the left shin's
KNEE_R, KNEE_L = 13, 17  # q of the knee hinges


def _round32(fr):
    """The float32 nearest to the rational fr, ties to even."""
    if fr == 0:
        return F(0.0)
    c = F(float(fr))
    cands = [c, np.nextafter(c, F(-np.inf)), np.nextafter(c, F(np.inf))]
    err = [abs(Fraction(float(x)) - fr) for x in cands]
    best = min(err)
    tied = [x for x, e in zip(cands, err) if e == best]
    if len(tied) > 1:
        tied = [x for x in tied if (x.view(np.uint32) & 1) == 0]
    return tied[0]


def fma32(a, b, c):
    """fmaf(a, b, c): one rounding of the exact a b + c."""
    return _round32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def variant(name):
    """(Model, env name) of a test model: the built-in humanoids, and humanoidrun with another reward kind ("generic": the
    instantiation without a compiled-in reward and substep count) or with five substeps per control step ("frames5")."""
    if name == "generic":
        m, env_name = si.model("humanoidrun")
        m.fields["reward_kind"] = type(m.fields["reward_kind"])(4)  # (the stand-up reward on the running humanoid)
        return m, env_name
    if name == "frames5":
        m, env_name = si.model("humanoidrun")
        m.fields["n_frames"] = type(m.fields["n_frames"])(5)
        return m, env_name
    return si.model(name)


def stages(orc, ms, L, s, a):
    """(state after the substep, stage dump [6][L][13]) of one substep from state s under the action a."""
    f32 = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
    orc.lib.orc_substep_stages.argtypes = [C.c_void_p, f32, f32, f32, f32]
    orc.lib.orc_substep_stages.restype = None
    out = np.zeros((L, 13), np.float32)
    dump = np.zeros((6, L, 13), np.float32)
    orc.lib.orc_substep_stages(C.addressof(ms), np.ascontiguousarray(s, np.float32).reshape(-1),
                               np.ascontiguousarray(a, np.float32).reshape(-1), out.reshape(-1), dump.reshape(-1))
    return out, dump


def replay_stage4(orc, m, dump):
    """Stage (4) of the substep that left `dump`, for every collider: a list of dicts (pen, active, ct2, stick, off, and the
    link's position after the stage), computed from the poses before the step (dump[0]) and after stage (3) (dump[2])."""
    f = m.fields
    n = int(f["n_col"])
    link, cpos, rad = np.asarray(f["col_link"], int), np.asarray(f["col_pos"], F), np.asarray(f["col_radius"], F)
    inv_mass, inv_inertia = np.asarray(f["inv_mass"], F), np.asarray(f["inv_inertia"], F)
    mu, scale = F(f["friction"]), F(f["collide_scale"])
    def ev(op, *xs):
        return orc.sp_eval(op, np.concatenate([np.asarray(x, F).reshape(-1) for x in xs]))[0]

    out = []
    for k in range(n):
        l = int(link[k])
        p, r = dump[2, l, 0:3], dump[2, l, 3:7]
        p0, r0 = dump[0, l, 0:3], dump[0, l, 3:7]
        im, ib = inv_mass[l], inv_inertia[l, 0]
        assert inv_inertia[l, 0] == inv_inertia[l, 1] == inv_inertia[l, 2] and not inv_inertia[l, 3:].any(), "isotropic links"
        off = ev("rot", cpos[k], r)
        ctr = p + off
        pen = F(rad[k] - ctr[2])
        rec = dict(link=l, pen=pen, active=bool(pen > 0), off=off, ct2=None, stick=None, p_after=p.copy())
        if rec["active"]:
            h = fma32(F(-0.5), pen, rad[k])
            pos = np.array([ctr[0], ctr[1], ctr[2] - h], F)
            rc = np.array([off[0], off[1], off[2] - h], F)
            cn = np.array([rc[1], -rc[0]], F)
            icn = cn * ib
            wn = F(im + fma32(cn[0], icn[0], cn[1] * icn[1]))
            dlam = F(ev("div_pos_", [pen, wn]) * scale)
            rl = cpos[k] + ev("irot_z", [-h], r)
            pprev = p0 + ev("rot", rl, r0)
            dx = np.array([pos[0] - pprev[0], pos[1] - pprev[1], 0], F)
            ct2 = fma32(dx[0], dx[0], dx[1] * dx[1])
            cnt = np.array([-(rc[2] * dx[1]), rc[2] * dx[0], fma32(rc[0], dx[1], -(rc[1] * dx[0]))], F)
            icnt = cnt * ib
            dent = fma32(im, ct2, fma32(cnt[0], icnt[0], fma32(cnt[1], icnt[1], cnt[2] * icnt[2])))
            gt = ev("div_pos_", [ct2, F(dent + F(1e-20))])
            lim = F(mu * dlam)
            stick = bool(F(F(ct2 * gt) * gt) < F(lim * lim))
            P = np.array([F(-gt) * dx[0] if stick else 0, F(-gt) * dx[1] if stick else 0, dlam], F)
            rec.update(ct2=ct2, stick=stick, dlam=dlam, dx=dx, p_after=p + im * P)
        out.append(rec)
    return out


def census(orc, m, s0, us):
    """Every substep of the rollout of `us` [B][H][Nu] from s0 through replay_stage4: a list over candidates of lists over
    substeps of the per-collider records.  The replay's positions after stage (4) must be the dump's, bit for bit."""
    ms, L, nf = m.to_struct(), m.n_links, int(m.fields["n_frames"])
    n_act = {}
    for k in range(int(m.fields["n_col"])):
        n_act[int(m.fields["col_link"][k])] = n_act.get(int(m.fields["col_link"][k]), 0) + 1
    assert set(n_act.values()) == {1}, "one collider per link"
    out = []
    for b in range(us.shape[0]):
        s, per = np.array(s0, np.float32), []
        for t in range(us.shape[1]):
            for _ in range(nf):
                s, dump = stages(orc, ms, L, s, us[b, t])
                recs = replay_stage4(orc, m, dump)
                for rec in recs:
                    si.same_bits(rec["p_after"], dump[3, rec["link"], 0:3], "replayed stage (4) against the checker's dump")
                per.append(recs)
        out.append(per)
    return out


# ---- the start states -----------------------------------------------------------------------------------------------------
def _q(m, z=None, knee_r=0.0, knee_l=0.0, quat=None):
    q = m.init_q.astype(np.float32).copy()
    if z is not None:
        q[2] = z
    q[KNEE_R], q[KNEE_L] = knee_r, knee_l
    if quat is not None:
        q[3:7] = quat
    return q


def _first(orc, m, q, qd):
    """The stage-(4) records of the first substep from pipeline_init(q, qd) under zero actions."""
    ms = m.to_struct()
    s = orc.forward(ms, q, qd)
    _, dump = stages(orc, ms, m.n_links, s, np.zeros(m.act_size(), np.float32))
    return replay_stage4(orc, m, dump)


def _pen(orc, m, q, qd, slot):
    """The penetration of collider `slot` in stage (4) of the first substep from pipeline_init(q, qd) under zero actions."""
    ms = m.to_struct()
    _, dump = stages(orc, ms, m.n_links, orc.forward(ms, q, qd), np.zeros(m.act_size(), np.float32))
    l = int(m.fields["col_link"][slot])
    off = orc.sp_eval("rot", np.concatenate([np.asarray(m.fields["col_pos"], F)[slot], dump[2, l, 3:7]]))[0]
    return F(F(m.fields["col_radius"][slot]) - F(dump[2, l, 2] + off[2]))


def _solve_pen(orc, m, q, qd, slot, want, knee=KNEE_L):
    """A start state whose collider `slot` has exactly the penetration `want` (a float32) in the first substep: the root
    height by bisection over its floats, then the root's vertical velocity by bisection (a float of it moves the sphere by
    far less than a float of the height does): the largest velocity whose penetration is not below `want`.  Where that
    penetration is not `want` itself (the sphere's height moves in coarser steps than its penetration counts in) the knee
    above the sphere is bent by another microradian, which reshuffles the roundings on the way, and the velocity is
    found again.  Returns (q, qd)."""
    q, qd = q.copy(), qd.copy()
    pen = lambda: _pen(orc, m, q, qd, slot)
    lo, hi = F(q[2] - 0.5), F(q[2] + 0.5)  # pen falls as the root rises: pen(lo) > want >= pen(hi)
    while True:
        mid = F((lo + hi) * F(0.5))
        if mid in (lo, hi):
            break
        q[2] = mid
        lo, hi = (mid, hi) if pen() > want else (lo, mid)
    q[2] = hi
    k0 = q[knee]
    for k in range(400):
        q[knee] = F(k0 - F(k) * F(1e-6))
        vlo, vhi = F(-2e-2), F(2e-2)  # pen rises as the velocity falls: pen(vlo) > want >= pen(vhi)
        while True:
            mid = F((vlo + vhi) * F(0.5))
            if mid in (vlo, vhi):
                break
            qd[2] = mid
            vlo, vhi = (mid, vhi) if pen() > want else (vlo, mid)
        qd[2] = vhi
        if pen() == want:
            return q, qd
    raise AssertionError(f"no start state puts the penetration at exactly {want!r}")


@functools.lru_cache(maxsize=None)
def cases(name):
    """[(case, q, qd)] of a test model; EXPECT says what stage (4) of the first substep must find in each."""
    from oracle.oracle import Oracle
    orc = Oracle("f32")
    m, _ = variant(name)
    zero = np.zeros(m.qd_size(), np.float32)
    touch_z = F(m.init_q[2] - si.lowest_gap(m, si.init_state(orc, m)))  # both spheres on the plane, to a float or so
    bent = -1.2  # a knee bent this far lifts its sphere about 15 cm
    out = [("air", _q(m), zero)]
    out.append(("rest_left", _q(m, touch_z - F(2e-3), knee_r=bent), _vel(zero, vx=0.01)))
    out.append(("slide_left", _q(m, touch_z - F(2e-3), knee_r=bent), _vel(zero, vx=3.0, vy=-1.0)))
    out.append(("both", _q(m, touch_z - F(1e-3)), _vel(zero, vx=0.02)))
    q, qd = _solve_pen(orc, m, _q(m, touch_z, knee_r=bent), zero, LEFT, F(0.0))
    out.append(("touch_left", q, qd))
    grid = np.spacing(F(m.fields["col_radius"][LEFT]))  # the spacing of the floats at the sphere centre's height
    q, qd = _solve_pen(orc, m, _q(m, touch_z, knee_r=bent), zero, LEFT, F(grid))
    out.append(("touch_left_one_float_below", q, qd))
    # at rest, knees bent to inside their limits (no limit correction swings the shins), both spheres 5 mm in: nothing moves
    # along the plane in the first substep
    q = _q(m, touch_z, knee_r=-0.3, knee_l=-0.3)
    q[2] = F(touch_z - si.lowest_gap(m, orc.forward(m.to_struct(), q, zero)) - 5e-3)
    out.append(("still", q, zero))
    out.append(("deep", _q(m, touch_z - F(2e-2)), _vel(zero, vx=0.1)))
    return out


def _vel(zero, vx=0.0, vy=0.0, vz=0.0):
    qd = zero.copy()
    qd[0:3] = (vx, vy, vz)
    return qd


def actions(m, b, h, seed=0):
    """[b][h][Nu]: a row of zeros, then clipped normals."""
    us = si.actions(m, si._seed("contact_pairs", seed), b=max(b, 6), h=h)[:b].copy()
    us[0] = np.float32(0.0)
    return us


# case -> what stage (4) of the FIRST substep under zero actions finds, per collider slot (RIGHT, LEFT): a predicate over the
# replay's record of that collider
def _air(r): return not r["active"] and r["pen"] < 0
def _stick(r): return r["active"] and r["stick"] and r["ct2"] > 0
def _slip(r): return r["active"] and not r["stick"] and r["ct2"] > 0
def _active(r): return r["active"]


EXPECT = {
    "air": (_air, _air),
    "rest_left": (_air, _stick),
    "slide_left": (_air, _slip),
    "both": (_active, _active),
    "touch_left": (_air, lambda r: not r["active"] and r["pen"] == 0),
    "touch_left_one_float_below": (_air, lambda r: r["active"] and r["pen"] == np.spacing(F(0.0625))),
    "still": (lambda r: r["active"] and r["ct2"] == 0, _active),
    "deep": (lambda r: r["active"] and r["pen"] >= F(0.02), lambda r: r["active"] and r["pen"] >= F(0.02)),
}
