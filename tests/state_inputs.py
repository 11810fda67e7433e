"""Start states and actions for the rollout kernels, away from `env.reset`: one list of named cases per model.

Shared by tests/test_state_coverage.py (the checker on the CPU, under gcov: which lines and branches of the step path the
cases reach) and tests/test_gpu_states.py (the kernels against the checker on the same cases, by bit pattern).  numpy and the
checker only; nothing here touches the library or a device.

`cases(orc, m)` yields `(name, state[n_links][13], actions[B][H][Nu])`; the part of a name before the first "/" is its family:

  random       init_q + U(-a, a) on every coordinate, U(-v, v) on every velocity, (a, v) = (0.3, 1), (1.5, 6), (3.2, 30); free
               roots get a uniformly random orientation and a height in [-0.1, 2].  N_RANDOM states per tier, fixed seeds.
  reached      final states of 50-step rollouts under saturated actions, fed back as start states: tangled poses, several of
               them with the body pushed far BELOW the plane (the contacts are soft: humanoidrun's root ends at z = -0.55 and
               -0.91, walker2d's at -0.36 ... -0.61) — legitimate states of the specification, not poses lying on the ground;
               and reached/unactuated: 100 control steps under zero actions.  (Nothing here "lies on the ground": only the
               feet of the hopper and of the running humanoid collide, so an unactuated body hangs from them with its root
               below the plane — hopper -1.06, humanoidrun -0.41.)
  exact        init_q at rest; every hinge at rot_lo / rot_hi and just beyond, every limited slide at slide_lo / slide_hi.
  contact      the lowest collider sphere touching the plane, one float to either side, a millimetre above (the mixed
               wavefronts start here), two centimetres below; DROP: the sphere's penetration exactly 0 and one float to either
               side after the first integration, an exactly vertical fall, and the resting state (tangential speed and
               normal velocity exactly 0: the clamp of the solver's square root, the flush of its division).
  orientation  the whole body turned by exactly 180 degrees about x, y, z through the root's centre of mass, the same with
               the root quaternion negated; the middle Euler angle of every 2- and 3-dof joint GIMBAL_MARGIN short of +-90 degrees; a jointless
               body turned half a turn against its parent (the alignment error's scalar part is a zero: its SIGN decides).
  raw          written into the state directly: link quaternions of norm 0.9 ... 1.2 around the renormalisation's switch
               at | |q|^2 - 1 | = 0.05, velocities of 1e-30, +0.0 and -0.0.  (Planar models: out-of-plane components zero.)

Every case carries the same kinds of action rows (`actions`): clipped normals, rows of +0.0, of -0.0, of exactly act_lo and
act_hi, and rows beyond both.  B is odd: a half-filled last pair for the two-candidate kernels, a ragged last wavefront
for the rest.

CONDITION (asserted by tests/test_state_coverage.py without exception): every candidate of every case stays finite in the
checker — rewards, tracked positions, final state.
"""
import zlib

import numpy as np

from conftest import load_model

B, H = 9, 6
N_RANDOM = 20
TIERS = ((0.3, 1.0), (1.5, 6.0), (3.2, 30.0))
FAMILIES = ("random", "reached", "exact", "contact", "orientation", "raw")
QUAT_NORMS = (0.9, 0.94, 0.96, 0.98, 1.02, 1.06, 1.2)  # |q|^2 - 1 = -0.19, -0.116, -0.078, -0.040, 0.040, 0.124, 0.44
BUILTIN = ("humanoidrun", "humanoidtrack", "humanoidstandup", "ant", "hopper", "walker2d", "halfcheetah", "cartpole")
CUSTOM = ("crab", "tripod", "tripod3d", "drop", "ant_unhealthy", "hopper3d", "walker2d3d", "halfcheetah3d", "cartpole3d",
          "hopper3d_yaxis", "crab_xz", "crab_yz", "tripod_hi")
# (name, planar, flag word): the specification-switch words tests/test_gpu_parity.py::test_specification_switches_bitexact
# parametrizes and the census of tests/test_state_coverage.py runs
SPEC_WORDS = [
    ("humanoidstandup", None, 4), ("humanoidstandup", None, 8), ("humanoidstandup", None, 12), ("humanoidstandup", None, 16),
    ("humanoidstandup", None, 64), ("humanoidstandup", None, 252),
    ("humanoidrun", None, 64), ("humanoidrun", None, 16 | 8), ("humanoidtrack", None, 64 | 16),
    ("ant", None, 4 | 8 | 16),
    ("hopper", None, 4), ("hopper", None, 8), ("hopper", None, 16), ("hopper", None, 4 | 8 | 16 | 32),
    ("walker2d", None, 12), ("halfcheetah", None, 4 | 8 | 16), ("cartpole", None, 16),
    ("tripod", None, 32), ("tripod", None, 4 | 8 | 16 | 32), ("tripod", False, 4 | 8 | 16 | 32 | 128),
    ("hopper", False, 4 | 8 | 16 | 128), ("walker2d", False, 128 | 8),
    ("crab", None, 4), ("crab", None, 8), ("crab", None, 16), ("crab", None, 32), ("crab", None, 64), ("crab", None, 128),
    ("crab", None, 252)]
LIMIT_EPS = 1e-3  # "just beyond" a joint limit (rad / m)
# The middle Euler angle stops this far short of +-90 degrees.  AT +-90 degrees the checker itself goes non-finite within six
# control steps, even at rest under zero actions (humanoidrun, humanoidtrack, humanoidstandup: the line of nodes is divided
# by cos b + 1e-10 with cos b floored at 1e-15, and the limit correction along that axis is then ~1e10 times too long); at
# 1e-3 short of it one humanoidtrack case still does.  A property of the specification, recorded here; the condition below
# wants finite cases, so the cases stop short.
GIMBAL_MARGIN = 1e-2

# A sphere with a mast on a vertical hinge: everything is symmetric about the vertical through the sphere's centre, so a
# state at rest or falling straight down keeps x, y, and the contact's tangential speed at exact zeros whatever the actuator
# does (it spins the mast about that vertical).  No built-in model can hold a contact's tangential speed at exactly 0.
DROP = """<mujoco><compiler angle="degree" inertiafromgeom="true"/>
<default><geom conaffinity="0" contype="0"/><joint damping="0" limited="false"/></default><option timestep="0.005"/>
<worldbody><geom conaffinity="1" type="plane" size="5 5 1"/>
<body name="ball" pos="0 0 0.3"><joint type="free" name="root"/><geom type="sphere" size="0.1" contype="1"/>
<body name="mast" pos="0 0 0"><joint type="hinge" axis="0 0 1" pos="0 0 0" name="spin"/>
<geom type="capsule" fromto="0 0 0.1 0 0 0.3" size="0.03"/></body></body></worldbody>
<actuator><motor joint="spin" gear="1" ctrllimited="true" ctrlrange="-1 1"/></actuator></mujoco>"""


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(got, ref, what=""):
    """Equality by BIT PATTERN (so that -0.0 differs from +0.0, which np.array_equal cannot see) of two float32 arrays
    with the same number of elements, compared in row-major order (the library hands final states back as [B][state], the
    checker as [B][links][13]: the same memory); the message names the first differing element."""
    g, r = bits(np.asarray(got, np.float32)).reshape(-1), bits(np.asarray(ref, np.float32)).reshape(-1)
    assert g.size == r.size, f"{what}: {g.size} values against {r.size}"
    bad = np.flatnonzero(g != r)
    if bad.size:
        i = int(bad[0])
        gf, rf = g.view(np.float32), r.view(np.float32)
        zero_only = bool(np.all((gf[bad] == 0) & (rf[bad] == 0)))
        raise AssertionError(f"{what}: {bad.size} of {g.size} values differ, first at flat index {i}: {gf[i]!r} "
                             f"(0x{g[i]:08x}) against {rf[i]!r} (0x{r[i]:08x})"
                             + ("; every difference is the sign of a zero" if zero_only else ""))


def model(name, bits=None, planar=None):
    """(Model, env_name): a built-in model, or one of CUSTOM — the crab and the tripod of tests/custom_models.py as
    tests/test_gpu_parity.py::_spec_env compiles them, the tripod and the planar built-ins on the 3-D arithmetic, DROP, and the ant with
    terminate_when_unhealthy off (its reward's `healthy` term then depends on the torso height).  bits: the specification
    switches (mbd_model_flags); planar=False: a planar model on the 3-D arithmetic."""
    from custom_models import CRAB, TRIPOD
    from test_oracle_physics import _compile
    if name == "crab":
        m, env_name = _compile(CRAB, env_name="hopper", n_frames=3, reset_noise=0.02, reward_params=(1.0, 0.5)), "hopper"
    elif name in ("tripod", "tripod3d"):
        m = _compile(TRIPOD, env_name="halfcheetah", n_frames=6, reset_noise=0.05, reward_params=(1.0, 0.1),
                     planar=False if name == "tripod3d" else planar)
        env_name = "halfcheetah"
    elif name == "drop":
        m, env_name = _compile(DROP, env_name="hopper", n_frames=4, reset_noise=0.01, reward_params=(0.3, 1.0)), "hopper"
    elif name == "ant_unhealthy":
        m, env_name = load_model("ant"), "ant"
        rp = np.array(m.fields["reward_params"], np.float32)
        rp[5] = 0.0 if rp[5] != 0.0 else 1.0
        m.fields["reward_params"] = rp
    elif name == "hopper3d_yaxis":
        # The hopper on the 3-D arithmetic with every link's inverse inertia (a, c, a): axisymmetric about the link's y axis.  No
        # capsule of a census model lies along y (the planar ones live in the x-z plane), so the checker's and the kernels'
        # choice of that axis is reached by no other model.  (The tensors need not match the geometry: the arithmetic is the
        # same, as in tests/test_gpu_parity.py::test_general_3d_kernels_by_inertia_class.)
        m, env_name = model("hopper3d")
        ib = np.array(m.fields["inv_inertia"], np.float32)
        for l in range(m.n_links):
            a, c = float(min(ib[l, :3])), float(max(ib[l, :3]))
            ib[l] = [a, c, a, 0, 0, 0]
        m.fields["inv_inertia"] = ib
    elif name in ("crab_xz", "crab_yz"):
        # The crab with only the xz (only the yz) product of every inverse inertia tensor kept: a principal 2 x 2 block of a
        # positive definite matrix beside a positive diagonal entry, so still positive definite; the first non-zero
        # off-diagonal entry that decides "not axisymmetric" is then the second (the third).
        m, env_name = model("crab")
        ib = np.array(m.fields["inv_inertia"], np.float32)
        keep = 4 if name == "crab_xz" else 5
        for k in (3, 4, 5):
            if k != keep:
                ib[:, k] = 0.0
        m.fields["inv_inertia"] = ib
    elif name == "tripod_hi":
        # The tripod with its root's vertical slide limited only ABOVE (its lower limit removed): the one census model whose
        # slide limits are found by the upper bound.
        m, env_name = model("tripod")
        lo = np.array(m.fields["slide_lo"], np.float32)
        assert lo[0, 1] > -1e8 and lo[0, 0] < -1e8
        lo[0, 1] = lo[0, 0]
        m.fields["slide_lo"] = lo
    elif name.endswith("3d"):  # a planar built-in model on the 3-D arithmetic
        m, env_name = load_model(name[:-2]), name[:-2]
        planar = False
    else:
        m, env_name = load_model(name), name
    if planar is False and name not in ("tripod", "tripod3d"):
        m.fields["flags"] = int(m.fields["flags"]) & ~2
    if bits is not None:
        m = m.with_spec(bits)
    return m, env_name


def _seed(*parts):
    return zlib.crc32("/".join(str(p) for p in parts).encode())


def _F(m, key, dtype=np.float64):
    return np.asarray(m.fields[key], dtype)


def is_planar(m):
    return bool(int(m.fields.get("flags", 0)) & 2)


def _key(m):
    """What a seed knows of a model: its sizes — variants of one model (switches, planar=False) get the same states and
    actions."""
    return (m.n_links, m.q_size(), m.act_size())


def actions(m, seed, b=B, h=H):
    """[b][h][Nu]: rows 0..b-6 clipped normals (sigma 0.6 of the widest limit), then a row of +0.0, of -0.0, of exactly
    act_lo, of exactly act_hi, and one 1.5 times beyond them (alternating per control step)."""
    nu = m.act_size()
    lo, hi = _F(m, "act_lo", np.float32)[:nu], _F(m, "act_hi", np.float32)[:nu]
    rng = np.random.default_rng(seed)
    amp = float(max(np.abs(lo).max(), np.abs(hi).max(), 1e-3)) if nu else 1.0
    us = np.clip(rng.normal(size=(b, h, nu)) * 0.6 * amp, -1.3 * amp, 1.3 * amp).astype(np.float32)
    us[b - 5] = np.float32(0.0)
    us[b - 4] = np.float32(-0.0)
    us[b - 3] = lo
    us[b - 2] = hi
    us[b - 1, 0::2] = np.float32(1.5) * hi
    us[b - 1, 1::2] = np.float32(1.5) * lo
    return us


def init_state(orc, m):
    return orc.forward(m.to_struct(), m.init_q, np.zeros(m.qd_size(), np.float32))


def _free_roots(m):
    return [l for l in range(m.n_links) if int(m.fields["n_rot"][l]) < 0]


# ---- families -------------------------------------------------------------------------------------------------------------
def random_states(orc, m):
    ms = m.to_struct()
    for tier, (a, v) in enumerate(TIERS):
        rng = np.random.default_rng(_seed("random", tier, *_key(m)))
        for i in range(N_RANDOM):
            q = m.init_q.astype(np.float64) + rng.uniform(-a, a, m.q_size())
            qd = rng.uniform(-v, v, m.qd_size())
            for l in _free_roots(m):
                qi = int(m.fields["q_idx"][l])
                r = rng.normal(size=4)
                q[qi + 3:qi + 7] = r / np.linalg.norm(r)
                q[qi + 2] = rng.uniform(-0.1, 2.0)
            yield f"random/tier{tier}/{i}", orc.forward(ms, q.astype(np.float32), qd.astype(np.float32))


def reached_states(orc, m, n=4, steps=50):
    ms = m.to_struct()
    nu = m.act_size()
    lo, hi = _F(m, "act_lo", np.float32)[:nu], _F(m, "act_hi", np.float32)[:nu]
    rng = np.random.default_rng(_seed("reached", *_key(m)))
    us = np.where(rng.random((n, steps, nu)) < 0.5, 1.5 * lo, 1.5 * hi).astype(np.float32)  # saturated, each value held
    us[:, :, :] = np.repeat(us[:, ::5], 5, axis=1)[:, :steps]                               # for five control steps
    _, fin = orc.rollout(ms, init_state(orc, m), us, want_final=True)
    for i in range(n):
        yield f"reached/{i}", fin[i].copy()
    _, fin = orc.rollout(ms, init_state(orc, m), np.zeros((1, 100, nu), np.float32), want_final=True)
    yield "reached/unactuated", fin[0].copy()


def exact_states(orc, m):
    ms = m.to_struct()
    zero = np.zeros(m.qd_size(), np.float32)
    yield "exact/init", init_state(orc, m)
    n_rot, n_slide, q_idx = _F(m, "n_rot", int), _F(m, "n_slide", int), _F(m, "q_idx", int)
    rot_lo, rot_hi, sign = _F(m, "rot_lo", np.float32), _F(m, "rot_hi", np.float32), _F(m, "rot_sign", np.float32)
    for which, lim, d in (("lo", rot_lo, 0.0), ("hi", rot_hi, 0.0), ("lo_beyond", rot_lo, -LIMIT_EPS), ("hi_beyond", rot_hi, LIMIT_EPS)):
        q, n = m.init_q.copy(), 0
        for l in range(m.n_links):
            for k in range(max(int(n_rot[l]), 0)):
                if abs(lim[l, k]) < 100.0:  # (an unlimited hinge carries a huge bound)
                    q[q_idx[l] + n_slide[l] + k] = sign[l, k] * (lim[l, k] + np.float32(d))
                    n += 1
        if n:
            yield f"exact/hinges_{which}", orc.forward(ms, q, zero)
    s_lo, s_hi = _F(m, "slide_lo", np.float32), _F(m, "slide_hi", np.float32)
    for which, lim, d in (("lo", s_lo, 0.0), ("hi", s_hi, 0.0), ("lo_beyond", s_lo, -LIMIT_EPS), ("hi_beyond", s_hi, LIMIT_EPS)):
        q, n = m.init_q.copy(), 0
        for l in range(m.n_links):
            if n_rot[l] < 0:
                continue
            for k in range(int(n_slide[l])):
                if abs(lim[l, k]) < 1e8:  # (mbd_oracle_planar.h: slide_limits)
                    q[q_idx[l] + k] = lim[l, k] + np.float32(d)
                    n += 1
        if n:
            yield f"exact/slides_{which}", orc.forward(ms, q, zero)


def _rot64(q, v):
    w, x, y, z = (float(t) for t in q)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    return R @ np.asarray(v, np.float64)


def lowest_gap(m, state):
    """Height of the lowest point of any collider sphere above the plane (float64 geometry of a float32 state)."""
    n = int(m.fields["n_col"])
    link, pos, rad = _F(m, "col_link", int), _F(m, "col_pos"), _F(m, "col_radius")
    s = np.asarray(state, np.float64)
    return min(s[link[k], 2] + _rot64(s[link[k], 3:7], pos[k])[2] - rad[k] for k in range(n))


def lifted(state, dz):
    s = np.array(state, np.float32)
    s[:, 2] = (s[:, 2].astype(np.float64) + dz).astype(np.float32)
    return s


def hover_state(orc, m, gap):
    """The rest pose translated so that its lowest collider sphere is `gap` above the plane."""
    s = init_state(orc, m)
    return lifted(s, gap - lowest_gap(m, s))


def contact_states(orc, m):
    if int(m.fields["n_col"]) == 0:
        return
    touch = hover_state(orc, m, 0.0)
    yield "contact/touch", touch
    for which, toward in (("above", np.inf), ("below", -np.inf)):
        s = touch.copy()
        s[:, 2] = np.nextafter(s[:, 2], np.float32(toward))
        yield f"contact/touch_one_float_{which}", s
    yield "contact/hover_1mm", hover_state(orc, m, 1e-3)
    yield "contact/sunk_2cm", hover_state(orc, m, -0.02)


def drop_states(orc, m):
    """DROP only.  Link 0 is the sphere (radius r at its centre of mass), the mast's joint error is an exact zero while both
    fall alike, so after the first integration the sphere's centre is z1 = fma(fl(g dt), dt, z0) and pen = r - z1."""
    ms = m.to_struct()
    s0 = init_state(orc, m)
    assert np.all(s0[:, :2] == 0) and np.all(s0[:, 4:7] == 0) and np.all(s0[:, 7:] == 0)
    r, dt, g = np.float32(_F(m, "col_radius")[0]), np.float32(m.fields["dt"]), np.float32(_F(m, "gravity")[2])
    v1 = np.float32(g * dt)

    def z1(z0):
        return np.float32(np.float64(v1) * np.float64(dt) + np.float64(z0))
    z = np.float32(np.float64(r) - np.float64(v1) * np.float64(dt))
    while z1(z) > r:
        z = np.nextafter(z, np.float32(-np.inf))
    while z1(z) < r:
        z = np.nextafter(z, np.float32(np.inf))
    assert z1(z) == r, "no start height puts the penetration at exactly 0"
    for which, zz in (("zero", z), ("one_float_in", np.nextafter(z, np.float32(-np.inf))),
                      ("one_float_out", np.nextafter(z, np.float32(np.inf)))):
        yield f"contact/drop_pen_{which}", lifted(s0, np.float64(zz) - np.float64(s0[0, 2]))
    fall = lifted(s0, 0.05 - lowest_gap(m, s0))
    fall[:, 9] = np.float32(-1.0)
    yield "contact/drop_vertical_fall", fall
    s, a = lifted(s0, -lowest_gap(m, s0)), np.zeros(m.act_size(), np.float32)
    for _ in range(4000):  # to rest: the state that a substep maps onto itself (or the end of the search)
        nxt = orc.substep(ms, s, a)
        if np.array_equal(nxt.view(np.uint32), s.view(np.uint32)):
            break
        s = nxt
    yield "contact/drop_at_rest", s


def _qmul64(a, b):
    aw, ax, ay, az = (float(t) for t in a)
    bw, bx, by, bz = (float(t) for t in b)
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def flipped(state, axis):
    """The whole body turned by exactly 180 degrees about the world axis `axis` (0, 1, 2) through link 0's centre of mass:
    sign changes and permutations only, so the quaternions stay the exact floats they were."""
    s = np.array(state, np.float64)
    c = s[0, :3].copy()
    sg = -np.ones(3)
    sg[axis] = 1.0
    e = np.zeros(4)
    e[1 + axis] = 1.0
    for l in range(s.shape[0]):
        s[l, :3] = c + sg * (s[l, :3] - c)
        s[l, 3:7] = _qmul64(e, s[l, 3:7])
        s[l, 7:10] *= sg
        s[l, 10:13] *= sg
    return s.astype(np.float32)


def orientation_states(orc, m):
    ms = m.to_struct()
    s0 = init_state(orc, m)
    for axis in ((1,) if is_planar(m) else (0, 1, 2)):
        s = flipped(s0, axis)
        yield f"orientation/half_turn_{'xyz'[axis]}", s
        n = s.copy()
        n[0, 3:7] = -n[0, 3:7]
        yield f"orientation/half_turn_{'xyz'[axis]}_root_negated", n
    n_rot, n_slide, q_idx = _F(m, "n_rot", int), _F(m, "n_slide", int), _F(m, "q_idx", int)
    multi = [l for l in range(m.n_links) if n_rot[l] >= 2]
    for which, ang in (("pos", np.pi / 2 - GIMBAL_MARGIN), ("neg", -np.pi / 2 + GIMBAL_MARGIN)):
        for others in ("init", "zero"):
            if not multi:
                break
            q = m.init_q.copy()
            for l in multi:
                a = q_idx[l] + n_slide[l]
                if others == "zero":
                    q[a:a + n_rot[l]] = 0.0
                q[a + 1] = np.float32(ang)
            yield f"orientation/gimbal_{which}_others_{others}", orc.forward(ms, q, np.zeros(m.qd_size(), np.float32))
    parent = _F(m, "parent", int)
    fused = [l for l in range(m.n_links) if n_rot[l] == 0 and n_slide[l] == 0 and parent[l] >= 0]
    for axis in ((1,) if is_planar(m) else (0, 1, 2)):
        if not fused:
            break
        s = s0.astype(np.float64)
        e = np.zeros(4)
        e[1 + axis] = 1.0
        for l in fused:
            s[l, 3:7] = _qmul64(s[l, 3:7], e)  # half a turn about the link's own axis, about its centre of mass
        yield f"orientation/fused_half_turn_{'xyz'[axis]}", s.astype(np.float32)


def raw_states(orc, m):
    s0 = init_state(orc, m)
    rng = np.random.default_rng(_seed("raw", *_key(m)))
    q = (m.init_q + rng.uniform(-0.3, 0.3, m.q_size())).astype(np.float32)
    s1 = orc.forward(m.to_struct(), q, rng.uniform(-1, 1, m.qd_size()).astype(np.float32))
    for k, norm in enumerate(QUAT_NORMS):
        for which, base in (("init", s0), ("moving", s1)):
            if which == "moving" and norm > 1.15:  # (the humanoids and the crab go non-finite from a moving state at 1.2)
                continue
            s = base.copy()
            s[:, 3:7] *= np.float32(norm)
            yield f"raw/quat_norm_{norm}_{which}", s
        s = s1.copy()  # one link only, a different one per norm
        s[k % m.n_links, 3:7] *= np.float32(norm)
        yield f"raw/quat_norm_{norm}_link{k % m.n_links}", s
    for which, v in (("1e-30", 1e-30), ("-1e-30", -1e-30), ("+0", 0.0), ("-0", -0.0)):
        s = s0.copy()
        s[:, 7:] = np.float32(v)
        if is_planar(m):
            s[:, [8, 10, 12]] = 0.0
        yield f"raw/velocities_{which}", s
        if int(m.fields["n_col"]):
            t = hover_state(orc, m, -1e-4)
            t[:, 7:] = s[:, 7:]
            yield f"raw/velocities_{which}_in_contact", t


def cases(orc, m, name="", families=FAMILIES):
    """(case name, state [n_links][13] float32, actions [B][H][Nu] float32) for model `m`; `name`: "drop" adds its own."""
    gens = dict(random=random_states, reached=reached_states, exact=exact_states, contact=contact_states,
                orientation=orientation_states, raw=raw_states)
    for fam in families:
        for case, state in gens[fam](orc, m):
            yield case, np.ascontiguousarray(state, np.float32), actions(m, _seed(case, *_key(m)))
        if fam == "contact" and name == "drop":
            for case, state in drop_states(orc, m):
                yield case, np.ascontiguousarray(state, np.float32), actions(m, _seed(case, *_key(m)))


def mixed_actions(m, b=129):
    """Actions that split one launch: eight kinds of rows in turn — every actuator held at act_hi, at act_lo, every second one
    reversed, halves, zeros — so that from a state hovering just above contact some candidates touch down within the first
    control step and some do not (the caller asserts that on the checker)."""
    nu = m.act_size()
    lo, hi = _F(m, "act_lo", np.float32)[:nu], _F(m, "act_hi", np.float32)[:nu]
    us = np.zeros((b, H, nu), np.float32)
    alt = np.arange(nu) % 2 == 0
    rows = (hi, lo, np.where(alt, hi, lo), np.where(alt, lo, hi), np.float32(0.5) * hi, np.float32(0.5) * lo,
            np.where(alt, hi, 0).astype(np.float32), np.where(alt, 0, lo).astype(np.float32))
    for i in range(b):  # (each block of eight starts one kind later: every two neighbouring kinds meet in an aligned pair)
        us[i] = rows[(i + i // len(rows)) % len(rows)]
    return us


def touches(orc, m, state, us):
    """[b] bool: candidate b's first control step differs from the same step of the model without colliders — a sphere was
    below the plane in one of its substeps."""
    ms, free = m.to_struct(), m.to_struct()
    free.n_col = 0
    return np.array([not np.array_equal(orc.env_step(ms, state, u[0])[0], orc.env_step(free, state, u[0])[0]) for u in us])


def mixed_case(orc, m, gaps=(1e-3, 5e-4, 2e-3, 2.5e-4, 4e-3, 8e-3, 1.6e-2, 1.25e-4, 3.2e-2)):
    """(gap, state, actions) of the first hover height, a millimetre first, at which the first 64 candidates of
    mixed_actions hold both kinds; None where no height of the list splits them (a model without colliders)."""
    if int(m.fields["n_col"]) == 0:
        return None
    us = mixed_actions(m)
    for gap in gaps:
        s = hover_state(orc, m, gap)
        t = touches(orc, m, s, us[:64])
        if t.any() and not t.all():
            return gap, s, us
    return None


# ---- car2d ----------------------------------------------------------------------------------------------------------------
def car2d_cases():
    """(name, q [3], actions [B][H][2]): headings at 0, +-pi, +-pi/2 and far outside [-pi, pi]; positions on, just inside and
    just outside the edge of the obstacle at the origin (radius 0.3) and of the reward's disc around the goal (0.5, 0;
    radius 0.2), inside an obstacle, and at the goal."""
    f = np.float32
    pts = [("start", (-0.5, 0.0))]
    for who, (cx, cy), r in (("obstacle", (0.0, 0.0), 0.3), ("obstacle_row", (-0.9, 0.6), 0.3), ("goal_disc", (0.5, 0.0), 0.2)):
        for dirn, (ux, uy) in (("east", (1, 0)), ("west", (-1, 0)), ("north", (0, 1))):
            x, y = f(cx + ux * r), f(cy + uy * r)
            pts.append((f"{who}_{dirn}_edge", (x, y)))
            pts.append((f"{who}_{dirn}_inside", (np.nextafter(x, f(cx)) if ux else x, np.nextafter(y, f(cy)) if uy else y)))
            pts.append((f"{who}_{dirn}_outside", (np.nextafter(x, f(x + ux)) if ux else x, np.nextafter(y, f(y + uy)) if uy else y)))
    pts += [("inside_obstacle", (0.0, 0.0)), ("goal", (0.5, 0.0))]
    thetas = [("0", 0.0), ("-0", -0.0), ("pi", np.pi), ("-pi", -np.pi), ("pi/2", np.pi / 2), ("-pi/2", -np.pi / 2),
              ("3pi/2", 1.5 * np.pi), ("100", 100.0), ("-1234.5", -1234.5), ("5000", 5000.0)]
    out = [(f"car2d/theta_{tn}", np.array([-0.5, 0.0, tv], f)) for tn, tv in thetas]
    out += [(f"car2d/{pn}_theta_{tn}", np.array([px, py, tv], f)) for pn, (px, py) in pts for tn, tv in thetas[:1] + thetas[4:6]]
    for name, q in out:
        rng = np.random.default_rng(_seed(name))
        us = np.clip(rng.normal(size=(B, H, 2)) * 0.8, -1.3, 1.3).astype(f)
        us[B - 5], us[B - 4], us[B - 3], us[B - 2] = f(0.0), f(-0.0), f(-1.0), f(1.0)
        us[B - 1, 0::2], us[B - 1, 1::2] = f(1.5), f(-1.5)
        yield name, q, us
