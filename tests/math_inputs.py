"""Inputs, float64 references and error bounds of the numerical-contract primitives, by the names of csrc/mbd_math.h.

Shared by tests/test_spec_math.py (the checker's copy, oracle/spec_math.h, on the CPU) and tests/test_gpu_math.py (the
kernels' copy through mbd_debug_eval_math): both copies are fed the same arrays and held to the same bounds.

Inputs cover the domain the kernels feed each primitive: a strided sweep of float32 bit patterns (a prime stride, so every
exponent and every low mantissa pattern appears), exhaustive windows of +-4096 floats around every constant and branch
point of the code, and the signed zeros a caller can produce.
"""
import numpy as np

N_SWEEP = 1 << 24
WIN = 4096
STRIDE = 2654435761  # prime
F32_MAX = np.finfo(np.float32).max


def bits(x) -> np.uint32:
    return np.float32(x).view(np.uint32)


def sweep(lo, hi, n=N_SWEEP, offset=0):
    """n float32 values of [lo, hi] (0 <= lo < hi) whose bit patterns step through the range by a prime stride."""
    a, b = int(bits(lo)), int(bits(hi))
    k = np.arange(n, dtype=np.uint64) + np.uint64(offset)
    return (np.uint64(a) + (k * np.uint64(STRIDE)) % np.uint64(b - a + 1)).astype(np.uint32).view(np.float32)


def window(x, w=WIN):
    """The 2w + 1 float32 values nearest to x (x != 0), on both sides of it."""
    x = np.float32(x)
    b = np.int64(bits(abs(x))) + np.arange(-w, w + 1, dtype=np.int64)
    v = b[b > 0].astype(np.uint32).view(np.float32)
    return -v if x < 0 else v


def signed(v, seed):
    """v with random signs."""
    s = np.random.default_rng(seed).integers(0, 2, v.size).astype(bool)
    return np.where(s, -v, v).astype(np.float32)


def pairs(*cols):
    return np.ascontiguousarray(np.stack([np.asarray(c, np.float32) for c in cols], axis=1))


def ulp(ref):
    """float32 unit in the last place at |ref| (float64 ref)."""
    return np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


def unit_quats(n, seed):
    q = np.random.default_rng(seed).normal(size=(n, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def rotmat(q):
    """float64 rotation matrices of the (not necessarily unit) quaternions q [n][4] by the contract's formula (what
    v + w t + u x t computes exactly; for a unit q, R(q))."""
    w, x, y, z = (q[:, k].astype(np.float64) for k in range(4))
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], 1)


def qmul64(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    aw, ax, ay, az = a.T
    bw, bx, by, bz = b.T
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], 1)


# ---- inputs ---------------------------------------------------------------------------------------------------------
def div_inputs():
    """(n, d): numerators of either sign in [0, 1e10] and at the 1e-28 flush / clamp edge, signed zeros; denominators of
    either sign in the contract's [1e-20, 1e10] (mantissas all ones / all zeros included)."""
    num = np.concatenate([signed(sweep(0.0, 1e10), 1), window(1e-28), window(-1e-28), np.float32([0.0, -0.0, 1e-28, -1e-28])])
    rng = np.random.default_rng(2)
    den = signed(sweep(1e-20, 1e10, num.size, offset=12345), 3)
    e = np.arange(int(bits(1e-20)) >> 23, (int(bits(1e10)) >> 23) + 1, dtype=np.uint32)
    hard = np.concatenate([(e << 23), (e << 23) | 0x7FFFFF]).view(np.float32)
    hard = hard[(hard >= np.float32(1e-20)) & (hard <= np.float32(1e10))]
    idx = rng.integers(0, num.size, 2 * hard.size)
    den[idx] = np.concatenate([hard, -hard])
    return pairs(num, den)


def rcp_inputs():
    """d in [1e-20, 1e20] of either sign, with every exponent's mantissa all ones / all zeros."""
    e = np.arange(int(bits(1e-20)) >> 23, (int(bits(1e20)) >> 23) + 1, dtype=np.uint32)
    hard = np.concatenate([(e << 23), (e << 23) | 0x7FFFFF]).view(np.float32)
    hard = hard[(hard >= np.float32(1e-20)) & (hard <= np.float32(1e20))]
    d = np.concatenate([sweep(1e-20, 1e20), hard, window(1e-20)[WIN:], window(1e20)[:WIN + 1]])
    return signed(d, 4)


def sqrt_inputs():
    """x in [0, FLT_MAX], the 1e-30 clamp edge, signed zeros and small negatives (clamped too)."""
    return np.concatenate([sweep(0.0, F32_MAX), window(1e-30), np.float32([0.0, -0.0, -1e-30, -1.0, 1e-30])])


def angle_inputs(defect=0.0, n=N_SWEEP, seed=5):
    """(s, c) = the correctly rounded (sin t, cos t) * (1 + defect) for t swept over [-pi, pi], plus windows around the
    swap line |s| = |c| (t = +-pi/4, +-3pi/4) and the axes, and the signed zeros of c and s."""
    t = np.linspace(-np.pi, np.pi, n)
    for t0 in (np.pi / 4, 3 * np.pi / 4, -np.pi / 4, -3 * np.pi / 4, np.pi / 2, -np.pi / 2, 0.0, np.pi):
        t = np.concatenate([t, t0 + np.arange(-WIN, WIN + 1) * 2.0 ** -26])
    s, c = np.sin(t) * (1 + defect), np.cos(t) * (1 + defect)
    x = pairs(s, c)
    z = np.float32([[0.0, 1.0], [-0.0, 1.0], [0.0, -1.0], [-0.0, -1.0], [1.0, 0.0], [1.0, -0.0], [-1.0, 0.0],
                    [-1.0, -0.0], [0.0, 0.0], [-0.0, 0.0], [0.0, -0.0], [-0.0, -0.0]])
    return np.concatenate([x, z])


def angle_cpos_inputs():
    """angle_inputs with c >= 0 (the caller's c is a square root)."""
    x = angle_inputs()
    x[:, 1] = np.abs(x[:, 1])
    return x


def sincos_inputs():
    """x in [-1e5, 1e5] (strided bit patterns, random signs), windows around the reduction's rounding boundaries
    (k + 1/2) pi/2 for k in [-64, 64) and a few far ones, signed zeros."""
    x = [signed(sweep(0.0, 1e5), 6), np.float32([0.0, -0.0])]
    for k in list(range(-64, 64)) + [-40000, -12345, 999, 40000, 63661]:
        x.append(window((k + 0.5) * np.pi / 2, 512))
    return np.concatenate(x)


def exp_inputs():
    """x in [-100, 88.7] (both cut-offs: -87 -> 0, > 88.7 -> inf) with windows around -87 and 88.7, -inf, signed zeros."""
    x = np.concatenate([-sweep(0.0, 100.0), sweep(0.0, 88.7, 1 << 20), window(-87.0), window(88.7),
                        np.float32([0.0, -0.0, -np.inf])])
    return x


def log_inputs():
    """x over the positive normal floats (log1p_ feeds it u in [2^-24, 1)), windows around the mantissa switch
    m = sqrt(1/2) of the exponents around 1 and around 1 itself."""
    x = [sweep(np.finfo(np.float32).tiny, F32_MAX), window(1.0)]
    for e in range(-24, 3):
        x.append(window(np.sqrt(0.5) * 2.0 ** e, 512))
    return np.concatenate(x)


def log1p_inputs():
    """t in (-1, 0] (strided), windows around u = 1 + t == 1 (t ~ -2^-25) and u <= 0 (t ~ -1), signed zeros, -1."""
    t = np.concatenate([-sweep(0.0, np.float32(1.0) - np.float32(2.0 ** -24)), -window(2.0 ** -25), window(-1.0),
                        np.float32([0.0, -0.0, -1.0])])
    return t[t >= -1.0]


def sampler_uniforms():
    """All 2^23 float32 uniforms jax.random.normal's sampler can produce: uniform(nextafter(-1, 0), 1) of every 23-bit
    mantissa (numpy's float32 restatement of the bit trick)."""
    b = np.arange(1 << 23, dtype=np.uint32) << 9
    return bits_to_uniform_np(b, np.float32(-0.99999994), np.float32(1.0)), b


def bits_to_uniform_np(b, lo, hi):
    """jax.random.uniform's bit trick in float32: (bits >> 9 | 0x3F800000) as float - 1, * (hi - lo) + lo, max(lo, .)."""
    lo, hi = np.float32(lo), np.float32(hi)
    f = ((b >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1.0)
    return np.maximum(lo, f * (hi - lo) + lo).astype(np.float32)


def erfinv_inputs():
    """every sampler uniform, plus windows around the polynomial switch w = -log1p(-x^2) = 5 on both signs, and +-1."""
    u, _ = sampler_uniforms()
    x5 = np.sqrt(1 - np.exp(-5.0))
    return np.concatenate([u, window(x5), window(-x5), np.float32([1.0, -1.0, 0.0, -0.0])])


def uniform_bits_inputs():
    """(bits as a float32 bit pattern, min, max): 2^24 strided 32-bit patterns under the sampler's and three other ranges."""
    k = np.arange(N_SWEEP, dtype=np.uint64)
    b = ((k * np.uint64(STRIDE)) % np.uint64(1 << 32)).astype(np.uint32)
    ranges = np.float32([[-0.99999994, 1.0], [0.0, 1.0], [-1.0, 1.0], [-3.5, 0.25]])
    r = ranges[np.arange(N_SWEEP) % 4]
    return np.ascontiguousarray(np.stack([b.view(np.float32), r[:, 0], r[:, 1]], 1))


def qnorm_inputs(n=1 << 20, seed=7):
    """quaternions with |q|^2 - 1 = e: random e in [-0.3, 0.3], and e on +-4096 steps of 2^-23 around the +-0.05 switch
    (the rounded n^2 - 1 then lands on both sides of it), plus exact unit axes."""
    rng = np.random.default_rng(seed)
    e = np.concatenate([rng.uniform(-0.3, 0.3, n), 0.05 + np.arange(-WIN, WIN + 1) * 2.0 ** -23,
                        -0.05 + np.arange(-WIN, WIN + 1) * 2.0 ** -23, np.zeros(1024)])
    d = rng.normal(size=(e.size, 4))
    q = d / np.linalg.norm(d, axis=1, keepdims=True) * np.sqrt(1 + e)[:, None]
    return np.concatenate([q.astype(np.float32), np.eye(4, dtype=np.float32), -np.eye(4, dtype=np.float32)])


def qrotvec_inputs(n=1 << 20, seed=8):
    """(unit q, th) with |th| up to 1.2 rad: both sides of the renormalisation's switch (|th|^2 / 4 = 0.05 at 0.447)."""
    rng = np.random.default_rng(seed)
    th = rng.normal(size=(n, 3))
    th *= (rng.uniform(0, 1.2, n) / np.linalg.norm(th, axis=1))[:, None]
    return np.concatenate([unit_quats(n, seed + 1), th.astype(np.float32)], 1)


def rot_inputs(n=1 << 20, seed=9):
    """(v, unit q): v of magnitudes 1e-3 ... 1e3."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-3, 3, (n, 1))
    return np.concatenate([v.astype(np.float32), unit_quats(n, seed + 1)], 1)


def irot_z_inputs(n=1 << 20, seed=10):
    rng = np.random.default_rng(seed)
    d = (rng.normal(size=n) * 10.0 ** rng.uniform(-3, 3, n)).astype(np.float32)
    return np.concatenate([d[:, None], unit_quats(n, seed + 1)], 1)


def qmul_inputs(n=1 << 20, seed=11):
    return np.concatenate([unit_quats(n, seed), unit_quats(n, seed + 1)], 1)


def vec_pair_inputs(n=1 << 20, seed=12):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(n, 6)) * 10.0 ** rng.uniform(-2, 2, (n, 1))).astype(np.float32)


def minmax_inputs(k, seed=13):
    """k operands: random finite values, equal operands, and every arrangement of signed zeros (lo <= hi for fclip)."""
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=(1 << 16, k)) * 10.0 ** rng.uniform(-3, 3, (1 << 16, 1))).astype(np.float32)
    if k == 3:
        x[:, 1:] = np.sort(x[:, 1:], axis=1)
    eq = np.repeat(x[:256, :1], k, 1)
    z = np.array(np.meshgrid(*[[0.0, -0.0, 1.0, -1.0]] * k)).reshape(k, -1).T.astype(np.float32)
    if k == 3:
        z = z[z[:, 1] <= z[:, 2]]
    return np.concatenate([x, eq, z])


def inputs(op):
    """The input array [n][k_in] (or [n]) of primitive `op`."""
    table = {
        "rcp_exact": rcp_inputs, "sqrt_floor": sqrt_inputs, "sincos_": sincos_inputs, "exp_": exp_inputs,
        "log_": log_inputs, "log1p_": log1p_inputs, "erfinv_": erfinv_inputs, "bits_to_uniform": uniform_bits_inputs,
        "bits_to_normal": lambda: sampler_uniforms()[1].view(np.float32),
        "angle_unit_cpos": angle_cpos_inputs,
        "qrotvec_raw": qrotvec_inputs, "qrotvec": qrotvec_inputs, "irot_z": irot_z_inputs,
        "fmin_": lambda: minmax_inputs(2), "fmax_": lambda: minmax_inputs(2), "fclip": lambda: minmax_inputs(3),
    }
    for name in ("div_", "div_pos_", "div2_", "div2_pos_", "div2_sp_"):
        table[name] = div_inputs
    for name in ("div2x2_", "div2x2_sp_"):
        table[name] = lambda: np.concatenate([div_inputs(), div_inputs()[::-1]], 1)
    for name in ("angle_unit", "angle_unit2"):
        table[name] = angle_inputs
    for name in ("qnormalize", "qnormalize_qm<1>", "qnormalize_qm<2>", "qaxes", "qaxes2"):
        table[name] = qnorm_inputs
    for name in ("rot", "irot", "rot2"):
        table[name] = rot_inputs
    for name in ("qmul", "qmul2"):
        table[name] = qmul_inputs
    for name in ("dot", "dot2", "cross", "cross2"):
        table[name] = vec_pair_inputs
    return table[op]()


# ---- float64 references and bounds ------------------------------------------------------------------------------------
# Each bound sits just above the worst case the contract's copies measure on these inputs, so that a mistyped coefficient or
# a wrong branch fails.  Division, square root and the uniform bit trick are exact: bit for bit against IEEE float32.
F32_PI = np.float32(np.pi)


def _eq_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _max(err, name):
    return f"{name}: max {float(np.max(err)):.4g}"


def _flush(n):
    return np.where(np.abs(n) < np.float32(1e-28), np.float32(0.0), n).astype(np.float32)


def _clamp(n):
    return np.maximum(n, np.float32(1e-28)).astype(np.float32)


def expected_division(op, x):
    """The IEEE float32 quotients the division ops must equal bit for bit (after the documented flush / clamp)."""
    even = (np.arange(x.shape[0]) % 2 == 0)
    if op in ("div_", "div2_"):
        return _flush(x[:, 0]) / x[:, 1]
    if op in ("div_pos_", "div2_pos_"):
        return _clamp(x[:, 0]) / x[:, 1]
    if op == "div2_sp_":  # the signed numerator in the low half of each pair, the non-negative one in the high half
        return np.where(even, _flush(x[:, 0]), _clamp(x[:, 0])) / x[:, 1]
    if op == "div2x2_":
        return np.stack([_clamp(x[:, 0]) / x[:, 1], _clamp(x[:, 2]) / x[:, 3]], 1)
    if op == "div2x2_sp_":
        return np.stack([_flush(x[:, 0]) / x[:, 1], _clamp(x[:, 2]) / x[:, 3]], 1)
    raise KeyError(op)


def check_angle(x, y, rounded=True, bound_unit=2.95e-7, slope=1.05, floor=3e-7):
    """angle_unit(s, c) against atan2 in float64: within bound_unit on correctly rounded unit vectors (rounded), within
    floor + slope * | |(s, c)| - 1 | on vectors with a norm defect (the asin of the smaller component sees the norm defect directly);
    signed zeros as np.arctan2: (+-0, 1) -> +-0, (+-0, -1) -> +-pi; the zero vector gives s back (+-0)."""
    s, c = x[:, 0].astype(np.float64), x[:, 1].astype(np.float64)
    zero = (s == 0) & (c == 0)
    assert _eq_bits(y[zero], x[zero, 0]), "angle of the zero vector"
    ref = np.arctan2(s, c)
    err = np.abs(y - ref)[~zero]
    defect = np.abs(np.hypot(s, c) - 1)[~zero]
    if rounded:
        assert err.max() <= bound_unit, _max(err, "angle_unit on rounded unit vectors")
    assert np.all(err <= floor + slope * defect), _max(err - slope * defect, "angle_unit: error - slope * defect")
    for sv, cv, want in ((0.0, 1.0, 0.0), (-0.0, 1.0, -0.0), (0.0, -1.0, F32_PI), (-0.0, -1.0, -F32_PI)):
        m = (x[:, 0].view(np.uint32) == np.float32(sv).view(np.uint32)) & (x[:, 1] == cv)
        if m.any():
            assert _eq_bits(y[m], np.full(m.sum(), want, np.float32)), (sv, cv)
            assert np.all(y[m] == np.arctan2(np.float32(sv), np.float32(cv)))


def check_contract(op, x, y):
    """Assert that y = op(x) (either copy of the contract) is within op's float64 bound, or exact where the contract says so."""
    from scipy import special
    with np.errstate(invalid="ignore"):  # (bits_to_uniform and _normal carry raw bit patterns)
        x64 = x.astype(np.float64)
    if op == "rcp_exact":
        assert _eq_bits(y, np.float32(1.0) / x), op
    elif op.startswith("div"):
        assert _eq_bits(y, expected_division(op, x)), op
    elif op == "sqrt_floor":
        assert _eq_bits(y, np.sqrt(np.maximum(x, np.float32(1e-30)))), op
    elif op in ("angle_unit", "angle_unit2", "angle_unit_cpos"):
        check_angle(x, y)
    elif op == "sincos_":
        m = np.abs(x) <= 1e5
        err = np.maximum(np.abs(y[:, 0] - np.sin(x64)), np.abs(y[:, 1] - np.cos(x64)))[m]
        assert err.max() <= 9.4e-8, _max(err, op)
        z = x == 0
        assert np.all(y[z, 0] == 0.0) and np.all(y[z, 1] == 1.0), "sincos of +-0"
    elif op == "exp_":
        ref = np.exp(x64)
        m = (x >= -87.0) & (x <= 88.7)
        err = np.abs(y[m] - ref[m]) / ulp(ref[m])
        assert err.max() <= 1.02, _max(err, "exp_ in ulp")
        assert np.all(y[x < -87.0] == 0.0) and np.all(np.isposinf(y[x > 88.7])), "exp_ cut-offs"
        assert np.all(y[x == 0] == 1.0)
    elif op == "log_":
        ref = np.log(x64)
        m = ref != 0
        err = np.abs(y[m] - ref[m]) / ulp(ref[m])
        assert err.max() <= 0.85, _max(err, "log_ in ulp")
        assert np.all(y[~m] == 0.0)
    elif op == "log1p_":
        inner = x > -1
        ref = np.log1p(x64[inner])
        m = ref != 0
        err = np.abs(y[inner][m] - ref[m]) / ulp(ref[m])
        assert err.max() <= 2.02, _max(err, "log1p_ in ulp")
        z = x == 0
        assert _eq_bits(y[z], x[z]), "log1p_(+-0) = +-0"
        assert np.all(np.isneginf(y[x == -1.0])), "log1p_(-1) = -inf"
    elif op == "erfinv_":
        check_erfinv(x, y)
    elif op == "bits_to_uniform":
        assert _eq_bits(y, bits_to_uniform_np(x[:, 0].view(np.uint32), x[:, 1], x[:, 2])), op
        # (per range: every row lies in [min, max))
    elif op == "bits_to_normal":
        u = bits_to_uniform_np(x.view(np.uint32), np.float32(-0.99999994), np.float32(1.0))
        ref = np.sqrt(2.0) * special.erfinv(u.astype(np.float64))
        m = ref != 0
        rel = np.abs(y[m] - ref[m]) / np.abs(ref[m])
        assert rel.max() <= 5.9e-6, _max(rel, op)  # XLA's ErfInv tail (check_erfinv)
    elif op in ("qnormalize", "qnormalize_qm<2>", "qnormalize_qm<1>"):
        ref = x64 / np.linalg.norm(x64, axis=1, keepdims=True)
        n2m1 = np.abs((x64 * x64).sum(1) - 1)
        if op == "qnormalize_qm<1>":
            # the series side unconditionally: the normalised values where |n2 - 1| <= 0.05 (a rollout re-runs the
            # control step otherwise); `worst` = |fl(n2) - 1|: n2's four-term fma chain rounds it by a few ulp of n2
            assert np.all(np.abs(y[:, 4] - n2m1) <= 3.5 * 2.0 ** -24 * (1 + n2m1)), "qnormalize_qm<1> worst"
            m = y[:, 4] <= 0.05
            err = np.abs(y[m, :4] - ref[m])
        else:
            err = np.abs(y - ref)
        assert err.max() <= 1.85e-7, _max(err, op)
    elif op in ("qrotvec_raw", "qrotvec"):
        q, th = x64[:, :4], np.concatenate([np.zeros((x.shape[0], 1)), x64[:, 4:]], 1)
        ref = q + 0.5 * qmul64(th, q)
        if op == "qrotvec":
            ref /= np.linalg.norm(ref, axis=1, keepdims=True)
        err = np.abs(y - ref)
        assert err.max() <= (1.75e-7 if op == "qrotvec_raw" else 1.85e-7), _max(err, op)
    elif op in ("rot", "rot2", "irot"):
        q = x[:, 3:].copy()
        if op == "irot":
            q[:, 1:] *= -1
        ref = np.einsum("nij,nj->ni", rotmat(q), x64[:, :3])
        err = np.abs(y - ref).max(1) / np.linalg.norm(x64[:, :3], axis=1)
        assert err.max() <= 3.3e-7, _max(err, op)
    elif op == "irot_z":
        ref = rotmat(x[:, 1:])[:, 2, :] * x64[:, :1]
        err = np.abs(y - ref).max(1) / np.abs(x64[:, 0])
        assert err.max() <= 3.4e-7, _max(err, op)
    elif op in ("qmul", "qmul2"):
        err = np.abs(y - qmul64(x[:, :4], x[:, 4:]))
        assert err.max() <= 1.2e-7, _max(err, op)
    elif op in ("qaxes", "qaxes2"):
        R = rotmat(x)
        err = np.abs(y - np.concatenate([R[:, :, 0], R[:, :, 1], R[:, :, 2]], 1))
        assert err.max() <= 2.55e-7, _max(err, op)
    elif op in ("dot", "dot2"):
        a, b = x64[:, :3], x64[:, 3:]
        err = np.abs(y - (a * b).sum(1)) / (np.abs(a) * np.abs(b)).sum(1)
        assert err.max() <= 1.6e-7, _max(err, op)
    elif op in ("cross", "cross2"):
        a, b = x64[:, :3], x64[:, 3:]
        err = np.abs(y - np.cross(a, b)).max(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
        assert err.max() <= 1.15e-7, _max(err, op)
    elif op == "fmin_":
        assert np.all(y == np.minimum(x[:, 0], x[:, 1])), op
    elif op == "fmax_":
        assert np.all(y == np.maximum(x[:, 0], x[:, 1])), op
    elif op == "fclip":
        assert np.all(y == np.clip(x[:, 0], x[:, 1], x[:, 2])), op
    else:
        raise KeyError(op)


def check_erfinv(x, y):
    """XLA's f32 ErfInv polynomial (Giles) against float64 erfinv.  Its error in the far tail is XLA's own — JAX samples
    with it — and the contract keeps it: the bounds pin it, they do not ask for better."""
    from scipy import special
    ref = special.erfinv(x.astype(np.float64))
    ax = np.abs(x)
    assert np.all(y[ax == 1.0] == x[ax == 1.0] * np.inf), "erfinv_(+-1) = +-inf"
    z = x == 0
    assert _eq_bits(y[z], x[z]), "erfinv_(+-0) = +-0"
    m = (ax < 1.0) & (ref != 0)
    err = np.abs(y[m] - ref[m]) / ulp(ref[m])
    for lim, bound in ((0.9, 3.75), (0.99, 4.95), (1.0, 65.5)):
        assert err[ax[m] < lim].max() <= bound, _max(err[ax[m] < lim], f"erfinv_ |u| < {lim}, ulp")
    rel = np.abs(y[m] - ref[m]) / np.abs(ref[m])
    assert rel.max() <= 5.9e-6, _max(rel, "erfinv_ relative")  # worst at u = 0.99982744: 65 ulp, 5.8e-6
