"""The numerical-contract primitives (oracle/spec_math.h) against numpy in float64; the kernels' copy of the same
primitives is held to the checker and to the same bounds in tests/test_gpu_math.py."""
import ctypes as C

import numpy as np
import pytest

import math_inputs as mi


def test_atan2_and_asin_accuracy(orc):
    rng = np.random.default_rng(0)
    y = rng.normal(size=5000).astype(np.float32)
    x = rng.normal(size=5000).astype(np.float32)
    got = np.array([orc.lib.orc_sp_atan2(float(a), float(b)) for a, b in zip(y, x)])
    assert np.abs(got - np.arctan2(y.astype(np.float64), x.astype(np.float64))).max() < 4e-7
    assert orc.lib.orc_sp_atan2(0.0, 0.0) == 0.0
    assert abs(orc.lib.orc_sp_atan2(1.0, 0.0) - np.pi / 2) < 2e-7
    assert abs(orc.lib.orc_sp_atan2(0.0, -1.0) - np.pi) < 3e-7
    v = np.linspace(-1, 1, 2001).astype(np.float32)
    got = np.array([orc.lib.orc_sp_asin(float(a)) for a in v])
    assert np.abs(got - np.arcsin(v.astype(np.float64))).max() < 5e-7


def test_sincos_accuracy(orc):
    xs = np.linspace(-40, 40, 8001).astype(np.float32)
    s, c = C.c_float(), C.c_float()
    err = 0.0
    for x in xs:
        orc.lib.orc_sp_sincos(float(x), C.byref(s), C.byref(c))
        err = max(err, abs(s.value - np.sin(np.float64(x))), abs(c.value - np.cos(np.float64(x))))
    assert err < 3e-7


def test_exp_log1p_accuracy(orc):
    xs = np.linspace(-80, 0, 4001).astype(np.float32)
    got = np.array([orc.lib.orc_sp_exp(float(x)) for x in xs])
    ref = np.exp(xs.astype(np.float64))
    assert (np.abs(got - ref) / ref).max() < 3e-7
    assert orc.lib.orc_sp_exp(-100.0) == 0.0
    ts = -np.linspace(0, 0.999999, 4001).astype(np.float32)
    got = np.array([orc.lib.orc_sp_log1p(float(t)) for t in ts])
    ref = np.log1p(ts.astype(np.float64))
    assert (np.abs(got - ref) / np.maximum(np.abs(ref), 1e-30)).max() < 5e-7


def test_rotation_primitives(orc):
    rng = np.random.default_rng(1)
    for _ in range(200):
        q = rng.normal(size=4)
        q = (q / np.linalg.norm(q)).astype(np.float32)
        v = rng.normal(size=3).astype(np.float32)
        out = np.zeros(3, np.float32)
        orc.lib.orc_sp_rot(v, q, out)
        w, x, y, z = q.astype(np.float64)
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        assert np.abs(out - R @ v).max() < 2e-6
        # asymmetric check of the quaternion product: (a*b) rotates like a after b
        b = rng.normal(size=4)
        b = (b / np.linalg.norm(b)).astype(np.float32)
        ab = np.zeros(4, np.float32)
        orc.lib.orc_sp_qmul(q, b, ab)
        o1, o2, o3 = np.zeros(3, np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32)
        orc.lib.orc_sp_rot(v, b, o1)
        orc.lib.orc_sp_rot(o1, q, o2)
        orc.lib.orc_sp_rot(v, ab, o3)
        assert np.abs(o2 - o3).max() < 3e-6


def test_canonical_sum_is_strided_then_butterfly(orc):
    x = np.random.default_rng(2).normal(size=1000).astype(np.float32)
    part = np.zeros(64, np.float32)
    for i, v in enumerate(x):
        part[i & 63] = np.float32(part[i & 63] + v)
    a = part.copy()
    off = 32
    while off >= 1:
        a = np.array([np.float32(a[j] + a[j ^ off]) for j in range(64)], np.float32)
        off >>= 1
    assert orc.lib.orc_sp_sum(x, 1000) == a[0]


def test_car2d_collision_threshold_is_the_sqrt_comparison():
    """csrc/mbd_kernels.h (car2d_rollout_kernel) tests `dx*dx + dy*dy < T` where car2d.py:84 and the checker compare
    `sqrt(dx*dx + dy*dy) < 0.3f`: T = 0x3db851ec is the smallest float32 whose correctly rounded square root is >= 0.3f,
    and the correctly rounded square root is monotonic — checked here on every float32 in [0.0899, 0.0901]."""
    c = np.float32(0.3)
    lo, hi = np.float32(0.0899), np.float32(0.0901)
    bits = np.arange(lo.view(np.uint32), hi.view(np.uint32) + 1, dtype=np.uint32)
    xs = bits.view(np.float32)
    s = np.sqrt(xs)  # float32: IEEE, correctly rounded
    T = np.uint32(0x3DB851EC).view(np.float32)
    assert float(T) == 0.09000000357627869
    assert np.array_equal(s < c, xs < T)
    assert np.all(np.diff(s) >= 0)


# ---- every primitive of the contract, by the kernels' names, against float64 (tests/math_inputs.py) ------------------
SP_OPS = ["rcp_exact", "div_", "div_pos_", "div2_", "div2_pos_", "div2_sp_", "div2x2_", "div2x2_sp_", "sqrt_floor",
          "angle_unit", "angle_unit_cpos", "angle_unit2", "sincos_", "exp_", "log_", "log1p_", "erfinv_",
          "bits_to_uniform", "bits_to_normal", "qnormalize", "qnormalize_qm<1>", "qnormalize_qm<2>", "qrotvec_raw",
          "qrotvec", "rot", "irot", "irot_z", "qmul", "qaxes", "dot", "cross", "rot2", "qmul2", "qaxes2", "dot2", "cross2",
          "fmin_", "fmax_", "fclip"]


def test_checker_names_every_primitive(orc):
    assert orc.sp_ops() == SP_OPS


@pytest.mark.parametrize("op", SP_OPS)
def test_checker_primitive_against_float64(orc, op):
    """The checker's copy (oracle/spec_math.h) on the op's whole input set: exact where the contract is IEEE (division,
    square root, the uniform bit trick), within a bound just above its measured worst case elsewhere — so that a shared
    mistake of both copies (a mistyped coefficient, a wrong octant) fails here, where bit-equality cannot see it."""
    x = mi.inputs(op)
    mi.check_contract(op, x, orc.sp_eval(op, x))


@pytest.mark.parametrize("defect", [1e-7, -1e-6, 1e-6, 1e-5, -3e-5])
def test_angle_unit_error_grows_with_the_norm_defect(orc, defect):
    """3.4e-7 at a defect of 1e-7, 1.2e-6 at 1e-6, 1.0e-5 at 1e-5: bounded by 3e-7 + 1.05 |defect|."""
    x = mi.angle_inputs(defect, n=1 << 20)
    mi.check_angle(x, orc.sp_eval("angle_unit", x), rounded=False)


def test_angle_unit_signed_zeros_follow_arctan2(orc):
    s = np.float32([0.0, -0.0, 0.0, -0.0])
    c = np.float32([-1.0, -1.0, 1.0, 1.0])
    got = orc.sp_eval("angle_unit", mi.pairs(s, c))
    want = np.arctan2(s, c)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)  # +-pi and +-0


def test_sampler_uniforms_are_jax_bit_trick(orc):
    """All 2^23 sampler uniforms of mi.sampler_uniforms (numpy's restatement of the bit trick) are what the checker's
    bits_to_uniform makes of the same bits, and they lie in [nextafter(-1, 0), 1)."""
    u, b = mi.sampler_uniforms()
    lo = np.float32(-0.99999994)
    got = orc.sp_eval("bits_to_uniform", mi.pairs(b.view(np.float32), np.full(b.size, lo), np.ones(b.size)))
    assert np.array_equal(got.view(np.uint32), u.view(np.uint32))
    assert u.min() == lo and u.max() < 1.0 and np.unique(u).size > (1 << 22)
