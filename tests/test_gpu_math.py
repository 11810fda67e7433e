"""The kernels' copy of the numerical contract (csrc/mbd_math.h), primitive by primitive, on the MI355X.

mbd_debug_eval_math runs one primitive of the library as built (same flags, same assembly pass) over arrays.  Each op gets
the inputs of tests/math_inputs.py — strided sweeps, windows around every branch point, signed zeros — and must
  (a) equal the checker's copy (oracle/spec_math.h through orc_sp_eval) bit for bit, -0 != +0;
  (b) meet the same float64 bounds as the checker (tests/test_spec_math.py), asserted on the device's own output;
  (c) for a packed op, equal its scalar op bit for bit;
  (d) for the renormalisation's speculative forms, equal qnormalize / report |n2 - 1| exactly.
The whole-plan tests only see the values a rollout happens to produce; these see every branch of every primitive."""
import numpy as np
import pytest

import math_inputs as mi

pytestmark = pytest.mark.gpu

OPS = ["rcp_exact", "div_", "div_pos_", "div2_", "div2_pos_", "div2_sp_", "div2x2_", "div2x2_sp_", "sqrt_floor",
       "angle_unit", "angle_unit_cpos", "angle_unit2", "sincos_", "exp_", "log_", "log1p_", "erfinv_", "bits_to_uniform",
       "bits_to_normal", "qnormalize", "qnormalize_qm<1>", "qnormalize_qm<2>", "qrotvec_raw", "qrotvec", "rot", "irot",
       "irot_z", "qmul", "qaxes", "dot", "cross", "rot2", "qmul2", "qaxes2", "dot2", "cross2", "fmin_", "fmax_", "fclip"]
# packed op -> the scalar op whose values it must have on the same inputs
PACKED = {"div2_": "div_", "div2_pos_": "div_pos_", "angle_unit2": "angle_unit", "rot2": "rot", "qmul2": "qmul",
          "qaxes2": "qaxes", "dot2": "dot", "cross2": "cross"}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b, what):
    a, b = _bits(a), _bits(b)
    assert a.shape == b.shape, what
    bad = np.flatnonzero((a != b).reshape(a.shape[0], -1).any(1))
    assert bad.size == 0, f"{what}: {bad.size} rows differ, first at row {bad[0]}: {a[bad[0]]} vs {b[bad[0]]}"


@pytest.fixture(scope="module")
def gpu(lib):
    from mbd_hip import _capi
    if _capi.device_count() < 1:
        pytest.fail("tests/test_gpu_math.py needs a GPU")
    return _capi


@pytest.fixture(scope="module")
def evals(gpu, orc):
    """op -> (inputs, device output, checker output); inputs and device outputs are kept for the later comparisons."""
    cache = {}

    def get(op):
        if op in cache:
            x, y = cache[op]
            return x, y, orc.sp_eval(op, x)
        x = mi.inputs(op)
        cache[op] = x, gpu.debug_eval_math(op, x)
        return cache[op] + (orc.sp_eval(op, x),)
    return get


def test_the_library_and_the_checker_name_the_same_primitives(gpu, orc):
    assert gpu.debug_math_ops() == OPS == orc.sp_ops()
    for op in OPS:
        assert gpu.debug_math_arity(op) == orc.sp_arity(op), op


@pytest.mark.parametrize("op", OPS)
def test_primitive_matches_the_checker_and_float64(evals, op):
    x, y, ref = evals(op)
    if op == "qnormalize_qm<1>":
        # (the speculative series side: the checker's values where |n2 - 1| <= 0.05; beyond, a rollout re-runs the step)
        ok = y[:, 4] <= 0.05
        assert ok.sum() > 100000 and (~ok).sum() > 100000
        _same_bits(y[ok, :4], ref[ok, :4], op)
        _same_bits(y[:, 4], ref[:, 4], op + " worst")
    elif op in ("fmin_", "fmax_", "fclip"):
        # v_min / v_max / v_med3 order -0 below +0; the checker's selects see a tie.  They differ in the sign of a zero
        # result only, where the operands are zeros of both signs: pinned in test_min_max_clip_order_signed_zeros.
        diff = np.flatnonzero(_bits(y) != _bits(ref))
        assert np.all(y[diff] == 0) and np.all(ref[diff] == 0), op
        keep = np.setdiff1d(np.arange(y.size), diff)
        _same_bits(y[keep], ref[keep], op)
    else:
        _same_bits(y, ref, op)
    mi.check_contract(op, x, y)


@pytest.mark.parametrize("op", sorted(PACKED))
def test_packed_primitive_equals_its_scalar_form(evals, op):
    x, y, _ = evals(op)
    _, ys, _ = evals(PACKED[op])
    _same_bits(y, ys, f"{op} vs {PACKED[op]}")


def test_packed_divisions_equal_the_scalar_divisions(gpu, evals):
    """div2_sp_: div_ in the low half of each pair, div_pos_ in the high half; div2x2_: two div2_pos_ quotients per half,
    div2x2_sp_ two div2_sp_-style ones."""
    x, y, _ = evals("div2_sp_")
    even = np.arange(x.shape[0]) % 2 == 0
    _same_bits(y, np.where(even, gpu.debug_eval_math("div_", x), gpu.debug_eval_math("div_pos_", x)), "div2_sp_")
    for op, first in (("div2x2_", "div_pos_"), ("div2x2_sp_", "div_")):
        x, y, _ = evals(op)
        _same_bits(y[:, 0], gpu.debug_eval_math(first, x[:, :2]), op + " first pair")
        _same_bits(y[:, 1], gpu.debug_eval_math("div_pos_", x[:, 2:]), op + " second pair")


def test_angle_unit_cpos_is_angle_unit_for_nonnegative_c(gpu, evals):
    x, y, _ = evals("angle_unit_cpos")
    assert np.all(x[:, 1] >= 0)
    _same_bits(y, gpu.debug_eval_math("angle_unit", x), "angle_unit_cpos vs angle_unit")


def test_speculative_renormalisation(evals):
    """qnormalize_qm<2> has the values of qnormalize (both sides computed, the exact one selected beyond |n2 - 1| = 0.05);
    qnormalize_qm<1> reports worst = |n2 - 1| exactly, the quantity the rollouts compare with 0.05, on both sides of it."""
    x, q, _ = evals("qnormalize")
    _, q2, _ = evals("qnormalize_qm<2>")
    _, q1, orc1 = evals("qnormalize_qm<1>")
    _same_bits(q2, q, "qnormalize_qm<2> vs qnormalize")
    _same_bits(q1[:, 4], orc1[:, 4], "qnormalize_qm<1> worst")
    near = np.abs(q1[:, 4] - 0.05) < 2e-4
    assert (q1[near, 4] > 0.05).sum() > 100 and (q1[near, 4] <= 0.05).sum() > 100  # the window straddles the switch
    series = q1[:, 4] <= 0.05
    _same_bits(q1[series, :4], q[series], "qnormalize_qm<1> vs qnormalize on the series side")


def test_angle_defects_within_the_bound(gpu, orc):
    """angle_unit on vectors whose norm is off by 1e-7 ... 3e-5: the error grows with the defect, never faster."""
    for d in (1e-7, -1e-6, 1e-6, 1e-5, -3e-5):
        x = mi.angle_inputs(d, n=1 << 20)
        y = gpu.debug_eval_math("angle_unit", x)
        _same_bits(y, orc.sp_eval("angle_unit", x), f"angle_unit, defect {d}")
        mi.check_angle(x, y, rounded=False)


def _total_order_key(v):
    """float32 -> int64 key of IEEE's totalOrder on non-NaN values (-0 < +0)."""
    b = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.int64)
    return np.where(b >> 31 == 1, -(b & 0x7FFFFFFF) - 1, b)


def test_min_max_clip_order_signed_zeros(gpu, evals):
    """fmin_ / fmax_ / fclip are one v_min_f32 / v_max_f32 / v_med3_f32: min, max and median under -0 < +0, on every
    input (finite).  The checker's sp_min / sp_max / sp_clip are selects, which return the second / first operand on a
    tie of zeros: the two copies differ only in the sign of a zero result (test_primitive_matches_the_checker_and_float64),
    and the whole-plan tests stay bit-exact through every caller."""
    for op in ("fmin_", "fmax_", "fclip"):
        x, y, ref = evals(op)
        k = _total_order_key(x)
        if op == "fmin_":
            want = np.where(k[:, 0] <= k[:, 1], x[:, 0], x[:, 1])
        elif op == "fmax_":
            want = np.where(k[:, 0] >= k[:, 1], x[:, 0], x[:, 1])
        else:
            want = np.take_along_axis(x, np.argsort(k, axis=1, kind="stable")[:, 1:2], 1)[:, 0]
        _same_bits(y, want, op)
        assert (_bits(y) != _bits(ref)).sum() > 0, op  # (the inputs hold the zero ties)
    z = np.float32([[0.0, -0.0], [-0.0, 0.0]])
    assert _bits(gpu.debug_eval_math("fmin_", z)).tolist() == [0x80000000, 0x80000000]
    assert _bits(gpu.debug_eval_math("fmax_", z)).tolist() == [0, 0]


def test_out_of_domain_values_are_pinned(gpu):
    """Inputs outside a primitive's documented domain (csrc/mbd_math.h) give the device values recorded here; the
    checker (IEEE division / sqrt, selects) gives others.  The callers keep these inputs out: denominators of the
    solver's division in [1e-20, 1e10], its square root's argument finite, min / max / clip arguments finite."""
    nan = np.float32(np.nan)
    r = gpu.debug_eval_math("rcp_exact", np.float32([0.0, -0.0, np.inf, -np.inf, 1e-38, 1e-40]))
    assert np.all(np.isnan(r))  # (the checker: +-inf, +-0, 1e38, inf)
    r = gpu.debug_eval_math("div_", mi.pairs([1.0, 1.0, 1e30], [0.0, np.inf, 1e-20]))
    assert np.all(np.isnan(r))  # (the checker: inf, 0, inf: the quotient overflows)
    assert np.isnan(gpu.debug_eval_math("sqrt_floor", np.float32([np.inf]))[0])  # (the checker: inf)
    assert _bits(gpu.debug_eval_math("sqrt_floor", np.float32([nan, -np.inf]))).tolist() == [_bits(np.float32(1e-15))] * 2
    assert gpu.debug_eval_math("fmin_", mi.pairs([1.0], [nan]))[0] == 1.0  # (the checker's select: NaN)
    assert gpu.debug_eval_math("fmax_", mi.pairs([1.0], [nan]))[0] == 1.0
