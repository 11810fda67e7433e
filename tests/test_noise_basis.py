"""Noise bases without a GPU (include/mbd_hip.h mbd_noise_basis, mbd_plan_set_noise_basis, mbd_sweep_set_noise_basis;
mbd_hip.planners.mpc.knot_basis and its arguments; DESIGN.md section 1 "N8 noise basis").

The two setters are exported and refuse what the record alone decides with MBD_ERR_INVALID, naming the field, before touching
a device; the ctypes record has the header's layout; knot_basis builds the tables the documentation states; and the checker's
restatement (tests/noise_basis_checker.py) keeps the contract's consequences — the identity basis is the flat sampler in
value, a row of zeros freezes its horizon row at clip(Ybar) with z = +0, zero weights are left out of the sum, the shape
comes after the basis — and gives every row the variance and neighbouring rows the correlation that W W^T states.  The
kernels are held to that restatement in tests/test_gpu_noise_basis.py."""
import ctypes as C
import os
import shutil
import subprocess
from dataclasses import replace

import numpy as np
import pytest

import mpc_checker
import noise_basis_checker as nbc
import noise_shape_checker as nsc
from conftest import ROOT, load_model
from oracle import planner as op


def _oenv(orc, name):
    m = load_model(name)
    return op.OracleEnv(orc, name, m.to_struct(), init_q=m.init_q)


def _reset(orc, oe, seed):
    return np.asarray(oe.reset(orc.split(orc.prng_key(seed), 2, 1)[1], 1), np.float32)


def _record(_capi, W, n_knots=None, when=0):
    W = np.ascontiguousarray(W, np.float32)
    rec = _capi.NoiseBasis()
    rec.basis = W.ctypes.data_as(C.POINTER(C.c_float))
    rec.n_knots = W.shape[1] if n_knots is None else n_knots
    rec.when = when
    return rec, W


def test_setters_are_exported(lib):
    from mbd_hip import _capi
    for name in ("mbd_plan_set_noise_basis", "mbd_sweep_set_noise_basis"):
        assert name in _capi.EXPORTS and hasattr(lib, name), name
    assert hasattr(lib, "mbd_debug_knot_noise") and hasattr(lib, "mbd_debug_knot_noise_host")
    text = open(os.path.join(ROOT, "include", "mbd_hip.h")).read()
    assert "#define MBD_MAX_KNOTS 16" in text and _capi.MAX_KNOTS == 16


def test_the_ctypes_record_has_the_headers_layout(tmp_path):
    from mbd_hip import _capi
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a C compiler is what builds the checker as well"
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mbd_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(mbd_noise_basis), offsetof(mbd_noise_basis, basis), '
                   'offsetof(mbd_noise_basis, n_knots), offsetof(mbd_noise_basis, when)); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = _capi.NoiseBasis
    assert got == [C.sizeof(S), S.basis.offset, S.n_knots.offset, S.when.offset]


@pytest.mark.parametrize("setter", ["mbd_plan_set_noise_basis", "mbd_sweep_set_noise_basis"])
def test_argument_errors_come_before_any_device_access(lib, setter):
    """The refusals the record alone decides, on a box with no device: MBD_ERR_INVALID and the field's name.  The handle is a
    zeroed stand-in whose Hsample is 0, so its table has no entry to look at and the call gets as far as `when`; the refusal of
    a non-finite entry needs a real handle (tests/test_gpu_noise_basis.py).  Every record here is refused, so none reaches the
    device."""
    from mbd_hip import _capi
    fn = getattr(lib, setter)
    ok, keep = _record(_capi, np.ones((4, 3), np.float32))

    def refused(rec, field, handle):
        assert fn(handle, C.byref(rec)) == _capi.MBD_ERR_INVALID, field
        assert field in lib.mbd_last_error(), (field, lib.mbd_last_error())

    refused(ok, b"plan" if "plan" in setter else b"sweep", None)
    stand_in = C.create_string_buffer(1 << 16)
    r, _ = _record(_capi, keep)
    r.basis = None
    refused(r, b"basis is NULL", stand_in)
    for k in (0, -3, 17, 1 << 20):
        refused(_record(_capi, keep, n_knots=k)[0], b"n_knots=%d" % k, stand_in)
    for when in (-1, 2, 7):
        refused(_record(_capi, keep, when=when)[0], b"when", stand_in)


# ---- the kernel's per-column code, on the host -------------------------------------------------------------------------------
# (the sizes of tests/test_gpu_noise_basis.py's kernel test; Nu > 1 is where a column's element h Nu + a of candidate n can go wrong)
_SIZES = [(1, 1, 1, 1), (3, 4, 1, 2), (37, 7, 3, 3), (5, 16, 2, 16), (101, 11, 3, 5), (257, 5, 1, 16), (64, 50, 17, 10), (513, 6, 3, 4)]


@pytest.mark.parametrize("layout", [0, 1], ids=["legacy", "part"])
@pytest.mark.parametrize("shaped", [False, True], ids=["noshape", "shape"])
@pytest.mark.parametrize("N,H_,Nu,K_", _SIZES, ids=["-".join(map(str, s)) for s in _SIZES])
def test_knot_column_on_the_host(lib, orc, N, H_, Nu, K_, shaped, layout):
    """knot_column — the text knot_noise_kernel runs per column — over all columns on the host (mbd_debug_knot_noise_host)
    against the checker, bit for bit: every element written, none twice, each where the ring buffers' layout puts it."""
    from mbd_hip import _capi
    from state_inputs import same_bits
    W = nbc.basis_of(H_, K_)
    g = None
    if shaped:
        g = (0.5 + np.arange(H_ * Nu, dtype=np.float64) / (H_ * Nu)).astype(np.float32).reshape(H_, Nu)
        g[H_ // 2] = 0.0
    key = orc.prng_key(700 + N)
    z = _capi.debug_knot_noise_host(key, layout, N, H_, Nu, W, g)
    _, want = nbc.BasisOracle(orc, W, g).sample(key, layout, N, H_, Nu, 0, N, 1.0, np.zeros((H_, Nu), np.float32), want_eps=True)
    same_bits(z, want, f"N={N} H={H_} Nu={Nu} K={K_}")


# ---- knot_basis ------------------------------------------------------------------------------------------------------------

def test_knot_basis_tables():
    from mbd_hip.planners.mpc import knot_basis
    for H, K in ((50, 10), (6, 3), (7, 7), (16, 16), (5, 2), (9, 4)):
        raw = knot_basis(H, K, "linear", normalise=False)
        assert raw.dtype == np.float32 and raw.shape == (H, K) and raw.flags["C_CONTIGUOUS"]
        assert (raw >= 0).all() and np.allclose(raw.sum(axis=1, dtype=np.float64), 1.0, atol=1e-6)
        assert ((raw != 0).sum(axis=1) <= 2).all()  # a row interpolates between the two knots around it
        assert raw[0, 0] == 1 and raw[-1, -1] == 1  # the first and the last knot sit on the first and the last row
        for kind in ("linear", "hold"):
            W = knot_basis(H, K, kind)
            assert np.allclose(np.sqrt((W.astype(np.float64) ** 2).sum(axis=1)), 1.0, atol=1e-6), (H, K, kind)
        hold = knot_basis(H, K, "hold", normalise=False)
        assert ((hold == 1).sum(axis=1) == 1).all() and ((hold == 0).sum(axis=1) == K - 1).all()
        assert np.array_equal(hold.argmax(axis=1), (np.arange(H) * K) // H)
        assert np.array_equal(hold, knot_basis(H, K, "hold"))  # (rows of norm 1 already)
    # the hat functions by hand: H = 5, knots at rows 0, 2, 4
    assert np.array_equal(knot_basis(5, 3, "linear", normalise=False),
                          np.array([[1, 0, 0], [.5, .5, 0], [0, 1, 0], [0, .5, .5], [0, 0, 1]], np.float32))
    assert np.array_equal(knot_basis(4, 1, "linear"), np.ones((4, 1), np.float32))  # one knot: a constant column
    assert np.array_equal(knot_basis(6, 6, "linear"), np.eye(6, dtype=np.float32))  # a knot per row: the identity
    assert np.array_equal(knot_basis(1, 1, "hold"), np.ones((1, 1), np.float32))


def test_arguments_and_their_refusals():
    from mbd_hip.planners import mpc
    a = mpc.MpcArgs(env_name="hopper", Nsample=16, Hsample=6, Ndiffuse=6, disable_recommended_params=True, not_render=True)
    assert not mpc._has_basis(a) and (a.noise_knots, a.noise_interp) == (0, "linear")
    b = replace(a, noise_knots=3, noise_interp="hold")
    W, when = mpc._basis_of(b)
    assert mpc._has_basis(b) and when == "always" and np.array_equal(W, mpc.knot_basis(6, 3, "hold"))
    assert mpc._basis_settings(b) == dict(noise_knots=3, noise_interp="hold")
    c = replace(b, tail_rows=2, tail_sigma=4.0)  # composable with the tail ramp
    assert mpc._has_shape(c) and mpc._has_basis(c)
    with pytest.raises(ValueError, match=r"noise_knots=17 outside \[1, 16\]"):
        mpc._basis_of(replace(a, noise_knots=17))
    with pytest.raises(ValueError, match=r"noise_knots=-2 outside \[1, 16\]"):
        mpc._basis_of(replace(a, noise_knots=-2))
    with pytest.raises(ValueError, match="noise_interp='cubic'"):
        mpc._basis_of(replace(a, noise_knots=3, noise_interp="cubic"))
    mpc._check_batch([b, replace(b, seed=1)])
    with pytest.raises(ValueError, match="noise_knots"):
        mpc._check_batch([b, replace(a, seed=1)])
    with pytest.raises(ValueError, match="noise_interp"):
        mpc._check_batch([b, replace(b, seed=1, noise_interp="linear")])


# ---- the checker's restatement ---------------------------------------------------------------------------------------------
# hopper, N = 16, H = 4: the sizes of tests/test_noise_shape.py
N, H, ND = 16, 4, 6


def _step_inputs(orc):
    oe = _oenv(orc, "hopper")
    s0 = _reset(orc, oe, 2)
    sched = orc.schedule(1e-4, 1e-2, ND)
    Ybar = (np.random.default_rng(5).normal(size=(H, oe.Nu)) * 0.3).astype(np.float32)
    Ybar[1, 2], Ybar[3, 0] = 1.5, -0.0  # (outside the clip; a signed zero)
    return oe, s0, sched, Ybar


@pytest.mark.parametrize("impl", [0, 1])
def test_checker_identity_basis_is_the_flat_sampler(orc, impl):
    """n_knots = H, W = I: the knot tensor IS the flat tensor (same size, same counters), and 0 + 1 * eps = eps in value —
    compared with ==, since +0 + (-0) = +0 where the flat sampler keeps -0."""
    oe, s0, sched, Ybar = _step_inputs(orc)
    key = orc.prng_key(11)
    for n, h, nu in ((N, H, oe.Nu), (37, 7, 3), (5, 16, 2)):
        yb = np.resize(Ybar, (h, nu)).astype(np.float32)
        flat, eps = orc.sample(key, impl, n, h, nu, 0, n, 0.7, yb, want_eps=True)
        got, z = nbc.BasisOracle(orc, np.eye(h, dtype=np.float32)).sample(key, impl, n, h, nu, 0, n, 0.7, yb, want_eps=True)
        assert np.array_equal(z, eps) and np.array_equal(got, flat), (n, h, nu)
    if impl == 1:
        for i in (ND - 1, 1):
            want = op.reverse_once(orc, oe, s0, i, key, Ybar, sched, N, H, 0.1, impl)
            got = nbc.reverse_once(orc, oe, np.eye(H, dtype=np.float32), s0, i, key, Ybar, sched, N, H, 0.1, impl)
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])


def test_checker_zero_row_freezes_it_at_the_clipped_mean(orc):
    oe, s0, sched, Ybar = _step_inputs(orc)
    key = orc.prng_key(12)
    W = np.array([[1, 0.5], [0, -0.0], [-2, 0.25], [0, 1]], np.float32)
    Y0s, z = nbc.BasisOracle(orc, W).sample(key, 1, N, H, oe.Nu, 0, N, 0.5, Ybar, want_eps=True)
    assert np.array_equal(z[:, 1, :].view(np.uint32), np.zeros((N, oe.Nu), np.uint32))  # z = +0, by bit pattern
    row = np.clip(Ybar[1], np.float32(-1), np.float32(1))
    assert np.array_equal(Y0s[:, 1, :], np.broadcast_to(row, (N, oe.Nu)))
    # rows are slices of the whole tensor
    part = nbc.BasisOracle(orc, W).sample(key, 1, N, H, oe.Nu, 5, 7, 0.5, Ybar)
    assert np.array_equal(part, Y0s[5:12])
    # the last row reads knot 1 alone, the first both
    eps = orc.normal(key, (N, 2, oe.Nu), 1)
    assert np.array_equal(z[:, 3, :], eps[:, 1, :])
    assert np.array_equal(z[:, 0, :], (eps[:, 0, :] + (np.float32(0.5) * eps[:, 1, :]).astype(np.float32)).astype(np.float32))


def test_checker_skips_zero_weights():
    """A zero weight is left out, not multiplied: an infinity among the normals never meets a zero, and the sum starts from
    +0, so a lone -0 term gives +0."""
    eps = np.array([[[np.inf], [2.0], [-0.0]]], np.float32)  # [N = 1, K = 3, Nu = 1]
    W = np.array([[0.0, 3.0, 0.0], [-0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0]], np.float32)
    with np.errstate(all="raise"):
        c = nbc.combine(W, eps)[0, :, 0]
    assert np.array_equal(c[:2], np.array([6.0, 0.0], np.float32)) and np.isposinf(c[2]) and not np.signbit(c[1])
    assert c[3] == 0 and not np.signbit(c[3])
    # two roundings per term: the product is rounded before it is added
    a, b = np.float32(1.0 + 2.0 ** -12), np.float32(1.0 + 2.0 ** -13)
    c = nbc.combine(np.array([[1.0, a]], np.float32), np.array([[[np.float32(-1.0)], [b]]], np.float32))[0, 0, 0]
    assert c == np.float32(np.float32(a * b) - np.float32(1.0)) and c != np.float32(np.float64(a) * np.float64(b) - 1.0)


def test_checker_applies_the_basis_first_then_the_shape(orc):
    oe, s0, sched, Ybar = _step_inputs(orc)
    key = orc.prng_key(13)
    W = np.array([[1, 0.5, 0], [0.25, -1, 0.75], [0, 0, 1.5], [0.3, 0.3, 0.3]], np.float32)
    g = (0.5 + np.arange(H * oe.Nu, dtype=np.float32).reshape(H, oe.Nu) / 7).astype(np.float32)
    for impl in (0, 1):
        _, c = nbc.BasisOracle(orc, W).sample(key, impl, N, H, oe.Nu, 0, N, 0.5, Ybar, want_eps=True)
        Y0s, z = nbc.BasisOracle(orc, W, g).sample(key, impl, N, H, oe.Nu, 0, N, 0.5, Ybar, want_eps=True)
        assert np.array_equal(z, (c * g[None]).astype(np.float32))
        y = ((z * np.float32(0.5)).astype(np.float32) + Ybar[None]).astype(np.float32)
        assert np.array_equal(Y0s, np.clip(y, np.float32(-1), np.float32(1)))
        # no basis: the shaped oracle's sample
        assert np.array_equal(nbc.BasisOracle(orc, None, g).sample(key, impl, N, H, oe.Nu, 0, N, 0.5, Ybar),
                              nsc.ShapedOracle(orc, g).sample(key, impl, N, H, oe.Nu, 0, N, 0.5, Ybar))


def test_checker_warm_episode_leaves_tick_0_alone(orc):
    """Each setting under its own `when`: with a warm basis tick 0 is mpc_checker.episode's and T ticks are a prefix of T + 1;
    a warm basis beside an always-shape leaves tick 0 to the shape alone."""
    oe = _oenv(orc, "hopper")
    s0, key = _reset(orc, oe, 3), orc.prng_key(14)
    T, K, E = 3, 2, 1
    W = np.array([[1, 0], [0.6, 0.8], [0, 1], [0, -1]], np.float32)
    g = np.full((H, oe.Nu), 0.5, np.float32)
    flat = mpc_checker.episode(oe, s0, key, N, H, ND, 0.1, T, K, E)
    warm = nbc.episode(mpc_checker.episode, oe, W, "warm", ND, s0, key, N, H, ND, 0.1, T, K, E)
    short = nbc.episode(mpc_checker.episode, oe, W, "warm", ND, s0, key, N, H, ND, 0.1, T - 1, K, E)
    always = nbc.episode(mpc_checker.episode, oe, W, "always", ND, s0, key, N, H, ND, 0.1, T, K, E)
    assert np.array_equal(warm["means"][0], flat["means"][0]) and not np.array_equal(warm["means"][1], flat["means"][1])
    assert not np.array_equal(always["means"][0], flat["means"][0])
    for k in ("means", "actions", "rewards", "states"):
        assert np.array_equal(short[k], warm[k][: len(short[k])]), k
    both = nbc.episode(mpc_checker.episode, oe, W, "warm", ND, s0, key, N, H, ND, 0.1, T, K, E, shape=g, shape_when="always")
    shaped = nsc.episode(mpc_checker.episode, oe, g, "always", ND, s0, key, N, H, ND, 0.1, T, K, E)
    assert np.array_equal(both["means"][0], shaped["means"][0]) and not np.array_equal(both["means"][1], shaped["means"][1])


@pytest.mark.parametrize("kind,H_,K_", [("linear", 12, 4), ("hold", 12, 4), ("linear", 50, 10)])
def test_rows_keep_their_variance_and_neighbours_correlate(orc, kind, H_, K_):
    """16 384 columns (N = 4096, Nu = 4) under a normalised basis: every row's sample variance is within 6 sqrt(2 / 16384) =
    0.066 of 1 (the standard error of a variance estimate of unit normals is sqrt(2 / n); six of them), and the lag-1 sample
    correlation of rows h, h + 1 within the same bound of (W W^T)[h][h + 1]."""
    from mbd_hip.planners.mpc import knot_basis
    n, nu = 4096, 4
    W = knot_basis(H_, K_, kind)
    _, z = nbc.BasisOracle(orc, W).sample(orc.prng_key(21), 1, n, H_, nu, 0, n, 1.0, np.zeros((H_, nu), np.float32), want_eps=True)
    cols = z.astype(np.float64).transpose(1, 0, 2).reshape(H_, n * nu)
    assert cols.shape[1] == 16384
    bound = 6.0 * np.sqrt(2.0 / 16384)
    var = cols.var(axis=1)
    assert np.abs(var - 1.0).max() <= bound, var
    cov = (W.astype(np.float64) @ W.astype(np.float64).T)
    cc = np.corrcoef(cols)
    lag1 = np.array([cc[h, h + 1] for h in range(H_ - 1)])
    want = np.array([cov[h, h + 1] for h in range(H_ - 1)])
    assert np.abs(lag1 - want).max() <= bound, (lag1, want)
    assert want.max() > 0.5  # (the basis does correlate neighbouring rows)
