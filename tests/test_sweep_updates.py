"""Without a GPU: mbd_debug_sweep_update's argument refusals (they come before any device access), the lists and inputs of
tests/sweep_update_inputs.py, and the (plan, tile) map of score_wmean_batch_kernel restated from the kernel's text."""
import ctypes as C

import numpy as np

import pi_inputs as pi
import sweep_update_inputs as su


def test_entry_is_declared_exported_and_refuses_arguments_before_the_device(lib):
    """NULL sweep / cand / ybar / rews, lp and sigma_in given where not taken, i outside [1, Ndiffuse - 1]: MBD_ERR_INVALID naming the
    field, on a box without a device.  The handle is a zeroed stand-in (update_method 0, enable_demo 0, Ndiffuse 0: every i is outside);
    the refusals of a missing lp / sigma_in need a demo or a cma-es sweep (tests/test_gpu_sweep_updates.py)."""
    from mbd_hip import _capi
    assert hasattr(lib, "mbd_debug_sweep_update")
    lib.mbd_debug_sweep_update.argtypes = _capi.SWEEP_UPDATE_ARGTYPES
    lib.mbd_last_error.restype = C.c_char_p
    stand_in = C.create_string_buffer(1 << 16)
    buf = np.zeros(8, np.float32)
    p = buf.ctypes.data

    def refused(field, h=stand_in, i=1, c=p, y=p, r=p, lp=None, sigma_in=None):
        assert lib.mbd_debug_sweep_update(h, i, c, y, r, lp, sigma_in, p, p, p, p, p) == _capi.MBD_ERR_INVALID, field
        assert field in lib.mbd_last_error(), (field, lib.mbd_last_error())

    refused(b"sweep is NULL", h=None)
    refused(b"cand is NULL", c=None)
    refused(b"ybar is NULL", y=None)
    refused(b"rews is NULL", r=None)
    refused(b"lp given", lp=p)
    refused(b"sigma_in given", sigma_in=p)
    for i in (1, 0, -3, 17):
        refused(b"i=%d outside" % i, i=i)
    assert not buf.any()  # (no output was written)


def test_ragged_sizes_sit_on_either_side_of_every_boundary_of_the_batch_body():
    """score_wmean_body<32, false, V>: a prefetch of 16 / V rows per group of 64 candidates, rounds of 32 / V, a tail of 16 / V, then
    single rows — for V = 1, 2, 4 the list has a size below, (at,) and above the prefetch, prefetch + tail and prefetch + round,
    sizes that are no multiple of 64, and the largest size a sweep takes."""
    Ns = set(su.RAGGED_N)
    for V in (1, 2, 4):
        pre, rnd, tail = 64 * 16 // V, 64 * 32 // V, 64 * 16 // V
        for edge in (pre, pre + tail, pre + rnd):
            assert any(edge - 64 < n < edge for n in Ns) and any(edge < n < edge + 64 for n in Ns), (V, edge)

        def path(N):  # (prefetched, rounds, tails, single rows) of group 0's chain
            n, took = 0, [0, 0, 0, 0]
            if (16 // V - 1) * 64 < N:
                took[0], n = 1, pre
            while n + (32 // V - 1) * 64 < N:
                took[1], n = took[1] + 1, n + rnd
            while n + (16 // V - 1) * 64 < N:
                took[2], n = took[2] + 1, n + tail
            while n < N:
                took[3], n = took[3] + 1, n + 64
            return tuple(took)
        paths = {path(N) for N in Ns}
        assert {(0, 0, 0, 1), (1, 0, 0, 0)} <= paths
        assert any(p[1] >= 1 and p[2] >= 1 and p[3] >= 1 for p in paths) and any(p[1] >= 2 for p in paths), V
    assert {1, 2, 63, 64, 65, 12288} <= Ns and max(Ns) == 12288
    assert all(su.ragged_plans(N) == (3 if N < 8192 else 2) for N in Ns)


def test_rounds_take_every_shape_and_case_through():
    for N in sorted(set(su.RAGGED_N + su.PI_N + su.MATRIX_N)):
        for P in (2, 3):
            rs = su.rounds(N, P)
            assert {s for r in rs for s in r} == set(pi.shapes(N)) and all(len(r) == P for r in rs)
            if len(pi.shapes(N)) >= P:
                assert all(len(set(r)) == P for r in rs), (N, P)
        seen = {(s, su.PI_TEMPS[k]) for r in su.pi_rounds(N) for k, s in enumerate(r)}
        assert seen >= {(s, t) for s, t, _ in pi.cases(N)}, N
        if N > 1:
            assert all(r[0] != r[1] for r in su.pi_rounds(N))
    assert len(set(su.MBD_TEMPS)) == 3 and len(set(su.PI_TEMPS)) == 3 and len(set(su.PI_SIGMAS)) == 3
    r = np.stack([su.plan_rewards(k, 65) for k in range(su.MAX_PLANS)])
    assert len({a.tobytes() for a in r[:7]}) == 7 and not np.array_equal(r[0], r[9]) and np.array_equal(np.sort(r[0]), np.sort(r[9]))
    for N in su.WEIGHTED_N:
        a, b = su.weighted_rounds(N)
        assert a.shape == b.shape == (3, N) and a.dtype == np.float32
        assert not np.isfinite(b[0]).any() and np.isfinite(b[1]).sum() == 1 and np.isfinite(b[2]).all()
        if N > 130:
            bad = [set(np.flatnonzero(~np.isfinite(x))) for x in a]
            assert all(bad) and not (bad[0] & bad[1]) and not (bad[0] & bad[2]) and not (bad[1] & bad[2])


def test_values_round_twice_and_clip():
    """values(): z * sigma rounded to float32, + ybar rounded, then the clip — against the same in float64 rounded step by step."""
    z, ybar = su.normals(2, 50, 7), su.means(2, 7)
    z[0, 0, 0], z[1, 3, 2] = 40.0, -40.0
    sigma = np.float32(0.731)
    t = (z.astype(np.float64) * np.float64(sigma)).astype(np.float32)
    t = (t.astype(np.float64) + ybar[:, None, :].astype(np.float64)).astype(np.float32)
    ref = np.minimum(np.maximum(t, np.float32(-1)), np.float32(1))
    got = su.values(z, sigma, ybar)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert got[0, 0, 0] == 1.0 and got[1, 3, 2] == -1.0 and np.abs(got).max() == 1.0


def _xcd_tile(x, n, first):
    """mbd_step_kernels.h xcd_tile, line by line."""
    c = (first + x) & 7
    start = 0
    for d in range(8):
        if d == c:
            break
        x0 = (d - first) & 7
        start += (n - 1 - x0) // 8 + 1 if x0 < n else 0
    return start + (x - ((c - first) & 7)) // 8


def test_plan_tile_map_of_the_batch_kernel_is_a_bijection():
    """score_wmean_batch_kernel's (blockIdx.y, blockIdx.x) -> (plan, tile), restated: xcd_tile with first = blockIdx.y T, and for a
    multiple of 8 plans k = c + 8 (m / T), tile = m % T of the linear index — one workgroup per pair for P = 1 .. 32, T = 1 .. 69."""
    for P in range(1, 33):
        for T in range(1, 70):
            pairs = set()
            for by in range(P):
                for bx in range(T):
                    k, tile = by, _xcd_tile(bx, T, by * T)
                    if P % 8 == 0:
                        lin = by * T + bx
                        c, m = lin & 7, lin >> 3
                        k, tile = c + 8 * (m // T), m % T
                    pairs.add((k, tile))
            assert pairs == {(k, t) for k in range(P) for t in range(T)}, (P, T)
    # the tile counts the GPU matrix runs under V = 1 (Nu = 1: H outputs)
    assert sorted({-(-h // 16) for h in su.TILE_H}) == [1, 2, 3, 4, 5, 7, 8, 9]
    assert any(h % 32 for h in su.TILE_H) and any(h % 64 for h in su.TILE_H)
