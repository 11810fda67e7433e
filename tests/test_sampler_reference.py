"""The sampler's table and reference (tests/sampler_inputs.py), without a GPU.

  * the numpy restatement of jax.random.normal reproduces every value JAX's documentation prints (the ones
    tests/test_oracle_prng.py holds the checker to): keys, uniform, normals, both layouts;
  * the checker's normals — orc.normal, and orc.sample(..., want_eps=True) on row ranges — agree with the restatement over the
    whole table, the four large cases included, within the float32 erf_inv polynomial's 1e-5 relative; orc_random_bits32
    equals the restatement's words exactly;
  * the REACH test: from the host arithmetic alone (mbd_debug_rollout_choice needs no device) every entry of the table takes
    the branch its comment claims — which side of N >= 5 count, of 65536 x 256, of 4096 x 256, of one workgroup; pinned or not;
    the noise job taken or not; need against spare — and every form, layout and boundary the table promises has an entry.  A
    table edit that silently stops covering a form fails here.
"""
import numpy as np
import pytest

import sampler_inputs as sx
from conftest import load_model

KEY = np.array([0x9E3779B9, 0x7F4A7C15], np.uint32)


# ---- the restatement against JAX's published outputs ----------------------------------------------------------------------

def _close32(got64, want):
    """a float64 normal against a float32 value JAX printed: within the polynomial's error and float32's rounding"""
    return abs(got64 - float(np.float32(want))) <= sx.RTOL * abs(float(np.float32(want)))


def test_restatement_reproduces_random123_known_answers():
    for k, c, want in (((0, 0), (0, 0), (0x6B200159, 0x99BA4EFE)),
                       ((0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF), (0x1CB996FC, 0xBB002BE7)),
                       ((0x13198A2E, 0x03707344), (0x243F6A88, 0x85A308D3), (0xC4923A9C, 0x483DF7A0))):
        o0, o1 = sx.threefry2x32(k[0], k[1], np.array([c[0]], np.uint32), np.array([c[1]], np.uint32))
        assert (int(o0[0]), int(o1[0])) == want


def test_restatement_reproduces_published_jax_outputs_legacy_layout():
    k0 = sx.prng_key(0)
    ks = sx.split(k0, 2, sx.LEGACY)
    assert ks.tolist() == [[4146024105, 967050713], [2718843009, 1272950319]]
    assert _close32(sx.normal64(k0, sx.LEGACY, 1)[0], -0.20584226)
    assert _close32(sx.normal64(ks[1], sx.LEGACY, 1)[0], -1.2515389)
    b = sx.bits_whole(k0, sx.LEGACY, 1)
    u01 = ((b >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1.0)  # uniform on [0, 1)
    assert u01[0] == np.float32(0.41845703)
    k42 = sx.prng_key(42)
    assert _close32(sx.normal64(k42, sx.LEGACY, 1)[0], -0.18471177)
    for got, want in zip(sx.normal64(k42, sx.LEGACY, 3), (0.18693547, -1.2806505, -1.5593132)):
        assert _close32(got, want)


def test_restatement_reproduces_published_jax_outputs_partitionable_layout():
    k42 = sx.prng_key(42)
    assert _close32(sx.normal64(k42, sx.PARTITIONABLE, 1)[0], -0.028304616)
    ks = sx.split(k42, 2, sx.PARTITIONABLE)
    assert ks[0].tolist() == [1832780943, 270669613]
    assert _close32(sx.normal64(ks[1], sx.PARTITIONABLE, 1)[0], 0.60576403)


def test_restatement_agrees_with_the_checkers_keys(orc):
    assert sx.prng_key((7 << 32) | 5).tolist() == orc.prng_key((7 << 32) | 5).tolist()
    for lay in sx.LAYOUTS:
        for num in (2, 3, 5):
            assert np.array_equal(sx.split(KEY, num, lay), orc.split(KEY, num, lay))


@pytest.mark.parametrize("layout", sx.LAYOUTS)
def test_element_by_element_words_are_slices_of_the_whole_tensor(layout):
    """bits_at (what ranges of the large cases use) against the whole-tensor form, at every small total of the table."""
    for total in sorted({c.total for c in sx.cases(large=False)}):
        whole = sx.bits_whole(KEY, layout, total)
        assert np.array_equal(sx.bits_at(KEY, layout, total, np.arange(total)), whole), total


# ---- the checker against the restatement ----------------------------------------------------------------------------------

def _shapes():
    """the distinct (layout, N, HNu) of the table, and with each the row ranges its cases sample"""
    out = {}
    for c in sx.CASES:
        ranges = out.setdefault((c.layout, c.N, c.HNu), set())
        ranges.add((0, c.N))
        if c.shard:
            b, n = c.shard
            ranges.update(r for r in ((b, n), (0, b), (b + n, c.N - b - n)) if r[1] > 0)
    return sorted((k, sorted(v)) for k, v in out.items())


def test_checker_normals_agree_with_the_restatement_over_the_whole_table(orc):
    """orc.normal over every (layout, N, H Nu) of the table and orc.sample(..., want_eps=True) over every row range its
    shards use, against sqrt(2) erfinv(u) in float64: |d| / |ref| < 1e-5.  Observed maximum over the table (33.6 million
    elements in the large cases): 5.8e-6, at max |z| = 5.42."""
    worst, zmax, n = 0.0, 0.0, 0
    for (layout, N, HNu), ranges in _shapes():
        ref = sx.normal64(KEY, layout, N * HNu)
        assert np.isfinite(ref).all()
        r = sx.ratio(orc.normal(KEY, (N, HNu), layout), ref)
        assert r < sx.RTOL, (layout, N, HNu, r)
        worst, zmax, n = max(worst, r), max(zmax, float(np.abs(ref).max())), n + ref.size
        Ybar = np.zeros(HNu, np.float32)
        for begin, count in ranges:
            if N * HNu > sx.WHOLE_LIMIT and count == N:
                continue  # (the large cases are unsharded: orc.normal above is their whole tensor)
            Y0s, eps = orc.sample(KEY, layout, N, HNu, 1, begin, count, 0.125, Ybar, want_eps=True)
            want = ref.reshape(N, HNu)[begin:begin + count]
            r = sx.ratio(eps, want)
            assert r < sx.RTOL, (layout, N, HNu, begin, count, r)
            # 0.125 is a power of two and 5.5 x 0.125 < 1: the candidates are the normals, scaled exactly
            assert np.array_equal(Y0s.reshape(-1), eps.reshape(-1) * np.float32(0.125))
            worst = max(worst, r)
    print(f"\n{n} elements, max |checker - float64| / |float64| = {worst:.3g}, max |z| = {zmax:.3f}")
    assert zmax < sx.MAX_ABS_NORMAL


def test_checker_words_equal_the_restatement(orc):
    """orc_random_bits32, which is called per element, on the first and last 600 elements and a stride through the middle of
    every total of the table: exactly the restatement's words."""
    for layout in sx.LAYOUTS:
        for total in sorted({c.total for c in sx.CASES if c.layout == layout}):
            step = max(1, total // 1009)
            idx = np.unique(np.concatenate([np.arange(min(600, total)), np.arange(0, total, step), np.arange(max(0, total - 600), total)]))
            got = np.array([orc.lib.orc_random_bits32(KEY, layout, int(j), total) for j in idx], np.uint32)
            want = sx.bits_at(KEY, layout, total, idx) if total > sx.WHOLE_LIMIT else sx.bits_whole(KEY, layout, total)[idx]
            assert np.array_equal(got, want), (layout, total)


# ---- reach ---------------------------------------------------------------------------------------------------------------

def test_table_names_every_form_layout_and_boundary():
    assert {c.form for c in sx.CASES} == set(sx.FORMS)
    assert len({c.id for c in sx.CASES}) == len(sx.CASES)
    for form in sx.FORMS:
        assert {c.layout for c in sx.cases(form)} == set(sx.LAYOUTS), form
    for name, nu in sx.NU.items():
        if name != "car2d":  # (car2d has no compiled model: its two actions are csrc's Car2dParams us [B][H][2])
            assert load_model(name).to_struct().n_act == nu, name
    for lay in sx.LAYOUTS:
        for form in ("whole", "noise"):
            cs = [c for c in sx.cases(form) if c.layout == lay]
            totals = {c.total for c in cs}
            assert {1, 2, 3} <= totals, (form, lay)
            # one 256-thread workgroup of thread-items: exactly, one fewer, one more
            assert {255, 256, 257} <= {c.items for c in cs}, (form, lay, sorted(c.items for c in cs))
            assert any(c.total % 2 == 1 and c.total > 3 and np.gcd(c.HNu, 256) == 1 and c.HNu > 1 for c in cs), (form, lay)
        # legacy pairs: an odd total whose padded pair is the last thread of a workgroup (511) and the first of the next (513)
        assert {511, 513} <= {c.total for c in sx.cases("whole") if c.layout == lay}
        # both sources of sigma, and a rigid-body MBD plan made to materialise
        whole = [c for c in sx.cases("whole") if c.layout == lay]
        assert any(c.kind == "pi" for c in whole) and any(c.env == "car2d" for c in whole)
        assert any(c.kind == "mbd" and c.levers.get("MBD_NO_LAZY") for c in whole)
    assert all(c.lazy == (c.form in ("noise", "fused")) for c in sx.CASES)


def test_sub_range_cases_fall_on_the_intended_side_of_the_hosts_switch():
    for lay in sx.LAYOUTS:
        three = [c for c in sx.cases("three_range") if c.layout == lay]
        one = [c for c in sx.cases("one_range") if c.layout == lay]
        for c in three:
            assert c.shard and c.N >= sx.AUX_RATIO * c.shard[1] and not c.levers.get("MBD_NO_AUX") and not c.lazy, c.id
            sp = sx.spans(c)
            assert sp[0][2] == 0 and all(s[2] == 1 for s in sp[1:]) and sum(s[1] for s in sp) == c.total, c.id
            assert all(not (b == 0 and n == c.total) for b, n, _ in sp), c.id  # (every launch is a true sub-range)
        for c in one:
            assert c.shard and not c.lazy and sx.spans(c) == [(0, c.total, 0)], c.id
        # the two sides of N >= 5 count, by one candidate
        assert any(c.N == sx.AUX_RATIO * c.shard[1] for c in three)
        assert any(c.N == sx.AUX_RATIO * c.shard[1] - 1 and not c.levers for c in one)
        # every three-range shard also runs under MBD_NO_AUX
        aux = {(c.env, c.N, c.H, c.shard, c.kind) for c in one if c.levers.get("MBD_NO_AUX")}
        assert {(c.env, c.N, c.H, c.shard, c.kind) for c in three if c.env == "hopper" and c.N == 45} <= aux
        half = lambda c: (c.total + 1) // 2  # noqa: E731
        own = lambda c: (c.shard[0] * c.HNu, (c.shard[0] + c.shard[1]) * c.HNu)  # noqa: E731
        assert any(own(c)[1] <= half(c) and own(c)[0] > 0 for c in three), "own rows entirely below half"
        assert any(own(c)[0] >= half(c) and own(c)[1] < c.total for c in three), "own rows entirely above half"
        assert any(own(c)[0] < half(c) < own(c)[1] and half(c) % c.HNu for c in three), "own rows straddling half, inside a row"
        assert any(c.shard[0] == 0 for c in three) and any(c.shard[0] + c.shard[1] == c.N for c in three)
        assert any(c.total % 2 == 1 for c in three) and any(c.total % 2 == 0 for c in three)
        # a range of more than one workgroup that starts off a multiple of 256, rows coprime to 256
        assert any(s[0] % 256 and s[1] > 512 and np.gcd(c.HNu, 256) == 1 for c in three for s in sx.spans(c))
        assert any(c.kind == "pi" for c in three) and any(c.env == "car2d" for c in three)
        assert any(c.kind == "mbd" and c.levers.get("MBD_NO_LAZY") for c in three)


def test_cap_cases_fall_either_side_of_the_grid_caps():
    large = sx.cases(large=True)
    assert len(large) == 4 and all(c.form == "noise" and c.lazy and c.shard is None for c in large)
    assert all(c.total > sx.WHOLE_LIMIT for c in large)
    for lay, row_items in ((sx.PARTITIONABLE, 256), (sx.LEGACY, 128)):
        items = sorted(c.items for c in large if c.layout == lay)
        assert items == [sx.NOISE_CAP, sx.NOISE_CAP + row_items], (lay, items)
    # what a lazy plan of the largest case allocates: Y0s and three rings of normals — well under 1 GB
    assert 4 * 4 * max(c.total for c in large) < 0.6e9
    assert all(c.items <= sx.NOISE_CAP // 16 for c in sx.cases(large=False))
    for env, N, H, steps, kind in sx.SWEEPS:
        total = N * H * sx.NU[env]
        assert (total + 1) // 2 > sx.BATCH_CAP and steps >= 2, (env, N)
        assert N <= 12288, "mbd_sweep_create refuses larger plans"
    assert any(kind == "pi" and (N * H * sx.NU[env]) % 2 == 1 for env, N, H, _, kind in sx.SWEEPS)
    assert any(kind == "mbd" for *_, kind in sx.SWEEPS)
    counts = [E * sx.NU["humanoidrun"] + 3 for E in sx.PLANT_E]
    # one workgroup of 256 threads: elements (partitionable) wrap above 256, pairs (legacy) above 512
    assert min(counts) < 256 < sorted(counts)[1] and sorted(counts)[2] < 512 < max(counts)
    assert {n % 2 for n in counts} == {0, 1}
    assert all(E <= 50 for E in sx.PLANT_E)


def test_sigmas_of_the_non_saturating_cases_cannot_clip(orc):
    _, _, sig = orc.schedule(1e-4, 1e-2, sx.ND)
    assert sx.MAX_ABS_NORMAL * float(sig[sx.I_SMALL]) < 1.0 and sx.MAX_ABS_NORMAL * sx.PI_SIGMA_SMALL < 1.0
    # the largest sigma of the schedule: normals beyond three deviations saturate even on a zero mean
    assert sx.I_LARGE == sx.ND - 1 and sig[sx.I_LARGE] == sig.max() and 3.0 * float(sig[sx.I_LARGE]) > 1.0


def test_fused_noise_cases_select_the_launch_they_claim(lib, levers):
    """choose_rollout for the rollout of every fused case (its shard), on a 256-CU device, under the case's levers: pinned
    or not, the noise job taken or not, and — restating launch_rollout's arithmetic — how the noise workgroups compare with
    the items they stride over."""
    from mbd_hip import _capi
    all_levers = sorted({k for c in sx.cases("fused") for k in c.levers})
    seen = set()
    for c in sx.cases("fused"):
        for k in all_levers:
            levers(**{k: c.levers.get(k, -1)})
        B = c.shard[1] if c.shard else c.N
        ch = _capi.debug_rollout_choice(load_model(c.env).to_struct(), sx.N_CUS, B, c.H)
        grid, block, pin = ch["grid"], ch["block"], bool(ch["xcd_pin"])
        assert pin == c.expect["pin"], (c.id, ch)
        assert bool(ch["fuses_noise"]) == (not c.levers.get("MBD_NO_FUSED_NOISE")), (c.id, ch)
        if pin:
            assert block == 256 and (9 <= grid <= 32 if c.levers.get("MBD_ROLL_PIN") == 1 else grid <= 8), (c.id, ch)
            threads = 7 * grid * block
            fits = c.items <= 256 * threads
            fused = bool(ch["fuses_noise"]) and fits
            wrap = c.items > threads
            if not fits:
                assert grid == 1 and c.shard, c.id
                seen.add("nz_fits false")
        else:
            need, spare = -(-c.items // block), sx.N_CUS - grid
            assert spare > 0
            fused = bool(ch["fuses_noise"]) and min(need, spare) > 0
            wrap = need > spare
            if fused and not wrap:
                assert c.items % block, f"{c.id}: the last noise workgroup is partial"
        assert fused == c.expect["fused"], (c.id, ch)
        if fused:
            assert wrap == c.expect["wrap"], (c.id, ch)
            seen.add(("pinned" if pin else "plain") + (" wrap" if wrap else " no wrap"))
            if c.levers.get("MBD_ROLL_PIN") == 1:
                seen.add("pinned on request")
        elif c.levers.get("MBD_NO_FUSED_NOISE"):
            seen.add("second stream by lever")
    for k in all_levers:
        levers(**{k: -1})
    assert seen == {"plain wrap", "plain no wrap", "pinned wrap", "pinned no wrap", "pinned on request", "nz_fits false",
                    "second stream by lever"}, seen
