"""The adapt record without a GPU (include/mbd_hip.h mbd_adapt, mbd_plan_set_adapt, mbd_plan_peek_adapt; DESIGN.md section 1 "N17
adapt").

The two calls are exported and declared; the ctypes record has the header's layout; what the record alone decides is refused with
the field's name before any device is touched; the kernels' per-element functions, looped on the host through mbd_debug_adapt_host
(one text for host and device), keep the bits of the checker's restatement (tests/adapt_checker.py) at every size of the table
below, lazy and materialised; the rule does what it is for on a synthetic problem, on the checker alone; and the records and inputs
the GPU tests use (tests/test_gpu_adapt.py imports them from here) are told apart by the checker, field by field."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import adapt_cases as cases
import adapt_checker as ac
import weighting_checker as wc
from conftest import ROOT
from state_inputs import same_bits

f32 = np.float32

# ---- the inputs of the step tests, shared with tests/test_gpu_adapt.py -----------------------------------------------------------
HOST_N, HOST_HNU = (1, 33, 64, 70, 1029), (12, 21, 85)
NU_OF = {12: 3, 21: 3, 32: 8, 85: 17, 2100: 21}  # HNu read as [H][Nu]: the frozen column is actuator 1
WIDE_HNU = 2100  # more elements than one chunk (2048) of the finish kernel's sum
KINDS = ("zeros", "equal", "ties", "one")
RULE = cases.RULE  # the GPU tests' record
SIGMA = f32(0.37)


def shape_of(HNu, frozen=True):
    """Distinct g[h][a] in [0.5, 1.5], actuator 1 frozen (a zero column)."""
    g = np.linspace(0.5, 1.5, HNu, dtype=np.float64).astype(f32).reshape(-1, NU_OF[HNu])
    if frozen:
        g[:, 1] = 0.0
    return g.reshape(-1)


def step_case(N, HNu, lazy, kind, with_shape=True):
    """dict(w [N], cand [N, HNu] (normals if lazy, else values), Y (values), ybar, sigma, a, g).  The weights favour candidates
    whose first half of the elements lies near a target, so selection narrows those elements and not the others; ``kind``: "zeros"
    every fifth weight exactly +0, "equal" all weights 1 / N, "ties" the weights in equal pairs, "one" all weight on one candidate."""
    rng = np.random.default_rng([N, HNu, int(lazy), KINDS.index(kind)])
    ybar = (rng.normal(size=HNu) * 0.3).astype(f32)
    g = shape_of(HNu) if with_shape else None
    a = rng.uniform(RULE.a_min, RULE.a_max, size=HNu).astype(f32)
    G = a if g is None else (a * g).astype(f32)
    z = (rng.normal(size=(N, HNu)).astype(f32) * G[None]).astype(f32)
    Y = ac.values(z, SIGMA, ybar)
    half = max(HNu // 2, 1)
    cost = ((Y[:, :half] - f32(0.1)) ** 2).sum(axis=1).astype(np.float64)
    w = np.exp(-(cost - cost.min()) * 4.0)
    if kind == "zeros":
        w[::5] = 0.0
        if not w.any():
            w[0] = 1.0
    elif kind == "equal":
        w[:] = 1.0
    elif kind == "ties":
        w[1::2] = w[:-1:2][: w[1::2].shape[0]]
    elif kind == "one":
        w[:] = 0.0
        w[N // 2] = 1.0
    w = (w / w.sum()).astype(f32)
    return dict(w=w, cand=z if lazy else Y, Y=Y, ybar=ybar, sigma=SIGMA, a=a, g=g)


def checked(orc, c, rule=RULE):
    return ac.update(orc, c["w"], c["Y"], c["ybar"], c["sigma"], c["a"], c["g"], rule)


def assert_step(got, ref, what):
    a, G, S, skipped = got
    assert skipped == int(ref["skipped"]), f"{what}: skipped {skipped}, the checker {ref['skipped']}"
    if np.isnan(ref["S"]):
        assert np.isnan(S), what
    else:
        same_bits(S, ref["S"], f"{what}: S")
    same_bits(a, ref["a"], f"{what}: a'")
    same_bits(G, ref["G"], f"{what}: G'")


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_the_calls_are_exported_and_declared(lib):
    from mbd_hip import _capi
    for name in ("mbd_plan_set_adapt", "mbd_plan_peek_adapt"):
        assert name in _capi.EXPORTS and hasattr(lib, name), name
    for name in ("mbd_debug_adapt_host", "mbd_debug_adapt_step", "mbd_debug_check_adapt"):
        assert hasattr(lib, name), name
    text = open(os.path.join(ROOT, "include", "mbd_hip.h")).read()
    for name in ("typedef struct mbd_adapt", "int mbd_plan_set_adapt(", "int mbd_plan_peek_adapt(", "wsum64", "G'[e] = a'[e] * g[e]",
                 "a_min == a_max == 1", "A frozen element stays frozen"):
        assert name in text, name
    dbg = open(os.path.join(ROOT, "include", "mbd_hip_debug.h")).read()
    for name in ("mbd_debug_adapt_host", "mbd_debug_adapt_step"):
        assert name in dbg, name


def test_the_ctypes_record_has_the_headers_layout(tmp_path):
    from mbd_hip import _capi
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a C compiler is what builds the checker as well"
    fields = ("rate", "a_min", "a_max", "carry", "reserved")
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mbd_hip.h"\nint main(void) { printf("%zu", sizeof(mbd_adapt));\n'
                   + "".join(f'printf(" %zu", offsetof(mbd_adapt, {f}));\n' for f in fields) + "return 0; }\n")
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = _capi.Adapt
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in fields] and C.sizeof(S) == 32


def test_refusals_come_before_any_device_access(lib):
    """On a box with no device: a NULL handle; on a zeroed stand-in handle (update_method 0, unsharded, no session, no record)
    every bad field with its name, a NULL record (nothing to clear) accepted, and peek without a record; through
    mbd_debug_check_adapt the refusals the handle's update_method and enable_demo decide."""
    from mbd_hip import _capi
    ok = _capi.adapt_record(0.3, 0.25, 4.0)
    n = C.c_int(0)
    assert lib.mbd_plan_set_adapt(None, C.byref(ok)) == _capi.MBD_ERR_INVALID and b"plan" in lib.mbd_last_error()
    assert lib.mbd_plan_peek_adapt(None, None, None, None, 0, C.byref(n)) == _capi.MBD_ERR_INVALID
    stand_in = C.create_string_buffer(1 << 16)
    bad = [(dict(rate=0.0), b"rate"), (dict(rate=1.5), b"rate"), (dict(rate=float("nan")), b"rate"), (dict(rate=-0.1), b"rate"),
           (dict(a_min=0.0), b"a_min"), (dict(a_min=1.5), b"a_min"), (dict(a_min=float("nan")), b"a_min"),
           (dict(a_max=0.5), b"a_max"), (dict(a_max=float("inf")), b"a_max"), (dict(a_max=float("nan")), b"a_max"),
           (dict(carry=2), b"carry=2"), (dict(carry=-1), b"carry=-1")]
    for kw, field in bad:
        rec = _capi.adapt_record(**dict(dict(rate=0.3, a_min=0.25, a_max=4.0, carry=1), **kw))
        for rc in (lib.mbd_plan_set_adapt(stand_in, C.byref(rec)), _capi.debug_check_adapt(rec)):
            assert rc == _capi.MBD_ERR_INVALID and field in lib.mbd_last_error(), (kw, rc, lib.mbd_last_error())
    for r in range(4):
        rec = _capi.adapt_record(0.3, 0.25, 4.0)
        rec.reserved[r] = 9
        assert lib.mbd_plan_set_adapt(stand_in, C.byref(rec)) == _capi.MBD_ERR_INVALID
        assert b"reserved[%d]=9" % r in lib.mbd_last_error()
    assert lib.mbd_plan_set_adapt(stand_in, None) == _capi.MBD_OK  # (nothing to clear)
    assert lib.mbd_plan_peek_adapt(stand_in, None, None, None, 0, C.byref(n)) == _capi.MBD_ERR_STATE
    assert b"no adapt record" in lib.mbd_last_error()
    assert not any(bytes(stand_in.raw))
    # the handle's configuration: the field checks come first, then update_method, then enable_demo
    assert _capi.debug_check_adapt(ok, 0) == _capi.MBD_OK and _capi.debug_check_adapt(ok, 1) == _capi.MBD_OK
    assert _capi.debug_check_adapt(_capi.adapt_record(1.0, 1.0, 1.0, False)) == _capi.MBD_OK  # (the bounds themselves are allowed)
    for m in (2, 3):
        assert _capi.debug_check_adapt(ok, m) == _capi.MBD_ERR_UNSUPPORTED and b"update_method=%d" % m in lib.mbd_last_error()
        assert _capi.debug_check_adapt(_capi.adapt_record(2.0, 0.25, 4.0), m) == _capi.MBD_ERR_INVALID
    assert _capi.debug_check_adapt(ok, 0, True) == _capi.MBD_ERR_UNSUPPORTED and b"enable_demo" in lib.mbd_last_error()
    assert _capi.debug_check_adapt(None) == _capi.MBD_ERR_INVALID
    # the debug entries check their rule as the set call does, and their sizes
    c = step_case(4, 12, False, "equal")
    with pytest.raises(_capi.MbdError) as e:
        _capi.debug_adapt_host(c["w"], c["cand"], c["ybar"], c["sigma"], False, c["a"], c["g"], 0.0, 0.5, 2.0)
    assert e.value.code == _capi.MBD_ERR_INVALID and b"rate" in lib.mbd_last_error()


# ---- the kernels' per-element functions, on the host -------------------------------------------------------------------------------
@pytest.mark.parametrize("lazy", [False, True], ids=["values", "lazy"])
@pytest.mark.parametrize("HNu", HOST_HNU)
@pytest.mark.parametrize("N", HOST_N)
def test_host_entry_against_the_checker(lib, orc, N, HNu, lazy):
    """Every kind of weights, under a shape with a frozen column and without one: a', G', S and skipped, bit for bit.  All weight on
    one candidate (and N = 1) is skipped and leaves a as it was; a frozen column keeps its a and G = 0."""
    from mbd_hip import _capi
    skipped = 0
    for kind in KINDS:
        for with_shape in (True, False):
            c = step_case(N, HNu, lazy, kind, with_shape)
            ref = checked(orc, c)
            what = f"N={N} HNu={HNu} lazy={lazy} {kind} shape={with_shape}"
            got = _capi.debug_adapt_host(c["w"], c["cand"], c["ybar"], c["sigma"], lazy, c["a"], c["g"], RULE.rate, RULE.a_min, RULE.a_max)
            assert_step(got, ref, what)
            if kind == "one" or N == 1:
                assert ref["skipped"], f"{what}: one candidate carries all weight, every var is zero"
                same_bits(got[0], c["a"], f"{what}: a skipped step leaves a as it was")
            elif N >= 33:
                assert not ref["skipped"] and np.isfinite(ref["S"]) and ref["S"] > 0, what
                assert not np.array_equal(ref["a"], c["a"]), f"{what}: the step moves the table"
                assert (ref["a"] >= f32(RULE.a_min)).all() and (ref["a"] <= f32(RULE.a_max)).all(), what
            if with_shape:
                col = np.arange(HNu) % NU_OF[HNu] == 1
                same_bits(got[0][col], c["a"][col], f"{what}: a frozen column keeps its a")
                assert (got[1][col].view(np.uint32) << 1 == 0).all(), f"{what}: a frozen column stays frozen"
            skipped += int(ref["skipped"])
    assert skipped >= 2


def test_host_entry_beyond_one_chunk_of_the_sum(lib, orc):
    """HNu = 2100: the finish kernel sums S in chunks of 2048 elements; the host entry and the checker agree there as well (the GPU
    test of that size shares these inputs)."""
    from mbd_hip import _capi
    for lazy in (False, True):
        c = step_case(33, WIDE_HNU, lazy, "equal")  # (over 1050 elements the cost-driven weights collapse onto one candidate)
        ref = checked(orc, c)
        assert not ref["skipped"]
        got = _capi.debug_adapt_host(c["w"], c["cand"], c["ybar"], c["sigma"], lazy, c["a"], c["g"], RULE.rate, RULE.a_min, RULE.a_max)
        assert_step(got, ref, f"HNu={WIDE_HNU} lazy={lazy}")


def test_identity_rule_keeps_the_shape(lib, orc):
    """a_min = a_max = 1: whatever the step finds, a stays all ones and G is g bit for bit (the plan then keeps the bits of the plan
    without a record) — the library's host entry and the checker alike."""
    from mbd_hip import _capi
    one = ac.Record(rate=0.7, a_min=1.0, a_max=1.0)
    for HNu in HOST_HNU:
        c = step_case(70, HNu, False, "zeros")
        c["a"] = np.ones(HNu, f32)
        ref = ac.update(orc, c["w"], c["Y"], c["ybar"], c["sigma"], c["a"], c["g"], one)
        got = _capi.debug_adapt_host(c["w"], c["cand"], c["ybar"], c["sigma"], False, c["a"], c["g"], one.rate, one.a_min, one.a_max)
        assert not ref["skipped"] and got[3] == 0
        for a, G in ((ref["a"], ref["G"]), got[:2]):
            same_bits(a, np.ones(HNu, f32), "a")
            same_bits(G, c["g"], "G")


BIG_N = (12289, 12300)  # beyond the 12288 weights the spread kernel stages in LDS: one past the boundary; ragged groups, the 32-row round


@pytest.mark.parametrize("N", BIG_N)
def test_host_entry_beyond_the_lds_window(lib, orc, N):
    """The sizes at which the GPU tests run the spread kernel's unstaged form (they share these inputs): the host entry and the
    checker agree, lazy and materialised, and the step is not skipped."""
    from mbd_hip import _capi
    for HNu in (12, 21):
        for lazy in (False, True):
            c = step_case(N, HNu, lazy, "zeros")
            ref = checked(orc, c)
            assert not ref["skipped"]
            got = _capi.debug_adapt_host(c["w"], c["cand"], c["ybar"], c["sigma"], lazy, c["a"], c["g"], RULE.rate, RULE.a_min, RULE.a_max)
            assert_step(got, ref, f"N={N} HNu={HNu} lazy={lazy}")


# ---- what the rule is for ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(8))
def test_the_rule_moves_noise_to_where_it_is_not_wasted(orc, seed):
    """A synthetic reward -5 sum_{e<4} (Y_e - 0.3)^2 over 8 elements, N = 256, sigma 0.2, temperature 0.1, rate 0.3, clamps 0.25 and
    4, 40 steps of sample / weigh / weighted mean / update from a zero mean: the four rewarded elements end narrower than the four
    free ones, and the mean within 0.02 of 0.3 on the four."""
    N, HNu, sigma = 256, 8, f32(0.2)
    rec = ac.Record(rate=0.3, a_min=0.25, a_max=4.0)
    rng = np.random.default_rng(seed)
    a, m = np.ones(HNu, f32), np.zeros(HNu, f32)
    for _ in range(40):
        z = (rng.standard_normal((N, HNu)).astype(f32) * a[None]).astype(f32)
        Y = ac.values(z, sigma, m)
        r = (f32(-5) * ((Y[:, :4] - f32(0.3)) ** 2).sum(axis=1)).astype(f32)
        w = wc.weigh(orc, r, 0.1)["weights"]
        res = ac.update(orc, w, Y, m, sigma, a, None, rec)
        assert not res["skipped"]
        m, a = wc.wmean(orc, w, Y), res["a"]
    assert a[:4].max() < a[4:].min(), a
    assert np.abs(m[:4] - f32(0.3)).max() < 0.02, m


# ---- the GPU tests' records and inputs, told apart -----------------------------------------------------------------------------------
GPU_SIZES, plan_shape = cases.SIZES, cases.plan_shape


@pytest.mark.parametrize("name", sorted(GPU_SIZES))
def test_the_gpu_tests_records_are_told_apart(orc, name):
    """At the GPU tests' sizes, on inputs of this file's kind: changing rate, a_min or a_max alone changes the table the update
    leaves, and carry alone changes the table a warm tick starts from."""
    N, H, Nu = GPU_SIZES[name]
    HNu = H * Nu
    rng = np.random.default_rng([N, H, Nu])
    ybar = (rng.normal(size=HNu) * 0.3).astype(f32)
    g = plan_shape(H, Nu).reshape(-1)
    a = rng.uniform(RULE.a_min, RULE.a_max, size=HNu).astype(f32)
    Y = ac.values((rng.normal(size=(N, HNu)).astype(f32) * (a * g)[None]).astype(f32), SIGMA, ybar)
    cost = ((Y[:, : HNu // 2] - f32(0.1)) ** 2).sum(axis=1).astype(np.float64)
    w = np.exp(-(cost - cost.min()) * 4.0)
    w = (w / w.sum()).astype(f32)
    ref = ac.update(orc, w, Y, ybar, SIGMA, a, g, RULE)
    assert not ref["skipped"]
    assert ref["a"].min() < f32(0.9) and ref["a"].max() > f32(1.1), "the table spreads to both sides of the tighter clamps below"
    for kw in (dict(rate=0.25), dict(a_min=0.9), dict(a_max=1.1)):
        other = ac.update(orc, w, Y, ybar, SIGMA, a, g, ac.Record(**dict(RULE.kwargs(), **kw)))
        assert not np.array_equal(other["a"], ref["a"]), kw
    st = [ac.State(ac.Record(**dict(RULE.kwargs(), carry=c)), H, Nu, g, g) for c in (True, False)]
    for s in st:
        s.a = ref["a"].copy()
        s.tick(False, 2)
    assert not np.array_equal(st[0].a, st[1].a) and (st[1].a == 1).all()
    same_bits(st[0].a[: HNu - 2 * Nu], ref["a"][2 * Nu:], "carry shifts the table E rows forward")
    assert (st[0].a[HNu - 2 * Nu:] == 1).all()


@pytest.mark.parametrize("case", cases.PLAN_CASES, ids=[c.id for c in cases.PLAN_CASES])
def test_the_whole_plan_cases_skip_no_step(orc, case):
    """The checker alone, from the env's reset state: every step of every whole-plan case of the GPU tests updates the table (none
    is skipped), S is finite and positive, the table stays inside the clamp and leaves all-ones, and a frozen element keeps a = 1."""
    oenv, s0 = cases.cpu_env(orc, case.name)
    s0 = s0 if case.state0 is None else case.state0
    ref = cases.plan_reference(orc, oenv, s0, orc.prng_key(4), case)
    N, H, Nu = cases.SIZES[case.name]
    assert len(ref["log"]) == cases.ND - 1 and ref["tables"].shape == (cases.ND - 1, H * Nu)
    for j, (S, skipped) in enumerate(ref["log"]):
        assert not skipped and np.isfinite(S) and S > 0, f"{case.id}: step {j} S={S!r}"
    assert np.isfinite(ref["mu_0ts"]).all()
    tab = ref["tables"]
    assert (tab >= f32(RULE.a_min)).all() and (tab <= f32(RULE.a_max)).all() and not (tab[-1] == 1).all()
    if case.shape:
        assert (tab[:, 1 * Nu + Nu - 1] == 1).all(), "the frozen element keeps its a"


@pytest.mark.parametrize("case", cases.EPISODE_CASES, ids=[c.id for c in cases.EPISODE_CASES])
def test_the_episode_cases_skip_no_step(orc, case):
    """The same for the episodes: (Ndiffuse - 1) + (T - 1) K updates, none skipped; without carry every warm tick's table is K
    updates away from ones, with carry the appended rows start from 1."""
    oenv, s0 = cases.cpu_env(orc, case.name)
    ref = cases.episode_reference(orc, oenv, s0, orc.prng_key(4), case)
    assert len(ref["log"]) == (cases.ND - 1) + (cases.T - 1) * cases.K
    for j, (S, skipped) in enumerate(ref["log"]):
        assert not skipped and np.isfinite(S) and S > 0, f"{case.id}: step {j} S={S!r}"
    assert np.isfinite(ref["means"]).all() and ref["tables"].shape[0] == cases.T


def test_cli_flags_map_to_the_record():
    """mpc.MpcArgs' adapt flags: none set means no record; each flag reaches the argument of ``Plan.set_adapt`` it names."""
    from mbd_hip.planners import mpc
    assert not mpc._has_adapt(mpc.MpcArgs()) and mpc._adapt_settings(mpc.MpcArgs()) == {}
    a = mpc.MpcArgs(adapt_rate=0.3)
    assert mpc._has_adapt(a) and mpc._adapt_of(a) == dict(rate=0.3, a_min=0.25, a_max=4.0, carry=False)
    a = mpc.MpcArgs(adapt_rate=0.5, adapt_min=0.5, adapt_max=2.0, adapt_carry=True)
    assert mpc._adapt_of(a) == dict(rate=0.5, a_min=0.5, a_max=2.0, carry=True)
    assert mpc._adapt_settings(a) == dict(adapt_rate=0.5, adapt_min=0.5, adapt_max=2.0, adapt_carry=True)
    from mbd_hip import _capi
    rec = _capi.adapt_record(**mpc._adapt_of(a))
    assert (f32(rec.rate), f32(rec.a_min), f32(rec.a_max), rec.carry) == (f32(0.5), f32(0.5), f32(2.0), 1)
    with pytest.raises(ValueError, match="adapt_rate"):  # (sweeps take no adapt record)
        mpc._check_batch([mpc.MpcArgs(env_name="hopper", adapt_rate=0.3)] * 2)
