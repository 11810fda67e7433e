"""The elite record without a GPU (include/mbd_hip.h mbd_elites, mbd_plan_set_elites, mbd_plan_peek_elites; DESIGN.md section 1 "N18
elites").

The calls are exported and declared; the ctypes record has the header's layout; what the record alone decides is refused with the
field's name before any device is touched; the kernels' per-element functions and their order, looped on the host through
mbd_debug_elites_host (one text for host and device), keep the bits of the checker's restatement (tests/elites_checker.py) over the
table of tests/elites_inputs.py, lazy and materialised; and the checker itself keeps the invariants the contract promises."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import elites_checker as ec
import elites_inputs as inputs
from conftest import ROOT
from state_inputs import same_bits

f32 = np.float32


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_the_calls_are_exported_and_declared(lib):
    from mbd_hip import _capi
    for name in ("mbd_plan_set_elites", "mbd_plan_peek_elites"):
        assert name in _capi.EXPORTS and hasattr(lib, name), name
    for name in ("mbd_debug_elites_host", "mbd_debug_elites_select", "mbd_debug_elites_inject", "mbd_debug_check_elites"):
        assert hasattr(lib, name), name
    text = open(os.path.join(ROOT, "include", "mbd_hip.h")).read()
    for name in ("typedef struct mbd_elites", "int mbd_plan_set_elites(", "int mbd_plan_peek_elites(", "NOT E[j] bit for bit",
                 "(E[j][e] - Ybar_i[e]) / sigma_i", "0x7fc00000", "A frozen element therefore stays frozen"):
        assert name in text, name
    dbg = open(os.path.join(ROOT, "include", "mbd_hip_debug.h")).read()
    for name in ("mbd_debug_elites_host", "mbd_debug_elites_select", "mbd_debug_elites_inject", "mbd_debug_check_elites"):
        assert name in dbg, name


def test_the_ctypes_record_has_the_headers_layout(tmp_path):
    from mbd_hip import _capi
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a C compiler is what builds the checker as well"
    fields = ("n_elites", "nominal", "carry", "reserved")
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mbd_hip.h"\nint main(void) { printf("%zu", sizeof(mbd_elites));\n'
                   + "".join(f'printf(" %zu", offsetof(mbd_elites, {f}));\n' for f in fields) + "return 0; }\n")
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = _capi.Elites
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in fields] and C.sizeof(S) == 32


def test_refusals_come_before_any_device_access(lib):
    """A NULL handle; through mbd_debug_check_elites every refusal the record alone decides, in the header's order, each naming its
    field; a good record accepted."""
    from mbd_hip import _capi
    rec = _capi.elites_record(3, True, True)
    assert lib.mbd_plan_set_elites(None, C.byref(rec)) == _capi.MBD_ERR_INVALID
    assert lib.mbd_plan_peek_elites(None, None, None, None, None, None, None, None, 0, None) == _capi.MBD_ERR_INVALID
    assert _capi.debug_check_elites(None, 64) == _capi.MBD_ERR_INVALID

    def refused(code, word, N=64, method=0, demo=False, **fields):
        r = _capi.elites_record(3, True, False)
        for k, v in fields.items():
            if k.startswith("reserved"):
                r.reserved[int(k[8:])] = v
            else:
                setattr(r, k, v)
        assert _capi.debug_check_elites(r, N, method, demo) == code, (fields, N, method, demo)
        assert word.encode() in lib.mbd_last_error(), (word, lib.mbd_last_error())

    I, U = _capi.MBD_ERR_INVALID, _capi.MBD_ERR_UNSUPPORTED
    refused(I, "n_elites=-1", n_elites=-1)
    refused(I, "n_elites=33", n_elites=33)
    refused(I, "nominal=2", nominal=2)
    refused(I, "nominal=-1", nominal=-1)
    refused(I, "carry=2", carry=2)
    refused(I, "n_elites=0 with nominal=0", n_elites=0, nominal=0)
    refused(I, "Nsample=4", N=4)            # 3 + 1 >= 4
    refused(I, "Nsample=3", N=3, nominal=0)  # 3 + 0 >= 3
    for k in range(5):
        refused(I, f"reserved[{k}]", **{f"reserved{k}": 1})
    refused(U, "update_method=2", method=2)
    refused(U, "update_method=3", method=3)
    refused(U, "enable_demo", demo=True)
    refused(I, "n_elites=33", n_elites=33, method=3)  # (the record's own fields come first)
    for n, nom, N in ((3, 1, 5), (32, 1, 34), (0, 1, 2), (1, 0, 2), (32, 0, 33)):
        assert _capi.debug_check_elites(_capi.elites_record(n, nom, True), N, 1) == _capi.MBD_OK, (n, nom, N)


# ---- the host restatement against the checker ---------------------------------------------------------------------------------------
def _host(c, **kw):
    from mbd_hip import _capi
    a = dict(c, **kw)
    return _capi.debug_elites_host(a["rews"], a["cand"], a["ybar"], a["sigma"], a["lazy"], a["g"], a["rec"].n_elites,
                                   int(a["rec"].nominal), a["E_in"])


@pytest.mark.parametrize("N", inputs.NS)
def test_the_host_form_keeps_the_checkers_bits(lib, N):
    """mbd_debug_elites_host over the table: every k and kind of rewards at this N, lazy and materialised, by bit pattern; sizes at
    which the record would be refused are refused here as well."""
    from mbd_hip import _capi
    cases = [c for c in inputs.table() if c["N"] == N]
    if N <= 2:  # (k + nominal >= N for most of the table: the entry refuses as the set call does)
        bad = inputs.case(64, 1, "random", True)
        with pytest.raises(_capi.MbdError) as e:
            _host(bad, rews=bad["rews"][:N], cand=bad["cand"][:N])
        assert e.value.code == _capi.MBD_ERR_INVALID and "must lie below N" in str(e.value)
    else:
        assert len(cases) >= 2 * len(inputs.KINDS) * 2
    for c in cases:
        ref = inputs.checked(c)
        inputs.assert_step(_host(c), ref, inputs.what(c), same_bits)
        n_fin = int(ec.finite(c["rews"]).sum())
        assert ref["count"] == min(c["k"], n_fin), inputs.what(c)
        if c["kind"] == "none":
            assert ref["count"] == 0 and np.asarray(ref["top"], f32).view(np.uint32) == 0x7fc00000
        if c["kind"] == "few":
            assert ref["count"] == min(c["k"], 3)


def test_the_table_reaches_what_it_is_for():
    """The inputs do what their names say, on the checker alone: ties whose winners cross the wavefronts' and the workgroup's
    boundaries, +0 beside -0 in index order, planted non-finite entries never selected, an injected slot kept."""
    c = inputs.case(2049, 32, "ties", False)
    ref = inputs.checked(c)
    assert list(ref["src"][:5]) == [63, 64, 1023, 1024, 2048] and (ref["R"][:5] == 7).all() and (ref["R"][5:] == 3).all()
    assert list(ref["src"][5:]) == sorted(ref["src"][5:])
    c = inputs.case(1025, 32, "zeros", True)
    ref = inputs.checked(c)
    assert (ref["R"] == 0).all() and list(ref["src"]) == sorted(ref["src"])
    signs = np.signbit(ref["R"])
    assert signs.any() and not signs.all(), "+0 and -0 tie: both are among the winners, in index order"
    c = inputs.case(8193, 32, "nonfinite", False)
    ref = inputs.checked(c)
    assert not set(ref["src"]) & set(inputs.PLANTED + (8192, 5)) and ref["src"][0] == 6
    c = inputs.case(64, 5, "equal", False, nominal=1)
    ref = inputs.checked(c)
    assert list(ref["src"]) == [0, 1, 2, 3, 4] and ref["kept"] == 3  # (the nominal and the two elites the step found)
    same_bits(ref["cand"][0], ec.clip(c["ybar"]), "the nominal of a materialised plan")
    same_bits(ref["cand"][1:3], c["E_in"], "the elites of a materialised plan")
    same_bits(ref["cand"][3:], c["cand"][3:], "the rows from slots on")
    c = inputs.case(64, 5, "equal", True, nominal=1)
    ref = inputs.checked(c)
    z = ref["cand"]
    assert (z[0].view(np.uint32) == 0).all() and (z[1:3, 2].view(np.uint32) == 0).all(), "the nominal's z and a frozen element's: +0"
    same_bits(z[3:], c["cand"][3:], "the normals from slots on")
    assert not np.array_equal(ref["E"][1:3], c["E_in"]), "a lazy elite is its z's value, not E[j] bit for bit (a frozen element)"
    far = np.delete(np.arange(inputs.HNU), 2)
    assert np.abs(ref["E"][1:3][:, far] - c["E_in"][:, far]).max() < 1e-6


def test_selection_is_a_strict_total_order():
    """No selected index is non-finite and src' is strictly ordered under pick_before, for every input of the table."""
    for c in inputs.table():
        ref = inputs.checked(c)
        r, src = c["rews"], list(ref["src"])
        assert ec.finite(r[src]).all() and len(set(src)) == len(src), inputs.what(c)
        for a, b in zip(src[:-1], src[1:]):
            assert ec.before(r[a], a, r[b], b) and not ec.before(r[b], b, r[a], a), inputs.what(c)
        rest = [i for i in np.flatnonzero(ec.finite(r)) if i not in set(src)]
        if src and rest and len(src) == c["k"]:
            assert all(ec.before(r[src[-1]], src[-1], r[i], i) for i in rest), inputs.what(c)


def test_the_tick_boundary_is_the_means_shift():
    from mpc_checker import shift
    st = ec.State(ec.Record(2, True, True), 4, 3, False)
    st.E = np.arange(24, dtype=f32).reshape(2, 12) + 1
    want = np.stack([shift(e.reshape(4, 3), 2).reshape(-1) for e in st.E])
    st.tick(False, 2)
    same_bits(st.E, want, "carry = 1: every present elite shifted with zeros behind it")
    assert st.count == 2
    st.tick(True, 2)
    assert st.count == 0, "a cold tick starts without elites"
    st.E = np.ones((2, 12), f32)
    st.rec = ec.Record(2, True, False)
    st.tick(False, 2)
    assert st.count == 0, "carry = 0: every tick starts without elites"


# ---- the checker's invariants on whole plans ----------------------------------------------------------------------------------------
def _run(orc, name, method, rec, s0=None, **kw):
    oenv, reset = inputs.cpu_env(orc, name)
    N, H, Nu = inputs.SIZES[name]
    st = ec.State(rec, H, Nu, inputs.lazy_of(name, method))
    s0 = reset if s0 is None else np.asarray(s0, f32)
    key = orc.prng_key(4)
    if method:
        out = ec.pi_run(oenv, s0, key, N, H, inputs.ND, inputs.TEMP, 1, st, **kw)
    else:
        out = ec.run(orc, oenv, s0, key, N, H, inputs.ND, inputs.TEMP, st, **kw)
    return oenv, s0, st, out


@pytest.mark.parametrize("method", [0, 1], ids=["mbd", "mppi"])
def test_on_car2d_top_never_decreases(orc, method):
    """car2d's candidates are materialised, so an elite is re-evaluated exactly: within a run the best return of a step is at
    least the previous step's, and the elites a step found are the first rows of the next step's candidates."""
    _, _, st, out = _run(orc, "car2d", method, ec.Record(3, True, False), s0=inputs.ac_cases.CAR2D_S0)
    tops = [t for _, _, t in st.log]
    assert len(tops) == inputs.ND - 1 and all(np.isfinite(tops))
    assert all(b >= a for a, b in zip(tops[:-1], tops[1:])), tops
    if method:  # (mppi samples with sigma = 1; the MBD steps of six-step schedule stay so close to the mean that all rewards tie)
        assert tops[-1] > tops[0], "the candidates' rewards differ from this start state"
    else:
        assert all(list(s["src"]) == [0, 1, 2] for s in st.steps), "all rewards equal: the lowest indices, the injected rows"
    for prev, d in zip(st.steps[:-1], out["details"][1:]):
        Y = np.asarray(d["Y0s"], f32).reshape(len(d["rews"]), -1)
        same_bits(Y[1:1 + len(prev["E"])], prev["E"], "the previous step's elites are candidates 1..")
        same_bits(np.asarray(d["rews"], f32)[1:1 + len(prev["R"])], prev["R"], "... and their returns are re-evaluated exactly")
    assert sum(k for _, k, _ in st.log) > 0, "elites stay among the best"


@pytest.mark.parametrize("name,method", [("hopper", 0), ("car2d", 0), ("car2d", 1)])
def test_the_nominal_alone_makes_candidate_0_the_means_return(orc, name, method):
    """nominal = 1, n_elites = 0: candidate 0's reward is the return of clip(Ybar_i), and no other row changes."""
    from oracle import planner as op
    s0 = inputs.ac_cases.CAR2D_S0 if name == "car2d" else None
    oenv, s0, st, out = _run(orc, name, method, ec.Record(0, True, False), s0=s0)
    N, H, Nu = inputs.SIZES[name]
    ybar = np.zeros((H, Nu), f32)
    for d, mu in zip(out["details"], out["mu_0ts"]):
        want = op.mean_h(orc, np.ascontiguousarray(oenv.rollout(s0, ec.clip(ybar)[None])))
        same_bits(np.asarray(d["rews"], f32)[:1], want, f"{name}: candidate 0's reward")
        same_bits(np.asarray(d["Y0s"], f32)[0], ec.clip(ybar), f"{name}: candidate 0")
        ybar = mu
    assert [(c, k) for c, k, _ in st.log] == [(0, 0)] * (inputs.ND - 1)
    assert all(np.asarray(t, f32).view(np.uint32) == 0x7fc00000 for _, _, t in st.log)


@pytest.mark.parametrize("name", ["hopper", "car2d"])
def test_rows_from_slots_on_are_the_rows_without_a_record(orc, name):
    """One step from the same key and mean with and without the injection: the rows from ``slots`` on keep every bit."""
    oenv, _ = inputs.cpu_env(orc, name)
    N, H, Nu = inputs.SIZES[name]
    st = ec.State(ec.Record(3, True, False), H, Nu, inputs.lazy_of(name, 0))
    st.E = ec.clip(np.random.default_rng(3).standard_normal((3, H * Nu)) * 0.5)
    ybar = (np.random.default_rng(4).standard_normal((H, Nu)) * 0.2).astype(f32)
    key = orc.prng_key(9)
    Y0, z0 = orc.sample(key, 1, N, H, Nu, 0, N, 0.5, ybar, want_eps=True)
    Y1, z1 = ec.ElitesOracle(orc, st).sample(key, 1, N, H, Nu, 0, N, 0.5, ybar, want_eps=True)
    assert st.slots == 4
    same_bits(Y1[4:], Y0[4:], f"{name}: candidates from slots on")
    same_bits(z1[4:], z0[4:], f"{name}: normals from slots on")
    assert not np.array_equal(Y1[:4], Y0[:4])
    if inputs.lazy_of(name, 0):
        same_bits(Y1[:4].reshape(4, -1), ec.values(z1[:4].reshape(4, -1), 0.5, ybar.reshape(-1)), "a lazy elite is its z's value")
        assert np.abs(Y1[1:4].reshape(3, -1) - st.E).max() < 1e-6
    else:
        same_bits(Y1[1:4].reshape(3, -1), st.E, "a materialised elite is E[j]")


def test_the_checker_composes_with_weighting_and_adapt_records(orc):
    """ec.run under a weighting record with an ESS target and beside an adapt record: every step selects, the adapt table moves, and
    a frozen element's z stays +0 in every injected row."""
    import adapt_checker as ac
    oenv, s0 = inputs.cpu_env(orc, "hopper")
    N, H, Nu = inputs.SIZES["hopper"]
    g = inputs.ac_cases.plan_shape(H, Nu)
    adapt = ac.State(inputs.ac_cases.RULE, H, Nu, g, g)
    st = ec.State(ec.Record(3, True, False), H, Nu, True)
    zs = []

    inject = st.inject

    def spy(Y0s, z, ybar, sigma):
        out = inject(Y0s, z, ybar, sigma)
        zs.append(out[1][:st.slots].copy())
        return out
    st.inject = spy
    out = ec.run(orc, oenv, s0, orc.prng_key(4), N, H, inputs.ND, inputs.TEMP, st, rec=inputs.ac_cases.ESS, adapt=adapt)
    assert [c for c, _, _ in st.log] == [3] * (inputs.ND - 1) and np.isfinite(out["mu_0ts"]).all()
    assert not (adapt.a == 1).all() and len(adapt.log) == inputs.ND - 1
    frozen = int(np.flatnonzero(g.reshape(-1) == 0)[0])
    assert len(zs) == inputs.ND - 1 and zs[-1].shape[0] == 4
    for z in zs:
        assert (z[:, frozen].view(np.uint32) == 0).all(), "a frozen element's z is +0 in every injected row"


# ---- the command line ----------------------------------------------------------------------------------------------------------------
def test_the_flags_reach_the_record_and_the_report():
    from dataclasses import replace

    from mbd_hip.planners import mpc
    base = mpc.MpcArgs(env_name="hopper", not_render=True)
    assert not mpc._has_elites(base) and mpc._elites_settings(base) == {}
    a = replace(base, elites=4, elite_nominal=True, elite_carry=True)
    assert mpc._has_elites(a) and mpc._elites_of(a) == dict(n_elites=4, nominal=True, carry=True)
    assert mpc._has_elites(replace(base, elite_nominal=True))
    log = dict(log_kept=np.array([0, 1, 2, 3, 4, 1, 1, 2, 2], np.int32), log_top=np.arange(9, dtype=f32))
    assert mpc._elites_log(log, 6, 2) == dict(elites_kept=[10, 2, 4], elites_top=[4.0, 6.0, 8.0])
    with pytest.raises(ValueError, match="elite"):
        mpc._check_batch([a, a])
