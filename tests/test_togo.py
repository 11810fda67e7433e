"""The to-go record without a device (include/mbd_hip.h mbd_togo, DESIGN.md section 1 "N19 to-go").

The calls are exported and declared; the ctypes record has the header's layout; the group layout at its edges; the host entry
(mbd_debug_togo_host: the functions the returns kernel calls, looped on the CPU) keeps the checker's bits, NaN and inf placement
included; the checker with one group is the oracle's update on the rewards, and group 0's rows are always the rows without a record;
what the record alone decides is refused before any device access, each message naming its field — through mbd_debug_check_togo and,
where a zeroed stand-in handle reaches them, through the set and peek calls themselves; the flags reach the record and sweeps refuse
it.  (The refusals that need a configured plan — another record on the handle, a shard, an open session, whose flag lies at an offset
only the library knows — are in tests/test_gpu_togo.py.)"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import togo_checker as tc
import togo_inputs as inputs
from conftest import ROOT
from state_inputs import same_bits

f32 = np.float32


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_the_calls_are_exported_and_declared(lib):
    from mbd_hip import _capi
    for name in ("mbd_plan_set_togo", "mbd_plan_peek_togo"):
        assert name in _capi.EXPORTS and hasattr(lib, name), name
    for name in ("mbd_debug_togo_host", "mbd_debug_togo_step", "mbd_debug_check_togo"):
        assert hasattr(lib, name), name
    text = open(os.path.join(ROOT, "include", "mbd_hip.h")).read()
    for name in ("typedef struct mbd_togo", "int mbd_plan_set_togo(", "int mbd_plan_peek_togo(", "R_j[n] = acc / float(H - s_j)",
                 "G = 1 is no record, bit for bit"):
        assert name in text, name
    dbg = open(os.path.join(ROOT, "include", "mbd_hip_debug.h")).read()
    for name in ("mbd_debug_togo_host", "mbd_debug_togo_step", "mbd_debug_check_togo"):
        assert name in dbg, name


def test_the_ctypes_record_has_the_headers_layout(tmp_path):
    from mbd_hip import _capi
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a C compiler is what builds the checker as well"
    fields = ("block", "min_tail", "reserved")
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mbd_hip.h"\nint main(void) { printf("%zu", sizeof(mbd_togo));\n'
                   + "".join(f'printf(" %zu", offsetof(mbd_togo, {f}));\n' for f in fields) + "return 0; }\n")
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = _capi.Togo
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in fields] and C.sizeof(S) == 16


def test_refusals_come_before_any_device_access(lib):
    """A NULL handle; through mbd_debug_check_togo every refusal the record alone decides, in the header's order, each naming its
    field; good records accepted."""
    from mbd_hip import _capi
    rec = _capi.togo_record(1, 1)
    assert lib.mbd_plan_set_togo(None, C.byref(rec)) == _capi.MBD_ERR_INVALID
    assert lib.mbd_plan_peek_togo(None, None, None, None, None) == _capi.MBD_ERR_INVALID
    assert _capi.debug_check_togo(None, 8, 64) == _capi.MBD_ERR_INVALID

    def refused(code, word, H=8, N=64, method=0, demo=False, **fields):
        r = _capi.togo_record(2, 1)
        for k, v in fields.items():
            if k.startswith("reserved"):
                r.reserved[int(k[8:])] = v
            else:
                setattr(r, k, v)
        assert _capi.debug_check_togo(r, H, N, method, demo) == code, (fields, H, N, method, demo)
        assert word.encode() in lib.mbd_last_error(), (word, lib.mbd_last_error())

    I, U = _capi.MBD_ERR_INVALID, _capi.MBD_ERR_UNSUPPORTED
    # a zeroed stand-in handle (Hsample 0, unsharded, no session, no record): the set call itself refuses in the same words, a NULL
    # record has nothing to clear, peek has no record to show, and nothing is written to the handle
    stand_in = C.create_string_buffer(1 << 16)
    for r, word in ((_capi.togo_record(0, 1), b"block=0"), (_capi.togo_record(2, 1), b"min_tail=1 outside [1, Hsample=0]"),
                    (_capi.togo_record(2, 0), b"min_tail=0")):
        assert lib.mbd_plan_set_togo(stand_in, C.byref(r)) == I and word in lib.mbd_last_error(), (word, lib.mbd_last_error())
    assert lib.mbd_plan_set_togo(stand_in, None) == _capi.MBD_OK  # (nothing to clear)
    assert lib.mbd_plan_peek_togo(stand_in, None, None, None, None) == _capi.MBD_ERR_STATE and b"no to-go record" in lib.mbd_last_error()
    assert not any(bytes(stand_in.raw))
    refused(I, "block=0", block=0)
    refused(I, "block=-3", block=-3)
    refused(I, "min_tail=0", min_tail=0)
    refused(I, "min_tail=9", min_tail=9)
    refused(I, "Hsample=8", min_tail=9)
    for k in range(2):
        refused(I, f"reserved[{k}]", **{f"reserved{k}": 1})
    refused(U, "update_method=2", method=2)
    refused(U, "update_method=3", method=3)
    refused(U, "enable_demo", demo=True)
    refused(U, "Nsample=12289", N=12289)
    refused(I, "block=0", block=0, method=3)  # (the record's own fields come first)
    for b, m, H, N, method in ((1, 1, 1, 2, 0), (1, 8, 8, 12288, 1), (100, 1, 8, 64, 0), (3, 5, 8, 64, 1)):
        assert _capi.debug_check_togo(_capi.togo_record(b, m), H, N, method) == _capi.MBD_OK, (b, m, H, N, method)


# ---- the layout ----------------------------------------------------------------------------------------------------------------------
def test_the_group_layout_at_the_edges(lib):
    """block >= H and min_tail = H give one group; a start whose tail is min_tail exactly is a start, one row further is none; H = 1
    has one group; the host entry's layout is the checker's at every (H, block, min_tail) up to H = 12."""
    from mbd_hip import _capi
    assert tc.groups(8, 8, 1).tolist() == [0] and tc.groups(8, 50, 1).tolist() == [0]
    assert tc.groups(8, 1, 8).tolist() == [0] and tc.groups(8, 3, 8).tolist() == [0]
    assert tc.groups(8, 2, 4).tolist() == [0, 2, 4]       # H - 4 = 4 = min_tail exactly: a start; H - 6 = 2: none
    assert tc.groups(8, 2, 5).tolist() == [0, 2]
    assert tc.groups(7, 3, 1).tolist() == [0, 3, 6] and tc.groups(7, 3, 2).tolist() == [0, 3]
    assert tc.groups(1, 1, 1).tolist() == [0]
    assert tc.groups(50, 10, 10).tolist() == [0, 10, 20, 30, 40] and tc.groups(50, 10, 11).tolist() == [0, 10, 20, 30]
    for H in range(1, 13):
        for block in range(1, H + 3):
            for min_tail in range(1, H + 1):
                assert _capi.debug_togo_layout(H, block, min_tail).tolist() == tc.groups(H, block, min_tail).tolist(), (H, block, min_tail)
    for bad in ((4, 0, 1), (4, 1, 0), (4, 1, 5)):
        with pytest.raises(_capi.MbdError) as e:
            _capi.debug_togo_layout(*bad)
        assert e.value.code == _capi.MBD_ERR_INVALID and ("block" in str(e.value) or "min_tail" in str(e.value))


# ---- the host entry against the checker -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [1, 2, 7, 16, 17, 33, 50])
def test_the_host_entry_keeps_the_checkers_bits(lib, H):
    """mbd_debug_togo_host against ``returns`` by bit pattern for every reward shape and layout: around the sixteen loads the chain
    keeps in flight (H = 16, 17, 33), with a NaN reaching exactly the groups with s_j <= t and +inf in step 0 reaching none."""
    from mbd_hip import _capi
    N = 37
    for lay in inputs.LAYOUTS + ((5, 10), (16, 1)):
        block, min_tail = inputs.layout(H, lay)
        starts = tc.groups(H, block, min_tail)
        for kind in inputs.KINDS:
            rews, rewss, t = inputs.rewards(kind, N, H, 9)
            got = _capi.debug_togo_host(rews, rewss, block, min_tail)
            ref = tc.returns(rews, rewss, starts)
            what = f"H={H} block={block} min_tail={min_tail} {kind}"
            assert got["starts"].tolist() == starts.tolist(), what
            same_bits(got["R"], ref, what)  # (sums and quotients of the same operands: a NaN's bits agree as well)
            same_bits(got["R"][0], rews, f"{what}: R_0 is rews")
            if kind in ("nan_step_t", "nan_from_t"):
                for j, s in enumerate(starts[1:], 1):
                    hit = np.isnan(got["R"][j])
                    if kind == "nan_from_t" or s <= t:
                        assert hit.sum() == 1 and hit[N // 2], f"{what}: the NaN candidate alone (group {j})"
                    else:
                        assert not hit.any(), f"{what}: group {j} starts behind step {t} and stays finite"
                assert np.isnan(rews[N // 2]) and np.isfinite(np.delete(rews, N // 2)).all()
            if kind == "inf_step0":
                assert np.isfinite(got["R"][1:]).all() and np.isinf(got["R"][0][N - 1]), f"{what}: +inf in step 0 reaches group 0 only"


def test_a_nan_in_a_late_step_leaves_the_later_groups_finite():
    """One candidate NaN in step t only: the groups with s_j <= t have it, the groups with s_j > t do not."""
    H, N, t = 12, 9, 7
    rews, rewss, _ = inputs.rewards("random", N, H, 2)
    rewss[4, t] = np.nan
    starts = tc.groups(H, 2, 1)
    R = tc.returns(rews, rewss, starts)
    for j, s in enumerate(starts[1:], 1):
        assert bool(np.isnan(R[j][4])) == (s <= t), (j, s)
        assert np.isfinite(np.delete(R[j], 4)).all()


# ---- the checker -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1])
def test_one_group_is_the_oracles_update_and_group_0_never_moves(orc, method):
    """G = 1 (block = H, and min_tail = H): the checker's step is ``orc.score_update`` / ``orc.pi_update`` on rews, bit for bit.
    With more groups the rows of group 0 are still that call's rows, the later rows differ, and the weights returned are group 0's."""
    N, H, Nu = 65, 7, 3
    c = inputs.step_case(N, H, Nu, (1, 1), "random", (False, (method, True)))
    if method == 0:
        out, w, m = orc.score_update(c["rews"], c["cand"], c["ybar"], *inputs.ALPHAS, inputs.TEMP, literal=True)
    else:
        out, _, w, m = orc.pi_update(1, c["rews"], c["cand"], c["ybar"], inputs.SIGMA, inputs.TEMP)
    for block, min_tail in ((H, 1), (1, H), (50, 1)):
        res = tc.update(orc, method, c["rews"], c["rewss"], c["cand"], c["ybar"], tc.groups(H, block, min_tail), inputs.TEMP,
                        alphas=inputs.ALPHAS, sigma=inputs.SIGMA)
        same_bits(res["out"], out, f"block={block} min_tail={min_tail}: the mean")
        same_bits(res["W"], w, "the weights")
        same_bits(res["rew_mean"], m, "the mean reward")
    for block in (1, 3):
        starts = tc.groups(H, block, 1)
        res = tc.update(orc, method, c["rews"], c["rewss"], c["cand"], c["ybar"], starts, inputs.TEMP, alphas=inputs.ALPHAS,
                        sigma=inputs.SIGMA)
        same_bits(res["out"][:starts[1]], out[:starts[1]], f"block={block}: group 0's rows")
        same_bits(res["W"][0], w, "group 0's weights")
        same_bits(res["rew_mean"], m, "the mean reward")
        assert not np.array_equal(res["out"][starts[1]:], out[starts[1]:]), "the later rows are weighed by what is still ahead"
        assert all(not np.array_equal(res["W"][j], w) for j in range(1, len(starts)))


def test_the_table_reaches_what_it_is_for(orc):
    """Every mode meets every reward shape somewhere in the table; Nu = 17 and 24 put tile starts off multiples of 16 and leave a
    group's last tile partial; zero spread is guarded for MBD and NaN for mppi, in the one group it concerns."""
    seen = set()
    for N in inputs.NS:
        for H, Nu in inputs.SHAPES:
            for c in inputs.step_cases(N, H, Nu):
                seen.add(((c["lazy"], c["method"], c["literal"]), c["kind"]))
    assert len(seen) == len(inputs.MODES) * len(inputs.KINDS)
    assert any((s * Nu) % 16 for H, Nu in inputs.SHAPES for s in tc.groups(H, 1, 1)[1:])
    assert any((Nu * 1) % 16 for _, Nu in inputs.SHAPES)
    for method in (0, 1):
        c = inputs.step_case(63, 7, 17, (1, 1), "late_tie", (False, (method, False)))
        res = inputs.checked_step(orc, c)
        last = np.isnan(res["out"][-1]).all()
        assert last == (method == 1) and np.isfinite(res["out"][:-1]).all(), method
        if method == 0:
            assert np.all(res["W"][-1] == res["W"][-1][0]), "the guard: equal weights in the tied group"


def test_whole_plans_differ_from_plans_without_a_record(orc):
    """hopper, N = 64, H = 8, three steps: with block 3 the first step's rows of group 0 are the plan's without a record, its later
    rows are not, and from the second step on every row differs (the candidates are drawn around another mean)."""
    import adapt_cases
    from oracle import planner as op
    oenv, s0 = adapt_cases.cpu_env(orc, "hopper")
    key = orc.prng_key(4)
    ref = tc.run(oenv, s0, key, 64, 8, 4, 0.1, 3)
    sched = orc.schedule(1e-4, 1e-2, 4)
    r, Ybar, plain = np.asarray(key, np.uint32), np.zeros((8, oenv.Nu), f32), []
    for i in range(3, 0, -1):
        r, Ybar, _, _ = op.reverse_once(orc, oenv, s0, i, r, Ybar, sched, 64, 8, 0.1, 1)
        plain.append(Ybar)
    same_bits(ref["mu_0ts"][0][:3], plain[0][:3], "step 1: group 0's rows")
    assert not np.array_equal(ref["mu_0ts"][0][3:], plain[0][3:])
    assert not np.array_equal(ref["mu_0ts"][2][:3], plain[2][:3])
    assert len(ref["steps"]) == 3 and ref["steps"][0]["R"].shape == (3, 64)
    one = tc.run(oenv, s0, key, 64, 8, 4, 0.1, 8)
    same_bits(one["mu_0ts"], np.stack(plain), "G = 1 is no record")


# ---- the command line ----------------------------------------------------------------------------------------------------------------
def test_the_flags_reach_the_record_and_sweeps_refuse_it():
    from dataclasses import replace

    from mbd_hip.planners import mpc
    base = mpc.MpcArgs(env_name="hopper", not_render=True)
    assert not mpc._has_togo(base) and mpc._togo_settings(base) == {}
    assert not mpc._has_togo(replace(base, togo_min_tail=5)), "there is no record unless togo_block is given"
    a = replace(base, togo_block=5, togo_min_tail=10)
    assert mpc._has_togo(a) and mpc._togo_of(a) == dict(block=5, min_tail=10)
    assert mpc._togo_settings(a) == dict(togo_block=5, togo_min_tail=10)
    with pytest.raises(ValueError, match="togo_block"):
        mpc._check_batch([a, a])
    mpc._check_togo(base)
    mpc._check_togo(a)
    for other in (dict(adapt_rate=0.3), dict(ess_frac=0.5), dict(reject_nonfinite=True), dict(value="net.npz"), dict(effort_cost=0.1),
                  dict(ens_mass="1.0,1.3")):
        with pytest.raises(ValueError, match="togo_block"):
            mpc._check_togo(replace(a, **other))
