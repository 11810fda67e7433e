"""The objective record without a GPU (include/mbd_hip.h mbd_objective, mbd_plan_set_objective, mbd_sweep_set_objective and the two
peek calls; mbd_hip.planners.mpc.discount_weights; DESIGN.md section 1 "N13 objective").

The four calls are exported and refuse what the record alone decides with MBD_ERR_INVALID, naming the field, before touching a
device; the ctypes record has the header's layout; the kernel's per-candidate functions, run on the host through
mbd_debug_objective_host (one text for host and device), keep the bits of the checker's restatement (tests/objective_checker.py)
— with all-ones weights the bits of the rollouts' own mean —; and the records the GPU tests use (tests/test_gpu_objective.py
imports them from here) are told apart by the checker at those tests' sizes, field by field."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import objective_checker as oc
from conftest import ROOT
from oracle import planner as op

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b, what=""):
    assert np.array_equal(bits(a), bits(b)), what


# ---- the records and sizes of the GPU tests (shared, so that what tells them apart is checked here) ---------------------------
def gpu_record(H, Nu, prev0=True, seed=0):
    """Distinct w[h], distinct q[a] with one zero, both costs non-zero; prev0 outside the clip in one actuator."""
    w = (1.0 + 0.25 * np.arange(H)[::-1]).astype(f32)
    q = (0.5 + 0.5 * np.arange(Nu)).astype(f32)
    q[Nu // 2] = 0.0
    p0 = None
    if prev0:
        p0 = (0.3 * np.cos(1.0 + np.arange(Nu))).astype(f32)
        p0[0] = 1.5
    return oc.Record(row_weight=w, effort=0.05, rate=0.2, act_weight=q, prev0=p0)


GPU_SIZES = {"hopper": (70, 7, 3), "ant": (33, 4, 8), "humanoidrun": (40, 5, 17), "car2d": (33, 6, 2)}  # env: (N, H, Nu)


def _record(_capi, H, Nu, **kw):
    """An mbd_objective of H x Nu with valid tables, and the arrays its pointers read; kw overrides fields."""
    keep = dict(w=np.ones(H, f32), q=np.ones(Nu, f32), p=np.zeros(Nu, f32))
    for k in ("w", "q", "p"):
        if k in kw:
            v = kw.pop(k)
            keep[k] = None if v is None else np.ascontiguousarray(v, f32)
    rec = _capi.Objective()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
    rec.row_weight, rec.act_weight, rec.prev0 = ptr(keep["w"]), ptr(keep["q"]), ptr(keep["p"])
    rec.effort, rec.rate, rec.rows, rec.cols = 0.5, 0.25, H, Nu
    for k, v in kw.items():
        if k == "reserved":
            rec.reserved[v[0]] = v[1]
        else:
            setattr(rec, k, v)
    return rec, keep


def test_the_calls_are_exported(lib):
    from mbd_hip import _capi
    for name in ("mbd_plan_set_objective", "mbd_sweep_set_objective", "mbd_plan_peek_objective", "mbd_sweep_peek_objective"):
        assert name in _capi.EXPORTS and hasattr(lib, name), name
    assert hasattr(lib, "mbd_debug_objective_host") and hasattr(lib, "mbd_debug_check_objective")
    text = open(os.path.join(ROOT, "include", "mbd_hip.h")).read()
    for name in ("mbd_plan_set_objective", "mbd_sweep_set_objective", "mbd_plan_peek_objective", "mbd_sweep_peek_objective",
                 "typedef struct mbd_objective"):
        assert name in text, name


def test_the_ctypes_record_has_the_headers_layout(tmp_path):
    from mbd_hip import _capi
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a C compiler is what builds the checker as well"
    fields = ("row_weight", "act_weight", "prev0", "effort", "rate", "rows", "cols", "reserved")
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mbd_hip.h"\nint main(void) { printf("%zu", sizeof(mbd_objective));\n'
                   + "".join(f'printf(" %zu", offsetof(mbd_objective, {f}));\n' for f in fields) + "return 0; }\n")
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = _capi.Objective
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in fields]


@pytest.mark.parametrize("setter", ["mbd_plan_set_objective", "mbd_sweep_set_objective"])
def test_handle_refusals_come_before_any_device_access(lib, setter):
    """On a box with no device: a NULL handle, and on a zeroed stand-in handle (Hsample = action_size = 0, no session) non-zero
    reserved, rows and cols — MBD_ERR_INVALID and the field's name.  Every record here is refused, so none reaches the device."""
    from mbd_hip import _capi
    fn = getattr(lib, setter)

    def refused(rec, field, handle):
        assert fn(handle, C.byref(rec)) == _capi.MBD_ERR_INVALID, field
        assert field in lib.mbd_last_error(), (field, lib.mbd_last_error())

    ok, keep = _record(_capi, 4, 3)
    refused(ok, b"plan" if "plan" in setter else b"sweep", None)
    stand_in = C.create_string_buffer(1 << 16)
    for r in range(5):
        refused(_record(_capi, 0, 0, reserved=(r, 7))[0], b"reserved[%d]=7" % r, stand_in)
    refused(_record(_capi, 4, 0)[0], b"rows=4", stand_in)
    refused(_record(_capi, 0, 3)[0], b"cols=3", stand_in)
    assert not any(bytes(stand_in.raw))
    for peek, args in (("mbd_plan_peek_objective", (None, None)), ("mbd_sweep_peek_objective", (0, None, None))):
        assert getattr(lib, peek)(None, *args) == _capi.MBD_ERR_INVALID
    # a handle without a record has nothing to show (the stand-in's record is all zero: none)
    assert lib.mbd_plan_peek_objective(stand_in, None, None) == _capi.MBD_ERR_STATE and b"no objective record" in lib.mbd_last_error()
    assert lib.mbd_sweep_peek_objective(stand_in, 0, None, None) == _capi.MBD_ERR_STATE and b"no objective record" in lib.mbd_last_error()
    del keep


def test_record_refusals_in_the_headers_order(lib):
    """The function both set calls run on their record (mbd_debug_check_objective), for a handle of H = 4, Nu = 3."""
    from mbd_hip import _capi
    H, Nu = 4, 3

    def code(rec):
        return _capi.debug_check_objective(rec[0], H, Nu), lib.mbd_last_error()

    def refused(rec, field):
        rc, msg = code(rec)
        assert rc == _capi.MBD_ERR_INVALID and field in msg, (field, rc, msg)

    assert code(_record(_capi, H, Nu))[0] == _capi.MBD_OK
    assert code(_record(_capi, H, Nu, w=None, q=None, p=None, effort=0.0, rate=0.0))[0] == _capi.MBD_OK
    assert lib.mbd_debug_check_objective(None, H, Nu) == _capi.MBD_ERR_INVALID
    refused(_record(_capi, H, Nu, reserved=(4, -1)), b"reserved[4]=-1")
    refused(_record(_capi, H + 1, Nu), b"rows=5")
    refused(_record(_capi, H, Nu - 1), b"cols=2")
    for bad in (-0.5, np.nan, np.inf):
        refused(_record(_capi, H, Nu, w=[1, bad, 1, 1]), b"row_weight[1]")
        refused(_record(_capi, H, Nu, q=[1, 1, bad]), b"act_weight[2]")
        refused(_record(_capi, H, Nu, effort=bad), b"effort")
        refused(_record(_capi, H, Nu, rate=bad), b"rate")
    for bad in (np.nan, -np.inf):
        refused(_record(_capi, H, Nu, p=[bad, 0, 0]), b"prev0[0]")
    assert code(_record(_capi, H, Nu, p=[-7.0, 0, 0]))[0] == _capi.MBD_OK  # (any finite value: it is clipped)
    refused(_record(_capi, H, Nu, w=np.zeros(H)), b"sum of row_weight")
    refused(_record(_capi, H, Nu, w=np.full(H, 3e38)), b"sum of row_weight")  # (finite weights, an infinite f32 sum)
    # the order: reserved before rows before the tables before the costs before prev0 before the sum
    refused(_record(_capi, H + 1, Nu, reserved=(0, 1), w=[-1, 0, 0, 0, 0]), b"reserved[0]")
    refused(_record(_capi, H + 1, Nu, w=[-1, 0, 0, 0, 0]), b"rows=5")
    refused(_record(_capi, H, Nu, w=np.zeros(H), rate=-1.0, p=[np.nan, 0, 0]), b"rate")
    refused(_record(_capi, H, Nu, w=np.zeros(H), p=[np.nan, 0, 0]), b"prev0")


# ---- the kernel's per-candidate functions, on the host --------------------------------------------------------------------------
_SIZES = [(1, 2), (7, 3), (5, 17), (50, 24)]


def _case(H, Nu, N=37, seed=0, members=1):
    rng = np.random.default_rng(100 * H + Nu + seed)
    Y = np.clip(rng.normal(size=(N, H, Nu)) * 0.7, -1, 1).astype(f32)
    rewss = (rng.normal(size=(members * N, H)) * 3).astype(f32)
    return Y, rewss


def _mean_h(orc, rewss):
    return op.mean_h(orc, np.ascontiguousarray(rewss, f32))


@pytest.mark.parametrize("with_prev", [False, True], ids=["noprev", "prev"])
@pytest.mark.parametrize("H,Nu", _SIZES, ids=[f"{h}-{n}" for h, n in _SIZES])
def test_host_entry_against_the_checker(lib, orc, H, Nu, with_prev):
    """Random rewards and candidates; values and lazy normals; one row per candidate and (an ensemble's) several."""
    from mbd_hip import _capi
    rec = gpu_record(H, Nu, prev0=with_prev)
    prev = oc.clip(rec.prev0)
    for members in (1, 3):
        Y, rewss = _case(H, Nu, members=members)
        rews = _mean_h(orc, rewss)
        want = oc.step(rewss, rews, Y, rec, prev)
        got = _capi.debug_objective_host(rewss, rews, Y, rec.row_weight, rec.act_weight, rec.effort, rec.rate, prev)
        for g, w_, what in zip(got, want, ("rews", "ret", "cost")):
            same_bits(g, w_, f"{what} H={H} Nu={Nu} M={members}")
    # lazy: the candidates formed from normals as the rollout's fetch forms them
    rng = np.random.default_rng(5)
    z, ybar, sigma = rng.normal(size=(37, H, Nu)).astype(f32), (rng.normal(size=(H, Nu)) * 0.4).astype(f32), f32(0.6)
    Y = np.clip(((z * sigma).astype(f32) + ybar[None]).astype(f32), f32(-1), f32(1))
    _, rewss = _case(H, Nu)
    rews = _mean_h(orc, rewss)
    got = _capi.debug_objective_host(rewss, rews, z, rec.row_weight, rec.act_weight, rec.effort, rec.rate, prev, lazy=(sigma, ybar))
    for g, w_ in zip(got, oc.step(rewss, rews, Y, rec, prev)):
        same_bits(g, w_, f"lazy H={H} Nu={Nu}")
    # act_weight None is ones; row_weight None copies the stored rews
    r2 = oc.Record(row_weight=None, effort=rec.effort, rate=rec.rate, prev0=rec.prev0)
    got = _capi.debug_objective_host(rewss, rews, Y, None, None, r2.effort, r2.rate, prev)
    for g, w_ in zip(got, oc.step(rewss, rews, Y, r2, prev)):
        same_bits(g, w_)
    same_bits(got[1], rews)


@pytest.mark.parametrize("H", [1, 3, 7, 50])
def test_all_ones_weights_give_the_rollouts_own_mean(lib, orc, H):
    """w = 1: acc = +0; acc = acc + (1 * r) in step order, / float(H) — the rollout kernels' own sum and division, so ret has
    mean_h's bits, including where the partial sums round (rewards of very different magnitudes) and for signed zeros."""
    from mbd_hip import _capi
    rng = np.random.default_rng(H)
    N = 64
    rewss = (rng.normal(size=(N, H)) * np.exp(rng.uniform(-12, 12, size=(N, H)))).astype(f32)
    rewss[0] = -0.0
    rewss[1, :] = f32(1) / f32(3)
    Y = np.zeros((N, H, 2), f32)
    rews = _mean_h(orc, rewss)
    out, ret, cost = _capi.debug_objective_host(rewss, np.full(N, np.nan, f32), Y, np.ones(H, f32))
    same_bits(ret, rews)
    same_bits(out, rews)
    same_bits(oc.ret(rewss, None, np.ones(H, f32)), rews)
    if H >= 7:  # (the partial sums do round: the f32 sum differs from the exactly rounded one somewhere)
        exact = (rewss.astype(np.float64).sum(axis=1) / H).astype(f32)
        assert not np.array_equal(exact, rews)
    assert not cost.any() and not np.signbit(cost).any()


def test_one_hot_weights_pick_their_row(lib, orc):
    from mbd_hip import _capi
    H, Nu = 7, 3
    Y, rewss = _case(H, Nu)
    for h0 in (0, 3, H - 1):
        w = np.zeros(H, f32)
        w[h0] = 2.0  # (a power of two: neither the product nor the division rounds)
        _, ret, _ = _capi.debug_objective_host(rewss, _mean_h(orc, rewss), Y, w)
        assert np.array_equal(ret, rewss[:, h0])
        same_bits(ret, oc.ret(rewss, None, w))
    w = np.zeros(H, f32)
    w[2] = 1.0
    _, ret, _ = _capi.debug_objective_host(rewss, _mean_h(orc, rewss), Y, w)
    assert np.array_equal(ret, rewss[:, 2])


def test_a_nan_stays_in_its_row(lib, orc):
    """A non-finite per-step reward makes its row's ret non-finite even under a zero weight (0 * NaN), and moves no other row."""
    from mbd_hip import _capi
    H, Nu = 7, 3
    rec = gpu_record(H, Nu)
    w = rec.row_weight.copy()
    w[4] = 0.0
    Y, rewss = _case(H, Nu)
    clean = _capi.debug_objective_host(rewss, _mean_h(orc, rewss), Y, w, rec.act_weight, rec.effort, rec.rate, oc.clip(rec.prev0))
    bad = rewss.copy()
    bad[5, 4], bad[9, 0] = np.nan, np.inf
    got = _capi.debug_objective_host(bad, _mean_h(orc, bad), Y, w, rec.act_weight, rec.effort, rec.rate, oc.clip(rec.prev0))
    assert np.isnan(got[1][5]) and np.isnan(got[0][5]) and not np.isfinite(got[1][9]) and not np.isfinite(got[0][9])
    keep = np.ones(len(rewss), bool)
    keep[[5, 9]] = False
    for g, c in zip(got[:2], clean[:2]):
        same_bits(g[keep], c[keep])
    same_bits(got[2], clean[2])
    want = oc.step(bad, _mean_h(orc, bad), Y, oc.Record(w, rec.effort, rec.rate, rec.act_weight, rec.prev0), oc.clip(rec.prev0))
    for g, w_ in zip(got, want):
        same_bits(g, w_)
    # a diverged candidate (NaN actions cannot happen: the clip; but a NaN normal) poisons its own cost only
    z = Y.copy()
    z[3, 2, 1] = np.nan
    got = _capi.debug_objective_host(rewss, _mean_h(orc, rewss), z, w, rec.act_weight, rec.effort, rec.rate, None)
    base = _capi.debug_objective_host(rewss, _mean_h(orc, rewss), Y, w, rec.act_weight, rec.effort, rec.rate, None)
    assert np.isnan(got[2][3]) and np.isnan(got[0][3])
    keep = np.arange(len(Y)) != 3
    same_bits(got[0][keep], base[0][keep])
    same_bits(got[2][keep], base[2][keep])


def test_zero_costs_skip_the_cost_pass(lib, orc):
    from mbd_hip import _capi
    H, Nu = 5, 17
    Y, rewss = _case(H, Nu)
    rews = _mean_h(orc, rewss)
    rews[3] = -0.0
    for w in (None, gpu_record(H, Nu).row_weight):
        out, ret, cost = _capi.debug_objective_host(rewss, rews, Y, w, gpu_record(H, Nu).act_weight, 0.0, 0.0, np.ones(Nu, f32))
        same_bits(cost, np.zeros(len(Y), f32))  # all +0
        same_bits(out, ret)
        same_bits(ret, oc.ret(rewss, rews, w))
    out, ret, _ = _capi.debug_objective_host(rewss, rews, Y)
    same_bits(out, rews)  # the NULL / zero record: the stored rewards, -0.0 included


def test_the_previous_action_enters_the_first_difference_only(lib, orc):
    from mbd_hip import _capi
    H, Nu = 4, 3
    Y, rewss = _case(H, Nu, N=5)
    rews = _mean_h(orc, rewss)
    none = oc.cost(Y, None, 0.0, 1.0, None)
    prev = np.array([0.25, -1.0, 1.0], f32)
    with_ = oc.cost(Y, None, 0.0, 1.0, prev)
    d0 = ((Y[:, 0, :].astype(np.float64) - prev) ** 2).sum(axis=1) / H
    assert np.allclose(with_.astype(np.float64) - none, d0, rtol=1e-5, atol=1e-6) and (with_ > none).all()
    same_bits(_capi.debug_objective_host(rewss, rews, Y, None, None, 0.0, 1.0, prev)[2], with_)
    # H = 1: without a previous action the rate cost has no term at all
    Y1 = Y[:, :1]
    out, ret, cost = _capi.debug_objective_host(rewss[:, :1], rews, Y1, None, None, 0.0, 1.0, None)
    same_bits(cost, np.zeros(5, f32))
    assert np.array_equal(oc.clip([1.5, -3.0, 0.5]), np.array([1.0, -1.0, 0.5], f32)) and oc.clip(None) is None


def test_discount_weights():
    from mbd_hip.planners.mpc import action_rate, discount_weights
    for H, g, term in ((50, 0.98, 1.0), (7, 0.5, 4.0), (1, 0.9, 3.0), (6, 1.0, 1.0), (5, 0.0, 2.0)):
        w = discount_weights(H, g, term)
        want = np.array([g ** h for h in range(H)], np.float64)
        want[-1] *= term
        assert w.dtype == np.float32 and w.shape == (H,) and w.flags["C_CONTIGUOUS"]
        assert np.array_equal(w, want.astype(np.float32)), (H, g, term)
    assert np.array_equal(discount_weights(6, 1.0), np.ones(6, np.float32))
    assert discount_weights(5, 0.0)[0] == 1 and not discount_weights(5, 0.0)[1:].any()  # (0 ** 0 = 1)
    for bad in (dict(H=0, gamma=0.9), dict(H=4, gamma=-0.1), dict(H=4, gamma=np.nan), dict(H=4, gamma=0.9, terminal=-1.0)):
        with pytest.raises(ValueError):
            discount_weights(**bad)
    a = np.array([[0.0, 1.0], [1.0, 1.0], [1.0, -1.0]])
    assert action_rate(a) == pytest.approx((1 + 0 + 0 + 4) / 4) and action_rate(a[:1]) == 0.0


def test_arguments():
    from dataclasses import replace

    from mbd_hip.planners import mpc
    a = mpc.MpcArgs(env_name="hopper", Nsample=16, Hsample=6, Ndiffuse=6, disable_recommended_params=True, not_render=True)
    assert not mpc._has_objective(a) and mpc._objective_settings(a) == {}
    b = replace(a, rate_cost=0.25)
    kw = mpc._objective_of(b)
    assert mpc._has_objective(b) and kw["row_weight"] is None and (kw["effort"], kw["rate"], kw["act_weight"]) == (0.0, 0.25, None)
    c = replace(a, discount=0.9, terminal_weight=3.0, effort_cost=0.5)
    kw = mpc._objective_of(c)
    assert np.array_equal(kw["row_weight"], mpc.discount_weights(6, 0.9, 3.0)) and kw["effort"] == 0.5 and kw["rate"] == 0.0
    assert mpc._objective_settings(c) == dict(discount=0.9, terminal_weight=3.0, effort_cost=0.5, rate_cost=0.0, act_weight="")
    mpc._check_batch([b, replace(b, seed=1)])
    with pytest.raises(ValueError, match="rate_cost"):
        mpc._check_batch([b, replace(a, seed=1)])


# ---- the records of the GPU tests are told apart ----------------------------------------------------------------------------------
@pytest.mark.parametrize("env", sorted(GPU_SIZES))
def test_the_gpu_cases_tell_their_records_apart(orc, env):
    """At the sizes of tests/test_gpu_objective.py, two records that differ in ONE field give different checker outputs for every
    field — so a kernel that ignored a field, read w or q at the wrong index, or dropped prev could not pass there."""
    N, H, Nu = GPU_SIZES[env]
    Y, rewss = _case(H, Nu, N=N, seed=1)
    rews = _mean_h(orc, rewss)
    base = gpu_record(H, Nu)
    out0 = oc.step(rewss, rews, Y, base, oc.clip(base.prev0))[0]

    def differs(**kw):
        r = oc.Record(**dict(base.kwargs(), **kw))
        out = oc.step(rewss, rews, Y, r, oc.clip(r.prev0))[0]
        return (bits(out) != bits(out0)).mean()

    assert differs(row_weight=None) > 0.9 and differs(act_weight=None) > 0.9
    assert differs(effort=0.0) > 0.9 and differs(rate=0.0) > 0.9 and differs(prev0=None) > 0.9
    for h in range(H):  # every row weight and (below) every actuator weight matters, each on its own
        w = base.row_weight.copy()
        w[h] += 0.5
        assert differs(row_weight=w) > 0.9, h
        if H > 1:  # two weights swapped
            w = base.row_weight.copy()
            w[h], w[(h + 1) % H] = w[(h + 1) % H], w[h]
            assert differs(row_weight=w) > 0.9, h
    for a in range(Nu):
        q = base.act_weight.copy()
        q[a] += 0.5
        assert differs(act_weight=q) > 0.9, a
        p = base.prev0.copy()
        p[a] = -p[a] if a else 0.5
        assert (differs(prev0=p) == 0.0) if base.act_weight[a] == 0 else (differs(prev0=p) > 0.9), a  # (a zero weight hides its actuator)
    assert differs() == 0.0
    # the clip of prev0 matters: the unclipped value gives other costs
    unclipped = oc.step(rewss, rews, Y, base, np.asarray(base.prev0, f32))[0]
    assert (bits(unclipped) != bits(out0)).mean() > 0.9


def test_checker_demo_episode_with_a_zero_record_is_the_demo_checkers(orc_omp):
    """tests/objective_checker.demo_episode — sessions ticked one by one, the tick's window and the shared previous action set in
    between — under a record of no weights and zero costs is tests/mpc_demo_checker.episode, log for log; under the GPU test's
    record it is not, and every tick's previous action is the clipped last committed row."""
    import mpc_demo_checker as mdc
    orc = orc_omp
    oenv = mdc.oracle_env(orc, "humanoidtrack")
    clip = mdc.extended(oenv.xref)
    s0 = np.asarray(oenv.reset(orc.prng_key(5), 1), f32).reshape(-1)
    args = (clip, 2, 1.0, s0, orc.prng_key(6), 33, 50, 4, 0.1, 3, 2, 2)
    ref = mdc.episode(oenv, *args)
    zero = oc.demo_episode(oenv, oc.Record(), *args)
    for k in ("means", "actions", "rewards", "states"):
        assert np.array_equal(zero[k], ref[k]), k
    rec = gpu_record(50, oenv.Nu)
    shaped = oc.demo_episode(oenv, rec, *args)
    assert np.isfinite(shaped["means"]).all() and not np.array_equal(shaped["means"], ref["means"])
    assert not np.array_equal(oc.demo_episode(oenv, oc.Record(**dict(rec.kwargs(), prev0=None)), *args)["means"][0], shaped["means"][0])
