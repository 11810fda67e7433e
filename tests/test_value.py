"""The value record (include/mbd_hip.h mbd_value; DESIGN.md section 1 "N16 value") without a GPU: the host form of the kernel's
arithmetic against the checker's restatement (tests/value_checker.py) bit for bit, the import convention against torch, what the
inputs of tests/value_inputs.py reach, every refusal, and ``mbd_hip.scripts.fit_value``."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import value_checker as vc
import value_inputs as vi
from conftest import ROOT
from state_inputs import same_bits

CASES = [(e, s, a, r) for e in vi.ENVS for s in vi.SHAPES for a in ("relu", "tanh") for r in ((False, True) if e != "car2d" else (False,))]


def test_the_boundary_is_declared_and_exported(lib):
    from mbd_hip import _capi
    for name in ("mbd_plan_set_value", "mbd_plan_peek_value", "mbd_plan_eval_value", "mbd_sweep_set_value"):
        assert name in _capi.EXPORTS and hasattr(lib, name), name
    assert hasattr(lib, "mbd_debug_value_host") and hasattr(lib, "mbd_debug_check_value")
    text = open(os.path.join(ROOT, "include", "mbd_hip.h")).read()
    assert "typedef struct mbd_value" in text and "#define MBD_VALUE_MAX_WIDTH 256" in text and "#define MBD_VALUE_MAX_LAYERS 4" in text
    assert (_capi.VALUE_MAX_LAYERS, _capi.VALUE_MAX_WIDTH, _capi.VALUE_RELU, _capi.VALUE_TANH, _capi.VALUE_REL_XY) == (4, 256, 0, 1, 1)
    rec = vi.net("car2d", "S-1").value_net().record()
    out = np.zeros(1, np.float32)
    assert lib.mbd_plan_set_value(None, C.byref(rec)) == _capi.MBD_ERR_INVALID and b"plan" in lib.mbd_last_error()
    assert lib.mbd_sweep_set_value(None, C.byref(rec)) == _capi.MBD_ERR_INVALID and b"sweep" in lib.mbd_last_error()
    assert lib.mbd_plan_peek_value(None, _capi.np_ptr(out)) == _capi.MBD_ERR_INVALID
    assert lib.mbd_plan_eval_value(None, _capi.np_ptr(out), 1, _capi.np_ptr(out)) == _capi.MBD_ERR_INVALID


def test_the_ctypes_record_has_the_headers_layout(tmp_path):
    from mbd_hip import _capi
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a C compiler is what builds the checker as well"
    fields = ("W", "b", "center", "in_scale", "n_in", "n_layers", "width", "act", "flags", "scale", "reserved")
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mbd_hip.h"\nint main(void) { printf("%zu", sizeof(mbd_value));\n'
                   + "".join(f'printf(" %zu", offsetof(mbd_value, {f}));\n' for f in fields) + "return 0; }\n")
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = _capi.Value
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in fields]


@pytest.mark.parametrize("env,shape,act,rel", CASES, ids=[f"{e}-{s}-{a}-{'rel' if r else 'abs'}" for e, s, a, r in CASES])
def test_host_form_is_the_checker_and_the_inputs_reach(lib, orc, env, shape, act, rel):
    """mbd_debug_value_host — the functions value_kernel calls — against the checker over every row of value_inputs, bit for bit,
    V and rews + scale * V; and what those inputs reach: in every hidden layer between 20 % and 80 % of the finite pre-activations
    are positive, tanh nets meet arguments beyond 44, masked inputs, -0, NaN and both infinities are among the rows."""
    from mbd_hip import _capi
    net, states = vi.net(env, shape, act, rel), vi.states(env)
    rews = (np.random.default_rng(1).normal(size=len(states))).astype(np.float32)
    rews[5] = np.float32(-0.0)
    V, pre = vc.value(orc, net, states, want_pre=True)
    got_v, got_r = _capi.debug_value_host(net.value_net().record(), states, rews, rigid_body=env != "car2d")
    same_bits(vc.canon(got_v), vc.canon(V), "V")
    same_bits(vc.canon(got_r), vc.canon(vc.add(rews, net.scale, V)), "rews + scale * V")
    healthy = np.isfinite(states).all(axis=1)
    assert np.isfinite(V[healthy]).all() and not np.isfinite(V[~healthy]).all() and (~healthy).sum() >= 5
    for l, a in enumerate(pre):
        frac = float((a[healthy] > 0).mean())
        assert 0.2 <= frac <= 0.8, f"layer {l + 1}: {frac:.2f} of the pre-activations are positive"
    if pre and act == "tanh":
        assert np.abs(pre[0][healthy]).max() > 44
    assert (np.asarray(net.in_scale) == 0).any()
    s = states.reshape(-1)
    assert np.isnan(s).any() and np.isposinf(s).any() and np.isneginf(s).any() and ((s == 0) & np.signbit(s)).any()
    assert any(((b == 0) & np.signbit(b)).any() for b in net.b) or shape in ("S-1", "S-1-1")


@pytest.mark.parametrize("env,shape,act", [("humanoidrun", "S-65-64-1", "relu"), ("humanoidrun", "S-65-64-1", "tanh"),
                                           ("hopper", "S-3-1", "tanh"), ("car2d", "S-1", "relu")])
def test_import_convention_is_torchs(orc, env, shape, act):
    """The checker on a net imported by ValueNet.from_torch agrees with the float32 torch.nn.Sequential itself within rtol 1e-4,
    atol 1e-5 (a condition: a transposed or mis-ordered import is wrong by O(1), rounding differs by about 1e-6)."""
    import torch
    import torch.nn as nn
    from mbd_hip.planners.value import ValueNet
    src = vi.net(env, shape, act)
    layers = []
    for l, (w, b) in enumerate(zip(src.W, src.b)):
        lin = nn.Linear(w.shape[1], w.shape[0])
        with torch.no_grad():
            lin.weight.copy_(torch.tensor(w))
            lin.bias.copy_(torch.tensor(b))
        layers.append(lin)
        if l + 1 < len(src.W):
            layers.append(nn.ReLU() if act == "relu" else nn.Tanh())
    seq = nn.Sequential(*layers)
    vn = ValueNet.from_torch(seq, center=src.center, in_scale=src.in_scale)
    assert vn.widths == [w.shape[0] for w in src.W] and vn.act == act and vn.n_in == src.W[0].shape[1]
    x = vi.healthy_states(env)
    net = vc.Net(vn.W, vn.b, vn.act, vn.center, vn.in_scale)
    with torch.no_grad():
        want = seq(torch.tensor(vc.inputs(net, x))).reshape(-1).numpy()
    np.testing.assert_allclose(vc.value(orc, net, x), want, rtol=1e-4, atol=1e-5)
    for bad in (nn.Sequential(nn.Linear(3, 2), nn.Linear(2, 1)), nn.Sequential(nn.Linear(3, 1), nn.ReLU()),
                nn.Sequential(nn.Linear(3, 2), nn.ReLU(), nn.Linear(2, 2), nn.Tanh(), nn.Linear(2, 1)),
                nn.Sequential(nn.Linear(3, 2), nn.Sigmoid(), nn.Linear(2, 1))):
        with pytest.raises(ValueError):
            ValueNet.from_torch(bad)


def test_save_and_load_keep_every_field(tmp_path):
    from mbd_hip.planners.value import ValueNet, terminal_scale
    vn = vi.net("hopper", "S-65-64-1", "tanh", True, scale=0.25).value_net()
    vn.save(tmp_path / "v.npz")
    back = ValueNet.load(tmp_path / "v.npz")
    assert (back.act, back.rel_xy, back.scale, back.widths, back.n_in) == ("tanh", True, 0.25, [65, 64, 1], vn.n_in)
    for a, b in zip(vn.W + vn.b + [vn.center, vn.in_scale], back.W + back.b + [back.center, back.in_scale]):
        same_bits(a, b, "a saved array")
    assert terminal_scale(2.0, 50) == pytest.approx(0.04)


def test_refusals_need_no_device(lib):
    """Every refusal of the record, by mbd_debug_check_value (the function both set calls run): the code and the field's name."""
    from mbd_hip import _capi
    S = vi.state_size("hopper")

    def check(mutate, code, field, state_size=S, rigid=True, shape="S-3-1"):
        net = vi.net("hopper" if state_size == S else "car2d", shape)
        vn = net.value_net()
        rec = vn.record()
        keep = mutate(rec, vn)
        assert _capi.debug_check_value(rec, state_size, rigid) == code, field
        assert field.encode() in lib.mbd_last_error(), (field, lib.mbd_last_error())
        del keep

    ok = vi.net("hopper", "S-3-1").value_net()
    assert _capi.debug_check_value(ok.record(), S, True) == _capi.MBD_OK
    lib.mbd_debug_check_value.argtypes = [C.c_void_p, C.c_int, C.c_int]
    assert lib.mbd_debug_check_value(None, S, 1) == _capi.MBD_ERR_INVALID and b"NULL" in lib.mbd_last_error()
    INV, UNS = _capi.MBD_ERR_INVALID, _capi.MBD_ERR_UNSUPPORTED
    check(lambda r, v: None, INV, "n_in", state_size=S + 13)
    check(lambda r, v: setattr(r, "n_layers", 0), INV, "n_layers")
    check(lambda r, v: setattr(r, "n_layers", 5), INV, "n_layers")
    check(lambda r, v: r.width.__setitem__(0, 0), INV, "width[0]")
    check(lambda r, v: r.width.__setitem__(0, 257), INV, "width[0]")
    check(lambda r, v: r.width.__setitem__(1, 2), INV, "width[1]")
    check(lambda r, v: setattr(r, "act", 2), INV, "act")
    check(lambda r, v: setattr(r, "flags", 2), INV, "flags")
    check(lambda r, v: setattr(r, "flags", 1), UNS, "REL_XY", state_size=3, rigid=False)
    check(lambda r, v: r.reserved.__setitem__(4, 1), INV, "reserved[4]")
    for bad in (np.nan, np.inf, -np.inf):
        check(lambda r, v: setattr(r, "scale", bad), INV, "scale")
        check(lambda r, v: v.W[1].__setitem__((0, 2), bad), INV, "W[1][0][2]")
        check(lambda r, v: v.W[0].__setitem__((2, 5), bad), INV, "W[0][2][5]")
        check(lambda r, v: v.b[0].__setitem__(1, bad), INV, "b[0][1]")
        check(lambda r, v: v.center.__setitem__(4, bad), INV, "center[4]")
        check(lambda r, v: v.in_scale.__setitem__(7, bad), INV, "in_scale[7]")
    null = C.POINTER(C.c_float)()
    check(lambda r, v: r.W.__setitem__(1, null), INV, "W[1]")
    check(lambda r, v: r.b.__setitem__(0, null), INV, "b[0]")
    # NULL center / in_scale are zeros / ones, not refusals
    rec = ok.record()
    rec.center, rec.in_scale = null, null
    assert _capi.debug_check_value(rec, S, True) == _capi.MBD_OK
    # the host form refuses what the set calls refuse, and its own NULL arguments
    x, out = np.zeros((1, S), np.float32), np.zeros(1, np.float32)
    lib.mbd_debug_value_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    rec = ok.record()
    for args in ((None, 1, x.ctypes.data, None, 1, out.ctypes.data, None), (C.addressof(rec), 1, None, None, 1, out.ctypes.data, None),
                 (C.addressof(rec), 1, x.ctypes.data, None, 1, None, None), (C.addressof(rec), 1, x.ctypes.data, None, 0, out.ctypes.data, None)):
        assert lib.mbd_debug_value_host(*args) == INV


def test_python_refuses_what_the_record_cannot_hold():
    from mbd_hip.planners.value import ValueNet
    with pytest.raises(ValueError, match="act"):
        ValueNet([np.zeros((1, 3))], [np.zeros(1)], act="gelu")
    with pytest.raises(ValueError, match="layer 2"):
        ValueNet([np.zeros((2, 3)), np.zeros((1, 3))], [np.zeros(2), np.zeros(1)])
    five = ValueNet([np.zeros((2, 3))] + [np.zeros((2, 2))] * 3 + [np.zeros((1, 2))], [np.zeros(2)] * 4 + [np.zeros(1)])
    with pytest.raises(ValueError, match="layers"):
        five.record()


def test_fit_value_learns_a_linear_reward(orc, tmp_path):
    """Synthetic episodes whose reward is a noiseless linear function of the state, fixed seed: the fit's final loss is below a
    tenth of the constant predictor's, and the file it writes loads and evaluates through the checker."""
    from mbd_hip.planners.value import ValueNet
    from mbd_hip.scripts import fit_value
    rng = np.random.default_rng(0)
    S, T, E, P = 6, 40, 2, 6
    A = np.eye(S) * 0.9 + rng.normal(size=(S, S)) * 0.05
    w = rng.normal(size=S)
    files = []
    for p in range(P):
        s = np.zeros((T * E + 1, S))
        s[0] = rng.normal(size=S)
        for t in range(T * E):
            s[t + 1] = A @ s[t] + rng.normal(size=S) * 0.3
        f = tmp_path / f"ep{p}.npz"
        np.savez(f, states=s[::E].astype(np.float32), rewards=(s[:-1] @ w).astype(np.float32))
        files.append(str(f))
    out = tmp_path / "value.npz"
    res = fit_value.main(["--episodes", *files, "--hidden", "16", "--discount", "0.9", "--steps_ahead", "4", "--steps", "600",
                          "--seed", "0", "--out", str(out)])
    print(res)
    assert res["samples"] == P * (T - 1) and res["loss"] < 0.1 * res["loss_const"]
    vn = ValueNet.load(out)
    assert vn.widths == [16, 1] and vn.n_in == S
    X, y = fit_value.targets(fit_value.load_episodes(files), 0.9, 4)
    V = vc.value(orc, vc.Net(vn.W, vn.b, vn.act, vn.center, vn.in_scale, vn.rel_xy, vn.scale), X)
    assert float(np.mean((V - y) ** 2)) == pytest.approx(res["loss"], rel=1e-3)
