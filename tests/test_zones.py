"""The zone record without a GPU (include/mbd_hip.h mbd_zones; DESIGN.md section 1 "N20 zones"): mbd_debug_zones_host — the
functions zones_kernel calls, looped on the CPU — against the numpy restatement tests/zones_checker.py at every size and crafted
input of tests/zones_inputs.py; the census of the whole-plan cases; every refusal the record alone decides, with its message, and
what a handle without a device reaches of the set, update and peek calls; Model.tracked and get_env(track=...); mpc.py's flags
reaching the Plan's and the Sweep's calls.  tests/test_gpu_zones.py holds the device code."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import zones_checker as zc
import zones_inputs as zi
from conftest import ROOT, load_model

F32 = np.float32
NEW = ("mbd_plan_set_zones", "mbd_plan_update_zones", "mbd_plan_peek_zones", "mbd_plan_peek_mpc_zones", "mbd_sweep_set_zones",
       "mbd_sweep_update_zones", "mbd_sweep_peek_zones", "mbd_sweep_peek_mpc_zones")
DEBUG = ("mbd_debug_check_zones", "mbd_debug_zones_host", "mbd_debug_zones_step")


def _rec(zones, K):
    from mbd_hip import _capi
    return _capi.zones_record(zones, K)


def test_header_exports_and_library_agree(lib):
    from mbd_hip import _capi
    text = open(os.path.join(ROOT, "include", "mbd_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for n in NEW:
        assert re.search(rf"\bint {n}\s*\(", code), f"{n} is not declared in include/mbd_hip.h"
        assert n in _capi.EXPORTS and hasattr(lib, n), n
    dbg = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mbd_hip_debug.h")).read(), flags=re.S)
    for n in DEBUG:
        assert re.search(rf"\bint {n}\s*\(", dbg) and hasattr(lib, n), n
    # the contract's text, as the issue gives it
    assert "#define MBD_MAX_ZONES 16" in text and "enum { MBD_ZONE_KEEP_OUT = 0, MBD_ZONE_GOAL = 1 };" in text
    assert ("typedef struct { int32_t kind; uint32_t links; float center[3]; float scale[3]; float radius, margin, weight; "
            "int32_t reserved; } mbd_zone;") in text
    assert "typedef struct { int32_t n_zones; int32_t reserved[3]; mbd_zone zone[MBD_MAX_ZONES]; } mbd_zones;" in text
    assert C.sizeof(_capi.Zone) == 48 and C.sizeof(_capi.Zones) == 16 + 16 * 48


# ---- the launch on the host against the restatement -------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H", [(B, H) for B in (1, 5) for H in (1, 50, 64, 65)])
def test_host_launch_matches_the_checker(lib, B, H):
    from mbd_hip import _capi
    for K in (1, 3, 8):
        for Z in (1, 16):
            zones, xpos, rews = zi.crafted(B, H, K, Z)
            what = f"B={B} H={H} K={K} Z={Z}"
            got = _capi.debug_zones_host(_rec(zones, K), xpos, rews)
            ref = zc.launch(zones, xpos, rews)
            zc.same_launch(got, ref, what)
            # the crafted row does what it is meant to: distances exactly AT r and AT r + m, every class of term, and — H allowing —
            # infinite and zero distances from the squares that overflow and underflow
            if H >= 50:
                n_r, n_rm = zi.boundary_hits(zones, xpos)
                assert n_r >= 2 and n_rm >= 2, what
                v = zc.classes(zones, xpos[:1])
                assert (v == 0).any() and ((v > 0) & (v < 1)).any() and (v == 1).any(), what
                d0 = zc.distance(xpos[0], zones[0])
                assert np.isinf(d0).any() and (d0 == 0).any() and ((d0 > 0) & (d0 < 1e-19)).any(), what
            if B > 2:  # the row with the inf and the NaN, next to clean rows: they keep the bits they have without it
                assert np.isnan(ref["pen"][2]) and np.isfinite(np.delete(ref["pen"], 2)).all(), what
                clean = xpos.copy()
                clean[2] = clean[1]
                alone = _capi.debug_zones_host(_rec(zones, K), clean, rews)
                for k in ("rews", "pen", "clr", "step_pen", "step_clr"):  # (clean rows hold no NaN: bit patterns throughout)
                    zc.same_clr(np.delete(got[k], 2, axis=0), np.delete(alone[k], 2, axis=0), f"{what}: the neighbours' {k}")
                if any(z["kind"] == zc.KEEP_OUT and z["links"] & (1 << (K - 1)) and z["scale"][1] for z in zones):
                    assert zc.bits(got["clr"])[2] == 0x7fc00000, f"{what}: the NaN of clr is the canonical one"


def test_masks_scales_and_zero_weights():
    """What the table of zones_inputs holds: a slot no zone covers, every single-axis and two-axis scale, a weight 0, a radius 0 —
    and the restatement honours them: a term outside the mask contributes nothing, a zone of weight 0 adds +0."""
    zones = zi.table(8, 16)
    assert {tuple(int(v) for v in z["scale"]) for z in zones} >= set(zi.SCALES)
    assert any(z["weight"] == 0 for z in zones) and any(z["radius"] == 0 for z in zones)
    one = zi.table(3, 1)
    assert one[0]["links"] == 0b101, "slot 1 is covered by no zone"
    _, xpos, _ = zi.crafted(5, 50, 3, 1)
    moved = xpos.copy()
    moved[:, :, 1] += F32(7.0)
    for k in ("pen", "clr"):
        zc.same_clr(zc.launch(one, moved)[k], zc.launch(one, xpos)[k], f"a slot outside the mask: {k}")
    zones, xpos, rews = zi.crafted(5, 50, 8, 16)
    xpos = np.nan_to_num(xpos, nan=0.0, posinf=1.0)
    zero = [dict(z, weight=0.0) for z in zones]
    out = zc.launch(zero, xpos, rews)
    assert not zc.bits(out["pen"]).any(), "every weight 0: pen is +0"
    zc.same(out["rews"], rews, "every weight 0: the rewards keep their bits")


@pytest.mark.parametrize("name,links,N,H", zi.PLANS, ids=[f"{p[0]}-N{p[2]}-H{p[3]}" for p in zi.PLANS])
def test_census_of_the_whole_plan_cases(lib, orc, name, links, N, H):
    """Every class of term holds at least 1 % of the (candidate, step, slot, zone) terms, at least a quarter of the candidates carry
    a penalty and at least one carries none — and the library's host launch agrees with the restatement on those positions."""
    from mbd_hip import _capi
    m = zi.plan_model(name, links)
    s0 = orc.forward(m.to_struct(), m.init_q, np.zeros(m.qd_size(), F32))
    zones, xpos = zi.place(orc, m, s0, N, H)
    zi.assert_census(zi.census(zones, xpos), f"{name} N={N} H={H}")
    rews = np.linspace(-1, 1, N).astype(F32)
    zc.same_launch(_capi.debug_zones_host(_rec(zones, 3), xpos, rews), zc.launch(zones, xpos, rews), f"{name} N={N} H={H}")


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def _good(K=3):
    from mbd_hip import _capi
    from mbd_hip.planners import mpc
    return _capi.zones_record([mpc.zone("out", (1, 0, 1), 0.3, 0.3, 5.0), mpc.zone("goal", (6, 0, 1.2), 0.2, 6.0, axes="xy", links=[0])], K)


REFUSALS = [
    (lambda r: setattr(r, "n_zones", 0), b"n_zones=0"),
    (lambda r: setattr(r, "n_zones", 17), b"n_zones=17"),
    (lambda r: r.reserved.__setitem__(1, 5), b"reserved[1]=5"),
    (lambda r: setattr(r.zone[1], "kind", 2), b"zone[1].kind=2"),
    (lambda r: setattr(r.zone[0], "kind", -1), b"zone[0].kind=-1"),
    (lambda r: setattr(r.zone[0], "links", 0), b"zone[0].links=0"),
    (lambda r: setattr(r.zone[1], "links", 0b1001), b"zone[1].links=0x9"),
    (lambda r: r.zone[0].center.__setitem__(2, float("inf")), b"zone[0].center[2]"),
    (lambda r: r.zone[0].center.__setitem__(0, float("nan")), b"zone[0].center[0]"),
    (lambda r: r.zone[1].scale.__setitem__(1, -1.0), b"zone[1].scale[1]"),
    (lambda r: r.zone[1].scale.__setitem__(0, float("nan")), b"zone[1].scale[0]"),
    (lambda r: [r.zone[0].scale.__setitem__(i, 0.0) for i in range(3)], b"zone[0].scale: all three"),
    (lambda r: setattr(r.zone[0], "radius", -0.1), b"zone[0].radius"),
    (lambda r: setattr(r.zone[0], "radius", float("inf")), b"zone[0].radius"),
    (lambda r: setattr(r.zone[1], "margin", 0.0), b"zone[1].margin"),
    (lambda r: setattr(r.zone[1], "margin", float("nan")), b"zone[1].margin"),
    (lambda r: setattr(r.zone[0], "weight", -1.0), b"zone[0].weight"),
    (lambda r: setattr(r.zone[0], "weight", float("inf")), b"zone[0].weight"),
    (lambda r: setattr(r.zone[1], "reserved", 1), b"zone[1].reserved=1"),
]


def test_every_refusal_names_its_field(lib):
    from mbd_hip import _capi
    I, S = _capi.MBD_ERR_INVALID, _capi.MBD_ERR_STATE
    assert _capi.debug_check_zones(_good(), 3) == 0
    assert _capi.debug_check_zones(None, 3) == I and b"NULL" in lib.mbd_last_error()
    assert _capi.debug_check_zones(_good(), 9) == I and b"n_track=9" in lib.mbd_last_error()
    # a zeroed stand-in handle (no env, no session, no record): the set call itself refuses in the same words before it looks at an
    # env; then, the record being fine, it refuses the env that tracks nothing
    stand_in = C.create_string_buffer(1 << 17)
    for mutate, word in REFUSALS:
        rec = _good()
        mutate(rec)
        assert _capi.debug_check_zones(rec, 3) == I and word in lib.mbd_last_error(), (word, lib.mbd_last_error())
        if b"links=0x9" in word:
            continue  # (a bit above n_track: decided against an env's tracks)
        for call in (lib.mbd_plan_set_zones, lib.mbd_sweep_set_zones):
            assert call(stand_in, C.byref(rec)) == I and word in lib.mbd_last_error(), (word, lib.mbd_last_error())
    for call in (lib.mbd_plan_set_zones, lib.mbd_sweep_set_zones):
        rec = _good()
        assert call(None, C.byref(rec)) == I and b"is NULL" in lib.mbd_last_error()
        assert call(stand_in, C.byref(rec)) == _capi.MBD_ERR_UNSUPPORTED
        msg = lib.mbd_last_error()
        assert b"tracks no link" in msg and b"planar=False" in msg and b"track_names" in msg
    rec = _good()
    for call in (lib.mbd_plan_update_zones, lib.mbd_sweep_update_zones):
        assert call(None, C.byref(rec)) == I
        assert call(stand_in, None) == I and b"zone record is NULL" in lib.mbd_last_error()
        assert call(stand_in, C.byref(rec)) == S and b"no zone record" in lib.mbd_last_error()
    assert lib.mbd_plan_peek_zones(None, None, None) == I and lib.mbd_plan_peek_mpc_zones(None, None, None) == I
    assert lib.mbd_sweep_peek_zones(None, 0, None, None) == I and lib.mbd_sweep_peek_mpc_zones(None, 0, None, None) == I
    assert lib.mbd_plan_peek_zones(stand_in, None, None) == S and b"no zone record" in lib.mbd_last_error()
    assert lib.mbd_plan_peek_mpc_zones(stand_in, None, None) == S and b"no zone record" in lib.mbd_last_error()
    assert not any(bytes(stand_in.raw))
    # the debug entries: argument errors before anything else; the device entry then says there is no device
    x = np.zeros((2, 3, 3, 3), F32)
    fn = lib.mbd_debug_zones_host
    fn.argtypes = [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p] * 5
    assert fn(None, x.ctypes.data, None, 2, 3, 3, None, None, None, None, None) == I
    assert fn(C.addressof(rec), None, None, 2, 3, 3, None, None, None, None, None) == I
    for B, H, K in ((0, 3, 3), (2, 0, 3), (2, 3, 0), (2, 3, 9)):
        assert fn(C.addressof(rec), x.ctypes.data, None, B, H, K, None, None, None, None, None) == I, (B, H, K)
    out = np.zeros(2, F32)
    assert fn(C.addressof(rec), x.ctypes.data, None, 2, 3, 3, out.ctypes.data, None, None, None, None) == I and b"rews_out needs rews" in lib.mbd_last_error()
    if _capi.device_count() == 0:
        with pytest.raises(_capi.MbdError) as e:
            _capi.debug_zones_step(rec, x, np.zeros(2, F32))
        assert e.value.code == _capi.MBD_ERR_NO_DEVICE


# ---- the Python layer -------------------------------------------------------------------------------------------------------------
def test_zone_entries_and_the_flag_syntax():
    from mbd_hip import _capi
    from mbd_hip.planners import mpc
    z = mpc.zone("out", (2, 0, 1), 0.3, 0.3, 5)
    assert z == dict(kind=0, center=[2.0, 0.0, 1.0], scale=[1.0, 1.0, 1.0], radius=0.3, margin=0.3, weight=5.0, links=None)
    assert mpc.zone("goal", (6, 0, 1.2), 0.2, 6, axes="xy")["scale"] == [1.0, 1.0, 0.0] and mpc.zone("goal", (0, 0, 0), 1, 1)["kind"] == 1
    assert mpc.zone("out", (0, 0, 0), 1, 1, axes="x")["scale"] == [1.0, 0.0, 0.0]
    for bad in (dict(kind="in"), dict(axes="xw"), dict(axes=""), dict(axes="xx"), dict(center=(1, 2))):
        kw = dict(kind="out", center=(0, 0, 0), radius=1, margin=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            mpc.zone(**kw)
    got = mpc.parse_zones("out:2,0,1:0.3:0.3:5;goal:6,0,1.2:0.2:6:1:xy")
    assert got == [mpc.zone("out", (2, 0, 1), 0.3, 0.3, 5), mpc.zone("goal", (6, 0, 1.2), 0.2, 6, 1, axes="xy")]
    assert mpc.parse_zones("out:0,0,0:1:1:2:z:torso,1")[0]["links"] == ["torso", 1]
    for bad in ("", "out:1,2,3:1", "out:a,b,c:1:1", "ring:0,0,0:1:1"):
        with pytest.raises(ValueError):
            mpc.parse_zones(bad)
    rec = _capi.zones_record(got, 3, ["torso", "left_shin", "right_shin"])
    assert rec.n_zones == 2 and rec.zone[0].links == 7 and rec.zone[1].kind == 1 and list(rec.zone[1].scale) == [1.0, 1.0, 0.0]
    named = _capi.zones_record([mpc.zone("out", (0, 0, 0), 1, 1, links=["left_shin", 0])], 3, ["torso", "left_shin", "right_shin"])
    assert named.zone[0].links == 0b011
    with pytest.raises(ValueError, match="not a tracked link"):
        _capi.zones_record([mpc.zone("out", (0, 0, 0), 1, 1, links=["head"])], 3, ["torso"])
    with pytest.raises(ValueError, match="1..16"):
        _capi.zones_record([], 3)
    rep = mpc.zones_report(dict(zone_pen=np.array([0.0, 0.5, 1.5], F32), zone_clear=np.array([0.2, -0.1, np.inf], F32)))
    assert rep == dict(zone_pen_mean=pytest.approx(2 / 3), zone_clear_min=pytest.approx(-0.1), zone_hits=1)


def test_model_tracked_and_get_env(lib):
    import track_inputs as ti
    from mbd_hip import _capi
    from mbd_hip.envs import builtin_model, get_env
    m = load_model("humanoidrun")
    t = m.tracked(["torso", m.n_links - 1, 5]) if "torso" in m.link_names else m.tracked([0, m.n_links - 1, 5])
    assert bytes(t.to_struct()) == bytes(ti.tracked(m, [0, m.n_links - 1, 5]).to_struct()), "the test helper's model"
    assert int(m.fields["n_track"]) == 0 and bytes(m.tracked([]).to_struct()) == bytes(m.to_struct())
    name = m.link_names[3]
    assert list(m.tracked([name]).fields["track_link"]) == [3]
    for bad, word in (([99], "outside"), (["no_such_link"], "no link named"), ([1, 1], "twice"), (list(range(9)), "at most 8")):
        with pytest.raises(ValueError, match=word):
            m.tracked(bad)
    with pytest.raises(ValueError, match="planar"):
        load_model("hopper").tracked([0])
    assert bytes(builtin_model("ant").to_struct()) == bytes(load_model("ant").to_struct())
    with pytest.raises(ValueError, match="car2d"):
        get_env("car2d", track=(0,))
    with pytest.raises(ValueError, match="planar"):
        get_env("hopper", track=(0,))
    with pytest.raises(ValueError, match="Unknown environment"):
        get_env("no_such_env", track=(0,))
    if _capi.device_count() == 0:  # (the retracked env is created like any other: loudly without a device)
        with pytest.raises(_capi.MbdError) as e:
            get_env("humanoidrun", track=(0, 5))
        assert e.value.code == _capi.MBD_ERR_NO_DEVICE


class _Recorder:
    """Stands in for a Plan or a Sweep: records the set_* calls ``mpc._setup`` / ``mpc._setup_batch`` make."""

    def __init__(self, *a, **kw):
        self.calls, self.P = {}, a[2] if len(a) > 2 else None

    def __getattr__(self, name):
        if name.startswith("set_"):
            return lambda *a, **kw: self.calls.__setitem__(name, (a, kw))
        raise AttributeError(name)


def test_the_python_layer_maps_every_flag(monkeypatch):
    """--zones and --zone_links reach get_env's track and Plan.set_zones / Sweep.set_zones; without the flags get_env is called as
    it always was and no record is set; a batch holds both fields equal."""
    from dataclasses import replace

    from mbd_hip.planners import mpc
    text = "out:2,0,1:0.3:0.3:5;goal:6,0,1.2:0.2:6:1:xy"
    base = mpc.MpcArgs(env_name="humanoidrun", not_render=True, disable_recommended_params=True)
    args = replace(base, zones=text, zone_links="torso,left_shin,7")

    class _Env:
        action_size = 3
    envs, made = [], []
    monkeypatch.setattr(mpc, "get_env", lambda name, **kw: envs.append(kw) or _Env())
    monkeypatch.setattr(mpc, "Plan", lambda *a, **kw: made.append(_Recorder(*a, **kw)) or made[-1])
    monkeypatch.setattr(mpc, "Sweep", lambda *a, **kw: made.append(_Recorder(*a, **kw)) or made[-1])
    monkeypatch.setattr(mpc, "_reset_and_key", lambda env, seed: (seed, (0, seed)))
    mpc._setup(args, 0)
    assert envs[-1] == dict(device=0, track=("torso", "left_shin", 7))
    assert made[-1].calls["set_zones"] == ((mpc.parse_zones(text),), {})
    mpc._setup(replace(args), 0, online=True)
    assert made[-1].calls["set_zones"] == ((mpc.parse_zones(text),), {}), "--online honours the flags"
    mpc._setup(base, 0)
    assert envs[-1] == dict(device=0) and "set_zones" not in made[-1].calls, "no flag: today's call, no record"
    arg_list = [replace(args, seed=k) for k in range(3)]
    mpc._check_batch_records(arg_list)
    mpc._setup_batch(arg_list, 0)
    assert made[-1].P == 3 and envs[-1] == dict(device=0, track=("torso", "left_shin", 7))
    assert made[-1].calls["set_zones"] == ((mpc.parse_zones(text),), {})
    mpc._setup_batch([replace(base, seed=k) for k in range(2)], 0)
    assert envs[-1] == dict(device=0) and "set_zones" not in made[-1].calls
    with pytest.raises(ValueError, match="zones differs"):
        mpc._check_batch_records([args, replace(args, zones="out:0,0,0:1:1", seed=1)])
    with pytest.raises(ValueError, match="zone_links differs"):
        mpc._check_batch_records([args, replace(args, zone_links="torso", seed=1)])
    assert mpc._zones_settings(args) == dict(zones=text, zone_links="torso,left_shin,7") and mpc._zones_settings(base) == {}
    assert "zone_pen" in mpc._logs(dict(zone_pen=0, zone_clear=0)) and "zone_clear" in mpc._logs(dict(zone_pen=0, zone_clear=0))
