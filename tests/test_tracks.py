"""Tracked links beyond humanoidtrack's five, without a device (tests/track_inputs.py): what check_model refuses of a caller's
n_track / track_link, the checker's tracked positions against the link origins recomputed in float64 from its own final
state, the checker's two demo log-densities against float64 numpy, and RigidBodyEnv's xref / rew_xref keywords.
tests/test_gpu_tracks.py holds the kernels to the checker by bit pattern; this file holds the checker."""
import ctypes as C

import numpy as np
import pytest

import state_inputs as si
import track_inputs as ti
from conftest import load_model

# Worst relative error of the checker's float32 log-densities against float64 numpy on the same float32 inputs, in units of
# 2^-24, measured over the inputs of test_checker_log_densities_against_float64 (random positions at four spreads and the
# crafted sets, K = 1 ... 8): 6.14 (track form) and 4.87 (car2d).  The bounds are twice that.
TRACK_WORST, CAR2D_WORST = 6.14, 4.87
TRACK_BOUND, CAR2D_BOUND = 2 * TRACK_WORST, 2 * CAR2D_WORST
U = 2.0 ** -24


def _create(lib, st, xref=None):
    """(code, message) of mbd_env_create_model on a stand-in struct; an env that does get created is destroyed again."""
    h = C.c_void_p()
    rc = lib.mbd_env_create_model(b"stand-in", 0, C.byref(st), None if xref is None else xref.ctypes.data_as(C.c_void_p), 0.0,
                                  C.byref(h))
    msg = lib.mbd_last_error().decode() if rc != 0 else ""
    if rc == 0:
        lib.mbd_env_destroy(h)
    return rc, msg


def _struct(name="humanoidrun", n_track=0, links=(), flags=None):
    st = load_model(name).to_struct()
    st.n_track = n_track
    for k, l in enumerate(links):
        st.track_link[k] = l
    if flags is not None:
        st.flags = flags
    return st


REFUSALS = [
    ("n_track_9", dict(n_track=9, links=range(8)), "n_track"),
    ("n_track_10", dict(n_track=10, links=range(8)), "n_track"),
    ("n_track_11", dict(n_track=11, links=range(8)), "n_track"),
    ("n_track_huge", dict(n_track=1 << 20), "n_track"),
    ("n_track_negative", dict(n_track=-1), "n_track"),
    ("link_at_n_links", dict(n_track=2, links=(0, 11)), "track_link[1]"),
    ("link_negative", dict(n_track=3, links=(4, 2, -1)), "track_link[2]"),
    ("link_twice", dict(n_track=4, links=(10, 0, 5, 5)), "track_link"),
    ("link_twice_first_and_last", dict(n_track=8, links=(3, 1, 2, 4, 5, 6, 7, 3)), "track_link"),
    ("planar_tracked", dict(name="hopper", n_track=1, links=(0,)), "MBD_FLAG_PLANAR"),
]


@pytest.mark.parametrize("case,kw,field", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_check_model_refuses_what_no_kernel_serves(lib, case, kw, field):
    """MBD_ERR_INVALID before any device is looked for (so here too), the message naming the field; the same structs through
    mbd_debug_rollout_choice, which checks a model the same way."""
    from mbd_hip import _capi
    st = _struct(**kw)
    if case == "planar_tracked":
        assert st.flags & 2, "hopper is compiled planar"
    xref = np.zeros((ti.MAX_TRACK, 50, 3), np.float32)
    for xr in (None, xref):
        rc, msg = _create(lib, st, xr)
        assert rc == _capi.MBD_ERR_INVALID, (case, rc, msg)
        assert field in msg, (case, msg)
    if case == "planar_tracked":
        assert "no positions" in msg and "planar=False" in msg, msg
    if case.startswith("link_twice"):
        assert "once" in msg, msg
    with pytest.raises(_capi.MbdError) as e:
        _capi.debug_rollout_choice(st, 256, 8, 7)
    assert e.value.code == _capi.MBD_ERR_INVALID and field in str(e.value)


def test_check_model_reads_no_slot_past_n_track(lib):
    """n_track = 0 with garbage in track_link, and K < 8 with garbage behind slot K: accepted as far as the device."""
    from mbd_hip import _capi
    for n, links in ((0, (-7, 99, 5, 5, 1 << 30, -1, 0, 0)), (2, (3, 0, 3, 0, -1, 77, 3, 3)), (8, (7, 6, 5, 4, 3, 2, 1, 0))):
        rc, msg = _create(lib, _struct(n_track=n, links=links))
        assert rc in (_capi.MBD_OK, _capi.MBD_ERR_NO_DEVICE), (n, rc, msg)
    # the compiler's own rule: a model with track_names is never flagged planar, so what it hands over is accepted
    m, _ = ti.base_model("tripod")
    assert int(m.fields["n_track"]) == 2 and not si.is_planar(m)
    rc, msg = _create(lib, m.to_struct())
    assert rc in (_capi.MBD_OK, _capi.MBD_ERR_NO_DEVICE), (rc, msg)


def test_tracked_is_a_copy():
    m = load_model("humanoidtrack")
    t = ti.tracked(m, [4, 6, 3])
    assert int(m.fields["n_track"]) == 5 and list(m.fields["track_link"]) == [0, 5, 3, 6, 4]
    st = t.to_struct()
    assert st.n_track == 3 and list(st.track_link)[:3] == [4, 6, 3]
    for name in ("parent", "com", "inv_mass"):
        assert t.fields[name] is m.fields[name]


def _origin64(m, state, l):
    s = np.asarray(state, np.float64)
    return s[l, :3] - si._rot64(s[l, 3:7], np.asarray(m.fields["com"], np.float64)[l])


@pytest.mark.parametrize("row,model,links,forms", ti.ROWS, ids=[r[0] for r in ti.ROWS])
def test_checker_positions_are_the_link_origins_of_its_final_state(orc, row, model, links, forms):
    """xpos[b, H - 1, k] = p - R(q) com of link track_link[k], in float64 from the checker's own final state, to 1e-6 m (measured over
    this table: 6.2e-8 at worst) — for every row of the table and, for the specification-switch form, the switched model.  Slots differ
    from one another (a slot written from its neighbour's link would show) and the positions change along the rollout."""
    m, _, ls = ti.row_model(model, links)
    B, H = 3, 7
    for form in ("tuned",) + (("spec",) if "spec" in forms else ()):
        mm = ti.form_model(m, form)
        s0 = si.init_state(orc, mm)
        us = si.actions(mm, si._seed("tracks", row), b=max(B, 6), h=H)[:B]
        rew, xpos, fin = orc.rollout(mm.to_struct(), s0, us, want_xpos=True, want_final=True)
        assert xpos.shape == (B, H, len(ls), 3) and np.isfinite(xpos).all() and np.isfinite(fin).all()
        worst = 0.0
        for b in range(B):
            for k, l in enumerate(ls):
                worst = max(worst, float(np.abs(xpos[b, H - 1, k] - _origin64(mm, fin[b], l)).max()))
        assert worst <= 1e-6, (row, form, worst)
        for k in range(1, len(ls)):
            assert not np.array_equal(xpos[:, :, k], xpos[:, :, k - 1])
        assert not np.array_equal(xpos[:, 0], xpos[:, H - 1])
        # positions AFTER the control step: the first row is not the start state's
        first = np.stack([_origin64(mm, s0, l) for l in ls])
        assert np.abs(xpos[0, 0] - first).max() > 1e-7, (row, form)


def test_checker_fills_every_slot_of_a_link_named_twice(orc):
    """What the library refuses the checker itself can do: slots 2 and 3 of tracks [10, 0, 5, 5] hold the same positions."""
    m = ti.tracked(load_model("humanoidrun"), [10, 0, 5, 5])
    us = si.actions(m, 1, b=6, h=4)
    _, xpos = orc.rollout(m.to_struct(), si.init_state(orc, m), us, want_xpos=True)
    assert np.array_equal(xpos[:, :, 2], xpos[:, :, 3]) and np.abs(xpos[:, :, 3]).min() > 0


def _random_inputs(K, spread, seed, B=24):
    g = np.random.default_rng(si._seed("logpd", K, spread, seed))
    xref = g.normal(size=(K, 50, 3)).astype(np.float32)
    xpos = (xref.transpose(1, 0, 2)[None] + g.normal(size=(B, 50, K, 3)) * spread).astype(np.float32)
    return xref, xpos


SPREADS = (0.01, 0.15, 0.4, 2.0)


def test_checker_log_densities_against_float64(orc):
    """orc.track_xref_logpd at K = 1 ... 8 and orc.car2d_xref_logpd against float64 numpy on the same float32 inputs: random
    positions at four spreads around the demonstration (nearly all inside the clip ... nearly all saturated) plus the crafted
    sets of track_inputs (distances of exactly 0, one float to either side of 0.5 and 0.5 itself, squares that overflow,
    underflow and land on subnormals, an infinite coordinate, and the sum-order candidate whose terms span ten orders of
    magnitude).  Worst relative error measured, in units of 2^-24: 6.14 for the track form (random inputs at spread 0.01, K = 1;
    the crafted sets alone: 2.05) and 4.87 for car2d; the bounds are twice the worst: 12.28 and 9.74.  The kernels are held to
    the checker by bit pattern (tests/test_gpu_tracks.py), the checker to float64 by this bound."""
    worst_t = worst_c = 0.0
    counts = np.zeros(3, int)
    for K in range(1, ti.MAX_TRACK + 1):
        sets = [_random_inputs(K, s, 0) for s in SPREADS]
        sets.append(ti.crafted(_random_inputs(K, 0.1, 1)[0], 9, K))
        for xref, xpos in sets:
            t = ti.terms64(xpos, xref)
            counts += ti.census(t)
            ref = ti.logpd64(xpos, xref)
            got = np.array([orc.track_xref_logpd(x, xref) for x in xpos], np.float64)
            assert np.isfinite(ref).all() and np.isfinite(got).all()
            assert np.all(np.abs(got - ref) <= TRACK_BOUND * U * np.abs(ref)), (K, np.abs(got - ref).max())
            nz = ref != 0
            worst_t = max(worst_t, float((np.abs(got - ref)[nz] / np.abs(ref)[nz]).max() / U))
    assert counts.min() > 0, counts
    g = np.random.default_rng(3)
    car = [(xr, (np.concatenate([xr, np.zeros((50, 1), np.float32)], 1)[None] + g.normal(size=(24, 50, 3)) * s).astype(np.float32))
           for s in SPREADS for xr in [g.normal(size=(50, 2)).astype(np.float32)]]
    car.append(ti.crafted_car2d(car[0][0], 9, 0))
    assert min(ti.census(ti.terms64_car2d(car[-1][1], car[-1][0]))) > 0  # (zero, inside and saturated terms)
    for xref, qs in car:
        ref = ti.logpd64_car2d(qs, xref)
        got = np.array([orc.car2d_xref_logpd(q, xref) for q in qs], np.float64)
        assert np.isfinite(ref).all() and np.isfinite(got).all()
        assert np.all(np.abs(got - ref) <= CAR2D_BOUND * U * np.abs(ref)), np.abs(got - ref).max()
        nz = ref != 0
        worst_c = max(worst_c, float((np.abs(got - ref)[nz] / np.abs(ref)[nz]).max() / U))
    print(f"worst relative error in units of 2^-24: track {worst_t:.3f}, car2d {worst_c:.3f}")
    # the recorded worst values are what this test measures (the bounds come from them, not the other way round)
    assert worst_t <= TRACK_WORST + 0.01 and worst_c <= CAR2D_WORST + 0.01, (worst_t, worst_c)
    assert worst_t > 0.5 * TRACK_WORST and worst_c > 0.5 * CAR2D_WORST, (worst_t, worst_c)


@pytest.mark.parametrize("K", range(1, ti.MAX_TRACK + 1))
def test_crafted_sets_hold_every_kind_of_term_and_tell_the_sum_orders_apart(orc, K):
    """Every crafted batch has terms that are zero, strictly inside the clip and saturated; the boundary entries sit where
    they are meant to (float32 arithmetic, exact); a numpy float32 restatement of the contract (track_inputs.terms32 and
    contract32) gives the checker's bits for every candidate; and the sum-order candidate's value differs from the same terms
    added as one chain over all K H of them — the order the contract replaced — for every K >= 2."""
    m = ti.tracked(load_model("humanoidrun"), list(range(10, 10 - K, -1)))
    xref0 = ti.make_xref(orc, m, si.init_state(orc, m), K)
    assert xref0.shape == (K, 50, 3)
    xref, xpos = ti.crafted(xref0, 9, K)
    assert np.array_equal(xref, ti.crafted(xref0, 2, K + 1)[0]), "xref' does not depend on B or the seed"
    z, i, s = ti.census(ti.terms64(xpos, xref))
    assert min(z, i, s) > 0
    d = (xpos[0, :, :, 0] - xref.transpose(1, 0, 2)[:, :, 0]).astype(np.float32)
    same = np.all(xpos[0, :, :, 1:] == xref.transpose(1, 0, 2)[:, :, 1:], axis=-1)
    for v in (ti.BELOW, np.float32(0.5), ti.ABOVE):
        assert np.any((d == v) & same), v
    last = xpos[-1]
    t32 = ti.terms32(last, xref)
    assert t32[:, 0].max() == 1.0 and 0 < t32[:, 0].min() < 2e-10
    # numpy's float32 restatement of the contract, term by term and in its order, is the checker bit for bit ...
    n = np.float32(K * 50)
    for x in xpos:
        si.same_bits(np.float32(np.float32(0) - ti.contract32(ti.terms32(x, xref)) / n), orc.track_xref_logpd(x, xref), f"K={K}")
    if K >= 2:  # ... and the same terms as one chain are not
        assert np.float32(orc.track_xref_logpd(last, xref)) != np.float32(np.float32(0) - ti.chain32(t32) / n)


def test_rollout_demonstrations_put_distances_on_both_sides_of_the_clip(orc):
    """make_xref's demonstrations, as the demo plans of tests/test_gpu_tracks.py use them: candidates sampled around the start
    state have terms strictly inside the clip and saturated terms (exact zeros come from the crafted sets only)."""
    for model, links in (("humanoidtrack", [0]), ("humanoidrun", [10, 0, 5]), ("ant", [8, 0, 4])):
        m = ti.tracked(load_model(model), links)
        s0 = si.init_state(orc, m)
        xref = ti.make_xref(orc, m, s0, 7)
        us = np.clip(np.random.default_rng(0).normal(size=(8, 50, m.act_size())) * 0.5, -1, 1).astype(np.float32)
        _, xpos = orc.rollout(m.to_struct(), s0, us, want_xpos=True)
        z, i, s = ti.census(ti.terms64(xpos, xref))
        assert i > 0 and s > 0, (model, z, i, s)
        lp = ti.logpd64(xpos, xref)
        assert np.ptp(lp) > 1e-3, "the candidates' log-densities differ"


class _FakeLib:
    """libmbd_hip as far as RigidBodyEnv's constructor calls it before mbd_env_create_model answers."""

    def __init__(self):
        self.calls = []

    def mbd_env_create(self, name, device, out):
        self.calls.append(("create", name))
        return -4

    def mbd_env_create_model(self, name, device, st, xref, rew_xref, out):
        n = st._obj.n_track * 50 * 3
        x = None if xref is None else np.ctypeslib.as_array(C.cast(xref, C.POINTER(C.c_float)), shape=(n,)).copy()
        self.calls.append(("create_model", name, st._obj.n_track, x, rew_xref))
        return -4

    def mbd_last_error(self):
        return b"no gfx950 device visible"


def test_rigid_body_env_hands_a_callers_demonstration_to_the_library(monkeypatch, orc):
    """RigidBodyEnv(env_name, model=..., xref=..., rew_xref=...) reaches mbd_env_create_model with those floats; without the
    keywords nothing changes: humanoidtrack gets its own demo and 1.0, every other name none and 0.0."""
    import os

    from mbd_hip import _capi
    from mbd_hip.envs.base import _ASSETS, RigidBodyEnv
    fake = _FakeLib()
    monkeypatch.setattr(_capi, "load", lambda: fake)
    m = ti.tracked(load_model("humanoidrun"), [10, 0, 5])
    xref = ti.make_xref(orc, m, si.init_state(orc, m), 3)

    def call(*a, **kw):
        with pytest.raises(_capi.MbdError) as e:
            RigidBodyEnv(*a, **kw)
        assert e.value.code == _capi.MBD_ERR_NO_DEVICE
        return fake.calls[-1]
    what, name, K, x, rx = call("humanoidrun", model=m, xref=xref, rew_xref=0.625)
    assert (what, name, K, rx) == ("create_model", b"humanoidrun", 3, 0.625) and x.tobytes() == xref.tobytes()
    what, name, K, x, rx = call("humanoidrun", model=m)
    assert (what, K, x, rx) == ("create_model", 3, None, 0.0)
    track = load_model("humanoidtrack")
    jog = np.load(os.path.join(_ASSETS, "compiled", "jog_xref.npy")).astype(np.float32)
    what, name, K, x, rx = call("humanoidtrack", model=track)
    assert (what, K, rx) == ("create_model", 5, 1.0) and x.tobytes() == jog.tobytes()
    one = ti.tracked(track, [0])
    what, name, K, x, rx = call("humanoidtrack", model=one, xref=xref[:1], rew_xref=2.0)  # (its own demo replaces the built-in one)
    assert (K, rx) == (1, 2.0) and x.tobytes() == xref[:1].tobytes()
    assert call("humanoidrun")[:2] == ("create", b"humanoidrun")
    with pytest.raises(ValueError, match="pass xref="):  # (its own five tracks do not fit a retracked model)
        RigidBodyEnv("humanoidtrack", model=one)
    with pytest.raises(ValueError, match="shape"):
        RigidBodyEnv("humanoidrun", model=m, xref=xref[:2])
    with pytest.raises(ValueError, match="model="):
        RigidBodyEnv("humanoidrun", xref=xref)
