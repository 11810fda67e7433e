"""The case table of tests/containment_inputs.py held to the checker and to the library's launch choices, without a device.

(1) Every poison is one: in the checker every healthy candidate stays finite, every poisoned one equals its healthy twin on
the rows before T0 and has a non-finite reward on every row from T0 on (the tracking reward, computed from the incoming
state: from T0 + 1 on); the poisoned start state diverges in the first control
step; a gear of 1e20 would not.  (2) Every case REACHES the sharing it claims: from mbd_debug_rollout_choice (instantiation,
candidates per wavefront) and mbd_debug_dpp_layout (the lane table) alone, a healthy and a poisoned candidate — or two plans of a
sweep — sit in one 16-lane DPP row, in one lane of a two-per-lane kernel, or only in one wavefront, as containment_inputs.EXPECT
and SWEEPS say; what the lone last candidate shares is worked out from the layout and may only be what the launch's kind says
or less.  An edit of the table or of choose_rollout that stops covering a form fails here."""
import ctypes as C

import numpy as np
import pytest

import containment_inputs as ci
import state_inputs as si

N_CUS = 256
MODELS = sorted({n for n, _ in ci.rollout_matrix()})


@pytest.mark.parametrize("name", MODELS)
def test_every_poison_diverges_and_every_twin_does_not(name):
    ref = ci.reference(name)
    rew_t, xpos_t, fin_t = ref["twin"]
    rew_b, xpos_b, fin_b = ref["bad"]
    assert np.isfinite(rew_t).all() and np.isfinite(xpos_t).all() and np.isfinite(fin_t).all()
    if ref["model"].act_size() > 1:  # (the cartpole's one actuator is the poisoned one: its healthy candidates are all zeros)
        assert len({r.tobytes() for r in rew_t}) == ref["B"], "healthy candidates must differ from each other"
    si.same_bits(rew_b[:, :ci.T0], rew_t[:, :ci.T0], f"{name}: a poisoned candidate before T0 is its twin")
    si.same_bits(xpos_b[:, :ci.T0], xpos_t[:, :ci.T0], f"{name}: tracked positions before T0")
    bad = ci.first_bad_row(ref["model"])
    assert not np.isfinite(rew_b[:, bad:]).any(), f"{name}: finite reward rows from row {bad} on: {np.isfinite(rew_b[:, bad:]).sum(0)}"
    assert not np.isfinite(fin_b).all(axis=tuple(range(1, fin_b.ndim))).any(), f"{name}: a poisoned candidate ends finite"


@pytest.mark.parametrize("name", ["hopper", "halfcheetah", "humanoidrun"])
def test_a_gear_of_1e20_is_no_poison(orc, name):
    m, _ = ci.model(name)
    g = np.array(m.fields["act_gear"], np.float32)
    g[0] = np.float32(1e20)
    m.fields["act_gear"] = g
    us = ci.poison_actions(ci.healthy_actions(m, 8), np.ones(8, bool), t0=0)
    assert np.isfinite(orc.rollout(m.to_struct(), si.init_state(orc, m), us)).all()


@pytest.mark.parametrize("name", sorted({n for n, *_ in ci.SWEEPS} | {ci.DEMO_SWEEP[0]}))
def test_the_poisoned_start_state_diverges_in_the_first_control_step(orc, name):
    m, _ = ci.model(name)
    s = ci.poison_state(si.init_state(orc, m))
    assert np.isfinite(s).all()
    us = ci.healthy_actions(m, 4)
    rew, fin = orc.rollout(m.to_struct(), s, us, want_final=True)
    bad = ci.first_bad_row(m, t0=0)  # (the tracking reward's row 0 is that of the start state itself: finite)
    assert not np.isfinite(rew[:, bad:]).any() and not np.isfinite(fin).all(axis=(1, 2)).any()
    assert np.isfinite(orc.rollout(m.to_struct(), si.init_state(orc, m), us)).all()


@pytest.mark.parametrize("name", sorted({n for n, _ in ci.ZERO_SIGN_MODELS}))
def test_the_zero_sign_cases_carry_zeros_of_both_signs_and_stay_finite(orc, name):
    m, _ = ci.model(name)
    n = 0
    for tag, s, us in ci.zero_sign_cases(orc, m):
        assert not us.any() and np.isfinite(orc.rollout(m.to_struct(), s, us)).all(), tag
        n += int(np.signbit(s[:, 11]).any() and not np.signbit(s[:, 11]).all())
    assert np.signbit(us).any() and not np.signbit(us).all() and n >= 2


# ---- reach ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def capi(lib):
    from mbd_hip import _capi
    return _capi


def dpp_layout(capi, ms):
    """(family, lane -> link table [16], shifts) of mbd_debug_dpp_layout."""
    from mbd_hip._capi import MbdModel
    lib = capi.load()
    lib.mbd_debug_dpp_layout.argtypes = [C.POINTER(MbdModel), C.c_char_p, C.POINTER(C.c_int)]
    tab = C.create_string_buffer(32)
    shifts = (C.c_int * 4)()
    fam = lib.mbd_debug_dpp_layout(C.byref(ms), tab, shifts)
    return fam, np.frombuffer(tab.raw, np.int8)[:16].copy(), list(shifts)


def crossing_reads(tab, shifts, lps):
    """The masked row shifts of a layout that leave the reader's lane group: [(reader lane, source lane, shift)] — a lane reads
    lane + D for every shift D of the layout (its parent's slot, used or discarded by the mask) and lane - D (its children's)."""
    out = []
    for d in [s for s in shifts if s != 0]:
        for sign in (1, -1):
            for lane in range(16):
                src = lane + sign * d
                if 0 <= src < 16 and src // lps != lane // lps:
                    out.append((lane, src, sign * d))
    return out


@pytest.mark.parametrize("name,kernel", ci.rollout_matrix())
def test_every_rollout_case_reaches_the_sharing_it_claims(capi, levers, name, kernel):
    ref = ci.reference(name)
    levers(**ci.KERNELS[kernel])
    ms = ref["model"].to_struct()
    healthy_choice = capi.debug_rollout_choice(ci.model(name)[0].to_struct(), N_CUS, ref["B"], ci.H, has_xref=False)
    choice = capi.debug_rollout_choice(ms, N_CUS, ref["B"], ci.H, has_xref=False)
    assert (choice["name"], choice["cpw"]) == (healthy_choice["name"], healthy_choice["cpw"]), \
        "the poisoned gear must not move the model off its instantiation"
    lay = ci.launch_layout(choice)
    claim = ci.EXPECT[(name, kernel)]
    if lay["per_lane"] == 1 and claim == "row":
        assert lay["lps"] == ref["lps"], (choice["name"], ref["lps"])
    if claim == "row":  # the layout's masked shifts really cross into the neighbouring lane group
        fam, tab, shifts = dpp_layout(capi, ms)
        assert fam >= 0 and lay["dpp"] and crossing_reads(tab, shifts, lay["lps"]), (choice["name"], fam, shifts)
    for pattern in ci.PATTERNS:
        kinds = ci.sharing(lay, ref["B"], ci.poisoned(pattern, ref["B"], ref["lps"]))
        got = ci.closest(kinds)
        what = f"{name} [{kernel}] {pattern}: {choice['name']} cpw {choice['cpw']} shares {kinds}, claimed {claim}"
        if pattern == "last":  # (B - 1 beside its own tail copies: the launch's kind or less, worked out from the layout)
            assert got in ci.NO_CLOSER[claim], what
        else:  # the closest sharing of the launch is the claimed one: the controls share nothing closer than a wavefront
            assert got == claim, what


def test_the_halfcheetah_default_launch_puts_two_candidates_into_one_row(capi):
    """At every size the issue names (the BASELINE config's N = 1024, sweeps of 33 and 96, this module's B): the filled kernel,
    lanes [3, 2, 1, 0, 6, 5, 4, -1], shifts (+1, -3); lanes 8-10 read lanes 5-7 and back."""
    m, _ = ci.model("halfcheetah")
    fam, tab, shifts = dpp_layout(capi, m.to_struct())
    assert list(tab[:8]) == [3, 2, 1, 0, 6, 5, 4, -1] and shifts[:2] == [1, -3]
    cr = crossing_reads(tab, shifts, 8)
    assert {(8, 5, -3), (9, 6, -3), (10, 7, -3), (5, 8, 3), (6, 9, 3), (7, 10, 3), (7, 8, 1), (8, 7, -1)} <= set(cr)
    for B, plan_N in ((1024, 0), (35, 0), (99, 33), (288, 96)):
        c = capi.debug_rollout_choice(m.to_struct(), N_CUS, B, ci.H, sweep_plan_N=plan_N)
        lay = ci.launch_layout(c)
        assert (lay["lps"], lay["dpp"], lay["cpw"]) == (8, True, 0), c


@pytest.mark.parametrize("name,kernel,N,claim", ci.SWEEPS)
def test_every_sweep_case_reaches_the_sharing_it_claims(capi, levers, name, kernel, N, claim):
    levers(**ci.KERNELS[kernel])
    m, _ = ci.model(name)
    B = ci.SWEEP_P * N
    choice = capi.debug_rollout_choice(m.to_struct(), N_CUS, B, ci.SWEEP_H, sweep_plan_N=N)
    lay = ci.launch_layout(choice)
    kinds = ci.sharing(lay, B, np.arange(B) // N == 1)
    if claim == "none":
        assert not kinds, (choice, kinds)
    else:
        assert claim in kinds and "lane" not in kinds, (choice, kinds)
        if claim == "wave":
            assert kinds == {"wave"}
    if kernel == "pk2":
        assert lay["per_lane"] == 2
    if N % 2:
        assert lay["per_lane"] == 1, "an odd plan must not be launched two candidates per lane"


def test_the_demo_sweep_accumulates_the_log_density_in_its_rollouts(capi):
    """The humanoidtrack sweep of containment_inputs.DEMO_SWEEP: its planning launch (P * N candidates, the demo's 50 rows, an
    env with the demo) takes the instantiation that accumulates the demo log-density itself, one candidate per row, and the
    poisoned plan shares wavefronts with both its neighbours."""
    name, N, H, _ = ci.DEMO_SWEEP
    m, _ = ci.model(name)
    B = ci.SWEEP_P * N
    choice = capi.debug_rollout_choice(m.to_struct(), N_CUS, B, H, sweep_plan_N=N, has_xref=True)
    assert choice["fuses_logpd"], choice
    lay = ci.launch_layout(choice)
    assert (lay["lps"], lay["per_lane"]) == (16, 1)
    assert ci.sharing(lay, B, np.arange(B) // N == 1) == {"wave"}
    assert not capi.debug_rollout_choice(m.to_struct(), N_CUS, B, ci.H, sweep_plan_N=N, has_xref=True)["fuses_logpd"], \
        "at the H = 6 of the env.rollout cases no launch accumulates it: the sweep is the only way there"


def test_every_kind_of_sharing_has_a_case():
    assert {ci.EXPECT[c] for c in ci.rollout_matrix()} == {"row", "lane", "wave", "none"}
    assert ci.EXPECT[("halfcheetah", "default")] == "row"
    assert any(c == "row" and N == 33 for *_, N, c in ci.SWEEPS)
