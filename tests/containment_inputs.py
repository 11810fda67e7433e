"""Candidates that leave the finite numbers, next to candidates that do not: the case table of tests/test_containment_cases.py
(the checker on the CPU, and which lanes the cases share) and tests/test_gpu_containment.py (the kernels on the same cases, by
bit pattern), and the checker's results on them (`reference`, computed once and shared by both).  numpy and the checker only;
nothing here touches the library or a device.

HOW A CANDIDATE DIVERGES, from legal and finite inputs:

  by its actions      `poison_model`: the model with ONE actuator's gear set to GEAR = 1e30.  Healthy candidates carry exactly 0.0
                      in that actuator's column in every row (0 * 1e30 = 0: the gear is never felt) and seeded clipped normals
                      elsewhere, so they differ from each other; poisoned candidates carry 0.0 there up to row T0 and 1.0 from T0
                      on.  A torque of 1e30 overflows float32 within one control step (tests/test_containment_cases.py asserts 6 of
                      6 finite reward rows for healthy candidates, finite rows < T0 and non-finite rows >= T0 for poisoned ones;
                      1e20 does not diverge within six rows and is no poison).  The TWIN of a poisoned candidate is the same row of
                      actions with the poisoned column zeroed.
  by its start state  `poison_state`: the reset state with the root's angular velocity at 3e38 — finite, non-finite after the
                      first substep.  For sweeps and batches, which take one start state per plan.

POISON PATTERNS over a batch of B = 4 * (64 / LPS) + 3 candidates (four full wavefronts of the one-candidate-per-lane-group
layouts and a partial one): every even candidate, every odd one, one in the middle of a wavefront, and only candidate B - 1 —
the kernels' tail groups repeat candidate B - 1, so the lanes past the batch then hold poisoned copies beside healthy candidates.

KINDS of sharing a case exercises (`sharing`, host arithmetic on what mbd_debug_rollout_choice and mbd_debug_dpp_layout report):

  row    a healthy and a poisoned candidate in one 16-lane DPP row, whose masked row shifts read the neighbour's lanes
  lane   a healthy and a poisoned candidate in the two halves of one lane (the two-candidates-per-lane kernels)
  wave   only a shared wavefront (one candidate per row, or an exchange by ds_bpermute inside the lane group): the controls
  none   not even that: one candidate per wavefront, or plans that end where wavefronts do
"""
import copy
import functools
import re
import zlib

import numpy as np

import state_inputs as si

GEAR = 1e30
H, T0 = 6, 2
PATTERNS = ("even", "odd", "middle", "last")
ROOT_SPIN = 3e38

PLANAR = ("hopper", "walker2d", "halfcheetah", "cartpole")
HOT3D = ("ant", "humanoidrun", "humanoidstandup", "humanoidtrack")
# lever settings of each kernel family, as tests/test_gpu_states.py names them
KERNELS = {"default": {}, "no_dpp": dict(MBD_NO_DPP=1),
           "general": dict(MBD_NO_PLANAR_FLAGS=1, MBD_NO_REWARD_CONST=1, MBD_NO_NFR_CONST=1), "pk2": dict(MBD_PK2=1),
           "cpw0": dict(MBD_CPW=0), "cpw1": dict(MBD_CPW=1), "cpw2": dict(MBD_CPW=2), "cpw4": dict(MBD_CPW=4), "cpw8": dict(MBD_CPW=8),
           "no_unit": dict(MBD_NO_UNIT_CONST=1)}
SPEC_MODEL = ("hopper_spec16", "hopper", 16)  # a model with a specification bit set: the 16-lane shuffle instantiation


def rollout_matrix():
    """(model name of `model`, kernel family) of every env.rollout case."""
    out = []
    for n in PLANAR:
        out += [(n, k) for k in ("default", "no_dpp", "general", "cpw0", "cpw1", "cpw2", "cpw4", "cpw8")]
        out += [(n + "3d", "default")]
    out += [("halfcheetahCA", "default")]
    for n in HOT3D:
        out += [(n, k) for k in ("default", "no_dpp", "general", "pk2")]
    out += [("humanoidrun", "no_unit"), ("tripod", "default"), ("crab", "default"), (SPEC_MODEL[0], "default")]
    return out


def model(name):
    """(Model, env_name) of a case's model name: state_inputs' names, the halfcheetah under collide_all_capsules (four spheres on
    its torso: mbd_planar.h MAXCOL = 4), and the hopper with a specification bit."""
    if name == "halfcheetahCA":
        import os
        from mbd_hip import mjcf
        from mbd_hip.envs import specs
        sp = specs.SPECS["halfcheetah"]
        pkg = os.path.dirname(os.path.dirname(os.path.abspath(mjcf.__file__)))
        m = mjcf.load(os.path.join(pkg, "assets", sp["xml"]), env_name="halfcheetah", n_frames=sp["n_frames"],
                      reset_noise=sp["reset_noise"], reward_params=sp.get("reward_params", ()),
                      gear_override=sp.get("gear_override", ()), collide_all_capsules=True, warn_unstable=False)
        return m, "halfcheetah"
    if name == SPEC_MODEL[0]:
        return si.model(SPEC_MODEL[1], bits=SPEC_MODEL[2])
    return si.model(name)


def poison_model(m, actuator=0):
    """A copy of `m` whose actuator `actuator` has a gear of GEAR."""
    p = copy.deepcopy(m)
    g = np.array(p.fields["act_gear"], np.float32)
    g[actuator] = np.float32(GEAR)
    p.fields["act_gear"] = g
    return p


def poison_state(state, root=0):
    s = np.array(state, np.float32)
    s[root, 11] = np.float32(ROOT_SPIN)  # angular velocity about y: in the plane of the planar models
    return s


def batch_size(lps):
    return 4 * (64 // lps) + 3


def poisoned(pattern, B, lps):
    """[B] bool: which candidates of the batch are poisoned."""
    b = np.arange(B)
    if pattern == "even":
        return b % 2 == 0
    if pattern == "odd":
        return b % 2 == 1
    if pattern == "middle":
        spw = 64 // lps
        return b == spw + spw // 2
    if pattern == "last":
        return b == B - 1
    raise ValueError(pattern)


def healthy_actions(m, B, actuator=0, h=H):
    """[B][h][Nu] seeded clipped normals with exactly 0.0 in the poisoned actuator's column: the twins of every candidate."""
    nu = m.act_size()
    rng = np.random.default_rng(zlib.crc32(f"containment/{m.n_links}/{nu}/{B}".encode()))
    us = np.clip(rng.normal(size=(B, h, nu)) * 0.6, -1.3, 1.3).astype(np.float32)
    us[:, :, actuator] = np.float32(0.0)
    return us


def poison_actions(us, mask, actuator=0, t0=T0):
    """`us` with the poisoned column of the candidates in `mask` at 1.0 from row t0 on."""
    out = np.array(us, np.float32)
    out[np.asarray(mask, bool), t0:, actuator] = np.float32(1.0)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """dict of a model's rollout cases, computed once and left unchanged: the poisoned model, its launch-independent batch (B
    from the model's own lane-group width), the start state, the twins' actions, and the checker's (rewards, tracked positions,
    final states) of the all-healthy batch (`twin`) and of the batch with EVERY candidate poisoned (`bad`: candidates are
    independent in the checker, so a pattern's reference takes each candidate's rows from one or the other)."""
    from oracle import oracle
    oracle.build()
    orc = oracle.Oracle("f32")
    m, env_name = model(name)
    pm = poison_model(m)
    lps = lps_of(m)
    B = batch_size(lps)
    s0 = si.init_state(orc, pm)
    us = healthy_actions(pm, B)
    bad_us = poison_actions(us, np.ones(B, bool))
    ms = pm.to_struct()
    twin = orc.rollout(ms, s0, us, want_xpos=True, want_final=True)
    bad = orc.rollout(ms, s0, bad_us, want_xpos=True, want_final=True)
    return dict(model=pm, env_name=env_name, lps=lps, B=B, s0=s0, us=us, twin=twin, bad=bad)


def expected(ref, mask):
    """The checker's (rewards, positions, final states) of the batch whose candidates in `mask` are poisoned."""
    sel = np.asarray(mask, bool)
    return tuple(np.where(sel.reshape((-1,) + (1,) * (t.ndim - 1)), b, t) for t, b in zip(ref["twin"], ref["bad"]))


# ---- which lanes a launch's candidates share (no device: what the library's two debug calls report) ----------------------------
def template_args(name):
    """('rollout_planar_kernel', ['8', '2', '1', '-3', ...]) of an instantiation's demangled name."""
    mt = re.search(r"(rollout\w*)<([^>]*)>", name)
    assert mt, name
    return mt.group(1), [a.strip() for a in mt.group(2).split(",")]


def launch_layout(choice):
    """dict(kernel, lps, dpp, per_lane, cpw) of an mbd_debug_rollout_choice result: the lane-group width, whether parent and
    child talk through DPP row shifts (the first shift D0 != 0), candidates per lane, candidates per wavefront (0: filled)."""
    kernel, args = template_args(choice["name"])
    if "pk2" in kernel:
        return dict(kernel=kernel, lps=16, dpp=True, per_lane=2, cpw=0)
    lps = int(args[0])
    d0 = int(args[2]) if "planar" in kernel else int(args[5])
    return dict(kernel=kernel, lps=lps, dpp=d0 != 0, per_lane=1, cpw=int(choice["cpw"]))


def rows_of(layout, B):
    """The candidates whose lanes make up each 16-lane row of the launch, [[b, ...], ...] (tail groups repeat B - 1; the
    groups beyond cpw of an early-out launch repeat the wavefront's own candidates), and the same per lane for pk2."""
    lps, cpw = layout["lps"], layout["cpw"]
    if layout["per_lane"] == 2:
        return [[min(2 * r, B - 1), min(2 * r + 1, B - 1)] for r in range((B + 1) // 2)]
    spw = 64 // lps
    k = cpw if cpw > 0 else spw
    rows = []
    for w in range((B + k - 1) // k):
        first = w * k
        cand = []
        for g in range(spw):
            b = first + ((g & (cpw - 1)) if cpw > 0 else g)
            cand.append(b if b < B else (first if cpw > 0 else B - 1))
        gpr = 16 // lps  # lane groups per row
        rows += [cand[i:i + gpr] for i in range(0, spw, gpr)]
    return rows


def sharing(layout, B, mask, plan_N=0):
    """The kinds of sharing (module docstring) between a healthy and a poisoned candidate that the launch contains; with
    plan_N > 0, `mask` marks the candidates of the poisoned PLAN and 'row' / 'lane' mean a plan boundary inside one."""
    mask = np.asarray(mask, bool)
    kinds = set()
    mixed = [r for r in rows_of(layout, B) if len({bool(mask[b]) for b in r}) == 2]
    if layout["per_lane"] == 2:
        if mixed:
            kinds.add("lane")
    elif layout["lps"] < 16 and layout["dpp"] and mixed:
        kinds.add("row")
    rows = rows_of(layout, B)
    for w in range(0, len(rows), 4):  # (a wavefront is four rows)
        if len({bool(mask[b]) for r in rows[w:w + 4] for b in r}) == 2:
            kinds.add("wave")
    return kinds


def closest(kinds):
    """The closest of a set of kinds of sharing: a row, a lane, a wavefront, or "none"."""
    return next((k for k in ("row", "lane", "wave") if k in kinds), "none")


# What the lone poisoned candidate B - 1 of the `last` pattern may share with a healthy candidate in a launch of each kind: it
# sits beside its own tail copies (the other half of its lane in a two-per-lane kernel, the other lane groups of its row and
# of its wavefront where B leaves them free), so it shares what the launch's kind says or less, never anything closer; which
# one, `sharing` works out from the launch's layout.
NO_CLOSER = {"row": ("row", "wave", "none"), "lane": ("lane", "wave", "none"), "wave": ("wave", "none"), "none": ("none",)}


def first_bad_row(m, t0=T0):
    """The first reward row a candidate poisoned from row t0 on cannot keep finite: t0 — except under the tracking reward
    (MBD_REW_HUMANOIDTRACK = 3, humanoidtrack.py:87-96), which is computed from the INCOMING state of a control step: row t0's
    reward is that of the healthy state row t0 - 1 left."""
    return t0 + 1 if int(m.fields["reward_kind"]) == 3 else t0


# What each (model, kernel family) launch of rollout_matrix() at its batch size is claimed to share between neighbouring
# candidates; tests/test_containment_cases.py derives the same from the library's launch choice and asserts they agree, so a
# change of choose_rollout that moves a case to another layout fails there instead of silently testing less.
#   planar models: DPP row shifts with 4 (LPS 4) or 2 (LPS 8) candidates per row, unless the launch puts ONE candidate on a
#   wavefront ("none": the hopper's and the walker's default at this size, MBD_CPW=1 where an early-out instantiation exists —
#   the cartpole has none) or exchanges by ds_bpermute (MBD_NO_DPP);  their 3-D twins: the 3-D kernel's LPS 4 / 8 DPP layouts;
#   ant and the humanoids: a row is a candidate, two per lane under MBD_PK2;  the tripod and the crab (ten links, trees that
#   fit no DPP family) and a model with a specification bit: 16 lanes, ds_bpermute.
EXPECT = {}
for _n in PLANAR:
    for _k in ("general", "cpw0", "cpw2", "cpw4", "cpw8"):
        EXPECT[(_n, _k)] = "row"
    EXPECT[(_n, "no_dpp")] = "wave"
    EXPECT[(_n, "cpw1")] = "row" if _n == "cartpole" else "none"
    EXPECT[(_n, "default")] = "row" if _n in ("halfcheetah", "cartpole") else "none"
    EXPECT[(_n + "3d", "default")] = "row"
for _n in HOT3D:
    for _k in ("default", "no_dpp", "general"):
        EXPECT[(_n, _k)] = "wave"
    EXPECT[(_n, "pk2")] = "lane"
EXPECT.update({("halfcheetahCA", "default"): "row", ("humanoidrun", "no_unit"): "wave", ("tripod", "default"): "wave",
               ("crab", "default"): "wave", (SPEC_MODEL[0], "default"): "wave"})

# Sweeps of P = 3 plans, plan 1 poisoned through its start state: (model, kernel family, N, what plans 0 / 2 share with plan 1).
# N = 33 puts a plan boundary inside a DPP row wherever a row holds several candidates; N = 32 aligns plans with rows, lanes and
# (LPS 8: 8 per wavefront) wavefronts — in the planning launches; the FINAL evaluation of a sweep is one launch of P candidates,
# one per plan, so its three candidates share a row whatever N is (with the product-form exchange the N = 32 cases of the
# planar models failed there: `rew_final`).  Odd plans never take a two-per-lane kernel (choose_rollout), so "a plan boundary inside a
# lane" cannot be launched: the N = 33 humanoid and ant sweeps assert that they run one candidate per lane.
SWEEPS = [("halfcheetah", "default", 33, "row"), ("halfcheetah", "default", 32, "none"),
          ("hopper", "default", 33, "none"), ("hopper", "default", 32, "none"),
          ("hopper", "cpw4", 33, "row"), ("hopper", "cpw4", 32, "none"),
          ("cartpole", "default", 33, "row"), ("cartpole", "default", 32, "none"),
          ("ant", "default", 33, "wave"), ("ant", "pk2", 32, "none"),
          ("humanoidrun", "default", 33, "wave"), ("humanoidrun", "pk2", 32, "none")]
SWEEP_P, SWEEP_H, SWEEP_ND = 3, 8, 4
# The sweep whose rollouts accumulate the demo log-density themselves (RolloutParams::lp): humanoidtrack with its demo, whose 50
# rows fix the horizon; N = 33, three diffusion steps.  (model, N, H, Ndiffuse)
DEMO_SWEEP = ("humanoidtrack", 33, 50, 3)


# ---- the sign of a zero ---------------------------------------------------------------------------------------------------------
# The confined exchange adds +0.0f for a child slot that a link does not have where the checker adds nothing, so a link whose
# own contribution is -0.0f sums to +0.0f there.  The cases below are where that could show: the planar models at rest, every
# exactly-zero velocity and quaternion component carrying one sign or the other, on the ground and one metre above it, every
# actuator at +0.0 or -0.0 (one candidate per sign pattern), so the forces and corrections of the childless links are zeros of
# either sign.  (A build of the checker that adds the +0.0f gives the same bits as the checker on these, on every sign pattern
# of the hopper's and the cartpole's zeros, and on every case of tests/state_inputs.py: the sign is lost before any output.)
ZERO_SIGN_MODELS = (("hopper", "default"), ("hopper", "cpw0"), ("walker2d", "cpw0"), ("halfcheetah", "default"), ("cartpole", "default"))
ZERO_SIGN_H = 2


def zero_sign_cases(orc, m):
    """[(tag, state [L][13], actions [2^Nu or 64][ZERO_SIGN_H][Nu])] for model `m`."""
    import itertools
    L, nu = m.n_links, m.act_size()
    z = np.array([0.0, -0.0], np.float32)
    us = np.array(list(itertools.product(z, repeat=nu)), np.float32)
    rng = np.random.default_rng(zlib.crc32(f"zero signs/{L}/{nu}".encode()))
    if len(us) > 64:
        us = us[rng.choice(len(us), 64, replace=False)]
    us = np.repeat(us[:, None, :], ZERO_SIGN_H, axis=1)
    s0 = si.init_state(orc, m)
    pats = [np.zeros(2 * L, int), np.ones(2 * L, int), np.arange(2 * L) % 2, rng.integers(0, 2, 2 * L)]
    for k, pat in enumerate(pats):
        for lift in (0.0, 1.0):
            s = s0.copy()
            for col, sel in ((7, pat[:L]), (9, pat[L:]), (11, pat[:L]), (5, pat[L:])):
                s[:, col] = np.where(s[:, col] == 0, z[sel], s[:, col])
            s[:, 2] += np.float32(lift)
            yield f"signs {k}, {'in the air' if lift else 'on the ground'}", s, us


def lps_of(m):
    """Lanes per candidate of the model's own layouts (the 16-lane instantiations of the specification switches aside)."""
    return 4 if m.n_links <= 4 else 8 if m.n_links <= 8 else 16
