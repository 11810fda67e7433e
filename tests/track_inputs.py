"""Tracked links and demonstrations beyond humanoidtrack's own five: the shared cases of tests/test_tracks.py (the checker on
the CPU, the library's refusals) and tests/test_gpu_tracks.py (every position-writing rollout instantiation, logpd_track_kernel
at every K, logpd_car2d_kernel, demo plans and a demo record on retracked models, by bit pattern against the checker).  numpy
and the checker only; nothing here touches a device.

`tracked(model, links)` retracks a model; `make_xref(orc, model, state0, seed, offset)` gives it a demonstration
[K][50][3]; `ROWS` is the table of (model, track set, forms), `FORMS` the lever settings of each form and `reaches` whether a
launch (mbd_debug_rollout_choice) is the instantiation a form is meant to reach — the tests assert it, so that the coverage is
checked and not assumed; `crafted(xref, B, seed)` and `crafted_car2d(xref, B, seed)` build positions at chosen distances
from a demonstration for the log-density kernels alone; `terms32` / `contract32` restate the log-density's float32 arithmetic
in numpy, `terms64` / `logpd64` give the float64 reference.
"""
import functools

import numpy as np

import state_inputs as si
from conftest import load_model

H_XREF = 50  # csrc/mbd_kernels.h kXrefRows
MAX_TRACK = 8
F32 = np.float32
BELOW, ABOVE = np.nextafter(F32(0.5), F32(0)), np.nextafter(F32(0.5), F32(1))


def tracked(model, links):
    """A copy of ``model`` that tracks ``links`` (positions in the model), in that order; everything else is shared."""
    from mbd_hip.model import Model
    f = dict(model.fields)
    f["n_track"] = len(links)
    f["track_link"] = np.asarray(list(links), np.int32)
    m = Model(f, model.link_names, model.actuator_names, model.env_name)
    for extra in ("masses", "inertias"):
        if hasattr(model, extra):
            setattr(m, extra, getattr(model, extra))
    return m


def make_xref(orc, model, state0, seed, offset=0.45):
    """[K][50][3] float32: the tracked positions of a 50-step checker rollout from ``state0`` under small random actions, each
    row (k, t) moved by a seeded offset of random direction and length U(0, 2) * ``offset``, every seventh row left where it
    was.  Candidates sampled around the same state stay within centimetres of the rollout for the first control steps and
    within a few decimetres later, so with ``offset`` near 0.5 / 1 their distances fall on both sides of the clip at 0.5 m
    (`census` counts them; the tests assert it)."""
    ms = model.to_struct()
    K = int(model.fields["n_track"])
    g = np.random.default_rng(si._seed("xref", seed, K, *si._key(model)))
    us = np.clip(g.normal(size=(1, H_XREF, model.act_size())) * 0.1, -0.3, 0.3).astype(F32)
    _, xpos = orc.rollout(ms, np.ascontiguousarray(state0, F32), us, want_xpos=True)
    base = xpos[0].transpose(1, 0, 2).astype(np.float64)  # [K][50][3]
    d = g.normal(size=base.shape)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    length = g.uniform(0.0, 2.0, base.shape[:2]) * offset
    length.reshape(-1)[::7] = 0.0
    out = np.ascontiguousarray((base + d * length[..., None]).astype(F32))
    assert np.isfinite(out).all()
    return out


def terms64(xpos, xref):
    """float64 [..., H, K]: (clip(|xpos - xref|, 0, .5) / .5)^2 of float32 positions [..., H, K, 3] against xref [K, H, 3]."""
    x = np.asarray(xpos, np.float64)
    c = np.asarray(xref, np.float64).transpose(1, 0, 2)
    with np.errstate(over="ignore", invalid="ignore"):
        d = np.sqrt(((x - c) ** 2).sum(axis=-1))
        return (np.clip(d, 0.0, 0.5) / 0.5) ** 2


def logpd64(xpos, xref):
    """float64 eval_xref_logpd (humanoidtrack.py:98-106) of float32 inputs: xpos [..., H, K, 3], xref [K, H, 3]."""
    return 0.0 - terms64(xpos, xref).mean(axis=(-1, -2))


def terms64_car2d(qs, xref):
    x = np.asarray(qs, np.float64)[..., :2]
    with np.errstate(over="ignore", invalid="ignore"):
        d = np.sqrt(((x - np.asarray(xref, np.float64)) ** 2).sum(axis=-1))
        return (np.clip(d, 0.0, 0.5) / 0.5) ** 2


def logpd64_car2d(qs, xref):
    """float64 Car2d.eval_xref_logpd (car2d.py:95-102): qs [..., H, 3], xref [H, 2]."""
    return 0.0 - terms64_car2d(qs, xref).mean(axis=-1)


def census(terms):
    """(zero, strictly inside the clip, saturated) counts of an array of terms."""
    t = np.asarray(terms)
    return int((t == 0).sum()), int(((t > 0) & (t < 1)).sum()), int((t == 1).sum())


def chain32(terms_hk):
    """The float32 sum of [H][K] terms as ONE chain in memory order (t outer, k inner) — the order of rounds 1-5, which the
    contract's S_k-then-links order replaced; for showing that a case tells the two apart."""
    acc = F32(0)
    for v in np.asarray(terms_hk, F32).reshape(-1):
        acc = F32(acc + v)
    return acc


def terms32(xpos, xref):
    """float32 [H, K] terms of one candidate, operation by operation as the contract has them: differences, squares and their
    sum left to right, square root, clip, division by 0.5, square — IEEE single arithmetic, which numpy's float32 is."""
    x, c = np.asarray(xpos, F32), np.asarray(xref, F32).transpose(1, 0, 2)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        e = (x - c).astype(F32)
        q = (e * e).astype(F32)
        d = np.sqrt(((q[..., 0] + q[..., 1]).astype(F32) + q[..., 2]).astype(F32)).astype(F32)
        d = np.where(d < 0, F32(0), np.where(d > F32(0.5), F32(0.5), d)).astype(F32)
        sd = (d / F32(0.5)).astype(F32)
        return (sd * sd).astype(F32)


def contract32(terms_hk):
    """The float32 sum of [H][K] terms in the contract's order: link k's H terms in t order (S_k), then S_0 + S_1 + ..."""
    acc = F32(0)
    for k, col in enumerate(np.asarray(terms_hk, F32).T):
        sk = F32(0)
        for v in col:
            sk = F32(sk + v)
        acc = sk if k == 0 else F32(acc + sk)
    return acc


# ---- crafted positions for the log-density kernels alone --------------------------------------------------------------------
# kinds of a crafted entry: the displacement from the demonstration's point
KINDS = ("zero", "below", "half", "above", "huge", "tiny", "tiny_sq_subnormal", "inf", "inside", "outside")
_ANCHOR = F32(-0.25)  # a demo coordinate at which -0.25 + d is a float for every d of BELOW, 0.5, ABOVE: fl(a - c) = d exactly


def _displace(c, kind, g, axes=3):
    """(demo point c' [axes], position a [axes]) of one crafted entry: c with, for the boundary kinds, its x moved to _ANCHOR."""
    c = np.array(c, F32)
    a = c.copy()
    if kind == "zero":
        pass
    elif kind in ("below", "half", "above"):
        d = {"below": BELOW, "half": F32(0.5), "above": ABOVE}[kind]
        c[0] = _ANCHOR
        a = c.copy()
        a[0] = F32(_ANCHOR + d)
        assert F32(a[0] - c[0]) == d  # (exact: both are multiples of 2^-26 below 1/2)
    elif kind == "huge":  # every square overflows to +inf: the term saturates at 1
        a = (c + F32(3e19)).astype(F32)
    elif kind == "tiny":  # every square underflows to 0
        c[:] = 0
        a = np.full(axes, 1e-30, F32)
    elif kind == "tiny_sq_subnormal":  # the squares are subnormal floats (1e-40): a flush to zero would show
        c[:] = 0
        a = np.full(axes, 1e-20, F32)
    elif kind == "inf":
        a[int(g.integers(0, axes))] = F32(np.inf)
    else:
        v = g.normal(size=axes)
        v /= np.linalg.norm(v)
        r = g.uniform(0.01, 0.49) if kind == "inside" else g.uniform(0.55, 3.0)
        a = (c.astype(np.float64) + v * r).astype(F32)
    return c, a


DISTINCT = 6  # candidates of a crafted batch built entry by entry; the rest repeat them with their far entries redrawn


def _fill_rest(x, far, g):
    """Candidates DISTINCT.. of a crafted batch x [B][...][axes]: candidate b % DISTINCT again, its "outside" entries (mask
    ``far`` over one candidate's entries) drawn anew — every candidate differs, at the cost of one vectorised draw."""
    B = x.shape[0]
    for b in range(DISTINCT, B):
        x[b] = x[b % DISTINCT]
    if B > DISTINCT and far.any():
        n, axes = B - DISTINCT, x.shape[-1] if x.shape[-1] == 3 and x.ndim == 4 else 2
        v = g.normal(size=(n, int(far.sum()), axes))
        v *= (g.uniform(0.55, 3.0, v.shape[:2]) / np.linalg.norm(v, axis=-1))[..., None]
        rest = x[DISTINCT:]
        rest[:, far, :axes] = (rest[:, far, :axes].astype(np.float64) + v).astype(F32)  # (from a far point: may come nearer)


def crafted(xref, B, seed):
    """(xref' [K][50][3], xpos [B][50][K][3]) float32 for logpd_track_kernel alone.  Row t of link k of every candidate is of
    kind KINDS[(t + 3 k) % len(KINDS)]; its demo point is shared by all candidates, so the kinds that place the demo point (the
    boundary kinds: x at -0.25; the tiny kinds: the origin) rewrite xref' — the same for every B and seed.  Candidates differ
    in their random entries and in which of their "inside" rows are replaced by exact zeros.  With B >= 2 the LAST candidate is
    the sum-order case: link 0's terms run from 1 down to 1e-10 (distances 0.5 ... 5e-6), every other link's entries are zero
    or inside."""
    xref = np.array(xref, F32)
    K = xref.shape[0]
    g = np.random.default_rng(si._seed("crafted", seed, K, B))
    kind = [[KINDS[(t + 3 * k) % len(KINDS)] for t in range(H_XREF)] for k in range(K)]
    for k in range(K):
        for t in range(H_XREF):
            xref[k, t], _ = _displace(xref[k, t], kind[k][t], g)
    xpos = np.zeros((B, H_XREF, K, 3), F32)
    for b in range(min(B, DISTINCT)):
        for k in range(K):
            for t in range(H_XREF):
                kd = kind[k][t]
                if kd == "inside" and g.random() < 0.3:
                    kd = "zero"
                c, a = _displace(xref[k, t], kd, g)
                assert c.tobytes() == xref[k, t].tobytes()
                xpos[b, t, k] = a
    far = np.array([[kind[k][t] == "outside" for k in range(K)] for t in range(H_XREF)])
    _fill_rest(xpos, far, g)
    if B >= 2:
        lengths = 0.5 * np.sqrt(np.logspace(0, -10, H_XREF))
        for attempt in range(32):  # (until the two orders of the sum give different floats: most draws do)
            for t in range(H_XREF):
                for k in range(K):
                    v = g.normal(size=3)
                    v /= np.linalg.norm(v)
                    r = lengths[t] if k == 0 else (0.0 if t % 4 == 0 else g.uniform(0.05, 0.3))
                    xpos[B - 1, t, k] = (xref[k, t].astype(np.float64) + v * r).astype(F32)
            t32 = terms32(xpos[B - 1], xref)
            if K == 1 or F32(contract32(t32) / F32(K * H_XREF)) != F32(chain32(t32) / F32(K * H_XREF)):
                break
    return np.ascontiguousarray(xref), xpos


def crafted_car2d(xref, B, seed):
    """(xref' [50][2], qs [B][50][3]) for logpd_car2d_kernel alone: the same kinds in the plane (theta random: not read)."""
    xref = np.array(xref, F32)
    g = np.random.default_rng(si._seed("crafted_car2d", seed, B))
    kind = [KINDS[t % len(KINDS)] for t in range(H_XREF)]
    for t in range(H_XREF):
        xref[t], _ = _displace(xref[t], kind[t], g, axes=2)
    qs = np.zeros((B, H_XREF, 3), F32)
    qs[:, :, 2] = g.uniform(-4, 4, (B, H_XREF))
    for b in range(min(B, DISTINCT)):
        for t in range(H_XREF):
            kd = kind[t]
            if kd == "inside" and g.random() < 0.3:
                kd = "zero"
            _, a = _displace(xref[t], kd, g, axes=2)
            qs[b, t, :2] = a
    _fill_rest(qs, np.array([k == "outside" for k in kind]), g)
    return np.ascontiguousarray(xref), qs


# ---- the models, their track sets and the instantiations they are meant to reach --------------------------------------------
# form -> (levers of conftest.levers, flag-word change).  MBD_NO_DPP is read when an env is created: set the levers first.
FORMS = {
    "tuned": ({}, 0),
    "no_helpers": (dict(MBD_NO_HELPERS=1), 0),
    "pk2": (dict(MBD_PK2=1), 0),
    "no_dpp": (dict(MBD_NO_DPP=1), 0),
    "rtib": (dict(MBD_NO_REWARD_CONST=1, MBD_NO_NFR_CONST=1, MBD_NO_UNIT_CONST=1), 0),
    "spec": ({}, 16),  # with_spec(word ^ 16): the specification-switch instantiation
}


def _desc(n, top):
    return list(range(top, top - n, -1))


def _random_links(seed, n_links):
    g = np.random.default_rng(si._seed("tracks", seed))
    return [int(l) for l in g.permutation(n_links)[: int(g.integers(1, 5))]]


@functools.lru_cache(maxsize=None)
def base_model(name):
    """(Model without tracks, env name): built-in models from the compiled assets; the tripod and the crab of
    tests/custom_models.py compiled WITH track_names (so on the 3-D arithmetic: the compiler flags no tracked model planar);
    "random<seed>": tests/random_models.py's 3-D model of that seed."""
    if name in ("tripod", "crab"):
        from custom_models import CRAB, TRIPOD
        from test_oracle_physics import _compile
        if name == "crab":
            m = _compile(CRAB, env_name="hopper", n_frames=3, reset_noise=0.02, reward_params=(1.0, 0.5), track_names=("root", "toe_c"))
            return m, "hopper"
        m = _compile(TRIPOD, env_name="halfcheetah", n_frames=6, reset_noise=0.05, reward_params=(1.0, 0.1), track_names=("torso", "foot_b"))
        assert not si.is_planar(m), "the compiler must not flag a tracked model planar"
        return m, "halfcheetah"
    if name.startswith("random") or name.startswith("small"):
        from random_models import stable_random_model
        from test_random_models import _comp
        if name.startswith("small"):  # "small<max_bodies>_<seed>": at most four links, or at most eight
            mb, seed = (int(x) for x in name[5:].split("_"))
            return stable_random_model(seed, _comp, max_bodies=mb)[1], "hopper"
        return stable_random_model(int(name[6:]), _comp)[1], "hopper"
    return load_model(name), name


def _rows():
    """(id, model, links spec, forms).  A links spec holds positions in the model, "last" for n_links - 1; None: the tracks the
    model was compiled with (track_names); "random": a seeded random set of 1-4 links — both resolved by `row_model`, so that
    importing this module compiles nothing."""
    rows = []

    def add(model, links, forms):
        tag = links if isinstance(links, str) else "own" if links is None else "_".join(map(str, links))
        rows.append((f"{model}-{tag}", model, links if links is None or isinstance(links, str) else tuple(links), tuple(forms)))
    every = ("tuned", "pk2", "no_dpp", "rtib", "spec")
    add("humanoidrun", [0], every)
    add("humanoidrun", ["last"], every)
    add("humanoidrun", ["last", 0, 5], every)
    add("humanoidrun", _desc(8, 10), every)
    add("humanoidtrack", [0], every)
    add("humanoidtrack", [4, 6, 3, 5, 0], every)
    add("humanoidtrack", [9, 0, 5, 3, 6, 4, 1, 10], every)
    # the torso lends its five colliders to the helper lanes; the shins carry the feet's
    add("humanoidstandup", [0, 4, 6], every + ("no_helpers",))
    add("humanoidstandup", _desc(8, 10), every + ("no_helpers",))
    add("ant", [8, 0, 4], every)
    # root and a leaf, from track_names (base_model).  Ten links each: lane groups of 16, and no DPP family fits their trees,
    # so their tuned form IS the shuffle exchange
    add("tripod", None, ("tuned", "spec"))
    add("crab", None, ("tuned", "spec"))
    for seed in range(4):  # (11, 8, 12 and 11 links: lane groups of 16, 8, 16, 16; shuffle exchange)
        add(f"random{seed}", "random", ("tuned",))
    # three links and five: lane groups of 4 and of 8, each on its DPP family and on the shuffle exchange
    add("small3_0", ["last", 0], ("tuned", "no_dpp"))
    add("small6_0", ["last", 0, 2], ("tuned", "no_dpp"))
    return rows


ROWS = _rows()
BUILTIN = ("humanoidrun", "humanoidtrack", "humanoidstandup", "ant")


def row_links(model, links):
    m, _ = base_model(model)
    if links is None:
        return [int(l) for l in np.asarray(m.fields["track_link"])[: int(m.fields["n_track"])]]
    if isinstance(links, str):
        return _random_links(int(model[6:]), m.n_links)  # ("random<seed>")
    return [m.n_links - 1 if l == "last" else int(l) for l in links]


def row_model(model, links):
    """(tracked Model, env name, links) of a table row."""
    m, env_name = base_model(model)
    ls = row_links(model, links)
    return tracked(m, ls), env_name, ls


LANES = {"small3_0": 4, "small6_0": 8, "random1": 8}  # lane groups of the custom rows (every other row: 16)
PK2_MAXCOL = {"humanoidrun": 1, "humanoidtrack": 1, "humanoidstandup": 5, "ant": 2}


def reaches(choice, model, form, m):
    """None where the launch `choice` (mbd_hip._capi.debug_rollout_choice) of table model `model` under `form` is the
    instantiation that form is meant to reach, else what is wrong.  The template arguments of rollout_kernel, by position
    (csrc/mbd_kernels.h): 0 lanes per candidate, 5 DPP exchange, 14 reward kind (-1: read at run time), 15 n_frames (0: read at
    run time), 16 helper lanes, 17 unit inverse inertia compiled in, 18 specification switches honoured at run time;
    rollout_pk2_kernel's first: collider slots per link."""
    import re
    name = choice["name"]
    kernel, args = re.match(r"void mbd::(\w+)<(.*)>\(", name).groups()
    a = [x.strip() for x in args.split(",")]
    rk, nf = str(int(m.fields["reward_kind"])), str(int(m.fields["n_frames"]))
    builtin = model in BUILTIN
    if form == "pk2":
        ok = kernel == "rollout_pk2_kernel" and a[0] == str(PK2_MAXCOL[model])
        return None if ok else f"{model} [pk2]: {name}"
    if kernel != "rollout_kernel" or a[0] != str(LANES.get(model, 16)):
        return f"{model} [{form}]: {name}"
    want = {"tuned": {18: "false"}, "no_helpers": {14: rk, 15: nf, 16: "false", 18: "false"}, "no_dpp": {5: "0", 18: "false"},
            "rtib": {5: "1", 14: "-1", 15: "0", 17: "false", 18: "false"}, "spec": {18: "true"}}[form]
    if form == "tuned" and builtin:
        want = {5: "1", 14: rk, 15: nf, 16: "true" if model == "humanoidstandup" else "false", 18: "false"}
    if form == "tuned" and model in ("small3_0", "small6_0"):
        want = {5: "1", 18: "false"}
    bad = {i: (a[i], v) for i, v in want.items() if a[i] != v}
    return f"{model} [{form}]: template arguments {bad} of {name}" if bad else None


def form_model(m, form):
    word = FORMS[form][1]
    return m.with_spec(int(m.fields.get("flags", 0)) ^ word) if word else m
