"""Inputs of the zone record's tests (tests/test_zones.py on the CPU, tests/test_gpu_zones.py on the device).  numpy and the
checker (tests/zones_checker.py) only; nothing here touches a device.

`crafted(B, H, K, Z, seed)` builds a table of Z zones with positions [B, H, K, 3] and rewards [B] for the launch alone: masks that
leave slots out, every single-axis and two-axis scale, a weight 0 and a radius 0, distances AT r and r + m and at their float
neighbours (from an anchor coordinate at which the difference is exact, as tests/track_inputs.py::_displace does), squares that
overflow and underflow, and — with B > 2 — an inf and a NaN coordinate in row 2, next to clean rows.

`place(orc, model, state0, N, H, seed)` places four zones from a checker rollout of N candidates, the way
tests/track_inputs.py::make_xref places demonstrations: the keep-out centres sit at tracked positions of chosen rows moved by a
seeded offset of the order of radius + margin, the goals lie ahead of the motion; radius and margin are quantiles of the rollout's
own distances, so that the census (`census`) finds every class of term whatever the model and the horizon."""
import numpy as np

import state_inputs as si
import zones_checker as zc

F32 = np.float32
SCALES = [(1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)]
ANCHOR = F32(-0.25)  # a centre coordinate at which ANCHOR + d is a float for the boundary distances below: fl(x - c) = d exactly
KINDS = ("at_r", "below_r", "above_r", "at_rm", "below_rm", "above_rm", "huge", "tiny", "tiny_sq_subnormal", "centre", "inside", "outside")


def zone(kind, center, scale, radius, margin, weight, links):
    return dict(kind=int(kind), center=[float(F32(v)) for v in center], scale=[float(v) for v in scale], radius=float(F32(radius)),
                margin=float(F32(margin)), weight=float(F32(weight)), links=int(links))


def table(K, Z, seed=0):
    """Z zones over K track slots.  Zone 0 is a keep-out sphere and zone 1 a goal slab along x, both centred at (ANCHOR, 0, 0)
    with radius = margin = 0.25, which the crafted rows are built against; the rest cycle through kinds, scales, radii (0 among
    them), margins, weights (0 among them) and masks (one slot; every other slot).  With K >= 3 zone 0 leaves slot 1 out, so that a
    one-zone table has a slot no zone covers."""
    g = np.random.default_rng(si._seed("zones_table", seed, K, Z))
    every = (1 << K) - 1
    out = []
    for i in range(Z):
        if i < 2:
            center = (ANCHOR, 0.0, 0.0)
        else:
            center = (ANCHOR, *g.uniform(-1.0, 1.0, 2))
        if i == 0:
            links = every & ~2 if K >= 3 else every
        elif i % 2:
            links = 1 << (i % K)
        else:
            links = (0x55 << (i // 2 % 2)) & every or every
        out.append(zone(i % 2, center, SCALES[i % len(SCALES)], (0.25, 0.25, 0.0, 0.5)[i % 4], (0.25, 0.25, 0.5, 1.0)[i % 4],
                        0.0 if i == 3 else (1.0, 2.5, 0.75)[i % 3], links))
    return out


def _axes(z):
    return [i for i in range(3) if z["scale"][i] != 0]


def _entry(z, kind, g):
    """A position [3] at a chosen distance from zone z, displaced along the zone's first active axis (the others at the centre)."""
    c = np.asarray(z["center"], F32)
    r, m = F32(z["radius"]), F32(z["margin"])
    rm = F32(r + m)
    ax = _axes(z)[0]
    x = c.copy()
    near = {"at_r": r, "below_r": np.nextafter(r, F32(0)), "above_r": np.nextafter(r, F32(9)), "at_rm": rm,
            "below_rm": np.nextafter(rm, F32(0)), "above_rm": np.nextafter(rm, F32(9))}
    if kind in near:
        x[ax] = F32(c[ax] + near[kind])
    elif kind == "huge":  # every square overflows to +inf
        x = (c + F32(3e19)).astype(F32)
    elif kind in ("tiny", "tiny_sq_subnormal"):  # the squares underflow to 0 / are subnormal floats: on the axes whose centre is 0
        v = F32(1e-30 if kind == "tiny" else 1e-20)
        for i in range(3):
            x[i] = F32(c[i] + v) if c[i] == 0 else c[i]
    elif kind == "centre":
        pass
    else:
        v = g.normal(size=3)
        v /= np.linalg.norm(v)
        length = g.uniform(0.02, 0.98) * float(r) if kind == "inside" else float(rm) + g.uniform(0.05, 2.0)
        x = (c.astype(np.float64) + v * length * (1.0 if kind == "outside" else 1.0)).astype(F32)
    return x


def crafted(B, H, K, Z, seed=0):
    """(zones, xpos [B, H, K, 3], rews [B]).  Row 0: entry (t, k) is of kind KINDS[(t + 5 k) % len(KINDS)] against zone
    (t + k) % min(Z, 2) — the two zones whose centre is the anchor.  The other rows: random positions at U(0, 2) (r + m) from the
    centre of zone (t + k + b) % Z.  With B > 2, row 2 carries +inf in its first entry and a NaN in its last."""
    zones = table(K, Z, seed)
    g = np.random.default_rng(si._seed("zones_crafted", seed, B, H, K, Z))
    xpos = np.zeros((B, H, K, 3), F32)
    for b in range(B):
        for t in range(H):
            for k in range(K):
                if b == 0:
                    z = zones[(t + k) % min(Z, 2)]
                    xpos[b, t, k] = _entry(z, KINDS[(t + 5 * k) % len(KINDS)], g)
                else:
                    z = zones[(t + k + b) % Z]
                    v = g.normal(size=3)
                    v /= np.linalg.norm(v)
                    length = g.uniform(0.0, 2.0) * (z["radius"] + z["margin"])
                    xpos[b, t, k] = (np.asarray(z["center"], np.float64) + v * length).astype(F32)
    if B > 2:
        xpos[2, 0, 0, 0] = F32(np.inf)
        xpos[2, H - 1, K - 1, 1] = F32(np.nan)
    rews = g.normal(size=B).astype(F32)
    rews[0] = F32(-0.0)
    return zones, np.ascontiguousarray(xpos), rews


def boundary_hits(zones, xpos):
    """How many entries of row 0 lie exactly AT r and AT r + m of zones 0 / 1 (the crafted rows are meant to: the tests assert it)."""
    n_r = n_rm = 0
    for z in zones[:2]:
        d = zc.distance(xpos[0], z)
        n_r += int((d == F32(z["radius"])).sum())
        n_rm += int((d == F32(F32(z["radius"]) + F32(z["margin"]))).sum())
    return n_r, n_rm


SIZES = [(B, H, K, Z) for B in (1, 5) for H in (1, 50, 64, 65) for K in (1, 3, 8) for Z in (1, 16)]


# ---- whole plans: zones placed from a checker rollout ---------------------------------------------------------------------------
def place(orc, model, state0, N, H, seed=0):
    """(zones, xpos [N, H, K, 3]): four zones for a plan of N candidates and H rows on ``model`` from ``state0``, placed from the
    checker rollout of N seeded candidates clip(normal, -1, 1) — what a plan's first diffusion step draws around Ybar = 0.
      0  keep-out sphere, every slot: centred at a tracked position of one candidate's late row, moved by a seeded offset
      1  keep-out cylinder (xy), slot 0: likewise, another candidate
      2  goal on the ground plane (xy), slot 0: ahead of the mean motion, with a long margin
      3  goal slab along x, slot 0, same centre: with a margin so short that most terms outside the radius saturate
    radius and margin are quantiles of the rollout's own distances to the centre (keep-out: the 4 % and 15 % quantiles of the
    terms; goals: the radius the tenth of the candidates that stays nearest never leaves), and the
    offset of a keep-out centre is U(0.5, 1.5) times the spread of the candidates' positions in that row — the order of
    radius + margin by construction."""
    ms = model.to_struct()
    K, Nu = int(model.fields["n_track"]), model.act_size()
    g = np.random.default_rng(si._seed("zones_place", seed, N, H, K, *si._key(model)))
    us = np.clip(g.normal(size=(N, H, Nu)), -1.0, 1.0).astype(F32)
    _, xpos = orc.rollout(ms, np.ascontiguousarray(state0, F32), us, want_xpos=True)
    xpos = np.asarray(xpos, F32)
    assert np.isfinite(xpos).all()
    every = (1 << K) - 1
    zones = []
    # the candidates no zone may touch: the tenth that stays nearest to the goals' common centre (slot 0) — every radius below is
    # bounded by THEIR distances, so that the census finds candidates without a penalty by construction
    start = xpos[:, 0, 0].astype(np.float64).mean(axis=0)
    move = xpos[:, H - 1, 0].astype(np.float64).mean(axis=0) - start
    if np.linalg.norm(move[:2]) < 1e-9:
        move = np.array([1.0, 0.0, 0.0])
    ahead = (start + 3.0 * move).astype(F32)  # ahead of the motion
    reach = np.linalg.norm((xpos[:, :, 0].astype(np.float64) - ahead)[..., :2], axis=-1).max(axis=1)
    free = np.argsort(reach)[: max(1, N // 10)]
    others = np.setdiff1d(np.arange(N), free)

    def keep_out(scale, links, slot, t0):
        row = xpos[:, t0, slot].astype(np.float64)
        spread = max(float(np.linalg.norm(row.std(axis=0))), 1e-4)
        v = g.normal(size=3) * np.asarray(scale, np.float64)
        v /= np.linalg.norm(v)
        n0 = int(others[g.integers(others.size)]) if others.size else 0
        c = (row[n0] + v * g.uniform(0.5, 1.5) * spread).astype(F32)
        z = zone(zc.KEEP_OUT, c, scale, 0.0, 1.0, 5.0, links)
        slots = [k for k in range(K) if (links >> k) & 1]
        d = np.stack([zc.distance(xpos[:, :, k], z).astype(np.float64) for k in slots], axis=-1)  # [N, H, slots]
        rm = min(np.quantile(d, 0.15), 0.999 * d[free].min())  # 15 % of the terms come inside r + m, none of the free candidates'
        r = min(np.quantile(d, 0.04), 0.5 * rm)
        return zone(zc.KEEP_OUT, c, scale, r, max(rm - r, 1e-6), 5.0, links)

    zones.append(keep_out((1, 1, 1), every, 0, H - 1))
    zones.append(keep_out((1, 1, 0), 1, 0, max(H // 2, 0)))

    def goal(scale, margin_frac):
        z = zone(zc.GOAL, ahead, scale, 0.0, 1.0, 1.0, 1)
        d = zc.distance(xpos[:, :, 0], z).astype(np.float64)  # [N, H]
        r = 1.0001 * d[free].max()  # the free candidates never leave the radius
        far = max(float(d.max()) - r, 1e-6)
        return zone(zc.GOAL, ahead, scale, r, far * margin_frac, 1.0, 1)

    zones.append(goal((1, 1, 0), 1.5))
    zones.append(goal((1, 0, 0), 0.02))
    return zones, xpos


def census(zones, xpos):
    """dict(zero, inside, saturated: the fractions of the (candidate, step, slot, zone) terms with v == 0, 0 < v < 1, v == 1;
    penalised: the fraction of candidates with a non-zero penalty; free: the number of candidates with none)."""
    v = zc.classes(zones, xpos)
    pen = zc.launch(zones, xpos)["pen"]
    return dict(zero=float((v == 0).mean()), inside=float(((v > 0) & (v < 1)).mean()), saturated=float((v == 1).mean()),
                penalised=float((pen != 0).mean()), free=int((pen == 0).sum()))


def assert_census(c, what=""):
    assert min(c["zero"], c["inside"], c["saturated"]) >= 0.01, f"{what}: a class of terms below 1 %: {c}"
    assert c["penalised"] >= 0.25, f"{what}: fewer than a quarter of the candidates carry a penalty: {c}"
    assert c["free"] >= 1, f"{what}: no candidate without a penalty: {c}"


# the whole-plan cases of tests/test_gpu_zones.py: (model, tracked links — "last": n_links - 1 —, N, H)
PLANS = [("humanoidrun", (0, "last", 5), N, H) for N in (64, 37) for H in (50, 7)] + [("ant", (8, 0, 4), 16, H) for H in (50, 7)]
ND = 4


def plan_model(name, links):
    from conftest import load_model
    m = load_model(name)
    return m.tracked([m.n_links - 1 if l == "last" else int(l) for l in links])
