"""The table behind tests/test_gpu_record_pairs.py, importable without a device (tests/test_record_pairs_table.py checks it there):
the fifteen records a ``Plan`` takes and the thirteen a ``Sweep`` takes, one small instance of each, the three configurations the
pairs run in — no single one takes every record: zones need tracked links on the 3-D arithmetic, a sigma record a path-integral
method, a demo record ``enable_demo`` —, which records each configuration holds, the pairs no configuration holds (a record the
configuration itself refuses, whatever came before it), and the pairs the set calls refuse between each other, with today's codes."""
import itertools

import numpy as np

RECORDS = ("objective", "weighting", "value", "adapt", "elites", "togo", "zones", "ensemble", "noise_shape", "noise_basis",
           "mpc_pick", "mpc_sigma", "mpc_plant", "mpc_delay", "mpc_demo")
PLAN_ONLY = ("adapt", "ensemble")
SWEEP_RECORDS = tuple(r for r in RECORDS if r not in PLAN_ONLY)
EPISODE = (3, 2, 1)  # (T, K, E) of the episodes

INVALID, UNSUPPORTED, STATE = -1, -2, -5  # mbd_hip._capi.MBD_ERR_*

# env, tracked links (tests/zones_inputs.py PLANS: the smallest tracked model; None: the env's own), N, H, Ndiffuse, update method
# (0 MBD, 1 mppi), enable_demo
CONFIGS = {
    "tracked": dict(env="ant", track=(8, 0, 4), N=16, H=7, Nd=4, method=0, demo=False),
    "pi": dict(env="ant", track=(8, 0, 4), N=16, H=7, Nd=4, method=1, demo=False),
    "demo": dict(env="humanoidtrack", track=None, N=16, H=50, Nd=4, method=0, demo=True),
}
HOLDS = {
    "tracked": frozenset(RECORDS) - {"mpc_sigma", "mpc_demo"},
    "pi": frozenset(RECORDS) - {"ensemble", "mpc_demo"},
    "demo": frozenset({"objective", "value", "noise_shape", "noise_basis", "mpc_plant", "mpc_delay", "mpc_demo"}),
}

# pairs no configuration holds: pair -> (the configuration the refusal is asserted in, the record it refuses, the code, why)
_NO_DEMO = "demo records need enable_demo, and a plan created with enable_demo takes no %s record"
IMPOSSIBLE = {
    ("weighting", "mpc_demo"): ("demo", "weighting", UNSUPPORTED, _NO_DEMO % "weighting"),
    ("adapt", "mpc_demo"): ("demo", "adapt", UNSUPPORTED, _NO_DEMO % "adapt"),
    ("elites", "mpc_demo"): ("demo", "elites", UNSUPPORTED, _NO_DEMO % "elite"),
    ("togo", "mpc_demo"): ("demo", "togo", UNSUPPORTED, _NO_DEMO % "to-go"),
    ("zones", "mpc_demo"): ("demo", "zones", UNSUPPORTED, _NO_DEMO % "zone"),
    ("ensemble", "mpc_demo"): ("demo", "ensemble", UNSUPPORTED, _NO_DEMO % "ensemble"),
    ("mpc_pick", "mpc_demo"): ("demo", "mpc_pick", UNSUPPORTED, _NO_DEMO % "pick"),
    ("mpc_sigma", "mpc_demo"): ("demo", "mpc_sigma", STATE, "a handle with demos and a path-integral method cannot be created; an MBD one takes no sigma record"),
    ("ensemble", "mpc_sigma"): ("pi", "ensemble", UNSUPPORTED, "sigma records need a path-integral method, ensembles score MBD plans only"),
}

# pairs the set calls refuse between each other (include/mbd_hip.h, each record's contract): pair -> (the code where the second of
# the pair comes second, the code where the first comes second).  Every other pair a configuration holds is accepted in both orders.
REFUSED = {
    ("objective", "togo"): (UNSUPPORTED, UNSUPPORTED),
    ("weighting", "togo"): (UNSUPPORTED, UNSUPPORTED),
    ("value", "togo"): (UNSUPPORTED, UNSUPPORTED),
    ("adapt", "togo"): (UNSUPPORTED, UNSUPPORTED),
    ("togo", "ensemble"): (UNSUPPORTED, UNSUPPORTED),
    ("togo", "zones"): (UNSUPPORTED, UNSUPPORTED),
    ("zones", "ensemble"): (UNSUPPORTED, UNSUPPORTED),
    ("zones", "mpc_pick"): (UNSUPPORTED, UNSUPPORTED),
    ("ensemble", "mpc_pick"): (UNSUPPORTED, UNSUPPORTED),
    ("value", "ensemble"): (STATE, STATE),  # (MBD_ERR_STATE in both orders, where the other refusals say MBD_ERR_UNSUPPORTED)
}


def records_of(kind):
    return RECORDS if kind == "plan" else SWEEP_RECORDS


def pairs_of(kind):
    """Every unordered pair of the kind's records, in RECORDS' order."""
    return list(itertools.combinations(records_of(kind), 2))


def config_of(a, b):
    """The first configuration that holds both records, or None."""
    for name, holds in HOLDS.items():
        if a in holds and b in holds:
            return name
    return None


def exercised(kind):
    return [(a, b, config_of(a, b)) for a, b in pairs_of(kind) if config_of(a, b) is not None]


def impossible(kind):
    return [(a, b) + IMPOSSIBLE[(a, b)] for a, b in pairs_of(kind) if config_of(a, b) is None]


def refused(kind):
    return {p: c for p, c in REFUSED.items() if p[0] in records_of(kind) and p[1] in records_of(kind)}


# ---- one instance per record, and one record that check_* refuses ----------------------------------------------------------------
# Each is a function of (handle, kind): kind is a tests/record_lifecycle.py kind, which knows the env, its sizes and the handle's
# episodes (a sweep's plant record goes to every episode, each with its own key).

def _rng(name):
    import zlib
    return np.random.default_rng(zlib.crc32(name.encode()))


def _plant_env(kind):
    if getattr(kind, "_plant", None) is None:
        from mbd_hip.envs.base import RigidBodyEnv
        kind._plant = RigidBodyEnv(kind.env.env_name, model=kind.env.sys.scaled(mass=1.3, friction=0.5, gear=0.8))
    return kind._plant


def _member_env(kind):
    if getattr(kind, "_member", None) is None:
        from mbd_hip.envs.base import RigidBodyEnv
        kind._member = RigidBodyEnv(kind.env.env_name, model=kind.env.sys.scaled(mass=1.2))
    return kind._member


def _value_net(kind, scale=0.2):
    from mbd_hip.planners.value import ValueNet
    g, S = _rng("value"), kind.S
    W = [(g.normal(size=(3, S)) / np.sqrt(S)).astype(np.float32), g.normal(size=(1, 3)).astype(np.float32)]
    b = [g.normal(size=3).astype(np.float32) * np.float32(0.1), np.zeros(1, np.float32)]
    return ValueNet(W, b, "tanh", scale=scale)


def _objective(h, kind, effort=0.05):
    from mbd_hip.planners.mpc import discount_weights
    prev0 = (np.arange(kind.Nu, dtype=np.float32) - np.float32(kind.Nu / 2)) / np.float32(4 * kind.Nu)
    h.set_objective(row_weight=discount_weights(h.H, 0.9, 2.0), effort=effort, rate=0.25, act_weight=1.0 + np.arange(kind.Nu) % 3, prev0=prev0)


def _noise_table(h, kind):
    return 0.5 + np.arange(h.H * kind.Nu, dtype=np.float32).reshape(h.H, kind.Nu) / np.float32(h.H * kind.Nu)


def _zones(h, kind, **over):
    import zones_inputs as zi
    tab = zi.table(kind.Kt, 3)
    h.set_zones([dict(tab[0], **over)] + tab[1:])


def _plant(h, kind, act_std=0.1):
    from record_lifecycle import P
    for k in range(P):
        kind.set_plant(h, k, env=_plant_env(kind), key=kind.gpu.prng_key(7 + k), act_std=act_std, kick_std=0.3, kick_every=2)


def _demo(h, kind, start_row=2):
    import mpc_demo_checker as mdc
    h.set_mpc_demo(mdc.extended(kind.env.xref), start_row)


def _knots(h, kind, bad=False):
    from mbd_hip.planners.mpc import knot_basis
    W = knot_basis(h.H, 3, "linear")
    if bad:
        W[1, 1] = np.nan
    h.set_noise_basis(W, "warm")


def _bad_shape(h, kind):
    g = _noise_table(h, kind)
    g[0, 0] = np.nan
    h.set_noise_shape(g, "always")


def _bad_ensemble(h, kind):
    import ctypes as C

    from mbd_hip import _capi
    rec = _capi.Ensemble()
    rec.n_members = 0
    _capi.check(h.lib.mbd_plan_set_ensemble(h.h, C.byref(rec)))


SET = {
    "objective": _objective,
    "weighting": lambda h, kind: h.set_weighting(True, 0.3, 0.02, 5.0, 8),
    "value": lambda h, kind: h.set_value(_value_net(kind)),
    "adapt": lambda h, kind: h.set_adapt(0.5, 0.5, 2.0, True),
    "elites": lambda h, kind: h.set_elites(3, nominal=True),
    "togo": lambda h, kind: h.set_togo(2, 2),
    "zones": _zones,
    "ensemble": lambda h, kind: h.set_ensemble([None, _member_env(kind)], "min"),
    "noise_shape": lambda h, kind: h.set_noise_shape(_noise_table(h, kind), "always"),
    "noise_basis": _knots,
    "mpc_pick": lambda h, kind: h.set_mpc_pick(True, True, True),
    "mpc_sigma": lambda h, kind: h.set_mpc_sigma(1.0, 0.5),
    "mpc_plant": _plant,
    "mpc_delay": lambda h, kind: h.set_mpc_delay(1, np.full((EPISODE[2], kind.Nu), 0.25, np.float32)),
    "mpc_demo": _demo,
}

# a record of each kind that the record's own check refuses (MBD_ERR_INVALID naming the field; the CPU modules list these)
SET_INVALID = {
    "objective": lambda h, kind: _objective(h, kind, effort=-1.0),
    "weighting": lambda h, kind: h.set_weighting(True, 1.5, 0.02, 5.0, 8),
    "value": lambda h, kind: h.set_value(_value_net(kind), float("nan")),
    "adapt": lambda h, kind: h.set_adapt(0.0, 0.5, 2.0, True),
    "elites": lambda h, kind: h.set_elites(0, nominal=False),
    "togo": lambda h, kind: h.set_togo(0, 2),
    "zones": lambda h, kind: _zones(h, kind, links=1 << kind.Kt),
    "ensemble": _bad_ensemble,
    "noise_shape": _bad_shape,
    "noise_basis": lambda h, kind: _knots(h, kind, bad=True),
    "mpc_pick": lambda h, kind: h.set_mpc_pick(False, False, False),
    "mpc_sigma": lambda h, kind: h.set_mpc_sigma(-1.0, 0.5),
    "mpc_plant": lambda h, kind: _plant(h, kind, act_std=-1.0),
    "mpc_delay": lambda h, kind: h.set_mpc_delay(9),
    "mpc_demo": lambda h, kind: _demo(h, kind, start_row=-1),
}
