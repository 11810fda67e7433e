"""Inputs of the value record's tests (tests/test_value.py, tests/test_gpu_value.py): states and nets.

States: the families of tests/state_inputs.py for hopper and humanoidrun and its car2d cases, cycled to ROWS rows, with rows
holding NaN, +inf, -inf and -0 written over some of them (SPECIAL: row -> what it holds).  Nets: the shapes of SHAPES over an env's
state record, weights drawn so that about half of every hidden layer's pre-activations are positive — the inputs are centred on
the states' medians and scaled by their spreads —, with a few inputs masked (in_scale 0), some weights exactly 0 and some biases
-0, and one input of the first unit scaled up so that tanh nets meet arguments beyond 44.  Everything is seeded."""
import functools
import zlib

import numpy as np

import value_checker as vc

f32 = np.float32
ROWS = 257
ENVS = ("hopper", "humanoidrun", "car2d")
SHAPES = {"S-1": (1,), "S-1-1": (1, 1), "S-3-1": (3, 1), "S-65-64-1": (65, 64, 1), "S-256-256-256-1": (256, 256, 256, 1)}
SPECIAL = {3: "nan", 7: "+inf in x of link 0", 12: "-inf", 19: "-0", 35: "nan everywhere", 256: "+inf last"}


def state_size(name):
    from conftest import load_model
    return 3 if name == "car2d" else load_model(name).n_links * vc.LINK


@functools.lru_cache(maxsize=None)
def healthy_states(name):
    """[ROWS, state_size] finite states of the env."""
    import state_inputs as si
    from oracle.oracle import Oracle
    if name == "car2d":
        rows = [q for _, q, _ in si.car2d_cases()]
    else:
        from conftest import load_model
        m = load_model(name)
        rows = [s.reshape(-1) for _, s, _ in si.cases(Oracle("f32"), m, name, families=("random", "reached", "exact", "contact"))]
    rows = np.stack(rows).astype(f32)
    assert np.isfinite(rows).all()
    return np.resize(rows, (ROWS, rows.shape[1])).copy()


@functools.lru_cache(maxsize=None)
def states(name):
    """healthy_states with the SPECIAL rows written in."""
    s = healthy_states(name).copy()
    S = s.shape[1]
    s[3, S // 2] = np.nan
    s[7, 0] = np.inf
    s[12, S - 1] = -np.inf
    s[19, ::2] = f32(-0.0)
    s[35, :] = np.nan
    s[256, S - 1] = np.inf
    return s


def net(name, shape, act="relu", rel_xy=False, scale=0.37, seed=0):
    """A ``value_checker.Net`` of SHAPES[shape] over env ``name``."""
    h = healthy_states(name)
    S = h.shape[1]
    rng = np.random.default_rng(zlib.crc32(f"{name}/{shape}/{act}/{rel_xy}/{seed}".encode()))
    x = vc.inputs(vc.Net([], [], rel_xy=rel_xy), h)  # (the states as the net sees them, before centre and scale)
    center = np.median(x, axis=0).astype(f32)
    spread = np.maximum(np.abs(x - center).mean(axis=0), 1e-3)
    in_scale = (1.0 / spread).astype(f32)
    masked = rng.choice(S, size=max(1, S // 10), replace=False) if S > 3 else np.array([1])
    in_scale[masked] = 0.0
    hot = int(np.setdiff1d(np.arange(S), masked)[np.argmax(spread[np.setdiff1d(np.arange(S), masked)])])
    in_scale[hot] = f32(in_scale[hot] * 40.0)
    W, b, K = [], [], S
    for l, width in enumerate(SHAPES[shape]):
        w = (rng.normal(size=(width, K)) * (1.5 / np.sqrt(K))).astype(f32)
        w[rng.random(w.shape) < 0.05] = 0.0
        bias = (rng.normal(size=width) * 0.1).astype(f32)
        bias[rng.random(width) < 0.2] = f32(-0.0)
        if width > 1:
            bias[width - 1] = f32(-0.0)
        if l == 0:
            w[:, hot] = (w[:, hot] * f32(0.02)).astype(f32)  # (the scaled-up input drives ...
            w[0, hot] = 2.0                                      # ... the first unit only)
        W.append(w)
        b.append(bias)
        K = width
    return vc.Net(W, b, act, center, in_scale, rel_xy, scale)
