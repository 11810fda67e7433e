"""What tests/test_gpu_record_lifecycle.py and tests/test_gpu_record_pairs.py share: a ``Plan`` or a ``Sweep`` of P = 3 as one kind of
handle; everything a handle can be asked for as one tree — ``run``'s outputs, ``run_mpc``'s whole dict, every peek of the Python
layer, and the episode logs read through the C entries into oversized buffers, so that a log longer than the reference's shows —;
and the comparison of two such trees by bit pattern.  A call the library refuses is a leaf of the tree too (its error code), so a
handle that answers where the reference refuses, or the other way round, differs from it."""
import ctypes as C

import numpy as np

import sweep_records_cases as sc
from state_inputs import same_bits

P = 3
LOG_T, LOG_E = 64, 4  # room of the raw episode logs, in ticks and rows per tick: far above what any test here runs (a log that
                      # went on counting over three stages and a session stays inside, and shows)


def attempt(call):
    """0 where ``call`` is accepted, else the library's error code."""
    from mbd_hip import _capi
    try:
        call()
    except _capi.MbdError as e:
        assert e.code != 0
        return e.code
    return 0


def _or_refusal(call):
    from mbd_hip import _capi
    try:
        return call()
    except _capi.MbdError as e:
        return {"refused": e.code}


def same_tree(got, ref, what):
    """``got`` and ``ref``: dicts, lists, None, arrays and numbers, of the same layout; floats by bit pattern."""
    if isinstance(ref, dict):
        assert isinstance(got, dict) and sorted(got) == sorted(ref), f"{what}: keys {sorted(got) if isinstance(got, dict) else got!r} against {sorted(ref)}"
        for k in ref:
            same_tree(got[k], ref[k], f"{what}: {k}")
    elif isinstance(ref, (list, tuple)):
        assert isinstance(got, (list, tuple)) and len(got) == len(ref), f"{what}: {len(got) if isinstance(got, (list, tuple)) else got!r} entries against {len(ref)}"
        for i, (g, r) in enumerate(zip(got, ref)):
            same_tree(g, r, f"{what}[{i}]")
    elif ref is None:
        assert got is None, f"{what}: {got!r} against None"
    else:
        assert not isinstance(got, (dict, list, tuple)) and got is not None, f"{what}: {got!r} against a value"
        g, r = np.asarray(got), np.asarray(ref)
        assert g.shape == r.shape and g.dtype.kind == r.dtype.kind, f"{what}: {g.dtype}{g.shape} against {r.dtype}{r.shape}"
        if r.dtype.kind == "f":
            same_bits(g, r, what)
        else:
            assert np.array_equal(g, r), f"{what}: {g.tolist()} against {r.tolist()}"


def differ(a, b) -> bool:
    """Whether two trees differ anywhere (a record that changes nothing a test compares would make the test vacuous)."""
    try:
        same_tree(a, b, "")
    except AssertionError:
        return True
    return False


def refused(tree) -> bool:
    return isinstance(tree, dict) and sorted(tree) == ["refused"]


def _raw(fn, *head_and_bufs):
    """A C peek into caller-sized buffers filled with NaN: (return code, the buffers)."""
    head, bufs = [a for a in head_and_bufs if not isinstance(a, np.ndarray)], [a for a in head_and_bufs if isinstance(a, np.ndarray)]
    from mbd_hip import _capi
    rc = fn(*head, *[_capi.np_ptr(b) for b in bufs])
    return dict(rc=int(rc), **{f"out{i}": b for i, b in enumerate(bufs)})


class _Kind:
    """A way to make handles of one configuration — env, args, update method — and to ask them for everything."""

    def __init__(self, gpu, env, a, method=0, states=None):
        self.gpu, self.env, self.a, self.method = gpu, env, a, int(method)
        states_, self.keys, self.temps = sc.inputs(gpu, env, P)
        self.states = states_ if states is None else list(states)
        sys_ = getattr(env, "sys", None)
        self.S, self.Nu = env._state_size, env.action_size
        self.Kt = max(int(sys_.fields["n_track"]), 1) if sys_ is not None else 1
        self.Cc = 3 if sys_ is not None else 2

    def _nan(self, *shape):
        return np.full(shape, np.nan, np.float32)

    def everything(self, h, episode=None):
        """The tree of ``h``: ``run``, then with ``episode`` = (T, K, E) ``run_mpc``, then every peek."""
        out = dict(run=self.run(h))
        if episode is not None:
            out["run_mpc"] = self.run_mpc(h, *episode)
        out["peeks"] = self.peeks(h)
        return out


class PlanKind(_Kind):
    """Plan 0 of the sweep's inputs, alone."""
    name = "plan"

    def make(self, configure=lambda h: None):
        return sc.make_plan(self.env, self.a, self.states[0], self.temps[0], self.method, configure)

    def run(self, h):
        def go():
            mu, rm, rf = h.run(self.keys[0])[:3]
            return dict(mu=mu, rew_means=rm, rew_final=np.float32(rf))
        return _or_refusal(go)

    def run_mpc(self, h, T, K, E):
        def go():
            ep = h.run_mpc(self.keys[0], T, K, E)
            del ep["seconds"]
            return ep
        return _or_refusal(go)

    def session(self, h, K, E, ticks=2):
        """A session of ``ticks`` ticks fed the start state: every tick's rows, mean, head, predicted, flags and pick."""
        out = []
        with h.mpc_open(self.keys[0], K, E) as s:
            for _ in range(ticks):
                t = s.tick(self.states[0])
                out.append({k: t[k] for k in ("rows", "mean", "head", "predicted", "flags", "rew_mean", "tick")} | {"pick": s.pick})
        return out

    def set_plant(self, h, k, **rec):
        if k == 0:
            h.set_mpc_plant(**rec)

    def clear_plant(self, h):
        h.clear_mpc_plant()

    def peeks(self, h):
        lib, p = h.lib, h.h
        out = {n: _or_refusal(getattr(h, "peek_" + n)) for n in ("objective", "weighting", "value", "adapt", "zones", "ensemble", "mpc_pick",
                                                                    "elites", "togo")}
        out["mpc_predicted"] = _raw(lib.mbd_plan_peek_mpc_predicted, p, self._nan(LOG_T, self.S))
        out["mpc_sigma"] = _raw(lib.mbd_plan_peek_mpc_sigma, p, self._nan(LOG_T, 2))
        out["mpc_track"] = _raw(lib.mbd_plan_peek_mpc_track, p, self._nan(LOG_T * LOG_E, self.Kt), self._nan(LOG_T, self.Kt, 50, self.Cc))
        out["mpc_zones"] = _raw(lib.mbd_plan_peek_mpc_zones, p, self._nan(LOG_T * LOG_E), self._nan(LOG_T * LOG_E))
        out["has"] = dict(elites=h.has_elites, togo=h.has_togo, zones=h.has_zones, pick=h.has_mpc_pick(), delay=h._has_delay,
                          sigma=h._has_sigma, demo=h._demo_shape)
        return [out]


class SweepKind(_Kind):
    name = "sweep"

    def make(self, configure=lambda h: None):
        return sc.make_sweep(self.env, self.a, P, self.states, self.temps, self.method, configure)

    def run(self, h):
        def go():
            mu, rm, rf = h.run(self.keys)[:3]
            return dict(mu=mu, rew_means=rm, rew_final=rf)
        return _or_refusal(go)

    def run_mpc(self, h, T, K, E):
        def go():
            ep = h.run_mpc(self.keys, T, K, E)
            del ep["seconds"]
            return ep
        return _or_refusal(go)

    def session(self, h, K, E, ticks=2):
        out = []
        with h.mpc_open(self.keys, K, E) as s:
            for _ in range(ticks):
                t = s.tick(self.states)
                out.append({k: t[k] for k in ("rows", "mean", "head", "predicted", "flags", "rew_mean", "tick")} | {"pick": s.pick})
        return out

    def set_plant(self, h, k, **rec):
        h.set_mpc_plant(k, **rec)

    def clear_plant(self, h):
        for k in range(P):
            h.clear_mpc_plant(k)

    def peeks(self, h):
        lib, p = h.lib, h.h
        outs = []
        for k in range(P):
            out = {n: _or_refusal(lambda n=n: getattr(h, "peek_" + n)(k)) for n in ("objective", "weighting", "zones", "mpc_pick", "elites", "togo")}
            out["mpc_sigma"] = _raw(lib.mbd_sweep_peek_mpc_sigma, p, k, self._nan(LOG_T, 2))
            out["mpc_track"] = _raw(lib.mbd_sweep_peek_mpc_track, p, k, self._nan(LOG_T * LOG_E, self.Kt), self._nan(LOG_T, self.Kt, 50, self.Cc))
            out["mpc_zones"] = _raw(lib.mbd_sweep_peek_mpc_zones, p, k, self._nan(LOG_T * LOG_E), self._nan(LOG_T * LOG_E))
            outs.append(out)
        outs[0]["mpc_predicted"] = _raw(lib.mbd_sweep_peek_mpc_predicted, p, self._nan(P, LOG_T, self.S))
        outs[0]["has"] = dict(elites=h.has_elites, togo=h.has_togo, zones=h.has_zones, pick=h.has_mpc_pick(), delay=h._has_delay,
                              sigma=h._has_sigma, demo=h._demo_shape)
        return outs


KINDS = (PlanKind, SweepKind)


def closing(*handles):
    for h in handles:
        if h is not None:
            h.close()
