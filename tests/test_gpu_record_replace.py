"""-m gpu: a record replaced on a live handle by one of another size (elites, to-go, noise basis, noise shape; DESIGN.md "Records
have one form"): a set call grows its buffers and never shrinks them, so the record it leaves must not keep rows, groups, knots or
strides of the one before.  By bit pattern, once for a ``Plan`` and once for a ``Sweep`` of the sizes of tests/sweep_records_cases.py
(hopper, N = 80, H = 50, Ndiffuse = 4, P = 3):

  handle X is given record A, runs, and is then given record B (and, where the case has one, C);
  a fresh handle Y is given B (C) alone;
  ``run`` of X and Y must agree — for the noise records ``run_mpc`` with T = 3, K = 2, E = 1 as well — and so must the records' peeks.

  elites        (5, nominal False) -> (2, nominal True) -> (0, nominal True)
  to-go         (block 10, min_tail 5) -> (1, 1) -> (10, 5)
  noise basis   8 knots in warm ticks -> 3 knots always
  noise shape   a table always -> another table in warm ticks"""
import numpy as np
import pytest

import sweep_records_cases as sc
from state_inputs import same_bits
from test_gpu_noise_shape import _env

pytestmark = pytest.mark.gpu
P, T, K, E = 3, 3, 2, 1


@pytest.fixture(scope="module")
def gpu(lib):
    from mbd_hip import _capi
    if _capi.device_count() < 1:
        pytest.fail("tests/test_gpu_record_replace.py needs a GPU")
    return _capi


class _PlanKind:
    """Plan 0 of the sweep's inputs, alone."""
    name = "plan"

    def __init__(self, gpu, env, a):
        states, keys, temps = sc.inputs(gpu, env, P)
        self.env, self.a, self.state, self.key, self.temp = env, a, states[0], keys[0], temps[0]

    def make(self, configure):
        return sc.make_plan(self.env, self.a, self.state, self.temp, 0, configure)

    def run(self, h):
        mu, rm, rf = h.run(self.key)[:3]
        return dict(mu=mu, rew_means=rm, rew_final=np.float32(rf))

    def run_mpc(self, h):
        return h.run_mpc(self.key, T, K, E)

    def peeks(self, h):
        return [dict(elites=h.peek_elites() if h.has_elites else None, togo=h.peek_togo() if h.has_togo else None)]


class _SweepKind:
    name = "sweep"

    def __init__(self, gpu, env, a):
        self.env, self.a = env, a
        self.states, self.keys, self.temps = sc.inputs(gpu, env, P)

    def make(self, configure):
        return sc.make_sweep(self.env, self.a, P, self.states, self.temps, 0, configure)

    def run(self, h):
        mu, rm, rf = h.run(self.keys)[:3]
        return dict(mu=mu, rew_means=rm, rew_final=rf)

    def run_mpc(self, h):
        return h.run_mpc(self.keys, T, K, E)

    def peeks(self, h):
        return [dict(elites=h.peek_elites(k) if h.has_elites else None, togo=h.peek_togo(k) if h.has_togo else None) for k in range(P)]


@pytest.fixture(scope="module", params=(_PlanKind, _SweepKind), ids=("plan", "sweep"))
def kind(request, gpu):
    return request.param(gpu, _env(sc.NAME), sc.args(sc.NAME, sc.N, sc.H, sc.ND))


def _same_outputs(got, ref, names, what):
    for n in names:
        same_bits(np.asarray(got[n], np.float32), np.asarray(ref[n], np.float32), f"{what}: {n}")


def _same_peeks(got, ref, what):
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert (g["elites"] is None) == (r["elites"] is None) and (g["togo"] is None) == (r["togo"] is None), what
        if r["elites"] is not None:
            sc.same_elites(g["elites"], r["elites"], f"{what}: plan {k}: elites")
        if r["togo"] is not None:
            sc.same_togo(g["togo"], r["togo"], f"{what}: plan {k}: to-go")


def _replace(kind, records, episodes):
    """records: the set calls A, B, ... as functions of a handle.  X takes them one after the other and runs under each; under every
    record but the first it must equal a fresh handle that took that record alone."""
    x = kind.make(records[0])
    try:
        kind.run(x)
        if episodes:
            kind.run_mpc(x)
        for i, rec in enumerate(records[1:], 1):
            what = f"{kind.name}: record {i} over record {i - 1}"
            rec(x)
            got, got_peeks = kind.run(x), kind.peeks(x)
            got_ep = kind.run_mpc(x) if episodes else None
            y = kind.make(rec)
            try:
                ref, ref_peeks = kind.run(y), kind.peeks(y)
                ref_ep = kind.run_mpc(y) if episodes else None
            finally:
                y.close()
            _same_outputs(got, ref, ("mu", "rew_means", "rew_final"), f"{what}: run")
            _same_peeks(got_peeks, ref_peeks, f"{what}: run")
            if episodes:
                _same_outputs(got_ep, ref_ep, ("actions", "rewards", "states", "means"), f"{what}: run_mpc")
    finally:
        x.close()


def test_elites_replaced(kind):
    _replace(kind, [lambda h: h.set_elites(5, nominal=False), lambda h: h.set_elites(2, nominal=True),
                    lambda h: h.set_elites(0, nominal=True)], episodes=False)


def test_togo_replaced(kind):
    _replace(kind, [lambda h: h.set_togo(10, 5), lambda h: h.set_togo(1, 1), lambda h: h.set_togo(10, 5)], episodes=False)


def test_noise_basis_replaced(kind):
    from mbd_hip.planners.mpc import knot_basis
    _replace(kind, [lambda h: h.set_noise_basis(knot_basis(sc.H, 8, "linear"), "warm"),
                    lambda h: h.set_noise_basis(knot_basis(sc.H, 3, "linear"), "always")], episodes=True)


def test_noise_shape_replaced(kind):
    Nu = kind.env.action_size
    g = 0.5 + np.arange(sc.H * Nu, dtype=np.float32).reshape(sc.H, Nu) / (sc.H * Nu)  # [0.5, 1.5): above and below 1
    _replace(kind, [lambda h: h.set_noise_shape(g, "always"), lambda h: h.set_noise_shape(g[::-1].copy() * np.float32(1.25), "warm")],
             episodes=True)
