"""-m gpu: a record replaced by a smaller one and then cleared on a live handle, for the eleven records
tests/test_gpu_record_replace.py leaves out (DESIGN.md "Records have one form": every record keeps device buffers that only grow and
host-side shapes beside them, so what a smaller record or a shorter episode runs on was sized by the use before it).  By bit pattern,
for a ``Plan`` and for a ``Sweep`` of P = 3 wherever the sweep has the set call (hopper, N = 80, H = 50, Ndiffuse = 4,
tests/sweep_records_cases.py; zones: tracked ant, N = 16, H = 7; the demo record: car2d for the plan, humanoidtrack for the sweep,
N = 16):

  handle X takes record A — the larger and fuller one — and runs: ``run``, then an episode of (T, K, E) = (4, 2, 2);
  X takes B — smaller and sparser — and runs ``run`` and an episode of (2, 1, 1): it must equal a fresh handle Y that took B alone;
  X is cleared and runs ``run`` and an episode of (5, 2, 3): it must equal a fresh handle that never had the record.

What is compared is the tree of tests/record_lifecycle.py: ``run``'s outputs, ``run_mpc``'s whole dict, every peek, and the episode
logs read through the C entries into oversized buffers — so a log's count that went on from A's instead of restarting shows.  The
reference handles run only the stage they are compared at.

  objective     row weights, effort, rate, actuator weights, prev0 -> effort only
  weighting     rejection + ESS target with bounds -> rejection only
  value         tests/value_inputs.py's widest and deepest net -> its linear net with another scale
  adapt         carry with wide bounds -> another rate, no carry
  zones         tests/zones_inputs.py's table of 16 -> of 1 -> update_zones to another of 3, against a handle set to that table
  ensemble      4 members, min -> 2 members, mean
  mpc pick      mean + prev + best -> mean + best
  mpc sigma     cma-es: a gain with cold > warm -> one sigma; mppi: cold > warm -> one sigma
  mpc plant     another env, action noise and kicks every tick -> the planning env, action noise only (a sweep: per episode, and B
                leaves episode 1 without a record)
  mpc delay     3 ticks with rows0 -> 1 tick without
  mpc demo      the env's demo extended, from row 2 -> its first 20 rows: shorter than c0 + T E + 50, so the clamp to the last row is
                reached; and between the stages a session on the same handle — mpc_open, two ticks, close: the demo record's
                mailbox and single-window path — which must equal a fresh handle's session under B"""
import numpy as np
import pytest

import record_lifecycle as rl
import sweep_records_cases as sc

pytestmark = pytest.mark.gpu
STAGES = ((4, 2, 2), (2, 1, 1), (5, 2, 3))  # (T, K, E) under A, under B — smaller after larger —, after the clear — growing again


@pytest.fixture(scope="module")
def gpu(lib):
    from mbd_hip import _capi
    if _capi.device_count() < 1:
        pytest.fail("tests/test_gpu_record_lifecycle.py needs a GPU")
    return _capi


def _args(name, N, H, demo=False):
    from mbd_hip.planners.mpc import MpcArgs
    return MpcArgs(env_name=name, Nsample=N, Hsample=H, Ndiffuse=sc.ND, temp_sample=0.1, enable_demo=demo, disable_recommended_params=True,
                   not_render=True)


def _hopper(gpu, cls, method=0):
    from mbd_hip.envs import get_env
    return cls(gpu, get_env(sc.NAME), _args(sc.NAME, sc.N, sc.H), method)


@pytest.fixture(scope="module", params=rl.KINDS, ids=("plan", "sweep"))
def kind(request, gpu):
    return _hopper(gpu, request.param)


@pytest.fixture(scope="module")
def plan_kind(gpu):
    return _hopper(gpu, rl.PlanKind)


def _scaled(kind, **scale):
    from mbd_hip.envs.base import RigidBodyEnv
    return RigidBodyEnv(kind.env.env_name, model=kind.env.sys.scaled(**scale))


def _lifecycle(kind, set_a, set_b, clear, update=None, session=False):
    """``set_a``, ``set_b``, ``clear``, ``update``: functions of a handle.  ``update``: one more step behind B (zones), given as
    (the call on X, the set call of the fresh handle it must equal)."""
    x = kind.make(set_a)
    try:
        kind.everything(x, STAGES[0])
        set_b(x)
        if session:
            got = kind.session(x, STAGES[1][1], STAGES[1][2])
            y = kind.make(set_b)
            try:
                rl.same_tree(got, kind.session(y, STAGES[1][1], STAGES[1][2]), f"{kind.name}: B over A: session")
            finally:
                y.close()
        got = kind.everything(x, STAGES[1])
        y, none = kind.make(set_b), kind.make()
        try:
            ref = kind.everything(y, STAGES[1])
            rl.same_tree(got, ref, f"{kind.name}: B over A")
            # (the comparison says something: B runs, its episode is served, and B shows in what is compared)
            assert not rl.refused(ref["run"]) and not rl.refused(ref["run_mpc"]), ref
            assert rl.differ(ref, kind.everything(none, STAGES[1])), f"{kind.name}: B leaves no mark on anything compared"
        finally:
            rl.closing(y, none)
        if update is not None:
            update[0](x)
            got = kind.everything(x, STAGES[1])
            y = kind.make(update[1])
            try:
                rl.same_tree(got, kind.everything(y, STAGES[1]), f"{kind.name}: updated behind B")
            finally:
                y.close()
        clear(x)
        got = kind.everything(x, STAGES[2])
        y = kind.make()
        try:
            rl.same_tree(got, kind.everything(y, STAGES[2]), f"{kind.name}: cleared")
        finally:
            y.close()
    finally:
        x.close()


def test_objective(kind):
    from mbd_hip.planners.mpc import discount_weights
    Nu = kind.Nu
    prev0 = np.linspace(-0.5, 0.5, Nu).astype(np.float32)
    _lifecycle(kind, lambda h: h.set_objective(discount_weights(sc.H, 0.97, 3.0), effort=0.05, rate=0.5, act_weight=1.0 + np.arange(Nu) % 3, prev0=prev0),
               lambda h: h.set_objective(effort=0.1), lambda h: h.clear_objective())


def test_weighting(kind):
    _lifecycle(kind, lambda h: h.set_weighting(True, 0.3, 0.02, 5.0, 8), lambda h: h.set_weighting(True), lambda h: h.clear_weighting())


def test_value(kind):
    import value_inputs as vi
    big = vi.net(sc.NAME, "S-256-256-256-1", "tanh", rel_xy=True, scale=0.37).value_net()
    linear = vi.net(sc.NAME, "S-1", "relu", rel_xy=False, scale=0.11).value_net()
    _lifecycle(kind, lambda h: h.set_value(big), lambda h: h.set_value(linear), lambda h: h.set_value(None))


def test_adapt(plan_kind):
    _lifecycle(plan_kind, lambda h: h.set_adapt(0.5, 0.125, 8.0, carry=True), lambda h: h.set_adapt(0.25, 0.5, 2.0, carry=False),
               lambda h: h.clear_adapt())


def test_ensemble(plan_kind):
    four = [None, _scaled(plan_kind, mass=1.2), _scaled(plan_kind, friction=0.7), _scaled(plan_kind, mass=0.8, gear=0.9)]
    _lifecycle(plan_kind, lambda h: h.set_ensemble(four, "min"), lambda h: h.set_ensemble(four[:2], "mean"), lambda h: h.clear_ensemble())


def test_mpc_pick(kind):
    _lifecycle(kind, lambda h: h.set_mpc_pick(True, True, True), lambda h: h.set_mpc_pick(True, False, True), lambda h: h.clear_mpc_pick())


@pytest.mark.parametrize("cls", rl.KINDS, ids=("plan", "sweep"))
@pytest.mark.parametrize("method", (1, 2), ids=("mppi", "cma-es"))
def test_mpc_sigma(gpu, cls, method):
    k = _hopper(gpu, cls, method)
    _lifecycle(k, lambda h: h.set_mpc_sigma(1.0, 0.5, 0.9 if method == 2 else 0.0), lambda h: h.set_mpc_sigma(0.7, 0.7),
               lambda h: h.clear_mpc_sigma())


def test_mpc_plant(kind):
    other = _scaled(kind, mass=1.3, friction=0.5, gear=0.8)

    def set_a(h):
        for k in range(rl.P):
            kind.set_plant(h, k, env=other, key=kind.gpu.prng_key(5 + k), act_std=0.3, kick_std=0.5, kick_every=1)

    def set_b(h):
        for k in (0, 2):
            kind.set_plant(h, k, env=None, key=kind.gpu.prng_key(9 + k), act_std=0.2)
        if kind.name == "sweep":
            h.clear_mpc_plant(1)

    _lifecycle(kind, set_a, set_b, kind.clear_plant)


def test_mpc_delay(kind):
    rows0 = np.linspace(-0.4, 0.4, 3 * STAGES[0][2] * kind.Nu).astype(np.float32).reshape(-1, kind.Nu)
    _lifecycle(kind, lambda h: h.set_mpc_delay(3, rows0), lambda h: h.set_mpc_delay(1), lambda h: h.clear_mpc_delay())


@pytest.mark.parametrize("cls", rl.KINDS, ids=("plan", "sweep"))
def test_zones(gpu, cls):
    import zones_inputs as zi
    from mbd_hip.envs import get_env
    name, links, N, H = min((p for p in zi.PLANS if p[0] == "ant"), key=lambda p: p[3])
    env = get_env(name, track=tuple(int(l) for l in links))
    k = cls(gpu, env, _args(name, N, H))
    K = k.Kt
    moved = zi.table(K, 3, seed=1)
    _lifecycle(k, lambda h: h.set_zones(zi.table(K, 16)), lambda h: h.set_zones(zi.table(K, 1)), lambda h: h.clear_zones(),
               update=(lambda h: h.update_zones(moved), lambda h: h.set_zones(moved)))


@pytest.mark.parametrize("cls,name", ((rl.PlanKind, "car2d"), (rl.SweepKind, "humanoidtrack")), ids=("plan-car2d", "sweep-humanoidtrack"))
def test_mpc_demo(gpu, cls, name):
    import mpc_demo_checker as mdc
    from mbd_hip.envs import get_env
    from mbd_hip.envs.base import State
    env = get_env(name)
    states = None
    if name == "car2d":  # (beside the goal region: from its reset state all rewards are equal)
        states = [State(np.array([0.5, 0.5, 0.0], np.float32), None, np.float32(0), np.float32(0), {})] * rl.P
    k = cls(gpu, env, _args(name, 16, mdc.ROWS, demo=True), states=states)
    clip = mdc.as_tracks(mdc.extended(env.xref))
    short = np.ascontiguousarray(clip[:, :20])
    assert short.shape[1] < 0 + STAGES[1][0] * STAGES[1][2] + mdc.ROWS
    _lifecycle(k, lambda h: h.set_mpc_demo(clip, 2), lambda h: h.set_mpc_demo(short, 0), lambda h: h.clear_mpc_demo(), session=True)
