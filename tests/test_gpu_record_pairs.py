"""-m gpu: the order of set calls, the symmetry of the refusals between records, and what a refused set call leaves behind — for every
unordered pair of the fifteen records a ``Plan`` takes and of the thirteen a ``Sweep`` (P = 3) takes, and for every record an invalid
record over a valid one.  tests/record_pairs_table.py has one small instance per record, the three configurations and which pair runs
in which; tests/test_record_pairs_table.py holds its completeness without a device (105 = 96 exercised + 9 impossible pairs for
plans, 78 = 72 + 6 for sweeps).  By bit pattern; the reference is never the handle under test but a fresh handle that took one
record alone, whose tree — ``run``, ``run_mpc`` with (T, K, E) = (3, 2, 1), every peek, the ``has_*`` properties; a refused call is its
error code (tests/record_lifecycle.py) — is computed once per record and configuration.

  a pair {A, B}     handle 1: set(A); set(B).  handle 2: set(B); set(A).  Both second calls are accepted or both are refused.
     accepted       handles 1 and 2 have the same tree.
     refused        each handle has the tree of a fresh handle with its first record alone; the codes are those of the table
                    (today's answer: MBD_ERR_UNSUPPORTED, for ensemble <-> value MBD_ERR_STATE, in both orders), and exactly the pairs
                    the table lists are refused.
  impossible        the configuration refuses one record R of the pair wherever it comes: set(O); set(R) and set(R); set(O) both
                    refuse R with the listed code, and both handles have the tree of a fresh handle with O alone.
  invalid on valid  set(A), run, a record of A's kind that its check refuses (MBD_ERR_INVALID), run: the tree of a fresh handle with
                    A alone — the old record stays in force, untouched."""
import pytest

import record_lifecycle as rl
import record_pairs_table as rp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(lib):
    from mbd_hip import _capi
    if _capi.device_count() < 1:
        pytest.fail("tests/test_gpu_record_pairs.py needs a GPU")
    return _capi


_KINDS, _ALONE = {}, {}


def _kind(gpu, kind, config):
    """The handle factory of a kind ("plan" / "sweep") in a configuration, made once."""
    if (kind, config) not in _KINDS:
        from mbd_hip.envs import get_env
        from mbd_hip.planners.mpc import MpcArgs
        c = rp.CONFIGS[config]
        env = get_env(c["env"]) if c["track"] is None else get_env(c["env"], track=list(c["track"]))
        a = MpcArgs(env_name=c["env"], Nsample=c["N"], Hsample=c["H"], Ndiffuse=c["Nd"], temp_sample=0.1, enable_demo=c["demo"],
                    disable_recommended_params=True, not_render=True)
        _KINDS[kind, config] = (rl.PlanKind if kind == "plan" else rl.SweepKind)(gpu, env, a, c["method"])
    return _KINDS[kind, config]


def _tree(k, h):
    return k.everything(h, rp.EPISODE)


def _alone(gpu, kind, config, record):
    """The tree of a fresh handle that took ``record`` alone (None: no record), computed once and left unchanged."""
    key = (kind, config, record)
    if key not in _ALONE:
        k = _kind(gpu, kind, config)
        h = k.make()
        try:
            if record is not None:
                rp.SET[record](h, k)
            _ALONE[key] = t = _tree(k, h)
        finally:
            h.close()
        # an episode is refused exactly where the configuration needs a record for one: a demo handle without a demo record, a
        # path-integral handle without a sigma record
        needs = {"demo": "mpc_demo", "pi": "mpc_sigma"}.get(config)
        assert not rl.refused(t["run"]) and rl.refused(t["run_mpc"]) == (needs is not None and record != needs), (key, t["run_mpc"])
    return _ALONE[key]


def _params(table):
    return [pytest.param(kind, *row, id=f"{kind}-{row[0]}-{row[1]}") for kind in ("plan", "sweep") for row in table(kind)]


def test_the_module_exercises_or_lists_every_pair():
    for kind, n in (("plan", 105), ("sweep", 78)):
        ex, im = {(a, b) for a, b, _ in rp.exercised(kind)}, {(a, b) for a, b, *_ in rp.impossible(kind)}
        assert len(ex) + len(im) == n == len(rp.pairs_of(kind)) and not ex & im and ex | im == set(rp.pairs_of(kind))


@pytest.mark.parametrize("kind", ("plan", "sweep"))
def test_every_record_shows_in_what_is_compared(gpu, kind):
    """A record's tree differs from the tree of a handle without records, in every configuration that holds it: no comparison
    below is between handles on which the records make no difference.  (Where a configuration serves no episode without its own
    record — demo, sigma — only that record is asked here; the others run there beside it, and test_pair_in_both_orders asks
    that the pair differs from each of its records alone.)"""
    for config, holds in rp.HOLDS.items():
        needs = {"demo": "mpc_demo", "pi": "mpc_sigma"}.get(config)
        for record in rp.records_of(kind):
            if record in holds and needs in (None, record):
                assert rl.differ(_alone(gpu, kind, config, record), _alone(gpu, kind, config, None)), (kind, config, record)


@pytest.mark.parametrize("kind,a,b,config", _params(rp.exercised))
def test_pair_in_both_orders(gpu, kind, a, b, config):
    k = _kind(gpu, kind, config)
    h1, h2 = k.make(), k.make()
    try:
        rp.SET[a](h1, k)
        rp.SET[b](h2, k)
        rc_b, rc_a = rl.attempt(lambda: rp.SET[b](h1, k)), rl.attempt(lambda: rp.SET[a](h2, k))
        assert (rc_b == 0) == (rc_a == 0), f"{a} then {b}: {rc_b}; {b} then {a}: {rc_a}: refused in one order only"
        assert ((a, b) in rp.REFUSED) == (rc_b != 0), f"{a} <-> {b}: codes {rc_b}, {rc_a}, the table says {rp.REFUSED.get((a, b), 'accepted')}"
        if rc_b == 0:
            t1 = _tree(k, h1)
            rl.same_tree(t1, _tree(k, h2), f"{kind}: {a} then {b} against {b} then {a}")
            for alone in (a, b):  # (both records are in force: neither call displaced the other's record)
                assert rl.differ(t1, _alone(gpu, kind, config, alone)), f"{kind}: {a} and {b} equal {alone} alone"
        else:
            assert (rc_b, rc_a) == rp.REFUSED[a, b]
            rl.same_tree(_tree(k, h1), _alone(gpu, kind, config, a), f"{kind}: {a}, {b} refused, against {a} alone")
            rl.same_tree(_tree(k, h2), _alone(gpu, kind, config, b), f"{kind}: {b}, {a} refused, against {b} alone")
    finally:
        rl.closing(h1, h2)


@pytest.mark.parametrize("kind,a,b,config,refused,code,why", _params(rp.impossible))
def test_pair_no_configuration_holds(gpu, kind, a, b, config, refused, code, why):
    k = _kind(gpu, kind, config)
    other = b if refused == a else a
    h1, h2 = k.make(), k.make()
    try:
        rp.SET[other](h1, k)
        assert rl.attempt(lambda: rp.SET[refused](h1, k)) == code, f"{other} then {refused}: {why}"
        assert rl.attempt(lambda: rp.SET[refused](h2, k)) == code, f"{refused} first: {why}"
        rp.SET[other](h2, k)
        ref = _alone(gpu, kind, config, other)
        rl.same_tree(_tree(k, h1), ref, f"{kind}: {other}, {refused} refused, against {other} alone")
        rl.same_tree(_tree(k, h2), ref, f"{kind}: {refused} refused, {other}, against {other} alone")
    finally:
        rl.closing(h1, h2)


@pytest.mark.parametrize("kind,record", [(kind, r) for kind in ("plan", "sweep") for r in rp.records_of(kind)])
def test_invalid_record_over_a_valid_one(gpu, kind, record):
    config = next(c for c, holds in rp.HOLDS.items() if record in holds)
    k = _kind(gpu, kind, config)
    ref = _alone(gpu, kind, config, record)
    h = k.make()
    try:
        rp.SET[record](h, k)
        rl.same_tree(_tree(k, h), ref, f"{kind}: {record}")
        assert rl.attempt(lambda: rp.SET_INVALID[record](h, k)) == rp.INVALID
        rl.same_tree(_tree(k, h), ref, f"{kind}: {record} after an invalid {record}")
    finally:
        h.close()
