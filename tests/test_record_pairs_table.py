"""On the CPU: the table of tests/test_gpu_record_pairs.py (tests/record_pairs_table.py) leaves no pair of records out — for a
``Plan`` the pairs it exercises plus the pairs it lists as impossible are all C(15, 2) = 105, for a ``Sweep`` all C(13, 2) = 78 —,
lists a pair as impossible exactly where no configuration holds both records, names for it a configuration that holds the other
record and not the refused one, and has an instance and a refused instance of every record."""
import math

import record_pairs_table as rp


def test_records_are_the_set_calls_of_the_python_layer():
    from mbd_hip.planners.mbd_planner import Plan, Sweep
    assert len(rp.RECORDS) == 15 and len(rp.SWEEP_RECORDS) == 13 and len(set(rp.RECORDS)) == 15
    for r in rp.RECORDS:
        assert hasattr(Plan, "set_" + r), r
        assert hasattr(Sweep, "set_" + r) == (r in rp.SWEEP_RECORDS), r
    assert sorted(rp.SET) == sorted(rp.SET_INVALID) == sorted(rp.RECORDS)


def test_no_pair_is_left_out():
    for kind, n in (("plan", 15), ("sweep", 13)):
        pairs = rp.pairs_of(kind)
        ex, im = rp.exercised(kind), rp.impossible(kind)
        assert len(pairs) == math.comb(n, 2) == len(ex) + len(im), kind
        assert {(a, b) for a, b, _ in ex} | {(a, b) for a, b, *_ in im} == set(pairs) and not {(a, b) for a, b, _ in ex} & {(a, b) for a, b, *_ in im}
    assert (len(rp.exercised("plan")), len(rp.impossible("plan"))) == (96, 9)
    assert (len(rp.exercised("sweep")), len(rp.impossible("sweep"))) == (72, 6)


def test_impossible_pairs_are_those_no_configuration_holds():
    order = {r: i for i, r in enumerate(rp.RECORDS)}
    assert set(rp.IMPOSSIBLE) == {p for p in rp.pairs_of("plan") if rp.config_of(*p) is None}
    for (a, b), (cfg, refused, code, why) in rp.IMPOSSIBLE.items():
        assert order[a] < order[b] and cfg in rp.CONFIGS and refused in (a, b) and why
        other = b if refused == a else a
        assert other in rp.HOLDS[cfg] and refused not in rp.HOLDS[cfg], (a, b)
        assert code in (rp.UNSUPPORTED, rp.STATE)


def test_refused_pairs_lie_in_a_configuration_and_configurations_hold_known_records():
    order = {r: i for i, r in enumerate(rp.RECORDS)}
    for (a, b), codes in rp.REFUSED.items():
        assert order[a] < order[b] and rp.config_of(a, b) is not None and len(codes) == 2, (a, b)
    assert set(rp.HOLDS) == set(rp.CONFIGS) and all(h <= set(rp.RECORDS) for h in rp.HOLDS.values())
    assert set().union(*rp.HOLDS.values()) == set(rp.RECORDS), "every record runs in some configuration"
    from mbd_hip import _capi
    assert (rp.INVALID, rp.UNSUPPORTED, rp.STATE) == (_capi.MBD_ERR_INVALID, _capi.MBD_ERR_UNSUPPORTED, _capi.MBD_ERR_STATE)
