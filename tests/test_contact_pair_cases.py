"""On the CPU: the start states of tests/contact_pair_inputs.py reach the cases of stage (4) they are named after — in the
checker alone, by replaying the stage from the checker's own stage dump and holding the replay to the dump bit for bit.
tests/test_gpu_contact_pairs.py runs the same states through the rollout kernels."""
import numpy as np
import pytest

import contact_pair_inputs as cp

MODELS = ("humanoidrun", "humanoidtrack", "generic", "frames5")


@pytest.mark.parametrize("name", MODELS)
def test_every_case_is_reached_in_the_first_substep(orc, name):
    m, _ = cp.variant(name)
    ms = m.to_struct()
    seen = set()
    for case, q, qd in cp.cases(name):
        s0 = orc.forward(ms, q, qd)
        first = cp.census(orc, m, s0, np.zeros((1, 1, m.act_size()), np.float32))[0][0]
        for slot, pred in enumerate(cp.EXPECT[case]):
            assert pred(first[slot]), f"{name} {case}: collider {slot} gives {first[slot]}"
        seen.add(case)
    assert seen == set(cp.EXPECT)


def test_replay_is_the_checkers_stage_4_along_whole_rollouts(orc):
    """Every substep of the short rollouts the GPU tests run (all candidates, random actions): census() asserts that the
    replayed positions after stage (4) are the checker's, and along the way both sides of the friction test and both
    contact flags turn up on one link."""
    m, _ = cp.variant("humanoidrun")
    ms = m.to_struct()
    kinds = set()
    for case, q, qd in cp.cases("humanoidrun"):
        for per in cp.census(orc, m, orc.forward(ms, q, qd), cp.actions(m, 5, 3)):
            for recs in per:
                kinds |= {(r["active"], r["stick"]) for r in recs}
    assert kinds == {(False, None), (True, True), (True, False)}
