"""One family of tests/state_inputs.py through a checker library given by path (the gcov build of oracle/Makefile's `cov`
target), in a process of its own so that the counters are written when it exits.  Started by tests/test_state_coverage.py:

    python state_census_worker.py <liboracle_f32.so> <family> <result.json>

Runs every case of the family on every model of the census — the eight rigid-body envs, the custom models of
state_inputs.CUSTOM and each specification-switch word of state_inputs.SPEC_WORDS — through
orc_rollout (rewards, tracked positions, final states), the first candidate's first step also through orc_env_step, and, in
the family "exact", one substep per model with the stage dump on.  car2d's cases run in the family "exact".  Writes the
counts and the names of the cases with a non-finite value."""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "model-based-diffusion_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def census_models():
    """(label, Model) of every model the census runs."""
    import state_inputs as si
    out = [(n, si.model(n)[0]) for n in si.BUILTIN + si.CUSTOM]
    for name, planar, word in si.SPEC_WORDS:
        out.append((f"{name}{'' if planar is None else '/3d'}/flags={word}", si.model(name, bits=word, planar=planar)[0]))
    return out


def main(lib_path, family, out_path):
    import state_inputs as si
    from oracle.oracle import Oracle
    orc = Oracle(path=lib_path)
    f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
    orc.lib.orc_substep_stages.argtypes = [C.c_void_p, f32p, f32p, f32p, f32p]
    res = dict(family=family, cases=0, candidates=0, nonfinite=[], max_abs=0.0)
    for label, m in census_models():
        ms = m.to_struct()
        base = label.split("/")[0]
        for case, state, us in si.cases(orc, m, name=base, families=(family,)):
            rew, xpos, fin = orc.rollout(ms, state, us, want_xpos=True, want_final=True)
            s1, r1 = orc.env_step(ms, state, us[0, 0])
            if case.endswith("/0"):  # (the planner's call: rewards only)
                assert np.array_equal(orc.rollout(ms, state, us[:1]).view(np.uint32), rew[:1].view(np.uint32))
            ok = np.isfinite(state).all() and all(np.isfinite(a).all() for a in (rew, xpos, fin, s1)) and np.isfinite(r1)
            res["cases"] += 1
            res["candidates"] += us.shape[0]
            if not ok:
                bad = [b for b in range(us.shape[0]) if not (np.isfinite(rew[b]).all() and np.isfinite(fin[b]).all())]
                res["nonfinite"].append(f"{label}: {case}: candidates {bad}")
            else:
                res["max_abs"] = max(res["max_abs"], float(np.abs(fin).max()))
        if family == "exact":
            s = si.init_state(orc, m)
            out, stages = np.zeros_like(s), np.zeros((6,) + s.shape, np.float32)
            orc.lib.orc_substep_stages(C.addressof(ms), s.reshape(-1), np.zeros(max(m.act_size(), 1), np.float32),
                                       out.reshape(-1), stages.reshape(-1))
            if not (np.isfinite(out).all() and np.isfinite(stages).all()):
                res["nonfinite"].append(f"{label}: stage dump")
    if family == "exact":
        for case, q, us in si.car2d_cases():
            rew, qs = orc.car2d_rollout(q, us, want_qs=True)
            res["cases"] += 1
            res["candidates"] += us.shape[0]
            if not (np.isfinite(rew).all() and np.isfinite(qs).all()):
                res["nonfinite"].append(f"car2d: {case}")
    with open(out_path, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main(*sys.argv[1:4])
