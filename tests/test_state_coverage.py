"""Census: do the start states of tests/state_inputs.py reach the checker's step path?

The float32 checker is built unoptimised with gcov counters into tmp_path (oracle/Makefile, target `cov`; nothing lands in
the tree), every family of state_inputs runs through it in a process of its own (tests/state_census_worker.py: the eight
rigid-body envs, car2d, the custom models and every specification-switch word the GPU suite parametrizes), and `gcov -b`
says which lines ran and which way every branch went.  Asserted:

  * every candidate of every case is finite in the checker (rewards, tracked positions, final states) — no exception;
  * every line of the step path ran: all of mbd_oracle_physics.c but the entry points named in NOT_CALLED, all of
    mbd_oracle_planar.h, every sp_* of spec_math.h that those call;
  * every branch on those lines was taken in each direction;
  * except ALLOWED, one reason per entry, of three admissible kinds: "dump" (the line belongs to the stage dump), "entry"
    (an exported entry point the census does not call), "never" (an argument from the code: no finite state takes it).
    An entry that no longer excuses anything fails the test too: the list cannot go stale.

Printed (-s): per family, what only that family reaches — a family that adds nothing shows as 0.
"""
import json
import os
import shutil
import subprocess
import sys

import pytest

import state_inputs as si
from conftest import ROOT

ORACLE = os.path.join(ROOT, "oracle")
WORKER = os.path.join(ROOT, "tests", "state_census_worker.py")
FILES = ("mbd_oracle_physics.c", "mbd_oracle_planar.h", "spec_math.h")

# exported entry points of mbd_oracle_physics.c outside the step path (kind "entry"): state construction and viewers' helpers
NOT_CALLED = {"orc_forward": "builds start states (forward kinematics); not part of a step",
              "orc_link_positions": "viewer / test helper", "orc_joint_angles": "viewer / test helper",
              "orc_reward": "the reward expressions on caller-given origins (tests/test_ref_golden.py)",
              "orc_real_bytes": "build probe", "orc_model_bytes": "build probe"}
# primitives of spec_math.h that no function of the step path calls (the sampling / softmax side, orc_sp_eval)
NOT_STEP_MATH = {"sp_atan2", "sp_asin", "sp_exp_f32", "sp_log_f32", "sp_log1p_f32", "sp_reduce_sum64", "sp_reduce_max64"}

# (file, function, text the source line contains, what is excused there, kind, reason).  What is excused: "line" (the line never
# runs) or the indices of the branch directions, in gcov's numbering, that are never taken — nothing else on that line, and
# no line of the same text in another function.  Kinds: "dump", "entry", "never".
ALLOWED = [
    ("mbd_oracle_physics.c", "inert_refresh", "if (in->iso || in->world) return;", {2}, "never",
     "branch 2 is `in->world` true.  inert_refresh is only ever called on in[l], l < n_links, whose .world substep() sets to 0 a "
     "few lines before; the world's record world_in is never refreshed: `in->world` is false whenever it is evaluated"),
    ("mbd_oracle_physics.c", "iinv_apply_z0", "if (in->world) { sp_set3(o, 0, 0, 0); return; }", {0}, "never",
     "branch 0 is `in->world` true.  iinv_apply_z0 is only called with &in[l] of a link that carries a collider (stages 4 and "
     "6), never with world_in (iinv_apply's line of the same text IS reached, by joints whose parent is the world)"),
    ("mbd_oracle_physics.c", "reward_origin", "switch (m->reward_kind) {", {6}, "never",
     "branch 6 is the default label.  reward_origin's switch names every reward kind but cartpole's, and env_step — its only "
     "caller on the step path — answers MBD_REW_CARTPOLE itself before it calls reward_origin"),
    ("mbd_oracle_physics.c", "reward_origin", "default: return 0;", {"line"}, "never",
     "the statement of that default label: see the switch"),
]


def _gcov():
    exe = shutil.which("gcov")
    if exe is None:
        return None
    help_ = subprocess.run([exe, "--help"], capture_output=True, text=True).stdout
    return exe if "--json-format" in help_ and "--stdout" in help_ else None


def _coverage(gcov, famdir):
    """{(file, line): (function, executed, [branch counts])} of FILES from the counters in famdir."""
    out = subprocess.run([gcov, "-b", "--json-format", "--stdout", "-o", famdir, os.path.join(famdir, "mbd_oracle_physics.gcda")],
                         capture_output=True, text=True, check=True, cwd=famdir).stdout
    cov = {}
    for doc in (json.loads(l) for l in out.splitlines() if l.strip().startswith("{")):
        for f in doc["files"]:
            name = os.path.basename(f["file"])
            if name not in FILES:
                continue
            for ln in f["lines"]:
                key = (name, int(ln["line_number"]))
                fn, cnt, br = ln.get("function_name", ""), int(ln["count"]), [int(b["count"]) for b in ln.get("branches", [])]
                if key in cov:  # (a line that belongs to two functions: counts add)
                    old = cov[key]
                    br = [a + b for a, b in zip(old[2], br)] if len(old[2]) == len(br) else old[2] + br
                    cnt, fn = cnt + old[1], old[0]
                cov[key] = (fn, cnt, br)
    return cov


def _items(cov):
    """The set of things reached: ("line", file, n) and ("branch", file, n, k)."""
    got = set()
    for (name, n), (_, cnt, br) in cov.items():
        if cnt > 0:
            got.add(("line", name, n))
        got.update(("branch", name, n, k) for k, c in enumerate(br) if c > 0)
    return got


def test_start_states_reach_every_line_and_branch_of_the_step_path(tmp_path):
    gcov = _gcov()
    if gcov is None:
        pytest.skip("gcov with --json-format is not installed: the census of tests/state_inputs.py did not run")
    build = tmp_path / "cov"
    subprocess.run(["make", "-s", "-C", ORACLE, "cov", f"COV={build}"], check=True)
    lib = str(build / "liboracle_f32.so")
    procs = {}
    for fam in si.FAMILIES:  # one process and one set of counters per family, side by side
        famdir = tmp_path / fam
        famdir.mkdir()
        for f in os.listdir(build):
            if f.endswith(".gcno"):
                shutil.copy(build / f, famdir / f)
        env = dict(os.environ, GCOV_PREFIX=str(famdir), GCOV_PREFIX_STRIP="64", OMP_NUM_THREADS="1")
        procs[fam] = subprocess.Popen([sys.executable, WORKER, lib, fam, str(famdir / "result.json")], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    results, reached, cov_all = {}, {}, {}
    for fam, p in procs.items():
        out, _ = p.communicate(timeout=3000)
        assert p.returncode == 0, f"family {fam}:\n{out[-4000:]}"
        with open(tmp_path / fam / "result.json") as f:
            results[fam] = json.load(f)
        cov = _coverage(gcov, str(tmp_path / fam))
        reached[fam] = _items(cov)
        for k, v in cov.items():
            cov_all.setdefault(k, (v[0], len(v[2])))

    # ---- the condition: finite, no exception
    n_cases = sum(r["cases"] for r in results.values())
    n_cand = sum(r["candidates"] for r in results.values())
    bad = [x for r in results.values() for x in r["nonfinite"]]
    print(f"\ncensus: {n_cases} cases, {n_cand} candidates, max |final state| = {max(r['max_abs'] for r in results.values()):.1f}")
    assert not bad, f"{len(bad)} of {n_cases} cases go non-finite in the checker:\n" + "\n".join(bad[:40])

    # ---- what has to be reached
    src = {f: open(os.path.join(ORACLE, f)).read().splitlines() for f in FILES}
    union = set().union(*reached.values())
    funcs = {fn for (name, _), (fn, _) in cov_all.items() if name == "mbd_oracle_physics.c"}
    assert {"substep", "env_step", "reward_origin", "orc_rollout", "joint_frames"} <= funcs, funcs
    assert set(NOT_CALLED) <= funcs, set(NOT_CALLED) - funcs
    missing = []  # (file, line, function, "line" or branch index, description)
    for (name, n), (fn, n_br) in sorted(cov_all.items()):
        if (name == "mbd_oracle_physics.c" and fn in NOT_CALLED) or (name == "spec_math.h" and fn in NOT_STEP_MATH):
            continue
        if ("line", name, n) not in union:
            missing.append((name, n, fn, "line", "line never executed"))
            continue
        for k in range(n_br):
            if ("branch", name, n, k) not in union:
                missing.append((name, n, fn, k, f"branch {k} of {n_br} never taken"))
    used, unexcused = set(), []
    for name, n, fn, item, what in missing:
        text = src[name][n - 1]
        hit = [(i, j) for i, (f, func, snippet, items, _, _) in enumerate(ALLOWED) for j in items
               if f == name and func == fn and snippet in text and j == item]
        if hit:
            used.update(hit)
        else:
            unexcused.append(f"{name}:{n} [{fn}] {what}: {text.strip()}")
    for fam in si.FAMILIES:
        others = set().union(*(v for k, v in reached.items() if k != fam))
        only = sorted(reached[fam] - others)
        print(f"family {fam:12s}: {results[fam]['cases']:5d} cases; reaches {len(reached[fam])} lines / branch directions, "
              f"{len(only)} of them alone" + (": " + ", ".join(f"{i[1]}:{i[2]}" for i in only[:12]) if only else ""))
    assert all(kind in ("dump", "entry", "never") for *_, kind, _ in ALLOWED)
    assert not unexcused, f"{len(unexcused)} lines / branches of the step path are not reached by any case:\n" + "\n".join(unexcused)
    stale = [ALLOWED[i][1:3] + (j,) for i in range(len(ALLOWED)) for j in ALLOWED[i][3] if (i, j) not in used]
    assert not stale, f"allow-list entries that excuse nothing (reached now, or the line is gone): {stale}"
