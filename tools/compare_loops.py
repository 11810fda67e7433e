#!/usr/bin/env python3
"""Compare the main loop of every kernel in two device-assembly files (hipcc --cuda-device-only -S of one translation unit,
before and after a change): a change meant for a kernel's prologue must leave the control-step loop — the substeps — the
same instruction sequence.

    python tools/compare_loops.py before.s after.s

Per kernel: the largest backward-branch loop, its instructions with register numbers erased; prints the kernels whose opcode
sequences differ, and changes of scratch size and VGPR count.  Exit status 1 when any loop differs or any kernel gained scratch."""
import collections
import re
import sys


def kernels(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None:
            continue
        t = line.strip()
        if t.startswith("s_endpgm"):
            cur = None
        elif t.endswith(":") and not t.startswith((".", ";")):
            out[cur].append(("L", t[:-1]))
        elif t and not t.startswith((".", ";", "//")):
            out[cur].append(("I", t.split(";")[0].strip()))
    return out


def meta(path):
    pat = (r"\.name:\s+(_Z\w+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)(?:.*\n)*?\s+\.sgpr_count:\s+(\d+)"
           r"(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)")
    return {m.group(1): tuple(int(m.group(k)) for k in (2, 3, 4)) for m in re.finditer(pat, open(path).read())}


def main_loop(ins):
    pos, loops = {}, []
    for i, (kind, t) in enumerate(ins):
        if kind == "L":
            pos[t] = i
        elif t.startswith(("s_cbranch", "s_branch")) and t.split()[-1] in pos:
            loops.append((pos[t.split()[-1]], i))
    if not loops:
        return []
    s, e = max(loops, key=lambda x: x[1] - x[0])
    return [t.split()[0] for kind, t in ins[s:e] if kind == "I"]


def main(before, after):
    a, b, ma, mb = kernels(before), kernels(after), meta(before), meta(after)
    bad = 0
    for k in sorted(a):
        if k not in b:
            print(f"gone: {k}")
            bad += 1
            continue
        A, B = main_loop(a[k]), main_loop(b[k])
        if A != B:
            d = collections.Counter(A)
            d.subtract(collections.Counter(B))
            print(f"LOOP DIFFERS {k}: {len(A)} -> {len(B)} instructions, {sum(abs(v) for v in d.values())} in the multiset difference")
            bad += 1
        if k in ma and k in mb and ma[k] != mb[k]:
            print(f"scratch/sgpr/vgpr {ma[k]} -> {mb[k]}  {k[:100]}")
            bad += mb[k][0] > ma[k][0]
    print(f"{len(a)} kernels, {bad} with a different main loop or more scratch")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
