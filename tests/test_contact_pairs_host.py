"""On the CPU: the (x, y)-pair form of stage (4) (csrc/mbd_kernels.h, MAXCOL == 1 && ISO) against the loop it stands in for,
both cut out of the kernel source as they are, compiled for the host by the ROCm clang with -ffp-contract=off and run on
400 000 random poses — exact touches, resting and sliding contacts, planar poses with zeros of either sign, zero collider
offsets, inactive lanes.  Corrections, contact flag, contact point and multiplier must agree bit for bit.  (What the GPU
compiler makes of the pair form is tests/test_gpu_contact_pairs.py's business.)"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "model-based-diffusion_amd", "csrc")

STUB = """#pragma once
#include <math.h>
#define __host__
#define __device__
#define __forceinline__ inline __attribute__((always_inline))
#define __builtin_amdgcn_rcpf(x) (1.0f / (x))
#define __builtin_amdgcn_rsqf(x) (1.0f / sqrtf(x))
"""


def _cut(text, begin, end, keep_end=False):
    a = text.index(begin)
    b = text.index(end, a)
    return text[a:b + (len(end) if keep_end else 0)]


def test_pair_form_of_stage4_is_the_loop_bit_for_bit(tmp_path):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    clang = os.path.join(g._llvm_bin(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), "clang++")
    with open(os.path.join(CSRC, "mbd_kernels.h")) as f:
        kern = f.read()
    with open(os.path.join(CSRC, "mbd_math.h")) as f:
        math_h = f.read()
    pair = _cut(kern, "          const f2 ib2 = mk2(ic.ib[0], ic.ib[0])", "        } else {\n#pragma unroll\n        for (int j = 0; j < MAXCOL; ++j) {")
    scal = _cut(kern, "          const v3 off = rot(col_pos[j], r);", "con_pos[j] = pos; con_dlam[j] = dlam; con_act[j] = active;", keep_end=True)
    assert "rot_p(" in pair and "div2_pos_" in pair and "div2_pos_" in scal
    fence = 'asm("" : "+v"(x));'  # (a register constraint of the GPU: the fence is a no-op for the values)
    assert math_h.count(fence) == 1
    os.makedirs(tmp_path / "hip")
    (tmp_path / "hip" / "hip_runtime.h").write_text(STUB)
    (tmp_path / "mbd_math.h").write_text(math_h.replace(fence, ""))
    (tmp_path / "pair.inc").write_text(pair)
    (tmp_path / "scal.inc").write_text(scal)
    exe = str(tmp_path / "chk")
    subprocess.run([clang, "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wno-unused-variable", f"-I{tmp_path}",
                    os.path.join(ROOT, "tests", "contact_pairs_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:]
    m = re.search(r"(\d+) cases, (\d+) active, (\d+) with a tangential impulse, 0 mismatches", r.stdout)
    assert m and int(m.group(1)) == 400000 and int(m.group(2)) > 100000 and int(m.group(3)) > 30000, r.stdout
