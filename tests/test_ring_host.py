"""On the CPU: the arithmetic every device ring log is read through (csrc/mbd_ring.h: the pick record's ticks, the adapt and the
elite record's steps — "the most recent n entries, oldest first, in two pieces at most"), compiled for the host by the ROCm clang
as it is and run over every combination of cap in 1..5, count in 0..3 cap + 1 and n in 0..cap + 2 (tests/ring_host.cpp) — the
smallest sizes at which every branch occurs; the logs themselves wrap after 65536 entries, which no test of a plan reaches."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "model-based-diffusion_amd", "csrc")


def test_ring_runs_read_the_most_recent_entries_oldest_first(tmp_path):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    clang = os.path.join(g._llvm_bin(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), "clang++")
    exe = str(tmp_path / "ring")
    subprocess.run([clang, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                    "-Werror", f"-I{CSRC}", os.path.join(ROOT, "tests", "ring_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    combos = sum((3 * cap + 2) * (cap + 3) for cap in range(1, 6))
    m = re.search(r"(\d+) combinations, 0 mismatches", r.stdout)
    assert m and int(m.group(1)) == combos == 360, r.stdout
