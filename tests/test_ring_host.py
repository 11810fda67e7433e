"""On the CPU: the arithmetic every device ring log is read through (csrc/mbd_ring.h: the pick record's ticks, the adapt and the
elite record's steps — "the most recent n entries, oldest first, in two pieces at most"), compiled for the host by the ROCm clang
as it is and run over every combination of cap in 1..5, count in 0..3 cap + 1 and n in 0..cap + 2 (tests/ring_host.cpp) — the
smallest sizes at which every branch occurs; the logs themselves wrap after 65536 entries, which no test of a plan reaches, so
tests/test_gpu_ring_read.py runs the device reader built on it (ring_read, through mbd_debug_ring_read) over small wrapped rings.
Here: that entry's refusals, which need no device."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

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


def test_the_device_reader_entry_refuses_on_the_host(lib):
    """mbd_debug_ring_read / _i32 (include/mbd_hip_debug.h): NULL arrays and sizes are refused before any device access; a valid
    call without a device is MBD_ERR_NO_DEVICE and leaves ``out`` alone."""
    from mbd_hip import _capi
    lib.mbd_last_error.restype = C.c_char_p
    for name, dtype in (("mbd_debug_ring_read", np.float32), ("mbd_debug_ring_read_i32", np.int32)):
        assert name not in _capi.EXPORTS, "the debug entries are no part of the boundary"
        fn = getattr(lib, name)
        fn.argtypes = _capi.RING_READ_ARGTYPES
        ring, out = np.arange(6, dtype=dtype), np.full(6, 7, dtype)
        r, o = ring.ctypes.data, out.ctypes.data
        assert fn(None, 1, 6, 6, 6, o) == _capi.MBD_ERR_INVALID and b"NULL" in lib.mbd_last_error()
        assert fn(r, 1, 6, 6, 6, None) == _capi.MBD_ERR_INVALID and b"NULL" in lib.mbd_last_error()
        for width, cap, count, n in ((0, 6, 6, 6), (17, 6, 6, 6), (1, 0, 6, 6), (1, 65537, 6, 6), (1, 6, -1, 6), (1, 6, 6, -1)):
            assert fn(r, width, cap, count, n, o) == _capi.MBD_ERR_INVALID and b"ring_read" in lib.mbd_last_error(), (width, cap, count, n)
        if _capi.device_count() == 0:
            assert fn(r, 3, 2, 5, 2, o) == _capi.MBD_ERR_NO_DEVICE
            with pytest.raises(_capi.MbdError):
                _capi.debug_ring_read(ring.reshape(2, 3), 5, 2)
        assert (out == 7).all()
