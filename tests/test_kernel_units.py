"""Every unit of libmbd_hip.so emits the kernels it launches and no others, as far as the headers are split: needs hipcc, no GPU.

A `static __global__` is emitted by every translation unit that sees it, launched or not.  mbd_internal.h therefore includes no
kernel: mbd_exchange.hip and mbd_debug_math.hip, which include it, must emit their own kernels and nothing else, and the
kernels of mbd_env_kernels.h must not appear in mbd_plan.hip or mbd_sweep.hip.  The kernels only members of the records launch are
mbd_record_kernels.h's, which mbd_records.hip alone includes: that unit must emit exactly them, each named in its own file, and
mbd_plan.hip and mbd_sweep.hip none of them; the four guard macros that used to steer this are gone.  The test compiles the device
assembly of those five units with the build's flags, side by side, and reads the `.amdhsa_kernel` names; it does not look at
instructions.  (mbd_env.hip takes about two minutes to compile and is not in the test: its 58 kernels — the rollout instantiations,
car2d_rollout_kernel, the two logpd kernels, lane_setup3_kernel — are counted in docs/experiments.md section 33.  mbd_plan.hip and
mbd_sweep.hip still share mbd_step_kernels.h and emit each other's step kernels, apart from those under the four guards that
remain: the test does not claim otherwise.)"""
import glob
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "model-based-diffusion_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

OWN = {"mbd_exchange.hip": ["exchange_push_kernel", "exchange_wait_kernel"], "mbd_debug_math.hip": ["eval_math_kernel"]}
STEP_UNITS = ("mbd_plan.hip", "mbd_sweep.hip")
RECORD_UNIT, RECORD_KERNELS = "mbd_records.hip", "mbd_record_kernels.h"
REMOVED_GUARDS = ("MBD_PICK_KERNEL", "MBD_VALUE_KERNEL", "MBD_ADAPT_KERNEL", "MBD_ZONE_KERNEL")


def base_name(symbol):
    """The kernel's own identifier from its mangled symbol _ZN <length><name> ... E: the last component of the nested name (an L in
    front of a length marks internal linkage; template arguments and the parameter types follow the name)."""
    assert symbol.startswith("_ZN"), symbol
    at, name = 3, None
    while True:
        m = re.match(r"L?(\d+)", symbol[at:])
        if not m:
            break
        at += m.end()
        name = symbol[at:at + int(m.group(1))]
        at += int(m.group(1))
    assert name and "_kernel" in name, symbol
    return name


def static_kernels(header):
    """the names of the `static __global__` definitions of a header of csrc/ (a template's line comes in front of it)"""
    with open(os.path.join(CSRC, header)) as f:
        return set(re.findall(r"^static __global__ [^\n]*?void (\w+)\(", f.read(), re.M))


@pytest.fixture(scope="module")
def emitted(tmp_path_factory):
    """unit -> the sorted base names of the kernels its device assembly holds"""
    from __graft_entry__ import HIPCC_FLAGS, TUS
    extra = dict(TUS)
    flags = [f for f in HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    td = tmp_path_factory.mktemp("units")

    def one(unit):
        asm = str(td / (unit + ".s"))
        subprocess.run([HIPCC, *flags, *extra[unit], "--cuda-device-only", "-S", os.path.join(CSRC, unit), "-o", asm], check=True,
                       capture_output=True)
        with open(asm) as f:
            return unit, sorted(base_name(s) for s in re.findall(r"^\s*\.amdhsa_kernel (\S+)", f.read(), re.M))

    units = list(OWN) + list(STEP_UNITS) + [RECORD_UNIT]
    with ThreadPoolExecutor(max_workers=len(units)) as ex:
        return dict(ex.map(one, units))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_units_without_step_launches_emit_their_own_kernels_only(emitted):
    for unit, own in OWN.items():
        assert emitted[unit] == own
        with open(os.path.join(CSRC, unit)) as f:
            text = f.read()
        for n in emitted[unit]:  # every kernel the unit emits is named, as an identifier, in the unit's own file
            assert re.search(r"\b%s\b" % n, text), (unit, n)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_env_kernels_are_emitted_by_no_step_unit(emitted):
    env_kernels = static_kernels("mbd_env_kernels.h")
    assert env_kernels == {"car2d_rollout_kernel", "logpd_track_kernel", "logpd_car2d_kernel", "lane_setup3_kernel"}
    for unit in STEP_UNITS:
        assert len(emitted[unit]) > 20  # (the names were read)
        assert not env_kernels & set(emitted[unit]), (unit, env_kernels & set(emitted[unit]))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_record_unit_emits_the_record_kernels_and_nothing_else(emitted):
    """mbd_records.hip emits exactly the kernels mbd_record_kernels.h defines (an instantiation of a template counts by its base
    name), and names each of them in its own file: it launches what it emits."""
    record_kernels = static_kernels(RECORD_KERNELS)
    assert len(record_kernels) >= 10  # (the definitions were read)
    assert set(emitted[RECORD_UNIT]) == record_kernels
    with open(os.path.join(CSRC, RECORD_UNIT)) as f:
        text = f.read()
    for n in record_kernels:
        assert re.search(r"\b%s\b" % n, text), n


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_record_kernels_are_emitted_by_no_step_unit(emitted):
    record_kernels = static_kernels(RECORD_KERNELS)
    for unit in STEP_UNITS:
        assert len(emitted[unit]) > 20  # (the names were read)
        assert not record_kernels & set(emitted[unit]), (unit, record_kernels & set(emitted[unit]))


def test_only_the_record_unit_includes_the_record_kernels():
    including = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        with open(path, errors="replace") as f:
            if re.search(r'^\s*#\s*include\s+"%s"' % re.escape(RECORD_KERNELS), f.read(), re.M):
                including.append(os.path.basename(path))
    assert including == [RECORD_UNIT]


def test_removed_guard_macros_are_gone():
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        with open(path, errors="replace") as f:
            text = f.read()
        for macro in REMOVED_GUARDS:
            assert macro not in text, (os.path.basename(path), macro)


def test_internal_header_sees_no_static_kernel():
    """No header mbd_internal.h includes, directly or not, defines a `static __global__` (the rollout templates of mbd_kernels.h are
    emitted only where they are instantiated)."""
    seen, todo = set(), ["mbd_internal.h"]
    while todo:
        name = todo.pop()
        if name in seen:
            continue
        seen.add(name)
        with open(os.path.join(CSRC, name)) as f:
            text = f.read()
        todo += [h for h in re.findall(r'^#include "(mbd_\w+\.h)"', text, re.M)]
        assert not re.search(r"^static __global__", text, re.M), name
    assert "mbd_step_args.h" in seen and "mbd_step_kernels.h" not in seen and "mbd_env_kernels.h" not in seen
    assert "mbd_step_device.h" in seen and RECORD_KERNELS not in seen
