"""-m gpu: the reader of the device ring logs on a device, wrapped and unwrapped (csrc/mbd_internal.h ring_read through
mbd_debug_ring_read / mbd_debug_ring_read_i32, include/mbd_hip_debug.h): the two copies, the advance of the output between them and
the scaling by the entry width.  tests/test_ring_host.py holds the integer arithmetic on the host; a plan's own logs wrap after
65536 entries, which no test of a plan reaches.

  cap in {1, 2, 3, 5, 8}, count in 0 .. 3 cap + 1, n in {0, 1, cap - 1, cap, cap + 3}, width in {1, 3}, float32 and int32;
  entry j holds the value j (column c: j * width + c), written at slot j % cap, later entries over earlier ones;
  the reference is the sentence itself: the last min(n, count, cap) entries, oldest first."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
CAPS, WIDTHS = (1, 2, 3, 5, 8), (1, 3)
UNWRITTEN = 1 << 20  # what a slot no entry reached holds: the reader must not return it


@pytest.fixture(scope="module")
def gpu(lib):
    from mbd_hip import _capi
    if _capi.device_count() < 1:
        pytest.fail("tests/test_gpu_ring_read.py needs a GPU")
    return _capi


def _entry(j, width):
    return [j * width + c for c in range(width)]


def _ring(cap, width, count, dtype):
    ring = np.full((cap, width), UNWRITTEN, dtype)
    for j in range(count):
        ring[j % cap] = _entry(j, width)
    return ring


def _expected(cap, width, count, n, dtype):
    entries = [_entry(j, width) for j in range(count)]
    m = min(n, count, cap)
    return np.array(entries[count - m:], dtype).reshape(m, width)


def cases():
    for cap in CAPS:
        for count in range(3 * cap + 2):
            for n in sorted({0, 1, cap - 1, cap, cap + 3}):
                for width in WIDTHS:
                    yield cap, count, n, width


def test_the_enumeration_is_what_the_module_says():
    cs = list(cases())
    assert len(cs) == len(set(cs)) == sum((3 * cap + 2) * len({0, 1, cap - 1, cap, cap + 3}) for cap in CAPS) * len(WIDTHS)
    assert any(count > cap and 1 < n for cap, count, n, _ in cs)  # (wrapped reads of more than one entry are among them)


@pytest.mark.parametrize("dtype", (np.float32, np.int32), ids=("float32", "int32"))
def test_ring_read_returns_the_most_recent_entries_oldest_first(gpu, dtype):
    wrong = []
    for cap, count, n, width in cases():
        got = gpu.debug_ring_read(_ring(cap, width, count, dtype), count, n)
        ref = _expected(cap, width, count, n, dtype)
        if got.shape != ref.shape or got.tobytes() != ref.tobytes():
            wrong.append((cap, count, n, width, got.tolist(), ref.tolist()))
    assert not wrong, f"{len(wrong)} cases, the first (cap, count, n, width, got, expected): {wrong[0]}"
