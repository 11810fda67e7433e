"""The sampler of a diffusion step, form by form: a table of plans that reach every launch form of the normals, and an
independent float64 restatement of `jax.random.normal(key, (N, HNu))` to hold them to.

Shared by tests/test_sampler_reference.py (the checker against the restatement, and the host arithmetic that proves every
entry takes the branch its comment claims — on the CPU) and tests/test_gpu_sampler.py (the kernels against the checker, by bit
pattern).  numpy and scipy only; nothing here touches the checker, the library or a device.

THE RESTATEMENT is written from JAX's own definition (jax/_src/prng.py, jax/_src/random.py), not from oracle/:

  threefry2x32   Threefry-2x32, 20 rounds (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): key schedule
                 ks = (k0, k1, k0 ^ k1 ^ 0x1BD11BDA), rotations (13, 15, 26, 6) and (17, 29, 16, 24) alternating per group of
                 four rounds, after group g = 1..5 the injection x0 += ks[g % 3], x1 += ks[(g + 1) % 3] + g.
  legacy layout  (jax_threefry_partitionable=False) random_bits of `size` 32-bit words: counters iota(size), padded with ONE
                 zero when size is odd, split into a first and a second half which are the two input words of size/2 blocks;
                 the output is concat(first words, second words)[:size].
  partitionable  element e has its own block with the counter words (e >> 32, e & 0xffffffff); its bits are the xor of the
                 two output words.
  normal         u = max(lo, f * (1 - lo) + lo) in float32, f = bitcast(bits >> 9 | 0x3f800000) - 1, lo = nextafter(-1, 0);
                 then sqrt(2) * erfinv(u) — here in float64 by scipy, in JAX by a float32 polynomial (Giles), which is what
                 the checker and the kernels restate: they may differ from this by that polynomial's error, 1e-5 relative
                 (tests/test_oracle_prng.py::test_erfinv_matches_giles_accuracy), never by more.

`bits(key, layout, size, begin, count)` and `normal64(...)` take flat element ranges; `rows64(key, layout, N, HNu, begin,
count)` takes candidate rows.  A range of a small tensor is a slice of the whole-tensor form above; beyond `WHOLE_LIMIT`
elements a range is computed element by element (`bits_at`), which tests/test_sampler_reference.py holds equal to the slice.

THE TABLE.  `CASES` lists `Case` records: the form (a key of `FORMS`), env, N, H, shard, layout (0 legacy, 1 partitionable),
levers, and as `why` the boundary the entry straddles.  Forms (the launch sites they name are in csrc/):

  whole        sample_kernel over the whole tensor: materialised plans — car2d MBD plans (sigma from the host), path-integral
               plans (sigma on the device), rigid-body MBD plans created under MBD_NO_LAZY
  three_range  a sharded materialised plan with N >= 5 shard_count: sample_kernel over [own0, own1) on the step's stream and
               over [0, own0) and [own1, total) on the second — the only launches of its sub-range branch
  one_range    the same shards where the host keeps everything in one whole-tensor launch (N < 5 shard_count, MBD_NO_AUX)
  noise        lazy plans (rigid-body MBD): noise_kernel, then shift_kernel at peek
  fused        lazy plans whose NEXT step's normals were declared (mbd_plan_prefetch_noise): the noise workgroups of the rollout
               launch (plain: noise_blocks, nb = min(need, spare CUs); XCD-pinned: 7 of every 8 workgroups), or noise_kernel on
               the second stream when the launch cannot take the job (MBD_NO_FUSED_NOISE, a one-workgroup shard: nz_fits false)

Sweeps (noise_batch_kernel, sample_batch_kernel) and the plant's rows (mpc_plant_rows_kernel) have no peek: their cases —
`SWEEPS`, `PLANT` — are whole runs compared with the plans run alone and with tests/mpc_plant_checker.py.
"""
from dataclasses import dataclass, field

import numpy as np

LEGACY, PARTITIONABLE = 0, 1
LAYOUTS = (LEGACY, PARTITIONABLE)
WHOLE_LIMIT = 1 << 22  # elements up to which a range is cut out of the whole-tensor form

# action sizes of the envs the table uses (tests/test_sampler_reference.py checks them against the compiled models)
NU = {"cartpole": 1, "car2d": 2, "hopper": 3, "ant": 8, "humanoidrun": 17}

_ROT = ((13, 15, 26, 6), (17, 29, 16, 24))
_M32 = np.uint64(0xFFFFFFFF)


def threefry2x32(k0, k1, c0, c1):
    """Threefry-2x32-20 of the counter words (c0, c1) — uint32 arrays of one shape — under the key (k0, k1): two uint32
    arrays.  (Computed in uint64 and masked: numpy warns about uint32 scalar overflow, never about this.)"""
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    ks = (k0, k1, k0 ^ k1 ^ np.uint64(0x1BD11BDA))
    x0 = (np.asarray(c0, np.uint32).astype(np.uint64) + ks[0]) & _M32
    x1 = (np.asarray(c1, np.uint32).astype(np.uint64) + ks[1]) & _M32
    for g in range(1, 6):
        for r in _ROT[(g - 1) % 2]:
            x0 = (x0 + x1) & _M32
            x1 = ((x1 << np.uint64(r)) | (x1 >> np.uint64(32 - r))) & _M32
            x1 = x1 ^ x0
        x0 = (x0 + ks[g % 3]) & _M32
        x1 = (x1 + ks[(g + 1) % 3] + np.uint64(g)) & _M32
    return x0.astype(np.uint32), x1.astype(np.uint32)


def split(key, num, layout):
    """jax.random.split(key, num): uint32 [num][2].  Legacy: the 2 num words of random_bits, row by row; partitionable: key j
    is both output words of the block with the counter (0, j)."""
    if layout == PARTITIONABLE:
        o0, o1 = threefry2x32(key[0], key[1], np.zeros(num, np.uint32), np.arange(num, dtype=np.uint32))
        return np.stack([o0, o1], axis=1)
    return bits_whole(key, LEGACY, 2 * num).reshape(num, 2)


def prng_key(seed):
    """jax.random.PRNGKey(seed): the high and the low word of the 64-bit seed."""
    return np.array([(int(seed) >> 32) & 0xFFFFFFFF, int(seed) & 0xFFFFFFFF], np.uint32)


def bits_whole(key, layout, size):
    """random_bits(key, 32, (size,)) as JAX lays it out: uint32 [size]."""
    size = int(size)
    if layout == PARTITIONABLE:
        e = np.arange(size, dtype=np.uint64)
        o0, o1 = threefry2x32(key[0], key[1], (e >> np.uint64(32)).astype(np.uint32), (e & _M32).astype(np.uint32))
        return o0 ^ o1
    half = (size + 1) // 2
    counts = np.arange(2 * half, dtype=np.uint64)
    counts[size:] = 0  # (the padding of an odd size)
    o0, o1 = threefry2x32(key[0], key[1], counts[:half].astype(np.uint32), counts[half:].astype(np.uint32))
    return np.concatenate([o0, o1])[:size]


def bits_at(key, layout, size, e):
    """The same words at the flat indices e (any integer array, all < size), element by element: in the legacy layout element
    e < half is the first word of block e, element e >= half the second word of block e - half."""
    e = np.asarray(e, np.uint64)
    size = int(size)
    assert e.size == 0 or int(e.max()) < size
    if layout == PARTITIONABLE:
        o0, o1 = threefry2x32(key[0], key[1], (e >> np.uint64(32)).astype(np.uint32), (e & _M32).astype(np.uint32))
        return o0 ^ o1
    half = np.uint64((size + 1) // 2)
    first = e < half
    j0 = np.where(first, e, e - half)
    j1 = j0 + half
    o0, o1 = threefry2x32(key[0], key[1], j0.astype(np.uint32), np.where(j1 < np.uint64(size), j1, np.uint64(0)).astype(np.uint32))
    return np.where(first, o0, o1)


def bits(key, layout, size, begin=0, count=None):
    count = int(size) - int(begin) if count is None else int(count)
    assert 0 <= begin and begin + count <= size
    if size <= WHOLE_LIMIT:
        return bits_whole(key, layout, size)[begin:begin + count]
    return bits_at(key, layout, size, np.arange(begin, begin + count, dtype=np.uint64))


def uniform32(b):
    """jax.random.uniform(minval=nextafter(-1, 0), maxval=1) of the words b, in float32 like JAX."""
    lo = np.nextafter(np.float32(-1.0), np.float32(0.0))
    f = ((np.asarray(b, np.uint32) >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1.0)
    return np.maximum(lo, f * (np.float32(1.0) - lo) + lo)


def normal64_of_bits(b):
    from scipy import special
    return np.sqrt(2.0) * special.erfinv(uniform32(b).astype(np.float64))


def normal64(key, layout, size, begin=0, count=None):
    """float64 [count]: elements [begin, begin + count) of normal(key, (size,))."""
    return normal64_of_bits(bits(key, layout, size, begin, count))


def rows64(key, layout, N, HNu, begin=0, count=None):
    """float64 [count][HNu]: candidate rows [begin, begin + count) of normal(key, (N, HNu))."""
    count = N - begin if count is None else count
    return normal64(key, layout, N * HNu, begin * HNu, count * HNu).reshape(count, HNu)


def ratio(got, ref64):
    """max |got - ref| / max(|ref|, 1e-30): the figure the float64 comparisons assert on (< RTOL)."""
    got, ref64 = np.asarray(got, np.float64).reshape(-1), np.asarray(ref64, np.float64).reshape(-1)
    assert got.size == ref64.size
    if got.size == 0:
        return 0.0
    return float((np.abs(got - ref64) / np.maximum(np.abs(ref64), 1e-30)).max())


RTOL = 1e-5  # the bound test_erfinv_matches_giles_accuracy asserts for the float32 polynomial
MAX_ABS_NORMAL = 5.5  # no float32 normal of JAX exceeds ~5.42: u = nextafter(-1, 0) or 1 - 2^-23 gives |z| = 5.42


# ---- the table -----------------------------------------------------------------------------------------------------------
FORMS = ("whole", "three_range", "one_range", "noise", "fused")
N_CUS = 256          # the MI355X the launch arithmetic below is asserted for
NOISE_CAP = 65536 * 256      # thread-items of noise_kernel's largest grid (mbd_plan.hip launch_noise)
BATCH_CAP = 4096 * 256       # thread-items per plan of noise_batch_kernel's and sample_batch_kernel's (mbd_sweep.hip)
AUX_RATIO = 5                # the three-range launch is used when N >= AUX_RATIO * shard_count (mbd_plan.hip)
# MBD plans: Ndiffuse, the step whose sigma cannot saturate (5.5 sigma_1 < 1: the clip is the identity on Ybar = 0) and the
# step of the schedule's largest sigma; path-integral plans: the sigmas set with set_sigma (0.125 is a power of two: the
# product with a normal is exact)
ND, I_SMALL, I_LARGE = 30, 1, 29
PI_SIGMA_SMALL, PI_SIGMA_LARGE = 0.125, 1.0


@dataclass(frozen=True)
class Case:
    form: str
    env: str
    N: int
    H: int
    layout: int
    why: str
    kind: str = "mbd"            # "mbd": an MBD plan; "pi": a path-integral (mppi) plan, sigma on the device
    shard: tuple = None          # (begin, count), or None: the whole plan
    levers: dict = field(default_factory=dict)
    expect: dict = field(default_factory=dict)  # what the reach test asserts of the launch (fused cases)
    large: bool = False          # one of the four cap cases

    @property
    def HNu(self):
        return self.H * NU[self.env]

    @property
    def total(self):
        return self.N * self.HNu

    @property
    def items(self):
        """thread-items of the whole-tensor forms: elements (partitionable) or pairs (legacy)"""
        return self.total if self.layout == PARTITIONABLE else (self.total + 1) // 2

    @property
    def id(self):
        s = f"{self.form}-{self.kind}-{self.env}-N{self.N}-H{self.H}-{'part' if self.layout else 'legacy'}"
        if self.shard:
            s += f"-shard{self.shard[0]}+{self.shard[1]}"
        for k, v in sorted(self.levers.items()):
            s += f"-{k[4:]}{v}"
        return s

    @property
    def lazy(self):
        return self.kind == "mbd" and self.env != "car2d" and not self.levers.get("MBD_NO_LAZY")


def _both(form, env, N, H, why, **kw):
    return [Case(form, env, N, H, lay, why, **kw) for lay in LAYOUTS]


def _build():
    c = []
    # ---- whole tensor, materialised ------------------------------------------------------------------------------------
    for n in (1, 2, 3):  # tiny totals: one pair and a padded counter (1, 3), exactly one pair (2)
        c += _both("whole", "cartpole", n, 1, f"total {n}", kind="pi")
    c += _both("whole", "hopper", 1, 1, "total 3 in one row: an odd total whose padded pair is the row's middle", kind="pi")
    c += _both("whole", "car2d", 1, 1, "total 2, sigma from the host")
    # around one 256-thread workgroup: elements (partitionable) 255 / 256 / 257; pairs (legacy) 255 / 256 / 257 = totals 510
    # (255 pairs), 511 (256, the last one padded), 512 (256), 513 (257, the first thread of a second workgroup has the
    # padded pair), 514 (257)
    for n in (255, 256, 257, 510, 511, 512, 513, 514):
        c += _both("whole", "cartpole", n, 1, f"total {n}: one workgroup of 256 threads, exactly, one more, one fewer", kind="pi")
    # odd totals (N odd and H Nu odd) with a row length coprime to 256: Ybar's index wraps at another place in every
    # workgroup, and `half` falls inside a row
    c += _both("whole", "cartpole", 37, 7, "odd total 259, rows of 7", kind="pi")
    c += _both("whole", "hopper", 101, 11, "odd total 3333, rows of 33 (coprime to 256): half = 1667 is inside row 50", kind="pi")
    c += _both("whole", "car2d", 65, 7, "even total 910, rows of 14, sigma from the host")
    c += _both("whole", "car2d", 1000, 50, "car2d at its usual horizon")
    c += _both("whole", "hopper", 33, 5, "a rigid-body MBD plan made to materialise: odd total 495", levers={"MBD_NO_LAZY": 1})
    # ---- sharded, materialised: the three-range launch and its neighbours -------------------------------------------------
    # hopper H = 5: rows of 15; N = 45: total 675 (odd), half = 338 = row 22, element 8.  count = 9 = N / 5: the switch's own side
    for begin, what in ((0, "own rows first: the first second-stream range is empty; own rows below half"),
                        (9, "own rows [9, 18) entirely below half (row 22.5)"),
                        (18, "own rows [18, 27) straddle half, which falls inside row 22"),
                        (27, "own rows [27, 36) entirely above half"),
                        (36, "own rows last: the last second-stream range is empty; own rows above half")):
        for kw in (dict(kind="pi"), dict(kind="mbd", levers={"MBD_NO_LAZY": 1})):
            c += _both("three_range", "hopper", 45, 5, f"N = 5 count, odd total; {what}", shard=(begin, 9), **kw)
            c += _both("one_range", "hopper", 45, 5, f"the same shard under MBD_NO_AUX; {what}", shard=(begin, 9),
                       **{**kw, "levers": {**kw.get("levers", {}), "MBD_NO_AUX": 1}})
    for begin in (0, 16, 32):  # car2d: rows of 14, even total 560, half = 280 = the start of row 20
        c += _both("three_range", "car2d", 40, 7, f"N = 5 count, even total, half on a row boundary; own rows [{begin}, {begin + 8})",
                   shard=(begin, 8))
    c += _both("three_range", "car2d", 64, 7, "N = 8 count (the eight-rank layout); own rows [24, 32) end at half", shard=(24, 8))
    # a long sub-range: more than one workgroup per range, row length coprime to 256, ranges that start off a multiple of 256
    c += _both("three_range", "hopper", 505, 11, "N = 5 count, odd total 16 665, rows of 33: every range spans many workgroups",
               shard=(202, 101), kind="pi")
    c += _both("one_range", "hopper", 44, 5, "N = 5 count - 1: the host keeps one whole-tensor launch", shard=(18, 9), kind="pi")
    c += _both("one_range", "car2d", 39, 7, "N = 5 count - 1: the host keeps one whole-tensor launch", shard=(16, 8))
    # ---- lazy plans: noise_kernel, shift_kernel at peek --------------------------------------------------------------------
    for n in (1, 2, 3):
        c += _both("noise", "cartpole", n, 1, f"total {n}")
    for n in (255, 256, 257, 510, 511, 512, 513, 514):
        c += _both("noise", "cartpole", n, 1, f"total {n}: around one workgroup of elements / of pairs")
    c += _both("noise", "hopper", 101, 11, "odd total 3333, rows of 33")
    c += _both("noise", "humanoidrun", 64, 10, "the smoke plan's shape")
    c += _both("noise", "humanoidrun", 48, 50, "a shard of a lazy plan still generates all N rows", shard=(16, 16))
    # the grid cap of noise_kernel, 65 536 workgroups: ant at H = 32 has rows of 256 = one workgroup of elements, two rows
    # a workgroup of pairs.  The only large cases: two per layout
    c.append(Case("noise", "ant", 65536, 32, PARTITIONABLE, "thread-items = 65 536 x 256 exactly: the largest grid, no wrap", large=True))
    c.append(Case("noise", "ant", 65537, 32, PARTITIONABLE, "one row above the cap: the first workgroup's threads wrap once", large=True))
    c.append(Case("noise", "ant", 131072, 32, LEGACY, "pairs = 65 536 x 256 exactly: the largest grid, no wrap", large=True))
    c.append(Case("noise", "ant", 131073, 32, LEGACY, "one row above: 128 more pairs, half of the first workgroup wraps", large=True))
    # ---- the next step's normals beside the rollout -------------------------------------------------------------------------
    fused = [
        ("humanoidrun", 300, 3, None, {}, dict(pin=False, fused=True, wrap=False),
         "19 rollout workgroups, need < spare: no wrap, the last noise workgroup is partial"),
        ("humanoidrun", 300, 50, None, {}, dict(pin=False, fused=True, wrap=True),
         "19 rollout workgroups, need > spare = 237: the noise workgroups wrap"),
        ("humanoidrun", 100, 20, None, {}, dict(pin=True, fused=True, wrap=True),
         "7 rollout workgroups pinned to one XCD: the 49 others take the job, index (q 7 + r - 1), stride 7 roll_blocks"),
        ("hopper", 31, 11, None, {}, dict(pin=True, fused=True, wrap=False),
         "8 one-candidate wavefront workgroups of a planar model, pinned; odd total 1023, fewer items than noise threads"),
        ("humanoidrun", 1100, 50, (16, 16), {}, dict(pin=True, fused=False, wrap=None),
         "a one-workgroup shard of a large plan: nz_fits is false, the job moves to the second stream"),
        ("humanoidrun", 300, 50, None, {"MBD_ROLL_PIN": 1}, dict(pin=True, fused=True, wrap=True),
         "19 workgroups pinned on request (9 to 32): 133 noise workgroups"),
    ]
    for env, N, H, shard, lv, expect, why in fused:
        c += _both("fused", env, N, H, why, shard=shard, levers=lv, expect=expect)
        if expect["fused"]:
            c += _both("fused", env, N, H, "the same launch with MBD_NO_FUSED_NOISE: noise_kernel on the second stream", shard=shard,
                       levers={**lv, "MBD_NO_FUSED_NOISE": 1}, expect=dict(pin=expect["pin"], fused=False, wrap=None))
    return c


CASES = _build()


def cases(form=None, large=None):
    return [c for c in CASES if (form is None or c.form == form) and (large is None or c.large == large)]


def spans(c):
    """The flat element ranges [(begin, count, stream)] the host launches sample_kernel over for a materialised case —
    mbd_plan.hip's own arithmetic, restated: stream 0 is the step's, 1 the plan's second stream."""
    total = c.total
    if c.shard is None or c.shard[1] == c.N or c.levers.get("MBD_NO_AUX") or c.N < AUX_RATIO * c.shard[1]:
        return [(0, total, 0)]
    own0, own1 = c.shard[0] * c.HNu, (c.shard[0] + c.shard[1]) * c.HNu
    return [s for s in ((own0, own1 - own0, 0), (0, own0, 1), (own1, total - own1, 1)) if s[1] > 0]


# a bench of Ybar values for the saturating cases: +-1, outside [-1, 1], +-0.0, subnormals, ordinary values
def ybar_edges(HNu, seed=0):
    g = np.random.default_rng([seed, HNu])
    y = (g.normal(size=HNu) * 0.4).astype(np.float32)
    sub = np.float32(1e-41)
    edge = np.array([1.0, -1.0, 1.5, -2.0, 0.0, -0.0, sub, -sub, np.float32(1.17549435e-38), 37.0, -1e30], np.float32)
    idx = g.permutation(HNu)[:min(HNu, edge.size)]
    y[idx] = edge[:idx.size]
    return y


# ---- sweeps and plant rows (whole runs) --------------------------------------------------------------------------------
# (env, N, H, steps, kind): per-plan thread-items above BATCH_CAP in both layouts, so the grid-stride loops wrap
SWEEPS = (
    ("humanoidrun", 4096, 50, 3, "mbd"),   # 3 481 600 elements per plan: noise_batch_kernel wraps 3.3 x (1.7 x in pairs)
    # (a sweep refuses plans of more than 12 288 candidates: the odd total needs N odd and H Nu odd, 171 at the least)
    ("hopper", 12287, 57, 3, "pi"),        # odd total 2 101 077: 1 050 539 pairs, 1963 above sample_batch_kernel's 4096 x 256
)
# exec_steps of humanoidrun (Nu = 17) whose E Nu + 3 normals sit either side of the one workgroup's 256 threads (elements) and
# of 512 (pairs): 241 (odd), 258 (even), 496 (even), 513 (odd)
PLANT_E = (14, 15, 29, 30)
