"""-m gpu: the sampler kernels on their own, in every launch form, layout and size of tests/sampler_inputs.py, against the
checker by bit pattern and against a float64 restatement of jax.random.normal.

Every other GPU test reaches the sampler through whole runs at a handful of even totals, or feeds `plan.peek()[0]` — the
GPU's own candidates — to the checker's update: a candidate tensor with a stale or misplaced element passes those.  An
element that a wrong stride or bound leaves unwritten is not a NaN either: it is whatever normal the ring buffer held two
steps earlier.  Only an element-by-element comparison sees it, so that is what happens here.

Pattern of a case (sampler_inputs.Case): create the Plan under the case's threefry layout and levers, call
mbd_plan_sample_rollout ONCE, and compare `plan.peek()[0]` — all N rows, a shard's peek returns all of them too — with
`orc.sample` on the same key, sigma and Ybar, by bit pattern (state_inputs.same_bits).  Two settings of the values per case:

  plain       Ybar = 0 at a sigma with 5.5 sigma < 1 (step 1 of the schedule; set_sigma(0.125) for path-integral plans): no
              float32 normal of JAX exceeds 5.42, so the clip is the identity, Y0s is a one-to-one image of the normals and no
              difference can hide behind saturation.  Also held to the float64 restatement within 1e-5 relative (the error
              of the float32 erf_inv polynomial; a layout error is O(1)).
  saturating  the schedule's largest sigma (step Nd - 1; set_sigma(1.0)) and a Ybar with +-1, values outside [-1, 1], +-0.0
              and subnormals: every output inside [-1, 1], and the checker's bits.

Forms and the launches they reach: see sampler_inputs.  The sweeps' batched kernels and the plant's rows have no peek: a
sweep is compared with its plans run alone (the existing contract) at per-plan sizes above the batched kernels' grid cap, a
disturbed episode with tests/mpc_plant_checker.py at counts of normals either side of the one workgroup that draws them.
"""
import functools

import numpy as np
import pytest

import sampler_inputs as sx
from state_inputs import same_bits

pytestmark = pytest.mark.gpu

KEY_SEED = 20240  # the key of the step under test is prng_key(KEY_SEED + N)


@pytest.fixture(scope="module")
def gpu(lib):
    from mbd_hip import _capi
    if _capi.device_count() < 1:
        pytest.fail("tests/test_gpu_sampler.py needs a GPU")
    return _capi


@functools.lru_cache(maxsize=None)
def _env(name):
    from mbd_hip.envs import get_env
    return get_env(name)


class _Sampler:
    """The plan of a case, and one sampler step of it at a time."""

    def __init__(self, gpu, orc, c, monkeypatch, levers):
        import torch
        from mbd_hip.planners import path_integral
        from mbd_hip.planners.mbd_planner import Args, Plan
        monkeypatch.setenv("MBD_THREEFRY_PARTITIONABLE", str(c.layout))
        if c.levers:
            levers(**c.levers)
        self.gpu, self.orc, self.c, self.torch = gpu, orc, c, torch
        env = _env(c.env)
        assert env.action_size == sx.NU[c.env]
        self.Nu = env.action_size
        begin, count = c.shard if c.shard else (0, c.N)
        self.count = count
        if c.kind == "pi":
            args = path_integral.Args(env_name=c.env, Nsample=c.N, Hsample=c.H, Nrefine=sx.ND, temp_sample=0.1,
                                      disable_recommended_params=True)
            self.plan = Plan(env, args, shard_begin=begin, shard_count=count, update_method=1)
        else:
            args = Args(env_name=c.env, Nsample=c.N, Hsample=c.H, Ndiffuse=sx.ND, temp_sample=0.1,
                        disable_recommended_params=True, not_render=True)
            self.plan = Plan(env, args, shard_begin=begin, shard_count=count)
        assert self.plan.cfg.prng_impl == c.layout
        self.plan.set_state0(env.reset(gpu.prng_key(3)))
        self.sched = orc.schedule(args.beta0 if c.kind == "mbd" else 1e-4, args.betaT if c.kind == "mbd" else 1e-2, sx.ND)
        assert np.array_equal(self.plan.schedule()[2], self.sched[2])
        self.loc = torch.zeros(count, device="cuda")
        self.all = torch.linspace(-1.0, 1.0, c.N, device="cuda")  # "gathered" rewards of a step nobody looks at
        self.out, self.rm = torch.zeros(c.HNu, device="cuda"), torch.zeros(1, device="cuda")
        self._keep = []

    def sigma(self, saturating):
        """(i, sigma) of the step: path-integral plans carry sigma on the device, MBD plans take the schedule's"""
        i = sx.I_LARGE if saturating else sx.I_SMALL
        if self.c.kind == "pi":
            s = sx.PI_SIGMA_LARGE if saturating else sx.PI_SIGMA_SMALL
            self.plan.set_sigma(s)
            return i, np.float32(s)
        return i, np.float32(self.sched[2][i])

    def ybar(self, saturating, seed=0):
        return sx.ybar_edges(self.c.HNu, seed) if saturating else np.zeros(self.c.HNu, np.float32)

    def sample_rollout(self, i, key, Ybar):
        d_Y = self.torch.tensor(Ybar, device="cuda")
        self._keep.append(d_Y)  # (the plan reads it until the step's second phase has run)
        self.gpu.check(self.plan.lib.mbd_plan_sample_rollout(self.plan.h, i, self.gpu.key_array(key), d_Y.data_ptr(),
                                                             self.loc.data_ptr(), None, None))
        return d_Y

    def score_update(self, i, key, d_Y):
        self.gpu.check(self.plan.lib.mbd_plan_score_update(self.plan.h, i, self.gpu.key_array(key), d_Y.data_ptr(),
                                                           self.all.data_ptr(), None, self.out.data_ptr(), self.rm.data_ptr(), None))

    def prefetch(self, key):
        self.gpu.check(self.plan.lib.mbd_plan_prefetch_noise(self.plan.h, self.gpu.key_array(key), None))

    def compare(self, key, sigma, Ybar, saturating, what):
        """peek()[0] of the last sample_rollout against the checker (bits) and, plain cases, the float64 restatement"""
        c = self.c
        self.torch.cuda.synchronize()
        assert self.torch.isfinite(self.loc).all(), f"{what}: rollout rewards"
        Y0s = self.plan.peek()[0]
        ref = self.orc.sample(key, c.layout, c.N, c.H, self.Nu, 0, c.N, float(sigma), Ybar.reshape(c.H, self.Nu))
        same_bits(Y0s, ref, what)
        assert np.abs(Y0s).max() <= 1.0, what
        if saturating:
            # (a handful of elements need not reach the clip; a thousand do: three deviations suffice on a zero mean)
            assert c.total < 1000 or (np.abs(Y0s) == 1.0).any(), f"{what}: nothing saturated"
            return None
        assert np.abs(Y0s).max() < 1.0, f"{what}: the plain setting saturated"
        if c.total > sx.WHOLE_LIMIT:  # the large cases: their first, middle (around `half`) and last rows, and a stride
            rows = sorted(set(range(3)) | set(range(c.N // 2 - 2, c.N // 2 + 3)) | set(range(c.N - 3, c.N)) | set(range(0, c.N, 1021)))
        else:
            rows = range(c.N)
        e = (np.asarray(rows, np.uint64)[:, None] * np.uint64(c.HNu) + np.arange(c.HNu, dtype=np.uint64)[None, :]).reshape(-1)
        want = sx.normal64_of_bits(sx.bits_at(key, c.layout, c.total, e)) * float(sigma)
        r = sx.ratio(Y0s.reshape(c.N, c.HNu)[list(rows)], want)
        print(f"{what}: max |Y0s - float64| / |float64| = {r:.3g}")
        assert r < sx.RTOL, f"{what}: max |Y0s - float64| / |float64| = {r:.3g}"
        return r

    def close(self):
        self.plan.close()


def _run(gpu, orc, c, monkeypatch, levers):
    s = _Sampler(gpu, orc, c, monkeypatch, levers)
    try:
        assert bool(c.lazy) == (c.form in ("noise", "fused"))
        key = gpu.prng_key(KEY_SEED + c.N)
        for saturating in (False, True):
            i, sigma = s.sigma(saturating)
            Ybar = s.ybar(saturating, seed=c.N)
            s.sample_rollout(i, key, Ybar)
            s.compare(key, sigma, Ybar, saturating, f"{c.id} {'saturating' if saturating else 'plain'}")
            key = gpu.prng_key(KEY_SEED + c.N + 7)
    finally:
        s.close()


def _ids(cs):
    return [c.id for c in cs]


@pytest.mark.parametrize("c", sx.cases("whole"), ids=_ids(sx.cases("whole")))
def test_sample_kernel_whole_tensor(gpu, orc, c, monkeypatch, levers):
    """sample_kernel over the whole tensor — one thread per pair in the legacy layout (element j with j + half, an odd total's
    last pair padded with counter 0), one per element in the partitionable — with sigma from the host (car2d MBD plans,
    rigid-body MBD plans under MBD_NO_LAZY) and from the device (path-integral plans): totals of 1, 2 and 3, one workgroup of
    thread-items exactly / one fewer / one more, odd totals, rows coprime to 256."""
    _run(gpu, orc, c, monkeypatch, levers)


@pytest.mark.parametrize("c", sx.cases("three_range"), ids=_ids(sx.cases("three_range")))
def test_sample_kernel_three_ranges_of_a_sharded_plan(gpu, orc, c, monkeypatch, levers):
    """A sharded materialised plan with N >= 5 shard_count: its own rows on the step's stream, [0, own0) and [own1, total) on
    the second — the sub-range branch of sample_kernel (legacy: j0 = e < half ? e : e - half), with own rows below, above and
    across `half`, an empty first and an empty last range, odd and even totals, ranges of many workgroups that start off a
    multiple of 256.  peek returns all N rows: the three launches must tile the tensor."""
    assert len(sx.spans(c)) >= 2
    _run(gpu, orc, c, monkeypatch, levers)


@pytest.mark.parametrize("c", sx.cases("one_range"), ids=_ids(sx.cases("one_range")))
def test_sample_kernel_sharded_plan_in_one_launch(gpu, orc, c, monkeypatch, levers):
    """The same shards on the other side of the host's switch (N = 5 shard_count - 1) and under MBD_NO_AUX: one whole-tensor
    launch on the step's stream."""
    assert sx.spans(c) == [(0, c.total, 0)]
    _run(gpu, orc, c, monkeypatch, levers)


@pytest.mark.parametrize("c", sx.cases("noise", large=False), ids=_ids(sx.cases("noise", large=False)))
def test_noise_kernel_and_shift_kernel(gpu, orc, c, monkeypatch, levers):
    """Lazy plans: noise_kernel writes the normals, shift_kernel forms Y0s at peek — the sampler's two roundings."""
    _run(gpu, orc, c, monkeypatch, levers)


@pytest.mark.parametrize("c", sx.cases("noise", large=True), ids=_ids(sx.cases("noise", large=True)))
def test_noise_kernel_at_its_grid_cap(gpu, orc, c, monkeypatch, levers):
    """noise_kernel's grid is capped at 65 536 workgroups and strides beyond: thread-items exactly at the cap and one row
    above it, per layout (33.6 million elements; every one compared with the checker, the rows at the ends and around
    `half` and a stride of rows with the float64 restatement)."""
    _run(gpu, orc, c, monkeypatch, levers)


@pytest.mark.parametrize("saturating", [False, True], ids=["plain", "saturating"])
@pytest.mark.parametrize("c", sx.cases("fused"), ids=_ids(sx.cases("fused")))
def test_prefetched_normals(gpu, orc, c, saturating, monkeypatch, levers):
    """The NEXT step's normals, declared with mbd_plan_prefetch_noise and generated beside the rollout: by the noise
    workgroups of the launch — plain (need below and above the spare CUs) and XCD-pinned (index (q 7 + r - 1), stride 7
    roll_blocks; at most 8 workgroups, and 9 to 32 under MBD_ROLL_PIN=1) — or by noise_kernel on the second stream
    (MBD_NO_FUSED_NOISE; a one-workgroup shard, whose 7 noise workgroups would be too few).  Three steps with other keys run
    first, so that every buffer of the ring holds another key's normals; then key B is declared, a step runs with key A, and
    the step after it asks for key B: its candidates are the checker's for key B, every element."""
    s = _Sampler(gpu, orc, c, monkeypatch, levers)
    try:
        i = sx.I_LARGE if saturating else sx.I_SMALL + 1
        keys = [gpu.prng_key(KEY_SEED + c.N + k) for k in range(5)]
        for k in range(3):
            Ybar = s.ybar(True, seed=k)
            d_Y = s.sample_rollout(sx.I_LARGE, keys[k], Ybar)
            s.score_update(sx.I_LARGE, keys[k], d_Y)
        A, B = keys[3], keys[4]
        s.prefetch(B)
        d_Y = s.sample_rollout(i, A, s.ybar(True, seed=3))
        s.score_update(i, A, d_Y)
        Ybar = s.ybar(saturating, seed=4)
        s.sample_rollout(i - 1, B, Ybar)
        s.compare(B, np.float32(s.sched[2][i - 1]), Ybar, saturating, f"{c.id} {'saturating' if saturating else 'plain'}")
    finally:
        s.close()


def _chain(gpu, orc, c, monkeypatch, levers, steps, wait):
    """`steps` diffusion steps of the case's plan from Ybar = 0, every next key declared, on fixed "gathered" rewards: the
    list of the Ybars.  wait: the caller synchronises after every step; otherwise it never waits for the device."""
    import torch
    s = _Sampler(gpu, orc, c, monkeypatch, levers)
    try:
        keys = [gpu.prng_key(KEY_SEED + c.N + 100 + k) for k in range(steps)]
        bufs = [torch.zeros(c.HNu, device="cuda") for _ in range(steps + 1)]
        torch.cuda.synchronize()
        lib, h = s.plan.lib, s.plan.h
        for k, i in enumerate(range(sx.I_LARGE, sx.I_LARGE - steps, -1)):
            if k + 1 < steps:
                s.prefetch(keys[k + 1])
            ks = gpu.key_array(keys[k])
            gpu.check(lib.mbd_plan_sample_rollout(h, i, ks, bufs[k].data_ptr(), s.loc.data_ptr(), None, None))
            gpu.check(lib.mbd_plan_score_update(h, i, ks, bufs[k].data_ptr(), s.all.data_ptr(), None, bufs[k + 1].data_ptr(),
                                                s.rm.data_ptr(), None))
            if wait:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        return [b.cpu().numpy() for b in bufs[1:]]
    finally:
        s.close()


@pytest.mark.parametrize("c", sx.cases("fused"), ids=_ids(sx.cases("fused")))
def test_prefetched_normals_for_a_caller_that_never_waits(gpu, orc, c, monkeypatch, levers):
    """The ring of three buffers under a caller that enqueues step after step without waiting (the sharded step loop with
    an asynchronous exchange): the normals of step k + 1 are written beside the rollout of step k into the buffer the weighted
    mean of step k - 2 read — which may not have run yet.  Twelve steps (the ring wraps four times) on fixed rewards: the
    Ybars equal those of the same plan stepped with a synchronisation after every step, bit for bit.  (The regression test of
    the one-workgroup shard, N = 1100: its pinned launch cannot take the noise job, and before `rollout_takes_noise` the plan
    sent the job to the second stream without ordering it behind that weighted mean — these two cases differed.)"""
    steps = 12
    ref = _chain(gpu, orc, c, monkeypatch, levers, steps, wait=True)
    got = _chain(gpu, orc, c, monkeypatch, levers, steps, wait=False)
    assert all(np.isfinite(r).all() for r in ref)
    for k in range(steps):
        same_bits(got[k], ref[k], f"{c.id}: Ybar after step {k}")
    assert not np.array_equal(ref[0], ref[1])


@pytest.mark.parametrize("layout", sx.LAYOUTS, ids=["legacy", "part"])
@pytest.mark.parametrize("name,N,H,steps,kind", sx.SWEEPS, ids=[f"{s[4]}-{s[0]}-N{s[1]}" for s in sx.SWEEPS])
def test_batched_samplers_above_their_grid_cap(gpu, name, N, H, steps, kind, layout, monkeypatch):
    """noise_batch_kernel (MBD sweeps) and sample_batch_kernel (path-integral sweeps) stride over a grid capped at 4096
    workgroups per plan.  Two plans of a size above 4096 x 256 thread-items in both layouts — the path-integral one at an odd
    total — as ONE sweep against the same plans run alone (whose noise_kernel / sample_kernel launches, far below their own
    cap at this size, are held to the checker above): means of every step, mean rewards, final rewards, bit for bit."""
    monkeypatch.setenv("MBD_THREEFRY_PARTITIONABLE", str(layout))
    from mbd_hip.planners import path_integral
    from mbd_hip.planners.mbd_planner import Args, Plan, Sweep
    env, P = _env(name), 2
    items = N * H * env.action_size if layout == sx.PARTITIONABLE else (N * H * env.action_size + 1) // 2
    assert items > sx.BATCH_CAP
    if kind == "mbd":
        um, args = 0, Args(env_name=name, Nsample=N, Hsample=H, Ndiffuse=steps + 1, temp_sample=0.1, disable_recommended_params=True,
                           not_render=True)
    else:
        um, args = 1, path_integral.Args(env_name=name, Nsample=N, Hsample=H, Nrefine=steps + 1, temp_sample=0.1,
                                         disable_recommended_params=True)
    keys = np.array([gpu.prng_key(50 + k) for k in range(P)], np.uint32)
    states = [env.reset(gpu.prng_key(k)) for k in range(P)]
    sw = Sweep(env, args, P, update_method=um)
    for k in range(P):
        sw.set_state0(k, states[k])
    mu, rm, rf, _ = sw.run(keys)
    sw.close()
    assert np.isfinite(mu).all() and np.isfinite(rm).all()
    for k in range(P):
        p = Plan(env, args, update_method=um)
        p.set_state0(states[k])
        mu1, rm1, rf1, _ = p.run(keys[k])
        p.close()
        same_bits(mu[k], mu1, f"{name} {kind} plan {k}: means")
        same_bits(rm[k], rm1, f"{name} {kind} plan {k}: mean rewards")
        same_bits(np.float32(rf[k]), np.float32(rf1), f"{name} {kind} plan {k}: final reward")
    assert not np.array_equal(mu[0], mu[1])


@pytest.mark.parametrize("layout", sx.LAYOUTS, ids=["legacy", "part"])
@pytest.mark.parametrize("E", sx.PLANT_E)
def test_plant_rows_either_side_of_one_workgroup(gpu, orc_omp, E, layout, monkeypatch):
    """mpc_plant_rows_kernel draws the E Nu + 3 normals of a tick's disturbances with ONE workgroup of 256 threads: its
    noise_fill wraps above 256 elements (partitionable) and above 512 (legacy pairs).  humanoidrun, Nu = 17: E = 14, 15, 29,
    30 give 241, 258, 496 and 513 normals — odd and even counts — in disturbed episodes of three ticks against
    tests/mpc_plant_checker.py: executed actions, rewards, states and means, bit for bit."""
    monkeypatch.setenv("MBD_THREEFRY_PARTITIONABLE", str(layout))
    from test_mpc_plant import _against_checker, _full
    det, ref = _against_checker(orc_omp, _full("humanoidrun", 64, H=50, Nd=6, K=2, E=E, T=3, seed=5))
    assert ref["actions"].shape == (3 * E, 17) and np.isfinite(ref["states"]).all()
