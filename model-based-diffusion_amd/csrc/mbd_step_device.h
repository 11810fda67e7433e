// mbd_step_device.h — what the two kernel headers (mbd_step_kernels.h, mbd_record_kernels.h) and the host code around them share:
// launch constants and host-and-device functions that a kernel of one header and a kernel, a launch or a host reference
// (mbd_debug_*_host) of another unit both use.  It defines NO kernel, so every unit may see it (mbd_internal.h includes it): a
// function nothing in a unit calls leaves nothing in that unit's code object.  Each block keeps the comment it had beside its kernel.
#pragma once

#include "mbd_kernels.h"
#include "mbd_step_args.h"

namespace mbd {

// ---- the noise basis: knot_noise_kernel's column (mbd_step_kernels.h) ----
// One column (n, a) = col of the N Nu: its `knots` normals through the slots drawn[0], drawn[slot_stride], ... and the walk over
// the H rows.  Host and device: mbd_debug_knot_noise_host runs this same text on the CPU, where a test without a device holds
// the indexing to the checker.
MBD_HD void knot_column(uint32_t k0, uint32_t k1, int impl, uint64_t size, int H, int Nu, int knots,
                        const float* __restrict__ W, const float* __restrict__ g, float* __restrict__ z, uint64_t col,
                        float* drawn, int slot_stride) {
  const uint64_t n = col / (uint64_t)Nu;
  const uint32_t a = (uint32_t)(col - n * (uint64_t)Nu);
  for (int k = 0; k < knots; ++k) {
    const uint64_t j = (n * (uint64_t)knots + (uint64_t)k) * (uint64_t)Nu + a;  // flat element of the knot tensor
    drawn[k * slot_stride] = bits_to_normal(random_bits32(k0, k1, impl, j, size));
  }
  float eps[MBD_MAX_KNOTS];
#pragma unroll
  for (int k = 0; k < MBD_MAX_KNOTS; ++k) eps[k] = k < knots ? drawn[k * slot_stride] : 0.0f;
  float* __restrict__ out = z + n * (uint64_t)H * (uint64_t)Nu;  // candidate n's [H][Nu]; the column's element of row h is h Nu + a
  for (int h = 0; h < H; ++h) {
    const float* __restrict__ Wh = W + (size_t)h * knots;
    float c = 0.0f;
#pragma unroll
    for (int k = 0; k < MBD_MAX_KNOTS; ++k) {
      if (k < knots) {  // (wave-uniform, like the weight)
        const float w = Wh[k];
        if (w != 0.0f) c = c + w * eps[k];
      }
    }
    const uint32_t r = (uint32_t)h * (uint32_t)Nu + a;
    out[r] = g ? c * g[r] : c;
  }
}

// threads of the one-workgroup kernels — score, weigh, pick, elite selection — and of their reductions (mbd_step_kernels.h block_sum)
constexpr int kScoreThreads = 1024;

// ---- the weighting record: weigh_kernel's arithmetic (mbd_step_kernels.h; mbd_plan_set_weighting, include/mbd_hip.h mbd_weighting; DESIGN.md section 1 "N14 weighting"): the
// candidates' rewards -> weights[N] with non-finite rewards left out and the temperature chosen per step by the effective sample
// size; under a record it stands where score_kernel stands, and the step takes the kernels that consume given weights ----
// The arithmetic of one entry and of the selection is the functions below, host and device text: the kernel's threads run them
// between the block reductions, mbd_debug_weighting_host runs them on the CPU between restatements of those reductions over the
// 1024 virtual threads.  f32, every operation rounded (the build's -ffp-contract=off); the one fused operation is the squared
// deviation's accumulation, score_block's own, which the bits of a step without a record oblige.
// decided on the bits (exponent all ones), not by a compare a fast-math flag could fold
MBD_HD bool weigh_keep(float r, int reject) { return !reject || (__builtin_bit_cast(uint32_t, r) & 0x7f800000u) != 0x7f800000u; }
MBD_HD float weigh_dev(float part, float r, float mean) {
  const float d = r - mean;
  return ffma(d, d, part);
}
MBD_HD float weigh_sd(float sumsq, int kept) {
  const float sd = fsqrt(sumsq / (float)kept);
  return sd < 1e-4f ? 1.0f : sd;  // (under a record every update method has the guard)
}
MBD_HD float weigh_z(float r, float mean, float sd) { return (r - mean) / sd; }
// ((r - mean) / sd) / T and the maximum through the largest reward: score_block's three operations, so the maximal entry is exp_(0) = 1
MBD_HD float weigh_e(float z, float zmax, float T) { return exp_(z / T - zmax / T); }
MBD_HD float weigh_ess(float S1, float S2) { return (S1 * S1) / S2; }
// T*: ess_at(T) is one pass over the kept entries (E(T) of the contract).  Both clamps and the loop compare with `!(a < b)` forms, so
// a NaN ess ends at a clamp instead of walking the loop.
template <class Ess>
MBD_HD float weigh_select(const WeighRec& R, float T0, int kept, Ess&& ess_at) {
  if (R.ess_frac == 0.0f) return T0;
  const float target = R.ess_frac * (float)kept;
  if (!(ess_at(R.temp_min) < target)) return R.temp_min;
  if (!(ess_at(R.temp_max) > target)) return R.temp_max;
  float lo = R.temp_min, hi = R.temp_max;
  for (int k = 0; k < R.iters; ++k) {
    const float mid = fsqrt(lo * hi);
    if (ess_at(mid) < target) lo = mid; else hi = mid;
  }
  return hi;
}

// ---- the weighted mean's decomposition (mbd_step_kernels.h wmean_kernel; adapt_spread_kernel takes the same): a workgroup owns
// kWmE consecutive outputs and splits the candidates into kWmG groups ----
constexpr int kWmE = 16, kWmG = 64;
// XCD-aware tile order.  Workgroups are dispatched round-robin over the chip's 8 XCDs — each with its own L2 — in the order
// of their linear index; a tile of 16 outputs reads 64-byte row segments, HALF a 128-byte line, so the tile next door wants
// the same lines again.  The workgroups that land on one XCD therefore take CONSECUTIVE tiles and the shared lines meet
// in one L2 instead of being fetched by two (PMC, round 4: 3.0x the algorithmic bytes per launch with tile = blockIdx.x).
// x: index within the row of n workgroups, first: linear index of the row's first workgroup (sweeps: blockIdx.y * n).
// A bijection on [0, n); which workgroup computes which outputs does not change their values.
__device__ __forceinline__ int xcd_tile(int x, int n, int first) {
  const int c = (first + x) & 7;
  int start = 0;
  for (int d = 0; d < 8; ++d) {
    if (d == c) break;
    const int x0 = (d - first) & 7;  // the first workgroup of the row on XCD d
    start += x0 < n ? (n - 1 - x0) / 8 + 1 : 0;
  }
  return start + (x - ((c - first) & 7)) / 8;
}

// ---- the order of the pick record's argmax (mbd_record_kernels.h), which the elite record's selection takes too ----
// finite on the bits (exponent not all ones), as weigh_keep decides it
MBD_HD bool pick_finite(float r) { return (__builtin_bit_cast(uint32_t, r) & 0x7f800000u) != 0x7f800000u; }
// whether the pair (v, i) goes in front of (bv, bi): i < 0 is "none"; the larger value, among equal values (+0 == -0) the lower index
MBD_HD bool pick_before(float v, int i, float bv, int bi) { return i >= 0 && (bi < 0 || v > bv || (v == bv && i < bi)); }

// n* of one plan's rewards by the calling 1024-thread workgroup; every thread returns the same value.  Thread t walks
// i = t, t + 1024, ... ascending and replaces on strictly greater only; the butterfly and the scan over the sixteen wavefronts'
// pairs order by (value, lower index), which is a total order on pairs of distinct indices: whatever the combination order, the
// winner is the lowest index among the maxima
__device__ __forceinline__ int pick_argmax_block(const float* __restrict__ rews, int N, float* red_v, int* red_i) {
  const int tid = threadIdx.x;
  float bv = 0.0f;
  int bi = -1;
  for (int i = tid; i < N; i += kScoreThreads) {
    const float x = rews[i];
    const bool take = pick_finite(x) && (bi < 0 || x > bv);
    bv = take ? x : bv;
    bi = take ? i : bi;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float ov = __shfl_xor(bv, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    const bool take = pick_before(ov, oi, bv, bi);
    bv = take ? ov : bv;
    bi = take ? oi : bi;
  }
  if ((tid & 63) == 0) { red_v[tid >> 6] = bv; red_i[tid >> 6] = bi; }
  __syncthreads();
  bv = red_v[0];
  bi = red_i[0];
#pragma unroll
  for (int w = 1; w < kScoreThreads / 64; ++w) {
    const float ov = red_v[w];
    const int oi = red_i[w];
    const bool take = pick_before(ov, oi, bv, bi);
    bv = take ? ov : bv;
    bi = take ? oi : bi;
  }
  return bi;
}

// ---- the adapt record's rule (AdaptRec keeps it by value; the kernels: mbd_record_kernels.h) ----
struct AdaptRule {
  float rate, a_min, a_max;
};

// ---- the elite record (the kernels: mbd_step_kernels.h) ----
// The arithmetic of one element and the order are the functions below, host and device text: mbd_debug_elites_host loops them on
// the CPU.  f32, every operation rounded.
constexpr int kEliteMax = 32;
// the normal that stands for an elite's element in a lazy plan: under a shape, a frozen element stays frozen
MBD_HD float elite_z(float Ej, float yb, float sigma, const float* __restrict__ g, int e) {
  return (g && g[e] == 0.0f) ? 0.0f : (Ej - yb) / sigma;
}
// the nominal's element: the normal +0 of a lazy plan, the clipped mean of a materialised one
MBD_HD float elite_nominal(float yb, int lazy) { return lazy ? 0.0f : fclip(yb, -1.0f, 1.0f); }
// a candidate's element as mbd_plan_peek forms it (pick_gather_kernel's)
MBD_HD float elite_value(float x, int lazy, float sigma, float yb) { return lazy ? fclip(x * sigma + yb, -1.0f, 1.0f) : x; }
// whether entry (x, i) can still be taken once (pv, pi) has been (pi < 0: nothing yet): finite, and strictly behind it in
// pick_before's order
MBD_HD bool elite_open(float x, int i, float pv, int pi) { return pick_finite(x) && (pi < 0 || pick_before(pv, pi, x, i)); }
// the selection on the host: k rounds, each the first open entry in the order.  Returns count'
static inline int elite_select_host(const float* r, int N, int k, int* src, float* R) {
  float pv = 0.0f;
  int pi = -1, cnt = 0;
  for (int j = 0; j < k; ++j) {
    float bv = 0.0f;
    int bi = -1;
    for (int i = 0; i < N; ++i)
      if (elite_open(r[i], i, pv, pi) && pick_before(r[i], i, bv, bi)) {
        bv = r[i];
        bi = i;
      }
    if (bi < 0) break;
    src[cnt] = bi;
    R[cnt] = bv;
    ++cnt;
    pv = bv;
    pi = bi;
  }
  return cnt;
}

// ---- the to-go record (the kernels: mbd_step_kernels.h) ----
// The layout and the arithmetic of the returns are the functions below, host and device text (mbd_debug_togo_host loops them on the
// CPU).  f32, every operation rounded.
// The starts are s_j = j block for every j >= 1 with H - j block >= min_tail (min_tail >= 1: then j block < H as well), a condition
// that holds for j = 1 .. (H - min_tail) / block and for no j beyond: G = 1 + (H - min_tail) / block, and s_j = j block for all j < G.
MBD_HD int togo_groups(int H, int block, int min_tail) { return 1 + (H - min_tail) / block; }
MBD_HD int togo_start(int j, int block) { return j * block; }
MBD_HD int togo_end(int j, int G, int H, int block) { return j + 1 < G ? (j + 1) * block : H; }
MBD_HD float togo_add(float acc, float r) { return acc + r; }
MBD_HD float togo_ret(float acc, int H, int s) { return acc / (float)(H - s); }
// One candidate's descending pass: acc = +0, acc += row[t] for t = H - 1 down to s_1 = block, and store(j, R_j) whenever t = s_j.
// Nothing is skipped: a NaN of step t is in acc for every t' <= t.  The loads of sixteen steps leave together, their adds follow in
// the contract's order.  Bounds: t runs over [block, H - 1] with block >= 1, j over [1, G - 1]; G = 1 runs no iteration.
template <class Store>
MBD_HD void togo_chain(const float* __restrict__ row, int H, int block, int G, Store&& store) {
  if (G < 2) return;
  float acc = 0.0f;
  int j = G - 1, s = togo_start(j, block);
  int t = H - 1;
  for (; t - 15 >= block; t -= 16) {
    float y[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) y[k] = row[t - k];
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_sched_barrier(0);
#endif
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      acc = togo_add(acc, y[k]);
      if (t - k == s) {
        store(j, togo_ret(acc, H, s));
        --j;
        s -= block;
      }
    }
  }
  for (; t >= block; --t) {
    acc = togo_add(acc, row[t]);
    if (t == s) {
      store(j, togo_ret(acc, H, s));
      --j;
      s -= block;
    }
  }
}

}  // namespace mbd
