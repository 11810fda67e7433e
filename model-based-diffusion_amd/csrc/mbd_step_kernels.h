// mbd_step_kernels.h — the kernels of a diffusion step around the rollout (mbd_planner.py:103-135): sampling / noise,
// score (standardise, demo blend, softmax), weighted mean + score update, their batched forms for sweeps, the tick boundaries, the
// path-integral update rules, and the kernels of the three records whose kernels share score_wmean_body or the samplers' buffers
// with a step (weighting, elites, to-go).  Non-template and `static`, so every unit that sees them emits them: only mbd_plan.hip
// and mbd_sweep.hip, which launch them, include this header; the four MBD_*_KERNEL guards keep a unit from emitting the kernels
// only the other one launches.  The other records' kernels are in mbd_record_kernels.h (mbd_records.hip's alone), mbd_env.hip's
// own in mbd_env_kernels.h; what this header and mbd_record_kernels.h share — constants, host-and-device functions — is in
// mbd_step_device.h, which defines no kernel.  The rollout kernels and what they share live in mbd_kernels.h.
#pragma once

#include "mbd_step_device.h"

namespace mbd {

// ---- A1: sampling (mbd_planner.py:103-106) -------------------------------------------------------------
// Y0s[e] for the flat elements [e_begin, e_begin + e_count) of the global [N][HNu] tensor (a rank's own rows
// first, the other ranks' rows on a second stream while the rollout runs).  Whole tensor, legacy layout: one
// thread per threefry block, which pairs element j with j+half (both outputs used).  Otherwise one thread per
// element (partitionable layout: its own block; legacy layout on a sub-range: the block it belongs to).
// g: the noise shape [HNu] (include/mbd_hip.h mbd_noise_shape) or nullptr — the normal of element e becomes
// z = eps * g[e mod HNu], rounded, before the two roundings above (shaped; g is wave-uniform, the index is Ybar's).
__device__ __forceinline__ float shaped(float eps, const float* __restrict__ g, uint64_t r) { return g ? eps * g[r] : eps; }
static __global__ __launch_bounds__(256) void sample_kernel(uint32_t k0, uint32_t k1, int impl, int N, int HNu,
                                                      unsigned long long e_begin, unsigned long long e_count,
                                                      float sigma_host, const float* __restrict__ sigma_dev,
                                                      const float* __restrict__ Ybar, float* __restrict__ Y0s,
                                                      const float* __restrict__ g) {
  const float sigma = sigma_dev ? *sigma_dev : sigma_host;  // path-integral plans carry sigma on the device
  const uint64_t size = (uint64_t)N * (uint64_t)HNu;
  const uint64_t half = (size + 1) / 2;
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (impl == 1) {
    if (tid >= e_count) return;
    const uint64_t e = e_begin + tid;
    uint32_t o0, o1;
    threefry2x32(k0, k1, (uint32_t)(e >> 32), (uint32_t)e, o0, o1);
    const uint64_t r = e % (uint64_t)HNu;
    float eps = shaped(bits_to_normal(o0 ^ o1), g, r);
    float y = eps * sigma + Ybar[r];
    Y0s[e] = fclip(y, -1.0f, 1.0f);
    return;
  }
  if (e_begin == 0 && e_count == size) {
    if (tid >= half) return;
    const uint64_t j1 = tid + half;
    uint32_t o0, o1;
    threefry2x32(k0, k1, (uint32_t)tid, j1 < size ? (uint32_t)j1 : 0u, o0, o1);
    {
      const uint64_t r = tid % (uint64_t)HNu;
      float y = shaped(bits_to_normal(o0), g, r) * sigma + Ybar[r];
      Y0s[tid] = fclip(y, -1.0f, 1.0f);
    }
    if (j1 < size) {
      const uint64_t r = j1 % (uint64_t)HNu;
      float y = shaped(bits_to_normal(o1), g, r) * sigma + Ybar[r];
      Y0s[j1] = fclip(y, -1.0f, 1.0f);
    }
    return;
  }
  if (tid >= e_count) return;
  const uint64_t e = e_begin + tid;
  const uint64_t j0 = e < half ? e : e - half, j1 = j0 + half;
  uint32_t o0, o1;
  threefry2x32(k0, k1, (uint32_t)j0, j1 < size ? (uint32_t)j1 : 0u, o0, o1);
  const uint64_t r = e % (uint64_t)HNu;
  float y = shaped(bits_to_normal(e < half ? o0 : o1), g, r) * sigma + Ybar[r];
  Y0s[e] = fclip(y, -1.0f, 1.0f);
}

// The sampler in two halves, for LAZY plans (RolloutParams): eps does not depend on the previous step's result, only
// the shift by Ybar does.
//   noise_kernel  eps = normal(key, (N, HNu)) — the threefry counters, layouts and the ErfInv polynomial of
//                 sample_kernel (grid-stride: any grid).  The same noise_fill runs in the noise workgroups of a rollout
//                 launch, which generate the NEXT step's normals on the CUs the rollout leaves idle.
//   shift_kernel  Y0s[e] = clip(eps[e] * sigma + Ybar[e mod HNu], -1, 1) — the same two roundings as sample_kernel;
//                 lazy plans form these values at the rollout's action fetch and inside the weighted mean instead, and
//                 run this kernel only when somebody asks for Y0s (mbd_plan_peek)
// (g: the noise shape or nullptr — noise_fill then stores z = eps * g[e mod HNu] and everything downstream is unchanged)
static __global__ __launch_bounds__(256) void noise_kernel(uint32_t k0, uint32_t k1, int impl, int N, int HNu,
                                                     float* __restrict__ eps, const float* __restrict__ g) {
  noise_fill(k0, k1, impl, (uint64_t)N * (uint64_t)HNu, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x,
             (uint64_t)gridDim.x * blockDim.x, eps, g, HNu);
}
// noise_fill's shaped loops with the index type chosen by the caller (mbd_debug_noise_shaped: the 64-bit instantiation, which
// the library itself takes only beyond 2^32 elements, held to the checker at a size a test can afford)
static __global__ __launch_bounds__(256) void noise_shaped_probe_kernel(uint32_t k0, uint32_t k1, int impl, int N, int HNu,
                                                                  float* __restrict__ eps, const float* __restrict__ g, int wide) {
  const uint64_t size = (uint64_t)N * (uint64_t)HNu, tid0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  if (wide) noise_fill_shaped<uint64_t>(k0, k1, impl, size, tid0, stride, eps, g, (uint32_t)HNu);
  else noise_fill_shaped<uint32_t>(k0, k1, impl, (uint32_t)size, (uint32_t)tid0, (uint32_t)stride, eps, g, (uint32_t)HNu);
}
// ---- the noise basis (include/mbd_hip.h mbd_noise_basis; DESIGN.md section 1 "N8 noise basis") -----------------------------
// z [N][H Nu], the layout of the buffers noise_fill writes, from eps = normal(key, (N, knots, Nu)):
//   z[n][h][a] = (sum over k ascending of W[h][k] * eps[n][k][a], from +0, product and sum rounded, zero weights left out)
//                * g[h][a] where there is a shape
// so that every consumer forms clip(z * sigma + Ybar) unchanged.  One thread per column (n, a), grid-stride over the N Nu
// columns from col0 by stride (any grid gives the same bits): it draws its `knots` normals — one threefry block each
// (random_bits32: the legacy layout pairs element j of the knot tensor with j + half, the thread keeps its half) — through a slot
// of LDS into registers (the draw is a loop, not sixteen copies of threefry and the ErfInv polynomial; the walk over the rows
// reads registers), then walks the H rows with W[h][k] wave-uniform: a scalar load, and a zero weight is a scalar branch around
// the term.  knots / H of the flat sampler's threefry + ErfInv work; a wavefront's stores of one row are runs of Nu floats
// (one per candidate it holds), which the H rows of the walk complete into whole lines in L2.  (The column itself, knot_column,
// is host and device text: mbd_step_device.h.)
constexpr int kKnotThreads = 64;
__device__ __forceinline__ void knot_fill(uint32_t k0, uint32_t k1, int impl, int N, int H, int Nu, int knots,
                                          const float* __restrict__ W, const float* __restrict__ g, float* __restrict__ z,
                                          uint64_t col0, uint64_t stride) {
  __shared__ float drawn[MBD_MAX_KNOTS * kKnotThreads];
  const uint64_t cols = (uint64_t)N * (uint64_t)Nu, size = cols * (uint64_t)knots;
  for (uint64_t col = col0; col < cols; col += stride)
    knot_column(k0, k1, impl, size, H, Nu, knots, W, g, z, col, drawn + threadIdx.x, kKnotThreads);
}
static __global__ __launch_bounds__(kKnotThreads) void knot_noise_kernel(uint32_t k0, uint32_t k1, int impl, int N, int H, int Nu,
                                                                   int knots, const float* __restrict__ W,
                                                                   const float* __restrict__ g, float* __restrict__ z) {
  knot_fill(k0, k1, impl, N, H, Nu, knots, W, g, z, (uint64_t)blockIdx.x * kKnotThreads + threadIdx.x,
            (uint64_t)gridDim.x * kKnotThreads);
}
// workgroups (of kKnotThreads) of a knot launch over N Nu columns; cap: 65536 for a plan, 1024 per plan of a sweep
inline unsigned knot_blocks(int N, int Nu, uint64_t cap) {
  const uint64_t blocks = ((uint64_t)N * (uint64_t)Nu + kKnotThreads - 1) / kKnotThreads;
  return (unsigned)(blocks < cap ? blocks : cap);
}
// the second half of a materialised step under a basis for the P plans of a sweep (blockIdx.y = plan): shift_kernel's two
// roundings with each plan's carried sigma and mean
static __global__ __launch_bounds__(256) void shift_batch_kernel(const float* __restrict__ z, int N, int HNu,
                                                           const float* __restrict__ sigma_dev /* [P] */,
                                                           const float* __restrict__ mu, long long mu_stride,
                                                           float* __restrict__ Y0s) {
  const uint64_t size = (uint64_t)N * (uint64_t)HNu, base = (uint64_t)blockIdx.y * size;
  const float sigma = sigma_dev[blockIdx.y];
  const float* __restrict__ Ybar = mu + (long long)blockIdx.y * mu_stride;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < size; e += (uint64_t)gridDim.x * blockDim.x) {
    const float y = z[base + e] * sigma + Ybar[e % (uint64_t)HNu];
    Y0s[base + e] = fclip(y, -1.0f, 1.0f);
  }
}
static __global__ __launch_bounds__(256) void shift_kernel(const float* __restrict__ eps, int HNu, unsigned long long e_begin,
                                                     unsigned long long e_count, float sigma_host,
                                                     const float* __restrict__ sigma_dev,
                                                     const float* __restrict__ Ybar, float* __restrict__ Y0s) {
  const float sigma = sigma_dev ? *sigma_dev : sigma_host;
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= e_count) return;
  const uint64_t e = e_begin + tid;
  float y = eps[e] * sigma + Ybar[e % (uint64_t)HNu];
  Y0s[e] = fclip(y, -1.0f, 1.0f);
}

// The boundary between two ticks of a receding-horizon episode (mbd_plan_run_mpc), one workgroup, behind the rollout that
// executed the tick's first E rows: the next tick's starting mean Ybar_K = shift_E(M) — M [H][Nu] moved E rows forward,
// the vacated last E rows zero (the cold plan's prior) — and the episode's logs of M and of s_next, the state the executed
// rows reached (it stays where it is: the host hands that buffer to the next tick's rollouts).  shift = E * Nu floats.
constexpr int kLinkVel = MBD_LINK_VEL;  // link 0's linear velocity inside a state (include/mbd_hip.h)
// (kick: the three values a tick's kick adds to link 0's linear velocity — floats kLinkVel .. kLinkVel + 2 of the state —
// before s_next is logged and before the next tick reads it, planar models leaving the y component alone; nullptr: no kick.)
__device__ __forceinline__ void mpc_boundary_body(const float* __restrict__ M, int HNu, int shift, float* s_next, int S,
                                                  const float* __restrict__ kick, int planar, float* __restrict__ ybar_next,
                                                  float* __restrict__ means_log, float* __restrict__ states_log) {
  for (int e = threadIdx.x; e < HNu; e += blockDim.x) {
    means_log[e] = M[e];
    ybar_next[e] = e < HNu - shift ? M[e + shift] : 0.0f;
  }
  for (int e = threadIdx.x; e < S; e += blockDim.x) {
    float v = s_next[e];
    const int j = e - kLinkVel;
    if (kick && j >= 0 && j < 3 && !(planar && j == 1)) {
      v = v + kick[j];
      s_next[e] = v;
    }
    states_log[e] = v;
  }
}
static __global__ __launch_bounds__(256) void mpc_boundary_kernel(const float* __restrict__ M, int HNu, int shift,
                                                            const float* __restrict__ s_next, int S,
                                                            float* __restrict__ ybar_next, float* __restrict__ means_log,
                                                            float* __restrict__ states_log) {
  mpc_boundary_body(M, HNu, shift, const_cast<float*>(s_next), S, nullptr, 0, ybar_next, means_log, states_log);
}
// mpc_boundary_kernel of a tick that ends with a kick (mbd_mpc_plant; single plan)
static __global__ __launch_bounds__(256) void mpc_boundary_kick_kernel(const float* __restrict__ M, int HNu, int shift, float* s_next,
                                                                 int S, const float* __restrict__ kick, int planar,
                                                                 float* __restrict__ ybar_next, float* __restrict__ means_log,
                                                                 float* __restrict__ states_log) {
  mpc_boundary_body(M, HNu, shift, s_next, S, kick, planar, ybar_next, means_log, states_log);
}

// The same boundary for the P lockstep episodes of a sweep (mbd_sweep_run_mpc), blockIdx.y = episode, one workgroup each, in
// FRONT of the rollout that executes the tick's first E rows: episode k's M (M_stride floats apart: the last slot of its
// means) goes into the tick's slice of the means log [P][HNu], its first `shift` = E * Nu floats into the compact rows
// [P][shift] that rollout reads as one candidate per episode, and shift_E(M) into the next tick's first Ybar [P][HNu].  (The
// states need no copy: that rollout writes s_next of every episode into the state log itself.)
static __global__ __launch_bounds__(256) void mpc_boundary_batch_kernel(const float* __restrict__ M, long long M_stride, int HNu,
                                                                  int shift, float* __restrict__ ybar_next,
                                                                  float* __restrict__ means_log, float* __restrict__ rows) {
  const long long k = blockIdx.y;
  M += k * M_stride; ybar_next += k * HNu; means_log += k * HNu; rows += k * shift;
  for (int e = threadIdx.x; e < HNu; e += blockDim.x) {
    const float m = M[e];
    means_log[e] = m;
    if (e < shift) rows[e] = m;
    ybar_next[e] = e < HNu - shift ? M[e + shift] : 0.0f;
  }
}

// The boundaries of an episode with a delay record (include/mbd_hip.h mbd_mpc_delay): the executed rows were the head C[0] of
// the committed queue C [D][shift] (Q = D * shift floats), not M's.  In the same launch the queue advances into its other
// buffer — q_out = C[1:] ++ M[0:shift]; two buffers, so that no thread overwrites what another has yet to read and the
// launches around this one may still read q_in — and the executed block C[0] goes into the tick's slice of the log of
// executed rows (exec_log; nullptr where mpc_plant_rows_kernel has already written the disturbed rows there).  Copies
// throughout: -0.0 stays -0.0.
__device__ __forceinline__ void mpc_queue_advance(const float* __restrict__ M, int shift, const float* __restrict__ q_in,
                                                  float* __restrict__ q_out, int Q, float* __restrict__ exec_log) {
  const int keep = Q - shift;
  for (int e = threadIdx.x; e < Q; e += blockDim.x) q_out[e] = e < keep ? q_in[e + shift] : M[e - keep];
  if (exec_log)
    for (int e = threadIdx.x; e < shift; e += blockDim.x) exec_log[e] = q_in[e];
}
static __global__ __launch_bounds__(256) void mpc_boundary_delay_kernel(const float* __restrict__ M, int HNu, int shift,
                                                                  const float* __restrict__ s_next, int S,
                                                                  float* __restrict__ ybar_next, float* __restrict__ means_log,
                                                                  float* __restrict__ states_log,
                                                                  const float* __restrict__ q_in, float* __restrict__ q_out,
                                                                  int Q, float* __restrict__ exec_log) {
  mpc_boundary_body(M, HNu, shift, const_cast<float*>(s_next), S, nullptr, 0, ybar_next, means_log, states_log);
  mpc_queue_advance(M, shift, q_in, q_out, Q, exec_log);
}
static __global__ __launch_bounds__(256) void mpc_boundary_delay_kick_kernel(const float* __restrict__ M, int HNu, int shift,
                                                                       float* s_next, int S, const float* __restrict__ kick,
                                                                       int planar, float* __restrict__ ybar_next,
                                                                       float* __restrict__ means_log,
                                                                       float* __restrict__ states_log,
                                                                       const float* __restrict__ q_in,
                                                                       float* __restrict__ q_out, int Q,
                                                                       float* __restrict__ exec_log) {
  mpc_boundary_body(M, HNu, shift, s_next, S, kick, planar, ybar_next, means_log, states_log);
  mpc_queue_advance(M, shift, q_in, q_out, Q, exec_log);
}
// ... and mpc_boundary_batch_kernel's form (blockIdx.y = episode): the queues [P][Q]; rows [P][shift] — the compact rows the
// rollout of the executed rows reads, here the tick's slice of their log — takes C[0] (nullptr: mpc_plant_rows_kernel forms them
// from the queue heads)
static __global__ __launch_bounds__(256) void mpc_boundary_delay_batch_kernel(const float* __restrict__ M, long long M_stride,
                                                                        int HNu, int shift, float* __restrict__ ybar_next,
                                                                        float* __restrict__ means_log,
                                                                        const float* __restrict__ q_in,
                                                                        float* __restrict__ q_out, int Q,
                                                                        float* __restrict__ rows) {
  const long long k = blockIdx.y;
  M += k * M_stride; ybar_next += k * HNu; means_log += k * HNu;
  for (int e = threadIdx.x; e < HNu; e += blockDim.x) {
    means_log[e] = M[e];
    ybar_next[e] = e < HNu - shift ? M[e + shift] : 0.0f;
  }
  mpc_queue_advance(M, shift, q_in + k * Q, q_out + k * Q, Q, rows ? rows + k * shift : nullptr);
}

// The boundary of a SESSION's tick (include/mbd_hip.h mbd_plan_mpc_submit), one workgroup behind the tick's last weighted mean:
// nothing was executed on the device, so there is no state to log — the launch shifts M into the next tick's Ybar, advances the
// committed queue into its other buffer (q_in nullptr: no delay record) and hands the tick's results to the host by writing
// them straight into the mailbox `mb`, pinned host memory mapped into the device's address space, so a tick ends with no copy
// launch: rows = M[0:shift] | mean = M | head = C[0] (without a queue: M[0:shift]) | predicted [S] (pred nullptr: left alone) |
// rew_mean | the flag word.  The flag word is 1 iff some element of rows is not finite, decided on the bits (exponent all
// ones), not by a compare a fast-math flag could fold; an OR over the workgroup.  Copies throughout: -0.0 stays -0.0.  Plain
// vector stores and a system-scope fence; the host waits on an event recorded behind the launch, it does not spin on the memory.
struct SessionMailbox {
  float* rows;   // [shift]
  float* mean;   // [HNu]
  float* head;   // [shift]
  float* pred;   // [S]
  float* rew_mean;
  int* flag;
};
__device__ __forceinline__ void mpc_session_boundary_body(const float* __restrict__ M, int HNu, int shift,
                                                          float* __restrict__ ybar_next, const float* __restrict__ q_in,
                                                          float* __restrict__ q_out, int Q, const float* __restrict__ pred, int S,
                                                          const float* __restrict__ rew_mean, const SessionMailbox& mb) {
  int bad = 0;
  for (int e = threadIdx.x; e < HNu; e += blockDim.x) {
    const float m = M[e];
    mb.mean[e] = m;
    if (e < shift) {
      mb.rows[e] = m;
      mb.head[e] = q_in ? q_in[e] : m;
      bad |= (__float_as_uint(m) & 0x7f800000u) == 0x7f800000u;
    }
    ybar_next[e] = e < HNu - shift ? M[e + shift] : 0.0f;
  }
  if (q_in) mpc_queue_advance(M, shift, q_in, q_out, Q, nullptr);
  if (pred)
    for (int e = threadIdx.x; e < S; e += blockDim.x) mb.pred[e] = pred[e];
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) {
    *mb.rew_mean = *rew_mean;
    *mb.flag = bad ? 1 : 0;
  }
  __threadfence_system();
}
static __global__ __launch_bounds__(256) void mpc_session_boundary_kernel(const float* __restrict__ M, int HNu, int shift,
                                                                    float* __restrict__ ybar_next, const float* __restrict__ q_in,
                                                                    float* __restrict__ q_out, int Q, const float* __restrict__ pred,
                                                                    int S, const float* __restrict__ rew_mean, SessionMailbox mb) {
  mpc_session_boundary_body(M, HNu, shift, ybar_next, q_in, q_out, Q, pred, S, rew_mean, mb);
}

// ... and the boundary of a tick of a SWEEP's session (mbd_sweep_mpc_submit), blockIdx.y = episode: episode k's M lies M_stride
// floats from episode 0's, its queue at q + k Q, its predicted state at pred + k S, its mean reward rew_stride floats from episode
// 0's; the mailbox holds rows [P][shift] | means [P][HNu] | heads [P][shift] | predicted [P][S] | rew_mean [P] | flags [P].
static __global__ __launch_bounds__(256) void mpc_session_boundary_batch_kernel(const float* __restrict__ M, long long M_stride, int HNu,
                                                                          int shift, float* __restrict__ ybar_next,
                                                                          const float* __restrict__ q_in, float* __restrict__ q_out,
                                                                          int Q, const float* __restrict__ pred, int S,
                                                                          const float* __restrict__ rew_mean, int rew_stride,
                                                                          SessionMailbox mb) {
  const long long k = blockIdx.y;
  SessionMailbox m;
  m.rows = mb.rows + k * shift; m.mean = mb.mean + k * HNu; m.head = mb.head + k * shift; m.pred = mb.pred + k * S;
  m.rew_mean = mb.rew_mean + k; m.flag = mb.flag + k;
  mpc_session_boundary_body(M + k * M_stride, HNu, shift, ybar_next + k * HNu, q_in ? q_in + k * Q : nullptr,
                            q_in ? q_out + k * Q : nullptr, Q, pred ? pred + k * S : nullptr, S, rew_mean + k * rew_stride, m);
}

// ---- A4-A6: standardise, demo blend, softmax -> weights[N] (mbd_planner.py:110-127) -------------------
// The canonical one-wavefront reduction of the numerical contract: lane j accumulates the elements
// i = j, j+64, ... in increasing i, then a xor-butterfly over the 64 lanes.
__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x = x + __shfl_xor(x, off, 64);
  return x;
}
__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x = fmax_(x, __shfl_xor(x, off, 64));
  return x;
}
// ONE 1024-thread workgroup.  Reduction order of the contract ("sumB"): thread t accumulates
// i = t, t+1024, ... in increasing i; each wavefront runs the xor-butterfly; the 16 wavefront sums are added
// sequentially in wavefront order (every thread does that same sum from LDS).  (kScoreThreads = 1024: mbd_step_device.h)
__device__ __forceinline__ float block_sum(float x, float* red) {
  x = wave_sum(x);
  __syncthreads();  // red[] may still be read from the previous reduction
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  float s = red[0];
#pragma unroll
  for (int w = 1; w < kScoreThreads / 64; ++w) s = s + red[w];
  return s;
}
__device__ __forceinline__ float block_max(float x, float* red) {
  x = wave_max(x);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  float s = red[0];
#pragma unroll
  for (int w = 1; w < kScoreThreads / 64; ++w) s = fmax_(s, red[w]);
  return s;
}

// sum and max of two values in one pass over the barriers (red: 2 x 16 entries)
__device__ __forceinline__ void block_sum_max(float& xs, float& xm, float* red) {
  xs = wave_sum(xs);
  xm = wave_max(xm);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = xs;
    red[kScoreThreads / 64 + (threadIdx.x >> 6)] = xm;
  }
  __syncthreads();
  float s = red[0], m = red[kScoreThreads / 64];
#pragma unroll
  for (int w = 1; w < kScoreThreads / 64; ++w) {
    s = s + red[w];
    m = fmax_(m, red[kScoreThreads / 64 + w]);
  }
  xs = s;
  xm = m;
}

// The body of the score step for ONE 1024-thread workgroup: leaves exp(logp0 - max) of every candidate in lg[] (LDS
// or a global scratch; each thread only ever touches its own entries i = tid, tid + 1024, ...) and returns the softmax
// denominator; the caller divides.  Shared by score_kernel and by the fused score + weighted-mean kernel, whose
// every workgroup re-derives the weights — same code, same order, same bits.
template <bool REGS = true>  // REGS = false: the rewards are re-read per pass (sweeps: registers for two workgroups per CU)
__device__ __forceinline__ float score_block(const float* __restrict__ rews, const float* __restrict__ lp_demo, int N,
                                             float rew_xref, float temp, int std_guard, float* __restrict__ lg,
                                             float* red, float& rew_mean_out, float* early_mean = nullptr) {
  const int tid = threadIdx.x;
  // the rewards cross from memory ONCE (up to 8 per thread: plans up to 8192 candidates; the passes below are then
  // register arithmetic — as three reads of rews[] each pass paid an L2 round trip), and their maximum rides on the first
  // reduction: logp0 is a monotonic function of the reward (the same three correctly rounded operations for every
  // candidate), so max(logp0) = logp0(max reward) exactly — one reduction fewer for plans without the demonstration blend
  constexpr int RK = 8;
  const bool in_regs = REGS && N <= RK * kScoreThreads;  // (uniform)
  float r[RK];
#pragma unroll
  for (int k = 0; k < RK; ++k) r[k] = (in_regs && tid + k * kScoreThreads < N) ? rews[tid + k * kScoreThreads] : 0.0f;
  float part = 0.0f, rmax = -__builtin_inff();
  if (in_regs) {
#pragma unroll
    for (int k = 0; k < RK; ++k) {
      const bool ok = tid + k * kScoreThreads < N;
      part = ok ? part + r[k] : part;
      rmax = ok ? fmax_(rmax, r[k]) : rmax;
    }
  } else {
    for (int i = tid; i < N; i += kScoreThreads) { part = part + rews[i]; rmax = fmax_(rmax, rews[i]); }
  }
  block_sum_max(part, rmax, red);
  const float rew_mean = part / (float)N;
  // (the caller's early copy of the step's mean reward: a host that polls for it turns around ~5 us sooner)
  if (early_mean && tid == 0) __hip_atomic_store(early_mean, rew_mean, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  part = 0.0f;
  if (in_regs) {
#pragma unroll
    for (int k = 0; k < RK; ++k) {
      const float d = r[k] - rew_mean;
      part = tid + k * kScoreThreads < N ? ffma(d, d, part) : part;
    }
  } else {
    for (int i = tid; i < N; i += kScoreThreads) {
      float d = rews[i] - rew_mean;
      part = ffma(d, d, part);
    }
  }
  float rew_std = fsqrt(block_sum(part, red) / (float)N);
  rew_std = (std_guard && rew_std < 1e-4f) ? 1.0f : rew_std;  // mbd_planner.py:112; path_integral.py:123 has none
  if (in_regs) {
#pragma unroll
    for (int k = 0; k < RK; ++k)
      if (tid + k * kScoreThreads < N) lg[tid + k * kScoreThreads] = ((r[k] - rew_mean) / rew_std) / temp;
  } else {
    for (int i = tid; i < N; i += kScoreThreads) lg[i] = ((rews[i] - rew_mean) / rew_std) / temp;
  }
  if (lp_demo) {  // (each thread only ever touches its own lg[i]: no barrier needed around them)
    float mx = -__builtin_inff();
    for (int i = tid; i < N; i += kScoreThreads) mx = fmax_(mx, lp_demo[i]);
    mx = block_max(mx, red);
    part = 0.0f;
    for (int i = tid; i < N; i += kScoreThreads) {
      float lpd = ((((lp_demo[i] - mx) + rew_xref) - rew_mean) / rew_std) / temp;
      float v = lpd > lg[i] ? lpd : lg[i];
      lg[i] = v;
      part = part + v;
    }
    const float m = block_sum(part, red) / (float)N;
    part = 0.0f;
    for (int i = tid; i < N; i += kScoreThreads) {
      float d = lg[i] - m;
      part = ffma(d, d, part);
    }
    const float sd = fsqrt(block_sum(part, red) / (float)N);
    for (int i = tid; i < N; i += kScoreThreads) lg[i] = ((lg[i] - m) / sd) / temp;
  }
  float mx;
  if (lp_demo || !std_guard) {  // (without the guard a zero deviation makes logp0 NaN: keep the reduction's own answer)
    mx = -__builtin_inff();
    for (int i = tid; i < N; i += kScoreThreads) mx = fmax_(mx, lg[i]);
    mx = block_max(mx, red);
  } else {
    mx = ((rmax - rew_mean) / rew_std) / temp;
  }
  part = 0.0f;
  for (int i = tid; i < N; i += kScoreThreads) {
    float e = exp_(lg[i] - mx);
    lg[i] = e;
    part = part + e;
  }
  rew_mean_out = rew_mean;
  return block_sum(part, red);
}

// ---- ensembles (mbd_plan_set_ensemble): the members' rewards r [M][N] -> the candidates' rewards, in front of the score ----
// MEAN: ((r_0 + r_1) + ... + r_{M-1}) / float(M) — f32, left to right, one division; MIN: min(min(r_0, r_1), ...), left to
// right, NaN-propagating (min(a, b) = b if b < a or b is NaN, else a).  Two copies: the caller's buffer (what mbd_plan_score_update is handed) and the plan's own (mbd_plan_peek_ensemble).
static __global__ __launch_bounds__(256) void ensemble_reduce_kernel(const float* __restrict__ r, int M, int N, int risk,
                                                               float* __restrict__ out, float* __restrict__ keep) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float a = r[n];
  if (risk == MBD_RISK_MIN) {
    for (int m = 1; m < M; ++m) {  // (a NaN return wins: a member that diverged IS the worst case, and MEAN spreads it too)
      const float b = r[(size_t)m * N + n];
      a = (b < a || b != b) ? b : a;
    }
  } else {
    for (int m = 1; m < M; ++m) a = a + r[(size_t)m * N + n];
    a = a / (float)M;
  }
  out[n] = a;
  keep[n] = a;
}

// Sweeps of path-integral plans (mbd_sweep_*, update_method != 0): the small kernels of the update rules take blockIdx.y
// = plan and these strides (in elements) from plan 0's data; a single plan launches them with one row and zero strides.
struct PiBatch {
  long long rews = 0, weights = 0, mean = 0, cand = 0, mu = 0, out = 0, spread = 0, sigma = 0, idx = 0;
  const float* temps = nullptr;  // [P], or nullptr: every plan at the launch's `temp`
};
static __global__ __launch_bounds__(kScoreThreads) void score_kernel(const float* __restrict__ rews,
                                                              const float* __restrict__ lp_demo, int N,
                                                              float rew_xref, float temp, int std_guard,
                                                              float* __restrict__ weights,
                                                              float* __restrict__ rew_mean_out,
                                                              float* __restrict__ lg_global, PiBatch pb) {
  const long long plan = blockIdx.y;
  rews += plan * pb.rews; weights += plan * pb.weights; rew_mean_out += plan * pb.mean;
  if (lp_demo) lp_demo += plan * pb.rews;
  if (pb.temps) temp = pb.temps[plan];
  // logp0 [N]: in LDS while it fits (every plan of the reference's sizes), in a plan-owned global scratch beyond
  // (each thread only ever touches its own entries, so the scratch needs no synchronisation either)
  extern __shared__ __attribute__((aligned(16))) float lg_lds[];
  float* __restrict__ lg = lg_global ? lg_global : lg_lds;
  __shared__ float red[2 * (kScoreThreads / 64)];
  float rew_mean;
  const float den = score_block<true>(rews, lp_demo, N, rew_xref, temp, std_guard, lg, red, rew_mean);
  for (int i = threadIdx.x; i < N; i += kScoreThreads) weights[i] = lg[i] / den;
  if (threadIdx.x == 0) *rew_mean_out = rew_mean;
}

// ---- A7-A8: weighted mean + score update (mbd_planner.py:128-133) ---------------------------------------
// A workgroup owns kWmE = 16 consecutive outputs e of [H][Nu] and splits the candidates into 64 groups:
// thread (g, j) runs a sequential fma over n = g, g+64, ... for output j (a wavefront reads four 64-byte row
// segments per load instruction); the 64 partials of an output are then added sequentially in g
// ("wsum64" of the contract).  ceil(HNu/16) workgroups of 1024 threads: every load of a thread is in flight at once.
// (kWmE, kWmG and the XCD-aware tile order, xcd_tile: mbd_step_device.h)
static __global__ __launch_bounds__(kWmE * kWmG) void wmean_kernel(const float* __restrict__ weights,
                                                            const float* __restrict__ Y0s, int N, int HNu,
                                                            const float* __restrict__ Ybar_i, float alpha_i,
                                                            float alpha_bar_i, float alpha_bar_im1, int literal,
                                                            float* __restrict__ Ybar_im1, int lazy, float sigma,
                                                            float* __restrict__ ybar_keep) {
  extern __shared__ __attribute__((aligned(16))) float wl[];  // the N weights: read once, shared by the 16 outputs
  __shared__ float red[kWmG][kWmE + 1];
  const int j = threadIdx.x & (kWmE - 1), g = threadIdx.x / kWmE;
  const int e_raw = xcd_tile(blockIdx.x, gridDim.x, 0) * kWmE + j;
  const int e = e_raw < HNu ? e_raw : HNu - 1;
  const float* __restrict__ col = Y0s + e;
  // lazy plans: Y0s holds the step's normals; the candidate value is formed here exactly as at the rollout's fetch
  const float yb = lazy ? Ybar_i[e] : 0.0f;
  auto val = [&](float x) { return lazy ? fclip(x * sigma + yb, -1.0f, 1.0f) : x; };
  for (int i = threadIdx.x; i < N; i += kWmE * kWmG) wl[i] = weights[i];
  __syncthreads();  // (plans of >= 4096 candidates take the row-major kernels below: N always fits here)
  float acc = 0.0f;
  int n = g;
  // the chain over n is sequential by contract, its loads are not: a thread keeps 32 rows of Y0s in flight while
  // there are that many, then 16, then the tail (the kernel is bound by memory round trips per batch, not by
  // bandwidth — multi-GPU plans average over all N_total candidates on every rank).  The scheduling barrier keeps
  // the compiler from interleaving loads and the dependent fma chain at a shallower depth.
  for (; n + 31 * kWmG < N; n += 32 * kWmG) {
    float y[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) y[k] = col[(size_t)(n + k * kWmG) * HNu];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < 32; ++k) acc = ffma(wl[n + k * kWmG], val(y[k]), acc);
  }
  for (; n + 15 * kWmG < N; n += 16 * kWmG) {
    float y[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) y[k] = col[(size_t)(n + k * kWmG) * HNu];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < 16; ++k) acc = ffma(wl[n + k * kWmG], val(y[k]), acc);
  }
  for (; n < N; n += kWmG) acc = ffma(wl[n], val(col[(size_t)n * HNu]), acc);
  red[g][j] = acc;
  __syncthreads();
  if (g != 0 || e_raw >= HNu) return;
  if (ybar_keep) ybar_keep[e] = Ybar_i[e];  // what mbd_plan_peek needs to materialise Y0s after the caller moved on
  float tot = red[0][j];
#pragma unroll 8
  for (int k = 1; k < kWmG; ++k) tot = tot + red[k][j];
  float out = tot;
  if (literal) {
    const float sab = fsqrt(alpha_bar_i);
    float Yi = Ybar_i[e] * sab;
    float t1 = 1.0f / (1.0f - alpha_bar_i);
    float t2 = sab * tot;
    float score = t1 * (-Yi + t2);
    float t3 = (1.0f - alpha_bar_i) * score;
    float Yim1 = (1.0f / fsqrt(alpha_i)) * (Yi + t3);
    out = Yim1 / fsqrt(alpha_bar_im1);
  }
  Ybar_im1[e] = out;
}

// Score + weighted mean in ONE launch (plans below 4096 candidates): every workgroup of the tile kernel above first
// re-derives the softmax weights from the N rewards — score_block, the code and order of score_kernel — straight into
// the LDS array the weighted mean reads them from; workgroup 0 also stores them and the step's mean reward.  A kernel
// of a few microseconds is mostly launch latency (an empty kernel takes 4 us on the timeline): one launch instead of
// two takes ~3.5 us off every step, and the rows of the candidates are already in flight while the weights are derived.
// V (round 5): outputs per thread — a workgroup owns 16 V CONSECUTIVE outputs (64 V bytes of every candidate row), thread
// (g, j) runs the V chains of outputs j V .. j V + V - 1 over its candidates n = g, g + 64, ...: the chains, their order and
// the order of the 64 partials are the contract's whatever V is (same bits).  What V changes is how many 128-byte lines a
// row segment shares with the tiles next door: a 64-byte segment touches 1.5 lines on average and shares each with a
// neighbour — when the neighbours drift apart in time and the line has left the L2 in between it is fetched twice (the sweep's
// batch form: 2.0x its algorithmic bytes, PMC round 4); a 256-byte segment touches 3 lines for 2 lines' worth of data:
// 1.5x at worst, whatever the L2 does.
// GIVEN (sweeps under a weighting record): weights_out already holds the plan's N weights — weigh_kernel's — and rew_mean_out its
// mean reward; the workgroups load them into wl[] in place of deriving them, and the chains below are the same text.
// SPAN (the to-go record's kernel, togo_update_kernel): the workgroup owns the outputs [e_base, e_base + 16 V) below e_lim <= HNu, a
// tile of one group's element range, in place of tile `tile` of the whole [0, HNu) — what rews, weights_out and writer mean is then
// per group.  Everything else is this text; without SPAN the two arguments are not read.
template <int ROUND, bool REGS, int V = 1, bool GIVEN = false, bool SPAN = false>  // rows in flight per round of the chain, score_block's REGS (48, true: one plan; sweeps: 32, false)
__device__ __forceinline__ void score_wmean_body(
    const float* __restrict__ rews, const float* __restrict__ lp_demo, int N, float rew_xref, float temp, int std_guard,
    float* __restrict__ weights_out, float* __restrict__ rew_mean_out, const float* __restrict__ Y0s, int HNu,
    const float* __restrict__ Ybar_i, float alpha_i, float alpha_bar_i, float alpha_bar_im1, int literal,
    float* __restrict__ Ybar_im1, int lazy, float sigma, float* __restrict__ ybar_keep, int tile, bool writer, int e_base = 0,
    int e_lim = 0) {
  // tile: which 16 outputs this workgroup owns (XCD-aware, xcd_tile / the batch kernel); writer: the one workgroup of the
  // plan that stores the weights and the mean reward (every workgroup derives the same values)
  static_assert(kWmE * kWmG == kScoreThreads, "score_block runs on the weighted mean's workgroup");
  extern __shared__ __attribute__((aligned(16))) float wl[];  // logp0, then the N weights
  __shared__ float red_s[2 * (kScoreThreads / 64)];
  __shared__ float red[kWmG][kWmE * V + 1];
  const int j = threadIdx.x & (kWmE - 1), g = threadIdx.x / kWmE;
  int e0;  // this thread's first output
  if constexpr (SPAN) e0 = e_base + j * V; else e0 = tile * (kWmE * V) + j * V;
  int e[V];
  float yb[V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    if constexpr (SPAN) e[v] = e0 + v < e_lim ? e0 + v : e_lim - 1; else e[v] = e0 + v < HNu ? e0 + v : HNu - 1;
    yb[v] = lazy ? Ybar_i[e[v]] : 0.0f;
  }
  auto val = [&](float x, int v) { return lazy ? fclip(x * sigma + yb[v], -1.0f, 1.0f) : x; };
  // the first rows of this thread's chains leave now and land while the weights are derived
  constexpr int PRE = 16 / V;
  const bool pre = g + (PRE - 1) * kWmG < N;
  float y0[PRE][V];
#pragma unroll
  for (int k = 0; k < PRE; ++k) {
#pragma unroll
    for (int v = 0; v < V; ++v) y0[k][v] = pre ? Y0s[(size_t)(g + k * kWmG) * HNu + e[v]] : 0.0f;
  }
  __builtin_amdgcn_sched_barrier(0);
  float rew_mean;
  // the step's mean reward may go to a pinned host slot the host is polling (per-step progress, mbd_planner.py:147):
  // a system-scope store leaves as soon as the first reduction has it — a plain one would sit in the cache until the
  // kernel ends — so the host turns around while the rest of the score and the weighted mean below run
  if constexpr (GIVEN) {
    for (int i = threadIdx.x; i < N; i += kScoreThreads) wl[i] = weights_out[i];
  } else {
    const float den = score_block<REGS>(rews, lp_demo, N, rew_xref, temp, std_guard, wl, red_s, rew_mean,
                                        writer ? rew_mean_out : nullptr);
    for (int i = threadIdx.x; i < N; i += kScoreThreads) {
      const float w = wl[i] / den;
      wl[i] = w;
      if (writer) weights_out[i] = w;
    }
  }
  __syncthreads();
  float acc[V];
#pragma unroll
  for (int v = 0; v < V; ++v) acc[v] = 0.0f;
  int n = g;
  if (pre) {  // (the chain over n is sequential by contract: the prefetched rows are its first terms)
#pragma unroll
    for (int k = 0; k < PRE; ++k) {
      const float w = wl[n + k * kWmG];
#pragma unroll
      for (int v = 0; v < V; ++v) acc[v] = ffma(w, val(y0[k][v], v), acc[v]);
    }
    n += PRE * kWmG;
  }
  // (a round = the rows in flight at once, then their dependent fma chain: large plans are bound by the number of rounds —
  // 48 rows per round: N = 4096 one round behind the prefetch instead of two, N = 8192 three instead of four)
  constexpr int RND = ROUND / V;
  for (; n + (RND - 1) * kWmG < N; n += RND * kWmG) {
    float y[RND][V];
#pragma unroll
    for (int k = 0; k < RND; ++k) {
#pragma unroll
      for (int v = 0; v < V; ++v) y[k][v] = Y0s[(size_t)(n + k * kWmG) * HNu + e[v]];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < RND; ++k) {
      const float w = wl[n + k * kWmG];
#pragma unroll
      for (int v = 0; v < V; ++v) acc[v] = ffma(w, val(y[k][v], v), acc[v]);
    }
  }
  constexpr int TAIL = 16 / V;
  for (; n + (TAIL - 1) * kWmG < N; n += TAIL * kWmG) {
    float y[TAIL][V];
#pragma unroll
    for (int k = 0; k < TAIL; ++k) {
#pragma unroll
      for (int v = 0; v < V; ++v) y[k][v] = Y0s[(size_t)(n + k * kWmG) * HNu + e[v]];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < TAIL; ++k) {
      const float w = wl[n + k * kWmG];
#pragma unroll
      for (int v = 0; v < V; ++v) acc[v] = ffma(w, val(y[k][v], v), acc[v]);
    }
  }
  for (; n < N; n += kWmG) {
    const float w = wl[n];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = ffma(w, val(Y0s[(size_t)n * HNu + e[v]], v), acc[v]);
  }
#pragma unroll
  for (int v = 0; v < V; ++v) red[g][j * V + v] = acc[v];
  __syncthreads();
  // the 16 V outputs of the tile, one per thread of the first 16 V threads: the 64 partials of an output in group order
  if ((int)threadIdx.x >= kWmE * V) return;
  const int jo = threadIdx.x;
  int eo;
  if constexpr (SPAN) eo = e_base + jo; else eo = tile * (kWmE * V) + jo;
  if (eo >= (SPAN ? e_lim : HNu)) return;
  if (ybar_keep) ybar_keep[eo] = Ybar_i[eo];
  float tot = red[0][jo];
#pragma unroll 8
  for (int k = 1; k < kWmG; ++k) tot = tot + red[k][jo];
  float out = tot;
  if (literal) {
    const float sab = fsqrt(alpha_bar_i);
    float Yi = Ybar_i[eo] * sab;
    float t1 = 1.0f / (1.0f - alpha_bar_i);
    float t2 = sab * tot;
    float score = t1 * (-Yi + t2);
    float t3 = (1.0f - alpha_bar_i) * score;
    float Yim1 = (1.0f / fsqrt(alpha_i)) * (Yi + t3);
    out = Yim1 / fsqrt(alpha_bar_im1);
  }
  Ybar_im1[eo] = out;
}
// XCD PINNING of the single-plan launches (round 5).  Workgroup i of a launch lands on XCD i mod 8.  A launch of T tiles is
// therefore made 8 ceil(T / X) workgroups long, and only those with (i mod 8) < X work — on tile (i mod 8) ceil(T / X) + i / 8
// — the others leave at once: the tiles of the launch then sit on X of the 8 XCDs, CONSECUTIVE tiles behind one L2, and a
// line of a candidate row that two tiles share is fetched from HBM once per XCD instead of once per tile.  X (host side,
// wmean_xcds): the fewest XCDs that give every tile a CU of its own (32 per XCD) and keep an XCD's share of the normals
// within its 4 MB L2.  hopper512's ten tiles sat on eight XCDs and read 3.3x their algorithmic bytes, the metric's 54 tiles
// 1.35x (seven tiles per XCD: 448 bytes of a row, plus a boundary line at each end).  -1: no such workgroup.
__device__ __forceinline__ int pinned_tile(int i, int T, int X) {
  const int c = i & 7, per = (T + X - 1) / X, t = c * per + (i >> 3);
  return (c < X && (i >> 3) < per && t < T) ? t : -1;
}
// V (round 6): outputs per thread of the single-plan launch, like the sweeps'.  Built to test the round-5 verdict's reading of
// the launch's extra traffic at large N (1.30x its algorithmic bytes at N = 8192, 1.15x at 4096) as half-line sharing between
// neighbouring tiles; MEASURED (profiles/r06_score_v1_ab.txt): V = 2 moves the bytes by 0 ... 3 % (36.3 -> 35.2 MB) and makes
// the kernel 45 ... 55 % SLOWER (27 workgroups in flight instead of 54: 15.5 -> 22.4 us at N = 4096, 25.3 -> 38.8 at 8192).
// The extra bytes are the XCD partition's boundary lines instead: a candidate's row is 3400 bytes — not a multiple of the
// 128-byte line — so the 448 bytes of a row that one XCD's seven tiles own (N = 8192: X = 8) start anywhere in a line and
// touch 4.5 lines on average for 3.5 lines of data, 1.29x; fourteen tiles (N = 4096: X = 4) 8 for 7, 1.14x — the measured
// ratios.  Only a row stride padded to whole lines would remove them (the normals' flat index would then no longer be their
// address: sampler, rollout fetch and the peek entries all change) — for a launch that is 3 % of a step.  V = 1 stays the
// library's choice at every size; MBD_WMEAN_V1 = 2 runs this form (same chains, same order, same bits).
template <int V>
static __global__ __launch_bounds__(kWmE * kWmG) void score_wmean_kernel(
    const float* __restrict__ rews, const float* __restrict__ lp_demo, int N, float rew_xref, float temp, int std_guard,
    float* __restrict__ weights_out, float* __restrict__ rew_mean_out, const float* __restrict__ Y0s, int HNu,
    const float* __restrict__ Ybar_i, float alpha_i, float alpha_bar_i, float alpha_bar_im1, int literal,
    float* __restrict__ Ybar_im1, int lazy, float sigma, float* __restrict__ ybar_keep, int T, int X) {
  const int tile = pinned_tile(blockIdx.x, T, X);
  if (tile < 0) return;  // (wave-uniform: the whole workgroup)
  score_wmean_body<48, true, V>(rews, lp_demo, N, rew_xref, temp, std_guard, weights_out, rew_mean_out, Y0s, HNu, Ybar_i, alpha_i,
                   alpha_bar_i, alpha_bar_im1, literal, Ybar_im1, lazy, sigma, ybar_keep, tile, tile == 0);
}
// SWEEPS (mbd_sweep_*): the same for P plans of one env in ONE launch — blockIdx.y is the plan, whose buffers sit at
// fixed strides (in floats) from plan 0's; temperatures may differ per plan (run_mbd.py:42-64).  The body is the
// single-plan kernel's: same code, same order, same bits.
struct ScoreBatch {
  long long rews, lp, weights, mean, cand, ybar_in, ybar_out, keep;
  const float* temps;  // [P], or nullptr: every plan at `temp`
};
// V = 1: eight wavefronts per SIMD — two workgroups per CU, 64 registers: the P x 54 workgroups of a sweep's step in one
// round (rounds 3-4).  V = 2 (round 5, the default for sweeps: mbd_sweep.hip wmean_batch_v): P x 27 workgroups of 32 outputs
// each, ONE per CU of plan k's XCD — they start together and stay together, a row segment is 128 bytes: the 2.0x of V = 1
// (plan k's 54 tiles, two to a CU, drifting apart behind XCD k's 4 MB L2 while 3.5 MB of normals stream through it) is gone:
// sweep8 28.2 MB per launch for 28.0 MB algorithmic, 11.3 us instead of 15.5 (profiles/r05_score_ab.txt).
template <int V, bool GIVEN = false>
static __global__ __launch_bounds__(kWmE * kWmG, V == 1 ? 8 : 4) void score_wmean_batch_kernel(
    const float* __restrict__ rews, const float* __restrict__ lp_demo, int N, float rew_xref, float temp, int std_guard,
    float* __restrict__ weights_out, float* __restrict__ rew_mean_out, const float* __restrict__ Y0s, int HNu,
    const float* __restrict__ Ybar_i, float alpha_i, float alpha_bar_i, float alpha_bar_im1, int literal,
    float* __restrict__ Ybar_im1, int lazy, float sigma, float* __restrict__ ybar_keep, ScoreBatch sb) {
  // Which plan and which tile: with a multiple of 8 plans, plan k's tiles all go to XCD k mod 8 (workgroups land on the
  // XCDs round-robin in linear order: the m-th workgroup of XCD c is linear index c + 8 m), so every line of a plan's
  // normals is fetched by ONE L2; otherwise each plan's row of workgroups gets the XCD-aware tile order of the
  // single-plan kernel.  A bijection on (plan, tile) either way; values do not depend on it.
  const int T = gridDim.x, P = gridDim.y;
  long long k = blockIdx.y;
  int tile = xcd_tile(blockIdx.x, T, blockIdx.y * T);
  if ((P & 7) == 0) {
    const int lin = blockIdx.y * T + blockIdx.x, c = lin & 7, m = lin >> 3;
    k = c + 8 * (m / T);
    tile = m % T;
  }
  score_wmean_body<32, false, V, GIVEN>(rews + k * sb.rews, lp_demo ? lp_demo + k * sb.lp : nullptr, N, rew_xref, sb.temps ? sb.temps[k] : temp,
                   std_guard, weights_out + k * sb.weights, rew_mean_out + k * sb.mean, Y0s + k * sb.cand, HNu,
                   Ybar_i + k * sb.ybar_in, alpha_i, alpha_bar_i, alpha_bar_im1, literal, Ybar_im1 + k * sb.ybar_out, lazy,
                   sigma, ybar_keep ? ybar_keep + k * sb.keep : nullptr, tile, tile == 0);
}
// the normals of P plans (one key each) in one launch: blockIdx.y is the plan
struct SweepKeys {
  uint32_t k[32][2];
};
// (g: the sweep's noise shape [HNu], one for all plans, or nullptr)
static __global__ __launch_bounds__(256) void noise_batch_kernel(SweepKeys keys, int impl, int N, int HNu, float* __restrict__ eps,
                                                           const float* __restrict__ g) {
  const uint64_t size = (uint64_t)N * (uint64_t)HNu;
  noise_fill(keys.k[blockIdx.y][0], keys.k[blockIdx.y][1], impl, size, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x,
             (uint64_t)gridDim.x * blockDim.x, eps + (uint64_t)blockIdx.y * size, g, HNu);
}
// knot_noise_kernel for the P plans of a sweep (blockIdx.y = plan): one basis and one shape for all, each plan its key
static __global__ __launch_bounds__(kKnotThreads) void knot_noise_batch_kernel(SweepKeys keys, int impl, int N, int H, int Nu,
                                                                         int knots, const float* __restrict__ W,
                                                                         const float* __restrict__ g, float* __restrict__ z) {
  knot_fill(keys.k[blockIdx.y][0], keys.k[blockIdx.y][1], impl, N, H, Nu, knots, W, g,
            z + (uint64_t)blockIdx.y * (uint64_t)N * (uint64_t)H * (uint64_t)Nu,
            (uint64_t)blockIdx.x * kKnotThreads + threadIdx.x, (uint64_t)gridDim.x * kKnotThreads);
}

// ---- the plant of a receding-horizon episode (include/mbd_hip.h mbd_mpc_plant): disturbances drawn and applied on the device ----
// One workgroup per episode, behind the tick's last weighted mean: eps = normal(d_t, (EN + 3,)) by noise_fill (the counters
// and layouts of every other normal of the library: bit-exact to the checker's; never shaped — a noise shape is the
// planner's exploration, the disturbances are the world's), then the executed rows
// rows[e] = M[e] + act_std * eps[e] — product and sum rounded separately, like every float32 expression of the library: the build
// compiles with -ffp-contract=off (the checker is numpy float32; the ISA shows v_mul_f32, then v_add_f32) — or M[e] itself where
// act_std == 0 (a copy: -0.0 stays -0.0), and the three kick values kick_std * eps[EN ..].  EN = E * Nu; M of episode k is M_stride floats further; eps [P][EN + 3] is scratch.
// M is wherever the undisturbed rows of the tick are: the tick's mean, or with a delay record (mbd_mpc_delay) the head of the
// committed queue, M_stride = D * EN floats apart.
static __global__ __launch_bounds__(256) void mpc_plant_rows_kernel(SweepPlant pl, int impl, const float* __restrict__ M,
                                                              long long M_stride, int EN, float* eps, float* __restrict__ rows,
                                                              float* __restrict__ kick) {
  const long long k = blockIdx.y;
  M += k * M_stride; eps += k * (EN + 3); rows += k * EN; kick += k * 3;
  const bool has = pl.has[k] != 0;  // (uniform over the workgroup)
  if (has) {
    noise_fill(pl.k[k][0], pl.k[k][1], impl, (uint64_t)(EN + 3), (uint64_t)threadIdx.x, (uint64_t)blockDim.x, eps);
    __syncthreads();  // (the normals are read back by other threads of this workgroup)
  }
  const float a = has ? pl.act_std[k] : 0.0f;
  for (int e = threadIdx.x; e < EN; e += blockDim.x) rows[e] = a == 0.0f ? M[e] : M[e] + a * eps[e];
  if (threadIdx.x < 3) kick[threadIdx.x] = has ? pl.kick_std[k] * eps[EN + threadIdx.x] : 0.0f;
}
// the kicks of a sweep's episodes, one workgroup per episode, behind the rollout(s) that wrote the tick's states [P][S] into
// the state log: episodes whose kick_std is 0 (no record, no kick, not in this tick) are left alone
static __global__ __launch_bounds__(64) void mpc_kick_batch_kernel(SweepPlant pl, float* __restrict__ states, int S,
                                                             const float* __restrict__ kick, int planar) {
  const long long k = blockIdx.y;
  const int j = threadIdx.x;
  if (!pl.has[k] || !(pl.kick_std[k] > 0.0f) || j >= 3 || (planar && j == 1)) return;
  float* v = states + k * S + kLinkVel + j;
  *v = *v + kick[k * 3 + j];
}

// the materialised candidates of P path-integral plans in one launch (blockIdx.y = plan; grid-stride over the thread-items
// of sample_kernel's whole-tensor forms — same counters, same two roundings): Y0s[k] = clip(eps_k * sigma[k] + mu[k], -1, 1);
// g: the sweep's noise shape or nullptr (sample_kernel's `shaped`)
static __global__ __launch_bounds__(256) void sample_batch_kernel(SweepKeys keys, int impl, int N, int HNu,
                                                            const float* __restrict__ sigma_dev /* [P] */,
                                                            const float* __restrict__ mu, long long mu_stride,
                                                            float* __restrict__ Y0s, const float* __restrict__ g) {
  const long long plan = blockIdx.y;
  const uint32_t k0 = keys.k[plan][0], k1 = keys.k[plan][1];
  const float sigma = sigma_dev[plan];
  const float* __restrict__ Ybar = mu + plan * mu_stride;
  const uint64_t size = (uint64_t)N * (uint64_t)HNu, half = (size + 1) / 2;
  float* __restrict__ out = Y0s + (uint64_t)plan * size;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t items = impl == 1 ? size : half;
  for (uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; tid < items; tid += stride) {
    uint32_t o0, o1;
    if (impl == 1) {
      threefry2x32(k0, k1, (uint32_t)(tid >> 32), (uint32_t)tid, o0, o1);
      const uint64_t r = tid % (uint64_t)HNu;
      const float y = shaped(bits_to_normal(o0 ^ o1), g, r) * sigma + Ybar[r];
      out[tid] = fclip(y, -1.0f, 1.0f);
    } else {
      const uint64_t j1 = tid + half;
      threefry2x32(k0, k1, (uint32_t)tid, j1 < size ? (uint32_t)j1 : 0u, o0, o1);
      const uint64_t r0 = tid % (uint64_t)HNu;
      const float y0 = shaped(bits_to_normal(o0), g, r0) * sigma + Ybar[r0];
      out[tid] = fclip(y0, -1.0f, 1.0f);
      if (j1 < size) {
        const uint64_t r1 = j1 % (uint64_t)HNu;
        const float y1 = shaped(bits_to_normal(o1), g, r1) * sigma + Ybar[r1];
        out[j1] = fclip(y1, -1.0f, 1.0f);
      }
    }
  }
}

// The same weighted mean for LARGE N (multi-GPU plans average over all N_total candidates on every rank).  The tile
// kernel above reads 64-byte pieces of rows 3.4 KB apart (1.4 TB/s at N = 8192); here a workgroup owns ONE candidate
// group g and 256 consecutive outputs, so a wavefront reads 256 contiguous bytes of a row per load and the weight is a
// scalar.  The (group, output) partials go through a [64][HNu] scratch and wmean_finish_kernel adds the 64 partials
// of an output in group order and applies the update: the same chains and the same final order as wmean_kernel —
// the same bits.
constexpr int kWmT = 256;  // outputs per workgroup of the row-major variant
static __global__ __launch_bounds__(kWmT) void wmean_partial_kernel(const float* __restrict__ weights,
                                                             const float* __restrict__ Y0s, int N, int HNu,
                                                             float* __restrict__ partial, int lazy, float sigma,
                                                             const float* __restrict__ Ybar_i) {
  const int g = blockIdx.y;
  const int e_raw = blockIdx.x * kWmT + threadIdx.x;
  const int e = e_raw < HNu ? e_raw : HNu - 1;
  const float* __restrict__ col = Y0s + e;
  const float yb = lazy ? Ybar_i[e] : 0.0f;  // lazy plans: Y0s holds normals (wmean_kernel)
  auto val = [&](float x) { return lazy ? fclip(x * sigma + yb, -1.0f, 1.0f) : x; };
  float acc = 0.0f;
  int n = g;
  for (; n + 31 * kWmG < N; n += 32 * kWmG) {
    float y[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) y[k] = col[(size_t)(n + k * kWmG) * HNu];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < 32; ++k) acc = ffma(weights[n + k * kWmG], val(y[k]), acc);
  }
  for (; n < N; n += kWmG) acc = ffma(weights[n], val(col[(size_t)n * HNu]), acc);
  if (e_raw < HNu) partial[(size_t)g * HNu + e_raw] = acc;
}
static __global__ __launch_bounds__(64) void wmean_finish_kernel(const float* __restrict__ partial, int HNu,
                                                          const float* __restrict__ Ybar_i, float alpha_i,
                                                          float alpha_bar_i, float alpha_bar_im1, int literal,
                                                          float* __restrict__ Ybar_im1, float* __restrict__ ybar_keep) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= HNu) return;
  if (ybar_keep) ybar_keep[e] = Ybar_i[e];
  float tot = partial[e];
#pragma unroll 8
  for (int k = 1; k < kWmG; ++k) tot = tot + partial[(size_t)k * HNu + e];
  float out = tot;
  if (literal) {
    const float sab = fsqrt(alpha_bar_i);
    float Yi = Ybar_i[e] * sab;
    float t1 = 1.0f / (1.0f - alpha_bar_i);
    float t2 = sab * tot;
    float score = t1 * (-Yi + t2);
    float t3 = (1.0f - alpha_bar_i) * score;
    float Yim1 = (1.0f / fsqrt(alpha_i)) * (Yi + t3);
    out = Yim1 / fsqrt(alpha_bar_im1);
  }
  Ybar_im1[e] = out;
}

// ---- path-integral baselines (mbd/planners/path_integral.py:39-52) ---------------------------------------
// cma-es: s[e] = sqrt(sum_n w_n (Y0s[n][e] - mu_t[e])^2), one thread per output, sequential fma over n
static __global__ __launch_bounds__(64) void cma_spread_kernel(const float* __restrict__ weights,
                                                        const float* __restrict__ Y0s, int N, int HNu,
                                                        const float* __restrict__ mu_t, float* __restrict__ s_out, PiBatch pb) {
  const long long plan = blockIdx.y;
  weights += plan * pb.weights; Y0s += plan * pb.cand; mu_t += plan * pb.mu; s_out += plan * pb.spread;
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= HNu) return;
  const float m = mu_t[e];
  float acc = 0.0f;
#pragma unroll 16
  for (int n = 0; n < N; ++n) {
    float d = Y0s[(size_t)n * HNu + e] - m;
    acc = ffma(weights[n], d * d, acc);
  }
  s_out[e] = fsqrt(acc);
}
// sigma <- max(mean_e(s) * sigma, 1e-3): one wavefront, canonical reduction order
static __global__ __launch_bounds__(64) void cma_sigma_kernel(const float* __restrict__ s, int HNu, float* __restrict__ sigma, PiBatch pb) {
  s += (long long)blockIdx.y * pb.spread; sigma += (long long)blockIdx.y * pb.sigma;
  float part = 0.0f;
  for (int i = threadIdx.x; i < HNu; i += 64) part = part + s[i];
  float sig = (wave_sum(part) / (float)HNu) * (*sigma);
  if (threadIdx.x == 0) *sigma = sig < 1e-3f ? 1e-3f : sig;  // jnp.maximum (path_integral.py:44): a NaN sigma stays NaN
}
// cem: indices of the K (<= 10, <= N) largest weights, ties towards the higher index: argsort(weights)[::-1][:10]
// (path_integral.py:50) of a stable sort that places NaN last — the selection ranks by the key isnan(w) ? +inf : w, so NaN
// weights (zero-spread rewards, a plan of one candidate: :123 has no guard) rank first, among themselves by descending index.
// Keys are in [0, 1] or +inf: above the -1 start value and the -2 "taken" mark, so every pass takes one untaken candidate
// and every index written to idx_out is in [0, N), for every input.
static __global__ __launch_bounds__(64) void cem_select_kernel(const float* __restrict__ weights, int N, int K,
                                                        int* __restrict__ idx_out, float* __restrict__ wl_global, PiBatch pb) {
  weights += (long long)blockIdx.y * pb.weights; idx_out += (long long)blockIdx.y * pb.idx;
  extern __shared__ __attribute__((aligned(16))) float wl_lds[];
  float* __restrict__ wl = wl_global ? wl_global : wl_lds;  // (a lane only ever touches the indices = lane mod 64)
  const int lane = threadIdx.x;
  for (int i = lane; i < N; i += 64) {
    const float w = weights[i];
    wl[i] = w != w ? __builtin_inff() : w;
  }
  for (int k = 0; k < K; ++k) {
    float bv = -1.0f;
    int bi = -1;
    for (int i = lane; i < N; i += 64)
      if (wl[i] >= bv) { bv = wl[i]; bi = i; }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      float ov = __shfl_xor(bv, off, 64);
      int oi = __shfl_xor(bi, off, 64);
      bool take = ov > bv || (ov == bv && oi > bi);
      bv = take ? ov : bv;
      bi = take ? oi : bi;
    }
    if (lane == 0) idx_out[k] = bi;
    if (bi >= 0 && (bi & 63) == lane) wl[bi] = -2.0f;
  }
}
static __global__ __launch_bounds__(64) void cem_mean_kernel(const int* __restrict__ idx, int K, const float* __restrict__ Y0s,
                                                      int HNu, float* __restrict__ mu_out, PiBatch pb) {
  idx += (long long)blockIdx.y * pb.idx; Y0s += (long long)blockIdx.y * pb.cand; mu_out += (long long)blockIdx.y * pb.out;
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= HNu) return;
  float acc = 0.0f;
  for (int k = 0; k < K; ++k) acc = acc + Y0s[(size_t)idx[k] * HNu + e];
  mu_out[e] = acc / (float)K;
}

// ---- the weigh kernel of a weighting record (the arithmetic: weigh_keep ... weigh_select, mbd_step_device.h).  Behind the step's own kernels and compiled
// only by the units that launch it (MBD_WEIGH_KERNEL: mbd_plan.hip, mbd_sweep.hip): a static kernel is emitted by every unit that
// sees it, and one emitted in front of other kernels moves their addresses — the code objects of the units that do not launch it,
// the rollouts' among them, stay what they were, and in the two that do every earlier kernel keeps its place ----
#ifdef MBD_WEIGH_KERNEL
// two sums in one pass over the barriers, each in block_sum's order (red: 2 x 16 entries)
__device__ __forceinline__ void block_sum2(float& xa, float& xb, float* red) {
  xa = wave_sum(xa);
  xb = wave_sum(xb);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = xa;
    red[kScoreThreads / 64 + (threadIdx.x >> 6)] = xb;
  }
  __syncthreads();
  float a = red[0], b = red[kScoreThreads / 64];
#pragma unroll
  for (int w = 1; w < kScoreThreads / 64; ++w) {
    a = a + red[w];
    b = b + red[kScoreThreads / 64 + w];
  }
  xa = a;
  xb = b;
}
// ONE 1024-thread workgroup per plan (blockIdx.y = plan, PiBatch's strides: a single plan launches one row and zero strides).
// Thread t owns the entries i = t, t + 1024, ... and nothing else, in every pass: up to 8192 candidates they cross from memory
// once and stay in registers (from the second reduction on as z), beyond that they are re-read; e[] of the last pass goes to lg —
// LDS, or the plan's global scratch beyond the LDS window — and needs no barrier of its own.  The selection's branches are taken
// on values every thread read from the same LDS words: uniform.  iters + 3 passes at most, each one exp_ per entry and one
// two-value block reduction.  Plain vector loads and stores; the mean reward leaves through a system-scope store as soon as the
// first reduction has it (the progress poll's slot, as in the fused score), the log entry through thread 0.
static __global__ __launch_bounds__(kScoreThreads) void weigh_kernel(const float* __restrict__ rews, int N, float temp, WeighRec R,
                                                              float* __restrict__ weights, float* __restrict__ rew_mean_out,
                                                              float* __restrict__ lg_global, WeighLog log, PiBatch pb) {
  const long long plan = blockIdx.y;
  rews += plan * pb.rews; weights += plan * pb.weights; rew_mean_out += plan * pb.mean;
  if (pb.temps) temp = pb.temps[plan];
  extern __shared__ __attribute__((aligned(16))) float lg_lds[];
  float* __restrict__ lg = lg_global ? lg_global : lg_lds;
  __shared__ float red[2 * (kScoreThreads / 64)];
  __shared__ int red_n[kScoreThreads / 64];
  const int tid = threadIdx.x;
  constexpr int RK = 8;
  const bool in_regs = N <= RK * kScoreThreads;  // (uniform)
  float r[RK];
  unsigned km = 0;  // bit k: entry tid + 1024 k exists and is kept
#pragma unroll
  for (int k = 0; k < RK; ++k) {
    const bool ok = in_regs && tid + k * kScoreThreads < N;
    r[k] = ok ? rews[tid + k * kScoreThreads] : 0.0f;
    km |= (ok && weigh_keep(r[k], R.reject)) ? 1u << k : 0u;
  }
  // f(i, x, keep) over this thread's entries in ascending i: x = the register's value, or rews[i] re-read
  auto each = [&](auto&& f) {
    if (in_regs) {
#pragma unroll
      for (int k = 0; k < RK; ++k)
        if (tid + k * kScoreThreads < N) f(tid + k * kScoreThreads, r[k], (km >> k & 1u) != 0, k);
    } else {
      for (int i = tid; i < N; i += kScoreThreads) {
        const float x = rews[i];
        f(i, x, weigh_keep(x, R.reject), 0);
      }
    }
  };
  float part = 0.0f, rmax = -__builtin_inff();
  int cnt = 0;
  each([&](int, float x, bool keep, int) {
    part = keep ? part + x : part;
    rmax = keep ? fmax_(rmax, x) : rmax;
    cnt += keep ? 1 : 0;
  });
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
  if ((tid & 63) == 0) red_n[tid >> 6] = cnt;
  block_sum_max(part, rmax, red);  // (its barriers cover red_n)
  int kept = 0;
#pragma unroll
  for (int w = 0; w < kScoreThreads / 64; ++w) kept += red_n[w];
  float* __restrict__ log_temp = log.temp + plan * log.stride;
  float* __restrict__ log_ess = log.ess + plan * log.stride;
  int* __restrict__ log_kept = log.kept + plan * log.stride;
  if (kept == 0) {  // (uniform) nothing to weigh: every weight +0, the mean reward NaN
    for (int i = tid; i < N; i += kScoreThreads) weights[i] = 0.0f;
    if (tid == 0) {
      __hip_atomic_store(rew_mean_out, __builtin_nanf(""), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      *log_temp = temp; *log_ess = 0.0f; *log_kept = 0;
    }
    return;
  }
  const float mean = part / (float)kept;
  if (tid == 0) __hip_atomic_store(rew_mean_out, mean, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  part = 0.0f;
  each([&](int, float x, bool keep, int) { part = keep ? weigh_dev(part, x, mean) : part; });
  const float sd = weigh_sd(block_sum(part, red), kept);
  const float zmax = weigh_z(rmax, mean, sd);
  if (in_regs) {  // the registers hold z from here on
#pragma unroll
    for (int k = 0; k < RK; ++k) r[k] = weigh_z(r[k], mean, sd);
  }
  float S1 = 0.0f, S2 = 0.0f;
  auto pass = [&](float T, bool store) {
    float p1 = 0.0f, p2 = 0.0f;
    each([&](int i, float x, bool keep, int) {
      const float e = keep ? weigh_e(in_regs ? x : weigh_z(x, mean, sd), zmax, T) : 0.0f;
      p1 = keep ? p1 + e : p1;
      p2 = keep ? p2 + e * e : p2;
      if (store) lg[i] = e;
    });
    block_sum2(p1, p2, red);
    S1 = p1;
    S2 = p2;
    return weigh_ess(p1, p2);
  };
  const float Ts = weigh_select(R, temp, kept, [&](float T) { return pass(T, false); });
  const float ess = pass(Ts, true);
  each([&](int i, float, bool keep, int) { weights[i] = keep ? lg[i] / S1 : 0.0f; });
  if (tid == 0) { *log_temp = Ts; *log_ess = ess; *log_kept = kept; }
}
#endif  // MBD_WEIGH_KERNEL

// ---- the elite record (mbd_plan_set_elites, include/mbd_hip.h mbd_elites; DESIGN.md section 1 "N18 elites"): a step's best
// candidates are candidates of the next step, and the step's mean itself may be candidate 0.  Injection behind the step's sampler,
// selection behind its update kernel, a shift at a tick boundary.  Under its own guard, for weigh_kernel's reason: mbd_plan.hip and
// mbd_sweep.hip emit the kernels, each its own forms (the arithmetic of one element, elite_z ... elite_select_host: mbd_step_device.h) ----
struct EliteSelect {
  const float* rews;    // [N] the rewards the step's score read
  int N, HNu;
  const float* cand;    // [N][HNu] the step's candidates, or their normals (lazy)
  int lazy;
  float sigma;          // lazy: sigma_i ...
  const float* ybar_i;  // ... and Ybar_i [HNu] of the step
  int n_elites, nominal;
  float* E;             // [n_elites][HNu]
  float* R;             // [n_elites]
  int* src;             // [n_elites]
  int* count;           // [1]: read (the step's slots), then rewritten
  int* log_count;       // the step's log entry
  int* log_kept;
  float* log_top;
};
struct EliteInject {
  float* cand;          // [N][HNu] the step's candidates, or their normals (lazy): rows 0 .. slots - 1 are rewritten
  int HNu;
  const float* ybar_i;  // [HNu]
  int lazy;
  float sigma;
  const float* g;       // [HNu] the shape the step's sampler was handed, or nullptr
  int n_elites, nominal;
  const float* E;
  const int* count;
};
#ifdef MBD_ELITE_KERNEL
constexpr int kEliteRegs = 8, kEliteThreads = 256;
// ONE 1024-thread workgroup: the n_elites best finite rewards in pick_before's order, then E', R', src', count' and the log entry.
// Thread t owns the entries t, t + 1024, ...: the first kEliteRegs of them (8192 candidates) stay in registers, those beyond are
// read again in every round.  Round j: every thread offers its best entry that is still open behind winner j - 1 (ascending i,
// replaced on pick_before only), the wavefront's butterfly and the scan over the sixteen wavefronts' offers combine them as
// pick_argmax_block does — a total order on distinct indices, so the combination order does not matter.  Every thread reads the
// round's winner from the same LDS words: the loop's exit and the gather's rows are uniform.  The offers' LDS words alternate
// between two sets, so a round costs ONE barrier: a thread that writes set b in round j + 2 has passed round j + 1's barrier, which
// every thread reaches behind its reads of round j.
// k rounds, not one sort of the sixteen wavefronts' top-k lists: a round is eight selects per thread, twelve cross-lane moves and
// one barrier with sixteen broadcast LDS reads behind it, all on one dependent chain; the merge would keep 32 offers per lane live
// or spill them.  Measured at N = 1024, HNu = 850 (docs/experiments.md section 28): 5.6 us at k = 1, 14.3 at k = 4, 95 at k = 32 —
// 2.9 us per elite, the round and the row's gather together, each gather a dependent load and store.  Fine at the few elites
// sampling MPC uses; at k = 32 it is a sixth of a humanoid step, and batching the gathers' loads is the first thing to try.
// Bounds: rews[i] for i < N; cand rows win_i[j] < N; E rows j < count' <= n_elites.  Plain vector loads and stores.
__device__ __forceinline__ void elite_select_body(const EliteSelect& A) {
  __shared__ float red_v[2][kScoreThreads / 64];
  __shared__ int red_i[2][kScoreThreads / 64];
  __shared__ float win_v[kEliteMax];
  __shared__ int win_i[kEliteMax];
  const int tid = threadIdx.x;
  float rv[kEliteRegs];
#pragma unroll
  for (int q = 0; q < kEliteRegs; ++q) {
    const int i = tid + q * kScoreThreads;
    rv[q] = i < A.N ? A.rews[i] : __builtin_nanf("");  // (a NaN is never open)
  }
  float pv = 0.0f;
  int pi = -1, cnt = 0;
  for (int j = 0; j < A.n_elites; ++j) {
    float bv = 0.0f;
    int bi = -1;
#pragma unroll
    for (int q = 0; q < kEliteRegs; ++q) {
      const int i = tid + q * kScoreThreads;
      const bool take = elite_open(rv[q], i, pv, pi) && pick_before(rv[q], i, bv, bi);
      bv = take ? rv[q] : bv;
      bi = take ? i : bi;
    }
    for (int i = tid + kEliteRegs * kScoreThreads; i < A.N; i += kScoreThreads) {
      const float x = A.rews[i];
      const bool take = elite_open(x, i, pv, pi) && pick_before(x, i, bv, bi);
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
    const int b = j & 1;
    if ((tid & 63) == 0) { red_v[b][tid >> 6] = bv; red_i[b][tid >> 6] = bi; }
    __syncthreads();
    bv = red_v[b][0];
    bi = red_i[b][0];
#pragma unroll
    for (int w = 1; w < kScoreThreads / 64; ++w) {
      const float ov = red_v[b][w];
      const int oi = red_i[b][w];
      const bool take = pick_before(ov, oi, bv, bi);
      bv = take ? ov : bv;
      bi = take ? oi : bi;
    }
    if (bi < 0) break;  // (no open entry is left: uniform)
    if (tid == 0) { win_v[j] = bv; win_i[j] = bi; }
    pv = bv;
    pi = bi;
    cnt = j + 1;
  }
  __syncthreads();
  for (int j = 0; j < cnt; ++j) {
    const float* __restrict__ row = A.cand + (size_t)win_i[j] * A.HNu;
    float* __restrict__ out = A.E + (size_t)j * A.HNu;
    for (int e = tid; e < A.HNu; e += kScoreThreads) out[e] = elite_value(row[e], A.lazy, A.sigma, A.ybar_i[e]);
  }
  if (tid == 0) {
    const int slots = A.nominal + *A.count;
    int kept = 0;
    for (int j = 0; j < cnt; ++j) {
      A.R[j] = win_v[j];
      A.src[j] = win_i[j];
      kept += win_i[j] < slots ? 1 : 0;
    }
    *A.count = cnt;
    *A.log_count = cnt;
    *A.log_kept = kept;
    *A.log_top = cnt > 0 ? win_v[0] : __builtin_bit_cast(float, 0x7fc00000u);
  }
}
static __global__ __launch_bounds__(kScoreThreads) void elite_select_kernel(EliteSelect A) { elite_select_body(A); }
// Behind the launch that made the step's normals (or candidates), in front of its rollout: rows 0 .. nominal + count - 1.  The grid
// covers (nominal + n_elites) HNu elements; every thread loads count and a thread of an absent slot writes nothing.  Bounds: the
// loaded count is held to [0, n_elites], and the set call refuses nominal + n_elites >= Nsample, so a written row lies below N.
__device__ __forceinline__ void elite_inject_body(const EliteInject& A) {
  const int idx = blockIdx.x * kEliteThreads + threadIdx.x;
  const int slot = idx / A.HNu, e = idx - slot * A.HNu;
  int cnt = *A.count;
  cnt = cnt < 0 ? 0 : (cnt > A.n_elites ? A.n_elites : cnt);
  if (slot >= A.nominal + cnt) return;
  const float yb = A.ybar_i[e];
  float v;
  if (slot < A.nominal) {
    v = elite_nominal(yb, A.lazy);
  } else {
    const float Ej = A.E[(size_t)(slot - A.nominal) * A.HNu + e];
    v = A.lazy ? elite_z(Ej, yb, A.sigma, A.g, e) : Ej;
  }
  A.cand[(size_t)slot * A.HNu + e] = v;
}
static __global__ __launch_bounds__(kEliteThreads) void elite_inject_kernel(EliteInject A) { elite_inject_body(A); }
// The elites at the start of a run or a tick: shift < 0: count = 0; otherwise every present elite's row shifted `shift` elements
// forward with zeros behind it (the mean's own shift), count as it is.  Workgroup j owns row j; the shift is in place, so a block of
// 256 elements is read, then — behind a barrier — written: a later block reads only elements no earlier block wrote.  A workgroup
// leaves as a whole (count is one word), so the barriers' trip count is uniform.
__device__ __forceinline__ void elite_shift_body(float* __restrict__ E, int* __restrict__ count, int HNu, int shift) {
  if (shift < 0) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *count = 0;
    return;
  }
  if ((int)blockIdx.x >= *count) return;
  float* __restrict__ row = E + (size_t)blockIdx.x * HNu;
  for (int base = 0; base < HNu; base += kEliteThreads) {
    const int e = base + threadIdx.x;
    float v = 0.0f;
    if (e < HNu && e + shift < HNu) v = row[e + shift];
    __syncthreads();
    if (e < HNu) row[e] = v;
    __syncthreads();
  }
}
static __global__ __launch_bounds__(kEliteThreads) void elite_shift_kernel(float* __restrict__ E, int* __restrict__ count, int HNu,
                                                                    int shift) {
  elite_shift_body(E, count, HNu, shift);
}

// SWEEPS (mbd_sweep_set_elites): the three launches for P plans of one env at once — blockIdx.y is the plan, whose candidates, Ybar_i,
// rewards and elite state (E, R, src, count, the log's slot) sit at fixed strides, in elements, from plan 0's.  The bodies are the
// single-plan kernels': same text, same order, same bits; only the indexing is new.  MBD_SWEEP_KERNEL: the unit that launches them
// (mbd_sweep.hip) alone emits them.  mask: bit k set = plan k takes part; the
// workgroups of a plan that does not return before they read or write anything (a session's mixed tick: the episodes that idle).
// Bounds: gridDim.y = P <= 32 = the mask's width; every stride is the size of one plan's array, so plan k's accesses are the
// single-plan kernel's inside slice k.
#ifdef MBD_SWEEP_KERNEL
struct EliteBatch {
  long long cand, ybar, rews;  // [P][N][HNu], Ybar_i of plan k (0: one for all), [P][N]
  long long E, R, log;         // rows HNu, rows (R and src), the log's capacity per plan; count: one word per plan
  unsigned mask;
};
static __global__ __launch_bounds__(kEliteThreads) void elite_inject_batch_kernel(EliteInject A, EliteBatch B) {
  const long long k = blockIdx.y;
  if (!((B.mask >> k) & 1u)) return;
  A.cand += k * B.cand; A.ybar_i += k * B.ybar; A.E += k * B.E; A.count += k;
  elite_inject_body(A);
}
// one int per plan: a shift (-1 empties, E Nu shifts with the mean, 0 leaves), or the slot of the plan's log its entry goes to
struct EliteShifts {
  int s[32];
};
static __global__ __launch_bounds__(kScoreThreads) void elite_select_batch_kernel(EliteSelect A, EliteBatch B, EliteShifts slot) {
  const long long k = blockIdx.y;
  if (!((B.mask >> k) & 1u)) return;  // (uniform: the whole workgroup, in front of every barrier)
  A.rews += k * B.rews; A.cand += k * B.cand; A.ybar_i += k * B.ybar; A.E += k * B.E; A.R += k * B.R; A.src += k * B.R; A.count += k;
  const long long entry = k * B.log + slot.s[k];  // (slot.s[k] in [0, B.log): the host's ring_slot)
  A.log_count += entry; A.log_kept += entry; A.log_top += entry;
  elite_select_body(A);
}
static __global__ __launch_bounds__(kEliteThreads) void elite_shift_batch_kernel(float* __restrict__ E, int* __restrict__ count, int HNu,
                                                                          EliteShifts sh, EliteBatch B) {
  const long long k = blockIdx.y;
  if (!((B.mask >> k) & 1u)) return;
  elite_shift_body(E + k * B.E, count + k, HNu, sh.s[k]);
}
#endif  // MBD_SWEEP_KERNEL
#endif  // MBD_ELITE_KERNEL

// ---- the to-go record (mbd_plan_set_togo, include/mbd_hip.h mbd_togo; DESIGN.md section 1 "N19 to-go"): the horizon's rows in G
// groups, group j's rows updated under weights derived from R_j, the candidates' mean reward from row s_j onwards.  Under a record
// the two kernels below stand where the fused score + weighted-mean launch stands (the layout and the returns' arithmetic,
// togo_groups ... togo_chain: mbd_step_device.h). ----
#ifdef MBD_TOGO_KERNEL
// R [G][N] from rewss [N][H]: row 0 is a copy of rews, the array the step's score reads (for the peek call: the update kernel reads
// group 0's returns from rews itself); rows 1 .. G - 1 are togo_chain's.  A lane owns a candidate and reads its row of rewss with
// direct strided loads — sixteen in flight — since the whole of rewss is N H floats (200 KB at the flagship size) and sits in L2 behind
// the rollout that wrote it; workgroups of one wavefront spread the candidates over the CUs.  Bounds: n < N guards every access; a
// load is rewss[n H + t] with t in [block, H - 1], a store R[j N + n] with j in [0, G - 1].
constexpr int kTogoThreads = 64;
struct TogoReturns {
  const float* rews;   // [N]
  const float* rewss;  // [N][H]
  float* R;            // [G][N]
  int N, H, block, G;
};
static __global__ __launch_bounds__(kTogoThreads) void togo_returns_kernel(TogoReturns A) {
  const int n = blockIdx.x * kTogoThreads + threadIdx.x;
  if (n >= A.N) return;
  float* __restrict__ R = A.R;
  R[n] = A.rews[n];
  togo_chain(A.rewss + (size_t)n * A.H, A.H, A.block, A.G, [&](int j, float v) { R[(size_t)j * A.N + n] = v; });
}

// Score and weighted mean per group in ONE launch: score_wmean_kernel's workgroup (kWmE x kWmG = 1024 threads) and text
// (score_wmean_body: score_block into the LDS weights, the prefetch, the rounds of 48 rows, the tail, the 64 partials in order, the
// final formula), over tiles that never straddle a group.  Groups 0 .. G - 2 hold block Nu elements each, tpg = ceil(block Nu / 16)
// tiles; the last group holds (H - s_{G-1}) Nu elements in the remaining T - (G - 1) tpg tiles; tile x of the XCD-aware order
// (xcd_tile: neighbouring tiles, which share candidate lines, meet in one L2) is tile t = x - j tpg of group j = min(x / tpg, G - 1).
// A group's last tile may be partial: the span holds its outputs below e_lim = s_{j+1} Nu.  Group j's workgroups derive W_j from
// R_j (group 0: from rews itself); its first workgroup stores W_j — group 0's into the plan's weights, with the mean reward and its
// early system-scope copy, as the fused kernel's workgroup 0 does — and every workgroup stores ybar_keep for its own elements.
// Bounds: the launch has exactly T workgroups and xcd_tile is a bijection on [0, T); t < the group's tile count, so
// e_base = s_j Nu + 16 t < e_lim <= H Nu: the span clamps its loads to e_lim - 1 and stores below e_lim only.  R and W rows j < G.
// LDS: N floats of weights (N <= 12288: the set call) beside the span's two reduction arrays.
struct TogoUpdate {
  const float* rews;  // [N]: R_0
  const float* R;     // [G][N]: rows 1 .. G - 1 are read
  float* W;           // [G][N]: rows 1 .. G - 1 are written
  float* weights;     // [N]: W_0
  float* rew_mean;
  const float* cand;  // [N][H Nu]
  const float* ybar_i;
  float* ybar_im1;
  float* ybar_keep;
  int N, H, Nu, G, block, tpg, T;
  float temp;
  int std_guard;
  float alpha_i, alpha_bar_i, alpha_bar_im1;
  int literal, lazy;
  float sigma;
};
static __global__ __launch_bounds__(kWmE * kWmG) void togo_update_kernel(TogoUpdate A) {
  const int x = xcd_tile(blockIdx.x, A.T, 0);
  int j = x / A.tpg;
  j = j < A.G - 1 ? j : A.G - 1;
  const int t = x - j * A.tpg;
  const int e_base = togo_start(j, A.block) * A.Nu + t * kWmE, e_lim = togo_end(j, A.G, A.H, A.block) * A.Nu;
  const size_t row = (size_t)j * A.N;
  score_wmean_body<48, true, 1, false, true>(j ? A.R + row : A.rews, nullptr, A.N, 0.0f, A.temp, A.std_guard, j ? A.W + row : A.weights,
                                             j ? nullptr : A.rew_mean, A.cand, A.H * A.Nu, A.ybar_i, A.alpha_i, A.alpha_bar_i,
                                             A.alpha_bar_im1, A.literal, A.ybar_im1, A.lazy, A.sigma, A.ybar_keep, 0, t == 0, e_base,
                                             e_lim);
}

#ifdef MBD_SWEEP_KERNEL
// SWEEPS (mbd_sweep_set_togo): the two launches for P plans at once.  rewss is [P N][H] contiguous and rews [P N], so a lane of the
// returns kernel still owns one candidate b = k N + n of the P N; it writes R [P][G][N], row 0 of every plan a copy of its rews.
// Bounds: b < P N guards every access; a load is rewss[b H + t] with t in [block, H - 1], a store R[(k G + j) N + n], j in [0, G - 1].
static __global__ __launch_bounds__(kTogoThreads) void togo_returns_batch_kernel(TogoReturns A, int P) {
  const long long b = (long long)blockIdx.x * kTogoThreads + threadIdx.x;
  if (b >= (long long)P * A.N) return;
  const int k = (int)(b / A.N), n = (int)(b - (long long)k * A.N);
  float* __restrict__ R = A.R + (size_t)k * A.G * A.N;
  R[n] = A.rews[b];
  togo_chain(A.rewss + (size_t)b * A.H, A.H, A.block, A.G, [&](int j, float v) { R[(size_t)j * A.N + n] = v; });
}
// The update: togo_update_kernel's tiles (the same closed form from tile x to group and tile of the group, never straddling a group)
// with score_wmean_batch_kernel's plan and tile order, strides and per-plan temperatures — gridDim.x = T tiles, blockIdx.y the plan;
// a multiple of 8 plans puts plan k's tiles on XCD k mod 8, otherwise each plan's row of workgroups takes the XCD-aware tile order.
// The chains are score_wmean_body's SPAN form with the sweeps' rounds (32 rows in flight, rewards re-read: same bits).  R and W are
// [P][G][N]; group 0's first workgroup stores plan k's weights and mean reward where the batch score kernel stores them.
// Bounds: as togo_update_kernel per plan; (k, x) is a bijection on [0, P) x [0, T).  LDS: N floats beside the span's arrays.
// One workgroup per CU (87 registers, none spilled; held to the 64 of two workgroups per CU the span's clamped indices spill 20 bytes).
static __global__ __launch_bounds__(kWmE * kWmG, 4) void togo_update_batch_kernel(TogoUpdate A, ScoreBatch sb) {
  const int T = gridDim.x, P = gridDim.y;
  long long k = blockIdx.y;
  int x = xcd_tile(blockIdx.x, T, blockIdx.y * T);
  if ((P & 7) == 0) {
    const int lin = blockIdx.y * T + blockIdx.x, c = lin & 7, m = lin >> 3;
    k = c + 8 * (m / T);
    x = m % T;
  }
  int j = x / A.tpg;
  j = j < A.G - 1 ? j : A.G - 1;
  const int t = x - j * A.tpg;
  const int e_base = togo_start(j, A.block) * A.Nu + t * kWmE, e_lim = togo_end(j, A.G, A.H, A.block) * A.Nu;
  const size_t row = ((size_t)k * A.G + j) * A.N;
  score_wmean_body<32, false, 1, false, true>(j ? A.R + row : A.rews + k * sb.rews, nullptr, A.N, 0.0f, sb.temps ? sb.temps[k] : A.temp,
                                              A.std_guard, j ? A.W + row : A.weights + k * sb.weights,
                                              j ? nullptr : A.rew_mean + k * sb.mean, A.cand + k * sb.cand, A.H * A.Nu,
                                              A.ybar_i + k * sb.ybar_in, A.alpha_i, A.alpha_bar_i, A.alpha_bar_im1, A.literal,
                                              A.ybar_im1 + k * sb.ybar_out, A.lazy, A.sigma, nullptr, 0, t == 0, e_base, e_lim);
}
#endif  // MBD_SWEEP_KERNEL
#endif  // MBD_TOGO_KERNEL

}  // namespace mbd
