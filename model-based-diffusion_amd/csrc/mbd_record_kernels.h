// mbd_record_kernels.h — the kernels only members of the records launch (mbd_internal.h; the members: mbd_records.hip): the sigma
// record's boundary kernel, the demo record's window and error kernels, the objective, pick, value, adapt and zone records'
// kernels, with their argument structs and the host-and-device functions only they and their host references call.  `static`, so
// every unit that sees them would emit them: ONLY mbd_records.hip includes this header, and that unit alone emits them, once, for
// plans and sweeps alike.  What a step kernel shares with them is in mbd_step_device.h.
#pragma once

#include "mbd_step_device.h"

namespace mbd {

// The carried sigma of a path-integral episode at a tick boundary (include/mbd_hip.h mbd_mpc_sigma).  The sigma the next tick
// starts from, from the one the last tick ended with: sigma_warm, or with a gain clamp(gain * sigma_end, sigma_warm, sigma_cold)
// — a product and two selects, three separately rounded f32 steps (the build's -ffp-contract=off), written so that a NaN sigma
// stays NaN (both compares are false).  Host and device: mbd_debug_mpc_sigma_next runs this same text on the CPU.
MBD_HD float mpc_pi_next_sigma(float sigma_end, float sigma_cold, float sigma_warm, float gain) {
  if (gain == 0.0f) return sigma_warm;
  float x = gain * sigma_end;
  x = x < sigma_warm ? sigma_warm : x;
  x = x > sigma_cold ? sigma_cold : x;
  return x;
}
// One launch per tick boundary, one thread per episode k < P (P = 1: a plan), behind the tick's last cma_sigma_kernel and in
// front of the next tick's sampler on the same stream.  sigma [P]: the carried sigmas (what cma_sigma_kernel left; mppi and cem
// leave them alone).  log: episode 0's slot t of the sigma log, episode k's log_stride floats further; a slot is (start, end).
// cold != 0: the launch in front of a cold tick — sigma and the slot's start take sigma_cold.  Otherwise: the slot's end takes
// the carried sigma, and the next sigma goes into the carried slot and into the following slot's start (the log has T + 1
// slots).  Plain loads and stores; the arguments are uniform.
static __global__ __launch_bounds__(64) void mpc_pi_sigma_kernel(float* __restrict__ sigma, int P, float* __restrict__ log,
                                                           long long log_stride, int cold, float sigma_cold, float sigma_warm,
                                                           float gain) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= P) return;
  float* __restrict__ slot = log + (long long)k * log_stride;
  if (cold) {
    sigma[k] = sigma_cold;
    slot[0] = sigma_cold;
    return;
  }
  const float end = sigma[k];
  slot[1] = end;
  const float next = mpc_pi_next_sigma(end, sigma_cold, sigma_warm, gain);
  sigma[k] = next;
  slot[2] = next;
}

// The demo clock of an episode with a demo record (include/mbd_hip.h mbd_mpc_demo).  ONE launch in front of the tick loop
// builds the table of every tick's window from the clip [K][L][C] (C = 3, car2d 2):
//   windows[t][k][h] = clip[k][min(c0 + (t + D) E + h, L - 1)]        h = 0 .. kXrefRows - 1
// so a tick hands its launches a pointer into the table and nothing else.  Grid-stride over the T K kXrefRows rows, every
// element written, the row arithmetic in 64 bits (c0 alone may be close to 2^31).
static __global__ __launch_bounds__(256) void demo_windows_kernel(const float* __restrict__ clip, int L, int c0, int T, int K,
                                                            int C, int E, int D, float* __restrict__ windows) {
  const long long rows = (long long)T * K * kXrefRows;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += stride) {
    const long long tk = r / kXrefRows;
    const long long h = r - tk * kXrefRows, t = tk / K, k = tk - t * K;
    long long src = (long long)c0 + (t + D) * E + h;
    if (src > (long long)L - 1) src = (long long)L - 1;
    const float* a = clip + (k * L + src) * C;
    float* o = windows + r * C;
    for (int c = 0; c < C; ++c) o[c] = a[c];
  }
}
// ... and ONE launch behind it: how far the executed motion was from the clip.  xlog [T][P][E][K][3] holds the positions the
// rollouts of the executed rows wrote (P = 1: a plan's [T E][K][3]; car2d: K = 1, its qs — x, y, theta); control step t E + j
// of every episode is compared with clip row min(c0 + t E + j, L - 1), whatever the delay: err, in xlog's order [T][P][E][K],
// is the unclipped Euclidean distance (C = 2: over x and y), products and sums in this order.
static __global__ __launch_bounds__(256) void mpc_track_err_kernel(const float* __restrict__ xlog, const float* __restrict__ clip,
                                                             int L, int c0, int T, int P, int E, int K, int C,
                                                             float* __restrict__ err) {
  const long long n = (long long)T * P * E * K;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const long long k = i % K, j = (i / K) % E, t = i / ((long long)K * E * P);
    long long row = (long long)c0 + t * E + j;
    if (row > (long long)L - 1) row = (long long)L - 1;
    const float* x = xlog + i * 3;
    const float* c = clip + (k * L + row) * C;
    const float dx = x[0] - c[0], dy = x[1] - c[1];
    float s = dx * dx + dy * dy;
    if (C == 3) {
      const float dz = x[2] - c[2];
      s = s + dz * dz;
    }
    err[i] = sqrtf(s);
  }
}
inline unsigned demo_blocks(long long items) {
  const long long b = (items + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b < 1024 ? b : 1024));
}

// ---- the objective (mbd_plan_set_objective, include/mbd_hip.h mbd_objective): between the rollout and the score, the rollout's
// per-step rewards and the candidates it fetched -> the rewards the score sees, rews[b] = ret[b] - cost[b % N] ----
// The arithmetic of one candidate is the functions below, host and device text: the per-row steps are what the kernel's lanes run,
// the loops over them what mbd_debug_objective_host runs on the CPU, where a test without a device holds them to the checker.
// f32, every operation rounded (the build's -ffp-contract=off).
// ret of one row: its per-step rewards r [H] under the row weights w [H] — acc = +0, acc = acc + (w[h] * r[h]) for h ascending,
// then ONE division by wsum, the f32 left-to-right sum of w the set call formed.  Nothing is skipped: 0 * NaN stays NaN.
MBD_HD float objective_ret_step(float acc, float w, float r) { return acc + w * r; }
MBD_HD float objective_ret(const float* __restrict__ r, const float* __restrict__ w, float wsum, int H) {
  float acc = 0.0f;
  for (int h = 0; h < H; ++h) acc = objective_ret_step(acc, w[h], r[h]);
  return acc / wsum;
}
// Column a of one candidate c [H][Nu] — values, or (lazy) the normals z of a plan that keeps them, formed as the rollout's fetch
// forms them: clip((z * sigma) + ybar[h][a], -1, 1), shift_kernel's two roundings —: eff = sum over h of u u, rat = sum over h of
// (u - u_prev)^2, both from +0 in ascending h.  u_prev stays in a register from the row before; at h = 0 it is prev[a], and
// without a previous action (have == false) the h = 0 term is left out.
MBD_HD float objective_value(float x, int lazy, float sigma, float yb) { return lazy ? fclip(x * sigma + yb, -1.0f, 1.0f) : x; }
MBD_HD void objective_column_step(float u, float& up, bool& have, float& eff, float& rat) {
  eff = eff + u * u;
  const float d = u - up;
  rat = have ? rat + d * d : rat;
  up = u;
  have = true;
}
MBD_HD void objective_column(const float* __restrict__ c, int H, int Nu, int a, int lazy, float sigma,
                             const float* __restrict__ ybar, const float* __restrict__ prev, float& eff, float& rat) {
  eff = 0.0f; rat = 0.0f;
  bool have = prev != nullptr;
  float up = have ? prev[a] : 0.0f;
  for (int h = 0; h < H; ++h)
    objective_column_step(objective_value(c[h * Nu + a], lazy, sigma, lazy ? ybar[h * Nu + a] : 0.0f), up, have, eff, rat);
}
// actuator a's term of the cost: q[a] * ((effort * eff_a) + (rate * rat_a)); the cost is their sum from +0 in ascending a, / float(H)
MBD_HD float objective_term(float q, float effort, float eff, float rate, float rat) { return q * (effort * eff + rate * rat); }

// One launch over the B rows of a rollout launch.  A candidate's row is served by a 32-lane half of a wavefront: lane a < Nu is
// actuator a (Nu <= MBD_MAX_ACT = 24) — row h of the candidate is ONE contiguous read of Nu floats across the half —, and the
// half's last lane, never an actuator, reads the row's H per-step rewards, forms ret and stores the results.  ONE loop over h
// serves both: every lane loads one float per row through its own pointer and stride (an actuator's column, the last lane's
// rewards; the other lanes a constant) and runs both per-row steps on it — each lane keeps the one that is its own, so the
// wavefront never diverges and the rewards' chain runs beside the columns' instead of behind them; the loads do not depend on the
// chains, and the loop is unrolled so that several rows are in flight.  The sum over the actuators is serial in ascending lane
// order, as the contract says (every lane of the half runs it, the last one keeps it): a butterfly would change the bits.  A
// half reads only its own lanes (__shfl of width 32), lanes >= Nu hold a term nobody reads and the halves of rows >= B read
// nothing of any candidate and store nothing, so no value crosses from one candidate to another: a diverged candidate's NaN stays in its own row.  No
// lane leaves early (the shuffles see whole halves).  Plain vector loads and stores.
constexpr int kObjLanes = 32;     // lanes per candidate
constexpr int kObjThreads = 256;  // 8 candidates per workgroup
static_assert(MBD_MAX_ACT < kObjLanes, "a candidate's half needs a lane beyond the actuators");
struct ObjectiveArgs {
  const float* rewss;  // [B][H] the per-step rewards of the launch's rows
  float* rews;         // [B] in: mean_H as the rollout stored it; out: ret - cost
  int B, N, row0;      // rows; row b is candidate row0 + b % N of cand (a shard: row0 = shard_begin, N = B; an ensemble: B = M N)
  int H, Nu;
  const float* cand;   // [.][H][Nu] the candidates' values, or their normals (lazy)
  int lazy;
  float sigma;
  const float* ybar;   // [H][Nu] Ybar_i (lazy)
  const float* w;      // [H] row weights, or nullptr: ret = rews as stored
  float wsum;
  const float* q;      // [Nu] actuator weights
  float effort, rate;
  int costs;           // 0: the cost pass is skipped (effort == 0 and rate == 0)
  const float* prev;   // [Nu] the action executed before row 0, clipped, or nullptr: none
  float* ret_keep;     // [B]  what mbd_*_peek_objective returns
  float* cost_keep;    // [N]
};
__device__ __forceinline__ void objective_body(const ObjectiveArgs& A) {
  const int lane = threadIdx.x & (kObjLanes - 1);
  const int b = blockIdx.x * (kObjThreads / kObjLanes) + threadIdx.x / kObjLanes;
  const bool live = b < A.B;
  const bool last = live && lane == kObjLanes - 1;
  const bool act = live && A.costs && lane < A.Nu;  // this lane walks a column
  const bool weighs = last && A.w;                  // this lane walks the row's rewards
  const int lazy = act ? A.lazy : 0;
  // what the lane reads in row h: x[h * stride] and, forming a lazy candidate, yb[h * ystride].  A lane with nothing of its own to
  // read — a lane between the actuators and the last one, every lane of a half beyond the rows — reads element 0 of the
  // actuator weights with stride 0 instead, a table every launch has: the loads need no branch, and what such a lane computes
  // is never looked at
  const float* __restrict__ x = A.q;
  int stride = 0;
  if (act) { x = A.cand + (size_t)(A.row0 + b % A.N) * (size_t)(A.H * A.Nu) + lane; stride = A.Nu; }
  if (weighs) { x = A.rewss + (size_t)b * A.H; stride = 1; }
  const float* __restrict__ yb = lazy ? A.ybar + lane : A.q;
  const int ystride = lazy ? A.Nu : 0;
  const float* __restrict__ w = A.w ? A.w : A.q;  // (uniform; without row weights acc is not looked at)
  const int wstride = A.w ? 1 : 0;
  bool have = act && A.prev;
  float up = have ? A.prev[lane] : 0.0f, eff = 0.0f, rat = 0.0f, acc = 0.0f;
#pragma unroll 4
  for (int h = 0; h < A.H; ++h) {
    const float v = x[h * stride];
    objective_column_step(objective_value(v, lazy, A.sigma, yb[h * ystride]), up, have, eff, rat);
    acc = objective_ret_step(acc, w[h * wstride], v);
  }
  const float term = act ? objective_term(A.q[lane], A.effort, eff, A.rate, rat) : 0.0f;
  float c = 0.0f;
  if (A.costs) {  // (uniform)
    for (int a = 0; a < A.Nu; ++a) c = c + __shfl(term, a, kObjLanes);
    c = c / (float)A.H;
  }
  if (last) {
    const float ret = A.w ? acc / A.wsum : A.rews[b];
    A.rews[b] = A.costs ? ret - c : ret;
    A.ret_keep[b] = ret;
    if (b < A.N) A.cost_keep[b] = c;
  }
}
static __global__ __launch_bounds__(kObjThreads) void objective_kernel(ObjectiveArgs A) { objective_body(A); }
// ... and for the P plans of a sweep, blockIdx.y = plan: plan k's N rows, candidates, results and previous action lie N rows,
// N candidates and Nu floats from plan 0's, its Ybar_i ybar_stride floats from plan 0's; B = N
static __global__ __launch_bounds__(kObjThreads) void objective_batch_kernel(ObjectiveArgs A, long long ybar_stride) {
  const long long k = blockIdx.y;
  A.rewss += k * A.N * A.H; A.rews += k * A.N; A.cand += k * A.N * (long long)(A.H * A.Nu);
  if (A.ybar) A.ybar += k * ybar_stride;
  if (A.prev) A.prev += k * A.Nu;
  A.ret_keep += k * A.N; A.cost_keep += k * A.N;
  objective_body(A);
}
inline unsigned objective_blocks(int B) { return (unsigned)((B + kObjThreads / kObjLanes - 1) / (kObjThreads / kObjLanes)); }
// The previous action of the NEXT tick of an episode or a session, one launch per tick in front of the boundary kernel:
// prev[k][a] = clip(src[k][a], -1, 1), src = row E-1 of episode k's mean M_t (src_stride floats from episode 0's) — or, in front
// of the first tick of an episode with a delay record, the last row of its committed queue.  blockIdx.y = episode.
static __global__ __launch_bounds__(64) void objective_prev_kernel(const float* __restrict__ src, long long src_stride, int Nu,
                                                             float* __restrict__ prev) {
  const int a = threadIdx.x;
  if (a < Nu) prev[(long long)blockIdx.y * Nu + a] = fclip(src[(long long)blockIdx.y * src_stride + a], -1.0f, 1.0f);
}

// ---- the pick record (mbd_plan_set_mpc_pick, include/mbd_hip.h mbd_mpc_pick; DESIGN.md section 1 "N15 pick"): what a tick hands
// on — its mean, the incumbent, or the best candidate of its last step.  Two kernels around one small rollout launch, behind the
// tick's last update kernel (the order of the argmax, pick_finite ... pick_argmax_block: mbd_step_device.h) ----
// the three plans of a tick that a choice is made among, per plan k (blockIdx.y; every pointer is plan 0's, plan k's lies its stride
// further): slot 0 = M, slot 1 = B (cold bit k set: M), slot 2 = candidate n* (none: M)
struct PickGather {
  const float* rews;    // [N] the rewards the last step's score read
  long long rews_stride;
  int N, HNu;
  const float* cand;    // [N][HNu] that step's candidates, or their normals (lazy)
  long long cand_stride;
  int lazy;
  float sigma;          // lazy: sigma_i ...
  const float* ybar_i;  // ... and Ybar_i [HNu] of that step
  long long ybar_i_stride;
  const float* M;       // [HNu] the tick's result
  long long M_stride;
  const float* B;       // [HNu] the Ybar the tick started from
  long long B_stride;
  unsigned cold;        // bit k: plan k's tick was cold — it has no incumbent
  float* slots;         // [3][HNu], plan k's 3 HNu further
  int* best;            // [1] n*, plan k's one further
};
// ONE 1024-thread workgroup per plan: n*, then the three slots — the candidate formed as mbd_plan_peek forms it (shift_kernel's
// element: eps * sigma rounded, + Ybar_i rounded, clipped; a materialised plan's row as it stands).  n* is read by every thread from
// the same LDS words (uniform) and never leaves the device.  Plain vector loads and stores.
static __global__ __launch_bounds__(kScoreThreads) void pick_gather_kernel(PickGather A) {
  const long long k = blockIdx.y;
  __shared__ float red_v[kScoreThreads / 64];
  __shared__ int red_i[kScoreThreads / 64];
  const int best = pick_argmax_block(A.rews + k * A.rews_stride, A.N, red_v, red_i);
  const float* __restrict__ M = A.M + k * A.M_stride;
  const float* __restrict__ B = A.B + k * A.B_stride;
  const float* __restrict__ yb = A.lazy ? A.ybar_i + k * A.ybar_i_stride : M;
  const float* __restrict__ row = best >= 0 ? A.cand + k * A.cand_stride + (long long)best * A.HNu : M;
  const bool lazy = A.lazy && best >= 0;
  const bool has_prev = !((A.cold >> k) & 1u);
  float* __restrict__ out = A.slots + k * 3 * A.HNu;
  for (int e = threadIdx.x; e < A.HNu; e += kScoreThreads) {
    const float m = M[e];
    const float x = row[e];
    out[e] = m;
    out[A.HNu + e] = has_prev ? B[e] : m;
    out[2 * A.HNu + e] = lazy ? fclip(x * A.sigma + yb[e], -1.0f, 1.0f) : x;
  }
  if (threadIdx.x == 0) A.best[k] = best;
}
// the argmax alone over P rows of N rewards (mbd_debug_pick_best)
static __global__ __launch_bounds__(kScoreThreads) void pick_best_probe_kernel(const float* __restrict__ rews, int N, int* __restrict__ best) {
  __shared__ float red_v[kScoreThreads / 64];
  __shared__ int red_i[kScoreThreads / 64];
  const int b = pick_argmax_block(rews + (long long)blockIdx.y * N, N, red_v, red_i);
  if (threadIdx.x == 0) best[blockIdx.y] = b;
}
// ONE 256-thread workgroup per plan, behind the rollout (and the objective launch) of the three slots: the choice c — in slot order,
// a slot that is enabled, present and of finite return takes over on strictly greater; none: 0 —, slot c over the tick's result
// where it lies (every consumer of M_t downstream then reads P_t), and the tick's log entry through thread 0.  c is decided by
// every thread from the same three loads: uniform.
struct PickChoose {
  const float* rets;   // [3], plan k's 3 further
  const float* slots;  // [3][HNu]
  const int* best;
  int HNu, mask;
  unsigned cold;
  float* out;          // [HNu] the tick's result, plan k's out_stride further
  long long out_stride;
  int* log_choice;     // the tick's entry of plan 0's logs; plan k's log_stride entries further (rets: 3 floats per entry)
  float* log_rets;
  int* log_best;
  long long log_stride;
};
static __global__ __launch_bounds__(256) void pick_choose_kernel(PickChoose A) {
  const long long k = blockIdx.y;
  const float* __restrict__ rets = A.rets + k * 3;
  const int best = A.best[k];
  const float r[3] = {rets[0], rets[1], rets[2]};
  const bool present[3] = {true, !((A.cold >> k) & 1u), best >= 0};
  int c = -1;
  float rc = 0.0f;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const bool take = ((A.mask >> j) & 1) && present[j] && pick_finite(r[j]) && (c < 0 || r[j] > rc);
    rc = take ? r[j] : rc;
    c = take ? j : c;
  }
  if (c < 0) c = 0;
  const float* __restrict__ src = A.slots + (k * 3 + c) * A.HNu;
  float* __restrict__ out = A.out + k * A.out_stride;
  for (int e = threadIdx.x; e < A.HNu; e += 256) out[e] = src[e];
  if (threadIdx.x == 0) {
    A.log_choice[k * A.log_stride] = c;
    float* lr = A.log_rets + k * A.log_stride * 3;
    lr[0] = r[0]; lr[1] = r[1]; lr[2] = r[2];
    A.log_best[k * A.log_stride] = best;
  }
}

// ---- the terminal value (mbd_plan_set_value, include/mbd_hip.h mbd_value): behind a rollout launch (and the objective's), the
// rows' final states -> rews[b] = rews[b] + (scale * V(s_H)) ----
// The arithmetic of one row is the functions below, host and device text: mbd_debug_value_host loops them on the CPU, where a test
// without a device holds them to the checker.  f32, every operation rounded (the build's -ffp-contract=off; the fma is explicit).
constexpr int kValueMaxLayers = 4;
constexpr int kValueMaxWidth = 256;
// input j of a row whose final state is s: under REL_XY the x and y of every link (floats 0 and 1 of its 13) less link 0's
MBD_HD float value_input(const float* __restrict__ s, int j, int rel, const float* __restrict__ center,
                         const float* __restrict__ in_scale) {
  float v = s[j];
  const int c = j % MBD_LINK_STATE;
  if (rel && c < 2) v = v - s[c];
  return (v - center[j]) * in_scale[j];
}
MBD_HD float value_step(float w, float x, float a) { return ffma(w, x, a); }
MBD_HD float value_relu(float a) { return a > 0.0f ? a : (a <= 0.0f ? 0.0f : a); }
MBD_HD float value_tanh(float a) {
  const float aa = fabs_(a);
  const float m = aa < 44.0f ? aa : 44.0f;
  const float t = exp_(-2.0f * m);
  const float y = (1.0f - t) / (1.0f + t);
  return a != a ? a : __builtin_copysignf(y, a);
}
MBD_HD float value_act(float a, int act) { return act == 1 ? value_tanh(a) : value_relu(a); }
MBD_HD float value_add(float rew, float scale, float V) { return rew + scale * V; }

// The net on the device: layer l's weights TRANSPOSED, Wt[l] [K_l][width_l] (K_l: the layer's inputs), so that the lanes of a
// wavefront — output units — read one row k with consecutive addresses.
struct ValueArgs {
  const float* fin;   // [B][S] the rows' final states
  float* rews;        // [B] in / out, or nullptr: V only (mbd_plan_eval_value)
  float* v_keep;      // [B] V
  int B, S, n_layers, act, rel;
  int width[kValueMaxLayers];
  const float* Wt[kValueMaxLayers];
  const float* b[kValueMaxLayers];
  const float* center;    // [S]
  const float* in_scale;  // [S]
  float scale;
};
// One workgroup takes a tile of C rows; its threads are output units.  The tile's activations lie in LDS as x[k][C]: in the loop
// over k every lane reads the SAME C floats (a broadcast: no bank conflict, one ds_read_b128 per four rows) and one weight of its
// own, and runs C independent fma chains in registers — the contract fixes the order within a (row, output) chain only, and each
// chain here runs k ascending from its bias.  A weight is read once per workgroup and used C times.  The last layer has one output:
// there the lanes are the tile's rows instead (lane c walks row c's chain; the weight is the uniform operand).  No MFMA: the matrix
// unit sums a tile's products in an order of its own that no checker can restate in float32, and this contract is bit for bit.
// Rows never meet: row c of the tile has its own accumulators and its own column of x; rows >= B stage zeros, compute and store
// nothing.  Bounds: fin is read at rows < B only, x0 / x1 hold kValueMaxWidth x C floats and every width and S is <= kValueMaxWidth
// (the set call), thread o writes x[o][.] only for o < width <= kValueMaxWidth.  Plain vector loads and stores.
template <int C>
static __global__ __launch_bounds__(kValueMaxWidth) void value_kernel(ValueArgs A) {
  static_assert(MBD_MAX_LINKS * MBD_LINK_STATE <= kValueMaxWidth, "a state record fits the activation buffers");
  __shared__ float xa[kValueMaxWidth * C];
  __shared__ float xb[kValueMaxWidth * C];
  const int tid = threadIdx.x;
  const int row0 = blockIdx.x * C;
  for (int e = tid; e < A.S * C; e += blockDim.x) {  // x_0, e = c S + j: consecutive threads read consecutive floats of a row
    const int c = e / A.S, j = e - c * A.S;
    const int b = row0 + c;
    xa[j * C + c] = b < A.B ? value_input(A.fin + (size_t)b * A.S, j, A.rel, A.center, A.in_scale) : 0.0f;
  }
  __syncthreads();
  float* xin = xa;
  float* xout = xb;
  int K = A.S;
  for (int l = 0; l + 1 < A.n_layers; ++l) {  // the hidden layers
    const int W = A.width[l];
    if (tid < W) {
      const float* __restrict__ w = A.Wt[l] + tid;
      const float bias = A.b[l][tid];
      float acc[C];
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] = bias;
#pragma unroll 8
      for (int k = 0; k < K; ++k) {  // (the loads do not depend on the chains: unrolled, eight weights are in flight)
        const float wv = w[(size_t)k * W];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = value_step(wv, xin[k * C + c], acc[c]);
      }
#pragma unroll
      for (int c = 0; c < C; ++c) xout[tid * C + c] = value_act(acc[c], A.act);
    }
    __syncthreads();
    float* t = xin; xin = xout; xout = t;
    K = W;
  }
  if (tid < C && row0 + tid < A.B) {  // the last layer: lane = row of the tile
    const int l = A.n_layers - 1;
    const float* __restrict__ w = A.Wt[l];
    float a = A.b[l][0];
#pragma unroll 8
    for (int k = 0; k < K; ++k) a = value_step(w[k], xin[k * C + tid], a);
    const int b = row0 + tid;
    A.v_keep[b] = a;
    if (A.rews) A.rews[b] = value_add(A.rews[b], A.scale, a);
  }
}

// ---- the adapt record (mbd_plan_set_adapt, include/mbd_hip.h mbd_adapt): behind a step's update kernel, the weighted spread of the
// step's candidates per element -> the table a and G = a * g the next step samples under (the rule, AdaptRule: mbd_step_device.h) ----
// The arithmetic of one element is the functions below, host and device text: mbd_debug_adapt_host loops them on the CPU, where a
// test without a device holds them to the checker.  f32, every operation rounded (the build's -ffp-contract=off; the fma is explicit).
// the candidate's value as the weighted mean forms it (wmean_kernel's val)
MBD_HD float adapt_value(float x, int lazy, float sigma, float yb) { return lazy ? fclip(x * sigma + yb, -1.0f, 1.0f) : x; }
// one candidate's term of the two chains of an element
MBD_HD void adapt_chain(float w, float y, float yb, float& m1, float& m2) {
  const float d = y - yb;
  m1 = ffma(w, d, m1);
  m2 = ffma(w, d * d, m2);
}
MBD_HD float adapt_var(float m1, float m2) {
  const float v = m2 - m1 * m1;
  return v < 0.0f ? 0.0f : v;  // (a NaN stays)
}
MBD_HD float adapt_s(float var, float sigma, float G) { return fsqrt(var) / (sigma * G); }
MBD_HD float adapt_ratio(float sumsq, int n_active) { return fsqrt(sumsq / (float)n_active); }
MBD_HD bool adapt_skip(float S, int n_active) { return n_active == 0 || !(S > 0.0f) || !(S < __builtin_inff()); }
MBD_HD float adapt_next(float a, float s, float S, const AdaptRule& R) {
  const float t = a * (s / S);
  const float v = a + R.rate * (t - a);
  return v < R.a_min ? R.a_min : (v > R.a_max ? R.a_max : v);
}
MBD_HD float adapt_G(float a, const float* __restrict__ g, int e) { return g ? a * g[e] : a; }

// The spread of every element: var[e] of the contract.  The weighted mean's decomposition (wmean_kernel): a workgroup owns kWmE = 16
// consecutive outputs, in the XCD-aware tile order (xcd_tile: the tile next door shares half of every 128-byte line, so one XCD's
// workgroups take consecutive tiles), and splits the candidates into 64 groups; thread (g, j) runs the TWO chains of output j over
// n = g, g + 64, ... — a wavefront reads four 64-byte row segments per load instruction, 32 rows in flight per round while there are
// that many, then 16, then the tail —, and the 64 partials of each sum are added in group order.  The candidate tensor is read once.
// The weights: STAGE = true stages all N in LDS once per workgroup, shared by the tile's 16 outputs — while they fit the default
// 48 KB window (N <= 12288); beyond it (STAGE = false) every thread reads its weights from memory — the 16 threads of a group the
// same word, so a wavefront's load touches four distinct weights, and all workgroups the same N floats, which the L2 holds —: same
// values, same chains, same bits, and no plan size is refused.
// Bounds: rows n < N only (each round's guard), column e <= HNu - 1 (clamped; a clamped thread stores nothing), wl[i] for i < N.
// No cross-lane sum, no MFMA: the order of every sum is the contract's.  Plain vector loads and stores.
template <bool STAGE>
static __global__ __launch_bounds__(kWmE * kWmG) void adapt_spread_kernel(const float* __restrict__ weights,
                                                                   const float* __restrict__ cand, int N, int HNu,
                                                                   const float* __restrict__ Ybar_i, int lazy, float sigma,
                                                                   const float* __restrict__ sigma_dev,
                                                                   float* __restrict__ var_out) {
  extern __shared__ __attribute__((aligned(16))) float wl[];
  __shared__ float red[2][kWmG][kWmE + 1];
  const int j = threadIdx.x & (kWmE - 1), g = threadIdx.x / kWmE;
  const int e_raw = xcd_tile(blockIdx.x, gridDim.x, 0) * kWmE + j;
  const int e = e_raw < HNu ? e_raw : HNu - 1;
  const float* __restrict__ col = cand + e;
  if (sigma_dev) sigma = *sigma_dev;  // (a path-integral plan's carried sigma: what its sampler read)
  const float yb = Ybar_i[e];
  if (STAGE) {
    for (int i = threadIdx.x; i < N; i += kWmE * kWmG) wl[i] = weights[i];
    __syncthreads();
  }
  const float* __restrict__ w = STAGE ? wl : weights;
  float m1 = 0.0f, m2 = 0.0f;
  int n = g;
  for (; n + 31 * kWmG < N; n += 32 * kWmG) {
    float y[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) y[k] = col[(size_t)(n + k * kWmG) * HNu];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < 32; ++k) adapt_chain(w[n + k * kWmG], adapt_value(y[k], lazy, sigma, yb), yb, m1, m2);
  }
  for (; n + 15 * kWmG < N; n += 16 * kWmG) {
    float y[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) y[k] = col[(size_t)(n + k * kWmG) * HNu];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < 16; ++k) adapt_chain(w[n + k * kWmG], adapt_value(y[k], lazy, sigma, yb), yb, m1, m2);
  }
  for (; n < N; n += kWmG) adapt_chain(w[n], adapt_value(col[(size_t)n * HNu], lazy, sigma, yb), yb, m1, m2);
  red[0][g][j] = m1;
  red[1][g][j] = m2;
  __syncthreads();
  if (g != 0 || e_raw >= HNu) return;
  float t1 = red[0][0][j], t2 = red[1][0][j];
#pragma unroll 8
  for (int k = 1; k < kWmG; ++k) {
    t1 = t1 + red[0][k][j];
    t2 = t2 + red[1][k][j];
  }
  var_out[e] = adapt_var(t1, t2);
}
// ONE workgroup: s[e] of the active elements in parallel (into buf, which arrives holding var), S by thread 0 in ascending e, then
// the new a and G of the active elements in parallel, and the log entry.  Thread t owns the elements e = t, t + 256, ... in both
// parallel passes, so a[e] and G[e] are read and written by one thread only.  The sum of S crosses to thread 0 through LDS, a chunk
// of kAdaptChunk squares at a time: its chain then waits for LDS reads, which the compiler batches, not for a memory round trip per
// element (850 dependent adds behind L2 loads took 83 us at humanoidrun, the whole rollout takes 504).  A frozen element's slot holds
// +0: the accumulator is +0, positive or NaN, so adding +0 leaves its bits — the sum is the contract's sum over the active elements
// in ascending e.  n_active is an integer count: an LDS atomic, whose order does not matter.  The trip counts are uniform.
constexpr int kAdaptThreads = 256, kAdaptChunk = 2048;
static __global__ __launch_bounds__(kAdaptThreads) void adapt_finish_kernel(float* __restrict__ buf, int HNu, float sigma,
                                                                     const float* __restrict__ sigma_dev, float* __restrict__ a,
                                                                     const float* __restrict__ g, float* __restrict__ G,
                                                                     AdaptRule R, float* __restrict__ log_S,
                                                                     int* __restrict__ log_skipped) {
  __shared__ float q[kAdaptChunk];
  __shared__ float sh_S;
  __shared__ int sh_skip, sh_n;
  if (sigma_dev) sigma = *sigma_dev;
  if (threadIdx.x == 0) sh_n = 0;
  int mine = 0;
  float acc = 0.0f;  // (thread 0's)
  for (int base = 0; base < HNu; base += kAdaptChunk) {
    const int cnt = HNu - base < kAdaptChunk ? HNu - base : kAdaptChunk;
    for (int k = threadIdx.x; k < cnt; k += kAdaptThreads) {
      const int e = base + k;
      const float Ge = G[e];
      const bool active = Ge > 0.0f;
      const float s = active ? adapt_s(buf[e], sigma, Ge) : 0.0f;
      buf[e] = s;
      q[k] = s * s;
      mine += active ? 1 : 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll 16
      for (int k = 0; k < cnt; ++k) acc = acc + q[k];
    }
    __syncthreads();
  }
  atomicAdd(&sh_n, mine);
  __syncthreads();
  if (threadIdx.x == 0) {
    const int n_active = sh_n;
    const float S = adapt_ratio(acc, n_active);
    const bool skip = adapt_skip(S, n_active);
    sh_S = S;
    sh_skip = skip ? 1 : 0;
    *log_S = S;
    *log_skipped = skip ? 1 : 0;
  }
  __syncthreads();
  if (sh_skip) return;
  const float S = sh_S;
  for (int e = threadIdx.x; e < HNu; e += kAdaptThreads) {
    if (!(G[e] > 0.0f)) continue;
    const float an = adapt_next(a[e], buf[e], S, R);
    a[e] = an;
    G[e] = adapt_G(an, g, e);
  }
}
// The table at the start of a run or a tick, and whenever the shape in force changes: shift < 0: a = ones; otherwise a[e] =
// a[e + shift], ones past the end (shift = 0: a as it is); then G = a * g under the shape g now in force (nullptr: none).  ONE
// workgroup; the shift is in place, so a block of 256 elements is read, then — behind a barrier — written: a later block reads
// only elements no earlier block wrote (its reads start at or behind its own first element).  The trip count is uniform.
static __global__ __launch_bounds__(kAdaptThreads) void adapt_table_kernel(float* __restrict__ a, float* __restrict__ G,
                                                                    const float* __restrict__ g, int HNu, int shift) {
  for (int base = 0; base < HNu; base += kAdaptThreads) {
    const int e = base + threadIdx.x;
    float v = 1.0f;
    if (e < HNu && shift >= 0 && e + shift < HNu) v = a[e + shift];
    __syncthreads();
    if (e < HNu) {
      a[e] = v;
      G[e] = adapt_G(v, g, e);
    }
    __syncthreads();
  }
}

// ---- the zone record (mbd_plan_set_zones, include/mbd_hip.h mbd_zones; DESIGN.md section 1 "N20 zones"): behind a rollout launch
// that wrote the tracked links' positions (and behind the objective's launch), rews[b] = rews[b] - pen[b] ----
// The arithmetic of one term and one step is the functions below, host and device text: mbd_debug_zones_host loops them on the CPU,
// where a test without a device holds them to the checker.  f32, every operation rounded (the build's -ffp-contract=off).
MBD_HD float zone_dist(const float* __restrict__ x, const mbd_zone& z) {
  const float e0 = (x[0] - z.center[0]) * z.scale[0];
  const float e1 = (x[1] - z.center[1]) * z.scale[1];
  const float e2 = (x[2] - z.center[2]) * z.scale[2];
  return fsqrt((e0 * e0 + e1 * e1) + e2 * e2);
}
MBD_HD float zone_u(int kind, float d, float r, float m) { return kind == MBD_ZONE_GOAL ? (d - r) / m : ((r + m) - d) / m; }
MBD_HD float zone_term(float w, float u) {
  const float v = fclip_nan(u, 0.0f, 1.0f);
  return w * (v * v);
}
// the minimum in which a NaN wins whichever side it stands on; zone_canon: the one NaN that is stored
MBD_HD float zone_min(float a, float b) { return a != a ? a : (b != b ? b : (b < a ? b : a)); }
MBD_HD float zone_canon(float v) { return v != v ? __builtin_bit_cast(float, 0x7fc00000u) : v; }
// One step: x [K][3] the tracked positions; s_t and clr_t of the contract, slot k outer and zone z inner.  The table's values do not
// depend on the lane: on the device they are scalar operands from the kernel's argument segment.
MBD_HD void zone_step(const float* __restrict__ x, int K, const mbd_zones& Z, float& s_t, float& clr_t) {
  float s = 0.0f, c = __builtin_inff();
  for (int k = 0; k < K; ++k) {
    const float xk[3] = {x[3 * k], x[3 * k + 1], x[3 * k + 2]};
    for (int z = 0; z < Z.n_zones; ++z) {
      const mbd_zone& zn = Z.zone[z];
      if (!((zn.links >> k) & 1u)) continue;
      const float d = zone_dist(xk, zn);
      s = s + zone_term(zn.weight, zone_u(zn.kind, d, zn.radius, zn.margin));
      if (zn.kind == MBD_ZONE_KEEP_OUT) c = zone_min(c, d - zn.radius);
    }
  }
  s_t = s;
  clr_t = c;
}

// One wavefront per row, kZoneRows rows per workgroup.  A lane owns steps t = lane, lane + 64, ...: it reads its K 3 contiguous
// floats, forms s_t and clr_t and leaves s_t in LDS; lane 0 of the row then runs the contract's ascending chain over the 64 steps of
// the pass (the loads of the chain do not depend on it).  The minimum crosses lanes (zone_min is order-free: a NaN wins on either
// side, and the stored NaN is canonical); no sum does.  The table is a kernel argument: nothing of it lives in device memory.
// Bounds: a row b >= B loads and stores nothing (it still meets the barriers: H does not depend on the row); a step t >= H
// likewise; a load is xpos[((b H + t) K + k) 3 + i] with b < B, t < H, k < K; the stores are rews / pen_keep / clr_keep [b] and
// step_pen / step_clr [b H + t].  LDS: kZoneRows x 64 floats.  Plain vector loads and stores.
constexpr int kZoneRows = 4;
struct ZoneArgs {
  const float* xpos;  // [B][H][K][3]
  float* rews;        // [B] in / out, or nullptr: the outputs below only
  float* pen_keep;    // [B] pen, or nullptr
  float* clr_keep;    // [B] clr, or nullptr
  float* step_pen;    // [B][H] s_t, or nullptr (planning launches)
  float* step_clr;    // [B][H] clr_t, or nullptr
  int B, H, K;
  mbd_zones Z;
};
static __global__ __launch_bounds__(64 * kZoneRows) void zones_kernel(ZoneArgs A) {
  __shared__ float sh[kZoneRows][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long b = (long long)blockIdx.x * kZoneRows + wave;
  const bool live = b < A.B;
  float pen = 0.0f, clr = __builtin_inff();
  for (int t0 = 0; t0 < A.H; t0 += 64) {
    const int t = t0 + lane;
    float s_t = 0.0f, c_t = __builtin_inff();
    if (live && t < A.H) {
      const size_t at = (size_t)b * A.H + t;
      zone_step(A.xpos + at * A.K * 3, A.K, A.Z, s_t, c_t);
      if (A.step_pen) A.step_pen[at] = s_t;
      if (A.step_clr) A.step_clr[at] = zone_canon(c_t);
      clr = zone_min(clr, c_t);
    }
    sh[wave][lane] = s_t;
    __syncthreads();
    if (live && lane == 0) {
      const int n = A.H - t0 < 64 ? A.H - t0 : 64;
      for (int j = 0; j < n; ++j) pen = pen + sh[wave][j];
    }
    __syncthreads();
  }
  for (int off = 32; off; off >>= 1) clr = zone_min(clr, __shfl_xor(clr, off, 64));
  if (live && lane == 0) {
    pen = pen / (float)A.H;
    if (A.pen_keep) A.pen_keep[b] = pen;
    if (A.clr_keep) A.clr_keep[b] = zone_canon(clr);
    if (A.rews) A.rews[b] = A.rews[b] - pen;
  }
}

}  // namespace mbd
