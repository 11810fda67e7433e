// mbd_sweep.hip — sweeps (include/mbd_hip.h): several plans of one env advanced in lockstep, one rollout launch over all
// their candidates per step (mbd/scripts/run_mbd.py:17-64); MBD plans and the path-integral baselines.  The sweep handle, its
// ring of noise buffers (sweep_step: another protocol than a plan's NoiseRing) and the batched receding-horizon loop.
#define MBD_WEIGH_KERNEL 1  // this unit launches weigh_kernel (mbd_step_kernels.h)
#define MBD_ELITE_KERNEL 1  // ... and the elite and to-go records' batch kernels
#define MBD_TOGO_KERNEL 1
#define MBD_SWEEP_KERNEL 1  // (their forms over P plans: this unit's alone)
#include "mbd_internal.h"
#include "mbd_step_kernels.h"
#include "../../include/mbd_hip_debug.h"

namespace {
// The elite record's launches for the P plans of a sweep (mbd_internal.h EliteRec): the batch kernels, which take the plans' strides
// (EliteBatch) and the mask of the plans that take part (bit k: plan k).
EliteBatch elite_batch(const EliteRec& L, long long cand, long long ybar, long long rews, int HNu, unsigned mask) {
  EliteBatch B{};
  B.cand = cand; B.ybar = ybar; B.rews = rews; B.E = (long long)L.rows * HNu; B.R = L.rows; B.log = L.log_cap; B.mask = mask;
  return B;
}
// the plans' elites at the start of a run or a tick: shift[k] < 0 empties plan k's, otherwise its rows move shift[k] elements forward
int elite_table(EliteRec& L, int P, int HNu, const EliteShifts& sh, unsigned mask, hipStream_t s) {
  if (!L.has) return MBD_OK;
  hipLaunchKernelGGL(elite_shift_batch_kernel, dim3((unsigned)L.rows, (unsigned)P), dim3(kEliteThreads), 0, s, L.d_E.get(), L.d_count.get(), HNu,
                     sh, elite_batch(L, 0, 0, 0, HNu, mask));
  HIP_TRY(hipGetLastError());
  return MBD_OK;
}
int elite_table_all(EliteRec& L, int P, int HNu, int shift, hipStream_t s) {
  EliteShifts sh;
  for (int& v : sh.s) v = shift;
  return elite_table(L, P, HNu, sh, 0xffffffffu, s);
}
// behind the launch that made the step's normals or candidates, in front of the rollout (a plan's elite_inject per plan)
int elite_inject(EliteRec& L, int P, float* cand, long long cand_stride, int HNu, int lazy, float sigma, const float* ybar,
                 long long ybar_stride, const float* g, unsigned mask, hipStream_t s) {
  if (!L.has) return MBD_OK;
  EliteInject A{};
  A.cand = cand; A.HNu = HNu; A.ybar_i = ybar; A.lazy = lazy; A.sigma = sigma; A.g = g;
  A.n_elites = L.n; A.nominal = L.nominal; A.E = L.d_E; A.count = L.d_count;
  const long long total = (long long)(L.nominal + L.n) * HNu;
  hipLaunchKernelGGL(elite_inject_batch_kernel, dim3((unsigned)((total + kEliteThreads - 1) / kEliteThreads), (unsigned)P),
                     dim3(kEliteThreads), 0, s, A, elite_batch(L, cand_stride, ybar_stride, 0, HNu, mask));
  HIP_TRY(hipGetLastError());
  return MBD_OK;
}
// behind the step's update kernel (a plan's elite_select per plan); the plans of the mask gain a log entry, each at its own ring's slot
int elite_select(EliteRec& L, int P, const float* rews, int N, const float* cand, long long cand_stride, int HNu, int lazy, float sigma,
                 const float* ybar, long long ybar_stride, unsigned mask, hipStream_t s) {
  if (!L.has) return MBD_OK;
  EliteSelect A{};
  A.rews = rews; A.N = N; A.HNu = HNu; A.cand = cand; A.lazy = lazy; A.sigma = sigma; A.ybar_i = ybar;
  A.n_elites = L.n; A.nominal = L.nominal; A.E = L.d_E; A.R = L.d_R; A.src = L.d_src; A.count = L.d_count;
  A.log_count = L.d_log_count; A.log_kept = L.d_log_kept; A.log_top = L.d_log_top;
  EliteBatch B = elite_batch(L, cand_stride, ybar_stride, N, HNu, mask);
  EliteShifts slots;  // (plan k's entry lies at slot[k] of its own ring)
  for (int k = 0; k < MBD_SWEEP_MAX_PLANS; ++k) slots.s[k] = 0;
  for (int k = 0; k < P; ++k)
    if ((mask >> k) & 1u) slots.s[k] = (int)ring_slot(L.steps[k], L.log_cap);
  hipLaunchKernelGGL(elite_select_batch_kernel, dim3(1, (unsigned)P), dim3(kScoreThreads), 0, s, A, B, slots);
  HIP_TRY(hipGetLastError());
  return MBD_OK;
}

// The to-go record's two launches for the P plans of a sweep (mbd_internal.h TogoRec), where the batch score + weighted mean stands:
// A and sb carry everything but the layout and R, W
int togo_launch(TogoRec& L, int P, const float* d_rewss, TogoUpdate A, const ScoreBatch& sb, hipStream_t s) {
  const int block = L.block, G = L.G;
  const TogoReturns Rt{A.rews, d_rewss, L.d_R.get(), A.N, A.H, block, G};
  const long long PN = (long long)P * A.N;
  hipLaunchKernelGGL(togo_returns_batch_kernel, dim3((unsigned)((PN + kTogoThreads - 1) / kTogoThreads)), dim3(kTogoThreads), 0, s, Rt, P);
  HIP_TRY(hipGetLastError());
  const long long last = (long long)(A.H - togo_start(G - 1, block)) * A.Nu;
  A.R = L.d_R; A.W = L.d_W; A.G = G; A.block = block;
  A.tpg = G > 1 ? (int)(((long long)block * A.Nu + kWmE - 1) / kWmE) : 1;
  A.T = (G - 1) * A.tpg + (int)((last + kWmE - 1) / kWmE);
  hipLaunchKernelGGL(togo_update_batch_kernel, dim3((unsigned)A.T, (unsigned)P), dim3(kWmE * kWmG), sizeof(float) * (size_t)A.N, s, A, sb);
  HIP_TRY(hipGetLastError());
  L.stepped = true;
  return MBD_OK;
}

// outputs per thread of the sweeps' score + weighted mean launch (score_wmean_batch_kernel<V>): 2 — a workgroup owns 32 outputs,
// 128 bytes of every candidate row, P x 27 workgroups for the humanoid.  Measured on sweep8 (profiles/r05_score_ab.txt; the
// launch's algorithmic bytes are 28.0 MB): V = 1 15.5 us / 48.2 MB, V = 2 11.3 us / 28.2 MB, V = 4 22.0 us / 28.2 MB.
// MBD_WMEAN_V = 1 / 2 / 4 forces it (A/B, tests; same bits whatever it is) — where it fits: the launch asks for 4 N bytes of
// dynamic LDS beside the kernel's own red[64][16 V + 1] and red_s[32] (the gfx950 code object's fixed group segment: 4480, 8576,
// 16 768 bytes for V = 1, 2, 4; 128 fewer in the GIVEN form), and nothing raises the launch's 64 KiB limit.  V = 4 passes it
// above N = 12 192 of the 12 288 candidates a sweep accepts: there the launch takes 2 (57 728 bytes at most).
int wmean_batch_v(int N) {
  const int v = lever("MBD_WMEAN_V");
  if (v != 1 && v != 2 && v != 4) return 2;
  const size_t fixed = sizeof(float) * (size_t)(mbd::kWmG * (mbd::kWmE * v + 1) + 2 * (mbd::kScoreThreads / 64));
  return fixed + sizeof(float) * (size_t)N <= 64 * 1024 ? v : 2;
}
// given: under a weighting record — weigh_kernel has written every plan's weights and mean reward, the launch loads the weights
// where it would derive them (score_wmean_body's GIVEN form; the same grid, tiles and plan-to-XCD mapping)
template <typename... Args>
void launch_score_wmean_batch(int V, bool given, int HNu, int P, size_t lds, hipStream_t s, Args... args) {
  using namespace mbd;
  const dim3 block(kWmE * kWmG);
  auto tiles = [&](int v) { return dim3((unsigned)((HNu + kWmE * v - 1) / (kWmE * v)), (unsigned)P); };
  if (given) {
    if (V == 1) hipLaunchKernelGGL((score_wmean_batch_kernel<1, true>), tiles(1), block, lds, s, args...);
    else if (V == 2) hipLaunchKernelGGL((score_wmean_batch_kernel<2, true>), tiles(2), block, lds, s, args...);
    else hipLaunchKernelGGL((score_wmean_batch_kernel<4, true>), tiles(4), block, lds, s, args...);
    return;
  }
  if (V == 1) hipLaunchKernelGGL(score_wmean_batch_kernel<1>, tiles(1), block, lds, s, args...);
  else if (V == 2) hipLaunchKernelGGL(score_wmean_batch_kernel<2>, tiles(2), block, lds, s, args...);
  else hipLaunchKernelGGL(score_wmean_batch_kernel<4>, tiles(4), block, lds, s, args...);
}
// the weigh kernel over the P plans of a step (blockIdx.y = plan), in front of the launch that consumes its weights
int launch_weigh_batch(WeightingRec& wt, int P, int N, int Nd, const float* d_rews, float temp, const float* d_temps, float* d_weights,
                       float* d_rew_mean, hipStream_t s) {
  using namespace mbd;
  PiBatch pb;
  pb.rews = N; pb.weights = N; pb.mean = Nd - 1; pb.temps = d_temps;
  hipLaunchKernelGGL(weigh_kernel, dim3(1, (unsigned)P), dim3(kScoreThreads), sizeof(float) * (size_t)N, s, d_rews, N, temp, wt.rec,
                     d_weights, d_rew_mean, (float*)nullptr, wt.slot(), pb);
  HIP_TRY(hipGetLastError());
  return MBD_OK;
}
}  // namespace

// A sweep's session (include/mbd_hip.h mbd_sweep_mpc_open): P episodes the caller drives in lockstep, one tick per call.  All
// zero: no session.
struct SweepSession {
  bool open = false, in_flight = false;
  mbd_mpc_config mc{};
  std::vector<uint32_t> rng;            // [P][2] the episodes' key chains: rng, k_t = split(rng) per tick
  bool cold[MBD_SWEEP_MAX_PLANS] = {};  // episode k's next tick runs Ndiffuse-1 steps from Ybar = zeros
  int flags[MBD_SWEEP_MAX_PLANS] = {};  // of the tick in flight: what the host decided (COLD, STATE_NONFINITE)
  int t = 0, qbuf = 0;
  PinnedBuf stage, mailbox;             // the states on their way up [P][S]; the results on their way down
  Event done;
  std::chrono::steady_clock::time_point t_submit{};
};

// ---- sweeps: P plans of one env in lockstep (mbd/scripts/run_mbd.py:17-64) ---------------------------------------
struct mbd_sweep {
  mbd_env* env = nullptr;
  mbd_plan_config cfg;
  int P = 0, HNu = 0, Nu = 0;
  std::vector<float> temps, alphas, alphas_bar, sigmas;
  Stream stream, aux;
  // The normals of a step live in a ring of THREE buffers, so that the stream of the steps carries no event at all: the
  // buffer step k+1's normals go into was last read by step k-2's weighted mean — with an elite record by step k-2's selection,
  // the launch behind it on the same stream; the record's injection into a buffer is on that stream too, behind the wait for
  // ev_ready and in front of every reader —, which has finished once the rollout of step k-1 has STARTED — the host learns that from the progress word the rollout launches store into (pinned memory),
  // and the loop stays that close behind the device.  (Two buffers + events: a record behind every weighted mean and a
  // wait in front of every rollout idled the queue 17 us per step, profiles/r03_ring_ab.txt.)
  Event ev_ready[3];  // eps[b] holds the normals of its step (recorded on aux)
  Event ev_order;     // the event-ordered fallback of a loop whose stream is slower than kInStepWaitMs (created on first use)
  PinnedWord h_progress;
  DevBuf<float> d_state0, d_eps[3], d_rews, d_rewss, d_lp, d_xpos, d_weights, d_zero, d_mu, d_rewmeans, d_temps, d_final, d_final_rew;
  // path-integral sweeps (update_method != 0; path_integral.py:111-127): materialised candidates, the carried sigma of
  // every plan, cma-es' spread, cem's selection
  DevBuf<float> d_Y0s, d_sigma, d_spread;
  DevBuf<int> d_idx;
  // batched receding-horizon episodes (mbd_sweep_run_mpc): the episodes' logs, TICK-major — states [T+1][P][state_size],
  // means [T][P][HNu], rewards [T][P][H-1] (E < H rows per tick) — grown on demand; the executed rows of a tick
  // [P][(H-1) Nu] (compact: what the one-candidate-per-episode rollout reads) and the next tick's first Ybar [P][HNu].
  // Sweep-owned, like a plan's.
  DevBuf<float> d_mpc_states, d_mpc_means, d_mpc_rewards, d_mpc_rows, d_mpc_ybar;
  // the episodes' plant records (mbd_sweep_set_mpc_plant; copies, the plant envs are the caller's), and what a batch with
  // records needs beyond the above: the log of the executed rows, tick-major [T][P][E Nu] — the tick's rollouts read their
  // slices of it —, the tick's normals [P][(H-1) Nu + 3] and kick values [P][3]
  mbd_mpc_plant plant_rec[MBD_SWEEP_MAX_PLANS] = {};
  bool has_plant[MBD_SWEEP_MAX_PLANS] = {};
  DevBuf<float> d_mpc_actions, d_plant_eps, d_plant_kick;
  // the delay record of all episodes (mbd_sweep_set_mpc_delay), and what a batch with one needs beyond the above: the
  // episodes' committed queues [2][P][D E Nu] (two buffers, as a plan's) and the predicted states, tick-major [T][P][state_size]
  // — slice t is what the tick's prediction launch writes and what its P N planning candidates start from.  (The executed rows
  // are the queues' heads: d_mpc_actions logs them, and the rollout of the executed rows reads its slice.)
  DelayRec delay;
  DevBuf<float> d_mpc_queue, d_mpc_pred;
  // the demo record of all episodes (mbd_sweep_set_mpc_demo): one clip and one clock, so ONE table of windows — a rollout
  // launch reads one demo table for all its candidates —; the position log and the distances are tick-major [T][P][E][K]...
  DemoRec demo;
  // the sigma record of all episodes of a path-integral sweep (mbd_sweep_set_mpc_sigma) with the log of the last batch's sigmas
  SigmaRec sigma_rec;
  // the noise shape and the noise basis of all the sweep's plans (mbd_sweep_set_noise_shape, mbd_sweep_set_noise_basis): a plan's;
  // d_knot_z [P][N][HNu]: the scratch of a path-integral sweep's knot_noise_batch_kernel in front of shift_batch_kernel
  NoiseRec noise;
  // the objective record of all the sweep's plans (mbd_sweep_set_objective): a plan's, with every plan's previous action [P][Nu]
  ObjectiveRec obj;
  // the value record of all the sweep's plans (mbd_sweep_set_value): one net, the P N rows' final states and the last step's V
  ValueRec val;
  // the weighting record of all the sweep's plans (mbd_sweep_set_weighting) with every plan's log [P][Ndiffuse - 1]
  WeightingRec wt;
  // the zone record of all the sweep's plans (mbd_sweep_set_zones): one table, the P N rows' tracked positions, pen and clr
  ZoneRec zone;
  // the pick record of all the sweep's episodes (mbd_sweep_set_mpc_pick) with every episode's slots and log
  PickRec pick;
  // the elite record of all the sweep's plans (mbd_sweep_set_elites) and the to-go record (mbd_sweep_set_togo)
  EliteRec elite;
  TogoRec togo;
  TimingPool timing;
  // the session a caller drives tick by tick (mbd_sweep_mpc_open): it uses the batch's buffers above — slice 0 of d_mpc_states for
  // the states handed in, slice 0 of d_mpc_pred, d_mpc_queue, d_mpc_ybar — so a handle runs batches or a session, not both
  SweepSession session;
  ~mbd_sweep() {  // (streams, events and buffers release themselves, on the env's device)
    if (env) (void)hipSetDevice(env->device);
  }
};

// the refusal of a call that would disturb an open session (include/mbd_hip.h mbd_sweep_mpc_close)
#define NO_SWEEP_SESSION(w, what) \
  if ((w)->session.open) return fail(MBD_ERR_STATE, what ": a session is open on this sweep (mbd_sweep_mpc_close first)")

extern "C" int mbd_sweep_create(mbd_env* env, const mbd_plan_config* cfg, int n_plans, const float* temps, mbd_sweep** out) {
  if (!env || !cfg || !out) return fail(MBD_ERR_INVALID, "NULL argument");
  if (device_count_quiet() < 1) return fail(MBD_ERR_NO_DEVICE, "no HIP device: this library has no CPU fallback");
  if (n_plans < 1 || n_plans > MBD_SWEEP_MAX_PLANS) return fail(MBD_ERR_INVALID, "n_plans=%d outside [1,%d]", n_plans, MBD_SWEEP_MAX_PLANS);
  if (cfg->Nsample < 1 || cfg->Hsample < 1 || cfg->Ndiffuse < 2) return fail(MBD_ERR_INVALID, "bad plan sizes");
  if (cfg->update_method < 0 || cfg->update_method > 3) return fail(MBD_ERR_INVALID, "update_method=%d", cfg->update_method);
  if (env->kind != ENV_MODEL) return fail(MBD_ERR_UNSUPPORTED, "sweeps batch plans on rigid-body envs; run car2d plans as plans");
  if (cfg->update_method > 0 && cfg->enable_demo) return fail(MBD_ERR_INVALID, "path-integral plans do not use demos");
  if (cfg->shard_begin != 0 || cfg->shard_count != cfg->Nsample) return fail(MBD_ERR_INVALID, "sweeps are not sharded");
  if ((size_t)cfg->Nsample * sizeof(float) > 48 * 1024)
    return fail(MBD_ERR_UNSUPPORTED, "plans of more than 12288 candidates fill the chip on their own: run them as plans");
  if (cfg->enable_demo && (!env->has_xref || cfg->Hsample != kXrefRows)) return fail(MBD_ERR_INVALID, "enable_demo: the env has no demo / H != %d", kXrefRows);
  HIP_TRY(hipSetDevice(env->device));
  std::unique_ptr<mbd_sweep> guard(new mbd_sweep());
  mbd_sweep* w = guard.get();
  w->env = env; w->cfg = *cfg; w->P = n_plans;
  const int N = cfg->Nsample, H = cfg->Hsample, Nu = env->action_size(), Nd = cfg->Ndiffuse, P = n_plans;
  w->HNu = H * Nu;
  w->Nu = Nu;
  w->temps.assign(P, cfg->temp_sample);
  if (temps) for (int k = 0; k < P; ++k) w->temps[k] = temps[k];
  host_schedule(cfg->beta0, cfg->betaT, Nd, w->alphas, w->alphas_bar, w->sigmas);
  HIP_TRY(w->stream.create());
  HIP_TRY(w->aux.create());
  for (int b = 0; b < 3; ++b) HIP_TRY(w->ev_ready[b].create());
  HIP_TRY(w->h_progress.create());
  const int K = env->model.n_track > 0 ? env->model.n_track : 1;
  const size_t PN = (size_t)P * N;
  HIP_TRY(w->d_state0.alloc((size_t)P * env->state_size()));
  if (cfg->update_method == 0) {  // MBD plans: lazy candidates, the normals in a ring of three buffers
    for (int b = 0; b < 3; ++b) HIP_TRY(w->d_eps[b].alloc(PN * w->HNu));
  } else {  // path-integral plans: the candidates themselves (their kernels read them), sigma per plan on the device
    HIP_TRY(w->d_Y0s.alloc(PN * w->HNu));
    HIP_TRY(w->d_sigma.alloc(P));
    HIP_TRY(w->d_spread.alloc((size_t)P * w->HNu));
    HIP_TRY(w->d_idx.alloc((size_t)P * 16));
  }
  HIP_TRY(w->d_rews.alloc(PN));
  HIP_TRY(w->d_rewss.alloc(PN * H));
  HIP_TRY(w->d_lp.alloc(PN));
  if (cfg->enable_demo) HIP_TRY(w->d_xpos.alloc(PN * H * K * 3));
  HIP_TRY(w->d_weights.alloc(PN));
  HIP_TRY(w->d_zero.alloc((size_t)P * w->HNu));
  HIP_TRY(hipMemset(w->d_zero, 0, sizeof(float) * (size_t)P * w->HNu));
  HIP_TRY(w->d_mu.alloc((size_t)P * (Nd - 1) * w->HNu));
  HIP_TRY(w->d_rewmeans.alloc((size_t)P * (Nd - 1)));
  HIP_TRY(w->d_temps.upload(w->temps.data(), P));
  HIP_TRY(w->d_final.alloc((size_t)P * w->HNu));
  HIP_TRY(w->d_final_rew.alloc(P));
  *out = guard.release();
  return MBD_OK;
}

extern "C" int mbd_sweep_destroy(mbd_sweep* w) {
  if (w && w->session.in_flight) {  // (an open session ends here: its last kernel still writes the mailbox)
    (void)hipSetDevice(w->env->device);
    (void)hipStreamSynchronize(w->stream);
  }
  delete w;
  return MBD_OK;
}

extern "C" int mbd_sweep_set_state0(mbd_sweep* w, int k, const float* state0) {
  if (!w || !state0) return fail(MBD_ERR_INVALID, "NULL argument");
  if (k < 0 || k >= w->P) return fail(MBD_ERR_INVALID, "plan %d outside [0,%d)", k, w->P);
  NO_SWEEP_SESSION(w, "set_state0");
  HIP_TRY(hipSetDevice(w->env->device));
  const size_t S = w->env->state_size();
  HIP_TRY(hipMemcpy(w->d_state0 + (size_t)k * S, state0, sizeof(float) * S, hipMemcpyHostToDevice));
  return MBD_OK;
}

extern "C" int mbd_sweep_kernel_time(mbd_sweep* w, int enable, float* avg_ms_out, int* count_out) {
  if (!w) return fail(MBD_ERR_INVALID, "sweep is NULL");
  HIP_TRY(hipSetDevice(w->env->device));
  MBD_TRY(w->timing.average(avg_ms_out, count_out, true));
  w->timing.on = enable != 0;
  return MBD_OK;
}

// what a finished run hands back, once its stream is idle: every plan's means and mean rewards, and the reward of its final
// mean — rollout_us(state_init, Yi[-1]).mean() (mbd_planner.py:179-180), eval_us(state_init, mu_0).mean()
// (path_integral.py:146) — from one launch of P candidates
static int sweep_results(mbd_sweep* w, float* mu_0ts_out, float* rew_means_out, float* rew_final_out) {
  const int P = w->P, Nd = w->cfg.Ndiffuse, HNu = w->HNu;
  hipStream_t s = w->stream;
  const size_t mu_n = (size_t)P * (Nd - 1) * HNu;
  HIP_TRY(w->d_mu.download(mu_0ts_out, mu_n));
  HIP_TRY(w->d_rewmeans.download(rew_means_out, (size_t)P * (Nd - 1)));
  if (!rew_final_out) return MBD_OK;
  HIP_TRY(hipMemcpy2DAsync(w->d_final, sizeof(float) * HNu, w->d_mu + (size_t)(Nd - 2) * HNu,
                           sizeof(float) * (size_t)(Nd - 1) * HNu, sizeof(float) * HNu, P, hipMemcpyDeviceToDevice, s));
  const int sw[3] = {1, w->env->state_size(), 0};
  MBD_TRY(launch_rollout(w->env, w->d_state0, w->d_final, P, w->cfg.Hsample, nullptr, w->d_final_rew, nullptr, nullptr, s, nullptr, sw));
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(w->d_final_rew.download(rew_final_out, P));
  return MBD_OK;
}

// A sweep of path-integral plans (mbd/scripts/run_mbd.py:22-26,46-50 over path_integral.py:111-127): per refinement step
// ONE sampling launch (every plan's key, carried sigma and mean), ONE rollout launch over the P * N materialised
// candidates, and the update rule's kernels with blockIdx.y = plan — mppi: the fused score + weighted mean; cma-es: plus
// spread and sigma; cem: score, selection, mean of the K best.  Same kernels, same order, same bits as mbd_plan_run.
// sweep_pi_step is that lockstep step, shared by mbd_sweep_run and the path-integral episodes of mbd_sweep_run_mpc.
namespace {
// the update rule's kernels of a lockstep step, behind the value record's launch: the step's, and mbd_debug_sweep_update's on
// uploaded rewards.  step: slot of every plan's d_mu / d_rewmeans; mu_in: the mean of plan 0 the candidates were sampled around
// recs: the step's (an elite and a to-go record's launches run; mask: the plans that take part in the selection), not the debug entry's
int sweep_pi_update(mbd_sweep* w, int step, const float* mu_in, long long mu_stride, bool recs = false, unsigned mask = 0xffffffffu) {
  mbd_env* e = w->env;
  const mbd_plan_config& c = w->cfg;
  const int P = w->P, N = c.Nsample, Nd = c.Ndiffuse, HNu = w->HNu;
  hipStream_t s = w->stream;
  const uint64_t per_plan = (uint64_t)N * HNu;
  const dim3 b64(64);
  PiBatch pb;
  pb.rews = N; pb.weights = N; pb.mean = Nd - 1; pb.cand = (long long)per_plan; pb.spread = HNu; pb.sigma = 1; pb.idx = 16;
  pb.out = (long long)(Nd - 1) * HNu; pb.temps = w->d_temps;
  float* mu_out = w->d_mu + (size_t)step * HNu;
  pb.mu = mu_stride;
  if (c.update_method == 3) {  // cem_update (path_integral.py:48-52)
    const int K = N < 10 ? N : 10;
    if (w->wt.has)
      MBD_TRY(launch_weigh_batch(w->wt, P, N, Nd, w->d_rews, c.temp_sample, w->d_temps, w->d_weights, w->d_rewmeans + step, s));
    else
      hipLaunchKernelGGL(score_kernel, dim3(1, (unsigned)P), dim3(kScoreThreads), sizeof(float) * (size_t)N, s, (const float*)w->d_rews,
                         (const float*)nullptr, N, e->rew_xref, c.temp_sample, 0, w->d_weights, w->d_rewmeans + step,
                         (float*)nullptr, pb);
    hipLaunchKernelGGL(cem_select_kernel, dim3(1, (unsigned)P), b64, sizeof(float) * (size_t)N, s, (const float*)w->d_weights, N, K,
                       w->d_idx, (float*)nullptr, pb);
    hipLaunchKernelGGL(cem_mean_kernel, dim3((HNu + 63) / 64, (unsigned)P), b64, 0, s, (const int*)w->d_idx, K,
                       (const float*)w->d_Y0s, HNu, mu_out, pb);
  } else {  // mppi (:33-36), cma-es (:39-45): softmax weights and the weighted mean in one launch
    ScoreBatch sb;
    sb.rews = N; sb.lp = N; sb.weights = N; sb.mean = Nd - 1; sb.cand = (long long)per_plan;
    sb.ybar_in = mu_stride; sb.ybar_out = (long long)(Nd - 1) * HNu; sb.keep = 0; sb.temps = w->d_temps;
    if (w->wt.has)
      MBD_TRY(launch_weigh_batch(w->wt, P, N, Nd, w->d_rews, c.temp_sample, w->d_temps, w->d_weights, w->d_rewmeans + step, s));
    if (recs && w->togo.has) {  // the to-go record's two launches in the fused launch's place (an mppi plan's TogoUpdate per plan)
      TogoUpdate A{};
      A.rews = w->d_rews; A.weights = w->d_weights; A.rew_mean = w->d_rewmeans + step; A.cand = w->d_Y0s; A.ybar_i = mu_in;
      A.ybar_im1 = mu_out; A.N = N; A.H = c.Hsample; A.Nu = w->Nu; A.temp = c.temp_sample; A.std_guard = 0;
      A.alpha_i = 1.0f; A.alpha_bar_i = 1.0f; A.alpha_bar_im1 = 1.0f; A.literal = 0; A.lazy = 0; A.sigma = 0.0f;
      MBD_TRY(togo_launch(w->togo, P, w->d_rewss, A, sb, s));
    } else {
      launch_score_wmean_batch(wmean_batch_v(N), w->wt.has, HNu, P, sizeof(float) * (size_t)N, s, w->d_rews.get(), (const float*)nullptr, N, e->rew_xref,
                               c.temp_sample, 0, w->d_weights.get(), w->d_rewmeans + step, (const float*)w->d_Y0s, HNu, mu_in, 1.0f, 1.0f,
                               1.0f, 0, mu_out, 0, 0.0f, (float*)nullptr, sb);
    }
    if (c.update_method == 2) {
      hipLaunchKernelGGL(cma_spread_kernel, dim3((HNu + 63) / 64, (unsigned)P), b64, 0, s, (const float*)w->d_weights,
                         (const float*)w->d_Y0s, N, HNu, mu_in, w->d_spread, pb);
      hipLaunchKernelGGL(cma_sigma_kernel, dim3(1, (unsigned)P), b64, 0, s, (const float*)w->d_spread, HNu, w->d_sigma, pb);
    }
  }
  HIP_TRY(hipGetLastError());
  // the elite record: the selection behind the update, over the rewards the score read and the materialised candidates
  if (recs) MBD_TRY(elite_select(w->elite, P, w->d_rews, N, w->d_Y0s, (long long)per_plan, HNu, 0, 0.0f, mu_in, mu_stride, mask, s));
  return MBD_OK;
}

struct PiStep {
  int slot;              // slot of every plan's d_mu / d_rewmeans the step writes
  const float* state0;   // [P][S] start states of the rollouts
  const float* mu_in;    // the mean of plan 0 the step samples around; plan k's is mu_stride floats further
  long long mu_stride;
  NoiseSpec ns;          // the noise shape and basis the step samples under
};
int sweep_pi_step(mbd_sweep* w, const PiStep& st, const SweepKeys& sk) {
  mbd_env* e = w->env;
  const mbd_plan_config& c = w->cfg;
  const int P = w->P, N = c.Nsample, H = c.Hsample, HNu = w->HNu, S = e->state_size();
  hipStream_t s = w->stream;
  const uint64_t per_plan = (uint64_t)N * HNu;
  const unsigned nblocks = noise_blocks(c.prng_impl, per_plan, 4096);
  const int step = st.slot;
  const float* mu_in = st.mu_in;
  const long long mu_stride = st.mu_stride;
  const NoiseSpec& ns = st.ns;
  if (ns.W) {  // under a noise basis: the knot kernel into the scratch z, then sample_batch_kernel's two roundings
    hipLaunchKernelGGL(knot_noise_batch_kernel, dim3(knot_blocks(N, w->Nu, 1024), (unsigned)P), dim3(kKnotThreads), 0, s, sk,
                       c.prng_impl, N, H, w->Nu, ns.knots, ns.W, ns.g, w->noise.d_knot_z.get());
    hipLaunchKernelGGL(shift_batch_kernel, dim3(noise_blocks(MBD_PRNG_PARTITIONABLE, per_plan, 4096), (unsigned)P), dim3(256), 0, s,
                       (const float*)w->noise.d_knot_z, N, HNu, (const float*)w->d_sigma, mu_in, mu_stride, w->d_Y0s.get());
  } else {
    hipLaunchKernelGGL(sample_batch_kernel, dim3(nblocks, (unsigned)P), dim3(256), 0, s, sk, c.prng_impl, N, HNu,
                       (const float*)w->d_sigma, mu_in, mu_stride, w->d_Y0s, ns.g);
  }
  HIP_TRY(hipGetLastError());
  // the elite record: ONE launch between the sampler and the rollout rewrites every plan's first rows
  MBD_TRY(elite_inject(w->elite, P, w->d_Y0s, (long long)per_plan, HNu, 0, 0.0f, mu_in, mu_stride, ns.g, 0xffffffffu, s));
  MBD_TRY(w->timing.begin(s));
  const int sw[3] = {N, S, 0};
  MBD_TRY(launch_rollout(e, st.state0, w->d_Y0s, P * N, H, w->d_rewss, w->d_rews, w->zone.xpos(), w->val.final(), s, nullptr, sw));
  MBD_TRY(w->timing.end(s));
  // the objective record: one launch over the P N rows (blockIdx.y = plan) on the materialised candidates
  if (w->obj.has) MBD_TRY(w->obj.launch(w->d_rewss, w->d_rews, N, 0, w->d_Y0s, false, 0.0f, nullptr, 0, s));
  // the zone record: one launch over the P N rows behind it (one table: the plans' rows are one batch)
  MBD_TRY(w->zone.launch_step(w->d_rews, P * N, s));
  // the value record: one launch over the P N rows behind it (one net: the plans' rows are one batch)
  MBD_TRY(w->val.launch_step(w->d_rews, P * N, s));
  return sweep_pi_update(w, step, mu_in, mu_stride, true);
}
}  // namespace

static int sweep_run_path_integral(mbd_sweep* w, const uint32_t* keys, float* mu_0ts_out, float* rew_means_out,
                                   float* rew_final_out, double* loop_seconds_out) {
  const mbd_plan_config& c = w->cfg;
  const int P = w->P, Nd = c.Ndiffuse, HNu = w->HNu;
  hipStream_t s = w->stream;
  std::vector<uint32_t> rng(keys, keys + 2 * (size_t)P);
  {
    std::vector<float> ones((size_t)P, 1.0f);  // sigma = 1.0 (path_integral.py:131)
    HIP_TRY(hipMemcpy(w->d_sigma, ones.data(), sizeof(float) * P, hipMemcpyHostToDevice));
  }
  MBD_TRY(elite_table_all(w->elite, P, HNu, -1, s));  // (an elite record: no plan has elites, and the logs begin)
  w->elite.restart();
  HIP_TRY(hipStreamSynchronize(s));
  auto t0 = std::chrono::steady_clock::now();
  w->wt.begin();
  for (int i = Nd - 1, step = 0; i >= 1; --i, ++step) {
    SweepKeys sk;
    for (int k = 0; k < P; ++k) {  // rng, Y0s_rng = split(rng) (path_integral.py:114)
      uint32_t ks[4];
      host_split(&rng[2 * k], 2, c.prng_impl, ks);
      rng[2 * k] = ks[0]; rng[2 * k + 1] = ks[1];
      sk.k[k][0] = ks[2]; sk.k[k][1] = ks[3];
    }
    PiStep st;
    st.slot = step; st.state0 = w->d_state0;
    st.mu_in = step == 0 ? w->d_zero.get() : w->d_mu + (size_t)(step - 1) * HNu;
    st.mu_stride = step == 0 ? HNu : (long long)(Nd - 1) * HNu;
    st.ns = w->noise.spec(false);
    MBD_TRY(sweep_pi_step(w, st, sk));
  }
  HIP_TRY(hipStreamSynchronize(s));
  auto t1 = std::chrono::steady_clock::now();
  if (loop_seconds_out) *loop_seconds_out = std::chrono::duration<double>(t1 - t0).count();
  return sweep_results(w, mu_0ts_out, rew_means_out, rew_final_out);
}

extern "C" int mbd_sweep_get_sigmas(mbd_sweep* w, float* sigmas_out) {
  if (!w || !sigmas_out) return fail(MBD_ERR_INVALID, "NULL argument");
  if (!w->d_sigma) return fail(MBD_ERR_STATE, "not a path-integral sweep (update_method == 0)");
  HIP_TRY(hipSetDevice(w->env->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(w->d_sigma.download(sigmas_out, w->P));
  return MBD_OK;
}

// ---- the lockstep diffusion step of MBD sweeps (update_method 0), shared by mbd_sweep_run and mbd_sweep_run_mpc ----------
namespace {
struct SweepStep {
  int q;                       // position of the step in its loop: the ring buffer q % 3, the progress word q + 1
  int i;                       // diffusion step Nd-1 .. 1
  int slot;                    // slot of every plan's d_mu / d_rewmeans the step writes
  const float* state0;         // [P][S] start states of the rollouts
  const float* ybar_in;        // Ybar_i of plan 0; plan k's is ybar_in_stride floats further
  long long ybar_in_stride;
  const SweepKeys* next_keys;  // Y0s_rng of the loop's following step (its normals go beside this rollout), or nullptr: none follows
  NoiseSpec next_ns;           // the noise shape and basis that following step samples under
  const float* xref = nullptr; // the demo table of the step: a tick's window of a batch with a demo record, nullptr: the env's ...
  float rew_xref = 0.0f;       // ... and the demo's reward level in the blend: the record's, or the env's
  const float* g = nullptr;    // the noise shape THIS step's sampler was handed (an elite record's injection keeps frozen elements)
  unsigned mask = 0xffffffffu; // the plans an elite record's launches take part for (a session's mixed tick: not the idling ones)
};

// the normals of a step depend on its keys only: they are generated on the second stream while the previous step's
// rollout runs (a ring of three buffers, see mbd_sweep), like a single large plan's
// (under a noise basis: knot_noise_batch_kernel, into the same buffers)
void sweep_noise(mbd_sweep* w, const SweepKeys& sk, int buf, hipStream_t st, const NoiseSpec& ns) {
  const mbd_plan_config& c = w->cfg;
  if (ns.W) {
    hipLaunchKernelGGL(knot_noise_batch_kernel, dim3(knot_blocks(c.Nsample, w->Nu, 1024), (unsigned)w->P), dim3(kKnotThreads), 0, st,
                       sk, c.prng_impl, c.Nsample, c.Hsample, w->Nu, ns.knots, ns.W, ns.g, w->d_eps[buf].get());
    return;
  }
  const unsigned nblocks = noise_blocks(c.prng_impl, (uint64_t)c.Nsample * w->HNu, 4096);
  hipLaunchKernelGGL(noise_batch_kernel, dim3(nblocks, (unsigned)w->P), dim3(256), 0, st, sk, c.prng_impl, c.Nsample, w->HNu,
                     w->d_eps[buf], ns.g);
}

// rng, Y0s_rng = split(rng) of every plan (mbd_planner.py:103) — the whole key chain is host arithmetic
void sweep_split_keys(const mbd_sweep* w, std::vector<uint32_t>& rng, SweepKeys& out) {
  for (int k = 0; k < w->P; ++k) {
    uint32_t ks[4];
    host_split(&rng[2 * k], 2, w->cfg.prng_impl, ks);
    rng[2 * k] = ks[0]; rng[2 * k + 1] = ks[1];
    out.k[k][0] = ks[2]; out.k[k][1] = ks[3];
  }
}

// what a lockstep step launches behind the value record's launch — the weigh kernel under a weighting record, then the score +
// weighted mean over the P plans —: the step's, and mbd_debug_sweep_update's on uploaded rewards.  i: diffusion step; slot: of
// every plan's d_mu / d_rewmeans; eps: the step's normals [P][N][HNu]; ybar_in: Ybar_i of plan 0, plan k's ybar_in_stride further
// recs: the step's (an elite and a to-go record's launches run; mask: the plans that take part in the selection), not the debug entry's
int sweep_update(mbd_sweep* w, int i, int slot, const float* eps, const float* ybar_in, long long ybar_in_stride, float rew_xref,
                 bool recs = false, unsigned mask = 0xffffffffu) {
  const mbd_plan_config& c = w->cfg;
  const int P = w->P, N = c.Nsample, Nd = c.Ndiffuse, HNu = w->HNu;
  hipStream_t s = w->stream;
  ScoreBatch sb;
  sb.rews = N; sb.lp = N; sb.weights = N; sb.mean = Nd - 1; sb.cand = (long long)N * HNu;
  sb.ybar_in = ybar_in_stride; sb.ybar_out = (long long)(Nd - 1) * HNu; sb.keep = 0; sb.temps = w->d_temps;
  if (w->wt.has)
    MBD_TRY(launch_weigh_batch(w->wt, P, N, Nd, w->d_rews, c.temp_sample, w->d_temps, w->d_weights, w->d_rewmeans + slot, s));
  if (recs && w->togo.has) {  // the to-go record's two launches in the fused launch's place (a plan's TogoUpdate per plan)
    TogoUpdate A{};
    A.rews = w->d_rews; A.weights = w->d_weights; A.rew_mean = w->d_rewmeans + slot; A.cand = eps; A.ybar_i = ybar_in;
    A.ybar_im1 = w->d_mu + (size_t)slot * HNu; A.N = N; A.H = c.Hsample; A.Nu = w->Nu; A.temp = c.temp_sample; A.std_guard = 1;
    A.alpha_i = w->alphas[i]; A.alpha_bar_i = w->alphas_bar[i]; A.alpha_bar_im1 = w->alphas_bar[i - 1]; A.literal = c.literal_score;
    A.lazy = 1; A.sigma = w->sigmas[i];
    MBD_TRY(togo_launch(w->togo, P, w->d_rewss, A, sb, s));
  } else {
    launch_score_wmean_batch(wmean_batch_v(N), w->wt.has, HNu, P, sizeof(float) * (size_t)N, s, w->d_rews.get(), c.enable_demo ? w->d_lp.get() : nullptr, N,
                             rew_xref, c.temp_sample, 1, w->d_weights.get(), w->d_rewmeans + slot, eps, HNu, ybar_in,
                             w->alphas[i], w->alphas_bar[i], w->alphas_bar[i - 1], c.literal_score,
                             w->d_mu + (size_t)slot * HNu, 1, w->sigmas[i], (float*)nullptr, sb);
  }
  HIP_TRY(hipGetLastError());
  // the elite record: the selection behind the update, over the rewards the score read and the step's normals — on the steps' stream,
  // so it is now eps[cur]'s last reader (see mbd_sweep)
  if (recs) MBD_TRY(elite_select(w->elite, P, w->d_rews, N, eps, (long long)N * HNu, HNu, 1, w->sigmas[i], ybar_in, ybar_in_stride, mask, s));
  return MBD_OK;
}

int sweep_step(mbd_sweep* w, const SweepStep& st) {
  mbd_env* e = w->env;
  const mbd_plan_config& c = w->cfg;
  const int P = w->P, N = c.Nsample, H = c.Hsample, S = e->state_size();
  const int step = st.q, i = st.i;
  hipStream_t s = w->stream;
  const int cur = step % 3, nxt = (step + 1) % 3;
  if (step > 0 && hipEventQuery(w->ev_ready[cur]) != hipSuccess) {  // (generated a whole step ago: ready in practice)
    (void)hipGetLastError();
    HIP_TRY(hipStreamWaitEvent(s, w->ev_ready[cur], 0));
  }
  if (st.next_keys) {  // the next step's normals beside this rollout
    // eps[nxt] was last read by the weighted mean of step - 2, finished once the rollout of step - 1 (which stores
    // `step` into the progress word) has started: the loop waits for that — one step behind the device, whose queue
    // still holds that rollout and its score — instead of ordering the two streams with events
    if (step >= 2 && !progress_wait(w->h_progress, step, kInStepWaitMs, 20)) {
      // a legitimately slow stream (shared / time-sliced GPU, profiler, system pause): order the streams with an
      // event instead — everything enqueued on s so far, the reader of eps[nxt] included, precedes the generation
      if (!w->ev_order) HIP_TRY(w->ev_order.create());
      HIP_TRY(hipEventRecord(w->ev_order, s));
      HIP_TRY(hipStreamWaitEvent(w->aux, w->ev_order, 0));
    }
    sweep_noise(w, *st.next_keys, nxt, w->aux, st.next_ns);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(w->ev_ready[nxt], w->aux));
  }
  // the elite record: ONE launch on the steps' stream, behind the wait for eps[cur] and in front of the rollout, rewrites every
  // plan's first rows of normals
  MBD_TRY(elite_inject(w->elite, P, w->d_eps[cur], (long long)N * w->HNu, w->HNu, 1, w->sigmas[i], st.ybar_in, st.ybar_in_stride, st.g, st.mask, s));
  LazyArgs lz;
  lz.ybar = st.ybar_in;
  lz.sigma = w->sigmas[i];
  lz.progress = w->h_progress;
  lz.progress_val = step + 1;
  const int sw[3] = {N, S, (int)st.ybar_in_stride};
  MBD_TRY(w->timing.begin(s));
  const bool fused_lp = c.enable_demo && rollout_choice(e, P * N, H, sw).fuses_logpd;  // (mbd_plan.hip: the log-densities out of the rollout)
  MBD_TRY(launch_rollout(e, st.state0, w->d_eps[cur], P * N, H, w->d_rewss, w->d_rews,
                         (c.enable_demo && !fused_lp) ? w->d_xpos.get() : w->zone.xpos(), w->val.final(), s, &lz, sw,
                         fused_lp ? w->d_lp.get() : nullptr, nullptr, st.xref));
  MBD_TRY(w->timing.end(s));
  if (c.enable_demo && !fused_lp) MBD_TRY(launch_logpd(e, w->d_xpos, P * N, H, w->d_lp, s, st.xref));
  // the objective record: one launch over the P N rows (blockIdx.y = plan) between the rollout and the score.  The ring needs no
  // change: the launch reads eps[cur] on the steps' stream in front of the weighted mean, which is the buffer's last reader.
  if (w->obj.has)
    MBD_TRY(w->obj.launch(w->d_rewss, w->d_rews, N, 0, w->d_eps[cur], true, w->sigmas[i], st.ybar_in, st.ybar_in_stride, s));
  // the zone record: one launch over the P N rows behind it (one table: the plans' rows are one batch)
  MBD_TRY(w->zone.launch_step(w->d_rews, P * N, s));
  // the value record: one launch over the P N rows behind it (one net: the plans' rows are one batch)
  MBD_TRY(w->val.launch_step(w->d_rews, P * N, s));
  return sweep_update(w, i, st.slot, w->d_eps[cur].get(), st.ybar_in, st.ybar_in_stride, st.rew_xref, true, st.mask);
}
}  // namespace

extern "C" int mbd_sweep_run(mbd_sweep* w, const uint32_t* keys, float* mu_0ts_out, float* rew_means_out,
                             float* rew_final_out, double* loop_seconds_out) {
  if (!w || !keys) return fail(MBD_ERR_INVALID, "NULL argument");
  NO_SWEEP_SESSION(w, "run");
  mbd_env* e = w->env;
  HIP_TRY(hipSetDevice(e->device));
  const mbd_plan_config& c = w->cfg;
  const int P = w->P, Nd = c.Ndiffuse, HNu = w->HNu;
  hipStream_t s = w->stream;
  if (c.update_method != 0) return sweep_run_path_integral(w, keys, mu_0ts_out, rew_means_out, rew_final_out, loop_seconds_out);
  std::vector<uint32_t> rng(keys, keys + 2 * (size_t)P);
  MBD_TRY(elite_table_all(w->elite, P, HNu, -1, s));  // (an elite record: no plan has elites, and the logs begin)
  w->elite.restart();
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipStreamSynchronize(w->aux));
  progress_reset(w->h_progress);
  auto t0 = std::chrono::steady_clock::now();
  SweepKeys sk;
  sweep_split_keys(w, rng, sk);
  sweep_noise(w, sk, 0, s, w->noise.spec(false));  // step Nd-1
  HIP_TRY(hipGetLastError());
  w->wt.begin();
  for (int i = Nd - 1, step = 0; i >= 1; --i, ++step) {
    if (i > 1) sweep_split_keys(w, rng, sk);
    SweepStep st;
    st.q = step; st.i = i; st.slot = step; st.state0 = w->d_state0;
    st.ybar_in = step == 0 ? w->d_zero : w->d_mu + (size_t)(step - 1) * HNu;
    st.ybar_in_stride = step == 0 ? HNu : (long long)(Nd - 1) * HNu;
    st.next_keys = i > 1 ? &sk : nullptr;
    st.next_ns = w->noise.spec(false);
    st.rew_xref = e->rew_xref;
    st.g = w->noise.shape_always();
    MBD_TRY(sweep_step(w, st));
  }
  HIP_TRY(hipStreamSynchronize(s));
  auto t1 = std::chrono::steady_clock::now();
  if (loop_seconds_out) *loop_seconds_out = std::chrono::duration<double>(t1 - t0).count();
  return sweep_results(w, mu_0ts_out, rew_means_out, rew_final_out);
}

// The update step of a sweep alone on uploaded arrays (include/mbd_hip_debug.h): sweep_update / sweep_pi_update — what a lockstep
// step launches behind its value record's launch — with slot 0 of every plan, ring buffer 0 (MBD) or d_Y0s as the candidates and
// d_final as the [P][HNu] buffer of the means.  No rollout, objective or value launch; d_zero is not written, and a run after it
// generates its own normals, resets sigma and rewrites every slot, so it equals a fresh sweep's.
extern "C" int mbd_debug_sweep_update(mbd_sweep* w, int i, const float* cand, const float* ybar, const float* rews, const float* lp,
                                      const float* sigma_in, float* ybar_out, float* weights_out, float* rew_mean_out,
                                      float* sigma_out, int32_t* idx_out) {
  if (!w) return fail(MBD_ERR_INVALID, "debug_sweep_update: sweep is NULL");
  if (!cand) return fail(MBD_ERR_INVALID, "debug_sweep_update: cand is NULL");
  if (!ybar) return fail(MBD_ERR_INVALID, "debug_sweep_update: ybar is NULL");
  if (!rews) return fail(MBD_ERR_INVALID, "debug_sweep_update: rews is NULL");
  const mbd_plan_config& c = w->cfg;
  if (c.enable_demo && !lp) return fail(MBD_ERR_INVALID, "debug_sweep_update: lp is NULL on a sweep with enable_demo");
  if (!c.enable_demo && lp) return fail(MBD_ERR_INVALID, "debug_sweep_update: lp given on a sweep without enable_demo");
  if (c.update_method == 2 && !sigma_in) return fail(MBD_ERR_INVALID, "debug_sweep_update: sigma_in is NULL on a cma-es sweep");
  if (c.update_method != 2 && sigma_in) return fail(MBD_ERR_INVALID, "debug_sweep_update: sigma_in given on a sweep that is not cma-es");
  if (i < 1 || i > c.Ndiffuse - 1) return fail(MBD_ERR_INVALID, "debug_sweep_update: i=%d outside [1,%d]", i, c.Ndiffuse - 1);
  NO_SWEEP_SESSION(w, "debug_sweep_update");
  mbd_env* e = w->env;
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());
  const int P = w->P, N = c.Nsample, Nd = c.Ndiffuse, HNu = w->HNu, K = N < 10 ? N : 10;
  const bool pi = c.update_method != 0;
  const size_t PN = (size_t)P * N, mu_pitch = sizeof(float) * (size_t)(Nd - 1) * HNu, row = sizeof(float) * HNu;
  float* d_cand = pi ? w->d_Y0s.get() : w->d_eps[0].get();
  HIP_TRY(hipMemcpy(d_cand, cand, sizeof(float) * PN * HNu, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(w->d_final, ybar, row * P, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(w->d_rews, rews, sizeof(float) * PN, hipMemcpyHostToDevice));
  if (lp) HIP_TRY(hipMemcpy(w->d_lp, lp, sizeof(float) * PN, hipMemcpyHostToDevice));
  if (sigma_in) HIP_TRY(hipMemcpy(w->d_sigma, sigma_in, sizeof(float) * P, hipMemcpyHostToDevice));
  {  // a quiet NaN over what is read back: an output no kernel wrote is seen
    const size_t PE = (size_t)P * HNu;
    const std::vector<float> nan(PN > PE ? PN : PE, __builtin_nanf(""));
    HIP_TRY(hipMemcpy(w->d_weights, nan.data(), sizeof(float) * PN, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy2D(w->d_mu, mu_pitch, nan.data(), row, row, P, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy2D(w->d_rewmeans, sizeof(float) * (Nd - 1), nan.data(), sizeof(float), sizeof(float), P, hipMemcpyHostToDevice));
    if (c.update_method == 3) HIP_TRY(hipMemset(w->d_idx, 0xff, sizeof(int) * (size_t)P * 16));
  }
  w->wt.begin();  // (the step's entry of a weighting record's log is entry 0: mbd_sweep_peek_weighting)
  if (pi) MBD_TRY(sweep_pi_update(w, 0, w->d_final, HNu));
  else MBD_TRY(sweep_update(w, i, 0, d_cand, w->d_final, HNu, e->rew_xref));
  HIP_TRY(hipStreamSynchronize(w->stream));
  if (ybar_out) HIP_TRY(hipMemcpy2D(ybar_out, row, w->d_mu, mu_pitch, row, P, hipMemcpyDeviceToHost));
  HIP_TRY(w->d_weights.download(weights_out, PN));
  if (rew_mean_out)
    HIP_TRY(hipMemcpy2D(rew_mean_out, sizeof(float), w->d_rewmeans, sizeof(float) * (Nd - 1), sizeof(float), P, hipMemcpyDeviceToHost));
  if (c.update_method == 2) HIP_TRY(w->d_sigma.download(sigma_out, P));
  if (idx_out && c.update_method == 3)
    HIP_TRY(hipMemcpy2D(idx_out, sizeof(int) * K, w->d_idx, sizeof(int) * 16, sizeof(int) * K, P, hipMemcpyDeviceToHost));
  return MBD_OK;
}

// one noise shape for all plans of the sweep (include/mbd_hip.h mbd_noise_shape).  A sweep prepares nothing across run calls:
// every run generates its first normals itself, so there is nothing to discard beyond waiting for the device.
extern "C" int mbd_sweep_set_noise_shape(mbd_sweep* w, const mbd_noise_shape* rec) {
  if (!w) return fail(MBD_ERR_INVALID, "sweep is NULL");
  NO_SWEEP_SESSION(w, "set_noise_shape");
  if (rec) MBD_TRY(check_noise_shape(rec, w->cfg.Hsample, w->Nu));
  return w->noise.set_shape(rec, w->HNu, w->env->device);
}

// one noise basis for all plans of the sweep (include/mbd_hip.h mbd_noise_basis), as mbd_sweep_set_noise_shape
extern "C" int mbd_sweep_set_noise_basis(mbd_sweep* w, const mbd_noise_basis* rec) {
  if (!w) return fail(MBD_ERR_INVALID, "sweep is NULL");
  NO_SWEEP_SESSION(w, "set_noise_basis");
  if (rec) MBD_TRY(check_noise_basis(rec, w->cfg.Hsample));
  // (path-integral sweeps alone run knot_noise_batch_kernel into the scratch z)
  return w->noise.set_basis(rec, w->cfg.Hsample, w->cfg.update_method != 0 ? (size_t)w->P * w->cfg.Nsample * w->HNu : 0, w->env->device);
}

// one objective record for all plans of the sweep (include/mbd_hip.h mbd_objective), as mbd_plan_set_objective
extern "C" int mbd_sweep_set_objective(mbd_sweep* w, const mbd_objective* rec) {
  if (!w) return fail(MBD_ERR_INVALID, "sweep is NULL");
  NO_SWEEP_SESSION(w, "set_objective");
  float wsum = 0.0f;
  if (rec) MBD_TRY(check_objective(rec, w->cfg.Hsample, w->Nu, &wsum));  // (before any device access)
  if (rec && w->togo.has) return refuse_beside_togo("objective record", "sweep");
  return w->obj.set(rec, wsum, w->env->device, w->P, w->cfg.Nsample, w->cfg.Hsample, w->Nu, (size_t)w->cfg.Nsample);
}

extern "C" int mbd_sweep_peek_objective(mbd_sweep* w, int k, float* ret_out, float* cost_out) {
  if (!w) return fail(MBD_ERR_INVALID, "sweep is NULL");
  return w->obj.peek(w->env, k, ret_out, cost_out, "sweep");
}

// one value record for all plans of the sweep (include/mbd_hip.h mbd_value), as mbd_plan_set_value
extern "C" int mbd_sweep_set_value(mbd_sweep* w, const mbd_value* rec) {
  if (!w) return fail(MBD_ERR_INVALID, "sweep is NULL");
  NO_SWEEP_SESSION(w, "set_value");
  if (rec) MBD_TRY(check_value(rec, w->env->state_size(), w->env->kind == ENV_MODEL));  // (before any device access)
  if (rec && w->togo.has) return refuse_beside_togo("value record", "sweep");
  return w->val.set(rec, w->env, (size_t)w->P * w->cfg.Nsample, w->P);
}

// one zone record for all plans of the sweep (include/mbd_hip.h mbd_zones), as mbd_plan_set_zones
extern "C" int mbd_sweep_set_zones(mbd_sweep* w, const mbd_zones* rec) {
  if (!w) return fail(MBD_ERR_INVALID, "sweep is NULL");
  if (rec) {  // (before any device access)
    const int n_track = w->env ? w->env->model.n_track : 0;
    MBD_TRY(check_zones(rec, n_track > 0 ? n_track : 32));
    MBD_TRY(check_zones_handle(w->env, w->cfg, "sweep"));
    if (w->togo.has) return refuse_beside_togo("zone record", "sweep");
    if (w->pick.has) return fail(MBD_ERR_UNSUPPORTED, "zone record: the sweep carries a pick record (its slots' rollouts write no positions)");
  }
  NO_SWEEP_SESSION(w, "set_zones");
  return w->zone.set(rec, w->env, (size_t)w->P * w->cfg.Nsample, w->cfg.Hsample);
}

extern "C" int mbd_sweep_update_zones(mbd_sweep* w, const mbd_zones* rec) {
  if (!w) return fail(MBD_ERR_INVALID, "sweep is NULL");
  if (w->session.in_flight) return fail(MBD_ERR_STATE, "update_zones: a tick is in flight (mbd_sweep_mpc_collect first)");
  return w->zone.update(rec, w->env, "sweep");
}

extern "C" int mbd_sweep_peek_zones(mbd_sweep* w, int k, float* pen_out, float* clear_out) {
  if (!w) return fail(MBD_ERR_INVALID, "sweep is NULL");
  if (k < 0 || k >= w->P) return fail(MBD_ERR_INVALID, "peek_zones: plan k=%d outside [0,%d)", k, w->P);
  return w->zone.peek(w->env, k, w->cfg.Nsample, pen_out, clear_out, "sweep");
}

extern "C" int mbd_sweep_peek_mpc_zones(mbd_sweep* w, int k, float* pen_out, float* clear_out) {
  if (!w) return fail(MBD_ERR_INVALID, "sweep is NULL");
  if (k < 0 || k >= w->P) return fail(MBD_ERR_INVALID, "peek_mpc_zones: episode k=%d outside [0,%d)", k, w->P);
  return w->zone.peek_mpc(w->env, k, pen_out, clear_out, "sweep");
}

// one weighting record for all plans of the sweep (include/mbd_hip.h mbd_weighting), as mbd_plan_set_weighting
extern "C" int mbd_sweep_set_weighting(mbd_sweep* w, const mbd_weighting* rec) {
  if (!w) return fail(MBD_ERR_INVALID, "sweep is NULL");
  NO_SWEEP_SESSION(w, "set_weighting");
  if (rec) MBD_TRY(check_weighting(rec));  // (before any device access)
  if (rec && w->cfg.enable_demo)
    return fail(MBD_ERR_UNSUPPORTED, "weighting record: enable_demo=1: the demo blend standardises twice, an ESS target is not defined there");
  if (rec && w->togo.has) return refuse_beside_togo("weighting record", "sweep");
  return w->wt.set(rec, w->env->device, w->P, w->cfg.Ndiffuse - 1, w->cfg.Nsample);
}

extern "C" int mbd_sweep_peek_weighting(mbd_sweep* w, int k, float* temp_out, float* ess_out, int32_t* kept_out, int capacity,
                                        int* count_out) {
  if (!w) return fail(MBD_ERR_INVALID, "sweep is NULL");
  return w->wt.peek(w->env, k, temp_out, ess_out, kept_out, capacity, count_out, "sweep");
}

// one elite record for all plans of the sweep (include/mbd_hip.h mbd_elites), as mbd_plan_set_elites: the field checks are the
// plan's, on the sweep's config; no plan has elites afterwards
extern "C" int mbd_sweep_set_elites(mbd_sweep* w, const mbd_elites* rec) {
  if (!w) return fail(MBD_ERR_INVALID, "sweep is NULL");
  if (rec) MBD_TRY(check_elites(rec, w->cfg.Nsample, w->cfg.update_method, w->cfg.enable_demo));  // (before any device access)
  NO_SWEEP_SESSION(w, "set_elites");
  if (!rec && !w->elite.has) return MBD_OK;  // (nothing to clear: no device is touched)
  MBD_TRY(w->elite.set(rec, w->P, w->HNu, w->env->device));
  MBD_TRY(elite_table_all(w->elite, w->P, w->HNu, -1, w->stream));  // (no plan has elites afterwards: one launch, waited for)
  if (w->elite.has) HIP_TRY(hipStreamSynchronize(w->stream));
  return MBD_OK;
}

extern "C" int mbd_sweep_peek_elites(mbd_sweep* w, int k, float* elites_out, float* returns_out, int32_t* src_out, int32_t* count_out,
                                     int32_t* log_count, int32_t* log_kept, float* log_top, int capacity, int* n_log_out) {
  if (!w) return fail(MBD_ERR_INVALID, "sweep is NULL");
  if (k < 0 || k >= w->P) return fail(MBD_ERR_INVALID, "peek_elites: plan k=%d outside [0,%d)", k, w->P);
  return w->elite.peek(w->env, k, w->HNu, elites_out, returns_out, src_out, count_out, log_count, log_kept, log_top, capacity, n_log_out,
                       "sweep");
}

// one to-go record for all plans of the sweep (include/mbd_hip.h mbd_togo), as mbd_plan_set_togo
extern "C" int mbd_sweep_set_togo(mbd_sweep* w, const mbd_togo* rec) {
  if (!w) return fail(MBD_ERR_INVALID, "sweep is NULL");
  if (rec) {  // (before any device access)
    MBD_TRY(check_togo(rec, w->cfg.Hsample, w->cfg.Nsample, w->cfg.update_method, w->cfg.enable_demo));
    const char* other = w->obj.has ? "an objective" : w->val.has ? "a value" : w->wt.has ? "a weighting" : nullptr;
    if (other)
      return fail(MBD_ERR_UNSUPPORTED, "to-go record: the sweep carries %s record: what that record means per horizon row is not defined",
                  other);
    if (w->zone.has) return refuse_beside_zones("to-go record", "sweep");
  }
  NO_SWEEP_SESSION(w, "set_togo");
  if (!rec && !w->togo.has) return MBD_OK;  // (nothing to clear: no device is touched)
  return w->togo.set(rec, w->P, w->cfg.Hsample, w->cfg.Nsample, w->env->device);
}

extern "C" int mbd_sweep_peek_togo(mbd_sweep* w, int k, int32_t* starts_out, float* R_out, float* W_out, int32_t* n_groups_out) {
  if (!w) return fail(MBD_ERR_INVALID, "sweep is NULL");
  if (k < 0 || k >= w->P) return fail(MBD_ERR_INVALID, "peek_togo: plan k=%d outside [0,%d)", k, w->P);
  return w->togo.peek(w->env, k, w->cfg.Nsample, w->d_weights, starts_out, R_out, W_out, n_groups_out, "sweep");
}

// include/mbd_hip_debug.h: an elite record's two batch launches alone on caller-given arrays for P plans — the injection, then the
// selection — by a scratch record's own members; no sweep.  What is read back is filled with all-ones bits first.
extern "C" int mbd_debug_sweep_elites_step(int P, uint32_t mask, const float* rews, const float* cand, int N, int HNu, const float* ybar,
                                           float sigma, int lazy, const float* g, int n_elites, int nominal, const float* E_in,
                                           const int32_t* count_in, float* cand_out, float* E_out, float* R_out, int32_t* src_out,
                                           int32_t* count_out, int32_t* kept_out, float* top_out) {
  if (!rews || !cand || !ybar || !count_in) return fail(MBD_ERR_INVALID, "sweep_elites_step: NULL argument");
  if (P < 1 || P > MBD_SWEEP_MAX_PLANS) return fail(MBD_ERR_INVALID, "sweep_elites_step: P=%d outside [1,%d]", P, MBD_SWEEP_MAX_PLANS);
  if (N < 1 || HNu < 1 || (uint64_t)P * (uint64_t)N * (uint64_t)HNu > (1ull << 27))
    return fail(MBD_ERR_INVALID, "sweep_elites_step: P=%d N=%d HNu=%d", P, N, HNu);
  if (n_elites < 0 || n_elites > kEliteMax) return fail(MBD_ERR_INVALID, "sweep_elites_step: n_elites=%d outside [0, %d]", n_elites, kEliteMax);
  if (nominal != 0 && nominal != 1) return fail(MBD_ERR_INVALID, "sweep_elites_step: nominal=%d: 0 or 1", nominal);
  if (n_elites + nominal >= N) return fail(MBD_ERR_INVALID, "sweep_elites_step: n_elites=%d + nominal=%d must lie below N=%d", n_elites, nominal, N);
  for (int k = 0; k < P; ++k) {
    if (count_in[k] < 0 || count_in[k] > n_elites)
      return fail(MBD_ERR_INVALID, "sweep_elites_step: count[%d]=%d outside [0, n_elites=%d]", k, count_in[k], n_elites);
    if (count_in[k] > 0 && !E_in) return fail(MBD_ERR_INVALID, "sweep_elites_step: count[%d]=%d without elites", k, count_in[k]);
  }
  if (lazy && !(sigma > 0.0f)) return fail(MBD_ERR_INVALID, "sweep_elites_step: sigma=%g: a lazy plan's sigma is > 0", (double)sigma);
  if (device_count_quiet() < 1) return fail(MBD_ERR_NO_DEVICE, "no HIP device: this library has no CPU fallback");
  const size_t PN = (size_t)P * N, per_plan = (size_t)N * HNu;
  DevBuf<float> d_rews, d_cand, d_ybar, d_g;
  EliteRec L;
  HIP_TRY(d_rews.upload(rews, PN));
  HIP_TRY(d_cand.upload(cand, PN * HNu));
  HIP_TRY(d_ybar.upload(ybar, (size_t)P * HNu));
  if (g) HIP_TRY(d_g.upload(g, HNu));
  MBD_TRY(L.scratch(n_elites, nominal, P, HNu, E_in, count_in));
  const size_t PR = (size_t)P * L.rows;
  MBD_TRY(elite_inject(L, P, d_cand, (long long)per_plan, HNu, lazy ? 1 : 0, sigma, d_ybar, HNu, d_g, mask, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(d_cand.download(cand_out, PN * HNu));
  MBD_TRY(elite_select(L, P, d_rews, N, d_cand, (long long)per_plan, HNu, lazy ? 1 : 0, sigma, d_ybar, HNu, mask, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(L.d_E.download(E_out, PR * HNu));
  HIP_TRY(L.d_R.download(R_out, PR));
  HIP_TRY(L.d_src.download(src_out, PR));
  HIP_TRY(L.d_count.download(count_out, P));
  HIP_TRY(L.d_log_kept.download(kept_out, P));
  HIP_TRY(L.d_log_top.download(top_out, P));
  std::vector<int32_t> cnt_word(P), cnt_log(P);  // (count' as the word holds it must agree with the log entry's copy)
  HIP_TRY(L.d_count.download(cnt_word.data(), P));
  HIP_TRY(L.d_log_count.download(cnt_log.data(), P));
  for (int k = 0; k < P; ++k)
    if (((mask >> k) & 1u) && cnt_word[k] != cnt_log[k])
      return fail(MBD_ERR_STATE, "sweep_elites_step: plan %d: count word %d, log entry %d", k, cnt_word[k], cnt_log[k]);
  return MBD_OK;
}

// include/mbd_hip_debug.h: a to-go record's two batch launches alone on caller-given arrays for P plans, by a scratch record's own
// launch; no sweep.  What is read back is filled with all-ones bits (quiet NaN) first.
extern "C" int mbd_debug_sweep_togo_step(int P, const float* temps, const float* cand, const float* ybar, const float* rews,
                                         const float* rewss, int N, int H, int Nu, int block, int min_tail, int lazy, float sigma,
                                         int std_guard, float alpha_i, float alpha_bar_i, float alpha_bar_im1, int literal,
                                         float* ybar_out, float* R_out, float* W_out, float* rew_mean_out) {
  if (!temps || !cand || !ybar || !rews || !rewss) return fail(MBD_ERR_INVALID, "sweep_togo_step: NULL argument");
  if (P < 1 || P > MBD_SWEEP_MAX_PLANS) return fail(MBD_ERR_INVALID, "sweep_togo_step: P=%d outside [1,%d]", P, MBD_SWEEP_MAX_PLANS);
  if (N < 1 || H < 1 || Nu < 1 || (uint64_t)P * (uint64_t)N * (uint64_t)H * (uint64_t)Nu > (1ull << 27))
    return fail(MBD_ERR_INVALID, "sweep_togo_step: P=%d N=%d H=%d Nu=%d", P, N, H, Nu);
  if (block < 1) return fail(MBD_ERR_INVALID, "sweep_togo_step: block=%d: at least 1", block);
  if (min_tail < 1 || min_tail > H) return fail(MBD_ERR_INVALID, "sweep_togo_step: min_tail=%d outside [1, H=%d]", min_tail, H);
  if (N > 12288) return fail(MBD_ERR_INVALID, "sweep_togo_step: N=%d above 12288", N);
  if (device_count_quiet() < 1) return fail(MBD_ERR_NO_DEVICE, "no HIP device: this library has no CPU fallback");
  const size_t HNu = (size_t)H * Nu, PN = (size_t)P * N;
  TogoRec L;
  L.layout(block, min_tail, H);
  const size_t gn = (size_t)P * L.G * N;
  DevBuf<float> d_temps, d_cand, d_ybar, d_rews, d_rewss, d_out, d_w, d_mean;
  HIP_TRY(d_temps.upload(temps, P));
  HIP_TRY(d_cand.upload(cand, PN * HNu));
  HIP_TRY(d_ybar.upload(ybar, (size_t)P * HNu));
  HIP_TRY(d_rews.upload(rews, PN));
  HIP_TRY(d_rewss.upload(rewss, PN * H));
  HIP_TRY(d_out.alloc_poisoned((size_t)P * HNu));
  HIP_TRY(d_w.alloc_poisoned(PN));
  HIP_TRY(d_mean.alloc_poisoned(P));
  HIP_TRY(L.d_R.alloc_poisoned(gn));
  HIP_TRY(L.d_W.alloc_poisoned(gn));
  TogoUpdate A{};
  A.rews = d_rews; A.weights = d_w; A.rew_mean = d_mean; A.cand = d_cand; A.ybar_i = d_ybar; A.ybar_im1 = d_out;
  A.N = N; A.H = H; A.Nu = Nu; A.temp = 0.0f; A.std_guard = std_guard ? 1 : 0; A.alpha_i = alpha_i; A.alpha_bar_i = alpha_bar_i;
  A.alpha_bar_im1 = alpha_bar_im1; A.literal = literal ? 1 : 0; A.lazy = lazy ? 1 : 0; A.sigma = sigma;
  ScoreBatch sb;
  sb.rews = N; sb.lp = N; sb.weights = N; sb.mean = 1; sb.cand = (long long)N * (long long)HNu; sb.ybar_in = (long long)HNu;
  sb.ybar_out = (long long)HNu; sb.keep = 0; sb.temps = d_temps;
  MBD_TRY(togo_launch(L, P, d_rewss, A, sb, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(d_out.download(ybar_out, (size_t)P * HNu));
  HIP_TRY(L.d_R.download(R_out, gn));
  HIP_TRY(L.d_W.download(W_out, gn));
  if (W_out)  // (group 0's weights: every plan's row 0)
    HIP_TRY(hipMemcpy2D(W_out, sizeof(float) * (size_t)L.G * N, d_w, sizeof(float) * N, sizeof(float) * N, P, hipMemcpyDeviceToHost));
  HIP_TRY(d_mean.download(rew_mean_out, P));
  return MBD_OK;
}

// one pick record for all episodes of the sweep (include/mbd_hip.h mbd_mpc_pick), as mbd_plan_set_mpc_pick
extern "C" int mbd_sweep_set_mpc_pick(mbd_sweep* w, const mbd_mpc_pick* rec) {
  if (!w) return fail(MBD_ERR_INVALID, "sweep is NULL");
  NO_SWEEP_SESSION(w, "set_mpc_pick");
  if (rec) MBD_TRY(check_mpc_pick(rec));  // (before any device access)
  if (rec && w->cfg.enable_demo)
    return fail(MBD_ERR_UNSUPPORTED, "mpc pick record: enable_demo=1: a demo plan's score is not the return the pick compares");
  if (rec && w->zone.has) return refuse_beside_zones("mpc pick record", "sweep");
  return w->pick.set(rec, w->env->device, w->P, w->HNu, w->cfg.Hsample);
}

extern "C" int mbd_sweep_peek_mpc_pick(mbd_sweep* w, int k, int32_t* choice_out, float* rets_out, int32_t* best_out, int capacity,
                                       int* count_out) {
  if (!w) return fail(MBD_ERR_INVALID, "sweep is NULL");
  return w->pick.peek(w->env, k, choice_out, rets_out, best_out, capacity, count_out, "sweep");
}

namespace {
// every episode's pick behind a tick's last step (PickRec::tick): the tick planned from plan_from [P][S] and started from ybar0
// [P][HNu]; i_start: its first diffusion step; buf: the ring buffer its last step's normals lie in (MBD sweeps)
int sweep_pick(mbd_sweep* w, const float* plan_from, const float* ybar0, int i_start, int buf, unsigned cold, hipStream_t s) {
  if (!w->pick.has) return MBD_OK;
  const int Nd = w->cfg.Ndiffuse, HNu = w->HNu;
  const long long mu_stride = (long long)(Nd - 1) * HNu;
  const bool lazy = w->cfg.update_method == 0;
  PickTick pt{};
  pt.state = plan_from; pt.N = w->cfg.Nsample; pt.rews = w->d_rews;
  pt.cand = lazy ? w->d_eps[buf].get() : w->d_Y0s.get();
  pt.lazy = lazy; pt.sigma = w->sigmas[1];
  pt.ybar_i = i_start == 1 ? ybar0 : w->d_mu + (size_t)(Nd - 3) * HNu;  // (Ybar_1 of the last step: the tick's own start, or slot Nd-3)
  pt.ybar_i_stride = i_start == 1 ? HNu : mu_stride;
  pt.M = w->d_mu + (size_t)(Nd - 2) * HNu; pt.M_stride = mu_stride;
  pt.B = ybar0; pt.B_stride = HNu;
  pt.cold = cold;
  return w->pick.tick(w->env, w->obj, w->val, pt, s);
}
}  // namespace

extern "C" int mbd_sweep_set_mpc_plant(mbd_sweep* w, int k, const mbd_mpc_plant* rec) {
  if (!w) return fail(MBD_ERR_INVALID, "sweep is NULL");
  if (k < 0 || k >= w->P) return fail(MBD_ERR_INVALID, "episode k=%d outside [0,%d)", k, w->P);
  NO_SWEEP_SESSION(w, "set_mpc_plant");
  if (!rec) {
    w->has_plant[k] = false;
    w->plant_rec[k] = mbd_mpc_plant{};
    return MBD_OK;
  }
  MBD_TRY(check_mpc_plant(w->env, rec));
  w->plant_rec[k] = *rec;
  w->has_plant[k] = true;
  return MBD_OK;
}

// one delay record for all episodes of the sweep (include/mbd_hip.h mbd_mpc_delay): host state until an episode starts
extern "C" int mbd_sweep_set_mpc_delay(mbd_sweep* w, const mbd_mpc_delay* rec) {
  if (!w) return fail(MBD_ERR_INVALID, "sweep is NULL");
  NO_SWEEP_SESSION(w, "set_mpc_delay");
  return w->delay.set(rec, w->Nu);
}

// one demo record for all episodes of the sweep (include/mbd_hip.h mbd_mpc_demo)
extern "C" int mbd_sweep_set_mpc_demo(mbd_sweep* w, const mbd_mpc_demo* rec) {
  if (!w) return fail(MBD_ERR_INVALID, "sweep is NULL");
  NO_SWEEP_SESSION(w, "set_mpc_demo");
  return w->demo.set(w->env, w->cfg, rec);
}

extern "C" int mbd_sweep_peek_mpc_track(mbd_sweep* w, int k, float* err_out, float* windows_out) {
  if (!w) return fail(MBD_ERR_INVALID, "sweep is NULL");
  if (k < 0 || k >= w->P) return fail(MBD_ERR_INVALID, "episode k=%d outside [0,%d)", k, w->P);
  return w->demo.peek(w->env->device, k, err_out, windows_out, "sweep");
}

// one sigma record for all episodes of a path-integral sweep (include/mbd_hip.h mbd_mpc_sigma): host state
extern "C" int mbd_sweep_set_mpc_sigma(mbd_sweep* w, const mbd_mpc_sigma* rec) {
  if (!w) return fail(MBD_ERR_INVALID, "sweep is NULL");
  if (w->cfg.update_method == 0) return fail(MBD_ERR_STATE, "set_mpc_sigma: not a path-integral sweep (update_method == 0)");
  NO_SWEEP_SESSION(w, "set_mpc_sigma");
  return w->sigma_rec.set(rec, w->cfg.update_method);
}

extern "C" int mbd_sweep_peek_mpc_sigma(mbd_sweep* w, int k, float* sigmas_out) {
  if (!w) return fail(MBD_ERR_INVALID, "sweep is NULL");
  if (k < 0 || k >= w->P) return fail(MBD_ERR_INVALID, "episode k=%d outside [0,%d)", k, w->P);
  return w->sigma_rec.peek(w->env->device, k, sigmas_out, "sweep");
}

extern "C" int mbd_sweep_peek_mpc_predicted(mbd_sweep* w, float* predicted_out) {
  if (!w) return fail(MBD_ERR_INVALID, "sweep is NULL");
  if (!w->delay.has) return fail(MBD_ERR_STATE, "peek_mpc_predicted: the sweep has no delay record");
  if (w->delay.pred_ticks < 1) return fail(MBD_ERR_STATE, "peek_mpc_predicted: no batch has run with the record yet");
  HIP_TRY(hipSetDevice(w->env->device));
  HIP_TRY(hipDeviceSynchronize());
  if (!predicted_out) return MBD_OK;
  const size_t T = (size_t)w->delay.pred_ticks, P = (size_t)w->P, S = (size_t)w->env->state_size();
  std::vector<float> tmp(T * P * S);  // (tick-major on the device, episode-major for the caller)
  HIP_TRY(hipMemcpy(tmp.data(), w->d_mpc_pred, sizeof(float) * tmp.size(), hipMemcpyDeviceToHost));
  for (size_t t = 0; t < T; ++t)
    for (size_t k = 0; k < P; ++k) memcpy(predicted_out + (k * T + t) * S, tmp.data() + (t * P + k) * S, sizeof(float) * S);
  return MBD_OK;
}

// Batched receding horizon (include/mbd_hip.h): P episodes in lockstep, the host only enqueues.  The episodes' logs are
// tick-major on the device, so that the rollout of the executed rows writes s_{.,t+1} of all P episodes straight into slice
// t+1 of the state log (state_final is [B][S]) and the next tick's rollouts read their start states from that same slice:
// the sweep's own start states are never touched.  A tick boundary adds two launches on the sweep's stream —
// mpc_boundary_batch_kernel and the rollout of the executed rows, one candidate per episode — stream-ordered between the
// tick's last weighted mean and the next tick's first rollout, so the ring of noise buffers and the progress word carry
// across ticks with their argument unchanged (mbd_sweep): the steps of all ticks count through as one loop.
// With plant records (mbd_sweep_set_mpc_plant) the boundary grows in the same place on the same stream — behind
// mpc_boundary_batch_kernel come mpc_plant_rows_kernel (every episode's normals, executed rows and kick values), one rollout
// launch per maximal run of consecutive episodes that share a plant handle, each over its slice of the tick's rows, rewards
// and states, and, in the ticks where an episode is kicked, mpc_kick_batch_kernel on slice t+1 of the state log — so that
// argument is unchanged once more; the disturbance key chains are host arithmetic.  Without records: the two launches above.
// With a delay record (mbd_sweep_set_mpc_delay) a tick gains ONE launch in front of its first diffusion step on the sweep's
// stream: the sweep's env's rollout of every episode's committed queue from s_{.,t}, one candidate per episode over D E rows
// (the per-episode start states through the state stride of a sweep of one-candidate plans), writing shat_{.,t} into slice t
// of the predicted states, where the tick's P N planning candidates start.  It is stream-ordered behind the previous tick's
// boundary and in front of the tick's first rollout, stores nothing into the progress word and generates no normals, so the
// steps of all ticks still count through as one loop; the normals of the tick's first step, generated on the second stream
// beside the previous tick's last rollout, depend on their keys only and not on it.  The boundary's first kernel is the delay
// variant: it advances the queues into their other buffer and hands the queues' heads to the rollout of the executed rows.
extern "C" int mbd_sweep_run_mpc(mbd_sweep* w, const mbd_mpc_config* mc, const uint32_t* keys, float* actions_out,
                                 float* rewards_out, float* states_out, float* means_out, double* loop_seconds_out) {
  if (!w) return fail(MBD_ERR_INVALID, "sweep is NULL");
  if (!mc) return fail(MBD_ERR_INVALID, "mpc config is NULL");
  if (!keys) return fail(MBD_ERR_INVALID, "keys is NULL");
  NO_SWEEP_SESSION(w, "run_mpc");
  const mbd_plan_config& c = w->cfg;
  const int T = mc->n_ticks, K = mc->warm_steps, E = mc->exec_steps, Nd = c.Ndiffuse, H = c.Hsample;
  MBD_TRY(check_mpc_config(c, mc, w->demo.has, w->sigma_rec.has));
  MBD_TRY(w->delay.check_run(E));
  mbd_env* e = w->env;
  HIP_TRY(hipSetDevice(e->device));
  const int P = w->P, HNu = w->HNu, Nu = e->action_size(), S = e->state_size();
  const bool pi = c.update_method != 0;  // a path-integral sweep (with a sigma record: check_mpc_config)
  HIP_TRY(w->d_mpc_rows.grow((size_t)P * (H - 1) * Nu));
  HIP_TRY(w->d_mpc_ybar.grow((size_t)P * HNu));
  HIP_TRY(w->d_mpc_states.grow(((size_t)T + 1) * P * S));
  HIP_TRY(w->d_mpc_means.grow((size_t)T * P * HNu));
  HIP_TRY(w->d_mpc_rewards.grow((size_t)T * P * (H - 1)));
  const int EN = E * Nu;
  bool any_plant = false;
  for (int k = 0; k < P; ++k) any_plant = any_plant || w->has_plant[k];
  const bool has_delay = w->delay.has;
  const int D = w->delay.D, Q = D * EN;  // (an episode's committed queue: D blocks of E rows)
  if (has_delay) {
    HIP_TRY(w->d_mpc_queue.grow(2 * (size_t)P * Q));
    HIP_TRY(w->d_mpc_pred.grow((size_t)T * P * S));
  }
  if (any_plant || has_delay) HIP_TRY(w->d_mpc_actions.grow((size_t)T * P * EN));
  if (any_plant) {
    HIP_TRY(w->d_plant_eps.grow((size_t)P * ((size_t)(H - 1) * Nu + 3)));
    HIP_TRY(w->d_plant_kick.grow((size_t)P * 3));
  }
  // with a demo record: every plant must write the positions of the sweep's env's tracked links
  const bool has_demo = w->demo.has;
  for (int k = 0; k < P; ++k)
    if (w->has_plant[k] && w->plant_rec[k].plant) MBD_TRY(w->demo.check_plant(e, w->plant_rec[k].plant));
  // with a zone record likewise, and room for the log of the executed steps
  for (int k = 0; k < P; ++k)
    if (w->has_plant[k] && w->plant_rec[k].plant) MBD_TRY(w->zone.check_plant(e, w->plant_rec[k].plant));
  MBD_TRY(w->zone.start(T, P, E));
  const int planar = (e->model.flags & MBD_FLAG_PLANAR) ? 1 : 0;
  // the disturbance key chains: dk, d_t = split(dk) per tick and episode
  std::vector<uint32_t> dk(2 * (size_t)P, 0u);
  for (int k = 0; k < P; ++k)
    if (w->has_plant[k]) { dk[2 * k] = w->plant_rec[k].key[0]; dk[2 * k + 1] = w->plant_rec[k].key[1]; }
  hipStream_t s = w->stream;
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipStreamSynchronize(w->aux));
  HIP_TRY(hipMemcpyAsync(w->d_mpc_states, w->d_state0, sizeof(float) * (size_t)P * S, hipMemcpyDeviceToDevice, s));  // s_{.,0}
  if (has_delay) {
    MBD_TRY(w->delay.upload(w->d_mpc_queue, P, E, Nu, s));
    w->delay.pred_ticks = 0;
  }
  // with an objective record: every episode's previous action of tick 0 (mbd_plan_run_mpc), and the episodes' slot to the call's end
  MBD_TRY(w->obj.episode_start(has_delay ? w->d_mpc_queue + (Q - Nu) : nullptr, Q, s));
  struct ObjEpisode {
    ObjectiveRec& o;
    ~ObjEpisode() { o.episode_end(); }
  } obj_episode{w->obj};
  MBD_TRY(w->pick.start(T));  // (a pick record's logs: one entry per tick and episode)
  w->elite.restart();         // (an elite record's logs: the episodes' steps)
  HIP_TRY(hipStreamSynchronize(s));
  progress_reset(w->h_progress);
  const auto t0 = std::chrono::steady_clock::now();
  if (has_demo) MBD_TRY(w->demo.start(T, P, E, has_delay ? D : 0, s));  // (the table of the ticks' windows: one launch)
  // per episode: rng, k_t = split(rng) per tick, the tick's chain r, Y0s_rng = split(r) per step from r = k_t.  The keys
  // are drawn in the order the steps run, one step ahead of the rollouts (the normals of a tick's first step are prepared
  // beside the previous tick's last rollout, like any other step's)
  std::vector<uint32_t> rng(keys, keys + 2 * (size_t)P), r(2 * (size_t)P);
  SweepKeys tick, sk;
  auto first_keys_of_tick = [&]() {
    sweep_split_keys(w, rng, tick);
    for (int k = 0; k < P; ++k) { r[2 * k] = tick.k[k][0]; r[2 * k + 1] = tick.k[k][1]; }
    sweep_split_keys(w, r, sk);
  };
  if (pi) {  // nothing is prepared ahead: sigma = sigma_cold of every episode and the logs' first entries, one launch
    MBD_TRY(w->sigma_rec.start(T, P));
    w->sigma_rec.launch(w->d_sigma, P, 0, true, s);
  } else {
    first_keys_of_tick();
    sweep_noise(w, sk, 0, s, w->noise.spec(false));  // tick 0, step Nd-1
  }
  HIP_TRY(hipGetLastError());
  const long long mu_stride = (long long)(Nd - 1) * HNu;
  const int exec_sw[3] = {1, S, 0};
  for (int t = 0, q = 0; t < T; ++t) {
    const float* states_t = w->d_mpc_states + (size_t)t * P * S;
    const int i_start = t == 0 ? Nd - 1 : K;
    w->wt.begin();  // (a weighting record's log holds the last tick's steps)
    // with an elite record, ONE launch in front of the tick's first sampler: no elites in tick 0 and without carry, otherwise every
    // episode's shifted E rows forward with its mean
    MBD_TRY(elite_table_all(w->elite, P, HNu, t == 0 || !w->elite.carry ? -1 : EN, s));
    // with a delay record: every episode's committed rows, the prediction of where they leave it, and the plans from there
    const float* q_in = has_delay ? w->d_mpc_queue + (size_t)(t & 1) * P * Q : nullptr;
    float* q_out = has_delay ? w->d_mpc_queue + (size_t)((t + 1) & 1) * P * Q : nullptr;
    const float* plan_from = states_t;
    if (has_delay) {
      float* shat = w->d_mpc_pred + (size_t)t * P * S;
      MBD_TRY(launch_rollout(e, states_t, q_in, P, D * E, nullptr, nullptr, nullptr, shat, s, nullptr, exec_sw));
      plan_from = shat;
    }
    if (pi) {
      // a path-integral tick (include/mbd_hip.h mbd_mpc_sigma): rng, k_t = split(rng); r = k_t; per refinement r, Y0s_rng =
      // split(r) and mbd_sweep_run's lockstep step from the tick's states — every episode's keys, carried sigma and mean in the
      // one sampling launch — then the carried sigmas [P] across the boundary in one launch
      sweep_split_keys(w, rng, tick);
      for (int k = 0; k < P; ++k) { r[2 * k] = tick.k[k][0]; r[2 * k + 1] = tick.k[k][1]; }
      for (int i = i_start; i >= 1; --i) {
        sweep_split_keys(w, r, sk);
        PiStep st;
        st.slot = Nd - 1 - i;  // (K <= Nd-1: a warm tick's steps use the last K slots)
        st.state0 = plan_from;
        st.mu_in = i == i_start ? (t == 0 ? w->d_zero.get() : w->d_mpc_ybar.get()) : w->d_mu + (size_t)(st.slot - 1) * HNu;
        st.mu_stride = i == i_start ? HNu : mu_stride;
        st.ns = w->noise.spec(t != 0);
        MBD_TRY(sweep_pi_step(w, st, sk));
      }
      w->sigma_rec.launch(w->d_sigma, P, t, false, s);
      HIP_TRY(hipGetLastError());
    }
    for (int i = pi ? 0 : i_start; i >= 1; --i, ++q) {
      const bool follows = i > 1 || t + 1 < T;
      if (i > 1) sweep_split_keys(w, r, sk);
      else if (follows) first_keys_of_tick();
      SweepStep st;
      st.q = q; st.i = i; st.slot = Nd - 1 - i;  // (K <= Nd-1: a warm tick's steps use the last K slots)
      st.state0 = plan_from;
      st.ybar_in = i == i_start ? (t == 0 ? w->d_zero : w->d_mpc_ybar) : w->d_mu + (size_t)(st.slot - 1) * HNu;
      st.ybar_in_stride = i == i_start ? HNu : mu_stride;
      st.next_keys = follows ? &sk : nullptr;
      // (the noise shape and basis of the following step: this tick's, or — behind a tick's last step — a warm tick's,
      // mbd_plan_run_mpc)
      st.next_ns = w->noise.spec(!(t == 0 && i > 1));
      st.xref = has_demo ? w->demo.window(t) : nullptr;
      st.rew_xref = has_demo ? w->demo.rew_xref : e->rew_xref;
      st.g = t == 0 ? w->noise.shape_always() : w->noise.shape_warm();
      MBD_TRY(sweep_step(w, st));
    }
    // the boundary: the logs of M_{.,t}, its first E rows and Ybar of tick t+1; then the rows executed from s_{.,t}
    // (with a delay record the rows executed are the queues' heads: into the tick's slice of their log, which the rollout
    // reads — unless plant records form the disturbed rows there themselves)
    float* rows_t = any_plant || has_delay ? w->d_mpc_actions + (size_t)t * P * EN : nullptr;
    // (in front of all of it, with a pick record: every episode's P_t over its M_t where it lies)
    MBD_TRY(sweep_pick(w, plan_from, t == 0 ? w->d_zero.get() : w->d_mpc_ybar.get(), i_start, pi ? 0 : (q + 2) % 3,
                       t == 0 ? 0xffffffffu : 0u, s));
    // (in front of it, with an objective record: the next tick's previous actions, clip(M_{.,t}[E-1]), one launch)
    MBD_TRY(w->obj.tick_advance(w->d_mu + (size_t)(Nd - 2) * HNu + (size_t)(E - 1) * Nu, mu_stride, s));
    if (has_delay)
      hipLaunchKernelGGL(mpc_boundary_delay_batch_kernel, dim3(1, (unsigned)P), dim3(256), 0, s,
                         (const float*)(w->d_mu + (size_t)(Nd - 2) * HNu), mu_stride, HNu, EN, w->d_mpc_ybar,
                         w->d_mpc_means + (size_t)t * P * HNu, q_in, q_out, Q, any_plant ? (float*)nullptr : rows_t);
    else
      hipLaunchKernelGGL(mpc_boundary_batch_kernel, dim3(1, (unsigned)P), dim3(256), 0, s,
                         (const float*)(w->d_mu + (size_t)(Nd - 2) * HNu), mu_stride, HNu, E * Nu, w->d_mpc_ybar,
                         w->d_mpc_means + (size_t)t * P * HNu, w->d_mpc_rows);
    HIP_TRY(hipGetLastError());
    if (!any_plant) {
      // (with a demo record the launch also writes the tracked positions of every episode's E steps into their log)
      MBD_TRY(launch_rollout(e, states_t, has_delay ? rows_t : w->d_mpc_rows.get(), P, E, w->d_mpc_rewards + (size_t)t * P * E, nullptr,
                             has_demo ? w->demo.xlog(t, P, E) : w->zone.xlog(t, P, E), w->d_mpc_states + (size_t)(t + 1) * P * S, s,
                             nullptr, exec_sw));
      // (with a zone record: s_t and clr_t of every episode's E executed steps into the log, one launch over the P rows)
      MBD_TRY(w->zone.log(t, P, E, s));
      continue;
    }
    SweepPlant sp{};
    bool any_kick = false;
    for (int k = 0; k < P; ++k)
      if (w->has_plant[k] && plant_tick_draw(w->plant_rec[k], c.prng_impl, t, &dk[2 * k], sp, k)) any_kick = true;
    float* rewards_t = w->d_mpc_rewards + (size_t)t * P * E;
    float* states_t1 = w->d_mpc_states + (size_t)(t + 1) * P * S;
    // (the undisturbed rows: the means' first E, or the queues' heads)
    const float* rows_from = has_delay ? q_in : w->d_mu + (size_t)(Nd - 2) * HNu;
    hipLaunchKernelGGL(mpc_plant_rows_kernel, dim3(1, (unsigned)P), dim3(256), 0, s, sp, c.prng_impl, rows_from,
                       has_delay ? (long long)Q : mu_stride, EN, w->d_plant_eps, rows_t, w->d_plant_kick);
    HIP_TRY(hipGetLastError());
    auto plant_of = [&](int k) { return w->has_plant[k] && w->plant_rec[k].plant ? w->plant_rec[k].plant : e; };
    for (int k0 = 0; k0 < P;) {  // one launch per run of episodes that share a plant handle
      int k1 = k0 + 1;
      while (k1 < P && plant_of(k1) == plant_of(k0)) ++k1;
      MBD_TRY(launch_rollout(plant_of(k0), states_t + (size_t)k0 * S, rows_t + (size_t)k0 * EN, k1 - k0, E,
                             rewards_t + (size_t)k0 * E, nullptr, has_demo ? w->demo.xlog(t, P, E, k0) : w->zone.xlog(t, P, E, k0),
                             states_t1 + (size_t)k0 * S, s, nullptr, exec_sw));
      k0 = k1;
    }
    MBD_TRY(w->zone.log(t, P, E, s));
    if (any_kick) {
      hipLaunchKernelGGL(mpc_kick_batch_kernel, dim3(1, (unsigned)P), dim3(64), 0, s, sp, states_t1, S,
                         (const float*)w->d_plant_kick, planar);
      HIP_TRY(hipGetLastError());
    }
  }
  if (has_demo) MBD_TRY(w->demo.finish(T, P, E, s));
  HIP_TRY(hipStreamSynchronize(s));
  const auto t1 = std::chrono::steady_clock::now();
  if (loop_seconds_out) *loop_seconds_out = std::chrono::duration<double>(t1 - t0).count();
  // the logs are tick-major, the outputs episode-major: ONE device->host copy per log, transposed on the host
  std::vector<float> tmp;
  auto fetch = [&](const float* d_log, size_t n) {
    tmp.resize(n);
    return hipMemcpy(tmp.data(), d_log, sizeof(float) * n, hipMemcpyDeviceToHost);
  };
  // out [P][rows][n] from the first n floats of every row of tmp [rows][P][row]
  auto episode_major = [&](float* out, int rows, size_t row, size_t n) {
    for (int t = 0; t < rows; ++t)
      for (int k = 0; k < P; ++k)
        memcpy(out + ((size_t)k * rows + t) * n, tmp.data() + ((size_t)t * P + k) * row, sizeof(float) * n);
  };
  if (rewards_out) {
    HIP_TRY(fetch(w->d_mpc_rewards, (size_t)T * P * E));
    episode_major(rewards_out, T, E, E);
  }
  if (states_out) {
    HIP_TRY(fetch(w->d_mpc_states, ((size_t)T + 1) * P * S));
    episode_major(states_out, T + 1, S, S);
  }
  if (has_delay) w->delay.pred_ticks = T;
  if (w->zone.has) { w->zone.ticks = T; w->zone.exec = E; w->zone.episodes = P; }
  if (pi) { w->sigma_rec.ticks = T; w->sigma_rec.episodes = P; }
  if ((any_plant || has_delay) && actions_out) {  // (the executed rows carry the action noise, or are the queues': their own log)
    HIP_TRY(fetch(w->d_mpc_actions, (size_t)T * P * EN));
    episode_major(actions_out, T, EN, EN);
    actions_out = nullptr;
  }
  if (means_out || actions_out) {  // (the executed rows are M_t[0:E]: taken from the one copy of the means)
    HIP_TRY(fetch(w->d_mpc_means, (size_t)T * P * HNu));
    if (means_out) episode_major(means_out, T, HNu, HNu);
    if (actions_out) episode_major(actions_out, T, HNu, EN);
  }
  return MBD_OK;
}

// ---- sessions of sweeps (include/mbd_hip.h mbd_sweep_mpc_open) ---------------------------------------------------------------
// P sessions in lockstep: episode k is mbd_plan_mpc_open's session on a plan of the sweep's config with temps[k], bit for bit.  A
// tick is a loop of its own over sweep_step — the lockstep step mbd_sweep_run and mbd_sweep_run_mpc run — with the ring of noise
// buffers and the progress word starting afresh: the host has waited for the previous tick's event, the tick's last step leaves no
// job on the second stream, so both streams are idle when a tick begins, the progress word is reset as between two runs, and the
// tick's first normals are generated on the sweep's stream in front of its first rollout, as a run's are.  (A plan's session has
// them prepared beside the previous tick's last rollout; here whether episode k's next tick is cold is not known then, and the
// launch that would read them differs with it.  The bits depend on keys alone.)
// Ticks of different lengths: after mbd_sweep_mpc_reset_mean(k) episode k's tick runs steps Ndiffuse-1 .. 1 and the others' K .. 1.
// The lockstep loop then runs Ndiffuse-1 .. 1 for all: an episode that is not cold IDLES through the steps above K — its
// candidates are rolled out from keys (0, 0) and its warm mean, its key chain does not advance, and what those steps wrote for it
// is overwritten, in front of step K, by its shifted mean (one device-to-device copy per such episode), from which steps K .. 1
// then run with its own keys: the same K launches' worth of arithmetic on the same inputs as in a tick of its own, and episodes
// share no arithmetic (mbd_sweep_run's guarantee).  One launch samples under ONE noise shape and basis, so a tick in which some
// episodes are cold and some are not is refused (MBD_ERR_UNSUPPORTED) when a record in force in the warm ticks only makes the two
// differ.
namespace {
size_t sweep_mailbox_floats(const mbd_sweep* w, int EN) {
  return (size_t)w->P * (2 * (size_t)EN + (size_t)w->HNu + (size_t)w->env->state_size() + 2);
}
SessionMailbox sweep_mailbox(const mbd_sweep* w, float* base, int EN) {
  const size_t P = (size_t)w->P;
  SessionMailbox mb;
  mb.rows = base;
  mb.mean = mb.rows + P * EN;
  mb.head = mb.mean + P * w->HNu;
  mb.pred = mb.head + P * EN;
  mb.rew_mean = mb.pred + P * w->env->state_size();
  mb.flag = (int*)(mb.rew_mean + P);
  return mb;
}
// rng, Y0s_rng = split(rng) of the episodes that take part in a step; the others' chains stay and their keys are (0, 0)
void session_split_keys(const mbd_sweep* w, std::vector<uint32_t>& r, const bool* active, SweepKeys& out) {
  for (int k = 0; k < w->P; ++k) {
    out.k[k][0] = 0; out.k[k][1] = 0;
    if (!active[k]) continue;
    uint32_t ks[4];
    host_split(&r[2 * k], 2, w->cfg.prng_impl, ks);
    r[2 * k] = ks[0]; r[2 * k + 1] = ks[1];
    out.k[k][0] = ks[2]; out.k[k][1] = ks[3];
  }
}
}  // namespace

extern "C" int mbd_sweep_mpc_open(mbd_sweep* w, const mbd_mpc_config* mc, const uint32_t* keys) {
  if (!w) return fail(MBD_ERR_INVALID, "sweep is NULL");
  if (!mc) return fail(MBD_ERR_INVALID, "mpc config is NULL");
  if (!keys) return fail(MBD_ERR_INVALID, "keys is NULL");
  MBD_TRY(check_mpc_config(w->cfg, mc, w->demo.has, w->sigma_rec.has, true));
  MBD_TRY(w->delay.check_run(mc->exec_steps));
  for (int k = 0; k < w->P; ++k)
    if (w->has_plant[k])
      return fail(MBD_ERR_STATE, "mpc_open: episode %d carries a plant record: in a session the caller is the plant", k);
  NO_SWEEP_SESSION(w, "mpc_open");
  mbd_env* e = w->env;
  HIP_TRY(hipSetDevice(e->device));
  SweepSession& ss = w->session;
  const int P = w->P, S = e->state_size(), EN = mc->exec_steps * w->Nu, Q = w->delay.D * EN;
  HIP_TRY(w->d_mpc_states.grow((size_t)P * S));
  HIP_TRY(w->d_mpc_ybar.grow((size_t)P * w->HNu));
  if (w->delay.has) {
    HIP_TRY(w->d_mpc_queue.grow(2 * (size_t)P * Q));
    HIP_TRY(w->d_mpc_pred.grow((size_t)P * S));
  }
  HIP_TRY(ss.stage.alloc((size_t)P * S));
  HIP_TRY(ss.mailbox.alloc(sweep_mailbox_floats(w, EN)));
  if (!ss.done) HIP_TRY(ss.done.create());
  hipStream_t s = w->stream;
  if (w->delay.has) MBD_TRY(w->delay.upload(w->d_mpc_queue, P, mc->exec_steps, w->Nu, s));
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipStreamSynchronize(w->aux));
  if (w->demo.has) MBD_TRY(w->demo.session_start());
  MBD_TRY(w->pick.start(mc->n_ticks));
  // an objective record's previous actions of the first tick and the session's slot until close: behind everything else that can
  // fail (a failed open leaves prev as it was); the launch is stream-ordered in front of the first tick
  MBD_TRY(w->obj.episode_start(w->delay.has ? w->d_mpc_queue + (Q - w->Nu) : nullptr, Q, s));
  // (nothing fails from here on: the bookkeeping of the previous batch's logs goes last)
  if (w->delay.has) w->delay.pred_ticks = 0;  // (mbd_sweep_peek_mpc_predicted does not serve sessions)
  w->elite.restart();                         // (an elite record's logs: the session's steps)
  ss.mc = *mc;
  ss.rng.assign(keys, keys + 2 * (size_t)P);
  for (int k = 0; k < MBD_SWEEP_MAX_PLANS; ++k) { ss.cold[k] = true; ss.flags[k] = 0; }
  ss.t = 0; ss.qbuf = 0;
  ss.in_flight = false;
  ss.open = true;
  return MBD_OK;
}

extern "C" int mbd_sweep_mpc_submit(mbd_sweep* w, const float* states) {
  if (!w) return fail(MBD_ERR_INVALID, "sweep is NULL");
  if (!states) return fail(MBD_ERR_INVALID, "states is NULL");
  SweepSession& ss = w->session;
  if (!ss.open) return fail(MBD_ERR_STATE, "mpc_submit: no session is open on this sweep");
  if (ss.in_flight) return fail(MBD_ERR_STATE, "mpc_submit: a tick is in flight (mbd_sweep_mpc_collect first)");
  if (ss.t >= ss.mc.n_ticks) return fail(MBD_ERR_STATE, "mpc_submit: the session has served its n_ticks=%d ticks", ss.mc.n_ticks);
  mbd_env* e = w->env;
  const mbd_plan_config& c = w->cfg;
  const int P = w->P, S = e->state_size(), E = ss.mc.exec_steps, K = ss.mc.warm_steps, EN = E * w->Nu, HNu = w->HNu, Nd = c.Ndiffuse;
  const bool has_delay = w->delay.has;
  const int D = w->delay.D, Q = D * EN;
  bool any_cold = false, all_cold = true;
  for (int k = 0; k < P; ++k) { any_cold = any_cold || ss.cold[k]; all_cold = all_cold && ss.cold[k]; }
  const NoiseSpec ns = w->noise.spec(!all_cold);
  if (any_cold && !all_cold && !(w->noise.spec(false) == w->noise.spec(true)))
    return fail(MBD_ERR_UNSUPPORTED, "mpc_submit: some episodes' ticks are cold and some are not, under a noise shape or basis in force "
                                     "in the warm ticks only: one launch samples under one; reset every episode's mean, or none's");
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t s = w->stream;
  ss.t_submit = std::chrono::steady_clock::now();
  int flags[MBD_SWEEP_MAX_PLANS];
  for (int k = 0; k < P; ++k) {
    flags[k] = ss.cold[k] ? MBD_TICK_COLD : 0;
    for (int j = 0; j < S; ++j)
      if (!std::isfinite(states[(size_t)k * S + j])) flags[k] |= MBD_TICK_STATE_NONFINITE;
  }
  memcpy(ss.stage.host(), states, sizeof(float) * (size_t)P * S);
  float* states_t = w->d_mpc_states;
  HIP_TRY(hipMemcpyAsync(states_t, ss.stage.host(), sizeof(float) * (size_t)P * S, hipMemcpyHostToDevice, s));
  for (int k = 0; k < P; ++k)
    if (ss.cold[k]) HIP_TRY(hipMemsetAsync(w->d_mpc_ybar + (size_t)k * HNu, 0, sizeof(float) * HNu, s));
  // the keys: a copy of the chains is advanced and committed with the tick
  std::vector<uint32_t> rng(ss.rng), r(2 * (size_t)P);
  SweepKeys tick, sk, sk_next;
  sweep_split_keys(w, rng, tick);
  for (int k = 0; k < P; ++k) { r[2 * k] = tick.k[k][0]; r[2 * k + 1] = tick.k[k][1]; }
  if (w->demo.has) MBD_TRY(w->demo.session_window(ss.t, E, has_delay ? D : 0, s));
  const float* q_in = has_delay ? w->d_mpc_queue + (size_t)ss.qbuf * P * Q : nullptr;
  float* q_out = has_delay ? w->d_mpc_queue + (size_t)(ss.qbuf ^ 1) * P * Q : nullptr;
  const float* plan_from = states_t;
  if (has_delay) {
    const int exec_sw[3] = {1, S, 0};
    MBD_TRY(launch_rollout(e, states_t, q_in, P, D * E, nullptr, nullptr, nullptr, w->d_mpc_pred, s, nullptr, exec_sw));
    plan_from = w->d_mpc_pred;
  }
  progress_reset(w->h_progress);  // (both streams are idle: see above)
  {  // with an elite record: a cold episode's elites go, the others' shift with their means (or go as well, without carry)
    EliteShifts sh;
    for (int k = 0; k < MBD_SWEEP_MAX_PLANS; ++k) sh.s[k] = ss.cold[k] || !w->elite.carry ? -1 : EN;
    MBD_TRY(elite_table(w->elite, P, HNu, sh, 0xffffffffu, s));
  }
  const int i_start = any_cold ? Nd - 1 : K;
  const long long mu_stride = (long long)(Nd - 1) * HNu;
  bool active[MBD_SWEEP_MAX_PLANS], active_next[MBD_SWEEP_MAX_PLANS];
  for (int k = 0; k < P; ++k) active[k] = ss.cold[k] || i_start <= K;
  session_split_keys(w, r, active, sk);
  sweep_noise(w, sk, 0, s, ns);
  HIP_TRY(hipGetLastError());
  w->wt.begin();
  for (int i = i_start, q = 0; i >= 1; --i, ++q) {
    if (i > 1) {
      for (int k = 0; k < P; ++k) active_next[k] = ss.cold[k] || i - 1 <= K;
      session_split_keys(w, r, active_next, sk_next);
    }
    SweepStep st;
    st.q = q; st.i = i; st.slot = Nd - 1 - i;
    st.state0 = plan_from;
    if (i == K && i != i_start)  // the episodes that idled so far start here, from their shifted means
      for (int k = 0; k < P; ++k)
        if (!ss.cold[k])
          HIP_TRY(hipMemcpyAsync(w->d_mu + (size_t)k * mu_stride + (size_t)(st.slot - 1) * HNu, w->d_mpc_ybar + (size_t)k * HNu,
                                 sizeof(float) * HNu, hipMemcpyDeviceToDevice, s));
    st.ybar_in = i == i_start ? w->d_mpc_ybar.get() : w->d_mu + (size_t)(st.slot - 1) * HNu;
    st.ybar_in_stride = i == i_start ? HNu : mu_stride;
    st.next_keys = i > 1 ? &sk_next : nullptr;
    st.next_ns = ns;
    st.xref = w->demo.has ? w->demo.window(0) : nullptr;
    st.rew_xref = w->demo.has ? w->demo.rew_xref : e->rew_xref;
    st.g = ns.g;
    st.mask = 0;  // (an elite record's launches leave out the episodes that idle through this step)
    for (int k = 0; k < P; ++k) st.mask |= (ss.cold[k] || i <= K) ? 1u << k : 0u;
    MBD_TRY(sweep_step(w, st));
  }
  // a pick record's launches, then the next tick's previous actions (an objective record), in FRONT of the boundary, which stays
  // the tick's last kernel
  {
    unsigned cold = 0;
    for (int k = 0; k < P; ++k) cold |= ss.cold[k] ? 1u << k : 0u;
    MBD_TRY(sweep_pick(w, plan_from, w->d_mpc_ybar.get(), i_start, (i_start - 1) % 3, cold, s));
  }
  MBD_TRY(w->obj.tick_advance(w->d_mu + (size_t)(Nd - 2) * HNu + (size_t)(E - 1) * w->Nu, mu_stride, s));
  hipLaunchKernelGGL(mpc_session_boundary_batch_kernel, dim3(1, (unsigned)P), dim3(256), 0, s,
                     (const float*)(w->d_mu + (size_t)(Nd - 2) * HNu), mu_stride, HNu, EN, w->d_mpc_ybar.get(), q_in, q_out, Q,
                     has_delay ? (const float*)w->d_mpc_pred : (const float*)nullptr, S, (const float*)(w->d_rewmeans + (Nd - 2)), Nd - 1,
                     sweep_mailbox(w, ss.mailbox.dev(), EN));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ss.done, s));
  ss.rng = rng;
  for (int k = 0; k < P; ++k) ss.flags[k] = flags[k];
  ss.in_flight = true;
  return MBD_OK;
}

extern "C" int mbd_sweep_mpc_collect(mbd_sweep* w, float* rows_out, float* means_out, float* heads_out, float* predicted_out,
                                     mbd_mpc_tick_info* infos_out) {
  if (!w) return fail(MBD_ERR_INVALID, "sweep is NULL");
  SweepSession& ss = w->session;
  if (!ss.open) return fail(MBD_ERR_STATE, "mpc_collect: no session is open on this sweep");
  if (!ss.in_flight) return fail(MBD_ERR_STATE, "mpc_collect: no tick is in flight (mbd_sweep_mpc_submit first)");
  HIP_TRY(hipSetDevice(w->env->device));
  HIP_TRY(hipEventSynchronize(ss.done));
  const size_t P = (size_t)w->P, S = (size_t)w->env->state_size(), EN = (size_t)ss.mc.exec_steps * w->Nu;
  const SessionMailbox mb = sweep_mailbox(w, ss.mailbox.host(), (int)EN);
  if (rows_out) memcpy(rows_out, mb.rows, sizeof(float) * P * EN);
  if (means_out) memcpy(means_out, mb.mean, sizeof(float) * P * w->HNu);
  if (heads_out) memcpy(heads_out, mb.head, sizeof(float) * P * EN);
  if (predicted_out) memcpy(predicted_out, w->delay.has ? mb.pred : ss.stage.host(), sizeof(float) * P * S);
  const auto t1 = std::chrono::steady_clock::now();
  for (size_t k = 0; k < P; ++k) {
    if (infos_out) {
      infos_out[k] = mbd_mpc_tick_info{};
      infos_out[k].tick = ss.t;
      infos_out[k].flags = ss.flags[k] | (mb.flag[k] ? MBD_TICK_ROWS_NONFINITE : 0);
      infos_out[k].rew_mean = mb.rew_mean[k];
      infos_out[k].seconds = std::chrono::duration<float>(t1 - ss.t_submit).count();
    }
    ss.cold[k] = false;
  }
  ss.in_flight = false;
  ss.qbuf ^= 1;
  ss.t += 1;
  return MBD_OK;
}

extern "C" int mbd_sweep_mpc_tick(mbd_sweep* w, const float* states, float* rows_out, float* means_out, float* heads_out,
                                  float* predicted_out, mbd_mpc_tick_info* infos_out) {
  MBD_TRY(mbd_sweep_mpc_submit(w, states));
  return mbd_sweep_mpc_collect(w, rows_out, means_out, heads_out, predicted_out, infos_out);
}

extern "C" int mbd_sweep_mpc_reset_mean(mbd_sweep* w, int k) {
  if (!w) return fail(MBD_ERR_INVALID, "sweep is NULL");
  if (!w->session.open) return fail(MBD_ERR_STATE, "mpc_reset_mean: no session is open on this sweep");
  if (k < 0 || k >= w->P) return fail(MBD_ERR_INVALID, "mpc_reset_mean: episode k=%d outside [0,%d)", k, w->P);
  if (w->session.in_flight) return fail(MBD_ERR_STATE, "mpc_reset_mean: a tick is in flight (mbd_sweep_mpc_collect first)");
  w->session.cold[k] = true;  // (the next submit zeroes its Ybar; its queue stays)
  if (w->elite.has) {  // (an elite record's elites of episode k are gone: written now as well, so that mbd_sweep_peek_elites says so)
    HIP_TRY(hipSetDevice(w->env->device));
    EliteShifts sh;
    for (int& v : sh.s) v = -1;
    MBD_TRY(elite_table(w->elite, w->P, w->HNu, sh, 1u << k, w->stream));
  }
  return MBD_OK;
}

extern "C" int mbd_sweep_mpc_close(mbd_sweep* w) {
  if (!w) return fail(MBD_ERR_INVALID, "sweep is NULL");
  SweepSession& ss = w->session;
  if (!ss.open) return fail(MBD_ERR_STATE, "mpc_close: no session is open on this sweep");
  HIP_TRY(hipSetDevice(w->env->device));
  if (ss.in_flight) HIP_TRY(hipStreamSynchronize(w->stream));  // (its last kernel writes the mailbox)
  ss.in_flight = false;
  ss.open = false;
  w->obj.episode_end();
  ss.stage.release();
  ss.mailbox.release();
  return MBD_OK;
}
