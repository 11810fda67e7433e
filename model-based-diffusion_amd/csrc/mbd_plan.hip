// mbd_plan.hip — the planner fast path (include/mbd_hip.h): the plan handle and the noise ring of lazy plans, one
// reverse-diffusion step split at its exchange point (mbd_plan_sample_rollout / mbd_plan_score_update; the step functions
// behind them take the rollouts' start state as a parameter), and the loops over steps (mbd_plan_reverse_once, mbd_plan_run,
// mbd_plan_eval, mbd_plan_peek; the receding-horizon loop mbd_plan_run_mpc, the session mbd_plan_mpc_*).  mbd_planner.py:84-148,179-180.
// Of the records a plan carries (mbd_internal.h; their members, check_* and kernels: mbd_records.hip) this unit holds what reads the
// handle: the mbd_plan_set_* / mbd_plan_peek_* entries with the refusals that depend on what else the plan carries, in their
// order; the ensemble and plant records, which are the plan's own; the launches of the elite and to-go records, whose kernels
// are step kernels; and the mbd_debug_* entries that launch a sampler or a step kernel.
#define MBD_WEIGH_KERNEL 1  // this unit launches weigh_kernel (mbd_step_kernels.h)
#define MBD_ELITE_KERNEL 1  // ... and the elite record's kernels (a plan's forms)
#define MBD_TOGO_KERNEL 1   // ... and the to-go record's
#include "mbd_internal.h"
#include "mbd_step_kernels.h"
#include "../../include/mbd_hip_debug.h"

// LAZY plans (the MBD update on a rigid-body env): the candidates are never materialised.  eps[b] holds the normals
// [N][HNu] of a diffusion step; the rollout's action fetch and the weighted mean form clip(eps sigma_i + Ybar_i)
// on the fly (RolloutParams).  A ring of buffers: while step k reads one, the normals of step k+1 (they depend on that
// step's key only) are generated into the next — by spare workgroups of step k's rollout launch, or on the aux
// stream when that launch fills the chip (mbd_plan_prefetch_noise declares the key).  THREE buffers, so that the aux
// stream needs no event from the step's stream while the caller keeps in step with the device: the buffer step k+1's
// normals go into was last read by step k-2's weighted mean, which has finished once the rollout of step k-1 has
// STARTED — every rollout launch of the plan stores its sequence number into the progress word (pinned host memory) as it
// starts, and the host looks there.  A caller that runs ahead of the device (mbd_plan_run's loop, the async leg of the
// bench) gets the event-ordered form: a mark on the step's stream in front of the rollout, a wait on the aux stream.
// (Other launches between two steps on the step's stream — a receding-horizon episode's two per tick — change neither
// argument: they are stream-ordered behind the weighted mean and in front of the next rollout.)
struct NoiseRing {
  Event ev_noise[3], ev_wm;  // created with the plan's second stream (ensure_aux): a plan without one carries no event
  DevBuf<float> eps[3];
  int cur = 0;                             // buffer of the step in flight (set by sample_rollout, read by score_update / peek)
  uint32_t key[3][2] = {{0, 0}, {0, 0}, {0, 0}};
  bool valid[3] = {false, false, false};   // eps[b] holds normal(key[b]) ...
  NoiseSpec spec[3];                       // ... made under this noise shape and basis (the plan's d_shape, d_basis)
  bool on_aux[3] = {false, false, false};  // ... generated on the aux stream: the reader checks ev_noise[b] first
  int read_seq[3] = {0, 0, 0};             // sequence number of the last rollout launch that read eps[b]
  PinnedWord progress;
  int seq = 0;
  bool in_step = false;        // the last sample_rollout found the host in step with the device (a per-step host read)
  bool wm_mark_valid = false;  // ev_wm was recorded behind the latest weighted mean
  bool kept_in_step = false;   // plan_keep_in_step held the host back for the coming sample_rollout (the queue is NOT draining)
  uint32_t hint_key[2] = {0, 0};  // mbd_plan_prefetch_noise: key of the step after the next sample_rollout
  NoiseSpec hint_ns;              // ... and the noise shape and basis that step samples under
  bool hint_valid = false;

  // the buffer that holds the normals of key k made under ns, or -1
  int find(const uint32_t k[2], const NoiseSpec& ns) const {
    int at = -1;
    for (int b = 0; b < 3; ++b)
      if (valid[b] && key[b][0] == k[0] && key[b][1] == k[1] && spec[b] == ns) at = b;
    return at;
  }
  void holds(int b, const uint32_t k[2], const NoiseSpec& ns) {
    key[b][0] = k[0]; key[b][1] = k[1];
    spec[b] = ns;
    valid[b] = true;
  }
  // nothing prepared ahead survives (mbd_plan_set_noise_shape, mbd_plan_set_noise_basis: the table behind a pointer has changed)
  void forget() {
    for (int b = 0; b < 3; ++b) valid[b] = false;
    hint_valid = false;
  }
  // the reader (or the next writer) of a buffer the aux stream filled: no wait on the step's stream when the job has
  // already finished
  int join(int b, hipStream_t s) {
    if (!on_aux[b]) return MBD_OK;
    on_aux[b] = false;
    if (hipEventQuery(ev_noise[b]) == hipSuccess) return MBD_OK;
    (void)hipGetLastError();  // (hipErrorNotReady is not an error here)
    HIP_TRY(hipStreamWaitEvent(s, ev_noise[b], 0));
    return MBD_OK;
  }
  // takes the declared key: whether there is one that is not this step's own
  bool take_hint(const uint32_t step_key[2], uint32_t out[2], NoiseSpec* ns_out) {
    const bool have = hint_valid && !(hint_key[0] == step_key[0] && hint_key[1] == step_key[1]);
    hint_valid = false;
    out[0] = hint_key[0]; out[1] = hint_key[1];
    *ns_out = hint_ns;
    return have;
  }
  // Aux-stream generation into eps[b] must start after the last reader of eps[b] — the weighted mean behind rollout launch
  // number read_seq[b] — and should not wait for the rollout about to be launched on s.  That reader has finished once the
  // NEXT rollout launch of the plan has started (the progress word); a host that has not seen that yet puts a mark onto s,
  // in front of the coming launch, for the aux stream to wait on (*marked)
  int mark_last_reader(int b, hipStream_t s, bool* marked) {
    const int r = read_seq[b];
    in_step = (r == 0 || progress_read(progress) >= r + 1) && !kept_in_step;
    kept_in_step = false;
    *marked = false;
    // the caller runs ahead of the device (an asynchronous loop): it is held here until the rollout before this one has
    // started — the queue still holds that rollout and its score, so the device does not wait for the host — rather
    // than paying a record on s and a wait on the aux stream per step (~20 us at N = 8192).  Bounded: a stream that is
    // itself waiting for something the caller has yet to do gets the mark after 5 ms.
    if (r != 0 && progress_read(progress) < r + 1) *marked = !progress_wait(progress, r + 1, 5, 10);
    if (*marked) HIP_TRY(hipEventRecord(ev_wm, s));
    return MBD_OK;
  }
  // ... and the aux stream's side of it, in front of the job.  (A caller in step with the device — it reads every step's
  // mean reward before it dispatches the next — launches the job while the previous step's weighted mean is still running:
  // the job waits for the mark behind that kernel, which cost nothing there (the queue was about to drain), instead of
  // competing with it for the memory system)
  int aux_waits_for_mark(hipStream_t aux, bool marked) {
    if (marked || (in_step && wm_mark_valid)) HIP_TRY(hipStreamWaitEvent(aux, ev_wm, 0));
    return MBD_OK;
  }
  // behind a weighted mean on s: the mark, only where the record is free (see aux_waits_for_mark)
  int mark_wmean(hipStream_t s, bool has_aux) {
    wm_mark_valid = false;
    if (has_aux && in_step && ev_wm) {
      HIP_TRY(hipEventRecord(ev_wm, s));
      wm_mark_valid = true;
    }
    return MBD_OK;
  }
};

// A session (include/mbd_hip.h mbd_plan_mpc_open): the episode state mbd_plan_run_mpc keeps in locals, kept across calls, and
// the two pinned buffers a tick talks to the host through.  All zero: no session (a zeroed stand-in handle has none).
struct MpcSession {
  bool open = false, in_flight = false;
  bool cold = true;             // the next tick runs Ndiffuse-1 steps from Ybar = zeros (tick 0; after mbd_plan_mpc_reset_mean)
  mbd_mpc_config mc{};
  uint32_t rng[2] = {0, 0};     // the episode's key chain: rng, k_t = split(rng) per tick
  int t = 0;                    // ticks served
  int qbuf = 0;                 // the buffer of d_mpc_queue the next tick reads
  int flags = 0;                // of the tick in flight: what the host decided (COLD, STATE_NONFINITE)
  PinnedBuf stage, mailbox;     // the state on its way up [S]; rows | mean | head | predicted | rew_mean | flag on their way down
  Event done;                   // recorded behind the tick's boundary kernel
  std::chrono::steady_clock::time_point t_submit{};
};

struct mbd_plan {
  mbd_env* env = nullptr;
  hipStream_t last_stream = nullptr;  // stream of the plan's previous phase call (plan_enter orders a change of stream)
  bool last_stream_set = false;
  mbd_plan_config cfg;
  int HNu = 0, Nu = 0;
  std::vector<float> alphas, alphas_bar, sigmas;
  Stream stream;
  // second stream: the non-lazy sharded sampler's other-rank rows, and the next step's normals of lazy plans whose
  // rollout fills the chip (smaller rollouts generate them in spare workgroups of their own launch).  Created on first use
  // (ensure_aux), with its events: a second stream per plan costs hardware queues beside other plans
  Stream aux;
  Event ev_xs, ev_in, ev_aux;
  bool aux_pending = false;
  DevBuf<float> d_state0, d_Y0s, d_rewss, d_rews, d_lp, d_xpos, d_weights, d_Ybar, d_mu, d_rewmeans, d_scratch;
  DevBuf<float> d_wm_partial;  // [64][HNu] partials of the split weighted mean (plans of >= 4096 candidates)
  DevBuf<float> d_lg;          // [N] logp0 scratch of the score kernel for plans beyond kLdsN candidates
  bool lazy = false;
  NoiseRing ring;
  DevBuf<float> d_ybar_keep;         // [HNu] Ybar_i of the last finished step (mbd_plan_peek materialises Y0s from it)
  const float* peek_ybar = nullptr;  // the caller's d_Ybar_i between phase 1 and phase 2 of a step, d_ybar_keep after
  float sigma_last = 0.0f;
  DevBuf<float> d_sigma, d_spread;  // path-integral plans
  DevBuf<int> d_idx;
  // receding-horizon episodes (mbd_plan_run_mpc): the two states its ticks ping-pong between [2][state_size], and the
  // episode's logs — states [T+1][state_size], means [T][HNu], rewards [T][H-1] (E < H rows per tick) — grown on demand.
  // Plan-owned, so that nothing an episode leaves behind points at freed memory.
  DevBuf<float> d_mpc_state, d_mpc_states, d_mpc_means, d_mpc_rewards;
  // the plant record of the plan's episodes (mbd_plan_set_mpc_plant; a copy, the plant env is the caller's), and what an
  // episode with a record needs beyond the above: the log of the executed rows [T][E Nu] — the tick's rollout reads its
  // slice, so the rows exist once —, the tick's normals [E Nu + 3] and its three kick values
  mbd_mpc_plant plant_rec{};
  bool has_plant = false;
  DevBuf<float> d_mpc_actions, d_plant_eps, d_plant_kick;
  // the delay record (mbd_plan_set_mpc_delay), and what an episode with one needs beyond the above: the committed queue
  // [2][D E Nu] — a tick reads one buffer, its boundary kernel writes the advanced queue into the other — and the predicted
  // states [T][state_size]: the prediction rollout of tick t writes slot t and the tick's planning launches start from that
  // slot, so the states exist once.  (The executed rows are the queue's head, not the mean's: d_mpc_actions logs them.)
  DelayRec delay;
  DevBuf<float> d_mpc_queue, d_mpc_pred;
  // the demo record (mbd_plan_set_mpc_demo) with its buffers: the clip, the table of every tick's window, the log of the
  // executed steps' tracked positions and their distances from the clip
  DemoRec demo;
  // the sigma record of a path-integral plan (mbd_plan_set_mpc_sigma) with the log of the last episode's sigmas
  SigmaRec sigma_rec;
  // the ensemble record (mbd_plan_set_ensemble; a copy, NULL members resolved to the plan's env — the envs are the caller's)
  // and its buffers: the members' rewards r_m [M][N] and per-step rewards [M][N][H] of the rollout launch over M N
  // candidates, and the library's own copy of the combined rewards [N] (mbd_plan_peek_ensemble)
  mbd_ensemble ens_rec{};
  bool has_ens = false, ens_stepped = false;
  DevBuf<float> d_ens_rews, d_ens_rewss, d_ens_comb;
  // the noise shape (mbd_plan_set_noise_shape) and the noise basis (mbd_plan_set_noise_basis) with their tables; d_knot_z [N][HNu]
  // for materialised plans only
  NoiseRec noise;
  // the objective record (mbd_plan_set_objective) with its tables, the previous action and the last step's ret and cost
  ObjectiveRec obj;
  // the weighting record (mbd_plan_set_weighting) with the device log of its score steps
  WeightingRec wt;
  // the pick record (mbd_plan_set_mpc_pick) with its slots and the device log of its ticks
  PickRec pick;
  // the value record (mbd_plan_set_value) with its net, the shard's final states and the last step's V
  ValueRec val;
  // the zone record (mbd_plan_set_zones) with its table, the step's tracked positions and the last step's pen and clr
  ZoneRec zone;
  // the adapt record (mbd_plan_set_adapt) with its table, the shape the samplers draw under and the device log of its steps
  AdaptRec adapt;
  // the elite record (mbd_plan_set_elites) with the elites, their count on the device and the device log of its steps
  EliteRec elite;
  // the to-go record (mbd_plan_set_togo) with the groups' returns and weights of the last step
  TogoRec togo;
  TimingPool timing;
  // the session a caller drives tick by tick (mbd_plan_mpc_open); it uses the episodes' buffers above — d_mpc_state for the
  // state handed in, d_mpc_pred for the one predicted state, d_mpc_queue — so a handle runs episodes or a session, not both
  MpcSession session;
  ~mbd_plan() {  // (streams, events and buffers release themselves, on the env's device)
    if (env) (void)hipSetDevice(env->device);
  }
};

// the refusal of a call that would disturb an open session (include/mbd_hip.h mbd_plan_mpc_close)
#define NO_SESSION(p, what) \
  if ((p)->session.open) return fail(MBD_ERR_STATE, what ": a session is open on this plan (mbd_plan_mpc_close first)")
// the refusal of a plan-only record on a sharded plan (kind: "adapt", "elite", "to-go", "zone")
static int refuse_sharded(const mbd_plan_config& c, const char* kind) {
  return fail(MBD_ERR_STATE, "%s record: shard_count=%d of Nsample=%d: sharded plans take no %s record", kind, c.shard_count, c.Nsample,
              kind);
}

// ==================================================================================================
// planner
// ==================================================================================================
extern "C" int mbd_plan_create(mbd_env* env, const mbd_plan_config* cfg, mbd_plan** out) {
  if (!env || !cfg || !out) return fail(MBD_ERR_INVALID, "NULL argument");
  if (cfg->Nsample < 1 || cfg->Hsample < 1 || cfg->Ndiffuse < 2) return fail(MBD_ERR_INVALID, "Nsample/Hsample/Ndiffuse");
  if (cfg->shard_begin < 0 || cfg->shard_count < 1 || cfg->shard_begin + cfg->shard_count > cfg->Nsample)
    return fail(MBD_ERR_INVALID, "shard [%d,+%d) outside N=%d", cfg->shard_begin, cfg->shard_count, cfg->Nsample);
  if (cfg->update_method < 0 || cfg->update_method > 3) return fail(MBD_ERR_INVALID, "update_method=%d", cfg->update_method);
  if (cfg->update_method > 0 && cfg->enable_demo) return fail(MBD_ERR_INVALID, "path-integral plans do not use demos");
  if (cfg->enable_demo) {
    if (!env->has_xref) return fail(MBD_ERR_INVALID, "enable_demo needs an env created with xref");
    if (cfg->Hsample != kXrefRows) return fail(MBD_ERR_INVALID, "demos require Hsample == %d (xref has %d rows)", kXrefRows, kXrefRows);
  }
  // logp0 [N] of the score kernel (and the cem selection's copy of the weights) live in LDS up to kLdsN candidates:
  // beyond the default 48 KB window the kernels' dynamic-LDS limit is raised; beyond kLdsN they use a plan-owned
  // global scratch instead — the candidate count is bounded by HBM, not by LDS
  if ((size_t)cfg->Nsample * sizeof(float) > 48 * 1024 && cfg->Nsample <= kLdsN) {
    HIP_TRY(hipSetDevice(env->device));
    HIP_TRY(hipFuncSetAttribute((const void*)score_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024));
    HIP_TRY(hipFuncSetAttribute((const void*)cem_select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024));
  }
  HIP_TRY(hipSetDevice(env->device));
  std::unique_ptr<mbd_plan> guard(new mbd_plan());
  mbd_plan* p = guard.get();
  p->env = env;
  p->cfg = *cfg;
  const int N = cfg->Nsample, H = cfg->Hsample, Nu = env->action_size(), Nd = cfg->Ndiffuse, sh = cfg->shard_count;
  p->HNu = H * Nu;
  p->Nu = Nu;
  host_schedule(cfg->beta0, cfg->betaT, Nd, p->alphas, p->alphas_bar, p->sigmas);
  HIP_TRY(p->stream.create());
  const int K = env->kind == ENV_CAR2D ? 1 : (env->model.n_track > 0 ? env->model.n_track : 1);
  HIP_TRY(p->d_state0.alloc(env->state_size()));
  HIP_TRY(p->d_Y0s.alloc((size_t)N * p->HNu));
  HIP_TRY(p->d_rewss.alloc((size_t)sh * H));
  HIP_TRY(p->d_rews.alloc(N));
  HIP_TRY(p->d_lp.alloc(N));
  if (cfg->enable_demo) HIP_TRY(p->d_xpos.alloc((size_t)sh * H * K * 3));
  HIP_TRY(p->d_weights.alloc(N));
  HIP_TRY(p->d_Ybar.alloc((size_t)p->HNu * 2));
  HIP_TRY(p->d_mu.alloc((size_t)(Nd - 1) * p->HNu));
  HIP_TRY(p->d_rewmeans.alloc(Nd));
  HIP_TRY(p->d_scratch.alloc((size_t)H + 8));
  HIP_TRY(p->d_wm_partial.alloc((size_t)kWmG * p->HNu));
  if (N > kLdsN) HIP_TRY(p->d_lg.alloc(N));
  // lazy candidates: the MBD update on a rigid-body env (the path-integral updates and car2d keep the materialised
  // Y0s: their kernels read it, and car2d's sampler is a few microseconds).  MBD_NO_LAZY=1: the materialised path (A/B)
  const bool no_lazy = env_flag("MBD_NO_LAZY");
  p->lazy = cfg->update_method == 0 && env->kind == ENV_MODEL && !no_lazy;
  if (p->lazy) {
    for (int b = 0; b < 3; ++b) HIP_TRY(p->ring.eps[b].alloc((size_t)N * p->HNu));
    HIP_TRY(p->ring.progress.create());
    HIP_TRY(p->d_ybar_keep.alloc(p->HNu));
  }
  if (cfg->update_method > 0) {
    const float one = 1.0f;  // path_integral.py:131
    HIP_TRY(p->d_sigma.upload(&one, 1));
    HIP_TRY(p->d_spread.alloc(p->HNu));
    HIP_TRY(p->d_idx.alloc(16));
  }
  *out = guard.release();
  return MBD_OK;
}

extern "C" int mbd_plan_destroy(mbd_plan* p) {
  if (p && p->session.in_flight) {  // (an open session ends here: its last kernel still writes the mailbox)
    (void)hipSetDevice(p->env->device);
    (void)hipStreamSynchronize(p->stream);
  }
  delete p;  // (nullptr is fine)
  return MBD_OK;
}

extern "C" int mbd_plan_schedule(const mbd_plan* p, float* alphas, float* alphas_bar, float* sigmas) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  const size_t nb = sizeof(float) * p->alphas.size();
  if (alphas) memcpy(alphas, p->alphas.data(), nb);
  if (alphas_bar) memcpy(alphas_bar, p->alphas_bar.data(), nb);
  if (sigmas) memcpy(sigmas, p->sigmas.data(), nb);
  return MBD_OK;
}

extern "C" int mbd_plan_set_state0(mbd_plan* p, const float* state0) {
  if (!p || !state0) return fail(MBD_ERR_INVALID, "NULL argument");
  NO_SESSION(p, "set_state0");
  HIP_TRY(hipSetDevice(p->env->device));
  HIP_TRY(hipMemcpy(p->d_state0, state0, sizeof(float) * p->env->state_size(), hipMemcpyHostToDevice));
  return MBD_OK;
}

// the choice of the plan's rollout launch — the one that carries the progress word and may take the noise job: the launch
// over M N candidates of a plan with an ensemble record (its first member launch when the members are launched one by one)
static RolloutChoice plan_rollout_choice(const mbd_plan* p) {
  if (p->has_ens) {
    bool one = false;
    const RolloutChoice c = ensemble_choice(p->env, p->ens_rec.n_members, p->ens_rec.members, p->cfg.Nsample, p->cfg.Hsample, &one);
    if (one) return c;
  }
  return rollout_choice(p->env, p->cfg.shard_count, p->cfg.Hsample);
}

static int ensure_aux(mbd_plan* p) {
  if (p->aux) return MBD_OK;
  HIP_TRY(p->aux.create());
  HIP_TRY(p->ev_in.create());
  HIP_TRY(p->ev_aux.create());
  for (int b = 0; b < 3; ++b) HIP_TRY(p->ring.ev_noise[b].create());
  HIP_TRY(p->ring.ev_wm.create());
  return MBD_OK;
}

// What a step's normals are made under (warm_tick: a step of the ticks t >= 1 of mbd_plan_run_mpc): the plan's noise record's, and
// under an adapt record the samplers draw under G = a * g: the record's table stands where the caller's shape stood, in every
// step — the launches that rewrite it are handed the caller's shape in force (AdaptRec::table)
static NoiseSpec noise_spec(const mbd_plan* p, bool warm_tick) {
  NoiseSpec ns = p->noise.spec(warm_tick);
  if (p->adapt.has) ns.g = p->adapt.d_G.get();
  return ns;
}

// Whether a step's candidates depend on the previous step's result — an adapt record's table, an elite record's rows —, so that
// nothing about them can be prepared ahead or reused: the noise ring declares nothing, reuses nothing, and the loops do not hold the
// host back for a second stream that has no job.
static bool follows_result(const mbd_plan* p) { return p->adapt.has || p->elite.has; }

// ---- the launches of the elite and to-go records (what a step and a tick run; the debug entries below run them on a scratch
// record) ---------------------------------------------------------------------------------------------------------------------------
// The elite record's launches for a plan (mbd_internal.h EliteRec, P = 1).  elite_table: the elites at the start of a run or a tick —
// shift < 0: count = 0, otherwise the present rows shifted `shift` elements forward.  ONE launch, a workgroup per row.
static int elite_table(EliteRec& L, int shift, int HNu, hipStream_t s) {
  if (!L.has) return MBD_OK;
  hipLaunchKernelGGL(elite_shift_kernel, dim3(L.rows), dim3(kEliteThreads), 0, s, L.d_E.get(), L.d_count.get(), HNu, shift);
  HIP_TRY(hipGetLastError());
  return MBD_OK;
}

// phase 1 of a step, behind the launch that made the step's normals or candidates, in front of the rollout: c.cand's first rows
// are rewritten; g is the shape the step's sampler was handed.  ONE launch.
static int elite_inject(EliteRec& L, const StepCand& c, const float* g, hipStream_t s) {
  if (!L.has) return MBD_OK;
  EliteInject A{};
  A.cand = const_cast<float*>(c.cand);  // (the one launch that writes a step's candidates behind their sampler)
  A.HNu = c.HNu; A.ybar_i = c.ybar_i; A.lazy = c.lazy; A.sigma = c.sigma; A.g = g;
  A.n_elites = L.n; A.nominal = L.nominal; A.E = L.d_E; A.count = L.d_count;
  const long long total = (long long)(L.nominal + L.n) * c.HNu;
  hipLaunchKernelGGL(elite_inject_kernel, dim3((unsigned)((total + kEliteThreads - 1) / kEliteThreads)), dim3(kEliteThreads), 0, s, A);
  HIP_TRY(hipGetLastError());
  return MBD_OK;
}

// phase 2 of a step, behind the step's update kernel (and an adapt record's launches): the selection over the rewards the score
// read, and the log entry.  ONE launch.
static int elite_select(EliteRec& L, const float* d_rews, const StepCand& c, hipStream_t s) {
  if (!L.has) return MBD_OK;
  const long long slot = ring_slot(L.steps[0], L.log_cap);
  EliteSelect A{};
  A.rews = d_rews; A.N = c.N; A.HNu = c.HNu; A.cand = c.cand; A.lazy = c.lazy; A.sigma = c.sigma; A.ybar_i = c.ybar_i;
  A.n_elites = L.n; A.nominal = L.nominal; A.E = L.d_E; A.R = L.d_R; A.src = L.d_src; A.count = L.d_count;
  A.log_count = L.d_log_count.get() + slot; A.log_kept = L.d_log_kept.get() + slot; A.log_top = L.d_log_top.get() + slot;
  hipLaunchKernelGGL(elite_select_kernel, dim3(1), dim3(kScoreThreads), 0, s, A);
  HIP_TRY(hipGetLastError());
  return MBD_OK;
}

// A step's two launches of a plan's to-go record, where the fused score and weighted mean stand without a record: A carries everything
// but the layout and the record's buffers.  Groups 0 .. G - 2 hold block Nu elements in tpg tiles each, the last group the rest.
static int togo_launch(TogoRec& L, const float* d_rewss, TogoUpdate A, hipStream_t s) {
  const int block = L.block, G = L.G;
  const TogoReturns Rt{A.rews, d_rewss, L.d_R.get(), A.N, A.H, block, G};
  hipLaunchKernelGGL(togo_returns_kernel, dim3((A.N + kTogoThreads - 1) / kTogoThreads), dim3(kTogoThreads), 0, s, Rt);
  HIP_TRY(hipGetLastError());
  const long long last = (long long)(A.H - togo_start(G - 1, block)) * A.Nu;
  A.R = L.d_R; A.W = L.d_W; A.G = G; A.block = block;
  A.tpg = G > 1 ? (int)(((long long)block * A.Nu + kWmE - 1) / kWmE) : 1;
  A.T = (G - 1) * A.tpg + (int)((last + kWmE - 1) / kWmE);
  hipLaunchKernelGGL(togo_update_kernel, dim3(A.T), dim3(kWmE * kWmG), sizeof(float) * (size_t)A.N, s, A);
  HIP_TRY(hipGetLastError());
  L.stepped = true;
  return MBD_OK;
}

// z [N][HNu] of a step into `out`: noise_kernel, or under a basis knot_noise_kernel
static void launch_noise(mbd_plan* p, hipStream_t st, const uint32_t key[2], float* out, const NoiseSpec& ns) {
  const mbd_plan_config& c = p->cfg;
  if (ns.W) {
    hipLaunchKernelGGL(knot_noise_kernel, dim3(knot_blocks(c.Nsample, p->Nu, 65536)), dim3(kKnotThreads), 0, st, key[0], key[1],
                       c.prng_impl, c.Nsample, c.Hsample, p->Nu, ns.knots, ns.W, ns.g, out);
    return;
  }
  const unsigned blocks = noise_blocks(c.prng_impl, (uint64_t)c.Nsample * p->HNu, 65536);
  hipLaunchKernelGGL(noise_kernel, dim3(blocks), dim3(256), 0, st, key[0], key[1], c.prng_impl, c.Nsample, p->HNu, out, ns.g);
}

// The normals of a diffusion step depend on its key only, not on the previous step's result.  This call DECLARES the
// key of the step AFTER the next mbd_plan_sample_rollout: that launch then also generates the declared step's normals —
// in spare workgroups of the rollout launch itself when the rollout leaves CUs idle (up to three quarters of the CUs:
// ~3000 humanoid candidates; no extra launch, no event), on the plan's second stream otherwise — so that the declared
// step starts without a sampler on its critical path.  A hint: a step whose normals were not prepared (no declaration,
// another key, a non-lazy plan) generates them on the spot; results are bit-identical either way.
// (ns: the noise shape and basis the declared step samples under — a warm tick's first step is declared beside tick 0's last
// rollout.  Under a basis the job is knot_noise_kernel's and always goes to the second stream: prepare_noise_job)
static int declare_next_key(mbd_plan* p, const uint32_t key_next[2], const NoiseSpec& ns) {
  const bool off = env_flag("MBD_NO_PREFETCH");
  // (under an adapt or an elite record a step's normals depend on the previous step's result: nothing is declared, every step makes
  // its own)
  if (off || !p->lazy || follows_result(p)) return MBD_OK;
  p->ring.hint_key[0] = key_next[0];
  p->ring.hint_key[1] = key_next[1];
  p->ring.hint_ns = ns;
  p->ring.hint_valid = true;
  return MBD_OK;
}
extern "C" int mbd_plan_prefetch_noise(mbd_plan* p, const uint32_t key_next[2], void* stream_) {
  (void)stream_;
  if (!p || !key_next) return fail(MBD_ERR_INVALID, "NULL argument");
  return declare_next_key(p, key_next, noise_spec(p, false));
}

// A plan's phases depend on each other through its buffers (the normals one step's launch prepares are read by the
// next; phase 2 reads what phase 1 wrote): stream order covers that while the caller stays on one stream; when a call
// arrives on another stream it is ordered behind the previous call with an event.
static int plan_enter(mbd_plan* p, hipStream_t s) {
  if (p->last_stream_set && p->last_stream != s) {
    if (!p->ev_xs) HIP_TRY(p->ev_xs.create());
    HIP_TRY(hipEventRecord(p->ev_xs, p->last_stream));
    HIP_TRY(hipStreamWaitEvent(s, p->ev_xs, 0));
  }
  p->last_stream = s;
  p->last_stream_set = true;
  return MBD_OK;
}

// Step 1 of phase 1, lazy: every rank holds the normals of ALL N candidates (counter-based noise), so that phase 2 needs no
// second collective and is bit-identical for every shard layout; the candidates themselves are formed at the rollout's
// action fetch and inside the weighted mean.  The step's normals: ring.cur afterwards.
static int obtain_normals(mbd_plan* p, const uint32_t key_sample[2], const NoiseSpec& ns, hipStream_t s) {
  NoiseRing& ring = p->ring;
  // (under an adapt record the table behind ns.g changes from step to step, under an elite record rows of the buffer are rewritten
  // behind the sampler: a buffer's tag says nothing, nothing is reused)
  int cur = follows_result(p) ? -1 : ring.find(key_sample, ns);
  if (cur >= 0) {  // prepared behind the previous rollout
    MBD_TRY(ring.join(cur, s));
  } else {  // not prepared: generate now, into the buffer behind the previous step's (stream order protects it)
    cur = (ring.cur + 1) % 3;
    MBD_TRY(ring.join(cur, s));  // (a stale prefetch may still be writing it)
    launch_noise(p, s, key_sample, ring.eps[cur], ns);
    HIP_TRY(hipGetLastError());
    ring.holds(cur, key_sample, ns);
  }
  ring.cur = cur;
  return MBD_OK;
}

// Step 1, materialised (car2d, path-integral updates): every rank samples ALL N candidate sequences.  A sharded plan
// samples its own rows first and the others' on a second stream, behind the rollout; mbd_plan_score_update joins
// that stream before it reads them.  Under a noise basis: knot_noise_kernel into the plan's scratch z, then shift_kernel —
// sample_kernel's two roundings — over the whole tensor on the caller's stream, sharded or not.
static int sample_candidates(mbd_plan* p, int i, const uint32_t key_sample[2], const float* d_Ybar_i, const NoiseSpec& ns,
                             hipStream_t s) {
  const mbd_plan_config& c = p->cfg;
  const int N = c.Nsample, HNu = p->HNu;
  const uint64_t total = (uint64_t)N * HNu;
  const float* g = ns.g;
  if (ns.W) {
    launch_noise(p, s, key_sample, p->noise.d_knot_z, ns);
    hipLaunchKernelGGL(shift_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const float*)p->noise.d_knot_z, HNu, 0ull,
                       (unsigned long long)total, p->sigmas[i],
                       c.update_method > 0 ? (const float*)p->d_sigma : (const float*)nullptr, d_Ybar_i, p->d_Y0s.get());
    HIP_TRY(hipGetLastError());
    return MBD_OK;
  }
  auto sample = [&](hipStream_t st, uint64_t e0, uint64_t cnt) {
    if (cnt == 0) return;
    const bool pair_blocks = c.prng_impl != MBD_PRNG_PARTITIONABLE && e0 == 0 && cnt == total;
    const uint64_t threads = pair_blocks ? (total + 1) / 2 : cnt;
    hipLaunchKernelGGL(sample_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, key_sample[0],
                       key_sample[1], c.prng_impl, N, HNu, (unsigned long long)e0, (unsigned long long)cnt,
                       p->sigmas[i], c.update_method > 0 ? (const float*)p->d_sigma : (const float*)nullptr,
                       d_Ybar_i, p->d_Y0s, g);
  };
  const uint64_t own0 = (uint64_t)c.shard_begin * HNu, own1 = own0 + (uint64_t)c.shard_count * HNu;
  const bool no_aux = env_flag("MBD_NO_AUX");
  if (c.shard_count == N || no_aux || (long long)N < 5LL * c.shard_count) {
    // worth the two events only when the other ranks' rows dominate (tools/gpu_rank_emu.sh: 8 shards 0.774 ->
    // 0.762 ms per step, 2 shards 0.736 -> 0.742); MBD_NO_AUX=1 keeps everything on the caller's stream (A/B)
    sample(s, 0, total);
  } else {
    MBD_TRY(ensure_aux(p));
    HIP_TRY(hipEventRecord(p->ev_in, s));  // Ybar_i is final and the previous step is done with Y0s
    HIP_TRY(hipStreamWaitEvent(p->aux, p->ev_in, 0));
    sample(s, own0, own1 - own0);
    sample(p->aux, 0, own0);
    sample(p->aux, own1, total - own1);
    HIP_TRY(hipEventRecord(p->ev_aux, p->aux));
    p->aux_pending = true;
  }
  HIP_TRY(hipGetLastError());
  return MBD_OK;
}

// Step 2, lazy: whether the coming rollout launch carries a noise job for the NEXT step — lz.nz_*, nz_out null: none — and
// the job's buffer, the one behind ring.cur, made ready for it; *marked: see NoiseRing::mark_last_reader.
static int prepare_noise_job(mbd_plan* p, const uint32_t key_sample[2], hipStream_t s, LazyArgs& lz, bool* marked) {
  const mbd_plan_config& c = p->cfg;
  NoiseRing& ring = p->ring;
  const int nxt = (ring.cur + 1) % 3;
  // Preparing the next step's normals ahead only pays for a plan that has the device to itself (the caller says so:
  // mbd_plan_config.shares_device): beside other plans
  // (seed / temperature sweeps as concurrent plans, scripts/run_mbd.py) the noise workgroups would hold — through
  // the launch's LDS reservation — the CUs the other plans' rollouts need, and a second stream per plan runs the
  // process out of hardware queues (four N=1024 plans: 3100 plan-steps/s either way against 6200 with the normals
  // generated in front of each rollout, where the other plans' rollouts hide them anyway).
  const bool alone = c.shares_device == 0;
  uint32_t declared[2];
  NoiseSpec declared_ns;
  const bool want = ring.take_hint(key_sample, declared, &declared_ns) && alone;
  if (!want) return MBD_OK;
  // eps[nxt] was last read two steps ago
  MBD_TRY(ring.join(nxt, s));  // (a stale prefetch of another key: let it finish before it is overwritten)
  ring.valid[nxt] = false;
  lz.nz_out = ring.eps[nxt];
  lz.nz_g = declared_ns.g; lz.nz_W = declared_ns.W; lz.nz_knots = declared_ns.knots;
  lz.nz_key[0] = declared[0]; lz.nz_key[1] = declared[1];
  lz.nz_impl = c.prng_impl; lz.nz_N = c.Nsample; lz.nz_HNu = p->HNu;
  // (launches that take the job into spare workgroups need no second stream and none of its events: a record
  // behind every weighted mean idles the queue ~5.5 us, 1 % of a step — profiles/r02_timeline.txt)
  // (asked of the launch's own decision: a one-workgroup shard of a large plan pins its rollout and still cannot take
  // the job — its normals then need the second stream's ordering like a full-chip launch's; and so does every job under a
  // noise basis, which no rollout launch takes)
  if (!declared_ns.W && rollout_takes_noise(plan_rollout_choice(p), c.prng_impl, c.Nsample, p->HNu)) return MBD_OK;
  MBD_TRY(ensure_aux(p));
  return ring.mark_last_reader(nxt, s, marked);
}

// Step 4, lazy: the job behind the launch.  One the launch did not take (the rollout fills the chip) runs on the second
// stream, beside the rollout; either way eps[nxt] holds the declared step's normals from here on.
static int finish_noise_job(mbd_plan* p, const LazyArgs& lz, bool marked) {
  if (!lz.nz_out) return MBD_OK;
  NoiseRing& ring = p->ring;
  const int nxt = (ring.cur + 1) % 3;
  NoiseSpec ns;
  ns.g = lz.nz_g; ns.W = lz.nz_W; ns.knots = lz.nz_knots;
  if (!lz.nz_fused) {
    MBD_TRY(ensure_aux(p));
    MBD_TRY(ring.aux_waits_for_mark(p->aux, marked));
    launch_noise(p, p->aux, lz.nz_key, lz.nz_out, ns);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ring.ev_noise[nxt], p->aux));
    ring.on_aux[nxt] = true;
  }
  ring.holds(nxt, lz.nz_key, ns);
  return MBD_OK;
}

// phase 1 of a step, from d_state0: the plan's own start state (mbd_plan_sample_rollout), or an episode's executed state;
// ns: the noise shape and basis the step samples under
// d_xref: the demo table the step's log-densities are taken against, nullptr: the env's own (a tick's window: DemoRec)
static int plan_sample_rollout(mbd_plan* p, int i, const uint32_t key_sample[2], const float* d_Ybar_i, float* d_rews_local,
                               float* d_logpd_local, hipStream_t s, const float* d_state0, const NoiseSpec& ns,
                               const float* d_xref = nullptr) {
  if (!p || !key_sample || !d_Ybar_i || !d_rews_local) return fail(MBD_ERR_INVALID, "NULL argument");
  const mbd_plan_config& c = p->cfg;
  if (i < 1 || i >= c.Ndiffuse) return fail(MBD_ERR_INVALID, "diffusion index %d outside [1,%d)", i, c.Ndiffuse);
  if (c.enable_demo && !d_logpd_local) return fail(MBD_ERR_INVALID, "enable_demo needs d_logpd_local");
  mbd_env* e = p->env;
  HIP_TRY(hipSetDevice(e->device));
  MBD_TRY(plan_enter(p, s));
  const int N = c.Nsample, H = c.Hsample, HNu = p->HNu;
  NoiseRing& ring = p->ring;
  LazyArgs lz;
  bool marked = false;
  // A1: this step's normals, then the next step's noise job; or this step's candidates
  if (p->lazy) {
    MBD_TRY(obtain_normals(p, key_sample, ns, s));
    p->peek_ybar = d_Ybar_i;  // (the caller keeps it unchanged until phase 2 has run)
    p->sigma_last = p->sigmas[i];
    lz.ybar = d_Ybar_i;
    lz.sigma = p->sigmas[i];
    MBD_TRY(prepare_noise_job(p, key_sample, s, lz, &marked));
  } else {
    MBD_TRY(sample_candidates(p, i, key_sample, d_Ybar_i, ns, s));
  }
  // The elite record: ONE launch between the sampler and the rollout rewrites the first rows — the step's mean, the elites the
  // previous step left; ns.g is the shape the step's sampler was handed.  The buffer of a lazy plan no longer holds what its tag
  // says: the ring forgets it.
  const float* d_cand = p->lazy ? ring.eps[ring.cur] : p->d_Y0s;
  if (p->elite.has) {
    if (p->lazy) ring.valid[ring.cur] = false;
    MBD_TRY(elite_inject(p->elite, StepCand{d_cand, N, HNu, p->lazy ? 1 : 0, p->sigmas[i], nullptr, d_Ybar_i}, ns.g, s));
  }
  // A2/A3: rollout of the local shard
  MBD_TRY(p->timing.begin(s));
  if (p->lazy) {
    lz.progress = ring.progress;
    lz.progress_val = ++ring.seq;
    ring.read_seq[ring.cur] = ring.seq;
  }
  // A5: the demo log-densities of the local shard come out of the rollout itself where its instantiation accumulates them
  // (round 6: no [shard][H][K][3] round trip, no second launch); otherwise from the tracked positions, below
  const bool fused_lp = c.enable_demo && rollout_choice(e, c.shard_count, H).fuses_logpd;
  if (p->has_ens) {
    // the ensemble (include/mbd_hip.h mbd_ensemble): the N candidates on every member, then the members' rewards combined
    // into the caller's buffer — phase 2 is handed those and is unchanged.  (unsharded, no demo: the set call's refusals)
    const EnsArgs ea{p->ens_rec.n_members, p->ens_rec.members};
    MBD_TRY(launch_rollout(e, d_state0, d_cand, N, H, p->d_ens_rewss, p->d_ens_rews, nullptr, nullptr, s,
                           p->lazy ? &lz : nullptr, nullptr, nullptr, &ea));
    // the objective over the M N rows, candidate b % N: each member's return is the shaped one, the combination is unchanged
    if (p->obj.has)
      MBD_TRY(p->obj.launch(p->d_ens_rewss, p->d_ens_rews, p->ens_rec.n_members * N, 0, d_cand, p->lazy, p->sigmas[i], d_Ybar_i, -1, s));
    hipLaunchKernelGGL(ensemble_reduce_kernel, dim3((N + 255) / 256), dim3(256), 0, s, (const float*)p->d_ens_rews,
                       p->ens_rec.n_members, N, p->ens_rec.risk, d_rews_local, p->d_ens_comb);
    HIP_TRY(hipGetLastError());
    p->ens_stepped = true;
  } else {
    MBD_TRY(launch_rollout(e, d_state0, d_cand + (size_t)c.shard_begin * HNu, c.shard_count, H, p->d_rewss, d_rews_local,
                           (c.enable_demo && !fused_lp) ? p->d_xpos.get() : p->zone.xpos(), p->val.final(), s,
                           p->lazy ? &lz : nullptr, nullptr, fused_lp ? d_logpd_local : nullptr, nullptr, d_xref));
  }
  MBD_TRY(p->timing.end(s));
  // The objective record: ONE launch between the rollout and the score rewrites the shard's rewards in place (a path-integral plan
  // samples under its carried sigma, but its candidates are materialised: d_Y0s holds the values).  The noise ring's bookkeeping
  // needs no change: the launch reads eps[cur] on the step's stream between the rollout and the weighted mean, and the weighted
  // mean is already marked as the buffer's last reader.
  if (p->obj.has && !p->has_ens)
    MBD_TRY(p->obj.launch(p->d_rewss, d_rews_local, c.shard_count, c.shard_begin, d_cand, p->lazy, p->sigmas[i], d_Ybar_i, -1, s));
  // The zone record: ONE launch behind the objective's subtracts the penalty of the tracked positions the rollout above wrote
  // (never under an ensemble, a demo or a shard: the set calls refuse them)
  MBD_TRY(p->zone.launch_step(d_rews_local, c.shard_count, s));
  // The value record: ONE launch behind the zones' adds scale * V of the shard's final states, which the rollout above wrote
  // (never under an ensemble: the set calls refuse the pair)
  MBD_TRY(p->val.launch_step(d_rews_local, c.shard_count, s));
  MBD_TRY(finish_noise_job(p, lz, marked));
  if (c.enable_demo && !fused_lp) MBD_TRY(launch_logpd(e, p->d_xpos, c.shard_count, H, d_logpd_local, s, d_xref));
  return MBD_OK;
}

extern "C" int mbd_plan_sample_rollout(mbd_plan* p, int i, const uint32_t key_sample[2], const float* d_Ybar_i,
                                       float* d_rews_local, float* d_logpd_local, void* stream_) {
  if (p) NO_SESSION(p, "sample_rollout");
  return plan_sample_rollout(p, i, key_sample, d_Ybar_i, d_rews_local, d_logpd_local, (hipStream_t)stream_,
                             p ? p->d_state0.get() : nullptr, p ? noise_spec(p, false) : NoiseSpec{});
}

// phase 2 of a step; rew_xref: the demo's reward level in the blend — the env's (mbd_plan_score_update), or an episode's
// demo record's
static int plan_score_update(mbd_plan* p, int i, const float* d_Ybar_i, const float* d_rews_all, const float* d_logpd_all,
                             float* d_Ybar_im1, float* d_rew_mean, void* stream_, float rew_xref) {
  if (!p || !d_Ybar_i || !d_rews_all || !d_Ybar_im1 || !d_rew_mean) return fail(MBD_ERR_INVALID, "NULL argument");
  const mbd_plan_config& c = p->cfg;
  if (i < 1 || i >= c.Ndiffuse) return fail(MBD_ERR_INVALID, "diffusion index %d outside [1,%d)", i, c.Ndiffuse);
  if (c.enable_demo && !d_logpd_all) return fail(MBD_ERR_INVALID, "enable_demo needs d_logpd_all");
  HIP_TRY(hipSetDevice(p->env->device));
  hipStream_t s = (hipStream_t)stream_;
  MBD_TRY(plan_enter(p, s));
  const int N = c.Nsample, HNu = p->HNu;
  if (p->aux_pending) {  // the other ranks' rows of Y0s (sampled behind the rollout)
    HIP_TRY(hipStreamWaitEvent(s, p->ev_aux, 0));
    p->aux_pending = false;
  }
  const size_t lds_n = N > kLdsN ? 0 : sizeof(float) * (size_t)N;
  // While the N weights fit the default 48 KB LDS window (12 288 candidates) score and weighted mean are ONE launch
  // (score_wmean_kernel: every workgroup re-derives the weights — same bits); beyond, score_kernel and the row-major
  // two-kernel weighted mean (same bits again: see wmean_partial_kernel).  One launch beats three even where the
  // row-major reads are faster (N = 4096: +0.8 % of a step, N = 8192: +0.3 %).  MBD_WMEAN_SPLIT=0/1,
  // MBD_NO_FUSED_SCORE=1 force the variants (A/B, tests).
  const int split_env = lever("MBD_WMEAN_SPLIT");
  const bool split = split_env >= 0 ? split_env != 0 : (size_t)N * sizeof(float) > 48 * 1024;
  const bool no_fused_score = env_flag("MBD_NO_FUSED_SCORE");
  // under a weighting record the weigh kernel stands where score_kernel stands and the step takes the kernels that consume given
  // weights, the ones MBD_NO_FUSED_SCORE=1 selects
  const bool fused_score = !split && c.update_method != 3 && (size_t)N * sizeof(float) <= 48 * 1024 && !no_fused_score && !p->wt.has;
  if (p->wt.has) {
    hipLaunchKernelGGL(weigh_kernel, dim3(1), dim3(kScoreThreads), lds_n, s, d_rews_all, N, c.temp_sample, p->wt.rec,
                       p->d_weights.get(), d_rew_mean, p->d_lg.get(), p->wt.slot(), PiBatch{});
    HIP_TRY(hipGetLastError());
  } else if (!fused_score) {
    hipLaunchKernelGGL(score_kernel, dim3(1), dim3(kScoreThreads), lds_n, s, d_rews_all,
                       c.enable_demo ? d_logpd_all : nullptr, N, rew_xref, c.temp_sample,
                       c.update_method == 0 ? 1 : 0, p->d_weights, d_rew_mean, p->d_lg, PiBatch{});
    HIP_TRY(hipGetLastError());
  }
  const dim3 ge((HNu + 63) / 64), b64(64);
  const float* d_cand = p->lazy ? p->ring.eps[p->ring.cur] : p->d_Y0s;
  const int lazy = p->lazy ? 1 : 0;
  const float sigma_i = p->sigmas[i];
  if (c.update_method == 3) {  // cem_update (path_integral.py:48-52)
    const int K = N < 10 ? N : 10;
    hipLaunchKernelGGL(cem_select_kernel, dim3(1), b64, lds_n, s, p->d_weights, N, K, p->d_idx, p->d_lg, PiBatch{});
    hipLaunchKernelGGL(cem_mean_kernel, ge, b64, 0, s, p->d_idx, K, p->d_Y0s, HNu, d_Ybar_im1, PiBatch{});
  } else {  // MBD (:128-133), mppi (:33-36), cma-es (:39-45)
    const int lit = c.update_method == 0 ? c.literal_score : 0;
    if (p->togo.has) {
      // The to-go record: TWO launches stand where the fused launch stands — the groups' returns from the rewards per step the
      // step's rollout left in d_rewss, then score and weighted mean per group (mbd_step_kernels.h togo_update_kernel)
      TogoUpdate A{};
      A.rews = d_rews_all; A.weights = p->d_weights; A.rew_mean = d_rew_mean; A.cand = d_cand; A.ybar_i = d_Ybar_i;
      A.ybar_im1 = d_Ybar_im1; A.ybar_keep = p->d_ybar_keep; A.N = N; A.H = c.Hsample; A.Nu = p->Nu; A.temp = c.temp_sample;
      A.std_guard = c.update_method == 0 ? 1 : 0; A.alpha_i = p->alphas[i]; A.alpha_bar_i = p->alphas_bar[i];
      A.alpha_bar_im1 = p->alphas_bar[i - 1]; A.literal = lit; A.lazy = lazy; A.sigma = sigma_i;
      MBD_TRY(togo_launch(p->togo, p->d_rewss, A, s));
    } else if (fused_score) {
      // XCD pinning (mbd_step_kernels.h pinned_tile): the T tiles on the fewest XCDs X in {1, 2, 4, 8} that give every tile
      // a CU of its own (32 per XCD) and keep an XCD's share of the candidates' rows within its 4 MB L2; the launch is
      // 8 ceil(T / X) workgroups long, those of the other XCDs leave at once.  MBD_WMEAN_XCDS = 1 / 2 / 4 / 8 forces X.
      // outputs per thread: one (two measured slower at every size and no lighter: mbd_step_kernels.h).  MBD_WMEAN_V1 = 2 forces two.
      const int V = lever("MBD_WMEAN_V1") == 2 ? 2 : 1;
      const int T = (HNu + kWmE * V - 1) / (kWmE * V);
      int X = 1;
      while (X < 8 && ((T + X - 1) / X > 32 || (size_t)N * HNu * sizeof(float) / X > (size_t)4 << 20)) X *= 2;
      if (!device_has_eight_xcds(p->env)) X = 8;  // (a partition or another part: the plain launch, no empty workgroups)
      const int x_env = lever("MBD_WMEAN_XCDS");
      if (x_env == 1 || x_env == 2 || x_env == 4 || x_env == 8) X = x_env;
      auto kern = V == 2 ? score_wmean_kernel<2> : score_wmean_kernel<1>;
      hipLaunchKernelGGL(kern, dim3(8 * ((T + X - 1) / X)), dim3(kWmE * kWmG), sizeof(float) * (size_t)N,
                         s, d_rews_all, c.enable_demo ? d_logpd_all : nullptr, N, rew_xref, c.temp_sample,
                         c.update_method == 0 ? 1 : 0, p->d_weights, d_rew_mean, d_cand, HNu, d_Ybar_i, p->alphas[i],
                         p->alphas_bar[i], p->alphas_bar[i - 1], lit, d_Ybar_im1, lazy, sigma_i, p->d_ybar_keep, T, X);
    } else if (split) {
      hipLaunchKernelGGL(wmean_partial_kernel, dim3((HNu + kWmT - 1) / kWmT, kWmG), dim3(kWmT), 0, s, p->d_weights,
                         d_cand, N, HNu, p->d_wm_partial, lazy, sigma_i, d_Ybar_i);
      hipLaunchKernelGGL(wmean_finish_kernel, dim3((HNu + 63) / 64), dim3(64), 0, s, p->d_wm_partial, HNu, d_Ybar_i,
                         p->alphas[i], p->alphas_bar[i], p->alphas_bar[i - 1], lit, d_Ybar_im1, p->d_ybar_keep);
    } else {
      hipLaunchKernelGGL(wmean_kernel, dim3((HNu + kWmE - 1) / kWmE), dim3(kWmE * kWmG), sizeof(float) * (size_t)N, s,
                         p->d_weights, d_cand, N, HNu, d_Ybar_i, p->alphas[i], p->alphas_bar[i],
                         p->alphas_bar[i - 1], lit, d_Ybar_im1, lazy, sigma_i, p->d_ybar_keep);
    }
    if (c.update_method == 2) {
      hipLaunchKernelGGL(cma_spread_kernel, ge, b64, 0, s, p->d_weights, p->d_Y0s, N, HNu, d_Ybar_i, p->d_spread, PiBatch{});
      hipLaunchKernelGGL(cma_sigma_kernel, dim3(1), b64, 0, s, p->d_spread, HNu, p->d_sigma, PiBatch{});
    }
  }
  HIP_TRY(hipGetLastError());
  // The adapt record: TWO launches behind the update kernel rewrite the table the next step samples under, from the weights, the
  // candidates (eps[cur] of a lazy plan: read here in front of the ring's mark, so the weighted mean's argument covers them) and the
  // Ybar_i the caller has not yet moved on from — with the sigma the step sampled with, an mppi plan's from the carried device scalar
  const StepCand sc{d_cand, N, HNu, lazy, sigma_i, c.update_method > 0 ? p->d_sigma.get() : nullptr, d_Ybar_i};
  if (p->adapt.has) MBD_TRY(p->adapt.update(p->d_weights, sc, s));
  // The elite record: ONE launch in the same place takes the step's best candidates over — from the rewards the score read, the
  // candidates (eps[cur]: in front of the ring's mark as well) and Ybar_i
  if (p->elite.has) MBD_TRY(elite_select(p->elite, d_rews_all, sc, s));
  if (p->lazy) {
    p->peek_ybar = p->d_ybar_keep;
    MBD_TRY(p->ring.mark_wmean(s, p->aux != nullptr));
  }
  return MBD_OK;
}

extern "C" int mbd_plan_score_update(mbd_plan* p, int i, const uint32_t key_sample[2], const float* d_Ybar_i,
                                     const float* d_rews_all, const float* d_logpd_all, float* d_Ybar_im1,
                                     float* d_rew_mean, void* stream_) {
  (void)key_sample;  // the candidates (or their normals) of all N are already resident from phase 1 of this step
  if (p) NO_SESSION(p, "score_update");
  if (p) p->wt.begin();
  return plan_score_update(p, i, d_Ybar_i, d_rews_all, d_logpd_all, d_Ybar_im1, d_rew_mean, stream_, p ? p->env->rew_xref : 0.0f);
}

extern "C" int mbd_plan_set_sigma(mbd_plan* p, float sigma) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  if (!p->d_sigma) return fail(MBD_ERR_STATE, "not a path-integral plan (update_method == 0)");
  HIP_TRY(hipSetDevice(p->env->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(p->d_sigma, &sigma, sizeof(float), hipMemcpyHostToDevice));
  return MBD_OK;
}
extern "C" int mbd_plan_get_sigma(mbd_plan* p, float* sigma_out) {
  if (!p || !sigma_out) return fail(MBD_ERR_INVALID, "NULL argument");
  if (!p->d_sigma) return fail(MBD_ERR_STATE, "not a path-integral plan (update_method == 0)");
  HIP_TRY(hipSetDevice(p->env->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(p->d_sigma.download(sigma_out, 1));
  return MBD_OK;
}

// ---- the records' entries (the noise records' here, the others' behind mbd_plan_run): the plan's refusals in their order, then the
// record's own set or peek (mbd_records.hip) ----------------------------------------------------------------------------------------
extern "C" int mbd_plan_set_noise_shape(mbd_plan* p, const mbd_noise_shape* rec) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  NO_SESSION(p, "set_noise_shape");
  if (rec) MBD_TRY(check_noise_shape(rec, p->cfg.Hsample, p->Nu));
  // Normals prepared ahead were scaled under the previous setting, and the table behind the pointer that tags them is about to
  // change: the ring forgets them and the declared key, so the next step generates its own under the new setting.
  p->ring.forget();
  MBD_TRY(p->noise.set_shape(rec, p->HNu, p->env->device));
  // an adapt record's G = a * g is formed again under the shape now in force outside warm ticks (a run and a tick form their own)
  MBD_TRY(p->adapt.table(0, p->noise.shape_always(), p->HNu, p->stream));
  if (p->adapt.has) HIP_TRY(hipStreamSynchronize(p->stream));
  return MBD_OK;
}

// include/mbd_hip_debug.h: the shaped normals z = normal(key, (N, HNu)) * g of noise_fill's two index widths, on `blocks`
// workgroups of 256 threads (fewer than the thread-items: the loops stride)
extern "C" int mbd_debug_noise_shaped(const uint32_t key[2], int impl, int N, int HNu, const float* g, int wide, int blocks,
                                      float* z_out) {
  if (!key || !g || !z_out) return fail(MBD_ERR_INVALID, "NULL argument");
  if (N < 1 || HNu < 1 || blocks < 1 || blocks > 65536 || (uint64_t)N * (uint64_t)HNu > (1ull << 26))
    return fail(MBD_ERR_INVALID, "noise_shaped: N=%d HNu=%d blocks=%d", N, HNu, blocks);
  if (device_count_quiet() < 1) return fail(MBD_ERR_NO_DEVICE, "no HIP device: this library has no CPU fallback");
  const size_t n = (size_t)N * HNu;
  DevBuf<float> d_g, d_z;
  HIP_TRY(d_g.upload(g, HNu));
  HIP_TRY(d_z.alloc_poisoned(n));  // (an element left unwritten reads back as NaN)
  hipLaunchKernelGGL(noise_shaped_probe_kernel, dim3((unsigned)blocks), dim3(256), 0, nullptr, key[0], key[1], impl, N, HNu, d_z.get(),
                     (const float*)d_g, wide);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(d_z.download(z_out, n));
  return MBD_OK;
}

extern "C" int mbd_plan_set_noise_basis(mbd_plan* p, const mbd_noise_basis* rec) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  NO_SESSION(p, "set_noise_basis");
  if (rec) MBD_TRY(check_noise_basis(rec, p->cfg.Hsample));
  p->ring.forget();  // (as mbd_plan_set_noise_shape: nothing prepared under the previous setting survives)
  // (materialised plans alone run knot_noise_kernel into the scratch z [N][HNu])
  return p->noise.set_basis(rec, p->cfg.Hsample, p->lazy ? 0 : (size_t)p->cfg.Nsample * p->HNu, p->env->device);
}

// include/mbd_hip_debug.h: knot_noise_kernel alone, on `blocks` workgroups of kKnotThreads threads
extern "C" int mbd_debug_knot_noise(const uint32_t key[2], int impl, int N, int H, int Nu, int n_knots, const float* W,
                                    const float* g, int blocks, float* z_out) {
  if (!key || !W || !z_out) return fail(MBD_ERR_INVALID, "NULL argument");
  if (N < 1 || H < 1 || Nu < 1 || n_knots < 1 || n_knots > MBD_MAX_KNOTS || blocks < 1 || blocks > 65536 ||
      (uint64_t)N * (uint64_t)H * (uint64_t)Nu > (1ull << 26))
    return fail(MBD_ERR_INVALID, "knot_noise: N=%d H=%d Nu=%d n_knots=%d blocks=%d", N, H, Nu, n_knots, blocks);
  if (device_count_quiet() < 1) return fail(MBD_ERR_NO_DEVICE, "no HIP device: this library has no CPU fallback");
  const size_t HNu = (size_t)H * Nu, n = (size_t)N * HNu;
  DevBuf<float> d_W, d_g, d_z;
  HIP_TRY(d_W.upload(W, (size_t)H * n_knots));
  if (g) HIP_TRY(d_g.upload(g, HNu));  // (without: d_g stays nullptr)
  HIP_TRY(d_z.alloc_poisoned(n));      // (an element left unwritten reads back as NaN)
  hipLaunchKernelGGL(knot_noise_kernel, dim3((unsigned)blocks), dim3(kKnotThreads), 0, nullptr, key[0], key[1], impl, N, H, Nu, n_knots,
                     (const float*)d_W, (const float*)d_g, d_z.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(d_z.download(z_out, n));
  return MBD_OK;
}

// Loops that enqueue step after step (mbd_plan_run): a plan whose next step's normals are generated on the second stream
// stays ONE step behind the device — it enqueues step q once the rollout of step q-1 has started (the queue still holds
// that rollout and its score: the device never waits for the host) — so that sample_rollout finds the progress word where
// it needs it and the step's stream carries no event (NoiseRing: the ring of three buffers).
static int plan_keep_in_step(mbd_plan* p) {
  NoiseRing& ring = p->ring;
  if (!p->lazy || !ring.progress || ring.seq == 0 || p->cfg.shares_device != 0 || follows_result(p)) return MBD_OK;
  // (a plan with a noise basis prepares its normals on the second stream whatever the launch could take)
  if (!p->noise.has_basis && rollout_takes_noise(plan_rollout_choice(p), p->cfg.prng_impl, p->cfg.Nsample, p->HNu)) return MBD_OK;
  // (a stream slower than the limit: the loop stops keeping step and the step orders the two streams with an event instead —
  // NoiseRing::mark_last_reader's own bounded wait, then a mark on the step's stream for the aux stream)
  ring.kept_in_step = progress_wait(ring.progress, ring.seq, kInStepWaitMs, 20);
  return MBD_OK;
}

// d_state0: where the step's rollouts start.  key_after: the Y0s_rng of the step that follows the LAST step (i == 1) of
// this loop in another one (a receding-horizon episode's next tick), or nullptr.  ns: the noise shape and basis this loop's
// steps sample under, ns_after: what key_after's step does.  d_xref: the demo table of the step, nullptr: the env's with the
// env's rew_xref (a tick of an episode with a demo record: its window and the record's rew_xref)
static int reverse_once_impl(mbd_plan* p, const float* d_state0, int i, uint32_t key_inout[2], const float* d_Ybar_in,
                             float* d_Ybar_out, float* d_rew_mean, hipStream_t s, const NoiseSpec& ns,
                             const uint32_t* key_after = nullptr, const NoiseSpec& ns_after = NoiseSpec{},
                             const float* d_xref = nullptr) {
  if (p->cfg.shard_count != p->cfg.Nsample)
    return fail(MBD_ERR_STATE, "reverse_once on a sharded plan: use sample_rollout + all-gather + score_update");
  uint32_t keys[4];
  host_split(key_inout, 2, p->cfg.prng_impl, keys);  // rng, Y0s_rng = split(rng)  (mbd_planner.py:103)
  const uint32_t ks[2] = {keys[2], keys[3]};
  if (i > 1) {  // the next step's normals beside this rollout: its key is the next split of the advanced rng
    uint32_t nk[4];
    const uint32_t adv[2] = {keys[0], keys[1]};
    host_split(adv, 2, p->cfg.prng_impl, nk);
    const uint32_t next_ks[2] = {nk[2], nk[3]};
    MBD_TRY(declare_next_key(p, next_ks, ns));
  } else if (key_after) {
    MBD_TRY(declare_next_key(p, key_after, ns_after));
  }
  MBD_TRY(plan_sample_rollout(p, i, ks, d_Ybar_in, p->d_rews, p->cfg.enable_demo ? p->d_lp.get() : nullptr, s, d_state0, ns, d_xref));
  MBD_TRY(plan_score_update(p, i, d_Ybar_in, p->d_rews, p->d_lp, d_Ybar_out, d_rew_mean, s,
                            d_xref ? p->demo.rew_xref : p->env->rew_xref));
  key_inout[0] = keys[0];
  key_inout[1] = keys[1];
  return MBD_OK;
}

extern "C" int mbd_plan_reverse_once(mbd_plan* p, int i, uint32_t key_inout[2], float* d_Ybar, float* d_rew_mean,
                                     void* stream_) {
  if (!p || !key_inout || !d_Ybar || !d_rew_mean) return fail(MBD_ERR_INVALID, "NULL argument");
  NO_SESSION(p, "reverse_once");
  hipStream_t s = (hipStream_t)stream_;
  // the update is not in place on the device (wmean reads Ybar_i while writing Ybar_{i-1})
  p->wt.begin();
  MBD_TRY(reverse_once_impl(p, p->d_state0, i, key_inout, d_Ybar, p->d_Ybar, d_rew_mean, s, noise_spec(p, false)));
  HIP_TRY(hipMemcpyAsync(d_Ybar, p->d_Ybar, sizeof(float) * p->HNu, hipMemcpyDeviceToDevice, s));
  return MBD_OK;
}

extern "C" int mbd_plan_run(mbd_plan* p, const uint32_t key[2], float* mu_0ts_out, float* rew_means_out,
                            float* rew_final_out, double* loop_seconds_out) {
  if (!p || !key) return fail(MBD_ERR_INVALID, "NULL argument");
  NO_SESSION(p, "run");
  HIP_TRY(hipSetDevice(p->env->device));
  const int Nd = p->cfg.Ndiffuse, HNu = p->HNu;
  hipStream_t s = p->stream;
  uint32_t rng[2] = {key[0], key[1]};
  float* cur = p->d_Ybar;  // YN = zeros (mbd_planner.py:95; mu_0T path_integral.py:107)
  if (p->d_sigma) {
    const float one = 1.0f;  // sigma = 1.0 (path_integral.py:131)
    HIP_TRY(hipMemcpy(p->d_sigma, &one, sizeof(float), hipMemcpyHostToDevice));
  }
  HIP_TRY(hipMemsetAsync(cur, 0, sizeof(float) * HNu, s));
  MBD_TRY(p->adapt.table(-1, p->noise.shape_always(), HNu, s));  // (an adapt record: a = ones, and its log begins)
  p->adapt.count = 0;
  MBD_TRY(elite_table(p->elite, -1, HNu, s));  // (an elite record: no elites, and its log begins)
  p->elite.restart();
  HIP_TRY(hipStreamSynchronize(s));
  p->wt.begin();
  auto t0 = std::chrono::steady_clock::now();
  for (int i = Nd - 1; i >= 1; --i) {  // reverse() (mbd_planner.py:138-148)
    float* nxt = p->d_mu + (size_t)(Nd - 1 - i) * HNu;  // Ybars.append(Yi)
    MBD_TRY(plan_keep_in_step(p));
    MBD_TRY(reverse_once_impl(p, p->d_state0, i, rng, cur, nxt, p->d_rewmeans + (Nd - 1 - i), s, noise_spec(p, false)));
    cur = nxt;
  }
  HIP_TRY(hipStreamSynchronize(s));
  auto t1 = std::chrono::steady_clock::now();
  if (loop_seconds_out) *loop_seconds_out = std::chrono::duration<double>(t1 - t0).count();
  HIP_TRY(p->d_mu.download(mu_0ts_out, (size_t)(Nd - 1) * HNu));
  HIP_TRY(p->d_rewmeans.download(rew_means_out, (size_t)(Nd - 1)));
  if (rew_final_out) {  // rollout_us(state_init, Yi[-1]).mean()  (mbd_planner.py:179-180)
    MBD_TRY(launch_rollout(p->env, p->d_state0, cur, 1, p->cfg.Hsample, nullptr, p->d_scratch, nullptr, nullptr, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(p->d_scratch.download(rew_final_out, 1));
  }
  return MBD_OK;
}

// (mbd_internal.h: what the plans' and the sweeps' episodes do alike)
bool plant_tick_draw(const mbd_mpc_plant& pr, int prng_impl, int t, uint32_t dk[2], SweepPlant& sp, int k) {
  uint32_t dkk[4];
  host_split(dk, 2, prng_impl, dkk);
  dk[0] = dkk[0]; dk[1] = dkk[1];
  const bool kick_now = pr.kick_std > 0.0f && (t + 1) % pr.kick_every == 0;
  sp.k[k][0] = dkk[2]; sp.k[k][1] = dkk[3];
  sp.act_std[k] = pr.act_std; sp.kick_std[k] = kick_now ? pr.kick_std : 0.0f; sp.has[k] = 1;
  return kick_now;
}

extern "C" int mbd_plan_set_mpc_sigma(mbd_plan* p, const mbd_mpc_sigma* rec) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  if (p->cfg.update_method == 0) return fail(MBD_ERR_STATE, "set_mpc_sigma: not a path-integral plan (update_method == 0)");
  NO_SESSION(p, "set_mpc_sigma");
  return p->sigma_rec.set(rec, p->cfg.update_method);
}

extern "C" int mbd_plan_peek_mpc_sigma(mbd_plan* p, float* sigmas_out) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  return p->sigma_rec.peek(p->env->device, 0, sigmas_out, "plan");
}

extern "C" int mbd_plan_set_mpc_plant(mbd_plan* p, const mbd_mpc_plant* rec) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  NO_SESSION(p, "set_mpc_plant");
  if (!rec) {
    p->has_plant = false;
    p->plant_rec = mbd_mpc_plant{};
    return MBD_OK;
  }
  MBD_TRY(check_mpc_plant(p->env, rec));
  p->plant_rec = *rec;
  p->has_plant = true;
  return MBD_OK;
}

extern "C" int mbd_plan_set_mpc_delay(mbd_plan* p, const mbd_mpc_delay* rec) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  NO_SESSION(p, "set_mpc_delay");
  return p->delay.set(rec, p->Nu);
}

extern "C" int mbd_plan_peek_mpc_predicted(mbd_plan* p, float* predicted_out) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  if (!p->delay.has) return fail(MBD_ERR_STATE, "peek_mpc_predicted: the plan has no delay record");
  if (p->delay.pred_ticks < 1) return fail(MBD_ERR_STATE, "peek_mpc_predicted: no episode has run with the record yet");
  HIP_TRY(hipSetDevice(p->env->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(p->d_mpc_pred.download(predicted_out, (size_t)p->delay.pred_ticks * p->env->state_size()));
  return MBD_OK;
}

extern "C" int mbd_plan_set_mpc_demo(mbd_plan* p, const mbd_mpc_demo* rec) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  NO_SESSION(p, "set_mpc_demo");
  return p->demo.set(p->env, p->cfg, rec);
}

extern "C" int mbd_plan_peek_mpc_track(mbd_plan* p, float* err_out, float* windows_out) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  return p->demo.peek(p->env->device, 0, err_out, windows_out, "plan");
}

// ---- the ensemble record (include/mbd_hip.h mbd_ensemble) ---------------------------------------------------------------
// the refusals of a record against the plan — host arithmetic, no launch
static int check_ensemble(const mbd_plan* p, const mbd_ensemble* rec) {
  const mbd_env* env = p->env;
  const mbd_plan_config& c = p->cfg;
  if (rec->n_members < 1 || rec->n_members > MBD_MAX_ENSEMBLE)
    return fail(MBD_ERR_INVALID, "ensemble record: n_members=%d outside [1, %d]", rec->n_members, MBD_MAX_ENSEMBLE);
  if (rec->risk != MBD_RISK_MEAN && rec->risk != MBD_RISK_MIN)
    return fail(MBD_ERR_INVALID, "ensemble record: risk=%d: MBD_RISK_MEAN (0) or MBD_RISK_MIN (1)", rec->risk);
  for (int r = 0; r < 6; ++r)
    if (rec->reserved[r] != 0) return fail(MBD_ERR_INVALID, "ensemble record: reserved[%d]=%d: must be 0", r, rec->reserved[r]);
  if (env->kind != ENV_MODEL) return fail(MBD_ERR_UNSUPPORTED, "ensemble record: env '%s' has no model to perturb", env->name.c_str());
  if (c.enable_demo) return fail(MBD_ERR_UNSUPPORTED, "ensemble record: enable_demo=1: which member's log-density would count?");
  if (c.update_method != 0)
    return fail(MBD_ERR_UNSUPPORTED, "ensemble record: update_method=%d: ensembles score MBD plans only", c.update_method);
  if (c.shard_count != c.Nsample)
    return fail(MBD_ERR_STATE, "ensemble record: shard_count=%d of Nsample=%d: ensembles run unsharded plans", c.shard_count, c.Nsample);
  const mbd_model_t& a = env->model;
  for (int m = 0; m < rec->n_members; ++m) {
    const mbd_env* me = rec->members[m];
    if (!me || me == env) continue;
#define ENS_SAME(what, x, y)                                                                                              \
  if ((x) != (y))                                                                                                         \
    return fail(MBD_ERR_INVALID, "ensemble record: member %d: %s=%d, the plan's env has %d", m, what, (int)(x), (int)(y))
    ENS_SAME("device", me->device, env->device);
    if (me->kind != ENV_MODEL) return fail(MBD_ERR_INVALID, "ensemble record: member %d: env '%s' has no model", m, me->name.c_str());
    const mbd_model_t& b = me->model;
    ENS_SAME("n_links", b.n_links, a.n_links);
    ENS_SAME("action_size", b.n_act, a.n_act);
    ENS_SAME("planar flag", (b.flags & MBD_FLAG_PLANAR) != 0, (a.flags & MBD_FLAG_PLANAR) != 0);
    ENS_SAME("flags (the spec-flag word)", b.flags & MBD_SPEC_FLAGS, a.flags & MBD_SPEC_FLAGS);
    ENS_SAME("reward_kind", b.reward_kind, a.reward_kind);
    ENS_SAME("n_frames", b.n_frames, a.n_frames);
    ENS_SAME("n_col", b.n_col, a.n_col);
    ENS_SAME("n_track", b.n_track, a.n_track);
    ENS_SAME("n_q", b.n_q, a.n_q);
    ENS_SAME("n_qd", b.n_qd, a.n_qd);
    for (int k = 0; k < a.n_col; ++k) ENS_SAME("col_link (colliders per link)", b.col_link[k], a.col_link[k]);
    for (int l = 0; l < a.n_links; ++l) {
      ENS_SAME("parent (the tree)", b.parent[l], a.parent[l]);
      ENS_SAME("n_rot (the tree)", b.n_rot[l], a.n_rot[l]);
      ENS_SAME("n_slide (the tree)", b.n_slide[l], a.n_slide[l]);
    }
    for (int k = 0; k < a.n_act; ++k) {
      ENS_SAME("act_link", b.act_link[k], a.act_link[k]);
      ENS_SAME("act_slot", b.act_slot[k], a.act_slot[k]);
    }
    for (int k = 0; k < a.n_track; ++k) ENS_SAME("track_link", b.track_link[k], a.track_link[k]);
    // the wave-uniform switches of RolloutParams, then the shape the launch decision and the template parameters are
    // derived from (EnvShape)
    ENS_SAME("slide_limits", me->slide_limits, env->slide_limits);
    ENS_SAME("max_children", me->max_children, env->max_children);
    ENS_SAME("max_rot", me->max_rot, env->max_rot);
    ENS_SAME("any_stiff", me->any_stiff, env->any_stiff);
    ENS_SAME("has_weld", me->has_weld, env->has_weld);
    ENS_SAME("lps (lane table)", me->lps, env->lps);
    ENS_SAME("dpp_family (lane table)", me->dpp_family, env->dpp_family);
    ENS_SAME("lane_tab", memcmp(me->lane_tab, env->lane_tab, sizeof(env->lane_tab)) != 0, 0);
    ENS_SAME("helpers (lane table)", me->helpers, env->helpers);
    ENS_SAME("spec", me->spec, env->spec);
    ENS_SAME("iso_inertia", me->iso, env->iso);
    ENS_SAME("diag_inertia (inertia shape)", me->diag_inertia, env->diag_inertia);
    ENS_SAME("axisym (inertia shape)", me->axisym, env->axisym);
    ENS_SAME("axi (inertia shape)", me->axi, env->axi);
    ENS_SAME("max_col", me->max_col, env->max_col);
    ENS_SAME("slides", me->slides, env->slides);
    ENS_SAME("max_slide", me->max_slide, env->max_slide);
    ENS_SAME("slides_world_only", me->slides_world_only, env->slides_world_only);
    ENS_SAME("humanoid_shape", me->humanoid_shape, env->humanoid_shape);
    ENS_SAME("fl (planar switches)", me->fl, env->fl);
#undef ENS_SAME
    // the reference table a tracking reward reads (RolloutParams::xref): the one launch reads the plan's env's for every
    // member, a member's own launch its own — they have to be the same table
    if ((me->d_xref != nullptr) != (env->d_xref != nullptr))
      return fail(MBD_ERR_INVALID, "ensemble record: member %d: xref %s, the plan's env's is %s", m, me->d_xref ? "present" : "absent",
                  env->d_xref ? "present" : "absent");
    if (env->d_xref && a.n_track > 0) {
      const size_t nx = (size_t)a.n_track * kXrefRows * 3;
      std::vector<float> xa(nx), xb(nx);
      HIP_TRY(hipSetDevice(env->device));
      HIP_TRY(hipMemcpy(xa.data(), env->d_xref, sizeof(float) * nx, hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(xb.data(), me->d_xref, sizeof(float) * nx, hipMemcpyDeviceToHost));
      if (memcmp(xa.data(), xb.data(), sizeof(float) * nx) != 0)
        return fail(MBD_ERR_INVALID, "ensemble record: member %d: xref differs from the plan's env's", m);
    }
  }
  return MBD_OK;
}

extern "C" int mbd_plan_set_ensemble(mbd_plan* p, const mbd_ensemble* rec) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  NO_SESSION(p, "set_ensemble");
  if (!rec) {
    p->has_ens = false;
    p->ens_stepped = false;
    p->ens_rec = mbd_ensemble{};
    return MBD_OK;
  }
  if (p->zone.has) return refuse_beside_zones("ensemble");
  if (p->togo.has) return refuse_beside_togo("ensemble");  // (before check_ensemble, which may read the members' reference from the device)
  MBD_TRY(check_ensemble(p, rec));
  if (p->pick.has)
    return fail(MBD_ERR_UNSUPPORTED, "ensemble: the plan carries a pick record (mbd_plan_set_mpc_pick): the pick compares returns, an "
                                     "ensemble's reward is a reduction over members");
  if (p->val.has)
    return fail(MBD_ERR_STATE, "ensemble: the plan carries a value record (mbd_plan_set_value): an ensemble launch returns rewards only");
  HIP_TRY(hipSetDevice(p->env->device));
  HIP_TRY(hipDeviceSynchronize());  // (a step in flight may still read the previous record's buffers)
  const size_t N = (size_t)p->cfg.Nsample, H = (size_t)p->cfg.Hsample, M = (size_t)rec->n_members;
  p->has_ens = false;
  HIP_TRY(p->d_ens_rews.grow(M * N));
  HIP_TRY(p->d_ens_rewss.grow(M * N * H));
  HIP_TRY(p->d_ens_comb.grow(N));
  p->ens_rec = *rec;
  for (int m = 0; m < rec->n_members; ++m)
    if (!p->ens_rec.members[m]) p->ens_rec.members[m] = p->env;
  for (int m = rec->n_members; m < MBD_MAX_ENSEMBLE; ++m) p->ens_rec.members[m] = nullptr;
  p->has_ens = true;
  p->ens_stepped = false;
  return MBD_OK;
}

extern "C" int mbd_plan_peek_ensemble(mbd_plan* p, float* rews_members_out, float* rews_out) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  if (!p->has_ens) return fail(MBD_ERR_STATE, "peek_ensemble: the plan has no ensemble record");
  if (!p->ens_stepped) return fail(MBD_ERR_STATE, "peek_ensemble: no diffusion step with the record to show yet");
  HIP_TRY(hipSetDevice(p->env->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t N = (size_t)p->cfg.Nsample, M = (size_t)p->ens_rec.n_members;
  HIP_TRY(p->d_ens_rews.download(rews_members_out, M * N));
  HIP_TRY(p->d_ens_comb.download(rews_out, N));
  return MBD_OK;
}

extern "C" int mbd_plan_set_objective(mbd_plan* p, const mbd_objective* rec) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  NO_SESSION(p, "set_objective");
  float wsum = 0.0f;
  if (rec) MBD_TRY(check_objective(rec, p->cfg.Hsample, p->Nu, &wsum));  // (before any device access)
  if (rec && p->togo.has) return refuse_beside_togo("objective record");
  return p->obj.set(rec, wsum, p->env->device, 1, p->cfg.Nsample, p->cfg.Hsample, p->Nu, (size_t)MBD_MAX_ENSEMBLE * p->cfg.Nsample);
}

extern "C" int mbd_plan_peek_objective(mbd_plan* p, float* ret_out, float* cost_out) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  return p->obj.peek(p->env, 0, ret_out, cost_out, "plan");
}

extern "C" int mbd_plan_set_value(mbd_plan* p, const mbd_value* rec) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  NO_SESSION(p, "set_value");
  if (rec) MBD_TRY(check_value(rec, p->env->state_size(), p->env->kind == ENV_MODEL));  // (before any device access)
  if (rec && p->has_ens)
    return fail(MBD_ERR_STATE, "value record: the plan carries an ensemble record (an ensemble launch returns rewards only)");
  if (rec && p->togo.has) return refuse_beside_togo("value record");
  return p->val.set(rec, p->env, (size_t)p->cfg.shard_count, 1);
}

extern "C" int mbd_plan_peek_value(mbd_plan* p, float* v_out) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  return p->val.peek(p->env, v_out, "plan");
}

extern "C" int mbd_plan_eval_value(mbd_plan* p, const float* states, int B, float* v_out) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  return p->val.eval(p->env, states, B, v_out, "plan");
}

extern "C" int mbd_plan_set_zones(mbd_plan* p, const mbd_zones* rec) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  if (rec) {  // (before any device access)
    const int n_track = p->env && p->env->kind == ENV_MODEL ? p->env->model.n_track : 0;
    MBD_TRY(check_zones(rec, n_track > 0 ? n_track : 32));  // (an env without tracks: the other fields first, then its own refusal)
    MBD_TRY(check_zones_handle(p->env, p->cfg, "plan"));
    if (p->has_ens) return fail(MBD_ERR_UNSUPPORTED, "zone record: the plan carries an ensemble record (an ensemble launch returns rewards only)");
    if (p->togo.has) return refuse_beside_togo("zone record");
    if (p->pick.has) return fail(MBD_ERR_UNSUPPORTED, "zone record: the plan carries a pick record (its slots' rollouts write no positions)");
    if (p->cfg.shard_count != p->cfg.Nsample) return refuse_sharded(p->cfg, "zone");
  }
  NO_SESSION(p, "set_zones");
  return p->zone.set(rec, p->env, (size_t)p->cfg.shard_count, p->cfg.Hsample);
}

extern "C" int mbd_plan_update_zones(mbd_plan* p, const mbd_zones* rec) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  if (p->session.in_flight) return fail(MBD_ERR_STATE, "update_zones: a tick is in flight (mbd_plan_mpc_collect first)");
  return p->zone.update(rec, p->env, "plan");
}

extern "C" int mbd_plan_peek_zones(mbd_plan* p, float* pen_out, float* clear_out) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  return p->zone.peek(p->env, 0, p->zone.rows, pen_out, clear_out, "plan");
}

extern "C" int mbd_plan_peek_mpc_zones(mbd_plan* p, float* pen_out, float* clear_out) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  return p->zone.peek_mpc(p->env, 0, pen_out, clear_out, "plan");
}

extern "C" int mbd_plan_set_weighting(mbd_plan* p, const mbd_weighting* rec) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  NO_SESSION(p, "set_weighting");
  if (rec) MBD_TRY(check_weighting(rec));  // (before any device access)
  if (rec && p->cfg.enable_demo)
    return fail(MBD_ERR_UNSUPPORTED, "weighting record: enable_demo=1: the demo blend standardises twice, an ESS target is not defined there");
  if (rec && p->togo.has) return refuse_beside_togo("weighting record");
  // weigh_kernel's logp0 window, as mbd_plan_create raises score_kernel's (a sweep never needs it: mbd_sweep_create refuses N > 12288)
  if (rec && (size_t)p->cfg.Nsample * sizeof(float) > 48 * 1024 && p->cfg.Nsample <= kLdsN) {
    HIP_TRY(hipSetDevice(p->env->device));
    HIP_TRY(hipFuncSetAttribute((const void*)weigh_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024));
  }
  return p->wt.set(rec, p->env->device, 1, p->cfg.Ndiffuse - 1, p->cfg.Nsample);
}

extern "C" int mbd_plan_peek_weighting(mbd_plan* p, float* temp_out, float* ess_out, int32_t* kept_out, int capacity, int* count_out) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  return p->wt.peek(p->env, 0, temp_out, ess_out, kept_out, capacity, count_out, "plan");
}

extern "C" int mbd_plan_set_mpc_pick(mbd_plan* p, const mbd_mpc_pick* rec) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  NO_SESSION(p, "set_mpc_pick");
  if (rec) MBD_TRY(check_mpc_pick(rec));  // (before any device access)
  if (rec && p->cfg.enable_demo)
    return fail(MBD_ERR_UNSUPPORTED, "mpc pick record: enable_demo=1: a demo plan's score is not the return the pick compares");
  if (rec && p->has_ens)
    return fail(MBD_ERR_UNSUPPORTED, "mpc pick record: the plan carries an ensemble record: its reward is a reduction over members");
  if (rec && p->zone.has) return refuse_beside_zones("mpc pick record");
  return p->pick.set(rec, p->env->device, 1, p->HNu, p->cfg.Hsample);
}

extern "C" int mbd_plan_peek_mpc_pick(mbd_plan* p, int32_t* choice_out, float* rets_out, int32_t* best_out, int capacity, int* count_out) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  return p->pick.peek(p->env, 0, choice_out, rets_out, best_out, capacity, count_out, "plan");
}

// include/mbd_hip_debug.h: ring_read on the device over a caller-given ring, both instantiations the logs use
template <typename T>
static int debug_ring_read(const T* ring, int width, long long cap, long long count, long long n, T* out) {
  if (!ring || !out) return fail(MBD_ERR_INVALID, "ring_read: NULL argument");
  if (width < 1 || width > 16 || cap < 1 || cap > kLogCap || count < 0 || n < 0)
    return fail(MBD_ERR_INVALID, "ring_read: width=%d cap=%lld count=%lld n=%lld", width, cap, count, n);
  if (device_count_quiet() < 1) return fail(MBD_ERR_NO_DEVICE, "no HIP device: this library has no CPU fallback");
  DevBuf<T> d_ring;
  HIP_TRY(d_ring.upload(ring, (size_t)cap * width));
  const long long m = std::min(std::min(n, count), cap);
  memset(out, 0xff, sizeof(T) * (size_t)m * width);
  return ring_read<T>(d_ring.get(), width, count, cap, n, out);
}

extern "C" int mbd_debug_ring_read(const float* ring, int width, long long cap, long long count, long long n, float* out) {
  return debug_ring_read<float>(ring, width, cap, count, n, out);
}

extern "C" int mbd_debug_ring_read_i32(const int32_t* ring, int width, long long cap, long long count, long long n, int32_t* out) {
  return debug_ring_read<int32_t>(ring, width, cap, count, n, out);
}

extern "C" int mbd_plan_set_adapt(mbd_plan* p, const mbd_adapt* rec) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  if (rec) MBD_TRY(check_adapt(rec, p->cfg.update_method, p->cfg.enable_demo));  // (before any device access)
  if (rec && p->cfg.shard_count != p->cfg.Nsample) return refuse_sharded(p->cfg, "adapt");
  NO_SESSION(p, "set_adapt");
  if (rec && p->togo.has) return refuse_beside_togo("adapt record");
  if (!rec && !p->adapt.has) return MBD_OK;  // (nothing to clear: no device is touched)
  // normals prepared ahead were made under another table: as mbd_plan_set_noise_shape, nothing prepared survives
  p->ring.forget();
  return p->adapt.set(rec, p->HNu, p->noise.shape_always(), p->env, p->stream);
}

extern "C" int mbd_plan_peek_adapt(mbd_plan* p, float* a_out, float* ratio_out, int32_t* skipped_out, int capacity, int* count_out) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  return p->adapt.peek(p->env, p->HNu, a_out, ratio_out, skipped_out, capacity, count_out);
}

extern "C" int mbd_plan_set_elites(mbd_plan* p, const mbd_elites* rec) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  if (rec) MBD_TRY(check_elites(rec, p->cfg.Nsample, p->cfg.update_method, p->cfg.enable_demo));  // (before any device access)
  if (rec && p->cfg.shard_count != p->cfg.Nsample) return refuse_sharded(p->cfg, "elite");
  NO_SESSION(p, "set_elites");
  if (!rec && !p->elite.has) return MBD_OK;  // (nothing to clear: no device is touched)
  // normals prepared ahead are not what the record's steps take, and a buffer the record rewrote is not what its tag said: as
  // mbd_plan_set_noise_shape, nothing prepared survives — in either direction
  p->ring.forget();
  MBD_TRY(p->elite.set(rec, 1, p->HNu, p->env->device));
  MBD_TRY(elite_table(p->elite, -1, p->HNu, p->stream));  // (no elites afterwards: one launch, waited for)
  if (p->elite.has) HIP_TRY(hipStreamSynchronize(p->stream));
  return MBD_OK;
}

extern "C" int mbd_plan_peek_elites(mbd_plan* p, float* elites_out, float* returns_out, int32_t* src_out, int32_t* count_out,
                                    int32_t* log_count, int32_t* log_kept, float* log_top, int capacity, int* n_log_out) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  return p->elite.peek(p->env, 0, p->HNu, elites_out, returns_out, src_out, count_out, log_count, log_kept, log_top, capacity,
                       n_log_out, "plan");
}

// include/mbd_hip_debug.h: the elite record's two launches alone on the DEVICE, on caller-given arrays, over a scratch record (the
// host reference, mbd_debug_elites_host: mbd_records.hip).  What is read back is filled with all-ones bits first; the log is one entry long (steps = 0: slot 0).
extern "C" int mbd_debug_elites_inject(const float* cand, int N, int HNu, const float* ybar, float sigma, int lazy, const float* g,
                                       int n_elites, int nominal, const float* E_in, int count_in, float* cand_out) {
  MBD_TRY(check_elites_args("elites_inject", cand, N, HNu, ybar, sigma, lazy, n_elites, nominal, E_in, count_in));
  if (!cand_out) return fail(MBD_ERR_INVALID, "elites_inject: NULL argument");
  if (device_count_quiet() < 1) return fail(MBD_ERR_NO_DEVICE, "no HIP device: this library has no CPU fallback");
  const size_t n = (size_t)N * HNu;
  DevBuf<float> d_cand, d_ybar, d_g;
  EliteRec L;
  HIP_TRY(d_cand.upload(cand, n));
  HIP_TRY(d_ybar.upload(ybar, HNu));
  if (g) HIP_TRY(d_g.upload(g, HNu));  // (without: d_g stays nullptr)
  MBD_TRY(L.scratch(n_elites, nominal, 1, HNu, E_in, &count_in));
  MBD_TRY(elite_inject(L, StepCand{d_cand, N, HNu, lazy ? 1 : 0, sigma, nullptr, d_ybar}, d_g, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(d_cand.download(cand_out, n));
  return MBD_OK;
}
extern "C" int mbd_debug_elites_select(const float* rews, const float* cand, int N, int HNu, const float* ybar, float sigma, int lazy,
                                       int n_elites, int nominal, int count_in, float* E_out, float* R_out, int32_t* src_out,
                                       int32_t* count_out, int32_t* kept_out, float* top_out) {
  MBD_TRY(check_elites_args("elites_select", cand, N, HNu, ybar, sigma, lazy, n_elites, nominal, nullptr, 0));
  if (!rews) return fail(MBD_ERR_INVALID, "elites_select: NULL argument");
  if (count_in < 0 || count_in > n_elites) return fail(MBD_ERR_INVALID, "elites_select: count=%d outside [0, n_elites=%d]", count_in, n_elites);
  if (device_count_quiet() < 1) return fail(MBD_ERR_NO_DEVICE, "no HIP device: this library has no CPU fallback");
  DevBuf<float> d_rews, d_cand, d_ybar;
  EliteRec L;
  HIP_TRY(d_rews.upload(rews, N));
  HIP_TRY(d_cand.upload(cand, (size_t)N * HNu));
  HIP_TRY(d_ybar.upload(ybar, HNu));
  MBD_TRY(L.scratch(n_elites, nominal, 1, HNu, nullptr, &count_in));
  MBD_TRY(elite_select(L, d_rews, StepCand{d_cand, N, HNu, lazy ? 1 : 0, sigma, nullptr, d_ybar}, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(L.d_E.download(E_out, (size_t)n_elites * HNu));
  HIP_TRY(L.d_R.download(R_out, n_elites));
  HIP_TRY(L.d_src.download(src_out, n_elites));
  // (count' as the plan's word holds it; the log entry's copy must agree with it: the caller gets the log's, the word is checked)
  int cnt_word = -1, cnt_log = -1;
  HIP_TRY(L.d_count.download(&cnt_word, 1));
  HIP_TRY(L.d_log_count.download(&cnt_log, 1));
  if (cnt_word != cnt_log) return fail(MBD_ERR_STATE, "elites_select: count word %d, log entry %d", cnt_word, cnt_log);
  if (count_out) *count_out = cnt_word;
  HIP_TRY(L.d_log_kept.download(kept_out, 1));
  HIP_TRY(L.d_log_top.download(top_out, 1));
  return MBD_OK;
}

extern "C" int mbd_plan_set_togo(mbd_plan* p, const mbd_togo* rec) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  if (rec) {  // (before any device access)
    MBD_TRY(check_togo(rec, p->cfg.Hsample, p->cfg.Nsample, p->cfg.update_method, p->cfg.enable_demo));
    const char* other = p->obj.has ? "an objective" : p->val.has ? "a value" : p->wt.has ? "a weighting" : p->adapt.has ? "an adapt"
                        : p->has_ens ? "an ensemble" : nullptr;
    if (other)
      return fail(MBD_ERR_UNSUPPORTED, "to-go record: the plan carries %s record: what that record means per horizon row is not defined",
                  other);
    if (p->zone.has) return refuse_beside_zones("to-go record");
    if (p->cfg.shard_count != p->cfg.Nsample) return refuse_sharded(p->cfg, "to-go");
  }
  NO_SESSION(p, "set_togo");
  if (!rec && !p->togo.has) return MBD_OK;  // (nothing to clear: no device is touched)
  return p->togo.set(rec, 1, p->cfg.Hsample, p->cfg.Nsample, p->env->device);
}

extern "C" int mbd_plan_peek_togo(mbd_plan* p, int32_t* starts_out, float* R_out, float* W_out, int32_t* n_groups_out) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  return p->togo.peek(p->env, 0, p->cfg.Nsample, p->d_weights, starts_out, R_out, W_out, n_groups_out, "plan");
}

// include/mbd_hip_debug.h: the to-go record's two launches of a step alone on the DEVICE, on caller-given arrays, by a scratch
// record's own launch (the host reference, mbd_debug_togo_host: mbd_records.hip).  What is read back is filled with all-ones bits
// (quiet NaN) first.
extern "C" int mbd_debug_togo_step(const float* cand, const float* ybar, const float* rews, const float* rewss, int N, int H, int Nu,
                                   int block, int min_tail, int lazy, float sigma, float temp, int std_guard, float alpha_i,
                                   float alpha_bar_i, float alpha_bar_im1, int literal, float* ybar_out, float* R_out, float* W_out,
                                   float* rew_mean_out) {
  if (!cand || !ybar || !rews || !rewss) return fail(MBD_ERR_INVALID, "togo_step: NULL argument");
  MBD_TRY(check_togo_args("togo_step", N, H, block, min_tail));
  if (Nu < 1 || (uint64_t)N * (uint64_t)H * (uint64_t)Nu > (1ull << 26)) return fail(MBD_ERR_INVALID, "togo_step: N=%d H=%d Nu=%d", N, H, Nu);
  if (N > kTogoMaxN) return fail(MBD_ERR_INVALID, "togo_step: N=%d above %d", N, kTogoMaxN);
  if (device_count_quiet() < 1) return fail(MBD_ERR_NO_DEVICE, "no HIP device: this library has no CPU fallback");
  const size_t HNu = (size_t)H * Nu;
  TogoRec L;
  L.layout(block, min_tail, H);
  const size_t gn = (size_t)L.G * N;
  DevBuf<float> d_cand, d_ybar, d_rews, d_rewss, d_out, d_keep, d_w, d_mean;
  HIP_TRY(d_cand.upload(cand, (size_t)N * HNu));
  HIP_TRY(d_ybar.upload(ybar, HNu));
  HIP_TRY(d_rews.upload(rews, N));
  HIP_TRY(d_rewss.upload(rewss, (size_t)N * H));
  HIP_TRY(d_out.alloc_poisoned(HNu));
  HIP_TRY(d_keep.alloc_poisoned(HNu));
  HIP_TRY(d_w.alloc_poisoned(N));
  HIP_TRY(d_mean.alloc_poisoned(1));
  HIP_TRY(L.d_R.alloc_poisoned(gn));
  HIP_TRY(L.d_W.alloc_poisoned(gn));
  TogoUpdate A{};
  A.rews = d_rews; A.weights = d_w; A.rew_mean = d_mean; A.cand = d_cand; A.ybar_i = d_ybar; A.ybar_im1 = d_out; A.ybar_keep = d_keep;
  A.N = N; A.H = H; A.Nu = Nu; A.temp = temp; A.std_guard = std_guard ? 1 : 0; A.alpha_i = alpha_i; A.alpha_bar_i = alpha_bar_i;
  A.alpha_bar_im1 = alpha_bar_im1; A.literal = literal ? 1 : 0; A.lazy = lazy ? 1 : 0; A.sigma = sigma;
  MBD_TRY(togo_launch(L, d_rewss, A, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(d_out.download(ybar_out, HNu));
  HIP_TRY(L.d_R.download(R_out, gn));
  HIP_TRY(L.d_W.download(W_out, gn));
  HIP_TRY(d_w.download(W_out, N));  // (group 0's weights)
  HIP_TRY(d_mean.download(rew_mean_out, 1));
  return MBD_OK;
}

// ---- one tick's planning, shared by the batch episode (mbd_plan_run_mpc) and the session (mbd_plan_mpc_submit) ------------------
// The tick's keys, host arithmetic: rng, k_t = split(rng) advances the episode's chain; r = k_t is where the tick's own chain
// starts (mbd_plan_run's from it); after = split(split(rng')[1])[1] is the Y0s_rng of tick t+1's first step, whose normals are
// prepared beside this tick's last rollout (rng' = the advanced rng: looked at, not advanced).
static void mpc_tick_keys(int prng_impl, uint32_t rng[2], uint32_t r[2], uint32_t after[2]) {
  uint32_t kk[4], nk[4];
  host_split(rng, 2, prng_impl, kk);
  rng[0] = kk[0]; rng[1] = kk[1];
  r[0] = kk[2]; r[1] = kk[3];
  host_split(rng, 2, prng_impl, kk);
  const uint32_t k_next[2] = {kk[2], kk[3]};
  host_split(k_next, 2, prng_impl, nk);
  after[0] = nk[2]; after[1] = nk[3];
}
// What a tick plans from and under.  s_t: the state the system is in.  q_in: the committed queue [DE][Nu] of an episode with a
// delay record — the tick then first predicts, with the plan's env, where those rows leave the system (ONE rollout, one
// candidate, into shat) and plans from there — or nullptr.  cold: Ybar = zeros was set by the caller and the tick runs steps
// Ndiffuse-1 .. 1 under the noise in force ALWAYS (tick 0; a session's tick after mbd_plan_mpc_reset_mean); otherwise steps K .. 1
// from the shifted mean in d_Ybar under the warm ticks' noise.  r: k_t, advanced along the tick's chain.  key_after: see
// mpc_tick_keys, nullptr: no tick follows.  d_xref: the tick's demo window, or nullptr.  *mean: where M_t lies afterwards.
struct MpcTick {
  const float* s_t = nullptr;
  const float* q_in = nullptr;
  float* shat = nullptr;
  int DE = 0;
  bool cold = false;
  int K = 1;
  int E = 1;  // exec_steps: row E-1 of M_t is the last row committed before the next plan's row 0 (an objective record's prev)
  const uint32_t* key_after = nullptr;
  const float* d_xref = nullptr;
};
static int mpc_plan_tick(mbd_plan* p, const MpcTick& tk, uint32_t r[2], hipStream_t s, const float** mean) {
  const int Nd = p->cfg.Ndiffuse, HNu = p->HNu;
  // with a delay record: the rows the system is committed to, the prediction of where they leave it, and the plan from there
  const float* plan_from = tk.s_t;
  if (tk.q_in) {
    MBD_TRY(launch_rollout(p->env, tk.s_t, tk.q_in, 1, tk.DE, nullptr, nullptr, nullptr, tk.shat, s));
    plan_from = tk.shat;
  }
  // the noise shape and basis: a cold tick is mbd_plan_run's loop (MBD_NOISE_WARM_TICKS: without), every other tick samples under
  // them in either mode — the first normals of the next tick, prepared beside this tick's last rollout, included
  const NoiseSpec ns = noise_spec(p, !tk.cold);
  // with an adapt record, ONE launch in front of the tick's first sampler: a = ones in a cold tick and without carry, otherwise a
  // shifted E rows forward with the mean; G under the caller's shape in force in this tick.  Stream order is the whole argument: it
  // stands behind the previous tick's last update and in front of this tick's first sampler, which reads G
  MBD_TRY(p->adapt.table(tk.cold || !p->adapt.carry ? -1 : tk.E * p->Nu, tk.cold ? p->noise.shape_always() : p->noise.shape_warm(), HNu, s));
  // with an elite record, ONE launch in the same place: no elites in a cold tick and without carry, otherwise the present ones
  // shifted E rows forward with the mean
  MBD_TRY(elite_table(p->elite, tk.cold || !p->elite.carry ? -1 : tk.E * p->Nu, HNu, s));
  p->wt.begin();  // (a weighting record's log holds the last tick's steps)
  const float* cur = p->d_Ybar;  // Ybar at a tick's first step: YN = zeros of a cold tick, shift_E(M_{t-1}) otherwise
  const float* last_in = cur;    // Ybar_i of the tick's last step
  float* last_out = nullptr;
  for (int i = tk.cold ? Nd - 1 : tk.K; i >= 1; --i) {
    float* nxt = p->d_mu + (size_t)(Nd - 1 - i) * HNu;  // (K <= Nd-1: a warm tick's steps use the last K slots)
    MBD_TRY(plan_keep_in_step(p));
    MBD_TRY(reverse_once_impl(p, plan_from, i, r, cur, nxt, p->d_rewmeans + (Nd - 1 - i), s, ns, tk.key_after, noise_spec(p, true), tk.d_xref));
    last_in = cur;
    cur = last_out = nxt;
  }
  // with a pick record: P_t over M_t where it lies, so that everything below and every boundary reads the picked plan
  if (p->pick.has) {
    PickTick pt{};
    pt.state = plan_from; pt.N = p->cfg.Nsample; pt.rews = p->d_rews;
    pt.cand = p->lazy ? p->ring.eps[p->ring.cur].get() : p->d_Y0s.get();
    pt.lazy = p->lazy; pt.sigma = p->sigmas[1]; pt.ybar_i = last_in; pt.ybar_i_stride = 0;
    pt.M = last_out; pt.M_stride = 0; pt.B = p->d_Ybar; pt.B_stride = 0;
    pt.cold = tk.cold ? 1u : 0u;
    MBD_TRY(p->pick.tick(p->env, p->obj, p->val, pt, s));
  }
  *mean = cur;
  // with an objective record, the next tick's previous action: clip(M_t[E-1]) — the commanded row, whatever a plant record adds to
  // it — by one launch behind the tick's last update kernel, hence in front of whatever boundary the caller runs: a session's
  // boundary kernel stays its tick's last kernel.  Here, so that the batch episode and the session cannot differ in it.
  MBD_TRY(p->obj.tick_advance(cur + (size_t)(tk.E - 1) * p->Nu, 0, s));
  return MBD_OK;
}

// Receding horizon (include/mbd_hip.h): the host only enqueues — the key chain is host arithmetic, the executed state never
// comes back — and keeps at most one step ahead of the device through plan_keep_in_step, as mbd_plan_run does.  A tick
// boundary adds two launches on the plan's stream: the rollout of M_t's first E rows (the env's rollout path, one candidate:
// what mbd_env_step runs) and mpc_boundary_kernel.  Both are stream-ordered between the tick's last weighted mean and the
// next tick's first rollout, so the ring of noise buffers keeps its argument (mbd_plan), aux-stream form included.
// With a plant record (mbd_plan_set_mpc_plant) the boundary is three launches in the same place on the same stream —
// mpc_plant_rows_kernel (the tick's normals, the executed rows, the kick values), the PLANT env's rollout of those rows, and
// the boundary kernel, in the ticks that end with a kick its kick variant — so that argument is unchanged again; the
// disturbance key chain is host arithmetic like the episode's.  Without a record: the two launches above, nothing else.
// With a delay record (mbd_plan_set_mpc_delay) a tick gains ONE launch, in FRONT of its first diffusion step on the same stream:
// the plan's env's rollout of the committed queue from s_t, one candidate over D E rows, whose final state is shat_t — written
// into slot t of the predicted states, which the tick's planning launches read as their start state.  The ring's argument,
// re-stated for it: the prediction is stream-ordered behind the previous tick's boundary (which wrote the queue it reads and
// s_t) and in front of the tick's first rollout (which reads shat_t); it carries no progress word and no noise job, so the
// sequence numbers the host looks for count the planning rollouts alone, as before.  The normals of the tick's first step were
// prepared beside the PREVIOUS tick's last rollout: they depend on their key only, not on shat_t, so the extra launch is not on
// their path — it sits between that rollout's weighted mean, which was the last reader of the buffer two steps back, and the
// rollout that reads them, like the boundary's launches.  The boundary itself stays where it was, in its delay variant: the
// rows executed are the queue's head, and the same launch that shifts the mean advances the queue into its other buffer.
// With a demo record (mbd_plan_set_mpc_demo; demo plans only) the tick loop launches nothing new: demo_windows_kernel fills the
// table of all T windows in ONE launch in front of the loop, on the same stream, and a tick's planning launches are handed a
// pointer into it where they read the env's demo (launch_rollout's and launch_logpd's d_xref) and the record's rew_xref where they
// read the env's; the rollout of the executed rows is handed its slice of the position log as d_xpos; mpc_track_err_kernel, ONE
// launch behind the loop, reads that log.  The ring's argument does not see any of it.
// A path-integral plan with a sigma record (mbd_plan_set_mpc_sigma) runs the same loop: mpc_plan_tick as it is — reverse_once_impl
// serves both families, a materialised plan ignores the declared keys, and the slots of d_mu and d_rewmeans are the same — so a
// tick's first normals are sampled in the tick.  Around it: ONE launch of mpc_pi_sigma_kernel in front of tick 0 (sigma = sigma_cold,
// the log's first entry) and one behind every tick's last update kernel, in front of the execution of its rows, which logs the
// sigma the tick ended with and leaves the next tick's in the carried slot.  Stream order is the whole argument: the kernel reads
// what cma_sigma_kernel wrote and writes what the next tick's sampler reads, all on the plan's stream; no host value, no
// synchronisation.  Launches per tick of K refinements: mppi 3 K (sampler, rollout, score + weighted mean), cma-es 5 K (plus
// spread and sigma), cem 5 K (sampler, rollout, score, selection, mean), under a noise basis one more per refinement; plus the
// sigma kernel and the boundary's two (three with a plant record, one more with a delay record).
// The planning of a tick — the prediction, the diffusion steps, the key chain — is mpc_plan_tick above, which a session
// (mbd_plan_mpc_submit) runs as well: what is said here about those launches holds for both, and the session restates the rest.
extern "C" int mbd_plan_run_mpc(mbd_plan* p, const mbd_mpc_config* mc, const uint32_t key[2], float* actions_out,
                                float* rewards_out, float* states_out, float* means_out, double* loop_seconds_out) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  if (!mc) return fail(MBD_ERR_INVALID, "mpc config is NULL");
  if (!key) return fail(MBD_ERR_INVALID, "key is NULL");
  NO_SESSION(p, "run_mpc");
  const mbd_plan_config& c = p->cfg;
  const int T = mc->n_ticks, K = mc->warm_steps, E = mc->exec_steps, H = c.Hsample;
  MBD_TRY(check_mpc_config(c, mc, p->demo.has, p->sigma_rec.has));
  if (c.shard_count != c.Nsample)
    return fail(MBD_ERR_STATE, "shard_count=%d of Nsample=%d: receding horizon runs unsharded plans", c.shard_count, c.Nsample);
  MBD_TRY(p->delay.check_run(E));
  mbd_env* e = p->env;
  const bool pi = c.update_method != 0;  // a path-integral plan (with a sigma record: check_mpc_config)
  HIP_TRY(hipSetDevice(e->device));
  const int HNu = p->HNu, Nu = e->action_size(), S = e->state_size();
  HIP_TRY(p->d_mpc_state.grow(2 * (size_t)S));
  HIP_TRY(p->d_mpc_states.grow(((size_t)T + 1) * S));
  HIP_TRY(p->d_mpc_means.grow((size_t)T * HNu));
  HIP_TRY(p->d_mpc_rewards.grow((size_t)T * (H - 1)));
  const bool has_plant = p->has_plant;
  const mbd_mpc_plant& pr = p->plant_rec;
  mbd_env* const pe = has_plant && pr.plant ? pr.plant : e;  // the env that executes the rows
  const int EN = E * Nu;
  const bool has_delay = p->delay.has;
  const int D = p->delay.D, Q = D * EN;  // (the committed queue: D blocks of E rows)
  if (has_delay) {
    HIP_TRY(p->d_mpc_queue.grow(2 * (size_t)Q));
    HIP_TRY(p->d_mpc_pred.grow((size_t)T * S));
  }
  if (has_plant || has_delay) HIP_TRY(p->d_mpc_actions.grow((size_t)T * EN));
  if (has_plant) {
    HIP_TRY(p->d_plant_eps.grow((size_t)EN + 3));
    HIP_TRY(p->d_plant_kick.grow(3));
  }
  // with a demo record (only a demo plan carries one): the table of the ticks' windows, one launch, and the position log
  const bool has_demo = p->demo.has;
  MBD_TRY(p->demo.check_plant(e, pe));
  // with a zone record: the same rule for the plant, and room for the log of the executed steps
  MBD_TRY(p->zone.check_plant(e, pe));
  MBD_TRY(p->zone.start(T, 1, E));
  const int planar = e->kind == ENV_MODEL && (e->model.flags & MBD_FLAG_PLANAR) ? 1 : 0;
  uint32_t dk[2] = {pr.key[0], pr.key[1]};  // the disturbance key chain: dk, d_t = split(dk) per tick
  const float* s_t = p->d_state0;  // where tick t's rollouts start: s_0 in the plan's own buffer, then the ping-pong buffers
  hipStream_t s = p->stream;
  float* const ybar0 = p->d_Ybar;  // Ybar at a tick's first step: YN = zeros at tick 0, shift_E(M_{t-1}) after
  HIP_TRY(hipMemsetAsync(ybar0, 0, sizeof(float) * HNu, s));
  HIP_TRY(hipMemcpyAsync(p->d_mpc_states, p->d_state0, sizeof(float) * S, hipMemcpyDeviceToDevice, s));
  if (has_delay) {
    MBD_TRY(p->delay.upload(p->d_mpc_queue, 1, E, Nu, s));
    p->delay.pred_ticks = 0;
  }
  // with an objective record: the previous action of tick 0 — the clipped last row of the committed queue, else clip(prev0) or
  // none — and from here to the end of the call the episode's slot, which one launch per tick re-forms
  MBD_TRY(p->obj.episode_start(has_delay ? p->d_mpc_queue + (Q - Nu) : nullptr, Q, s));
  struct ObjEpisode {
    ObjectiveRec& o;
    ~ObjEpisode() { o.episode_end(); }
  } obj_episode{p->obj};
  MBD_TRY(p->pick.start(T));  // (a pick record's log: one entry per tick)
  p->adapt.count = 0;         // (an adapt record's log: the episode's steps)
  p->elite.restart();         // (an elite record's log likewise)
  if (pi) {  // sigma = sigma_cold and the log's first entry, by the kernel that carries sigma across the boundaries
    MBD_TRY(p->sigma_rec.start(T, 1));
    p->sigma_rec.launch(p->d_sigma, 1, 0, true, s);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(s));
  const auto t0 = std::chrono::steady_clock::now();
  if (has_demo) MBD_TRY(p->demo.start(T, 1, E, has_delay ? D : 0, s));
  uint32_t rng[2] = {key[0], key[1]};
  for (int t = 0; t < T; ++t) {
    uint32_t r[2], after[2];  // k_t: the tick's key chain is mbd_plan_run's from it; the first Y0s_rng of tick t+1
    mpc_tick_keys(c.prng_impl, rng, r, after);
    // with a delay record: the queue the tick reads, and the one its boundary kernel advances it into
    const float* q_in = has_delay ? p->d_mpc_queue + (size_t)(t & 1) * Q : nullptr;
    float* q_out = has_delay ? p->d_mpc_queue + (size_t)((t + 1) & 1) * Q : nullptr;
    MpcTick tk;
    tk.s_t = s_t; tk.q_in = q_in; tk.shat = has_delay ? p->d_mpc_pred + (size_t)t * S : nullptr; tk.DE = D * E;
    tk.cold = t == 0; tk.K = K; tk.E = E; tk.key_after = t + 1 < T ? after : nullptr;
    tk.d_xref = has_demo ? p->demo.window(t) : nullptr;
    const float* cur = nullptr;
    MBD_TRY(mpc_plan_tick(p, tk, r, s, &cur));
    if (pi) {  // the sigma the tick ended with into the log, the next tick's into the carried slot: one launch, no host value
      p->sigma_rec.launch(p->d_sigma, 1, t, false, s);
      HIP_TRY(hipGetLastError());
    }
    // execute M_t's first E rows from s_t — with a delay record the queue's head —, then the boundary: Ybar of tick t+1, the
    // logs of M_t and s_{t+1}
    float* s_next = p->d_mpc_state + (size_t)(t & 1) * S;
    const float* rows = has_delay ? q_in : cur;
    bool kick_now = false;
    if (has_plant) {  // the rows the plant is fed: M_t[0:E] plus the tick's action noise, into the tick's slice of their log
      SweepPlant sp{};
      kick_now = plant_tick_draw(pr, c.prng_impl, t, dk, sp, 0);
      float* exec_rows = p->d_mpc_actions + (size_t)t * EN;
      hipLaunchKernelGGL(mpc_plant_rows_kernel, dim3(1, 1), dim3(256), 0, s, sp, c.prng_impl, rows, 0ll, EN, p->d_plant_eps,
                         exec_rows, p->d_plant_kick);
      HIP_TRY(hipGetLastError());
      rows = exec_rows;
    }
    // (with a demo record the launch also writes the tracked positions of its E steps into their log: same rewards, same state)
    // (and with a zone record — never beside a demo record, which only demo plans carry)
    MBD_TRY(launch_rollout(pe, s_t, rows, 1, E, p->d_mpc_rewards + (size_t)t * E, nullptr,
                           has_demo ? p->demo.xlog(t, 1, E) : p->zone.xlog(t, 1, E), s_next, s));
    // with a zone record: s_t and clr_t of the E executed steps into the episode's log, ONE launch over that single row
    MBD_TRY(p->zone.log(t, 1, E, s));
    float* const exec_log = has_plant ? nullptr : p->d_mpc_actions + (size_t)t * EN;  // (a plant's rows kernel has logged them)
    if (has_delay && kick_now)
      hipLaunchKernelGGL(mpc_boundary_delay_kick_kernel, dim3(1), dim3(256), 0, s, cur, HNu, EN, s_next, S,
                         (const float*)p->d_plant_kick, planar, ybar0, p->d_mpc_means + (size_t)t * HNu,
                         p->d_mpc_states + (size_t)(t + 1) * S, q_in, q_out, Q, exec_log);
    else if (has_delay)
      hipLaunchKernelGGL(mpc_boundary_delay_kernel, dim3(1), dim3(256), 0, s, cur, HNu, EN, (const float*)s_next, S, ybar0,
                         p->d_mpc_means + (size_t)t * HNu, p->d_mpc_states + (size_t)(t + 1) * S, q_in, q_out, Q, exec_log);
    else if (kick_now)
      hipLaunchKernelGGL(mpc_boundary_kick_kernel, dim3(1), dim3(256), 0, s, cur, HNu, EN, s_next, S,
                         (const float*)p->d_plant_kick, planar, ybar0, p->d_mpc_means + (size_t)t * HNu,
                         p->d_mpc_states + (size_t)(t + 1) * S);
    else
      hipLaunchKernelGGL(mpc_boundary_kernel, dim3(1), dim3(256), 0, s, cur, HNu, E * Nu, (const float*)s_next, S, ybar0,
                         p->d_mpc_means + (size_t)t * HNu, p->d_mpc_states + (size_t)(t + 1) * S);
    HIP_TRY(hipGetLastError());
    s_t = s_next;
  }
  if (has_demo) MBD_TRY(p->demo.finish(T, 1, E, s));
  // an adapt record's G leaves the episode formed under the shape in force OUTSIDE warm ticks again (the table itself stays): the
  // phase calls that may follow sample under it, as they would under the caller's shape without a record
  MBD_TRY(p->adapt.table(0, p->noise.shape_always(), HNu, s));
  HIP_TRY(hipStreamSynchronize(s));
  const auto t1 = std::chrono::steady_clock::now();
  if (loop_seconds_out) *loop_seconds_out = std::chrono::duration<double>(t1 - t0).count();
  HIP_TRY(p->d_mpc_rewards.download(rewards_out, (size_t)T * E));
  HIP_TRY(p->d_mpc_states.download(states_out, ((size_t)T + 1) * S));
  if (has_delay) p->delay.pred_ticks = T;
  if (p->zone.has) { p->zone.ticks = T; p->zone.exec = E; p->zone.episodes = 1; }
  if (pi) { p->sigma_rec.ticks = T; p->sigma_rec.episodes = 1; }
  if (has_plant || has_delay) {  // (the executed rows carry the action noise, or are the committed queue's: their own log)
    HIP_TRY(p->d_mpc_actions.download(actions_out, (size_t)T * EN));
    HIP_TRY(p->d_mpc_means.download(means_out, (size_t)T * HNu));
  } else if (means_out || actions_out) {  // (the executed rows are M_t[0:E]: taken from the one copy of the means)
    std::vector<float> tmp(means_out ? 0 : (size_t)T * HNu);
    float* m = means_out ? means_out : tmp.data();
    HIP_TRY(p->d_mpc_means.download(m, (size_t)T * HNu));
    if (actions_out)
      for (int t = 0; t < T; ++t) memcpy(actions_out + (size_t)t * E * Nu, m + (size_t)t * HNu, sizeof(float) * (size_t)E * Nu);
  }
  return MBD_OK;
}

// ---- sessions (include/mbd_hip.h mbd_plan_mpc_open) --------------------------------------------------------------------------
// A session is mbd_plan_run_mpc's loop with the body of one tick per call and the caller in the plant's place.  A tick enqueues,
// on the plan's stream: the upload of the state from its pinned staging buffer (one hipMemcpyAsync), with a demo record the launch
// that builds the tick's window, mpc_plan_tick — the function the batch episode runs — and mpc_session_boundary_kernel, which
// shifts the mean, advances the queue and writes the results into the mailbox; then an event.  No rollout of executed rows, no log.
// The ring of noise buffers (mbd_plan) keeps its argument, restated: the launches a tick adds are stream-ordered behind the previous
// tick's boundary and in front of the tick's first rollout, carry no progress word and no noise job, so the sequence numbers the
// host looks for count the planning rollouts alone; the host waits at every tick's end (collect, on the event), and nothing is
// enqueued between collect and the next submit, so when a tick's first step looks for the last reader of a buffer the stream is
// idle and the progress word holds the last rollout's number — the in-step form, always.  A session always declares the next
// tick's first key (it is known: the chain is host arithmetic), unless mc.n_ticks says no tick follows; the normals prepared
// beside the tick's last rollout — on the second stream for a rollout that fills the chip or a plan with a basis — are joined by
// the next tick's first step as any prepared buffer is, or regenerated when that tick turns out cold under a warm-only shape
// (the tag differs).  The bits depend on none of this.
// What close leaves behind: a session opened without a limit (n_ticks = INT32_MAX) declares a next key at EVERY tick, its last one
// included, so after close one ring buffer holds normals nobody asked for — prepared on the second stream, possibly still being
// written.  That is a stale prepared buffer like any other: its tag (key, shape, basis) matches no later step unless it IS that
// step's, the next writer of the buffer first joins the job through ring.join (obtain_normals, prepare_noise_job), and
// mbd_plan_destroy frees the buffers with hipFree, which waits for the device.  run and run_mpc after a session give a fresh
// handle's bits (tests/test_gpu_mpc_online.py).
// The materialised case (car2d; a path-integral plan with a sigma record): there is no ring.  sample_candidates writes d_Y0s on
// the plan's stream in front of the rollout that reads it, the update kernels read it behind that rollout, and the next step's
// sampler overwrites it behind them: stream order alone.  No key is declared (declare_next_key returns at once), the second
// stream is never created, the progress word is never written.  A path-integral tick adds mpc_pi_sigma_kernel in FRONT of
// mpc_session_boundary_kernel — behind the tick's last cma_sigma_kernel, whose value it reads — so the boundary stays the tick's
// last kernel and the event behind it covers the mailbox as before; the sigma kernel touches device memory only (the carried
// sigma, a two-slot log nobody reads back).  A cold tick's launch of the same kernel (sigma = sigma_cold) stands in front of the
// tick's first sampler; mbd_plan_mpc_reset_mean launches it too, between two ticks, so that mbd_plan_get_sigma already says so.
static size_t session_mailbox_floats(const mbd_plan* p, int EN) {
  return 2 * (size_t)EN + (size_t)p->HNu + (size_t)p->env->state_size() + 2;
}
static SessionMailbox session_mailbox(const mbd_plan* p, float* base, int EN) {
  SessionMailbox mb;
  mb.rows = base;
  mb.mean = mb.rows + EN;
  mb.head = mb.mean + p->HNu;
  mb.pred = mb.head + EN;
  mb.rew_mean = mb.pred + p->env->state_size();
  mb.flag = (int*)(mb.rew_mean + 1);
  return mb;
}

extern "C" int mbd_plan_mpc_open(mbd_plan* p, const mbd_mpc_config* mc, const uint32_t key[2]) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  if (!mc) return fail(MBD_ERR_INVALID, "mpc config is NULL");
  if (!key) return fail(MBD_ERR_INVALID, "key is NULL");
  const mbd_plan_config& c = p->cfg;
  MBD_TRY(check_mpc_config(c, mc, p->demo.has, p->sigma_rec.has));
  if (c.shard_count != c.Nsample)
    return fail(MBD_ERR_STATE, "shard_count=%d of Nsample=%d: receding horizon runs unsharded plans", c.shard_count, c.Nsample);
  MBD_TRY(p->delay.check_run(mc->exec_steps));
  if (p->has_plant) return fail(MBD_ERR_STATE, "mpc_open: the plan carries a plant record: in a session the caller is the plant");
  NO_SESSION(p, "mpc_open");
  mbd_env* e = p->env;
  HIP_TRY(hipSetDevice(e->device));
  MpcSession& ss = p->session;
  const int S = e->state_size(), EN = mc->exec_steps * p->Nu, Q = p->delay.D * EN;
  HIP_TRY(p->d_mpc_state.grow(2 * (size_t)S));
  if (p->delay.has) {
    HIP_TRY(p->d_mpc_queue.grow(2 * (size_t)Q));
    HIP_TRY(p->d_mpc_pred.grow(S));
  }
  HIP_TRY(ss.stage.alloc(S));
  HIP_TRY(ss.mailbox.alloc(session_mailbox_floats(p, EN)));
  if (!ss.done) HIP_TRY(ss.done.create());
  hipStream_t s = p->stream;
  if (p->delay.has) MBD_TRY(p->delay.upload(p->d_mpc_queue, 1, mc->exec_steps, p->Nu, s));
  if (c.update_method != 0) {  // (a session keeps no sigma log: one slot and its successor; mbd_plan_get_sigma: sigma_cold from here on)
    MBD_TRY(p->sigma_rec.start(1, 1));
    p->sigma_rec.launch(p->d_sigma, 1, 0, true, s);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(s));
  if (p->demo.has) MBD_TRY(p->demo.session_start());
  MBD_TRY(p->pick.start(mc->n_ticks));  // (a pick record's log: the session's ticks, the most recent kLogCap of them)
  // the objective record's previous action of the first tick, as mbd_plan_run_mpc forms it, and the session's slot until close —
  // behind everything else that can fail, and itself leaving the slot alone when it fails: a failed open leaves prev as it was
  MBD_TRY(p->obj.episode_start(p->delay.has ? p->d_mpc_queue + (Q - p->Nu) : nullptr, Q, s));
  // (nothing fails from here on: a refused or failed open leaves the last episode's logs readable)
  if (p->delay.has) p->delay.pred_ticks = 0;  // (mbd_plan_peek_mpc_predicted does not serve sessions)
  p->adapt.count = 0;                         // (an adapt record's log: the session's steps)
  p->elite.restart();                         // (an elite record's log likewise)
  ss.mc = *mc;
  ss.rng[0] = key[0]; ss.rng[1] = key[1];
  ss.t = 0; ss.qbuf = 0; ss.flags = 0;
  ss.cold = true;
  ss.in_flight = false;
  ss.open = true;
  return MBD_OK;
}

extern "C" int mbd_plan_mpc_submit(mbd_plan* p, const float* state) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  if (!state) return fail(MBD_ERR_INVALID, "state is NULL");
  MpcSession& ss = p->session;
  if (!ss.open) return fail(MBD_ERR_STATE, "mpc_submit: no session is open on this plan");
  if (ss.in_flight) return fail(MBD_ERR_STATE, "mpc_submit: a tick is in flight (mbd_plan_mpc_collect first)");
  if (ss.t >= ss.mc.n_ticks) return fail(MBD_ERR_STATE, "mpc_submit: the session has served its n_ticks=%d ticks", ss.mc.n_ticks);
  mbd_env* e = p->env;
  HIP_TRY(hipSetDevice(e->device));
  const mbd_plan_config& c = p->cfg;
  const int S = e->state_size(), E = ss.mc.exec_steps, EN = E * p->Nu, HNu = p->HNu, Nd = c.Ndiffuse;
  const bool has_delay = p->delay.has;
  const int D = p->delay.D, Q = D * EN;
  hipStream_t s = p->stream;
  ss.t_submit = std::chrono::steady_clock::now();
  int flags = ss.cold ? MBD_TICK_COLD : 0;
  for (int k = 0; k < S; ++k)
    if (!std::isfinite(state[k])) flags |= MBD_TICK_STATE_NONFINITE;
  memcpy(ss.stage.host(), state, sizeof(float) * S);
  float* s_t = p->d_mpc_state;
  HIP_TRY(hipMemcpyAsync(s_t, ss.stage.host(), sizeof(float) * S, hipMemcpyHostToDevice, s));
  if (ss.cold) HIP_TRY(hipMemsetAsync(p->d_Ybar, 0, sizeof(float) * HNu, s));
  const bool pi = c.update_method != 0;
  if (pi && ss.cold) {  // a cold tick starts from sigma_cold
    p->sigma_rec.launch(p->d_sigma, 1, 0, true, s);
    HIP_TRY(hipGetLastError());
  }
  uint32_t rng[2] = {ss.rng[0], ss.rng[1]}, r[2], after[2];  // (a copy of the chain: committed with the tick, below)
  mpc_tick_keys(c.prng_impl, rng, r, after);
  if (p->demo.has) MBD_TRY(p->demo.session_window(ss.t, E, has_delay ? D : 0, s));
  const float* q_in = has_delay ? p->d_mpc_queue + (size_t)ss.qbuf * Q : nullptr;
  float* q_out = has_delay ? p->d_mpc_queue + (size_t)(ss.qbuf ^ 1) * Q : nullptr;
  MpcTick tk;
  tk.s_t = s_t; tk.q_in = q_in; tk.shat = has_delay ? p->d_mpc_pred.get() : nullptr; tk.DE = D * E;
  tk.cold = ss.cold; tk.K = ss.mc.warm_steps; tk.E = E; tk.key_after = ss.t + 1 < ss.mc.n_ticks ? after : nullptr;
  tk.d_xref = p->demo.has ? p->demo.window(0) : nullptr;
  const float* M = nullptr;
  MBD_TRY(mpc_plan_tick(p, tk, r, s, &M));
  if (pi) {  // the next tick's sigma, in FRONT of the boundary: that stays the tick's last kernel, the one the event stands behind
    p->sigma_rec.launch(p->d_sigma, 1, 0, false, s);
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(mpc_session_boundary_kernel, dim3(1), dim3(256), 0, s, M, HNu, EN, p->d_Ybar.get(), q_in, q_out, Q,
                     has_delay ? (const float*)p->d_mpc_pred : (const float*)nullptr, S, (const float*)(p->d_rewmeans + (Nd - 2)),
                     session_mailbox(p, ss.mailbox.dev(), EN));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ss.done, s));
  ss.rng[0] = rng[0]; ss.rng[1] = rng[1];  // (a submit that failed above has not moved the chain: a retry plans tick t with k_t)
  ss.flags = flags;
  ss.in_flight = true;
  return MBD_OK;
}

extern "C" int mbd_plan_mpc_collect(mbd_plan* p, float* rows_out, float* mean_out, float* head_out, float* predicted_out,
                                    mbd_mpc_tick_info* info_out) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  MpcSession& ss = p->session;
  if (!ss.open) return fail(MBD_ERR_STATE, "mpc_collect: no session is open on this plan");
  if (!ss.in_flight) return fail(MBD_ERR_STATE, "mpc_collect: no tick is in flight (mbd_plan_mpc_submit first)");
  HIP_TRY(hipSetDevice(p->env->device));
  HIP_TRY(hipEventSynchronize(ss.done));
  const int S = p->env->state_size(), EN = ss.mc.exec_steps * p->Nu;
  const SessionMailbox mb = session_mailbox(p, ss.mailbox.host(), EN);
  if (rows_out) memcpy(rows_out, mb.rows, sizeof(float) * EN);
  if (mean_out) memcpy(mean_out, mb.mean, sizeof(float) * p->HNu);
  if (head_out) memcpy(head_out, mb.head, sizeof(float) * EN);
  if (predicted_out) memcpy(predicted_out, p->delay.has ? mb.pred : ss.stage.host(), sizeof(float) * S);
  const auto t1 = std::chrono::steady_clock::now();
  if (info_out) {
    *info_out = mbd_mpc_tick_info{};
    info_out->tick = ss.t;
    info_out->flags = ss.flags | (*mb.flag ? MBD_TICK_ROWS_NONFINITE : 0);
    info_out->rew_mean = *mb.rew_mean;
    info_out->seconds = std::chrono::duration<float>(t1 - ss.t_submit).count();
  }
  ss.in_flight = false;
  ss.cold = false;
  ss.qbuf ^= 1;
  ss.t += 1;
  return MBD_OK;
}

extern "C" int mbd_plan_mpc_tick(mbd_plan* p, const float* state, float* rows_out, float* mean_out, float* head_out,
                                 float* predicted_out, mbd_mpc_tick_info* info_out) {
  MBD_TRY(mbd_plan_mpc_submit(p, state));
  return mbd_plan_mpc_collect(p, rows_out, mean_out, head_out, predicted_out, info_out);
}

extern "C" int mbd_plan_mpc_reset_mean(mbd_plan* p) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  if (!p->session.open) return fail(MBD_ERR_STATE, "mpc_reset_mean: no session is open on this plan");
  if (p->session.in_flight) return fail(MBD_ERR_STATE, "mpc_reset_mean: a tick is in flight (mbd_plan_mpc_collect first)");
  p->session.cold = true;  // (the next submit zeroes Ybar; the queue stays)
  if (p->adapt.has) {      // (an adapt record's table is all ones again: written now as well, so that mbd_plan_peek_adapt says so)
    HIP_TRY(hipSetDevice(p->env->device));
    MBD_TRY(p->adapt.table(-1, p->noise.shape_always(), p->HNu, p->stream));
  }
  if (p->elite.has) {  // (an elite record's elites are gone: written now as well, so that mbd_plan_peek_elites says so)
    HIP_TRY(hipSetDevice(p->env->device));
    MBD_TRY(elite_table(p->elite, -1, p->HNu, p->stream));
  }
  if (p->cfg.update_method != 0) {  // (and starts from sigma_cold: written now as well, so that mbd_plan_get_sigma says so)
    HIP_TRY(hipSetDevice(p->env->device));
    p->sigma_rec.launch(p->d_sigma, 1, 0, true, p->stream);
    HIP_TRY(hipGetLastError());
  }
  return MBD_OK;
}

extern "C" int mbd_plan_mpc_close(mbd_plan* p) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  MpcSession& ss = p->session;
  if (!ss.open) return fail(MBD_ERR_STATE, "mpc_close: no session is open on this plan");
  HIP_TRY(hipSetDevice(p->env->device));
  if (ss.in_flight) HIP_TRY(hipStreamSynchronize(p->stream));  // (its last kernel writes the mailbox)
  if (p->adapt.has) {  // (as behind mbd_plan_run_mpc: G under the shape in force outside warm ticks, for the phase calls)
    MBD_TRY(p->adapt.table(0, p->noise.shape_always(), p->HNu, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
  }
  ss.in_flight = false;
  ss.open = false;
  p->obj.episode_end();
  ss.stage.release();
  ss.mailbox.release();
  return MBD_OK;
}

extern "C" int mbd_plan_eval(mbd_plan* p, const float* Y, float* rew_final_out) {
  if (!p || !Y || !rew_final_out) return fail(MBD_ERR_INVALID, "NULL argument");
  NO_SESSION(p, "eval");
  HIP_TRY(hipSetDevice(p->env->device));
  HIP_TRY(hipMemcpy(p->d_Ybar + p->HNu, Y, sizeof(float) * p->HNu, hipMemcpyHostToDevice));
  MBD_TRY(launch_rollout(p->env, p->d_state0, p->d_Ybar + p->HNu, 1, p->cfg.Hsample, nullptr, p->d_scratch, nullptr, nullptr,
                         p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  HIP_TRY(p->d_scratch.download(rew_final_out, 1));
  return MBD_OK;
}

extern "C" int mbd_plan_peek(mbd_plan* p, float* Y0s_out, float* rewss_out, float* weights_out) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  HIP_TRY(hipSetDevice(p->env->device));
  HIP_TRY(hipDeviceSynchronize());
  const mbd_plan_config& c = p->cfg;
  if (Y0s_out && p->lazy) {  // lazy plans never formed Y0s: do it now from the last step's normals, Ybar_i and sigma_i
    if (!p->peek_ybar) return fail(MBD_ERR_STATE, "peek: no diffusion step to show yet");
    const uint64_t total = (uint64_t)c.Nsample * p->HNu;
    hipLaunchKernelGGL(shift_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, p->stream,
                       p->ring.eps[p->ring.cur], p->HNu, 0ull, (unsigned long long)total, p->sigma_last,
                       (const float*)nullptr, p->peek_ybar, p->d_Y0s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(p->stream));
  }
  HIP_TRY(p->d_Y0s.download(Y0s_out, (size_t)c.Nsample * p->HNu));
  // (with an ensemble record that has stepped: member 0's rows of the launch over all members)
  const float* rewss = p->has_ens && p->ens_stepped ? p->d_ens_rewss : p->d_rewss;
  if (rewss_out) HIP_TRY(hipMemcpy(rewss_out, rewss, sizeof(float) * (size_t)c.shard_count * c.Hsample, hipMemcpyDeviceToHost));
  HIP_TRY(p->d_weights.download(weights_out, (size_t)c.Nsample));
  return MBD_OK;
}

extern "C" int mbd_plan_enable_timing(mbd_plan* p, int enable) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  p->timing.on = enable != 0;
  return MBD_OK;
}

extern "C" int mbd_plan_kernel_time(mbd_plan* p, float* avg_ms_out, int* count_out, int reset) {
  if (!p) return fail(MBD_ERR_INVALID, "plan is NULL");
  HIP_TRY(hipSetDevice(p->env->device));
  return p->timing.average(avg_ms_out, count_out, reset != 0);
}
