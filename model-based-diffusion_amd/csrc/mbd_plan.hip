// mbd_plan.hip — the planner fast path (include/mbd_hip.h): the plan handle and the noise ring of lazy plans, one
// reverse-diffusion step split at its exchange point (mbd_plan_sample_rollout / mbd_plan_score_update; the step functions
// behind them take the rollouts' start state as a parameter), and the loops over steps (mbd_plan_reverse_once, mbd_plan_run,
// mbd_plan_eval, mbd_plan_peek; the receding-horizon loop mbd_plan_run_mpc).  mbd_planner.py:84-148,179-180.
#define MBD_WEIGH_KERNEL 1  // this unit launches weigh_kernel (mbd_step_kernels.h)
#define MBD_PICK_KERNEL 1   // ... and, for plans and sweeps alike, the pick record's kernels
#define MBD_VALUE_KERNEL 1  // ... and the value record's
#define MBD_ADAPT_KERNEL 1  // ... and the adapt record's (plans only)
#define MBD_ELITE_KERNEL 1  // ... and the elite record's (plans only)
#define MBD_TOGO_KERNEL 1   // ... and the to-go record's (plans only)
#define MBD_ZONE_KERNEL 1   // ... and, for plans and sweeps alike, the zone record's
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

// A step's candidates as the launches behind its sampler are handed them (an adapt record's update, an elite record's injection
// and selection): cand [N][HNu], or their normals (lazy) with the sigma_i and Ybar_i the step sampled with — an mppi plan's sigma
// from the carried device scalar, which its sampler read (d_sigma, nullptr: the host value).
struct StepCand {
  const float* cand;
  int N, HNu, lazy;
  float sigma;
  const float* d_sigma;
  const float* ybar_i;
};

// The plan-only record, in the form of mbd_internal.h's: set behind the handle's refusals (nullptr clears), the launches a step or
// a tick makes — each returns at once without a record, and the mbd_debug_* entries run the same members on a scratch record —, and
// peek.  All zero: no record (a zeroed stand-in handle has none).
// The adapt record (include/mbd_hip.h mbd_adapt): the rule, the table a and G = a * g [HNu] on the device — G is what the samplers
// take as their shape while the record is in force (noise_spec) —, the scratch the update's two kernels hand var and s through, and
// the device log, a ring of kLogCap entries (count: steps since the log began).  g_cur: the caller's shape G was last formed under
// (the plan's d_shape or nullptr), which the update's second kernel forms G' under again.
struct AdaptRec {
  bool has = false;
  AdaptRule rule{};
  int carry = 0;
  long long count = 0;
  const float* g_cur = nullptr;
  DevBuf<float> d_a, d_G, d_buf, d_log_S;
  DevBuf<int> d_log_skipped;
  // g: the caller's shape in force outside warm ticks; the table is all ones afterwards (one launch on s, waited for)
  MBD_HIDDEN int set(const mbd_adapt* rec, int HNu, const float* g, const mbd_env* env, hipStream_t s);
  // The table at the start of a run or a tick, or under a new shape: shift < 0: a = ones, otherwise a shifted `shift` elements
  // forward (0: as it is); G = a * g under the caller's shape g now in force, which the updates that follow keep forming G under.
  // ONE launch.
  MBD_HIDDEN int table(int shift, const float* g, int HNu, hipStream_t s);
  // behind a step's update kernel, on the step's stream, from the step's weights d_w [N]: var into d_buf, then S, a', G' and the
  // log entry.  TWO launches; the weights are staged in LDS while they fit the default 48 KB window, read from memory beyond
  MBD_HIDDEN int update(const float* d_w, const StepCand& c, hipStream_t s);
  // HOST a_out [HNu] and the most recent min(count, capacity, kLogCap) log entries, oldest first
  MBD_HIDDEN int peek(const mbd_env* env, int HNu, float* a_out, float* ratio_out, int32_t* skipped_out, int capacity, int* count_out) const;
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
// the refusal of a record beside a to-go record (who: how the refused record's messages begin), and of a plan-only record on a
// sharded plan (kind: "adapt", "elite", "to-go")
int refuse_beside_togo(const char* who, const char* handle) {  // (mbd_internal.h: the sweeps' set calls refuse with the same text)
  return fail(MBD_ERR_UNSUPPORTED, "%s: the %s carries a to-go record (mbd_%s_set_togo): what the record means per horizon row is not "
                                   "defined", who, handle, handle);
}
static int refuse_sharded(const mbd_plan_config& c, const char* kind) {
  return fail(MBD_ERR_STATE, "%s record: shard_count=%d of Nsample=%d: sharded plans take no %s record", kind, c.shard_count, c.Nsample,
              kind);
}

// ==================================================================================================
// planner
// ==================================================================================================
void host_schedule(float beta0, float betaT, int Nd, std::vector<float>& alphas,
                          std::vector<float>& alphas_bar, std::vector<float>& sigmas) {
  // mbd_planner.py:84-87; jnp.linspace = start*(1-t) + stop*t with the endpoint appended
  alphas.resize(Nd); alphas_bar.resize(Nd); sigmas.resize(Nd);
  float cp = 1.0f;
  for (int i = 0; i < Nd; ++i) {
    float t = Nd > 1 ? (float)i / (float)(Nd - 1) : 0.0f;
    float beta = (i == Nd - 1 && Nd > 1) ? betaT : beta0 * (1.0f - t) + betaT * t;
    float a = 1.0f - beta;
    cp = cp * a;
    alphas[i] = a; alphas_bar[i] = cp; sigmas[i] = fsqrt(1.0f - cp);
  }
}

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

// ---- the launches of the adapt, elite and to-go records (what a step and a tick run; set, peek and the debug entries, which run
// the same members on a scratch record: below, record by record) ------------------------------------------------------------------
int AdaptRec::table(int shift, const float* g, int HNu, hipStream_t s) {
  if (!has) return MBD_OK;
  g_cur = g;
  hipLaunchKernelGGL(adapt_table_kernel, dim3(1), dim3(kAdaptThreads), 0, s, d_a.get(), d_G.get(), g, HNu, shift);
  HIP_TRY(hipGetLastError());
  return MBD_OK;
}

int AdaptRec::update(const float* d_w, const StepCand& c, hipStream_t s) {
  if (!has) return MBD_OK;
  const long long slot = ring_slot(count, kLogCap);
  const dim3 grid((c.HNu + kWmE - 1) / kWmE), block(kWmE * kWmG);
  if ((size_t)c.N * sizeof(float) <= 48 * 1024)
    hipLaunchKernelGGL(adapt_spread_kernel<true>, grid, block, sizeof(float) * (size_t)c.N, s, d_w, c.cand, c.N, c.HNu, c.ybar_i, c.lazy,
                       c.sigma, c.d_sigma, d_buf.get());
  else
    hipLaunchKernelGGL(adapt_spread_kernel<false>, grid, block, 0, s, d_w, c.cand, c.N, c.HNu, c.ybar_i, c.lazy, c.sigma, c.d_sigma,
                       d_buf.get());
  hipLaunchKernelGGL(adapt_finish_kernel, dim3(1), dim3(kAdaptThreads), 0, s, d_buf.get(), c.HNu, c.sigma, c.d_sigma, d_a.get(), g_cur,
                     d_G.get(), rule, d_log_S.get() + slot, d_log_skipped.get() + slot);
  HIP_TRY(hipGetLastError());
  return MBD_OK;
}

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

void TogoRec::layout(int block_, int min_tail_, int H) {
  block = block_; min_tail = min_tail_;
  G = togo_groups(H, block, min_tail);
  starts.resize(G);
  for (int j = 0; j < G; ++j) starts[j] = togo_start(j, block);
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

// ---- the noise shape (include/mbd_hip.h mbd_noise_shape) ----------------------------------------------------------------
int check_noise_shape(const mbd_noise_shape* rec, int Hsample, int action_size) {
  for (int r = 0; r < 5; ++r)
    if (rec->reserved[r] != 0) return fail(MBD_ERR_INVALID, "noise shape: reserved[%d]=%d: must be 0", r, rec->reserved[r]);
  if (rec->when != MBD_NOISE_ALWAYS && rec->when != MBD_NOISE_WARM_TICKS)
    return fail(MBD_ERR_INVALID, "noise shape: when=%d: MBD_NOISE_ALWAYS (0) or MBD_NOISE_WARM_TICKS (1)", rec->when);
  if (!rec->scale) return fail(MBD_ERR_INVALID, "noise shape: scale is NULL");
  if (rec->rows < 1) return fail(MBD_ERR_INVALID, "noise shape: rows=%d: must be >= 1", rec->rows);
  if (rec->cols < 1) return fail(MBD_ERR_INVALID, "noise shape: cols=%d: must be >= 1", rec->cols);
  const size_t n = (size_t)rec->rows * (size_t)rec->cols;
  for (size_t e = 0; e < n; ++e)
    if (!std::isfinite(rec->scale[e]) || rec->scale[e] < 0.0f)
      return fail(MBD_ERR_INVALID, "noise shape: scale[%d][%d]=%g: must be finite and >= 0", (int)(e / rec->cols), (int)(e % rec->cols),
                  (double)rec->scale[e]);
  if (rec->rows != Hsample) return fail(MBD_ERR_INVALID, "noise shape: rows=%d, the handle's Hsample is %d", rec->rows, Hsample);
  if (rec->cols != action_size) return fail(MBD_ERR_INVALID, "noise shape: cols=%d, the env's action_size is %d", rec->cols, action_size);
  return MBD_OK;
}

int NoiseRec::set_shape(const mbd_noise_shape* rec, int HNu, int device) {
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipDeviceSynchronize());  // (a step in flight, or normals being prepared ahead, may still read the previous table)
  has_shape = false;
  if (!rec) return MBD_OK;
  HIP_TRY(d_shape.grow(HNu));
  HIP_TRY(hipMemcpy(d_shape, rec->scale, sizeof(float) * HNu, hipMemcpyHostToDevice));
  shape_when = rec->when;
  has_shape = true;
  return MBD_OK;
}

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

// ---- the noise basis (include/mbd_hip.h mbd_noise_basis) ----------------------------------------------------------------
int check_noise_basis(const mbd_noise_basis* rec, int Hsample) {
  if (!rec->basis) return fail(MBD_ERR_INVALID, "noise basis: basis is NULL");
  if (rec->n_knots < 1 || rec->n_knots > MBD_MAX_KNOTS)
    return fail(MBD_ERR_INVALID, "noise basis: n_knots=%d outside [1, %d]", rec->n_knots, MBD_MAX_KNOTS);
  const size_t n = (size_t)Hsample * (size_t)rec->n_knots;
  for (size_t e = 0; e < n; ++e)
    if (!std::isfinite(rec->basis[e]))
      return fail(MBD_ERR_INVALID, "noise basis: basis[%d][%d]=%g: must be finite", (int)(e / rec->n_knots), (int)(e % rec->n_knots),
                  (double)rec->basis[e]);
  if (rec->when != MBD_NOISE_ALWAYS && rec->when != MBD_NOISE_WARM_TICKS)
    return fail(MBD_ERR_INVALID, "noise basis: when=%d: MBD_NOISE_ALWAYS (0) or MBD_NOISE_WARM_TICKS (1)", rec->when);
  return MBD_OK;
}

int NoiseRec::set_basis(const mbd_noise_basis* rec, int Hsample, size_t knot_z_elems, int device) {
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipDeviceSynchronize());  // (as set_shape)
  has_basis = false;
  if (!rec) return MBD_OK;
  HIP_TRY(d_basis.grow((size_t)Hsample * MBD_MAX_KNOTS));
  HIP_TRY(d_knot_z.grow(knot_z_elems));
  HIP_TRY(hipMemcpy(d_basis, rec->basis, sizeof(float) * (size_t)Hsample * (size_t)rec->n_knots, hipMemcpyHostToDevice));
  knots = rec->n_knots;
  basis_when = rec->when;
  has_basis = true;
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

// include/mbd_hip_debug.h: the same columns on the host (knot_column is host and device text) — no device is touched
extern "C" int mbd_debug_knot_noise_host(const uint32_t key[2], int impl, int N, int H, int Nu, int n_knots, const float* W,
                                         const float* g, float* z_out) {
  if (!key || !W || !z_out) return fail(MBD_ERR_INVALID, "NULL argument");
  if (N < 1 || H < 1 || Nu < 1 || n_knots < 1 || n_knots > MBD_MAX_KNOTS || (uint64_t)N * (uint64_t)H * (uint64_t)Nu > (1ull << 26))
    return fail(MBD_ERR_INVALID, "knot_noise_host: N=%d H=%d Nu=%d n_knots=%d", N, H, Nu, n_knots);
  const uint64_t cols = (uint64_t)N * (uint64_t)Nu;
  float slots[MBD_MAX_KNOTS];
  for (uint64_t col = 0; col < cols; ++col)
    knot_column(key[0], key[1], impl, cols * (uint64_t)n_knots, H, Nu, n_knots, W, g, z_out, col, slots, 1);
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

// ---- the plant record (include/mbd_hip.h mbd_mpc_plant) ----------------------------------------------------------------
int check_mpc_plant(const mbd_env* env, const mbd_mpc_plant* rec) {
  for (int r = 0; r < 3; ++r)
    if (rec->reserved[r] != 0) return fail(MBD_ERR_INVALID, "plant record: reserved[%d]=%d: must be 0", r, rec->reserved[r]);
  if (!std::isfinite(rec->act_std) || rec->act_std < 0.0f)
    return fail(MBD_ERR_INVALID, "plant record: act_std=%g: must be finite and >= 0", (double)rec->act_std);
  if (!std::isfinite(rec->kick_std) || rec->kick_std < 0.0f)
    return fail(MBD_ERR_INVALID, "plant record: kick_std=%g: must be finite and >= 0", (double)rec->kick_std);
  if (rec->kick_every < 1) return fail(MBD_ERR_INVALID, "plant record: kick_every=%d: must be >= 1", rec->kick_every);
  auto links = [](const mbd_env* e) { return e->kind == ENV_MODEL ? e->model.n_links : 0; };
  auto planar = [](const mbd_env* e) { return e->kind == ENV_MODEL && (e->model.flags & MBD_FLAG_PLANAR) ? 1 : 0; };
  const mbd_env* pe = rec->plant ? rec->plant : env;
  if (pe != env) {  // the plant executes rows planned for env and hands its states back: one topology, one device
    if (pe->device != env->device)
      return fail(MBD_ERR_INVALID, "plant record: the plant's device=%d, the planning env's is %d", pe->device, env->device);
    // (state_size is 13 n_links for a rigid-body env and 3 for car2d, which has no links: n_links covers it)
    if (links(pe) != links(env))
      return fail(MBD_ERR_INVALID, "plant record: the plant's n_links=%d (state_size=%d), the planning env's is %d (state_size=%d)",
                  links(pe), pe->state_size(), links(env), env->state_size());
    if (pe->action_size() != env->action_size())
      return fail(MBD_ERR_INVALID, "plant record: the plant's action_size=%d, the planning env's is %d", pe->action_size(),
                  env->action_size());
    if (planar(pe) != planar(env))
      return fail(MBD_ERR_INVALID, "plant record: the plant's planar flag=%d, the planning env's is %d", planar(pe), planar(env));
  }
  if (rec->kick_std > 0.0f) {  // a kick moves link 0's linear velocity: the link has to be free to translate in the model's plane
    const bool free_root = links(pe) > 0 && (pe->model.n_rot[0] == -1 || (planar(pe) && pe->model.n_slide[0] >= 2));
    if (!free_root)
      return fail(MBD_ERR_UNSUPPORTED, "plant record: kick_std=%g on env '%s', whose link 0 cannot translate freely in its plane",
                  (double)rec->kick_std, pe->name.c_str());
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

int check_mpc_config(const mbd_plan_config& c, const mbd_mpc_config* mc, bool has_demo_rec, bool has_sigma_rec, bool pi_sessions) {
  const int T = mc->n_ticks, K = mc->warm_steps, E = mc->exec_steps, Nd = c.Ndiffuse, H = c.Hsample;
  if (T < 1) return fail(MBD_ERR_INVALID, "n_ticks=%d: must be >= 1", T);
  if (K < 1 || K > Nd - 1) return fail(MBD_ERR_INVALID, "warm_steps=%d outside [1, Ndiffuse-1=%d]", K, Nd - 1);
  if (E < 1 || E >= H) return fail(MBD_ERR_INVALID, "exec_steps=%d outside [1, Hsample=%d)", E, H);
  for (int r = 0; r < 5; ++r)
    if (mc->reserved[r] != 0) return fail(MBD_ERR_INVALID, "reserved[%d]=%d: must be 0", r, mc->reserved[r]);
  if (c.enable_demo && !has_demo_rec)
    return fail(MBD_ERR_UNSUPPORTED, "enable_demo: demos are time-indexed, an episode has no clock for them: set a demo record");
  if (c.update_method != 0 && pi_sessions)
    return fail(MBD_ERR_UNSUPPORTED, "update_method=%d: sessions of sweeps run MBD plans only (a path-integral sweep runs whole "
                                     "episodes: mbd_sweep_run_mpc with a sigma record)", c.update_method);
  if (c.update_method != 0 && !has_sigma_rec)
    return fail(MBD_ERR_UNSUPPORTED, "update_method=%d: receding horizon runs a path-integral plan only with a sigma record "
                                     "(mbd_plan_set_mpc_sigma / mbd_sweep_set_mpc_sigma)", c.update_method);
  return MBD_OK;
}

// ---- the sigma record (include/mbd_hip.h mbd_mpc_sigma) ------------------------------------------------------------------
int check_mpc_sigma(const mbd_mpc_sigma* rec, int update_method) {
  if (!std::isfinite(rec->sigma_cold) || !(rec->sigma_cold > 0.0f))
    return fail(MBD_ERR_INVALID, "sigma record: sigma_cold=%g: must be finite and > 0", (double)rec->sigma_cold);
  if (!std::isfinite(rec->sigma_warm) || !(rec->sigma_warm > 0.0f))
    return fail(MBD_ERR_INVALID, "sigma record: sigma_warm=%g: must be finite and > 0", (double)rec->sigma_warm);
  if (!std::isfinite(rec->gain) || rec->gain < 0.0f)
    return fail(MBD_ERR_INVALID, "sigma record: gain=%g: must be finite and >= 0", (double)rec->gain);
  if (rec->gain > 0.0f && update_method != 2)
    return fail(MBD_ERR_INVALID, "sigma record: gain=%g with update_method=%d: only cma-es (2) changes sigma within a tick", (double)rec->gain,
                update_method);
  if (rec->gain > 0.0f && rec->sigma_warm > rec->sigma_cold)
    return fail(MBD_ERR_INVALID, "sigma record: gain=%g with sigma_warm=%g > sigma_cold=%g: the clamp needs sigma_warm <= sigma_cold",
                (double)rec->gain, (double)rec->sigma_warm, (double)rec->sigma_cold);
  for (int r = 0; r < 5; ++r)
    if (rec->reserved[r] != 0) return fail(MBD_ERR_INVALID, "sigma record: reserved[%d]=%d: must be 0", r, rec->reserved[r]);
  return MBD_OK;
}
extern "C" int mbd_debug_check_mpc_sigma(const mbd_mpc_sigma* rec, int update_method) {
  if (!rec) return fail(MBD_ERR_INVALID, "sigma record is NULL");
  return check_mpc_sigma(rec, update_method);
}
// include/mbd_hip_debug.h: the boundary function on the host (mpc_pi_next_sigma is host and device text) — no device is touched
extern "C" int mbd_debug_mpc_sigma_next(const float* sigma_end, int n, float sigma_cold, float sigma_warm, float gain, float* next_out) {
  if (!sigma_end || !next_out) return fail(MBD_ERR_INVALID, "NULL argument");
  if (n < 0) return fail(MBD_ERR_INVALID, "n=%d", n);
  for (int j = 0; j < n; ++j) next_out[j] = mpc_pi_next_sigma(sigma_end[j], sigma_cold, sigma_warm, gain);
  return MBD_OK;
}

int SigmaRec::set(const mbd_mpc_sigma* rec, int update_method) {
  if (!rec) {
    has = false;
    ticks = episodes = 0;
    return MBD_OK;
  }
  MBD_TRY(check_mpc_sigma(rec, update_method));
  cold = rec->sigma_cold; warm = rec->sigma_warm; gain = rec->gain;
  ticks = episodes = 0;
  has = true;
  return MBD_OK;
}
int SigmaRec::start(int T, int P) {
  ticks = episodes = 0;
  HIP_TRY(d_log.grow((size_t)P * 2 * ((size_t)T + 1)));
  log_ticks = T;
  return MBD_OK;
}
void SigmaRec::launch(float* d_sigma, int P, int t, bool cold_tick, hipStream_t s) const {
  hipLaunchKernelGGL(mpc_pi_sigma_kernel, dim3((P + 63) / 64), dim3(64), 0, s, d_sigma, P, d_log.get() + 2 * (size_t)t, stride(),
                     cold_tick ? 1 : 0, cold, warm, gain);
}
int SigmaRec::peek(int device, int k, float* sigmas_out, const char* what) const {
  if (!has) return fail(MBD_ERR_STATE, "peek_mpc_sigma: the %s has no sigma record", what);
  if (ticks < 1) return fail(MBD_ERR_STATE, "peek_mpc_sigma: no episode has run with the record yet");
  if (k < 0 || k >= episodes) return fail(MBD_ERR_INVALID, "peek_mpc_sigma: episode k=%d outside [0,%d)", k, episodes);
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipDeviceSynchronize());
  if (sigmas_out)
    HIP_TRY(hipMemcpy(sigmas_out, d_log.get() + (size_t)k * stride(), sizeof(float) * 2 * (size_t)ticks, hipMemcpyDeviceToHost));
  return MBD_OK;
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

// ---- the delay record (include/mbd_hip.h mbd_mpc_delay) -----------------------------------------------------------------
int check_mpc_delay(const mbd_mpc_delay* rec, int action_size) {
  if (rec->delay_ticks < 1 || rec->delay_ticks > MBD_MAX_MPC_DELAY)
    return fail(MBD_ERR_INVALID, "delay record: delay_ticks=%d outside [1, %d]", rec->delay_ticks, MBD_MAX_MPC_DELAY);
  for (int r = 0; r < 4; ++r)
    if (rec->reserved[r] != 0) return fail(MBD_ERR_INVALID, "delay record: reserved[%d]=%d: must be 0", r, rec->reserved[r]);
  if (!rec->rows0 && rec->n_rows != 0)
    return fail(MBD_ERR_INVALID, "delay record: rows0 is NULL and n_rows=%d: must then be 0", rec->n_rows);
  if (rec->rows0 && rec->n_rows < 1)
    return fail(MBD_ERR_INVALID, "delay record: n_rows=%d with rows0 given: must be >= 1", rec->n_rows);
  if (rec->rows0 && action_size > 0) {
    const size_t n = (size_t)rec->n_rows * (size_t)action_size;
    for (size_t e = 0; e < n; ++e)
      if (!std::isfinite(rec->rows0[e]))
        return fail(MBD_ERR_INVALID, "delay record: rows0[%d][%d]=%g: must be finite", (int)(e / action_size), (int)(e % action_size),
                    (double)rec->rows0[e]);
  }
  return MBD_OK;
}
extern "C" int mbd_debug_check_mpc_delay(const mbd_mpc_delay* rec, int action_size) {
  if (!rec) return fail(MBD_ERR_INVALID, "delay record is NULL");
  if (action_size < 0) return fail(MBD_ERR_INVALID, "action_size=%d", action_size);
  return check_mpc_delay(rec, action_size);
}

int DelayRec::set(const mbd_mpc_delay* rec, int action_size) {
  if (!rec) {
    *this = DelayRec{};
    return MBD_OK;
  }
  MBD_TRY(check_mpc_delay(rec, action_size));
  has = true;
  D = rec->delay_ticks;
  n_rows = rec->n_rows;
  pred_ticks = 0;
  rows0.clear();
  if (rec->rows0) rows0.assign(rec->rows0, rec->rows0 + (size_t)rec->n_rows * (size_t)action_size);
  return MBD_OK;
}
int DelayRec::check_run(int exec_steps) const {
  if (has && n_rows != 0 && n_rows != D * exec_steps)
    return fail(MBD_ERR_INVALID, "delay record: n_rows=%d, this run needs 0 or delay_ticks * exec_steps = %d * %d", n_rows, D,
                exec_steps);
  return MBD_OK;
}
int DelayRec::upload(float* d_queue, int copies, int E, int Nu, hipStream_t s) const {
  const size_t Q = (size_t)D * E * Nu;
  if (n_rows == 0) {
    HIP_TRY(hipMemsetAsync(d_queue, 0, sizeof(float) * Q * copies, s));
    return MBD_OK;
  }
  for (int k = 0; k < copies; ++k)
    HIP_TRY(hipMemcpyAsync(d_queue + (size_t)k * Q, rows0.data(), sizeof(float) * Q, hipMemcpyHostToDevice, s));
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

// ---- the demo record (include/mbd_hip.h mbd_mpc_demo) -------------------------------------------------------------------
int DemoRec::set(const mbd_env* env, const mbd_plan_config& cfg, const mbd_mpc_demo* rec) {
  if (!rec) {
    has = false;
    ticks = exec = episodes = 0;
    return MBD_OK;
  }
  if (!rec->clip) return fail(MBD_ERR_INVALID, "demo record: clip is NULL");
  if (rec->n_rows < 1) return fail(MBD_ERR_INVALID, "demo record: n_rows=%d: must be >= 1", rec->n_rows);
  if (rec->start_row < 0) return fail(MBD_ERR_INVALID, "demo record: start_row=%d: must be >= 0", rec->start_row);
  if (!std::isfinite(rec->rew_xref)) return fail(MBD_ERR_INVALID, "demo record: rew_xref=%g: must be finite", (double)rec->rew_xref);
  for (int r = 0; r < 4; ++r)
    if (rec->reserved[r] != 0) return fail(MBD_ERR_INVALID, "demo record: reserved[%d]=%d: must be 0", r, rec->reserved[r]);
  if (!env->has_xref) return fail(MBD_ERR_INVALID, "demo record: env '%s' has no xref: nothing of it follows a demonstration", env->name.c_str());
  if (!cfg.enable_demo) return fail(MBD_ERR_INVALID, "demo record: enable_demo=0: the plan does not use demos");
  const int k_ = env->kind == ENV_CAR2D ? 1 : env->model.n_track, c_ = env->kind == ENV_CAR2D ? 2 : 3;
  const size_t n = (size_t)k_ * (size_t)rec->n_rows * (size_t)c_;
  for (size_t e = 0; e < n; ++e)
    if (!std::isfinite(rec->clip[e]))
      return fail(MBD_ERR_INVALID, "demo record: clip[%d][%d][%d]=%g: must be finite", (int)(e / ((size_t)rec->n_rows * c_)),
                  (int)(e / c_ % rec->n_rows), (int)(e % c_), (double)rec->clip[e]);
  HIP_TRY(hipSetDevice(env->device));
  HIP_TRY(hipDeviceSynchronize());  // (an episode's last launch may still read the previous clip)
  has = false;
  ticks = exec = episodes = 0;
  HIP_TRY(d_clip.grow(n));
  HIP_TRY(hipMemcpy(d_clip, rec->clip, sizeof(float) * n, hipMemcpyHostToDevice));
  L = rec->n_rows; c0 = rec->start_row; K = k_; C = c_;
  rew_xref = rec->rew_xref;
  has = true;
  return MBD_OK;
}

int DemoRec::check_plant(const mbd_env* env, const mbd_env* plant) const {
  if (!has || plant == env || env->kind != ENV_MODEL) return MBD_OK;
  if (plant->model.n_track != env->model.n_track)
    return fail(MBD_ERR_INVALID, "demo record: the plant's n_track=%d, the planning env's is %d", plant->model.n_track, env->model.n_track);
  for (int k = 0; k < env->model.n_track; ++k)
    if (plant->model.track_link[k] != env->model.track_link[k])
      return fail(MBD_ERR_INVALID, "demo record: the plant's track_link[%d]=%d, the planning env's is %d", k,
                  plant->model.track_link[k], env->model.track_link[k]);
  return MBD_OK;
}

int DemoRec::start(int T, int P, int E, int D, hipStream_t s) {
  ticks = exec = episodes = 0;
  const size_t steps = (size_t)T * P * E;
  HIP_TRY(d_windows.grow((size_t)T * K * kXrefRows * C));
  HIP_TRY(d_xlog.grow(steps * K * 3));
  HIP_TRY(d_err.grow(steps * K));
  hipLaunchKernelGGL(demo_windows_kernel, dim3(demo_blocks((long long)T * K * kXrefRows)), dim3(256), 0, s, (const float*)d_clip, L, c0,
                     T, K, C, E, D, d_windows.get());
  HIP_TRY(hipGetLastError());
  return MBD_OK;
}

int DemoRec::session_start() {
  HIP_TRY(d_windows.grow((size_t)K * kXrefRows * C));
  ticks = exec = episodes = 0;  // (behind what can fail)
  return MBD_OK;
}

int DemoRec::session_window(long long t, int E, int D, hipStream_t s) {
  // windows[t][k][h] = clip[k][min(c0 + (t + D) E + h, L - 1)]: a table of one tick whose start row is the tick's own — a start
  // at or past the clip's last row reads that row for every h, so the start is clamped there and stays an int
  long long start = (long long)c0 + (t + D) * (long long)E;
  if (start > (long long)L - 1) start = (long long)L - 1;
  hipLaunchKernelGGL(demo_windows_kernel, dim3(demo_blocks((long long)K * kXrefRows)), dim3(256), 0, s, (const float*)d_clip, L,
                     (int)start, 1, K, C, E, 0, d_windows.get());
  HIP_TRY(hipGetLastError());
  return MBD_OK;
}

int DemoRec::finish(int T, int P, int E, hipStream_t s) {
  hipLaunchKernelGGL(mpc_track_err_kernel, dim3(demo_blocks((long long)T * P * E * K)), dim3(256), 0, s, (const float*)d_xlog,
                     (const float*)d_clip, L, c0, T, P, E, K, C, d_err.get());
  HIP_TRY(hipGetLastError());
  ticks = T; exec = E; episodes = P;
  return MBD_OK;
}

int DemoRec::peek(int device, int k, float* err_out, float* windows_out, const char* what) const {
  if (!has) return fail(MBD_ERR_STATE, "peek_mpc_track: the %s has no demo record", what);
  if (ticks < 1) return fail(MBD_ERR_STATE, "peek_mpc_track: no episode has run with the record yet");
  if (k < 0 || k >= episodes) return fail(MBD_ERR_INVALID, "peek_mpc_track: episode k=%d outside [0,%d)", k, episodes);
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t T = (size_t)ticks, P = (size_t)episodes, EK = (size_t)exec * K;
  if (err_out) {  // (tick-major on the device: [T][P][E][K])
    std::vector<float> tmp(T * P * EK);
    HIP_TRY(hipMemcpy(tmp.data(), d_err, sizeof(float) * tmp.size(), hipMemcpyDeviceToHost));
    for (size_t t = 0; t < T; ++t) memcpy(err_out + t * EK, tmp.data() + (t * P + (size_t)k) * EK, sizeof(float) * EK);
  }
  HIP_TRY(d_windows.download(windows_out, T * K * kXrefRows * C));
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

// ---- the objective record (include/mbd_hip.h mbd_objective) -------------------------------------------------------------
int check_objective(const mbd_objective* rec, int Hsample, int action_size, float* wsum_out) {
  for (int r = 0; r < 5; ++r)
    if (rec->reserved[r] != 0) return fail(MBD_ERR_INVALID, "objective: reserved[%d]=%d: must be 0", r, rec->reserved[r]);
  if (rec->rows != Hsample) return fail(MBD_ERR_INVALID, "objective: rows=%d, the handle's Hsample is %d", rec->rows, Hsample);
  if (rec->cols != action_size) return fail(MBD_ERR_INVALID, "objective: cols=%d, the env's action_size is %d", rec->cols, action_size);
  if (rec->row_weight)
    for (int h = 0; h < Hsample; ++h)
      if (!std::isfinite(rec->row_weight[h]) || rec->row_weight[h] < 0.0f)
        return fail(MBD_ERR_INVALID, "objective: row_weight[%d]=%g: must be finite and >= 0", h, (double)rec->row_weight[h]);
  if (rec->act_weight)
    for (int a = 0; a < action_size; ++a)
      if (!std::isfinite(rec->act_weight[a]) || rec->act_weight[a] < 0.0f)
        return fail(MBD_ERR_INVALID, "objective: act_weight[%d]=%g: must be finite and >= 0", a, (double)rec->act_weight[a]);
  if (!std::isfinite(rec->effort) || rec->effort < 0.0f)
    return fail(MBD_ERR_INVALID, "objective: effort=%g: must be finite and >= 0", (double)rec->effort);
  if (!std::isfinite(rec->rate) || rec->rate < 0.0f)
    return fail(MBD_ERR_INVALID, "objective: rate=%g: must be finite and >= 0", (double)rec->rate);
  if (rec->prev0)
    for (int a = 0; a < action_size; ++a)
      if (!std::isfinite(rec->prev0[a])) return fail(MBD_ERR_INVALID, "objective: prev0[%d]=%g: must be finite", a, (double)rec->prev0[a]);
  if (rec->row_weight) {
    float wsum = 0.0f;
    for (int h = 0; h < Hsample; ++h) wsum = wsum + rec->row_weight[h];
    if (!std::isfinite(wsum) || !(wsum > 0.0f))
      return fail(MBD_ERR_INVALID, "objective: the sum of row_weight is %g: must be finite and > 0", (double)wsum);
    if (wsum_out) *wsum_out = wsum;
  }
  return MBD_OK;
}
extern "C" int mbd_debug_check_objective(const mbd_objective* rec, int Hsample, int action_size) {
  if (!rec) return fail(MBD_ERR_INVALID, "objective record is NULL");
  if (Hsample < 0 || action_size < 0) return fail(MBD_ERR_INVALID, "Hsample=%d action_size=%d", Hsample, action_size);
  return check_objective(rec, Hsample, action_size, nullptr);
}
// include/mbd_hip_debug.h: the per-candidate functions of objective_kernel on the host (one text for host and device) over B rows
// in a loop, the actuators' terms summed in ascending order as the kernel's lanes are — no device is touched
extern "C" int mbd_debug_objective_host(const float* rewss, const float* rews, int B, int N, int H, int Nu, const float* cand, int lazy,
                                        float sigma, const float* ybar, const float* w, float wsum, const float* q, float effort,
                                        float rate, const float* prev, float* rews_out, float* ret_out, float* cost_out) {
  if (!rewss || !rews || !cand || !q || !rews_out || !ret_out || !cost_out || (lazy && !ybar))
    return fail(MBD_ERR_INVALID, "NULL argument");
  if (B < 1 || N < 1 || H < 1 || Nu < 1 || Nu > MBD_MAX_ACT) return fail(MBD_ERR_INVALID, "objective_host: B=%d N=%d H=%d Nu=%d", B, N, H, Nu);
  const bool costs = effort != 0.0f || rate != 0.0f;
  for (int b = 0; b < B; ++b) {
    const float ret = w ? objective_ret(rewss + (size_t)b * H, w, wsum, H) : rews[b];
    float c = 0.0f;
    if (costs) {
      for (int a = 0; a < Nu; ++a) {
        float eff, rat;
        objective_column(cand + (size_t)(b % N) * H * Nu, H, Nu, a, lazy, sigma, ybar, prev, eff, rat);
        c = c + objective_term(q[a], effort, eff, rate, rat);
      }
      c = c / (float)H;
    }
    rews_out[b] = costs ? ret - c : ret;
    ret_out[b] = ret;
    if (b < N) cost_out[b] = c;
  }
  return MBD_OK;
}

int ObjectiveRec::set(const mbd_objective* rec, float ws, int device, int P_, int N_, int H_, int Nu_, size_t max_rows) {
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipDeviceSynchronize());  // (a step in flight may still read the previous record's tables)
  has = false;
  stepped = false;
  prev = nullptr;
  if (!rec) return MBD_OK;
  P = P_; N = N_; H = H_; Nu = Nu_;
  HIP_TRY(d_w.grow(H));
  HIP_TRY(d_q.grow(Nu));
  HIP_TRY(d_prev0.grow((size_t)P * Nu));
  HIP_TRY(d_prev.grow((size_t)P * Nu));
  HIP_TRY(d_ret.grow((size_t)P * max_rows));
  HIP_TRY(d_cost.grow((size_t)P * N));
  has_w = rec->row_weight != nullptr;
  if (has_w) HIP_TRY(hipMemcpy(d_w, rec->row_weight, sizeof(float) * H, hipMemcpyHostToDevice));
  std::vector<float> q((size_t)Nu, 1.0f);  // (NULL: ones — x * 1 = x)
  if (rec->act_weight) q.assign(rec->act_weight, rec->act_weight + Nu);
  HIP_TRY(hipMemcpy(d_q, q.data(), sizeof(float) * Nu, hipMemcpyHostToDevice));
  has_prev0 = rec->prev0 != nullptr;
  if (has_prev0) {  // clip(prev0), one copy per plan
    std::vector<float> pv((size_t)P * Nu);
    for (size_t e = 0; e < pv.size(); ++e) pv[e] = fclip(rec->prev0[e % Nu], -1.0f, 1.0f);
    HIP_TRY(hipMemcpy(d_prev0, pv.data(), sizeof(float) * pv.size(), hipMemcpyHostToDevice));
  }
  effort = rec->effort; rate = rec->rate; wsum = ws;
  has = true;
  episode_end();
  return MBD_OK;
}

int ObjectiveRec::launch(const float* d_rewss, float* d_rews, int B, int row0, const float* d_cand, bool lazy, float sigma,
                         const float* d_ybar, long long ybar_stride, hipStream_t s) {
  ObjectiveArgs A;
  A.rewss = d_rewss; A.rews = d_rews;
  // (rows cycle through the plan's N candidates under an ensemble, B = M N; a shard's B <= N rows are its own candidates, from row0)
  A.B = B; A.N = B < N ? B : N; A.row0 = row0; A.H = H; A.Nu = Nu;
  A.cand = d_cand; A.lazy = lazy ? 1 : 0; A.sigma = sigma; A.ybar = d_ybar;
  A.w = has_w ? d_w.get() : nullptr; A.wsum = wsum;
  A.q = d_q; A.effort = effort; A.rate = rate; A.costs = costs() ? 1 : 0;
  A.prev = prev;
  A.ret_keep = d_ret; A.cost_keep = d_cost;
  if (ybar_stride < 0)
    hipLaunchKernelGGL(objective_kernel, dim3(objective_blocks(B)), dim3(kObjThreads), 0, s, A);
  else
    hipLaunchKernelGGL(objective_batch_kernel, dim3(objective_blocks(B), (unsigned)P), dim3(kObjThreads), 0, s, A, ybar_stride);
  HIP_TRY(hipGetLastError());
  rows = B;
  stepped = true;
  return MBD_OK;
}

int ObjectiveRec::launch_rows(const float* d_rewss, float* d_rews, int B, const float* d_plans, float* d_ret_keep, float* d_cost_keep,
                              bool batch, hipStream_t s) {
  ObjectiveArgs A;
  A.rewss = d_rewss; A.rews = d_rews;
  A.B = B; A.N = B; A.row0 = 0; A.H = H; A.Nu = Nu;
  A.cand = d_plans; A.lazy = 0; A.sigma = 0.0f; A.ybar = nullptr;
  A.w = has_w ? d_w.get() : nullptr; A.wsum = wsum;
  A.q = d_q; A.effort = effort; A.rate = rate; A.costs = costs() ? 1 : 0;
  A.prev = prev;
  A.ret_keep = d_ret_keep; A.cost_keep = d_cost_keep;
  if (!batch)
    hipLaunchKernelGGL(objective_kernel, dim3(objective_blocks(B)), dim3(kObjThreads), 0, s, A);
  else
    hipLaunchKernelGGL(objective_batch_kernel, dim3(objective_blocks(B), (unsigned)P), dim3(kObjThreads), 0, s, A, 0ll);
  HIP_TRY(hipGetLastError());
  return MBD_OK;
}

int ObjectiveRec::episode_start(const float* d_queue_last, long long Q, hipStream_t s) {
  if (!has) return MBD_OK;
  episode_end();  // the first tick without a delay record: clip(prev0), or none
  if (d_queue_last) {
    hipLaunchKernelGGL(objective_prev_kernel, dim3(1, (unsigned)P), dim3(64), 0, s, d_queue_last, Q, Nu, d_prev.get());
    HIP_TRY(hipGetLastError());
    prev = d_prev;
  }
  return MBD_OK;
}

int ObjectiveRec::tick_advance(const float* d_row, long long stride, hipStream_t s) {
  if (!has) return MBD_OK;
  hipLaunchKernelGGL(objective_prev_kernel, dim3(1, (unsigned)P), dim3(64), 0, s, d_row, stride, Nu, d_prev.get());
  HIP_TRY(hipGetLastError());
  prev = d_prev;
  return MBD_OK;
}

int ObjectiveRec::peek(const mbd_env* env, int k, float* ret_out, float* cost_out, const char* what) const {
  if (!has) return fail(MBD_ERR_STATE, "peek_objective: the %s has no objective record", what);
  if (!stepped) return fail(MBD_ERR_STATE, "peek_objective: no diffusion step with the record to show yet");
  if (k < 0 || k >= P) return fail(MBD_ERR_INVALID, "peek_objective: plan k=%d outside [0,%d)", k, P);
  HIP_TRY(hipSetDevice(env->device));
  HIP_TRY(hipDeviceSynchronize());
  const int nc = rows < N ? rows : N;
  if (ret_out) HIP_TRY(hipMemcpy(ret_out, d_ret.get() + (size_t)k * rows, sizeof(float) * rows, hipMemcpyDeviceToHost));
  if (cost_out) HIP_TRY(hipMemcpy(cost_out, d_cost.get() + (size_t)k * nc, sizeof(float) * nc, hipMemcpyDeviceToHost));
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

// ---- the value record (include/mbd_hip.h mbd_value) ---------------------------------------------------------------------------
int check_value(const mbd_value* rec, int state_size, bool rigid_body) {
  for (int r = 0; r < 5; ++r)
    if (rec->reserved[r] != 0) return fail(MBD_ERR_INVALID, "value: reserved[%d]=%d: must be 0", r, rec->reserved[r]);
  if (rec->n_in != state_size) return fail(MBD_ERR_INVALID, "value: n_in=%d, the env's state_size is %d", rec->n_in, state_size);
  if (rec->n_layers < 1 || rec->n_layers > MBD_VALUE_MAX_LAYERS)
    return fail(MBD_ERR_INVALID, "value: n_layers=%d: must lie in 1..%d", rec->n_layers, MBD_VALUE_MAX_LAYERS);
  for (int l = 0; l < rec->n_layers; ++l)
    if (rec->width[l] < 1 || rec->width[l] > MBD_VALUE_MAX_WIDTH)
      return fail(MBD_ERR_INVALID, "value: width[%d]=%d: must lie in 1..%d", l, rec->width[l], MBD_VALUE_MAX_WIDTH);
  if (rec->width[rec->n_layers - 1] != 1)
    return fail(MBD_ERR_INVALID, "value: width[%d]=%d: the last layer's width must be 1", rec->n_layers - 1, rec->width[rec->n_layers - 1]);
  if (rec->act != MBD_VALUE_RELU && rec->act != MBD_VALUE_TANH) return fail(MBD_ERR_INVALID, "value: act=%d: RELU (0) or TANH (1)", rec->act);
  if (rec->flags & ~MBD_VALUE_REL_XY) return fail(MBD_ERR_INVALID, "value: flags=%d: unknown bits (REL_XY 1)", rec->flags);
  if ((rec->flags & MBD_VALUE_REL_XY) && !rigid_body)
    return fail(MBD_ERR_UNSUPPORTED, "value: flags: MBD_VALUE_REL_XY needs a rigid-body env (car2d has no links)");
  if (!std::isfinite(rec->scale)) return fail(MBD_ERR_INVALID, "value: scale=%g: must be finite", (double)rec->scale);
  if (state_size > kValueMaxWidth) return fail(MBD_ERR_INVALID, "value: n_in=%d: at most %d", rec->n_in, kValueMaxWidth);
  for (int j = 0; rec->center && j < state_size; ++j)
    if (!std::isfinite(rec->center[j])) return fail(MBD_ERR_INVALID, "value: center[%d]=%g: must be finite", j, (double)rec->center[j]);
  for (int j = 0; rec->in_scale && j < state_size; ++j)
    if (!std::isfinite(rec->in_scale[j])) return fail(MBD_ERR_INVALID, "value: in_scale[%d]=%g: must be finite", j, (double)rec->in_scale[j]);
  int K = state_size;
  for (int l = 0; l < rec->n_layers; ++l) {
    const int W = rec->width[l];
    if (!rec->W[l]) return fail(MBD_ERR_INVALID, "value: W[%d] is NULL", l);
    if (!rec->b[l]) return fail(MBD_ERR_INVALID, "value: b[%d] is NULL", l);
    for (size_t e = 0; e < (size_t)W * K; ++e)
      if (!std::isfinite(rec->W[l][e]))
        return fail(MBD_ERR_INVALID, "value: W[%d][%zu][%zu]=%g: must be finite", l, e / K, e % K, (double)rec->W[l][e]);
    for (int o = 0; o < W; ++o)
      if (!std::isfinite(rec->b[l][o])) return fail(MBD_ERR_INVALID, "value: b[%d][%d]=%g: must be finite", l, o, (double)rec->b[l][o]);
    K = W;
  }
  return MBD_OK;
}
extern "C" int mbd_debug_check_value(const mbd_value* rec, int state_size, int rigid_body) {
  if (!rec) return fail(MBD_ERR_INVALID, "value record is NULL");
  if (state_size < 0) return fail(MBD_ERR_INVALID, "state_size=%d", state_size);
  return check_value(rec, state_size, rigid_body != 0);
}
// include/mbd_hip_debug.h: value_kernel's functions on the host (one text for host and device), row by row — no device is touched
extern "C" int mbd_debug_value_host(const mbd_value* rec, int rigid_body, const float* states, const float* rews, int B, float* v_out,
                                    float* rews_out) {
  if (!rec || !states || !v_out) return fail(MBD_ERR_INVALID, "NULL argument");
  if (B < 1) return fail(MBD_ERR_INVALID, "value_host: B=%d", B);
  if (rews_out && !rews) return fail(MBD_ERR_INVALID, "value_host: rews_out needs rews");
  MBD_TRY(check_value(rec, rec->n_in, rigid_body != 0));
  const int S = rec->n_in, rel = rec->flags & MBD_VALUE_REL_XY;
  std::vector<float> center((size_t)S, 0.0f), in_scale((size_t)S, 1.0f), x(kValueMaxWidth), y(kValueMaxWidth);
  if (rec->center) center.assign(rec->center, rec->center + S);
  if (rec->in_scale) in_scale.assign(rec->in_scale, rec->in_scale + S);
  for (int b = 0; b < B; ++b) {
    for (int j = 0; j < S; ++j) x[j] = value_input(states + (size_t)b * S, j, rel, center.data(), in_scale.data());
    int K = S;
    float V = 0.0f;
    for (int l = 0; l < rec->n_layers; ++l) {
      const int W = rec->width[l];
      for (int o = 0; o < W; ++o) {
        float a = rec->b[l][o];
        for (int k = 0; k < K; ++k) a = value_step(rec->W[l][(size_t)o * K + k], x[k], a);
        y[o] = l + 1 < rec->n_layers ? value_act(a, rec->act) : a;
      }
      V = y[0];
      x.swap(y);
      K = W;
    }
    v_out[b] = V;
    if (rews_out) rews_out[b] = value_add(rews[b], rec->scale, V);
  }
  return MBD_OK;
}

int ValueRec::set(const mbd_value* rec, const mbd_env* env, size_t max_rows_, int P) {
  HIP_TRY(hipSetDevice(env->device));
  HIP_TRY(hipDeviceSynchronize());  // (a step in flight may still read the previous record's net)
  has = false;
  stepped = false;
  if (!rec) return MBD_OK;
  S = rec->n_in; n_layers = rec->n_layers; act = rec->act; rel = rec->flags & MBD_VALUE_REL_XY; scale = rec->scale;
  max_rows = max_rows_;
  std::vector<float> net((size_t)2 * S);
  for (int j = 0; j < S; ++j) {
    net[j] = rec->center ? rec->center[j] : 0.0f;
    net[(size_t)S + j] = rec->in_scale ? rec->in_scale[j] : 1.0f;
  }
  int K = S;
  for (int l = 0; l < n_layers; ++l) {
    const int W = width[l] = rec->width[l];
    off_W[l] = net.size();
    net.resize(net.size() + (size_t)K * W);
    for (int o = 0; o < W; ++o)  // transposed: Wt[k][o]
      for (int k = 0; k < K; ++k) net[off_W[l] + (size_t)k * W + o] = rec->W[l][(size_t)o * K + k];
    off_b[l] = net.size();
    net.insert(net.end(), rec->b[l], rec->b[l] + W);
    K = W;
  }
  HIP_TRY(d_net.upload(net.data(), net.size()));
  HIP_TRY(d_final.grow(max_rows * S));
  HIP_TRY(d_v.grow(max_rows));
  HIP_TRY(d_pick_final.grow((size_t)3 * P * S));
  HIP_TRY(d_pick_v.grow((size_t)3 * P));
  has = true;
  return MBD_OK;
}

// The tile: how many rows a workgroup takes.  More rows reuse a weight more often, leave fewer workgroups and make each one's
// chain of dependent loads longer.  Measured (docs/experiments.md section 26): 4 rows beat 8 and 16 at 1024 rows and at 4096, where
// even 16 rows leave every CU a workgroup — the launch is bound by the latency of its weight loads, not by their volume — so 4 it
// is.  The lever MBD_VALUE_TILE = 8 / 16 selects the other instantiations for tests and A/B runs (the bits do not depend on it: a
// row's chains are its own whatever the tile).
static int value_tile() {
  const int forced = lever("MBD_VALUE_TILE");
  return (forced == 8 || forced == 16) ? forced : 4;
}

int ValueRec::launch(const float* d_fin, float* d_rews, int B, float* d_v_keep, hipStream_t s) const {
  if (!has) return MBD_OK;
  ValueArgs A;
  A.fin = d_fin; A.rews = d_rews; A.v_keep = d_v_keep;
  A.B = B; A.S = S; A.n_layers = n_layers; A.act = act; A.rel = rel ? 1 : 0; A.scale = scale;
  int widest = 64;  // threads: the widest hidden layer, in whole wavefronts (the staging loop and the last layer take any count >= 16)
  for (int l = 0; l < kValueMaxLayers; ++l) {
    A.width[l] = l < n_layers ? width[l] : 0;
    A.Wt[l] = l < n_layers ? d_net.get() + off_W[l] : nullptr;
    A.b[l] = l < n_layers ? d_net.get() + off_b[l] : nullptr;
    if (l + 1 < n_layers && width[l] > widest) widest = width[l];
  }
  A.center = d_net.get();
  A.in_scale = d_net.get() + S;
  const dim3 block((unsigned)((widest + 63) / 64 * 64));
  const int C = value_tile();
  const dim3 grid((unsigned)((B + C - 1) / C));
  if (C == 16) hipLaunchKernelGGL(value_kernel<16>, grid, block, 0, s, A);
  else if (C == 8) hipLaunchKernelGGL(value_kernel<8>, grid, block, 0, s, A);
  else hipLaunchKernelGGL(value_kernel<4>, grid, block, 0, s, A);
  HIP_TRY(hipGetLastError());
  return MBD_OK;
}

int ValueRec::peek(const mbd_env* env, float* v_out, const char* what) const {
  if (!has) return fail(MBD_ERR_STATE, "peek_value: the %s has no value record", what);
  if (!stepped) return fail(MBD_ERR_STATE, "peek_value: no diffusion step with the record to show yet");
  HIP_TRY(hipSetDevice(env->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(d_v.download(v_out, rows));
  return MBD_OK;
}

int ValueRec::eval(const mbd_env* env, const float* states, int B, float* v_out, const char* what) {
  if (!states || !v_out) return fail(MBD_ERR_INVALID, "eval_value: NULL argument");
  if (B < 1) return fail(MBD_ERR_INVALID, "eval_value: B=%d", B);
  if (!has) return fail(MBD_ERR_STATE, "eval_value: the %s has no value record", what);
  HIP_TRY(hipSetDevice(env->device));
  HIP_TRY(d_eval_in.grow((size_t)B * S));
  HIP_TRY(d_eval_v.grow(B));
  HIP_TRY(hipMemcpy(d_eval_in, states, sizeof(float) * (size_t)B * S, hipMemcpyHostToDevice));
  MBD_TRY(launch(d_eval_in, nullptr, B, d_eval_v, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(d_eval_v.download(v_out, B));
  return MBD_OK;
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

// ---- the zone record (include/mbd_hip.h mbd_zones) ----------------------------------------------------------------------------
int check_zones(const mbd_zones* rec, int n_track) {
  if (rec->n_zones < 1 || rec->n_zones > MBD_MAX_ZONES)
    return fail(MBD_ERR_INVALID, "zones: n_zones=%d: must lie in 1..%d", rec->n_zones, MBD_MAX_ZONES);
  for (int r = 0; r < 3; ++r)
    if (rec->reserved[r] != 0) return fail(MBD_ERR_INVALID, "zones: reserved[%d]=%d: must be 0", r, rec->reserved[r]);
  for (int z = 0; z < rec->n_zones; ++z) {
    const mbd_zone& zn = rec->zone[z];
    if (zn.kind != MBD_ZONE_KEEP_OUT && zn.kind != MBD_ZONE_GOAL)
      return fail(MBD_ERR_INVALID, "zones: zone[%d].kind=%d: KEEP_OUT (0) or GOAL (1)", z, zn.kind);
    if (zn.links == 0u) return fail(MBD_ERR_INVALID, "zones: zone[%d].links=0: at least one track slot", z);
    if (n_track < 32 && (zn.links >> n_track) != 0u)
      return fail(MBD_ERR_INVALID, "zones: zone[%d].links=0x%x: a bit at or above the env's n_track=%d", z, zn.links, n_track);
    for (int i = 0; i < 3; ++i)
      if (!std::isfinite(zn.center[i]))
        return fail(MBD_ERR_INVALID, "zones: zone[%d].center[%d]=%g: must be finite", z, i, (double)zn.center[i]);
    for (int i = 0; i < 3; ++i)
      if (!std::isfinite(zn.scale[i]) || zn.scale[i] < 0.0f)
        return fail(MBD_ERR_INVALID, "zones: zone[%d].scale[%d]=%g: must be finite and >= 0", z, i, (double)zn.scale[i]);
    if (zn.scale[0] == 0.0f && zn.scale[1] == 0.0f && zn.scale[2] == 0.0f)
      return fail(MBD_ERR_INVALID, "zones: zone[%d].scale: all three entries are 0", z);
    if (!std::isfinite(zn.radius) || zn.radius < 0.0f)
      return fail(MBD_ERR_INVALID, "zones: zone[%d].radius=%g: must be finite and >= 0", z, (double)zn.radius);
    if (!std::isfinite(zn.margin) || !(zn.margin > 0.0f))
      return fail(MBD_ERR_INVALID, "zones: zone[%d].margin=%g: must be finite and > 0", z, (double)zn.margin);
    if (!std::isfinite(zn.weight) || zn.weight < 0.0f)
      return fail(MBD_ERR_INVALID, "zones: zone[%d].weight=%g: must be finite and >= 0", z, (double)zn.weight);
    if (zn.reserved != 0) return fail(MBD_ERR_INVALID, "zones: zone[%d].reserved=%d: must be 0", z, zn.reserved);
  }
  return MBD_OK;
}
extern "C" int mbd_debug_check_zones(const mbd_zones* rec, int n_track) {
  if (!rec) return fail(MBD_ERR_INVALID, "zone record is NULL");
  if (n_track < 0 || n_track > MBD_MAX_TRACK) return fail(MBD_ERR_INVALID, "check_zones: n_track=%d outside [0, %d]", n_track, MBD_MAX_TRACK);
  return check_zones(rec, n_track);
}
static int check_zones_args(const char* what, const mbd_zones* rec, const float* xpos, int B, int H, int K) {
  if (!rec || !xpos) return fail(MBD_ERR_INVALID, "%s: NULL argument", what);
  if (B < 1 || H < 1 || K < 1 || K > MBD_MAX_TRACK || (long long)B * H * K > (1ll << 26))
    return fail(MBD_ERR_INVALID, "%s: B=%d H=%d K=%d (K <= %d, B H K <= 2^26)", what, B, H, K, MBD_MAX_TRACK);
  return check_zones(rec, K);
}
// include/mbd_hip_debug.h: zones_kernel's functions on the host (one text for host and device), row by row in the kernel's order —
// no device is touched
extern "C" int mbd_debug_zones_host(const mbd_zones* rec, const float* xpos, const float* rews, int B, int H, int K, float* rews_out,
                                    float* pen_out, float* clr_out, float* step_pen_out, float* step_clr_out) {
  MBD_TRY(check_zones_args("zones_host", rec, xpos, B, H, K));
  if (rews_out && !rews) return fail(MBD_ERR_INVALID, "zones_host: rews_out needs rews");
  for (int b = 0; b < B; ++b) {
    float pen = 0.0f, clr = __builtin_inff();
    for (int t = 0; t < H; ++t) {
      const size_t at = (size_t)b * H + t;
      float s_t, c_t;
      zone_step(xpos + at * K * 3, K, *rec, s_t, c_t);
      if (step_pen_out) step_pen_out[at] = s_t;
      if (step_clr_out) step_clr_out[at] = zone_canon(c_t);
      pen = pen + s_t;
      clr = zone_min(clr, c_t);
    }
    pen = pen / (float)H;
    if (pen_out) pen_out[b] = pen;
    if (clr_out) clr_out[b] = zone_canon(clr);
    if (rews_out) rews_out[b] = rews[b] - pen;
  }
  return MBD_OK;
}

int ZoneRec::launch(const float* d_xp, float* d_rews, int B, int H_, float* d_pen_keep, float* d_clr_keep, float* d_step_pen,
                    float* d_step_clr, hipStream_t s) const {
  ZoneArgs A;
  A.xpos = d_xp; A.rews = d_rews; A.pen_keep = d_pen_keep; A.clr_keep = d_clr_keep; A.step_pen = d_step_pen; A.step_clr = d_step_clr;
  A.B = B; A.H = H_; A.K = K;
  A.Z = tab;
  hipLaunchKernelGGL(zones_kernel, dim3((unsigned)((B + kZoneRows - 1) / kZoneRows)), dim3(64 * kZoneRows), 0, s, A);
  HIP_TRY(hipGetLastError());
  return MBD_OK;
}
// include/mbd_hip_debug.h: the kernel alone on the same arguments; what is read back is filled with all-ones bits first
extern "C" int mbd_debug_zones_step(const mbd_zones* rec, const float* xpos, const float* rews, int B, int H, int K, float* rews_out,
                                    float* pen_out, float* clr_out, float* step_pen_out, float* step_clr_out) {
  MBD_TRY(check_zones_args("zones_step", rec, xpos, B, H, K));
  if (rews_out && !rews) return fail(MBD_ERR_INVALID, "zones_step: rews_out needs rews");
  if (device_count_quiet() < 1) return fail(MBD_ERR_NO_DEVICE, "zones_step: no gfx950 device visible (there is no CPU fallback)");
  ZoneRec zr;
  zr.tab = *rec;
  zr.K = K;
  DevBuf<float> d_x, d_rews, d_pen, d_clr, d_sp, d_sc;
  const size_t BH = (size_t)B * H;
  HIP_TRY(d_x.upload(xpos, BH * K * 3));
  if (rews) HIP_TRY(d_rews.upload(rews, B));
  HIP_TRY(d_pen.alloc_poisoned(B));
  HIP_TRY(d_clr.alloc_poisoned(B));
  HIP_TRY(d_sp.alloc_poisoned(BH));
  HIP_TRY(d_sc.alloc_poisoned(BH));
  MBD_TRY(zr.launch(d_x, rews ? d_rews.get() : nullptr, B, H, d_pen, d_clr, d_sp, d_sc, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  if (rews) HIP_TRY(d_rews.download(rews_out, B));
  HIP_TRY(d_pen.download(pen_out, B));
  HIP_TRY(d_clr.download(clr_out, B));
  HIP_TRY(d_sp.download(step_pen_out, BH));
  HIP_TRY(d_sc.download(step_clr_out, BH));
  return MBD_OK;
}

int ZoneRec::set(const mbd_zones* rec, const mbd_env* env, size_t max_rows, int H_) {
  HIP_TRY(hipSetDevice(env->device));
  HIP_TRY(hipDeviceSynchronize());  // (a step in flight may still write the previous record's buffers)
  has = false;
  stepped = false;
  ticks = exec = episodes = 0;
  if (!rec) return MBD_OK;
  K = env->model.n_track;
  H = H_;
  HIP_TRY(d_x.grow(max_rows * H * K * 3));
  HIP_TRY(d_pen.grow(max_rows));
  HIP_TRY(d_clr.grow(max_rows));
  tab = *rec;
  has = true;
  return MBD_OK;
}

int ZoneRec::update(const mbd_zones* rec, const mbd_env* env, const char* what) {
  if (!rec) return fail(MBD_ERR_INVALID, "update_zones: zone record is NULL");
  if (!has) return fail(MBD_ERR_STATE, "update_zones: the %s has no zone record (mbd_%s_set_zones first)", what, what);
  MBD_TRY(check_zones(rec, env->model.n_track));
  tab = *rec;  // (launches already enqueued carry the table they were launched with)
  return MBD_OK;
}

int ZoneRec::check_plant(const mbd_env* env, const mbd_env* plant) const {
  if (!has || plant == env) return MBD_OK;
  if (plant->model.n_track != env->model.n_track)
    return fail(MBD_ERR_INVALID, "zone record: the plant's n_track=%d, the planning env's is %d", plant->model.n_track, env->model.n_track);
  for (int k = 0; k < env->model.n_track; ++k)
    if (plant->model.track_link[k] != env->model.track_link[k])
      return fail(MBD_ERR_INVALID, "zone record: the plant's track_link[%d]=%d, the planning env's is %d", k,
                  plant->model.track_link[k], env->model.track_link[k]);
  return MBD_OK;
}

int ZoneRec::start(int T, int P, int E) {
  ticks = exec = episodes = 0;
  if (!has) return MBD_OK;
  const size_t steps = (size_t)T * P * E;
  HIP_TRY(d_xlog.grow(steps * K * 3));
  HIP_TRY(d_log_pen.grow(steps));
  HIP_TRY(d_log_clr.grow(steps));
  return MBD_OK;
}

int ZoneRec::log(int t, int P, int E, hipStream_t s) const {
  if (!has) return MBD_OK;
  const size_t at = (size_t)t * P * E;
  return launch(xlog(t, P, E), nullptr, P, E, nullptr, nullptr, d_log_pen.get() + at, d_log_clr.get() + at, s);
}

int ZoneRec::peek(const mbd_env* env, int k, int N, float* pen_out, float* clr_out, const char* what) const {
  if (!has) return fail(MBD_ERR_STATE, "peek_zones: the %s has no zone record", what);
  if (!stepped) return fail(MBD_ERR_STATE, "peek_zones: no diffusion step with the record to show yet");
  HIP_TRY(hipSetDevice(env->device));
  HIP_TRY(hipDeviceSynchronize());
  if (pen_out) HIP_TRY(hipMemcpy(pen_out, d_pen.get() + (size_t)k * N, sizeof(float) * N, hipMemcpyDeviceToHost));
  if (clr_out) HIP_TRY(hipMemcpy(clr_out, d_clr.get() + (size_t)k * N, sizeof(float) * N, hipMemcpyDeviceToHost));
  return MBD_OK;
}

int ZoneRec::peek_mpc(const mbd_env* env, int k, float* pen_out, float* clr_out, const char* what) const {
  if (!has) return fail(MBD_ERR_STATE, "peek_mpc_zones: the %s has no zone record", what);
  if (!ticks) return fail(MBD_ERR_STATE, "peek_mpc_zones: no episode has run with the record yet");
  HIP_TRY(hipSetDevice(env->device));
  HIP_TRY(hipDeviceSynchronize());
  for (int t = 0; t < ticks; ++t) {  // the log is tick-major [T][P][E]
    const size_t at = ((size_t)t * episodes + k) * exec;
    if (pen_out) HIP_TRY(hipMemcpy(pen_out + (size_t)t * exec, d_log_pen.get() + at, sizeof(float) * exec, hipMemcpyDeviceToHost));
    if (clr_out) HIP_TRY(hipMemcpy(clr_out + (size_t)t * exec, d_log_clr.get() + at, sizeof(float) * exec, hipMemcpyDeviceToHost));
  }
  return MBD_OK;
}

// the refusals of a zone record a handle's env and config decide (plans and sweeps alike), behind check_zones
int check_zones_handle(const mbd_env* env, const mbd_plan_config& c, const char* handle) {
  if (env && env->kind == ENV_CAR2D) return fail(MBD_ERR_UNSUPPORTED, "zone record: car2d has no tracked links");
  if (!env || env->model.n_track < 1)
    return fail(MBD_ERR_UNSUPPORTED, "zone record: the env's model tracks no link (n_track=0): compile planar models planar=False with "
                                     "track_names");
  if (c.enable_demo) return fail(MBD_ERR_UNSUPPORTED, "zone record: the %s was created with enable_demo: demo plans are out of scope", handle);
  return MBD_OK;
}
int refuse_beside_zones(const char* who, const char* handle) {
  return fail(MBD_ERR_UNSUPPORTED, "%s: the %s carries a zone record (mbd_%s_set_zones): the pair is out of scope", who, handle, handle);
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

// ---- the weighting record (include/mbd_hip.h mbd_weighting) --------------------------------------------------------------
int check_weighting(const mbd_weighting* rec) {
  for (int r = 0; r < 6; ++r)
    if (rec->reserved[r] != 0) return fail(MBD_ERR_INVALID, "weighting: reserved[%d]=%d: must be 0", r, rec->reserved[r]);
  if (rec->reject_nonfinite != 0 && rec->reject_nonfinite != 1)
    return fail(MBD_ERR_INVALID, "weighting: reject_nonfinite=%d: must be 0 or 1", rec->reject_nonfinite);
  if (!std::isfinite(rec->ess_frac) || rec->ess_frac < 0.0f || rec->ess_frac > 1.0f)
    return fail(MBD_ERR_INVALID, "weighting: ess_frac=%g: must lie in [0, 1]", (double)rec->ess_frac);
  if (rec->ess_frac > 0.0f) {
    if (!std::isfinite(rec->temp_min) || !(rec->temp_min > 0.0f))
      return fail(MBD_ERR_INVALID, "weighting: temp_min=%g: must be finite and > 0", (double)rec->temp_min);
    if (!std::isfinite(rec->temp_max) || !(rec->temp_max >= rec->temp_min))
      return fail(MBD_ERR_INVALID, "weighting: temp_max=%g: must be finite and >= temp_min=%g", (double)rec->temp_max,
                  (double)rec->temp_min);
    if (rec->iters < 1 || rec->iters > 32) return fail(MBD_ERR_INVALID, "weighting: iters=%d: must lie in 1..32", rec->iters);
  }
  return MBD_OK;
}
static WeighRec weigh_rec_of(const mbd_weighting* rec) {
  WeighRec R{};
  if (rec) {
    R.reject = rec->reject_nonfinite; R.ess_frac = rec->ess_frac; R.temp_min = rec->temp_min; R.temp_max = rec->temp_max;
    R.iters = rec->iters;
  }
  return R;
}

// include/mbd_hip_debug.h: weigh_kernel on the host.  The reductions of the kernel's workgroup, restated: partial t of 1024 takes
// the entries i = t, t + 1024, ... in ascending i, each wavefront's 64 partials go through the xor-butterfly — at every stage lane l
// takes x[l] (+ or max) x[l ^ off], so every lane ends with the same value —, and the 16 wavefront values are combined in order.
namespace {
struct HostBlock {
  float part[kScoreThreads];
  template <class Op> float reduce(Op op) {
    float wave[kScoreThreads / 64];
    for (int w = 0; w < kScoreThreads / 64; ++w) {
      float x[64], y[64];
      for (int l = 0; l < 64; ++l) x[l] = part[w * 64 + l];
      for (int off = 32; off >= 1; off >>= 1) {
        for (int l = 0; l < 64; ++l) y[l] = op(x[l], x[l ^ off]);
        for (int l = 0; l < 64; ++l) x[l] = y[l];
      }
      wave[w] = x[0];
    }
    float s = wave[0];
    for (int w = 1; w < kScoreThreads / 64; ++w) s = op(s, wave[w]);
    return s;
  }
  float sum() { return reduce([](float a, float b) { return a + b; }); }
  float max() { return reduce([](float a, float b) { return fmax_(a, b); }); }
  void fill(float v) { for (int t = 0; t < kScoreThreads; ++t) part[t] = v; }
};
}  // namespace
extern "C" int mbd_debug_weighting_host(const float* rews, int N, float temp, int std_guard, const mbd_weighting* rec,
                                        float* weights_out, float* rew_mean_out, float* temp_out, float* ess_out, int32_t* kept_out) {
  (void)std_guard;
  if (!rews || N < 1) return fail(MBD_ERR_INVALID, "weighting_host: rews=%p N=%d", (const void*)rews, N);
  if (rec) MBD_TRY(check_weighting(rec));
  const WeighRec R = weigh_rec_of(rec);
  std::vector<float> e((size_t)N, 0.0f);
  std::vector<char> keep((size_t)N);
  HostBlock a, b;
  int kept = 0;
  a.fill(0.0f); b.fill(-__builtin_inff());
  for (int i = 0; i < N; ++i) {
    keep[i] = weigh_keep(rews[i], R.reject) ? 1 : 0;
    if (!keep[i]) continue;
    ++kept;
    a.part[i % kScoreThreads] = a.part[i % kScoreThreads] + rews[i];
    b.part[i % kScoreThreads] = fmax_(b.part[i % kScoreThreads], rews[i]);
  }
  const float sum = a.sum(), rmax = b.max();
  if (kept == 0) {
    if (weights_out) for (int i = 0; i < N; ++i) weights_out[i] = 0.0f;
    if (rew_mean_out) *rew_mean_out = __builtin_nanf("");
    if (temp_out) *temp_out = temp;
    if (ess_out) *ess_out = 0.0f;
    if (kept_out) *kept_out = 0;
    return MBD_OK;
  }
  const float mean = sum / (float)kept;
  a.fill(0.0f);
  for (int i = 0; i < N; ++i)
    if (keep[i]) a.part[i % kScoreThreads] = weigh_dev(a.part[i % kScoreThreads], rews[i], mean);
  const float sd = weigh_sd(a.sum(), kept);
  const float zmax = weigh_z(rmax, mean, sd);
  float S1 = 0.0f;
  auto pass = [&](float T) {
    a.fill(0.0f); b.fill(0.0f);
    for (int i = 0; i < N; ++i) {
      e[i] = keep[i] ? weigh_e(weigh_z(rews[i], mean, sd), zmax, T) : 0.0f;
      if (!keep[i]) continue;
      a.part[i % kScoreThreads] = a.part[i % kScoreThreads] + e[i];
      b.part[i % kScoreThreads] = b.part[i % kScoreThreads] + e[i] * e[i];
    }
    S1 = a.sum();
    return weigh_ess(S1, b.sum());
  };
  const float Ts = weigh_select(R, temp, kept, pass);
  const float ess = pass(Ts);
  if (weights_out) for (int i = 0; i < N; ++i) weights_out[i] = keep[i] ? e[i] / S1 : 0.0f;
  if (rew_mean_out) *rew_mean_out = mean;
  if (temp_out) *temp_out = Ts;
  if (ess_out) *ess_out = ess;
  if (kept_out) *kept_out = kept;
  return MBD_OK;
}

// (N is no longer read — the launching unit raises weigh_kernel's LDS window, mbd_plan_set_weighting — and stays in the signature:
// the member is one of the library's symbols, and the symbol list does not change)
int WeightingRec::set(const mbd_weighting* r, int device, int P_, int cap_, int N) {
  (void)N;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipDeviceSynchronize());  // (a step in flight may still write the log)
  has = false;
  count = 0;
  if (!r) return MBD_OK;
  P = P_; cap = cap_;
  HIP_TRY(d_temp.grow((size_t)P * cap));
  HIP_TRY(d_ess.grow((size_t)P * cap));
  HIP_TRY(d_kept.grow((size_t)P * cap));
  rec = weigh_rec_of(r);
  has = true;
  return MBD_OK;
}

int WeightingRec::peek(const mbd_env* env, int k, float* temp_out, float* ess_out, int32_t* kept_out, int capacity, int* count_out,
                       const char* what) const {
  if (!has) return fail(MBD_ERR_STATE, "peek_weighting: the %s has no weighting record", what);
  if (k < 0 || k >= P) return fail(MBD_ERR_INVALID, "peek_weighting: plan k=%d outside [0,%d)", k, P);
  if (capacity < 0) return fail(MBD_ERR_INVALID, "peek_weighting: capacity=%d", capacity);
  HIP_TRY(hipSetDevice(env->device));
  HIP_TRY(hipDeviceSynchronize());
  const int n = count < capacity ? count : capacity;
  const size_t off = (size_t)k * cap;
  if (n > 0 && temp_out) HIP_TRY(hipMemcpy(temp_out, d_temp.get() + off, sizeof(float) * n, hipMemcpyDeviceToHost));
  if (n > 0 && ess_out) HIP_TRY(hipMemcpy(ess_out, d_ess.get() + off, sizeof(float) * n, hipMemcpyDeviceToHost));
  if (n > 0 && kept_out) HIP_TRY(hipMemcpy(kept_out, d_kept.get() + off, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  if (count_out) *count_out = count;
  return MBD_OK;
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

// ---- the pick record (include/mbd_hip.h mbd_mpc_pick) ------------------------------------------------------------------------
int check_mpc_pick(const mbd_mpc_pick* rec) {
  const int all = MBD_PICK_MEAN | MBD_PICK_PREV | MBD_PICK_BEST;
  if (rec->candidates == 0) return fail(MBD_ERR_INVALID, "mpc pick: candidates=0: at least one of MEAN (1), PREV (2), BEST (4)");
  if (rec->candidates & ~all) return fail(MBD_ERR_INVALID, "mpc pick: candidates=%d: unknown bits (MEAN 1, PREV 2, BEST 4)", rec->candidates);
  for (int r = 0; r < 7; ++r)
    if (rec->reserved[r] != 0) return fail(MBD_ERR_INVALID, "mpc pick: reserved[%d]=%d: must be 0", r, rec->reserved[r]);
  return MBD_OK;
}

int PickRec::set(const mbd_mpc_pick* rec, int device, int P_, int HNu_, int H_) {
  if (!rec) {
    has = false;
    return MBD_OK;
  }
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipDeviceSynchronize());
  has = false;
  P = P_; HNu = HNu_; H = H_;
  HIP_TRY(d_slots.grow((size_t)P * 3 * HNu));
  HIP_TRY(d_rets.grow((size_t)P * 3));
  HIP_TRY(d_rewss.grow((size_t)P * 3 * H));
  HIP_TRY(d_obj_ret.grow((size_t)P * 3));
  HIP_TRY(d_obj_cost.grow((size_t)P * 3));
  HIP_TRY(d_best.grow(P));
  mask = rec->candidates;
  cap = 0;
  count = 0;
  has = true;
  return MBD_OK;
}

int PickRec::start(long long n_ticks) {
  if (!has) return MBD_OK;
  const int want = (int)(n_ticks < kLogCap ? (n_ticks < 1 ? 1 : n_ticks) : kLogCap);
  HIP_TRY(d_log_choice.grow((size_t)P * want));
  HIP_TRY(d_log_rets.grow((size_t)P * want * 3));
  HIP_TRY(d_log_best.grow((size_t)P * want));
  cap = want;
  count = 0;
  return MBD_OK;
}

// A tick's pick, on the tick's stream behind its last update kernel: pick_gather_kernel (n* and the three slots of every plan),
// ONE rollout launch of the plan's env over the 3 P slots from the states the tick planned from — no progress word, no noise job,
// like a delay record's prediction launch —, under an objective record its launch over those rows with the tick's previous action,
// and pick_choose_kernel.  Stream order is the whole argument: the gather reads the last step's rewards, normals and Ybar_i behind
// that step's weighted mean — the buffer of normals is next written two steps later, by a job that is ordered behind the NEXT
// rollout launch of the handle or behind a mark on this stream, both behind this launch —, and the choose kernel writes P_t over
// M_t in front of everything that reads it: the objective's next prev, the boundary kernels, the execution of the rows.
// Under a value record the slots' rollout writes their final states and the value launch follows the objective's, as in a step: the
// three returns are what the planner maximises.
int PickRec::tick(mbd_env* env, ObjectiveRec& obj, const ValueRec& val, const PickTick& tk, hipStream_t s) {
  if (!has) return MBD_OK;
  if (cap < 1) return fail(MBD_ERR_STATE, "mpc pick: the record's log was not started");
  const int S = env->state_size();
  PickGather G;
  G.rews = tk.rews; G.rews_stride = tk.N; G.N = tk.N; G.HNu = HNu;
  G.cand = tk.cand; G.cand_stride = (long long)tk.N * HNu; G.lazy = tk.lazy ? 1 : 0; G.sigma = tk.sigma;
  G.ybar_i = tk.ybar_i; G.ybar_i_stride = tk.ybar_i_stride;
  G.M = tk.M; G.M_stride = tk.M_stride; G.B = tk.B; G.B_stride = tk.B_stride;
  G.cold = tk.cold;
  G.slots = d_slots; G.best = d_best;
  hipLaunchKernelGGL(pick_gather_kernel, dim3(1, (unsigned)P), dim3(kScoreThreads), 0, s, G);
  HIP_TRY(hipGetLastError());
  const int sw[3] = {3, S, 0};  // (a sweep of three-candidate plans: plan k's slots start from plan k's state)
  MBD_TRY(launch_rollout(env, tk.state, d_slots, 3 * P, H, d_rewss, d_rets, nullptr, val.pick_final(), s, nullptr, P > 1 ? sw : nullptr));
  if (obj.has) MBD_TRY(obj.launch_rows(d_rewss, d_rets, 3, d_slots, d_obj_ret, d_obj_cost, P > 1, s));
  MBD_TRY(val.launch(val.pick_final(), d_rets, 3 * P, val.d_pick_v, s));
  const long long at = count % cap;  // (ring_slot's slot; count advances behind the launch check)
  PickChoose C;
  C.rets = d_rets; C.slots = d_slots; C.best = d_best; C.HNu = HNu; C.mask = mask; C.cold = tk.cold;
  C.out = tk.M; C.out_stride = tk.M_stride;
  C.log_choice = d_log_choice.get() + at; C.log_rets = d_log_rets.get() + at * 3; C.log_best = d_log_best.get() + at;
  C.log_stride = cap;
  hipLaunchKernelGGL(pick_choose_kernel, dim3(1, (unsigned)P), dim3(256), 0, s, C);
  HIP_TRY(hipGetLastError());
  count += 1;
  return MBD_OK;
}

int PickRec::peek(const mbd_env* env, int k, int32_t* choice_out, float* rets_out, int32_t* best_out, int capacity, int* count_out,
                  const char* what) const {
  if (!has) return fail(MBD_ERR_STATE, "peek_mpc_pick: the %s has no pick record", what);
  if (k < 0 || k >= P) return fail(MBD_ERR_INVALID, "peek_mpc_pick: plan k=%d outside [0,%d)", k, P);
  if (capacity < 0) return fail(MBD_ERR_INVALID, "peek_mpc_pick: capacity=%d", capacity);
  HIP_TRY(hipSetDevice(env->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t at = (size_t)k * cap;  // (plan k's rings)
  MBD_TRY(ring_read(d_log_choice.get() + at, 1, count, cap, capacity, choice_out));
  MBD_TRY(ring_read(d_log_rets.get() + 3 * at, 3, count, cap, capacity, rets_out));
  MBD_TRY(ring_read(d_log_best.get() + at, 1, count, cap, capacity, best_out));
  if (count_out) *count_out = (int)(count < 0x7fffffff ? count : 0x7fffffff);
  return MBD_OK;
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

// include/mbd_hip_debug.h: the device argmax of pick_gather_kernel over P rows of N rewards
extern "C" int mbd_debug_pick_best(const float* rews, int P, int N, int32_t* best_out) {
  if (!rews || !best_out) return fail(MBD_ERR_INVALID, "pick_best: NULL argument");
  if (P < 1 || P > 65535 || N < 1) return fail(MBD_ERR_INVALID, "pick_best: P=%d N=%d", P, N);
  if (device_count_quiet() < 1) return fail(MBD_ERR_NO_DEVICE, "no HIP device: this library has no CPU fallback");
  DevBuf<float> d_rews;
  DevBuf<int> d_best;
  HIP_TRY(d_rews.upload(rews, (size_t)P * N));
  HIP_TRY(d_best.alloc(P));
  hipLaunchKernelGGL(pick_best_probe_kernel, dim3(1, (unsigned)P), dim3(kScoreThreads), 0, 0, (const float*)d_rews, N, d_best.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(d_best.download(best_out, P));
  return MBD_OK;
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

// ---- the adapt record (include/mbd_hip.h mbd_adapt) ---------------------------------------------------------------------------
// the refusals the record alone decides against the handle's update_method and enable_demo, in the header's order, each naming the
// field — host arithmetic, before any device access
static int check_adapt(const mbd_adapt* rec, int update_method, int enable_demo) {
  if (!std::isfinite(rec->rate) || !(rec->rate > 0.0f) || rec->rate > 1.0f)
    return fail(MBD_ERR_INVALID, "adapt record: rate=%g: must lie in (0, 1]", (double)rec->rate);
  if (!std::isfinite(rec->a_min) || !(rec->a_min > 0.0f) || rec->a_min > 1.0f)
    return fail(MBD_ERR_INVALID, "adapt record: a_min=%g: must be finite with 0 < a_min <= 1", (double)rec->a_min);
  if (!std::isfinite(rec->a_max) || rec->a_max < 1.0f)
    return fail(MBD_ERR_INVALID, "adapt record: a_max=%g: must be finite and >= 1", (double)rec->a_max);
  if (rec->carry != 0 && rec->carry != 1) return fail(MBD_ERR_INVALID, "adapt record: carry=%d: 0 or 1", rec->carry);
  for (int r = 0; r < 4; ++r)
    if (rec->reserved[r] != 0) return fail(MBD_ERR_INVALID, "adapt record: reserved[%d]=%d: must be 0", r, rec->reserved[r]);
  if (update_method == 2 || update_method == 3)
    return fail(MBD_ERR_UNSUPPORTED, "adapt record: update_method=%d: cma-es (2) and cem (3) adapt their own sigma", update_method);
  if (enable_demo) return fail(MBD_ERR_UNSUPPORTED, "adapt record: enable_demo=1: demo plans take no adapt record");
  return MBD_OK;
}
extern "C" int mbd_debug_check_adapt(const mbd_adapt* rec, int update_method, int enable_demo) {
  if (!rec) return fail(MBD_ERR_INVALID, "adapt record is NULL");
  return check_adapt(rec, update_method, enable_demo);
}

int AdaptRec::set(const mbd_adapt* rec, int HNu, const float* g, const mbd_env* env, hipStream_t s) {
  HIP_TRY(hipSetDevice(env->device));
  HIP_TRY(hipDeviceSynchronize());  // (a step in flight may still read G or write the log)
  has = false;
  count = 0;
  if (!rec) return MBD_OK;
  HIP_TRY(d_a.grow(HNu));
  HIP_TRY(d_G.grow(HNu));
  HIP_TRY(d_buf.grow(HNu));
  HIP_TRY(d_log_S.grow(kLogCap));
  HIP_TRY(d_log_skipped.grow(kLogCap));
  rule = AdaptRule{rec->rate, rec->a_min, rec->a_max};
  carry = rec->carry;
  has = true;
  MBD_TRY(table(-1, g, HNu, s));
  HIP_TRY(hipStreamSynchronize(s));
  return MBD_OK;
}

int AdaptRec::peek(const mbd_env* env, int HNu, float* a_out, float* ratio_out, int32_t* skipped_out, int capacity, int* count_out) const {
  if (!has) return fail(MBD_ERR_STATE, "peek_adapt: the plan has no adapt record");
  if (capacity < 0) return fail(MBD_ERR_INVALID, "peek_adapt: capacity=%d", capacity);
  HIP_TRY(hipSetDevice(env->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(d_a.download(a_out, HNu));
  MBD_TRY(ring_read(d_log_S.get(), 1, count, kLogCap, capacity, ratio_out));
  MBD_TRY(ring_read(d_log_skipped.get(), 1, count, kLogCap, capacity, skipped_out));
  if (count_out) *count_out = (int)(count < 0x7fffffffll ? count : 0x7fffffffll);
  return MBD_OK;
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

// include/mbd_hip_debug.h: the update on the HOST — the per-element functions the kernels call (one text for host and device), the
// chains and the sums in the kernels' order, no device touched
static int check_adapt_step_args(const char* what, const float* w, const float* cand, int N, int HNu, const float* ybar, const float* a,
                                 float rate, float a_min, float a_max) {
  if (!w || !cand || !ybar || !a) return fail(MBD_ERR_INVALID, "%s: NULL argument", what);
  if (N < 1 || HNu < 1 || (uint64_t)N * (uint64_t)HNu > (1ull << 26)) return fail(MBD_ERR_INVALID, "%s: N=%d HNu=%d", what, N, HNu);
  mbd_adapt rec{};
  rec.rate = rate; rec.a_min = a_min; rec.a_max = a_max;
  return check_adapt(&rec, 0, 0);
}
extern "C" int mbd_debug_adapt_host(const float* w, const float* cand, int N, int HNu, const float* ybar, float sigma, int lazy,
                                    const float* a, const float* g, float rate, float a_min, float a_max, float* a_out, float* G_out,
                                    float* S_out, int32_t* skipped_out) {
  MBD_TRY(check_adapt_step_args("adapt_host", w, cand, N, HNu, ybar, a, rate, a_min, a_max));
  const AdaptRule R{rate, a_min, a_max};
  std::vector<float> G((size_t)HNu), s((size_t)HNu, 0.0f), an(a, a + HNu);
  for (int e = 0; e < HNu; ++e) G[e] = adapt_G(a[e], g, e);
  float acc = 0.0f;
  int n_active = 0;
  for (int e = 0; e < HNu; ++e) {
    float m1[kWmG], m2[kWmG];
    for (int k = 0; k < kWmG; ++k) {
      m1[k] = m2[k] = 0.0f;
      for (int n = k; n < N; n += kWmG)
        adapt_chain(w[n], adapt_value(cand[(size_t)n * HNu + e], lazy, sigma, ybar[e]), ybar[e], m1[k], m2[k]);
    }
    float t1 = m1[0], t2 = m2[0];
    for (int k = 1; k < kWmG; ++k) {
      t1 = t1 + m1[k];
      t2 = t2 + m2[k];
    }
    if (!(G[e] > 0.0f)) continue;
    s[e] = adapt_s(adapt_var(t1, t2), sigma, G[e]);
    acc = acc + s[e] * s[e];
    ++n_active;
  }
  const float S = adapt_ratio(acc, n_active);
  const bool skip = adapt_skip(S, n_active);
  if (!skip)
    for (int e = 0; e < HNu; ++e)
      if (G[e] > 0.0f) {
        an[e] = adapt_next(a[e], s[e], S, R);
        G[e] = adapt_G(an[e], g, e);
      }
  if (a_out) memcpy(a_out, an.data(), sizeof(float) * HNu);
  if (G_out) memcpy(G_out, G.data(), sizeof(float) * HNu);
  if (S_out) *S_out = S;
  if (skipped_out) *skipped_out = skip ? 1 : 0;
  return MBD_OK;
}
// ... and on the DEVICE, by a scratch record's own launches: its table launch forms G = a * g from the uploaded arrays, then the
// update's two.  The log is one entry long (count = 0: slot 0); what is read back and left unwritten reads back as NaN, or -1.
extern "C" int mbd_debug_adapt_step(const float* w, const float* cand, int N, int HNu, const float* ybar, float sigma,
                                    int sigma_on_device, int lazy, const float* a, const float* g, float rate, float a_min, float a_max,
                                    float* a_out, float* G_out, float* S_out, int32_t* skipped_out) {
  MBD_TRY(check_adapt_step_args("adapt_step", w, cand, N, HNu, ybar, a, rate, a_min, a_max));
  if (device_count_quiet() < 1) return fail(MBD_ERR_NO_DEVICE, "no HIP device: this library has no CPU fallback");
  DevBuf<float> d_w, d_cand, d_ybar, d_g, d_sigma;
  AdaptRec A;
  HIP_TRY(d_w.upload(w, N));
  HIP_TRY(d_cand.upload(cand, (size_t)N * HNu));
  HIP_TRY(d_ybar.upload(ybar, HNu));
  if (g) HIP_TRY(d_g.upload(g, HNu));  // (without: d_g stays nullptr)
  HIP_TRY(d_sigma.upload(&sigma, 1));
  HIP_TRY(A.d_a.upload(a, HNu));
  HIP_TRY(A.d_G.alloc_poisoned(HNu));
  HIP_TRY(A.d_buf.alloc_poisoned(HNu));
  HIP_TRY(A.d_log_S.alloc_poisoned(1));
  HIP_TRY(A.d_log_skipped.alloc_poisoned(1));
  A.rule = AdaptRule{rate, a_min, a_max};
  A.has = true;
  MBD_TRY(A.table(0, d_g, HNu, nullptr));
  // (sigma from the device scalar: the host value handed to the kernels is then a NaN they must not use)
  MBD_TRY(A.update(d_w, StepCand{d_cand, N, HNu, lazy ? 1 : 0, sigma_on_device ? __builtin_nanf("") : sigma,
                                 sigma_on_device ? d_sigma.get() : nullptr, d_ybar}, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(A.d_a.download(a_out, HNu));
  HIP_TRY(A.d_G.download(G_out, HNu));
  HIP_TRY(A.d_log_S.download(S_out, 1));
  HIP_TRY(A.d_log_skipped.download(skipped_out, 1));
  return MBD_OK;
}

// ---- the elite record (include/mbd_hip.h mbd_elites) --------------------------------------------------------------------------
// the refusals the record alone decides against the handle's Nsample, update_method and enable_demo, in the header's order, each
// naming the field — host arithmetic, before any device access
int check_elites(const mbd_elites* rec, int Nsample, int update_method, int enable_demo) {
  if (rec->n_elites < 0 || rec->n_elites > kEliteMax)
    return fail(MBD_ERR_INVALID, "elite record: n_elites=%d outside [0, %d]", rec->n_elites, kEliteMax);
  if (rec->nominal != 0 && rec->nominal != 1) return fail(MBD_ERR_INVALID, "elite record: nominal=%d: 0 or 1", rec->nominal);
  if (rec->carry != 0 && rec->carry != 1) return fail(MBD_ERR_INVALID, "elite record: carry=%d: 0 or 1", rec->carry);
  if (rec->n_elites + rec->nominal == 0)
    return fail(MBD_ERR_INVALID, "elite record: n_elites=0 with nominal=0: the record asks for nothing (NULL clears)");
  if (rec->n_elites + rec->nominal >= Nsample)
    return fail(MBD_ERR_INVALID, "elite record: n_elites=%d + nominal=%d must lie below Nsample=%d", rec->n_elites, rec->nominal, Nsample);
  for (int r = 0; r < 5; ++r)
    if (rec->reserved[r] != 0) return fail(MBD_ERR_INVALID, "elite record: reserved[%d]=%d: must be 0", r, rec->reserved[r]);
  if (update_method == 2 || update_method == 3)
    return fail(MBD_ERR_UNSUPPORTED, "elite record: update_method=%d: cem (3) keeps elites of its own kind, cma-es' (2) spread would "
                                     "be biased by repeated rows", update_method);
  if (enable_demo) return fail(MBD_ERR_UNSUPPORTED, "elite record: enable_demo=1: a demo plan's score is not the return");
  return MBD_OK;
}
extern "C" int mbd_debug_check_elites(const mbd_elites* rec, int Nsample, int update_method, int enable_demo) {
  if (!rec) return fail(MBD_ERR_INVALID, "elite record is NULL");
  return check_elites(rec, Nsample, update_method, enable_demo);
}

int EliteRec::set(const mbd_elites* rec, int P_, int HNu, int device) {
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipDeviceSynchronize());  // (a step in flight may still read the elites or write the logs)
  has = false;
  restart();
  if (!rec) return MBD_OK;
  layout(rec->n_elites, rec->nominal, rec->carry, P_);
  const size_t PR = (size_t)P * rows;
  HIP_TRY(d_E.grow(PR * HNu));
  HIP_TRY(d_R.grow(PR));
  HIP_TRY(d_src.grow(PR));
  HIP_TRY(d_count.grow(P));
  HIP_TRY(d_log_count.grow((size_t)P * log_cap));
  HIP_TRY(d_log_kept.grow((size_t)P * log_cap));
  HIP_TRY(d_log_top.grow((size_t)P * log_cap));
  has = true;
  return MBD_OK;
}

int EliteRec::scratch(int n_elites, int nominal_, int P_, int HNu, const float* E_in, const int32_t* count_in) {
  layout(n_elites, nominal_, 0, P_);
  log_cap = 1;
  has = true;
  const size_t PR = (size_t)P * rows;
  HIP_TRY(d_E.alloc_poisoned(PR * HNu));
  HIP_TRY(d_R.alloc_poisoned(PR));
  HIP_TRY(d_src.alloc_poisoned(PR));
  HIP_TRY(d_count.upload(count_in, P));
  HIP_TRY(d_log_count.alloc_poisoned(P));
  HIP_TRY(d_log_kept.alloc_poisoned(P));
  HIP_TRY(d_log_top.alloc_poisoned(P));
  // (the rows from count_in[k] on stay poisoned: E' of a plan no launch writes reads back as it went in)
  for (int k = 0; E_in && k < P; ++k) {
    const size_t at = (size_t)k * rows * HNu;
    if (count_in[k] > 0) HIP_TRY(hipMemcpy(d_E + at, E_in + at, sizeof(float) * (size_t)count_in[k] * HNu, hipMemcpyHostToDevice));
  }
  return MBD_OK;
}

int EliteRec::peek(const mbd_env* env, int k, int HNu, float* elites_out, float* returns_out, int32_t* src_out, int32_t* count_out,
                   int32_t* log_count, int32_t* log_kept, float* log_top, int capacity, int* n_log_out, const char* what) const {
  if (!has) return fail(MBD_ERR_STATE, "peek_elites: the %s has no elite record", what);
  if (capacity < 0) return fail(MBD_ERR_INVALID, "peek_elites: capacity=%d", capacity);
  HIP_TRY(hipSetDevice(env->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t row = (size_t)k * rows, log = (size_t)k * log_cap;
  if (elites_out && n) HIP_TRY(hipMemcpy(elites_out, d_E + row * HNu, sizeof(float) * (size_t)n * HNu, hipMemcpyDeviceToHost));
  if (returns_out && n) HIP_TRY(hipMemcpy(returns_out, d_R + row, sizeof(float) * n, hipMemcpyDeviceToHost));
  if (src_out && n) HIP_TRY(hipMemcpy(src_out, d_src + row, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  if (count_out) HIP_TRY(hipMemcpy(count_out, d_count + k, sizeof(int32_t), hipMemcpyDeviceToHost));
  MBD_TRY(ring_read(d_log_count.get() + log, 1, steps[k], log_cap, capacity, log_count));
  MBD_TRY(ring_read(d_log_kept.get() + log, 1, steps[k], log_cap, capacity, log_kept));
  MBD_TRY(ring_read(d_log_top.get() + log, 1, steps[k], log_cap, capacity, log_top));
  if (n_log_out) *n_log_out = (int)(steps[k] < 0x7fffffffll ? steps[k] : 0x7fffffffll);
  return MBD_OK;
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

// include/mbd_hip_debug.h: one step of the record on the HOST — the injection, then the selection — from the functions the kernels
// call (one text for host and device); no device touched
static int check_elites_args(const char* what, const float* cand, int N, int HNu, const float* ybar, float sigma, int lazy, int n_elites,
                             int nominal, const float* E_in, int count_in) {
  if (!cand || !ybar) return fail(MBD_ERR_INVALID, "%s: NULL argument", what);
  if (N < 1 || HNu < 1 || (uint64_t)N * (uint64_t)HNu > (1ull << 26)) return fail(MBD_ERR_INVALID, "%s: N=%d HNu=%d", what, N, HNu);
  if (n_elites < 0 || n_elites > kEliteMax) return fail(MBD_ERR_INVALID, "%s: n_elites=%d outside [0, %d]", what, n_elites, kEliteMax);
  if (nominal != 0 && nominal != 1) return fail(MBD_ERR_INVALID, "%s: nominal=%d: 0 or 1", what, nominal);
  if (n_elites + nominal >= N) return fail(MBD_ERR_INVALID, "%s: n_elites=%d + nominal=%d must lie below N=%d", what, n_elites, nominal, N);
  if (count_in < 0 || count_in > n_elites) return fail(MBD_ERR_INVALID, "%s: count=%d outside [0, n_elites=%d]", what, count_in, n_elites);
  if (count_in > 0 && !E_in) return fail(MBD_ERR_INVALID, "%s: count=%d without elites", what, count_in);
  if (lazy && !(sigma > 0.0f)) return fail(MBD_ERR_INVALID, "%s: sigma=%g: a lazy plan's sigma is > 0", what, (double)sigma);
  return MBD_OK;
}
static void elites_inject_host(float* cand, int HNu, const float* ybar, float sigma, int lazy, const float* g, int nominal,
                               const float* E_in, int count_in) {
  for (int slot = 0; slot < nominal + count_in; ++slot)
    for (int e = 0; e < HNu; ++e) {
      float v;
      if (slot < nominal) {
        v = elite_nominal(ybar[e], lazy);
      } else {
        const float Ej = E_in[(size_t)(slot - nominal) * HNu + e];
        v = lazy ? elite_z(Ej, ybar[e], sigma, g, e) : Ej;
      }
      cand[(size_t)slot * HNu + e] = v;
    }
}
extern "C" int mbd_debug_elites_host(const float* rews, const float* cand, int N, int HNu, const float* ybar, float sigma, int lazy,
                                     const float* g, int n_elites, int nominal, const float* E_in, int count_in, float* cand_out,
                                     float* E_out, float* R_out, int32_t* src_out, int32_t* count_out, int32_t* kept_out,
                                     float* top_out) {
  MBD_TRY(check_elites_args("elites_host", cand, N, HNu, ybar, sigma, lazy, n_elites, nominal, E_in, count_in));
  if (!rews) return fail(MBD_ERR_INVALID, "elites_host: NULL argument");
  std::vector<float> c(cand, cand + (size_t)N * HNu);
  elites_inject_host(c.data(), HNu, ybar, sigma, lazy, g, nominal, E_in, count_in);
  int src[kEliteMax];
  float R[kEliteMax];
  const int cnt = elite_select_host(rews, N, n_elites, src, R);
  int kept = 0;
  for (int j = 0; j < cnt; ++j) kept += src[j] < nominal + count_in ? 1 : 0;
  if (cand_out) memcpy(cand_out, c.data(), sizeof(float) * c.size());
  // (rows and entries from count' on are left as the device entry leaves them: all bits set)
  if (E_out) memset(E_out, 0xff, sizeof(float) * (size_t)n_elites * HNu);
  if (R_out) memset(R_out, 0xff, sizeof(float) * n_elites);
  if (src_out) memset(src_out, 0xff, sizeof(int32_t) * n_elites);
  for (int j = 0; j < cnt; ++j) {
    if (E_out)
      for (int e = 0; e < HNu; ++e) E_out[(size_t)j * HNu + e] = elite_value(c[(size_t)src[j] * HNu + e], lazy, sigma, ybar[e]);
    if (R_out) R_out[j] = R[j];
    if (src_out) src_out[j] = src[j];
  }
  if (count_out) *count_out = cnt;
  if (kept_out) *kept_out = kept;
  if (top_out) *top_out = cnt > 0 ? R[0] : __builtin_bit_cast(float, 0x7fc00000u);
  return MBD_OK;
}
// ... and the two launches alone on the DEVICE, on caller-given arrays, by a scratch record's own members.  What is read back is
// filled with all-ones bits first; the log is one entry long (steps = 0: slot 0).
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

// ---- the to-go record (include/mbd_hip.h mbd_togo) ---------------------------------------------------------------------------
// the refusals the record alone decides against the handle's Hsample, Nsample, update_method and enable_demo, in the header's order,
// each naming the field — host arithmetic, before any device access
constexpr int kTogoMaxN = 12288;  // the N weights of a group in the default 48 KB LDS window
int check_togo(const mbd_togo* rec, int Hsample, int Nsample, int update_method, int enable_demo) {
  if (rec->block < 1) return fail(MBD_ERR_INVALID, "to-go record: block=%d: at least 1", rec->block);
  if (rec->min_tail < 1 || rec->min_tail > Hsample)
    return fail(MBD_ERR_INVALID, "to-go record: min_tail=%d outside [1, Hsample=%d]", rec->min_tail, Hsample);
  for (int r = 0; r < 2; ++r)
    if (rec->reserved[r] != 0) return fail(MBD_ERR_INVALID, "to-go record: reserved[%d]=%d: must be 0", r, rec->reserved[r]);
  if (update_method == 2 || update_method == 3)
    return fail(MBD_ERR_UNSUPPORTED, "to-go record: update_method=%d: cma-es (2) and cem (3) have no per-row form here", update_method);
  if (enable_demo) return fail(MBD_ERR_UNSUPPORTED, "to-go record: enable_demo=1: a demo plan's score is not the return");
  if (Nsample > kTogoMaxN)
    return fail(MBD_ERR_UNSUPPORTED, "to-go record: Nsample=%d above %d: a group's weights must fit LDS", Nsample, kTogoMaxN);
  return MBD_OK;
}
extern "C" int mbd_debug_check_togo(const mbd_togo* rec, int Hsample, int Nsample, int update_method, int enable_demo) {
  if (!rec) return fail(MBD_ERR_INVALID, "to-go record is NULL");
  return check_togo(rec, Hsample, Nsample, update_method, enable_demo);
}

int TogoRec::set(const mbd_togo* rec, int P, int H, int N, int device) {
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipDeviceSynchronize());  // (a step in flight may still write R and W)
  has = false;
  if (!rec) return MBD_OK;
  layout(rec->block, rec->min_tail, H);
  const size_t n = (size_t)P * G * N;
  HIP_TRY(d_R.grow(n));
  HIP_TRY(d_W.grow(n));
  HIP_TRY(hipMemset(d_R, 0xff, sizeof(float) * n));  // (no step yet: mbd_*_peek_togo says so)
  HIP_TRY(hipMemset(d_W, 0xff, sizeof(float) * n));
  HIP_TRY(hipDeviceSynchronize());
  stepped = false;
  has = true;
  return MBD_OK;
}

int TogoRec::peek(const mbd_env* env, int k, int N, const float* d_weights, int32_t* starts_out, float* R_out, float* W_out,
                  int32_t* n_groups_out, const char* what) const {
  if (!has) return fail(MBD_ERR_STATE, "peek_togo: the %s has no to-go record", what);
  HIP_TRY(hipSetDevice(env->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t gn = (size_t)G * N;
  if (starts_out) memcpy(starts_out, starts.data(), sizeof(int32_t) * G);
  if (R_out) HIP_TRY(hipMemcpy(R_out, d_R + (size_t)k * gn, sizeof(float) * gn, hipMemcpyDeviceToHost));
  if (W_out) HIP_TRY(hipMemcpy(W_out, d_W + (size_t)k * gn, sizeof(float) * gn, hipMemcpyDeviceToHost));
  // (group 0's weights are the plan's own slice of d_weights, once a step of the record has written them)
  if (W_out && stepped) HIP_TRY(hipMemcpy(W_out, d_weights + (size_t)k * N, sizeof(float) * N, hipMemcpyDeviceToHost));
  if (n_groups_out) *n_groups_out = G;
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

// include/mbd_hip_debug.h: the layout and the returns on the HOST, from the functions the returns kernel calls; no device touched
static int check_togo_args(const char* what, int N, int H, int block, int min_tail) {
  if (N < 1 || H < 1 || (uint64_t)N * (uint64_t)H > (1ull << 26)) return fail(MBD_ERR_INVALID, "%s: N=%d H=%d", what, N, H);
  if (block < 1) return fail(MBD_ERR_INVALID, "%s: block=%d: at least 1", what, block);
  if (min_tail < 1 || min_tail > H) return fail(MBD_ERR_INVALID, "%s: min_tail=%d outside [1, H=%d]", what, min_tail, H);
  return MBD_OK;
}
extern "C" int mbd_debug_togo_host(const float* rews, const float* rewss, int N, int H, int block, int min_tail, int32_t* starts_out,
                                   float* R_out, int32_t* n_groups_out) {
  MBD_TRY(check_togo_args("togo_host", N, H, block, min_tail));
  if (R_out && (!rews || !rewss)) return fail(MBD_ERR_INVALID, "togo_host: NULL argument");
  const int G = togo_groups(H, block, min_tail);
  if (starts_out)
    for (int j = 0; j < G; ++j) starts_out[j] = togo_start(j, block);
  if (n_groups_out) *n_groups_out = G;
  if (!R_out) return MBD_OK;
  for (int n = 0; n < N; ++n) {
    R_out[n] = rews[n];
    togo_chain(rewss + (size_t)n * H, H, block, G, [&](int j, float v) { R_out[(size_t)j * N + n] = v; });
  }
  return MBD_OK;
}
// ... and the step's two launches alone on the DEVICE, on caller-given arrays, by a scratch record's own launch.  What is read back
// is filled with all-ones bits (quiet NaN) first.
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
