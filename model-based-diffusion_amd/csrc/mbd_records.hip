// mbd_records.hip — the records plans and sweeps carry (mbd_internal.h: noise, sigma, delay, demo, objective, value, zone, weighting,
// pick, elite, to-go; adapt, which only plans hold): every member function, record by record, with the record's check_* — the
// refusals the record alone decides, host arithmetic — and the mbd_debug_* entries that launch the records' own kernels or none
// (include/mbd_hip_debug.h: the check_* entries, the *_host references, the kernels alone on caller-given arrays); and what the two
// handle units share beside the records: the noise schedule, check_mpc_plant, check_mpc_config, the refusals of a record beside a
// zone or a to-go record.  The kernels the members launch are mbd_record_kernels.h's, which this unit alone includes and emits.
// An entry that launches a sampler or a step kernel is mbd_plan.hip's, and the launches of the elite and to-go records, whose
// kernels are step kernels, are each handle unit's own.  The handles themselves and their set_* wrappers — the refusals that
// depend on what else a handle carries, and their order — are mbd_plan.hip's and mbd_sweep.hip's.
#include "mbd_internal.h"
#include "mbd_record_kernels.h"
#include "../../include/mbd_hip_debug.h"

// noise schedule (mbd_planner.py:84-87)
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

// ---- the adapt record (include/mbd_hip.h mbd_adapt) ---------------------------------------------------------------------------
int check_adapt(const mbd_adapt* rec, int update_method, int enable_demo) {
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

// include/mbd_hip_debug.h: one step of the record on the HOST — the injection, then the selection — from the functions the kernels
// call (one text for host and device); no device touched
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

// ---- the to-go record (include/mbd_hip.h mbd_togo) ---------------------------------------------------------------------------
// the refusals the record alone decides against the handle's Hsample, Nsample, update_method and enable_demo, in the header's order,
// each naming the field — host arithmetic, before any device access
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
int refuse_beside_togo(const char* who, const char* handle) {
  return fail(MBD_ERR_UNSUPPORTED, "%s: the %s carries a to-go record (mbd_%s_set_togo): what the record means per horizon row is not "
                                   "defined", who, handle, handle);
}

void TogoRec::layout(int block_, int min_tail_, int H) {
  block = block_; min_tail = min_tail_;
  G = togo_groups(H, block, min_tail);
  starts.resize(G);
  for (int j = 0; j < G; ++j) starts[j] = togo_start(j, block);
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

// include/mbd_hip_debug.h: the layout and the returns on the HOST, from the functions the returns kernel calls; no device touched
int check_togo_args(const char* what, int N, int H, int block, int min_tail) {
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
