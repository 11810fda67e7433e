/* mbd_hip_debug.h — test and A/B levers of libmbd_hip.so.  NOT part of the drop-in boundary (include/mbd_hip.h): nothing a
 * caller of the reference's planner needs is here, and results are bit-identical whatever the levers say — the test-suite
 * holds every alternative they select to the same checker. */
#ifndef MBD_HIP_DEBUG_H
#define MBD_HIP_DEBUG_H
#include "mbd_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
/* One process-wide table of integer levers, initialised ONCE from the environment variables of the same names
 * (MBD_NO_DPP, MBD_NO_NFR_CONST, MBD_NO_REWARD_CONST, MBD_NO_PLANAR_FLAGS, MBD_NO_FAST_SLIDES, MBD_NO_FUSED_NOISE,
 * MBD_NO_LAZY, MBD_NO_PREFETCH, MBD_NO_AUX, MBD_WMEAN_SPLIT, MBD_NO_FUSED_SCORE, MBD_PK2, MBD_WPB, MBD_LDS_RESERVE,
 * MBD_NO_HELPERS, MBD_ENS_SPLIT, MBD_NO_UNIT_CONST);
 * -1 = not set: the library decides.  The launch paths read the table, never the environment. */
int mbd_debug_set(const char* name, int value);
int mbd_debug_get(const char* name, int* value_out);
/* the DPP layout family (0..3, -1: none) a model's link tree fits, with its lane <-> link table and shifts */
int mbd_debug_dpp_layout(const mbd_model_t* model, signed char tab[32], int shifts_out[4]);
/* the rollout launch the library picks for a model (no device needed): n_cus compute units, B candidates, horizon H,
 * sweep_plan_N > 0: a sweep of plans of that many candidates, has_xref: the env has a demo.  out = grid (workgroups of
 * the rollout itself), block, dynamic LDS bytes, candidates per wavefront (0: filled), wavefronts per SIMD asked of a
 * two-candidates-per-lane kernel, XCD-pinned, takes a noise job into spare workgroups, accumulates the demo log-density;
 * name: the instantiation's demangled symbol.  Reads the levers like a launch. */
int mbd_debug_rollout_choice(const mbd_model_t* model, int n_cus, int B, int H, int sweep_plan_N, int has_xref,
                             char* name, int cap, int out[8]);
/* per-wavefront clock records of the 3-D rollout kernels (tools/probes/rollout_timeline.py); d_buf: device, caller-owned */
int mbd_debug_set_clock_buffer(mbd_env* env, void* d_buf);
/* the arithmetic primitives of csrc/mbd_math.h over host arrays, one GPU thread per element (op: the primitive's name
 * there, e.g. "div_", "angle_unit2", "qnormalize_qm<1>"; mbd_debug_math_name(k) lists them, NULL past the last).
 * in: [n][k_in] row-major, out: [n][k_out], both fixed per op (mbd_debug_math_arity; no device needed).  Packed ops take
 * elements (2j, 2j+1) as the two halves of their pairs.  Argument errors first (unknown op, n outside [0, 2^26], NULL
 * arrays), then MBD_ERR_NO_DEVICE. */
const char* mbd_debug_math_name(int k);
int mbd_debug_math_arity(const char* op, int* k_in, int* k_out);
int mbd_debug_eval_math(const char* op, long long n, const float* in, float* out);
/* The shaped normals of a diffusion step on their own (include/mbd_hip.h mbd_noise_shape): z_out HOST [N][HNu] =
 * normal(key, (N, HNu)) * g[e mod HNu] by the loops the noise kernels run with a shape, on `blocks` workgroups of 256 threads,
 * with 32-bit indices (wide = 0: what the library takes below 2^32 elements) or 64-bit ones (wide = 1: beyond) — so that the
 * wide form is held to the checker at a size a test can afford.  g HOST [HNu]; N * HNu <= 2^26.  Argument errors first, then
 * MBD_ERR_NO_DEVICE. */
int mbd_debug_noise_shaped(const uint32_t key[2], int impl, int N, int HNu, const float* g, int wide, int blocks, float* z_out);
/* The normals of a diffusion step under a noise basis on their own (include/mbd_hip.h mbd_noise_basis): z_out HOST [N][H Nu] by
 * knot_noise_kernel on `blocks` workgroups (fewer than the columns need: the column loop strides).  W HOST [H][n_knots]; g HOST
 * [H Nu] or NULL: no shape; N * H * Nu <= 2^26.  Argument errors first, then MBD_ERR_NO_DEVICE. */
int mbd_debug_knot_noise(const uint32_t key[2], int impl, int N, int H, int Nu, int n_knots, const float* W, const float* g,
                         int blocks, float* z_out);
/* The same on the HOST: the kernel's per-column code (one text for host and device) over all N Nu columns in a loop, no device
 * touched — a test without a GPU holds the kernel's indexing and arithmetic to the checker.  z_out HOST [N][H Nu]. */
int mbd_debug_knot_noise_host(const uint32_t key[2], int impl, int N, int H, int Nu, int n_knots, const float* W, const float* g,
                              float* z_out);
/* The refusals a delay record alone decides (include/mbd_hip.h mbd_mpc_delay) for a handle of that action_size: the function
 * both set calls run on their record, host arithmetic, no device — so that a test without a GPU, which has no handle whose
 * action_size is not 0, reaches the refusal of a non-finite row value too. */
int mbd_debug_check_mpc_delay(const mbd_mpc_delay* rec, int action_size);
/* The sigma a warm tick of a path-integral episode starts from (include/mbd_hip.h mbd_mpc_sigma), on the HOST: the function
 * mpc_pi_sigma_kernel calls (one text for host and device) over n values of sigma_end, no device touched.  HOST sigma_end [n],
 * next_out [n]. */
int mbd_debug_mpc_sigma_next(const float* sigma_end, int n, float sigma_cold, float sigma_warm, float gain, float* next_out);
/* The refusals a sigma record alone decides for a handle of that update_method: the function both set calls run on their record,
 * host arithmetic, no device. */
int mbd_debug_check_mpc_sigma(const mbd_mpc_sigma* rec, int update_method);
/* The refusals an objective record alone decides (include/mbd_hip.h mbd_objective) for a handle of that Hsample and action_size:
 * the function both set calls run on their record, host arithmetic, no device — so that a test without a GPU, whose stand-in handle
 * has Hsample = action_size = 0, reaches the refusals of the tables' values too. */
int mbd_debug_check_objective(const mbd_objective* rec, int Hsample, int action_size);
/* objective_kernel's arithmetic on the HOST: the per-candidate functions the kernel calls (one text for host and device) over B rows
 * in a loop, the actuators' terms summed in ascending order as the kernel's lanes are, no device touched.  HOST rewss [B][H], rews
 * [B] (mean_H as a rollout stores it), cand [N][H][Nu] — values, or with lazy != 0 normals formed as clip((z * sigma) + ybar[h][a],
 * -1, 1) —, row b is candidate b % N; w [H] or NULL with its f32 left-to-right sum wsum, q [Nu], prev [Nu] (already clipped) or
 * NULL; rews_out [B], ret_out [B], cost_out [min(B, N)]. */
int mbd_debug_objective_host(const float* rewss, const float* rews, int B, int N, int H, int Nu, const float* cand, int lazy,
                             float sigma, const float* ybar, const float* w, float wsum, const float* q, float effort, float rate,
                             const float* prev, float* rews_out, float* ret_out, float* cost_out);
/* weigh_kernel's arithmetic on the HOST (include/mbd_hip.h mbd_weighting): the per-entry functions and the temperature selection
 * the kernel calls (one text for host and device), with the block reductions restated as loops over the 1024 virtual threads, their
 * 64-lane butterflies and the 16 wavefront values in order; no device touched.  HOST rews [N]; temp: T0; std_guard is accepted for
 * symmetry with the score and ignored (under a record every update method has the guard); rec NULL: rejection off, ess_frac 0.
 * weights_out [N]; rew_mean_out, temp_out, ess_out, kept_out: one value each; any may be NULL.  The record is checked as the set
 * calls check it (MBD_ERR_INVALID naming the field). */
int mbd_debug_weighting_host(const float* rews, int N, float temp, int std_guard, const mbd_weighting* rec, float* weights_out,
                             float* rew_mean_out, float* temp_out, float* ess_out, int32_t* kept_out);
/* the argmax of pick_gather_kernel alone (include/mbd_hip.h mbd_mpc_pick), on the DEVICE: HOST rews [P][N], one 1024-thread
 * workgroup per row; best_out [P]: the lowest index among the maxima of the row's finite entries, -1 where none is finite.  NULL
 * arguments, P outside [1, 65535] or N < 1 -> MBD_ERR_INVALID before any device access; no device -> MBD_ERR_NO_DEVICE. */
int mbd_debug_pick_best(const float* rews, int P, int N, int32_t* best_out);
/* The refusals a value record alone decides (include/mbd_hip.h mbd_value) for an env of that state_size; rigid_body != 0: the env
 * has links (MBD_VALUE_REL_XY allowed).  The function both set calls run on their record, host arithmetic, no device. */
int mbd_debug_check_value(const mbd_value* rec, int state_size, int rigid_body);
/* value_kernel's arithmetic on the HOST: the functions the kernel calls (one text for host and device) over B rows in a loop, no
 * device touched.  The record is checked as the set calls check it against state_size = rec->n_in.  HOST states [B][n_in], rews
 * [B] or NULL; v_out [B]: V; rews_out [B] or NULL: rews + (scale * V). */
int mbd_debug_value_host(const mbd_value* rec, int rigid_body, const float* states, const float* rews, int B, float* v_out,
                         float* rews_out);
/* The update step of a sweep on its own, on the DEVICE: what a lockstep step launches behind its rollout and its records' launches
 * — under a weighting record the weigh kernel, then score + weighted mean over the P plans (MBD, mppi, cma-es: plus spread and sigma)
 * or score, selection and mean of the best (cem) — with every plan's temperature, on uploaded arrays, for diffusion step i's schedule
 * values and the env's rew_xref.  All arrays HOST.  cand [P][N][H Nu]: update_method 0 the step's normals z, a candidate being
 * clip((z * sigma_i) + ybar, -1, 1) as the lazy plans form it, otherwise the candidates; ybar [P][H Nu]: Ybar_i, or the mean; rews
 * [P][N]; lp [P][N]: exactly with enable_demo; sigma_in [P]: exactly for cma-es.  ybar_out [P][H Nu], weights_out [P][N],
 * rew_mean_out [P], sigma_out [P] (cma-es), idx_out [P][min(N, 10)] (cem); any may be NULL.  What is read back is filled with quiet
 * NaN (idx: -1) first.  Argument errors first (NULL sweep / cand / ybar / rews, lp or sigma_in missing or given where not taken, i
 * outside [1, Ndiffuse - 1]), before any device access; then MBD_ERR_STATE while a session is open.  Launches no rollout; a
 * weighting record's entry of the step is entry 0 of mbd_sweep_peek_weighting.  A run after it equals a fresh sweep's. */
int mbd_debug_sweep_update(mbd_sweep* sweep, int i, const float* cand, const float* ybar, const float* rews, const float* lp,
                           const float* sigma_in, float* ybar_out, float* weights_out, float* rew_mean_out, float* sigma_out,
                           int32_t* idx_out);
/* The refusals an adapt record alone decides (include/mbd_hip.h mbd_adapt) for a plan of that update_method and enable_demo: the
 * function the set call runs on its record, host arithmetic, no device. */
int mbd_debug_check_adapt(const mbd_adapt* rec, int update_method, int enable_demo);
/* An adapt record's update on the HOST: the per-element functions the two kernels call (one text for host and device) looped on the
 * CPU, the chains over the 64 groups and every sum in the kernels' order; no device touched.  HOST w [N] the weights; cand [N][HNu]
 * — values, or with lazy != 0 shaped normals formed as clip((z * sigma) + ybar[e], -1, 1) —; ybar [HNu] Ybar_i; a [HNu]; g [HNu] or
 * NULL: no shape; G = a * g is formed first.  a_out, G_out [HNu], S_out, skipped_out: one value each; any may be NULL.  rate, a_min
 * and a_max are checked as the set call checks them (MBD_ERR_INVALID naming the field); N * HNu <= 2^26. */
int mbd_debug_adapt_host(const float* w, const float* cand, int N, int HNu, const float* ybar, float sigma, int lazy, const float* a,
                         const float* g, float rate, float a_min, float a_max, float* a_out, float* G_out, float* S_out,
                         int32_t* skipped_out);
/* The same on the DEVICE, by the launches a step makes: the table kernel forms G = a * g from the uploaded arrays, then
 * adapt_spread_kernel and adapt_finish_kernel.  sigma_on_device != 0: the kernels read sigma from a device scalar, as an mppi plan's
 * do.  What is read back is filled with NaN (skipped: -1) first.  Argument errors first, then MBD_ERR_NO_DEVICE. */
int mbd_debug_adapt_step(const float* w, const float* cand, int N, int HNu, const float* ybar, float sigma, int sigma_on_device,
                         int lazy, const float* a, const float* g, float rate, float a_min, float a_max, float* a_out, float* G_out,
                         float* S_out, int32_t* skipped_out);
/* The refusals an elite record alone decides (include/mbd_hip.h mbd_elites) for a plan of that Nsample, update_method and
 * enable_demo: the function the set call runs on its record, host arithmetic, no device. */
int mbd_debug_check_elites(const mbd_elites* rec, int Nsample, int update_method, int enable_demo);
/* One step of an elite record on the HOST: the injection of E_in [count_in][HNu] (and the nominal) into a copy of cand [N][HNu] —
 * values, or with lazy != 0 normals —, then the selection over rews [N] from that copy; the per-element functions and the order the
 * kernels use (one text for host and device), no device touched.  ybar [HNu] Ybar_i; g [HNu] or NULL: no shape.  cand_out [N][HNu]
 * the candidates behind the injection; E_out [n_elites][HNu], R_out, src_out [n_elites]: rows and entries from count' on have all
 * bits set; count_out, kept_out, top_out: the log entry.  Any output may be NULL.  n_elites, nominal and N are checked as the set
 * call checks them; 0 <= count_in <= n_elites; N * HNu <= 2^26. */
int mbd_debug_elites_host(const float* rews, const float* cand, int N, int HNu, const float* ybar, float sigma, int lazy,
                          const float* g, int n_elites, int nominal, const float* E_in, int count_in, float* cand_out, float* E_out,
                          float* R_out, int32_t* src_out, int32_t* count_out, int32_t* kept_out, float* top_out);
/* The two launches alone on the DEVICE, on caller-given arrays: elite_inject_kernel over cand (count_in in a device word, as a
 * plan's), and elite_select_kernel over rews and cand (count_in: the word it finds; what is read back is filled with all-ones bits
 * first).  Argument errors first, then MBD_ERR_NO_DEVICE. */
int mbd_debug_elites_inject(const float* cand, int N, int HNu, const float* ybar, float sigma, int lazy, const float* g, int n_elites,
                            int nominal, const float* E_in, int count_in, float* cand_out);
int mbd_debug_elites_select(const float* rews, const float* cand, int N, int HNu, const float* ybar, float sigma, int lazy,
                            int n_elites, int nominal, int count_in, float* E_out, float* R_out, int32_t* src_out, int32_t* count_out,
                            int32_t* kept_out, float* top_out);
/* The refusals a to-go record alone decides (include/mbd_hip.h mbd_togo) for a plan of that Hsample, Nsample, update_method and
 * enable_demo: the function the set call runs on its record, host arithmetic, no device. */
int mbd_debug_check_togo(const mbd_togo* rec, int Hsample, int Nsample, int update_method, int enable_demo);
/* A to-go record's group layout and returns on the HOST: the functions the returns kernel calls (one text for host and device)
 * looped over the candidates on the CPU; no device touched.  HOST rews [N], rewss [N][H]; starts_out [G] (room for H entries),
 * R_out [G][N] (room for H rows; row 0 = rews), *n_groups_out = G; any output may be NULL, and rews / rewss may be NULL when R_out
 * is.  block and min_tail are checked as the set call checks them; N * H <= 2^26. */
int mbd_debug_togo_host(const float* rews, const float* rewss, int N, int H, int block, int min_tail, int32_t* starts_out,
                        float* R_out, int32_t* n_groups_out);
/* The step's two launches alone on the DEVICE, on caller-given arrays: togo_returns_kernel, then togo_update_kernel.  HOST cand
 * [N][H * Nu] — values, or with lazy != 0 normals formed as clip((z * sigma) + ybar[e], -1, 1) —, ybar [H * Nu] Ybar_i, rews [N],
 * rewss [N][H]; std_guard != 0: MBD's guard of the standard deviation (0: mppi); literal as mbd_plan_config's literal_score.
 * ybar_out [H * Nu] Ybar_{i-1}, R_out and W_out [G][N], rew_mean_out: one value; any may be NULL.  What is read back is filled with
 * quiet NaN first.  Argument errors first (NULL inputs, sizes, block, min_tail, N > 12288), then MBD_ERR_NO_DEVICE. */
int mbd_debug_togo_step(const float* cand, const float* ybar, const float* rews, const float* rewss, int N, int H, int Nu, int block,
                        int min_tail, int lazy, float sigma, float temp, int std_guard, float alpha_i, float alpha_bar_i,
                        float alpha_bar_im1, int literal, float* ybar_out, float* R_out, float* W_out, float* rew_mean_out);
/* The refusals a zone record alone decides (include/mbd_hip.h mbd_zones) for an env of that n_track: the function the set call runs on
 * its record, host arithmetic, no device. */
int mbd_debug_check_zones(const mbd_zones* rec, int n_track);
/* A zone record's launch on the HOST: the functions the kernel calls (one text for host and device) looped over B rows of H steps
 * and K tracks on the CPU in the kernel's order; no device touched.  HOST xpos [B][H][K][3], rews [B] (may be NULL when rews_out is).
 * rews_out, pen_out, clr_out [B], step_pen_out, step_clr_out [B][H]; any output may be NULL.  The record is checked as the set call
 * checks it against n_track = K; 1 <= K <= MBD_MAX_TRACK, B * H * K <= 2^26. */
int mbd_debug_zones_host(const mbd_zones* rec, const float* xpos, const float* rews, int B, int H, int K, float* rews_out,
                         float* pen_out, float* clr_out, float* step_pen_out, float* step_clr_out);
/* zones_kernel alone on the DEVICE, on the same arguments.  What is read back is filled with all-ones bits first.  Argument errors
 * first, then MBD_ERR_NO_DEVICE. */
int mbd_debug_zones_step(const mbd_zones* rec, const float* xpos, const float* rews, int B, int H, int K, float* rews_out,
                         float* pen_out, float* clr_out, float* step_pen_out, float* step_clr_out);
/* An elite record's two batch launches alone on the DEVICE for P plans at once, on caller-given HOST arrays, keeping no sweep state:
 * elite_inject_batch_kernel, then elite_select_batch_kernel.  mask: bit k set = plan k takes part; a plan left out is neither read
 * nor written.  rews [P][N], cand [P][N][HNu] (values, or with lazy != 0 normals), ybar [P][HNu], g [HNu] or NULL, E_in
 * [P][max(n_elites, 1)][HNu] (plan k's first count_in[k] rows are read; the rest is replaced by all-ones bits), count_in [P].
 * cand_out [P][N][HNu] the candidates behind the injection; E_out, R_out, src_out [P][max(n_elites, 1)] rows; count_out, kept_out,
 * top_out [P]; any output may be NULL.  What no kernel wrote reads back with all bits set (count_out: count_in).  Argument errors
 * first (as mbd_debug_elites_inject's, P outside [1, 32]), then MBD_ERR_NO_DEVICE. */
int mbd_debug_sweep_elites_step(int P, uint32_t mask, const float* rews, const float* cand, int N, int HNu, const float* ybar, float sigma,
                                int lazy, const float* g, int n_elites, int nominal, const float* E_in, const int32_t* count_in,
                                float* cand_out, float* E_out, float* R_out, int32_t* src_out, int32_t* count_out, int32_t* kept_out,
                                float* top_out);
/* A to-go record's two batch launches alone on the DEVICE for P plans at once: togo_returns_batch_kernel, then
 * togo_update_batch_kernel under temps [P].  As mbd_debug_togo_step with a leading [P] on every array: cand [P][N][H * Nu], ybar
 * [P][H * Nu], rews [P][N], rewss [P][N][H]; ybar_out [P][H * Nu], R_out and W_out [P][G][N], rew_mean_out [P]. */
int mbd_debug_sweep_togo_step(int P, const float* temps, const float* cand, const float* ybar, const float* rews, const float* rewss,
                              int N, int H, int Nu, int block, int min_tail, int lazy, float sigma, int std_guard, float alpha_i,
                              float alpha_bar_i, float alpha_bar_im1, int literal, float* ybar_out, float* R_out, float* W_out,
                              float* rew_mean_out);
/* The reader of the device ring logs alone on the DEVICE (a pick record's ticks, an adapt and an elite record's steps): HOST ring
 * [cap][width] is uploaded as a log that has seen `count` entries, entry j at slot j % cap, and the function every peek calls reads
 * the most recent min(n, count, cap) of them into HOST out [min(n, count, cap)][width], oldest first — the two copies, the advance
 * of out between them and the scaling by width, wrapped or not.  out is filled with all-ones bits first (give it room for one
 * element where nothing is read).  The _i32 entry is the instantiation the integer logs use.  NULL arguments, width outside
 * [1, 16], cap outside [1, 65536], count < 0 or n < 0 -> MBD_ERR_INVALID before any device access; no device ->
 * MBD_ERR_NO_DEVICE. */
int mbd_debug_ring_read(const float* ring, int width, long long cap, long long count, long long n, float* out);
int mbd_debug_ring_read_i32(const int32_t* ring, int width, long long cap, long long count, long long n, int32_t* out);
#ifdef __cplusplus
}
#endif
#endif
