/*
 * mbd_hip.h — C ABI of libmbd_hip.so: the MI355X-native reverse-diffusion sampling loop of
 * LeCAR-Lab/model-based-diffusion (mbd/planners/mbd_planner.py:84-148,179-180).
 *
 * Every entry point below replaces one piece of the reference's (pure Python/JAX) plugin surface; the
 * reference file:line it stands in for is cited on each declaration.  The reference has no FFI of its own —
 * the binding a maintainer would add is the ctypes stub shown in INTEGRATION.md (and shipped as
 * model-based-diffusion_amd/mbd_hip/_capi.py).
 *
 * Conventions
 *   - plain C types only; every function returns int (0 = MBD_OK, <0 = mbd_status); no exceptions/aborts
 *     cross the ABI; mbd_last_error() returns a thread-local message for the last failure.
 *   - pointers named d_* are DEVICE pointers (HBM, caller-owned, e.g. torch.Tensor.data_ptr()); all other
 *     pointers are HOST pointers. The library never keeps a caller pointer after return.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream). Functions taking a stream are
 *     asynchronous w.r.t. the host unless documented otherwise.
 *   - all floating point data is IEEE float32, all PRNG words uint32 (reference: everything is f32,
 *     mbd_planner.py:13-14 keeps x64 disabled).
 *   - a handle is not thread-safe; distinct handles are independent.
 */
#ifndef MBD_HIP_H
#define MBD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------ */
/* status codes                                                                                      */
/* ------------------------------------------------------------------------------------------------ */
typedef enum mbd_status {
  MBD_OK = 0,
  MBD_ERR_INVALID = -1,     /* bad argument (shape, NULL, range)                                     */
  MBD_ERR_UNSUPPORTED = -2, /* env name / model feature outside the hot-path scope (-> ValueError)   */
  MBD_ERR_HIP = -3,         /* a HIP runtime call failed; message carries hipGetErrorString           */
  MBD_ERR_NO_DEVICE = -4,   /* no gfx950 device visible: the product path NEVER falls back to a CPU  */
  MBD_ERR_STATE = -5        /* call sequence error (e.g. plan used after destroy)                    */
} mbd_status;

/* ------------------------------------------------------------------------------------------------ */
/* compiled rigid-body model ("sys")                                                                 */
/* ------------------------------------------------------------------------------------------------ */
/* What brax.io.mjcf.load returns as a `System` pytree (call sites mbd/envs/humanoidrun.py:15,
 * hopper.py:14, humanoidtrack.py:16) flattened to one POD struct.  It is produced on the host by
 * mbd_hip/mjcf.py (or loaded from a committed .json) and handed to mbd_env_create_model().
 * Frames: every link carries a centre-of-mass frame whose ORIENTATION equals the link frame
 * (offset `com` only), so inverse inertia is a full symmetric body-frame tensor. */
#define MBD_MAX_LINKS 16
#define MBD_MAX_Q 40
#define MBD_MAX_ACT 24
#define MBD_MAX_COL 16
#define MBD_MAX_TRACK 8

enum mbd_reward_kind {
  MBD_REW_HUMANOIDRUN = 0,   /* mbd/envs/humanoidrun.py:46-51                                        */
  MBD_REW_HOPPER = 1,        /* mbd/envs/hopper.py:57-65 and walker2d.py:57-62: x - clip(|z - p0|,-1,1)*p1,
                                reward_params = (p0, p1) = (1.0, 0.5) hopper / (1.1, 0.5) walker2d     */
  MBD_REW_HALFCHEETAH = 2,   /* brax.envs.half_cheetah (absent from the reference tree)              */
  MBD_REW_HUMANOIDTRACK = 3, /* mbd/envs/humanoidtrack.py:87-96 (computed from the INCOMING state)   */
  MBD_REW_HUMANOIDSTANDUP = 4, /* mbd/envs/humanoidstandup.py:50-56                                   */
  MBD_REW_ANT = 6,           /* brax.envs.ant (absent): forward_reward + healthy_reward - ctrl_cost:
                                p0*(x1-x0)/dt + (p5 != 0 || p2 <= z <= p3 ? p4 : 0) - p1*|a|^2, reward_params =
                                (1, 0.5, 0.2, 1.0, 1.0, 1) — p5 = terminate_when_unhealthy (stock: on, the
                                healthy term is then a constant); recollection, unpinned                 */
  MBD_REW_CARTPOLE = 5       /* mbd/envs/cartpole.py:45: cos(q[1]) - |qd[0]| (hinge of link 1, slide of link 0) */
};

enum mbd_model_flags {
  MBD_FLAG_RESET_QUAT_RAW = 1, /* reset(): leave the noise-perturbed root quaternion un-normalised (humanoidrun.py:24-26
                                  perturbs all 7 root coordinates; whether kinematics.forward renormalises is unverified).
                                  Default 0: normalised.                                                          */
  MBD_FLAG_PLANAR = 2,         /* the model moves in the x-z plane (every hinge about the world y axis, slides and offsets
                                  in the plane, no free joint: hopper, walker2d, halfcheetah, cartpole) and is simulated by
                                  the planar restatement of the same six stages — in-plane coordinates only — instead
                                  of the general 3-D arithmetic, whose float round-off leaks 1e-5..1e-3 out of the
                                  plane over a rollout.  Set by mbd_hip/mjcf.py when the model qualifies (planar=False
                                  keeps the 3-D path); a specification of its own for these models. */
  /* ---- SPECIFICATION SWITCHES: the places where this engine had to guess at CODE level what Brax's positional
   * pipeline does.  Each bit selects the named form, in the checker and in the kernels alike (bit-exact
   * against each other either way), so that a golden vector of the real reference flips a flag instead of forcing a rewrite
   * (tools/compare_golden.py --search tries every combination).  The DEFAULT word is MBD_DEFAULT_SPEC (below): what
   * mbd_hip.mjcf.load gives a model, what the built-in models carry and what the shipped library's tuned kernels compile in
   * (mbd_tuned_spec()); a model with another word runs the general `spec` kernel instantiations. */
  MBD_FLAG_CONTACT_AVG = 4,        /* several ACTIVE contacts on one link: the link's position correction (stage 4) and —
                                      unless CONTACT6_GAUSS_SEIDEL — its velocity change (stage 6) are the AVERAGE over
                                      them (sum * 1/n, n >= 2) instead of the sum; single contacts are untouched.
                                      SET BY DEFAULT since round 6: contacts solved independently (Jacobi, below) and
                                      SUMMED blow up when a link's contacts sit close to its centre of mass — four
                                      spheres 1 cm around it turn -0.5 m/s into -9.5 m/s in ONE substep
                                      (tests/test_oracle_invariants.py) — so an engine that vmaps its contacts has to
                                      average them (Brax v1's colliders divided by the contact count); bit clear: the
                                      sum of rounds 1-5                                                                    */
  MBD_FLAG_CONTACT6_GAUSS_SEIDEL = 8, /* stage (6), collisions.resolve_velocity.  DEFAULT (bit clear, since round 5): every
                                      contact of a link computes its impulse from the SAME velocities (those stage (5)
                                      left) and the changes are added in collider order (Jacobi) — the only form Brax's code
                                      structure allows: it vmaps its contacts and segment-sums their changes per link.
                                      Bit set: one contact after the other, each seeing what the link's previous contacts
                                      left (Gauss-Seidel per link — the default of rounds 1-4, kept as the alternative)    */
  MBD_FLAG_FRICTION_VEL_BOUND = 16, /* stage (6) dynamic friction: |dv_t| = min(mu lambda_n / h, |v_t|) (Mueller et al.
                                      2020, eq. 30, literally: the bound is a velocity) instead of
                                      min(mu lambda_n / h * w_t, |v_t|) (the bound is an impulse)                         */
  MBD_FLAG_RESTITUTION_MIN = 32,   /* stage (6): the literal min(-e vn_prev, 0) of eq. 34 (Brax's sign convention unknown;
                                      with this engine's +z normal it makes elasticity a no-op) instead of max(.., 0)     */
  MBD_FLAG_EULER_EXTRINSIC = 64,   /* joints with 2 or 3 hinge dofs: q composes as rotations about the FIXED joint-frame
                                      axes (R = Rz(q2) Ry(q1) Rx(q0): gimbal axes Xc, Zp x Xc, Zp) instead of the moving
                                      ones (R = Rx(q0) Ry(q1) Rz(q2): Xp, Zc x Xp, Zc) — forward kinematics at reset, the
                                      angles / axes of stage (1) torques and stage (3) limits, observations               */
  MBD_FLAG_GYROSCOPIC = 128        /* stage (2): angular acceleration includes -I^-1 (w x I w) (Mueller et al., eq. for
                                      the velocity update); identically zero for isotropic tensors and planar models,
                                      which ignore the bit                                                                */
};
#define MBD_SPEC_FLAGS (4 | 8 | 16 | 32 | 64 | 128)
#define MBD_DEFAULT_SPEC 4 /* Jacobi per link + average over a link's active contacts */

typedef struct mbd_model {
  /* sizes */
  int32_t n_links, n_q, n_qd, n_act, n_col, n_track, n_frames, reward_kind;
  int32_t iso_inertia; /* 1: every inv_inertia is s*identity (spring_inertia_scale = 1 models)    */
  int32_t flags;       /* mbd_model_flags: named switches for the places where this engine had to GUESS what
                          Brax does — flipping one is a recompile of the model, not of the code */
  int32_t reserved_i[2];
  /* solver scalars */
  float dt;            /* physics substep (opt.timestep); control dt = dt * n_frames                */
  float vel_fac;       /* exp(vel_damping * dt)                                                     */
  float ang_fac;       /* exp(ang_damping * dt)                                                     */
  float joint_scale_pos, joint_scale_ang, collide_scale;
  float friction, elasticity;
  float gravity[3];
  float reset_noise;   /* U(-reset_noise, reset_noise) on q and qd at reset; 0 = deterministic     */
  float reward_params[8];
  /* per link */
  int32_t parent[MBD_MAX_LINKS];  /* -1 = world                                                    */
  int32_t n_rot[MBD_MAX_LINKS];   /* hinge dofs of the link's joint (0..3); -1 = free joint        */
  int32_t n_slide[MBD_MAX_LINKS]; /* slide dofs (0..3), listed before the hinges in q              */
  int32_t q_idx[MBD_MAX_LINKS], qd_idx[MBD_MAX_LINKS];
  float inv_mass[MBD_MAX_LINKS];
  float inv_inertia[MBD_MAX_LINKS][6]; /* xx yy zz xy xz yz, link frame, about the COM             */
  float com[MBD_MAX_LINKS][3];         /* COM in the link frame                                    */
  float ap_pos[MBD_MAX_LINKS][3], ap_rot[MBD_MAX_LINKS][4]; /* joint frame on the parent, in the
                                                               parent's COM frame (world if -1)   */
  float ac_pos[MBD_MAX_LINKS][3], ac_rot[MBD_MAX_LINKS][4]; /* joint frame on the child, in the
                                                               child's COM frame                  */
  float ang_damp[MBD_MAX_LINKS], vel_damp[MBD_MAX_LINKS];   /* constraint_{ang,vel}_damping        */
  float rot_lo[MBD_MAX_LINKS][3], rot_hi[MBD_MAX_LINKS][3]; /* limits on the joint-frame Euler
                                                               angles (x, y', z''), radians       */
  float rot_stiff[MBD_MAX_LINKS][3], rot_damp[MBD_MAX_LINKS][3];
  float rot_sign[MBD_MAX_LINKS][3]; /* q_k = rot_sign_k * euler_k (handedness of the MJCF axes)    */
  float slide_axis[MBD_MAX_LINKS][3][3]; /* slide axes in the joint frame                          */
  float slide_lo[MBD_MAX_LINKS][3], slide_hi[MBD_MAX_LINKS][3]; /* slide limits (metres)            */
  float slide_damp[MBD_MAX_LINKS][3];    /* MJCF joint damping of the slide dofs                    */
  /* actuators (brax.actuator.to_tau: clip to ctrlrange, * gear, scatter to the dof)               */
  int32_t act_link[MBD_MAX_ACT];
  int32_t act_slot[MBD_MAX_ACT]; /* 0..2 hinge k, 3..5 slide k                                     */
  float act_gear[MBD_MAX_ACT], act_lo[MBD_MAX_ACT], act_hi[MBD_MAX_ACT];
  /* sphere colliders vs the z = 0 plane                                                            */
  int32_t col_link[MBD_MAX_COL];
  float col_pos[MBD_MAX_COL][3]; /* sphere centre in the link's COM frame                          */
  float col_radius[MBD_MAX_COL];
  /* forward kinematics (reset only; kinematics.forward)                                            */
  float link_pos[MBD_MAX_LINKS][3], link_rot[MBD_MAX_LINKS][4]; /* link frame in the parent frame  */
  float joint_pos[MBD_MAX_LINKS][3];     /* joint anchor in the link frame                         */
  float rot_axis[MBD_MAX_LINKS][3][3];   /* hinge axes in the link frame                           */
  float slide_axis_body[MBD_MAX_LINKS][3][3];
  float init_q[MBD_MAX_Q];
  /* demo tracking (humanoidtrack.py:26-28)                                                         */
  int32_t track_link[MBD_MAX_TRACK];
} mbd_model_t;

/* Dynamic state of one environment = per link 13 floats: COM position p[3], orientation quaternion
 * r[4] = (w,x,y,z), linear velocity v[3], angular velocity w[3] (world frame).  This is brax's
 * positional State.x_i / State.xd_i — the only quantities integrated from step to step. Layout of a
 * state buffer: float[n_links][13].  car2d's state is float[3] = (x, y, theta) (car2d.py:35-40). */
#define MBD_LINK_STATE 13
#define MBD_LINK_VEL 7 /* offset of a link's linear velocity v[3] inside its 13 floats (what a plant record's kick moves) */

/* ------------------------------------------------------------------------------------------------ */
/* library                                                                                           */
/* ------------------------------------------------------------------------------------------------ */
const char* mbd_last_error(void);
int mbd_version(void);
/* The word of specification switches (mbd_model_flags, MBD_SPEC_FLAGS) this BUILD's tuned kernels compile in: models whose
 * switches equal it run them, any other word runs the general instantiations that read the switches per launch (same results,
 * a third to a half of the speed).  MBD_DEFAULT_SPEC in the shipped library; -DMBD_TUNED_SPEC=<word> rebuilds it (no
 * counterpart in the reference, whose physics has ONE specification — Brax's, which no vector pins yet). */
int mbd_tuned_spec(void);
/* number of usable gfx950 devices (0 on a box without a GPU — every compute entry then returns
 * MBD_ERR_NO_DEVICE; there is deliberately no CPU fallback in this library). */
int mbd_device_count(int* count);

/* ------------------------------------------------------------------------------------------------ */
/* JAX PRNG (threefry2x32) — replaces jax.random.{PRNGKey,split} at mbd_planner.py:40,79,103,150    */
/* host-side, pure integer arithmetic, no device needed.                                             */
/* ------------------------------------------------------------------------------------------------ */
enum mbd_prng_impl {
  MBD_PRNG_LEGACY = 0,       /* jax_threefry_partitionable = False (JAX < 0.5.0 default)            */
  MBD_PRNG_PARTITIONABLE = 1 /* jax_threefry_partitionable = True  (JAX >= 0.5.0 default)           */
};
int mbd_prng_key(uint64_t seed, uint32_t key_out[2]);
int mbd_prng_split(const uint32_t key[2], int num, int impl, uint32_t* keys_out /* [num][2] */);

/* ------------------------------------------------------------------------------------------------ */
/* environments — replaces mbd.envs.get_env (mbd/envs/__init__.py:13-33) and the env methods the    */
/* planner uses: reset (mbd_planner.py:75,80), step (:74), action_size/observation_size (:71-72),   */
/* eval_xref_logpd (:118), rew_xref (:121)                                                           */
/* ------------------------------------------------------------------------------------------------ */
typedef struct mbd_env mbd_env;

/* get_env(env_name) (mbd/envs/__init__.py:13-33): a string in, an env out.  The compiled models ("sys" of
 * humanoidrun.py:15, hopper.py:14, humanoidtrack.py:16, ...) and the demo trajectories (car2d.py:66,
 * humanoidtrack.py:33-43) are constant data inside the library, so a C caller needs no Python and no MJCF
 * compiler.  Names: car2d, hopper, halfcheetah, humanoidrun, humanoidtrack, walker2d, humanoidstandup, cartpole,
 * ant.  "pushT" (generalized backend) and unknown names return MBD_ERR_UNSUPPORTED — the Python shim raises
 * ValueError for both, like :33. */
int mbd_env_create(const char* env_name, int device, mbd_env** out);
/* the names mbd_env_create accepts: index 0, 1, ... until NULL (host only) */
const char* mbd_env_name(int index);
/* the embedded compiled model of a built-in rigid-body env (host only, no device needed) */
int mbd_builtin_model(const char* env_name, mbd_model_t* model_out);

/* The two constructors below take caller-supplied data instead (custom MJCF models compiled by
 * mbd_hip/mjcf.py, other demo paths).
 * car2d needs no model; `env_name` must be "car2d" (mbd/envs/car2d.py:43-71).  xref = demo path
 * [50][2] float32 (car2d_xref.npy cast to f32) or NULL when demos are not used. */
int mbd_env_create_car2d(int device, const float* xref, mbd_env** out);
/* rigid-body envs: humanoidrun / humanoidtrack / hopper / halfcheetah — the caller passes the
 * compiled model. xref = [n_track][50][3] float32 demo body positions or NULL. rew_xref as
 * humanoidtrack.py:44.
 * Tracked links (n_track, track_link): slot k of every rollout's positions [B][H][n_track][3], of xref and of the demo
 * log-density is link track_link[k].  Refused with MBD_ERR_INVALID before any device is looked for, the message naming the
 * field: n_track outside [0, MBD_MAX_TRACK]; a track_link[k], k < n_track, outside [0, n_links); one link in two slots (a link
 * is tracked once); MBD_FLAG_PLANAR together with n_track > 0 — the planar kernels return no positions: compile such a
 * model planar=False (mbd_hip/mjcf.py) to track its links.  Entries of track_link at or past n_track are not read. */
int mbd_env_create_model(const char* env_name, int device, const mbd_model_t* model,
                         const float* xref, float rew_xref, mbd_env** out);
int mbd_env_destroy(mbd_env* env);

/* action_size / observation_size / state record size (floats) / H limit of the demo (0 = none)   */
int mbd_env_info(const mbd_env* env, int* action_size, int* observation_size, int* state_size,
                 int* n_links, int* n_frames, float* dt);
/* reset(rng) -> state (humanoidrun.py:19-32, hopper.py:20-34, humanoidtrack.py:48-61, car2d.py:73-75).
 * Host computation (forward kinematics once per run). state_out: float[state_size] HOST. */
int mbd_env_reset(const mbd_env* env, const uint32_t key[2], int prng_impl, float* state_out);
/* PipelineEnv.pipeline_init(q, qd) -> pipeline_state (the call every wrapper's reset ends in: humanoidrun.py:29,
 * hopper.py:30, walker2d.py:29, humanoidstandup.py:29, cartpole.py:29, humanoidtrack.py:54): forward kinematics of the
 * generalized coordinates — a state to plan FROM that is not a reset (receding-horizon use).  q: float[n_q] (free root:
 * position, quaternion w-first — normalised like reset's unless MBD_FLAG_RESET_QUAT_RAW), qd: float[n_qd]; n_q / n_qd must
 * be the model's (mbd_env_get_model).  car2d: q = (x, y, theta), n_q = 3, qd ignored (may be NULL, n_qd = 0).  Host
 * arithmetic, no device needed; all pointers HOST. */
int mbd_env_pipeline_init(const mbd_env* env, const float* q, int n_q, const float* qd, int n_qd, float* state_out);
/* step(state, action) -> (state', reward, obs) for ONE environment (rendering / verification path,
 * mbd_planner.py:163; utils.py:23-33).  Runs the same HIP rollout kernel with B=1,H=1; synchronous.
 * All pointers HOST. reward_out / obs_out (float[observation_size], see mbd_env_observe) may be NULL. */
int mbd_env_step(mbd_env* env, const float* state_in, const float* action, float* state_out,
                 float* reward_out, float* obs_out);
/* rew_xref (car2d.py:71, humanoidtrack.py:44) */
int mbd_env_rew_xref(const mbd_env* env, float* out);
/* env.sys (mbd_planner.py:174; humanoidrun.py:15): a copy of the env's compiled model */
int mbd_env_get_model(const mbd_env* env, mbd_model_t* model_out);
/* env.xref (mbd_planner.py:167; car2d.py:66 [50][2], humanoidtrack.py:36-43 [n_track][50][3]) copied to the HOST
 * buffer xref_out[capacity]; count_out = number of floats (0: the env has no demonstration). xref_out may be NULL. */
int mbd_env_xref(const mbd_env* env, float* xref_out, int capacity, int* count_out);
/* jax.vmap(env.eval_xref_logpd)(qs) (mbd_planner.py:118; humanoidtrack.py:98-106, car2d.py:95-102):
 *   d_xpos      : [B][H][K][3] tracked link positions after every control step (car2d: [B][H][3] = q) — the
 *                 d_xpos output of mbd_env_rollout
 *   d_logpd_out : [B]
 * H must be 50 (the demos have 50 rows). asynchronous on `stream`.  A candidate with a NaN position gets a NaN (jnp.clip
 * keeps a NaN distance); an infinite one a saturated term. */
int mbd_env_xref_logpd(const mbd_env* env, const float* d_xpos, int B, int H, float* d_logpd_out, void* stream);
/* _get_obs (humanoidrun.py:43-44, hopper.py:49-55, car2d.py:86; brax ant / half_cheetah) of ONE state:
 * kinematics.inverse on the host (the planner never reads observations, mbd_planner.py:71 — API parity only).
 * state: float[state_size] HOST; obs_out: float[observation_size] HOST. */
int mbd_env_observe(const mbd_env* env, const float* state, float* obs_out);
/* the same from a bare model, plus the generalized coordinates: q_out[n_q], qd_out[n_qd], obs_out — any may be
 * NULL.  Pure host arithmetic, no device needed. */
int mbd_model_observe(const mbd_model_t* model, const float* state, float* q_out, float* qd_out, float* obs_out);

/* pipeline_init from a bare model (the inverse of mbd_model_observe's q_out / qd_out): q[model->n_q], qd[model->n_qd] ->
 * state_out[13 * n_links].  Pure host arithmetic, no device needed. */
int mbd_model_forward(const mbd_model_t* model, const float* q, const float* qd, float* state_out);

/* Batched rollout = jax.vmap(rollout_us, in_axes=(None,0)) (mbd_planner.py:109, utils.py:14-20).
 *   d_state0 : [state_size]        one initial state shared by all B candidates
 *   d_us     : [B][H][Nu]          action sequences
 *   d_rewss  : [B][H]              reward after every control step
 *   d_xpos   : [B][H][K][3] or NULL  world positions of the K tracked links after every step
 *                                  (car2d: [B][H][3] = q).  Only what eval_xref_logpd consumes of the
 *                                  reference's `pipline_states` output.
 *   d_state_final : [B][state_size] or NULL
 * asynchronous on `stream`.
 * Candidates are independent, also where one of them leaves the finite numbers (a rollout that diverges from finite inputs:
 * summed contacts, a huge gear): every other candidate's rewards, positions and final state are bit for bit what they are
 * without it, in every launch form, and the diverged candidate's outputs are non-finite wherever the specification's are —
 * never a finite number that hides it.  (NaN payloads and which non-finite value appears are not part of the contract.) */
int mbd_env_rollout(mbd_env* env, const float* d_state0, const float* d_us, int B, int H,
                    float* d_rewss, float* d_xpos, float* d_state_final, void* stream);

/* ------------------------------------------------------------------------------------------------ */
/* planner fast path — replaces reverse_once / reverse / run_diffusion (mbd_planner.py:97-151,179)  */
/* ------------------------------------------------------------------------------------------------ */
typedef struct mbd_plan mbd_plan;

typedef struct mbd_plan_config {
  int32_t Nsample;     /* GLOBAL number of candidates N (Args.Nsample, mbd_planner.py:29)           */
  int32_t Hsample;     /* horizon H (Args.Hsample :30)                                              */
  int32_t Ndiffuse;    /* diffusion steps (Args.Ndiffuse :31)                                       */
  float temp_sample;   /* (:32)                                                                     */
  float beta0, betaT;  /* (:33-34)                                                                  */
  int32_t enable_demo; /* (:35)                                                                     */
  int32_t prng_impl;   /* mbd_prng_impl                                                             */
  int32_t shard_begin; /* this process owns candidates [shard_begin, shard_begin + shard_count)     */
  int32_t shard_count; /* = Nsample on one GPU                                                      */
  int32_t literal_score; /* 1: evaluate score/Yim1/Ybar_im1 literally (:130-133); 0: use identity   */
  int32_t update_method; /* 0 = MBD (mbd_planner.py); path-integral baselines of
                            mbd/planners/path_integral.py:33-52 on the same rollout kernel:
                            1 = mppi (softmax_update), 2 = cma-es, 3 = cem. For these Ndiffuse plays
                            Nrefine (:28), sigma is a carried scalar starting at 1.0 (:131), the
                            standardisation has no zero-std guard (:123) and demos are not used.      */
  int32_t shares_device; /* 1: other plans run on this GPU at the same time (plans of a sweep on separate streams):
                            the plan then generates each step's normals in front of its rollout instead of one step
                            ahead in workgroups / on a stream the other plans need (results identical either way)  */
  int32_t reserved[3];
} mbd_plan_config;

int mbd_plan_create(mbd_env* env, const mbd_plan_config* cfg, mbd_plan** out);
int mbd_plan_destroy(mbd_plan* plan);
/* noise schedule (mbd_planner.py:84-87): copies alphas, alphas_bar, sigmas ([Ndiffuse] each, HOST) */
int mbd_plan_schedule(const mbd_plan* plan, float* alphas, float* alphas_bar, float* sigmas);
/* state_init = reset(rng_reset) (mbd_planner.py:79-80): uploads a HOST state to the plan */
int mbd_plan_set_state0(mbd_plan* plan, const float* state0);

/* ---- one reverse-diffusion step, split at the (only) exchange point so that N can be sharded ---- */
/* phase 1 (mbd_planner.py:103-110): eps -> Y0s = clip(eps*sigma_i + Ybar_i) for the local shard,
 * rollout, rews = mean_H(rewss) [+ demo log-densities].  (MBD plans on rigid-body envs keep eps and form the
 * candidate values where they are consumed — the rollout's action fetch, the weighted mean, mbd_plan_peek — with the
 * same two roundings; d_Ybar_i must stay unchanged until phase 2 of the step has run.)  d_Ybar_i [H][Nu] (device, read), key_sample
 * is Y0s_rng of (:103).  Writes d_rews_local [shard_count] and, with demos, d_logpd_local
 * [shard_count] (else may be NULL).  async on stream. */
int mbd_plan_sample_rollout(mbd_plan* plan, int i, const uint32_t key_sample[2],
                            const float* d_Ybar_i, float* d_rews_local, float* d_logpd_local,
                            void* stream);
/* Optional hint BEFORE phase 1: declares key_next, the Y0s_rng of the diffusion step AFTER the one the next
 * mbd_plan_sample_rollout runs.  Its normals (jax.random.normal(Y0s_rng, ...), mbd_planner.py:104 — they depend on that
 * step's key only) are then generated beside that rollout: in spare workgroups of the rollout launch itself when it
 * leaves CUs idle, on the plan's second stream otherwise; the declared step finds them ready when its key_sample
 * equals key_next and generates its own otherwise.  Results are bit-identical with and without the hint.  Plans that
 * materialise Y0s (car2d, path-integral updates) ignore it.  `stream` is unused (kept for ABI stability). */
int mbd_plan_prefetch_noise(mbd_plan* plan, const uint32_t key_next[2], void* stream);
/* phase 2 (mbd_planner.py:111-135): from ALL N rewards (after the all-gather) standardise, demo
 * blend, softmax, weighted mean over all N candidates (noise regenerated from the counter-based PRNG,
 * so the result is bit-identical on every rank and for every shard layout), score update.
 * Writes d_Ybar_im1 [H][Nu] and d_rew_mean [1] (= rews.mean(), :135). async on stream.
 * (The phases of a plan may be issued on different streams: the library orders each call behind the plan's previous
 * one with an event when the stream changes — the normals prepared by one step's launch are read by the next.) */
int mbd_plan_score_update(mbd_plan* plan, int i, const uint32_t key_sample[2], const float* d_Ybar_i,
                          const float* d_rews_all, const float* d_logpd_all, float* d_Ybar_im1,
                          float* d_rew_mean, void* stream);
/* path-integral plans: the carried sampling sigma (path_integral.py:113,131). set before the first
 * step (mbd_plan_run does it itself); synchronous.  After an episode with a sigma record (mbd_mpc_sigma, below), and between
 * the ticks of a session, mbd_plan_get_sigma returns the sigma the NEXT tick starts from (after mbd_plan_mpc_reset_mean:
 * sigma_cold). */
int mbd_plan_set_sigma(mbd_plan* plan, float sigma);
int mbd_plan_get_sigma(mbd_plan* plan, float* sigma_out);
/* single-GPU convenience = reverse_once (mbd_planner.py:97-135): phase 1 + phase 2 on `stream`;
 * key_inout is advanced exactly as `rng, Y0s_rng = split(rng)` (:103). async; d_Ybar updated in
 * place; d_rew_mean [1]. */
int mbd_plan_reverse_once(mbd_plan* plan, int i, uint32_t key_inout[2], float* d_Ybar,
                          float* d_rew_mean, void* stream);
/* Host blocking of the phase calls: a plan whose next step's normals are generated on its second stream (plans that
 * fill the chip) keeps the host at most one step ahead of the device — mbd_plan_sample_rollout may then sleep up to 5 ms
 * (mbd_plan_run / mbd_sweep_run: 20 ms) for the previous rollout to START; when the stream is slower than that (a shared
 * or time-sliced GPU, earlier work on the caller's stream, a profiler) the call falls back to ordering its two streams
 * with an event and returns — a slow stream is never an error. */
/* whole reverse loop = reverse() (mbd_planner.py:138-148) + final evaluation (:179-180).
 * key = rng_exp of (:150).  mu_0ts_out HOST [Ndiffuse-1][H][Nu] (the array saved at :156),
 * rew_means_out HOST [Ndiffuse-1] (the tqdm postfix values, :147) — either may be NULL.
 * Synchronous; one device->host copy at the end instead of the reference's per-step sync. */
int mbd_plan_run(mbd_plan* plan, const uint32_t key[2], float* mu_0ts_out, float* rew_means_out,
                 float* rew_final_out, double* loop_seconds_out);
/* rew_final = rollout_us(state_init, Y).mean() for one plan Y [H][Nu] HOST (mbd_planner.py:179-180) */
int mbd_plan_eval(mbd_plan* plan, const float* Y, float* rew_final_out);

/* ---- receding horizon (no counterpart in the reference, which plans open loop) ---- */
typedef struct mbd_mpc_config {
  int32_t n_ticks;     /* T >= 1 */
  int32_t warm_steps;  /* K: diffusion steps i = K..1 of every tick after the first, 1 <= K <= Ndiffuse-1 */
  int32_t exec_steps;  /* E: control steps executed per tick, 1 <= E < Hsample; the mean then shifts by E */
  int32_t reserved[5]; /* must be 0 */
} mbd_mpc_config;
/* Closed-loop episode from the plan's state0 s_0: every tick t replans from the state s_t the system reached and executes the
 * first E rows of that plan through the env's rollout path, on the device, with no host synchronisation between ticks.
 *   rng = key; Ybar = zeros; i_start = Ndiffuse-1                  (tick 0: a cold plan, exactly mbd_plan_run's loop)
 *   per tick t:  rng, k_t = split(rng)
 *                Ybar = reverse_once(i, ., Ybar) from s_t for i = i_start .. 1, key chain from k_t  -> M_t [H][Nu]
 *                rewards[tE .. tE+E), s_{t+1} = rollout(s_t, M_t[0:E])   (rows fed unclipped; the env clips)
 *                Ybar = M_t shifted E rows forward, the last E rows 0 (the cold prior); i_start = K
 * so tick 0 equals mbd_plan_run(plan, k_0) bit for bit, and an episode of T ticks is a prefix of one of T+1.  K sets both
 * the cost of a tick and the noise level sigma_K it restarts from.
 * HOST outputs, each may be NULL: actions_out [T*E][Nu] (the rows executed), rewards_out [T*E], states_out
 * [T+1][state_size] (s_0 .. s_T), means_out [T][H][Nu] (M_t); loop_seconds_out: wall time of the tick loop.
 * Synchronous; ONE device->host copy per output at the end.  The plan's state0 is unchanged afterwards.
 * Unsharded plans; demo plans need a demo record (mbd_plan_set_mpc_demo below) and path-integral plans a sigma record
 * (mbd_plan_set_mpc_sigma below, which also says what their episode is): NULL plan / config / key and out-of-range fields ->
 * MBD_ERR_INVALID (the NULL checks before any device access), enable_demo without a demo record or a path-integral update
 * (update_method != 0) without a sigma record -> MBD_ERR_UNSUPPORTED (demos are time-indexed: the record is the clock that
 * follows the episode; a path-integral plan carries a sigma an episode has to be told how to restart), a sharded plan ->
 * MBD_ERR_STATE. */
int mbd_plan_run_mpc(mbd_plan* plan, const mbd_mpc_config* mc, const uint32_t key[2], float* actions_out,
                     float* rewards_out, float* states_out, float* means_out, double* loop_seconds_out);

/* ---- path-integral episodes: mppi, cma-es and cem as receding-horizon controllers (path_integral.py:111-127 is the open-loop
 * refinement loop; the reference has no episode; DESIGN.md section 1 "N12 path-integral episodes") ---- */
/* A sigma record turns a path-integral plan (update_method 1 / 2 / 3) into one that episodes accept, and says what sigma a tick
 * starts from.  A setting of a plan (of a sweep) beside the plant, delay and noise records, read by mbd_plan_run_mpc,
 * mbd_plan_mpc_open and mbd_sweep_run_mpc only: mbd_plan_run, mbd_sweep_run and the phase calls ignore it, and mbd_plan_run's
 * own reset of sigma to 1 is untouched.  The record is the switch: without one a path-integral handle stays refused. */
typedef struct mbd_mpc_sigma {
  float sigma_cold;    /* > 0, finite: sigma at the first step of a cold tick (tick 0; a session's tick after
                          mbd_plan_mpc_reset_mean).  1.0 is path_integral.py:131 */
  float sigma_warm;    /* > 0, finite: sigma at the first step of every other tick */
  float gain;          /* >= 0, finite.  0: a warm tick starts at sigma_warm.  > 0 (cma-es only, needs sigma_warm <= sigma_cold):
                          it starts at clamp(gain * sigma_end of the previous tick, sigma_warm, sigma_cold) */
  int32_t reserved[5]; /* must be 0 */
} mbd_mpc_sigma;
/* With a record the episode of mbd_plan_run_mpc (above) is — everything not shown is unchanged:
 *   rng = key; mu = zeros; n_it = Ndiffuse-1; sigma = sigma_cold
 *   per tick t:  rng, k_t = split(rng);  r = k_t;  sigmas[t][0] = sigma
 *                n_it times:  r, ks = split(r)
 *                             Y0s  = clip(normal(ks, (N,H,Nu)) * sigma + mu)     (path_integral.py:116-119; under a noise shape
 *                                                                                 or basis what mbd_plan_run forms for this plan)
 *                             rews = mean_H(rollout(s_t, Y0s))                   (from the predicted state under a delay record)
 *                             mu, sigma = update_fn(softmax(standardise(rews)/temp), Y0s, sigma, mu)   (:122-125, no zero-std guard)
 *                M_t = mu;  sigmas[t][1] = sigma
 *                execute M_t[0:E] as above / as the plant and delay records say;  mu = shift_E(M_t);  n_it = K
 *                sigma = sigma_warm                        if gain == 0
 *                      = x, three separately rounded f32 steps, no fma:
 *                          x = fl32(gain * sigma);  x = x < sigma_warm ? sigma_warm : x;  x = x > sigma_cold ? sigma_cold : x
 *                        (so that a NaN sigma stays NaN)
 * For mppi and cem sigma never changes within a tick, so gain > 0 is refused there rather than silently meaningless; cma-es'
 * sigma collapses as it converges, and gain lets a warm tick's regrowth follow how converged the last tick was.
 * Bit for bit: with sigma_cold = 1, tick 0's mean and sigma are mbd_plan_run(k_0)'s; an episode of T ticks is a prefix of one of
 * T + 1; the record {1, 1, 0} makes every tick the reference's update() from the shifted mean, with K refinements.
 * On the device the carried sigma never leaves it: one launch of one small kernel per tick boundary (and one in front of tick 0)
 * logs it and forms the next — no host write of sigma inside the tick loop, no synchronisation.
 * The plant record, the delay record (the prediction is unchanged: one candidate on the plan's env) and the noise shape and basis,
 * in both `when` modes, compose as for MBD episodes; the first normals of a tick are sampled in the tick.  An ensemble record
 * stays refused for path-integral plans, and a path-integral handle with demos cannot be created.
 * The set call copies the record; rec == NULL clears it and brings the run call's refusal back.  Refused before any device access,
 * the message naming the field: a NULL handle -> MBD_ERR_INVALID; update_method == 0 -> MBD_ERR_STATE ("not a path-integral
 * plan"); a session open on the handle -> MBD_ERR_STATE; a non-finite or non-positive sigma_cold / sigma_warm, a negative or
 * non-finite gain, gain > 0 with update_method != 2, gain > 0 with sigma_warm > sigma_cold, non-zero reserved -> MBD_ERR_INVALID. */
int mbd_plan_set_mpc_sigma(mbd_plan* plan, const mbd_mpc_sigma* rec);
/* the sigmas of the last episode run with a record (synchronises the device): HOST sigmas_out [T][2] — what tick t started from
 * and ended with; may be NULL.  MBD_ERR_STATE without a record, or before an episode has run with one (sessions keep no log). */
int mbd_plan_peek_mpc_sigma(mbd_plan* plan, float* sigmas_out);

/* ---- the plant of an episode: a system that is NOT the planner's model (DESIGN.md section 1 "N5 plant") ---- */
/* A plant record names the env that executes a closed-loop episode's rows, and the episode's disturbances.  It is a setting
 * of the plan (of an episode of a sweep) that mbd_plan_run_mpc (mbd_sweep_run_mpc) reads; mbd_plan_run / mbd_sweep_run ignore
 * it.  Without a record the two run calls are unchanged: same launches, same bits. */
typedef struct mbd_mpc_plant {
  mbd_env* plant;      /* the env that executes the rows; NULL = the plan's own env.  Not owned: the caller keeps it alive */
  uint32_t key[2];     /* the disturbance key; its chain is separate from the episode's key chain */
  float act_std;       /* >= 0: std of the normal noise added to every executed action (before the env's clip) */
  float kick_std;      /* >= 0: std per component (m/s) of the velocity kick on link 0 */
  int32_t kick_every;  /* >= 1: a kick at the end of every tick t with (t+1) % kick_every == 0 */
  int32_t reserved[3]; /* must be 0 */
} mbd_mpc_plant;
/* With a plant record, the episode of mbd_plan_run_mpc (above) becomes — everything not shown is unchanged; the planner
 * always plans with the PLAN's env, from the state the PLANT reached:
 *   dk = rec.key
 *   per tick t:  M_t as above (from s_t, the plan's env, the episode's key chain)
 *                dk, d_t = split(dk)                                  (the plan's prng_impl)
 *                eps = normal(d_t, (E*Nu + 3,))                       (always this many, whatever is switched on)
 *                rows = M_t[0:E]                         if act_std == 0  (copied, not computed: -0.0 stays -0.0)
 *                     = M_t[0:E] + act_std * eps[0:E*Nu]  otherwise       (f32 product, then f32 sum: two roundings, no fma)
 *                rewards[tE .. tE+E), s' = rollout_PLANT(s_t, rows)   (the plant env's rollout path and its reward)
 *                if kick_std > 0 and (t+1) % kick_every == 0:
 *                  s'.v[link 0] += kick_std * eps[E*Nu .. E*Nu+3)     (f32 product then sum; planar models,
 *                                                                      MBD_FLAG_PLANAR: the y component is not applied)
 *                s_{t+1} = s';  Ybar = shift_E(M_t)                   (the shift takes the UNDISTURBED mean)
 * actions_out then holds `rows` (what the plant was fed), means_out the undisturbed M_t, rewards_out the plant's rewards,
 * states_out the states after the kick.  A record with plant NULL (or a second env of the same model) and both stds 0 gives
 * the episode without a record bit for bit; the prefix property and "tick 0's mean is mbd_plan_run(k_0)'s" hold with any
 * record.  Still no host synchronisation between ticks: the disturbances are drawn and applied on the device.
 * The record is copied and stays until cleared (rec == NULL) or the handle is destroyed.  Refused at the set call, before
 * any launch: NULL plan -> MBD_ERR_INVALID; a plant on another device, or whose n_links (hence state_size) / action_size / planar
 * flag differ from the plan's env -> MBD_ERR_INVALID naming the field; a negative or non-finite std, kick_every < 1, non-zero
 * reserved -> MBD_ERR_INVALID; kick_std > 0 on an env whose link 0 cannot translate freely in its plane ->
 * MBD_ERR_UNSUPPORTED (allowed iff the model's n_rot[0] == -1, a free joint, or it is planar with n_slide[0] >= 2; refused for
 * cartpole's cart on a rail and for car2d, which has no links).  act_std works for every env. */
int mbd_plan_set_mpc_plant(mbd_plan* plan, const mbd_mpc_plant* rec);

/* ---- ensembles: planning over perturbed copies of the model (domain randomisation; no counterpart in the reference, which
 * scores every candidate on one nominal model; DESIGN.md section 1 "N6 ensemble") ---- */
#define MBD_MAX_ENSEMBLE 8
enum mbd_risk_mode {
  MBD_RISK_MEAN = 0, /* a candidate's reward is its mean over the members */
  MBD_RISK_MIN = 1   /* ... its worst over the members */
};
/* An ensemble record is a setting of a plan, like the plant record: the M member envs every candidate is rolled out on, and how
 * the M returns become the candidate's reward. */
typedef struct mbd_ensemble {
  mbd_env* members[MBD_MAX_ENSEMBLE]; /* entries [0, n_members); NULL = the plan's own env.  Not owned: the caller keeps them alive */
  int32_t n_members;                  /* M, 1 <= M <= MBD_MAX_ENSEMBLE */
  int32_t risk;                       /* mbd_risk_mode */
  int32_t reserved[6];                /* must be 0 */
} mbd_ensemble;
/* With a record, diffusion step i becomes — everything not shown is unchanged:
 *   eps, Y0s = as without a record (ONE set of normals and candidates, from the step's key; mbd_planner.py:103-106)
 *   for m in 0..M-1:  r_m[n] = mean_H( rollout_{member m}(state0, Y0s[n]) )   (each exactly what that env's rollout path gives)
 *   rews[n] = ((r_0[n] + r_1[n]) + ... + r_{M-1}[n]) / float(M)               MBD_RISK_MEAN: f32, left to right, ONE division
 *           = min(min(r_0[n], r_1[n]), ...)                                   MBD_RISK_MIN: left to right
 *             (min(a, b) = b if b < a or b is NaN, else a: a member whose rollout diverged to NaN makes the candidate's
 *             reward NaN under MIN as it does under MEAN — a diverged member is the worst case, never hidden)
 *   standardise, softmax, weighted mean, score update on rews as without a record; rew_mean out = rews.mean()
 * Hence: a plan without a record is unchanged (same launches, same bits); a record of M = 1 whose member is NULL, or a second
 * env of the same model, gives the plan without a record under either risk mode; MIN does not depend on the members' order;
 * r_m equals mbd_env_rollout on member m's env for the same Y0s.  mbd_plan_eval and the final reward of mbd_plan_run keep
 * using the plan's own env.  One rollout launch over the M * Nsample candidates per step (a wavefront picks its member's model
 * in its prologue) and one small launch that combines the M rows in front of the score; when Nsample is not a multiple of the
 * candidates a wavefront of the chosen instantiation holds, M rollout launches on the plan's stream instead (same bits).
 * The record is read by mbd_plan_sample_rollout (whose d_rews_local receives the COMBINED rewards; mbd_plan_score_update is
 * unchanged), mbd_plan_reverse_once, mbd_plan_run and mbd_plan_run_mpc — there the planner plans with the ensemble from the
 * state the plant reached, and the executed rows still go through the plant's env (the plan's env without a plant record).
 * The record is copied and stays until cleared (rec == NULL) or the handle is destroyed.  Refused at the set call, before any
 * launch, each message naming the field.  MBD_ERR_INVALID: NULL plan; n_members outside [1, MBD_MAX_ENSEMBLE]; an unknown risk;
 * non-zero reserved; a member on another device; a member that differs from the plan's env in anything that decides a launch
 * or a template parameter — n_links (hence state_size), action_size (n_act), the planar flag, the spec-flag word (flags),
 * reward_kind, n_frames, colliders per link, the tree and lane tables, the demo reference table xref (a tracking reward reads it), iso_inertia / the inertia shape, and the wave-uniform
 * switches slide_limits, max_children, max_rot, any_stiff, has_weld.  Members may differ in data only — masses, inertias,
 * friction, gears, damping and the like: everything mbd_hip.model.Model.scaled produces is accepted.  MBD_ERR_UNSUPPORTED:
 * enable_demo (which member's log-density would count?), a path-integral update_method, car2d (it has no model).
 * MBD_ERR_STATE: a sharded plan.  Sweeps (mbd_sweep_*) take no ensemble: at M = 4 a single plan already fills the chip. */
int mbd_plan_set_ensemble(mbd_plan* plan, const mbd_ensemble* rec);
/* the last step's per-member rewards r_m, rews_members_out [M][Nsample], and the combined rewards, rews_out [Nsample] (HOST;
 * either may be NULL; synchronises the device).  MBD_ERR_STATE without a record or before the first step with one.  With a
 * record, mbd_plan_peek's rewss_out is member 0's. */
int mbd_plan_peek_ensemble(mbd_plan* plan, float* rews_members_out, float* rews_out);

/* ---- noise shapes: the sampling noise per horizon row and actuator (no counterpart in the reference, whose sigma_i is one
 * scalar per diffusion step; DESIGN.md section 1 "N7 noise shape") ---- */
#define MBD_NOISE_ALWAYS     0  /* every diffusion step of every call that samples */
#define MBD_NOISE_WARM_TICKS 1  /* only the steps of ticks t >= 1 of mbd_plan_run_mpc / mbd_sweep_run_mpc */
/* A noise shape is a table g [Hsample][action_size] of finite floats >= 0, a setting of a plan (of a sweep) beside the plant
 * and ensemble records.  With a shape in force, a candidate element of diffusion step i is
 *   z   = eps[n][h][a] * g[h][a]                   (eps: the normals the plan draws anyway: same key, counters, layout)
 *   Y0s = clip((z * sigma_i) + Ybar_i[h][a], -1, 1)
 * three float32 operations, each rounded, no fma; sigma_i is the schedule's, or a path-integral plan's carried sigma.
 * Everything else of the step is unchanged — the rollout, mean_H, standardisation, softmax, the weighted mean over these same
 * candidates, the score update, the path-integral updates.  Hence, bit for bit: a table of all ones is no shape at all
 * (x * 1 = x, -0.0 and NaN included), and a row or column of zeros freezes those elements at clip(Ybar_i).  The table is
 * applied where the normals are produced, so mbd_plan_peek's Y0s are the shaped candidates; the disturbance normals of a
 * plant record (mbd_mpc_plant) are never shaped.
 * MBD_NOISE_WARM_TICKS exists for receding-horizon episodes, whose warm ticks restart at sigma_K: the rows a shift has just
 * appended get a larger g (a horizon-row schedule), while mbd_plan_run, mbd_sweep_run, the phase calls and tick 0 of an
 * episode stay flat — tick 0 is still mbd_plan_run(k_0), and an episode of T ticks still a prefix of one of T + 1.  Under
 * MBD_NOISE_ALWAYS both hold as well, with the shape in both.
 * Every plan that samples takes a shape: MBD and path-integral updates, rigid-body envs and car2d, sharded plans (every rank
 * sets the same record: the table is indexed by the global element), plans with a plant or an ensemble record, sweeps.
 * The set call copies the table, is synchronous (it waits for the device) and discards normals prepared ahead for a key_next
 * (mbd_plan_prefetch_noise), so no step consumes normals scaled under the previous setting; call it between diffusion steps,
 * not between the two phases of one.  rec == NULL clears.  Refused with MBD_ERR_INVALID before any device access, the message
 * naming the field: a NULL handle, non-zero reserved, an unknown when, a NULL scale, rows / cols below 1, a negative or
 * non-finite scale value, rows != Hsample, cols != action_size. */
typedef struct mbd_noise_shape {
  const float* scale;   /* HOST [rows][cols], copied by the set call */
  int32_t rows, cols;   /* must equal Hsample, action_size */
  int32_t when;         /* MBD_NOISE_ALWAYS or MBD_NOISE_WARM_TICKS */
  int32_t reserved[5];  /* must be 0 */
} mbd_noise_shape;
int mbd_plan_set_noise_shape(mbd_plan* plan, const mbd_noise_shape* rec);

/* ---- noise bases: the sampling noise correlated along the horizon through a few knots per actuator (no counterpart in the
 * reference, whose normals are white along the horizon; DESIGN.md section 1 "N8 noise basis") ---- */
#define MBD_MAX_KNOTS 16
/* A noise basis is a table W [Hsample][n_knots] of finite floats of any sign, 1 <= n_knots <= MBD_MAX_KNOTS, a setting of a
 * plan (of a sweep) beside the noise shape.  With a basis in force a diffusion step draws
 *   eps = normal(key, (Nsample, n_knots, action_size))
 * INSTEAD of the (Nsample, Hsample, action_size) tensor — the step's own sampling key, the plan's prng_impl, and the counters
 * and pairing those give a tensor of Nsample n_knots action_size elements (the legacy layout pairs element j with j + half,
 * the padded last block as for every other normal of the library) — and a candidate element of step i is
 *   c = +0.0f;  for k = 0 .. n_knots-1, ascending:  if (W[h][k] != 0) c = c + (W[h][k] * eps[n][k][a])   (two roundings a term)
 *   z = c                        without a noise shape
 *   z = c * g[h][a]              with one: the basis first, then the shape
 *   Y0s = clip((z * sigma_i) + Ybar_i[h][a], -1, 1)
 * float32 operations, each rounded, no fma.  Terms whose weight is exactly zero (of either sign) are left out, so a sparse
 * basis — interpolation, hold — may be evaluated per element or per column with the same bits.  Everything else of the step is
 * unchanged: the rollout, mean_H, standardisation, softmax, the weighted mean over these same candidates in the full [H][Nu]
 * space, the score update, the path-integral updates.  Hence: a row of zeros in W freezes that horizon row at clip(Ybar_i),
 * z = +0; and with n_knots = Hsample <= 16 and W the identity the plan equals the plan without a basis in value (only the sign
 * of a zero normal may differ).  The disturbance normals of a plant record are the world's and pass no basis.
 * `when` takes mbd_noise_shape's two values with their meaning; a plan may carry a shape and a basis with different `when`.
 * Every plan that samples takes a basis, as it takes a shape.  The set call copies the table, is synchronous (it waits for
 * the device) and discards normals prepared ahead for a key_next, so no step consumes normals made under the previous setting;
 * call it between diffusion steps.  rec == NULL clears.  Refused with MBD_ERR_INVALID before any device access, the message
 * naming the field: a NULL handle, a NULL basis, n_knots outside [1, MBD_MAX_KNOTS], a non-finite basis value, an unknown
 * when. */
typedef struct mbd_noise_basis {
  const float* basis;  /* HOST [Hsample][n_knots], copied by the set call */
  int32_t n_knots;     /* 1 .. MBD_MAX_KNOTS */
  int32_t when;        /* MBD_NOISE_ALWAYS or MBD_NOISE_WARM_TICKS */
} mbd_noise_basis;
int mbd_plan_set_noise_basis(mbd_plan* plan, const mbd_noise_basis* rec);

/* ---- the objective: what a plan maximises (no counterpart in the reference, whose plans maximise the unweighted mean of the
 * env's per-step rewards, mbd_planner.py:110; DESIGN.md section 1 "N13 objective") ---- */
/* An objective record is a setting of a plan (of a sweep) beside the ensemble and noise records: weights over the horizon's rows —
 * a discount, a terminal weight —, an effort cost and a rate cost that are the controller's, not the env's, and the action the
 * system executed just before the plan begins, which the rate cost's first term is taken against. */
typedef struct mbd_objective {
  const float* row_weight;  /* HOST [Hsample] or NULL: w[h], finite, >= 0, f32 left-to-right sum > 0 and finite */
  const float* act_weight;  /* HOST [action_size] or NULL (= ones): q[a], finite, >= 0 */
  const float* prev0;       /* HOST [action_size] or NULL: the action executed before row 0 of the first plan */
  float effort;             /* lambda_u  >= 0, finite */
  float rate;               /* lambda_du >= 0, finite */
  int32_t rows, cols;       /* must equal Hsample, action_size */
  int32_t reserved[5];      /* must be 0 */
} mbd_objective;
/* With a record in force, phase 1 of a diffusion step leaves in the rewards buffer, in place of mean_H(rewss) — f32 throughout,
 * every operation rounded, no fma (H = Hsample, N = Nsample; row b of the launch is candidate b of the shard, under an ensemble
 * record row b of the M N rows is candidate b % N on member b / N):
 *   ret[b]  = rews[b] as the rollout stored it                          row_weight == NULL (copied, not recomputed)
 *           = acc / wsum,  acc = +0; for h ascending: acc = acc + (w[h] * rewss[b][h])
 *             wsum = f32 left-to-right sum of w, formed once on the host by the set call
 *   u[n][h][a] = the candidate value the rollout fetched: Y0s, or clip((z*sigma) + Ybar_i[h][a], -1, 1) from the normals z the
 *                plan keeps, with the sampler's two roundings (z is already shaped or basis-spread where those records are in force)
 *   per actuator a:  eff_a = +0; rat_a = +0
 *                    for h ascending:
 *                        eff_a = eff_a + (u*u)
 *                        d = u - u_prev;  rat_a = rat_a + (d*d)
 *                            u_prev = u[n][h-1][a] for h >= 1
 *                            u_prev = prev[a] for h = 0; without a previous action the h = 0 term is left out
 *   cost[n] = (c / float(H)),  c = +0; for a ascending: c = c + (q[a] * ((effort * eff_a) + (rate * rat_a)))
 *   rews[b] = ret[b] - cost[b % N]              effort == 0 and rate == 0: the cost pass is skipped, rews[b] = ret[b]
 * The order — per actuator over h, then over the actuators — is part of the contract.  Everything downstream is unchanged and sees
 * these rews: the ensemble's combination of its members' (shaped) returns, standardisation, the demo blend (the log-densities
 * are untouched), softmax, the weighted mean, the score update, the path-integral updates, rew_mean out.  mbd_plan_eval, the final
 * reward of mbd_plan_run, an episode's rewards log and mbd_env_rollout keep the env's own rewards.
 * Bit for bit: no record, or a cleared one, leaves every call as it is — same launches, same bits; a record of NULL weights and zero
 * costs gives the same bits; so does row_weight all ones with zero costs (the rollout kernels accumulate rew_sum = 0; rew_sum =
 * rew_sum + rew in step order and divide by float(H): the sum above with w = 1 and wsum = float(H)); a one-hot w gives ret[b] ==
 * rewss[b][h0] in value; a candidate whose rewss holds a non-finite value has a non-finite ret (nothing is skipped: 0 * NaN stays
 * NaN) and no other candidate's bits move.
 * The previous action.  mbd_plan_run, mbd_sweep_run and the phase calls use clip(prev0, -1, 1), or none when prev0 is NULL.  In an
 * episode or a session, every tick after the first uses clip(M_{t-1}[E-1], -1, 1), the last row committed before the new plan's
 * row 0 — the same row with a delay record and without, because C = C[1:] ++ M_t[0:E]; with a plant record it is the commanded row,
 * not the disturbed one.  The first tick uses the clipped last row of the delay record's queue C (rows0, or zeros), and without a
 * delay record clip(prev0), or none.  prev lives on the device: one small launch per tick, in front of the boundary kernel, forms
 * the next tick's — no host write, no synchronisation inside a tick loop — and mbd_*_mpc_reset_mean leaves it alone, as it leaves
 * the delay queue alone.
 * Every call that samples takes the record: MBD and path-integral plans, rigid-body envs and car2d, sharded plans (every rank sets
 * the same record), plans with a plant, delay, demo, sigma, ensemble, noise-shape or noise-basis record, sweeps (one record for
 * all plans) and both kinds of session (read at open).  Under a record a step gains exactly one launch, between the rollout and
 * the score (under an ensemble: in front of the launch that combines the members).
 * The set call copies its tables, is synchronous (it waits for the device) and is to be called between diffusion steps; rec ==
 * NULL clears.  Refused with MBD_ERR_INVALID before any device access, the message naming the field: a NULL handle, non-zero
 * reserved, rows != Hsample, cols != action_size, a negative or non-finite row_weight / act_weight / effort / rate, a non-finite
 * prev0, a sum of row_weight that is not finite and positive.  MBD_ERR_STATE while a session is open on the handle. */
int mbd_plan_set_objective(mbd_plan* plan, const mbd_objective* rec);
/* the last step's ret and cost (HOST; either may be NULL; synchronises the device): ret_out [shard_count], under an ensemble
 * record [n_members * Nsample]; cost_out [shard_count], all +0 when the cost pass is skipped.  MBD_ERR_STATE without a record, or
 * before a step has run with one. */
int mbd_plan_peek_objective(mbd_plan* plan, float* ret_out, float* cost_out);

/* ---- weighting: how a step turns the candidates' rewards into weights (no counterpart in the reference, whose softmax runs at
 * the configured temp_sample over all Nsample rewards, mbd_planner.py:110-127; DESIGN.md section 1 "N14 weighting") ---- */
/* A weighting record is a setting of a plan (of a sweep) beside the objective, ensemble and noise records.  It does two things to
 * the score of every diffusion step: candidates whose reward is not finite are left out — a diverged candidate no longer turns the
 * whole plan's mean into NaN —, and the temperature of the softmax can be chosen per step so that the effective sample size
 * ESS = (sum w)^2 / sum w^2 of the weights meets a target fraction of the candidates kept. */
typedef struct mbd_weighting {
  int32_t reject_nonfinite; /* 0 / 1: candidates whose reward is NaN or +-inf get weight +0 and leave the statistics */
  float   ess_frac;         /* 0: keep the plan's temperature; in (0, 1]: choose it so that ESS ~= ess_frac * kept  */
  float   temp_min, temp_max; /* the bracket when ess_frac > 0: finite, 0 < temp_min <= temp_max                    */
  int32_t iters;            /* bisection steps, 1..32 (ess_frac > 0)                                                */
  int32_t reserved[6];      /* must be 0 */
} mbd_weighting;
/* With a record in force the score of a step is — f32 throughout, every operation rounded; r [N] is the rewards buffer as the score
 * receives it (behind the objective and ensemble records, whose NaN it then drops), T0 the plan's temp_sample (plan k's temperature
 * in a sweep); sumB and maxB are the score's block reductions (thread t of 1024 takes i = t, t + 1024, ... ascending, a xor-
 * butterfly over the 64 lanes, the 16 wavefront values combined in order); a dropped entry takes part as +0 in a sum and -inf in a
 * max, positions never move:
 *   keep[n] = !reject_nonfinite || isfinite(r[n]);   kept = count (integer)
 *   mean = sumB(r) / float(kept);   sd = sqrt(sumB((r - mean)^2) / float(kept));   sd < 1e-4 -> 1   (every update method)
 *          (the squared deviations accumulate as the score without a record accumulates them: acc = fma(d, d, acc))
 *   z[n] = (r[n] - mean) / sd;   zmax = (maxB(r) - mean) / sd
 *   E(T): e[n] = exp_((z[n] / T) - (zmax / T));  S1 = sumB(e);  S2 = sumB(e * e);  ess = (S1 * S1) / S2
 *   ess_frac == 0:  T* = T0
 *   else: target = ess_frac * float(kept)
 *         if !(ess(temp_min) < target) T* = temp_min
 *         else if !(ess(temp_max) > target) T* = temp_max
 *         else lo, hi = temp_min, temp_max; iters times: mid = sqrt(lo * hi); ess(mid) < target ? lo = mid : hi = mid;   T* = hi
 *   w[n] = e[n] / S1 at T*, dropped: +0;   rew_mean out = mean;   log: T*, ess(T*), kept
 *   kept == 0: every weight +0 (the new mean is then all zeros, or what the literal score form makes of them), rew_mean NaN,
 *              log T0, 0, 0
 * Two consequences.  With ess_frac == 0, no reward dropped and sd >= 1e-4 the step has the bits of the step without a record: the
 * three operations ((r - mean) / sd) / T and the maximum through the largest reward are the existing ones.  ESS lies in [1, kept],
 * because the maximal entry has e = exp_(0) = 1, and nothing overflows — as long as z / T itself is finite: z is a standardised reward,
 * at most sqrt(kept) in size, so any temp_min above 1e-30 is safe; the set call does not refuse a smaller one, under which zmax / T
 * overflows, the maximal entry becomes inf - inf and the step's weights NaN.  Everything downstream is untouched and consumes these weights: the
 * weighted mean, the score update, cma-es' spread and sigma, cem's selection — a dropped candidate's +0 sorts below every positive
 * weight.
 * Under a record a step gains at most one launch: the weigh kernel stands where the score kernel stands and the step takes the
 * kernels that consume given weights (the ones MBD_NO_FUSED_SCORE=1 selects; sweeps: the batch weighted mean in its weights-given
 * form).  No record, or a cleared one: every call keeps its launches and its bits.
 * Every mode takes the record — all four update methods, lazy and materialised candidates, plans with an ensemble, objective,
 * plant, delay, sigma, noise-shape or noise-basis record, sharded plans (every rank scores all N gathered rewards through
 * mbd_plan_score_update and sets the same record), sweeps (one record for all plans), episodes and both kinds of session (read at
 * open) — except a plan created with enable_demo: the demo blend re-standardises and applies the temperature twice, and what an
 * ESS target should mean there is out of scope: MBD_ERR_UNSUPPORTED.
 * The set call is synchronous (it waits for the device) and is to be called between diffusion steps; rec == NULL clears.  Refused
 * with MBD_ERR_INVALID before any device access, the message naming the field: a NULL handle, non-zero reserved,
 * reject_nonfinite outside {0, 1}, ess_frac outside [0, 1] or non-finite, and with ess_frac > 0 a bracket that is not finite with
 * 0 < temp_min <= temp_max, or iters outside 1..32.  MBD_ERR_STATE while a session is open on the handle. */
int mbd_plan_set_weighting(mbd_plan* plan, const mbd_weighting* rec);
/* The log of the record's score steps (HOST; any of the three may be NULL; synchronises the device): the temperature used, the
 * ESS at that temperature and the kept count of every score step of the last mbd_plan_run (Ndiffuse - 1 entries), the last
 * mbd_plan_reverse_once or mbd_plan_score_update (1), or the last tick of an episode or session (warm_steps of a warm tick,
 * Ndiffuse - 1 of a cold one), in the order the steps ran.  The log lives on the device and the weigh kernel writes it: nothing is
 * read by the host inside a loop.  *count_out: the entries there are; at most `capacity` are copied.  MBD_ERR_STATE without a
 * record. */
int mbd_plan_peek_weighting(mbd_plan* plan, float* temp_out, float* ess_out, int32_t* kept_out, int capacity, int* count_out);

/* ---- what a tick executes: its mean, the incumbent or the best candidate (predictive sampling's and guarded MPPI's rule; no
 * counterpart in the reference; DESIGN.md section 1 "N15 pick") ---- */
/* Every receding-horizon path hands on one thing, the tick's new mean M_t, which is never rolled out.  Two other plans are at hand
 * when a tick ends: the incumbent — the plan the last tick committed to, shifted E rows: the Ybar the tick started from — and the
 * best candidate of the tick's last step.  A pick record evaluates the three on the plan's env and hands on the best of those the
 * record enables.  A setting of a plan (of a sweep), read by mbd_plan_run_mpc, mbd_sweep_run_mpc and both kinds of session (at open).
 * The contract, f32 throughout.  With a record in force a tick adds, behind its last diffusion or refinement step and in front of
 * the objective record's next previous action and of every boundary kernel:
 *   inputs   r[N]: the rewards the last step's score read (with an objective record: the shaped returns); Y_i, sigma_i: that step's
 *            mean and sigma; M_t: the tick's result; B_t: the Ybar the tick started from; s: the state the tick planned from (under
 *            a delay record the predicted state).
 *   n*       the lowest index among the maxima of the FINITE r[n] (NaN and +-inf never qualify, +0 and -0 tie); -1: none is finite.
 *   slots    [3][H][Nu]: 0 = M_t; 1 = B_t, present except on a cold tick (tick 0; a session's tick after reset_mean); 2 = candidate
 *            n*, present when n* >= 0, formed exactly as mbd_plan_peek forms it — clip(eps[n*] * sigma_i + Y_i) from the step's
 *            normals with the product and the sum each rounded (a noise shape or basis is already in those normals), or row n* of
 *            the materialised candidates (car2d, path-integral plans).  An absent slot holds M_t: the launches never change shape.
 *   ret[3]   the plan's env's rollout of the three slots from s over H rows, ONE launch — on the planner's model, never the plant —
 *            and under an objective record its launch over those rows with the tick's previous action.  Candidates are independent
 *            in every launch form, so ret[2] == r[n*] bit for bit.
 *   choice   c = -1; for k = 0, 1, 2: slot k enabled, present and isfinite(ret[k]), and (c < 0 or ret[k] > ret[c]) -> c = k; c < 0
 *            at the end -> c = 0.  Ties keep the earlier slot; a non-finite return is never picked while a finite one is available.
 *   output   P_t = slot c stands wherever M_t stood: the rows executed (or queued under a delay record), the shift into the next
 *            tick's Ybar, means_out and a session's mean_out, the objective record's next previous action.
 *   log      per tick and plan, on the device: choice, ret[3] (all three, whatever is enabled or present) and n*.
 * A tick gains three launches (the gather of n* and the slots, the rollout, the choice), four with an objective record; in a sweep
 * the rollout is one launch over the 3 n_plans slots.  Stream order on the handle's stream is the whole synchronisation; the extra
 * rollout carries no progress word and no noise job, and a session's boundary kernel stays its tick's last kernel.
 * Without a record nothing is launched and every bit is as it was.  candidates == MBD_PICK_MEAN: the episode is the episode without a
 * record bit for bit, and the log carries the value of every executed plan.
 * Composes with plant, delay, sigma, objective, weighting, noise-shape and noise-basis records, sweeps and sessions (under a
 * weighting record a dropped candidate is not finite and is never n*).  rec == NULL clears.  Refused before any device access, the
 * message naming the field: a NULL handle, candidates == 0 or with unknown bits, non-zero reserved -> MBD_ERR_INVALID; a plan created
 * with enable_demo (its score is not the return) or carrying an ensemble record (its reward is a reduction over members) ->
 * MBD_ERR_UNSUPPORTED, and so is mbd_plan_set_ensemble on a plan that carries a pick record; a session open on the handle ->
 * MBD_ERR_STATE. */
enum { MBD_PICK_MEAN = 1, MBD_PICK_PREV = 2, MBD_PICK_BEST = 4 };
typedef struct mbd_mpc_pick {
  int32_t candidates;  /* non-empty union of the bits above */
  int32_t reserved[7]; /* 0 */
} mbd_mpc_pick;
int mbd_plan_set_mpc_pick(mbd_plan* plan, const mbd_mpc_pick* rec);
/* The log of the last episode's or the session's ticks (HOST; any of the three may be NULL; synchronises the device): choice_out
 * [capacity], rets_out [capacity][3], best_out [capacity].  *count_out: the ticks served so far; min(count, capacity) entries are
 * copied — the most recent ones, oldest first, so a capacity of at least count gives the ticks from 0 on (the device keeps the last
 * 65536 ticks of a longer session).  MBD_ERR_STATE without a record. */
int mbd_plan_peek_mpc_pick(mbd_plan* plan, int32_t* choice_out, float* rets_out, int32_t* best_out, int capacity, int* count_out);

/* ---- terminal value: what the state a candidate's rollout ends in is worth (MPPI with a value function, TD-MPC, value-guided
 * predictive sampling; no counterpart in the reference, whose plans score their Hsample rows and nothing beyond; DESIGN.md
 * section 1 "N16 value") ---- */
/* A value record is a small fully connected net V over the env's state record, a setting of a plan (of a sweep) beside the
 * objective, weighting and pick records.  With a record in force every rollout launch that scores candidates also writes their
 * final states, and ONE launch behind it (behind the objective record's, where there is one) adds scale * V(s_H) to each row's
 * reward; the score, the weights and every update rule are unchanged and consume those rewards.  All pointers HOST, copied by the
 * set call. */
#define MBD_VALUE_MAX_LAYERS 4
#define MBD_VALUE_MAX_WIDTH 256
enum { MBD_VALUE_RELU = 0, MBD_VALUE_TANH = 1 };
enum { MBD_VALUE_REL_XY = 1 };
typedef struct mbd_value {
  const float* W[MBD_VALUE_MAX_LAYERS]; /* W[l-1] of layer l = 1..n_layers: [width[l-1]][width of layer l-1 (n_in for l = 1)],
                                           row-major — torch's nn.Linear.weight.  All entries finite                          */
  const float* b[MBD_VALUE_MAX_LAYERS]; /* [width[l-1]], finite                                                               */
  const float* center;   /* [n_in] or NULL = zeros; finite                                                                    */
  const float* in_scale; /* [n_in] or NULL = ones; finite; 0 masks an input                                                   */
  int32_t n_in;          /* must equal the env's state_size (n_links * 13; car2d 3)                                           */
  int32_t n_layers;      /* 1 .. MBD_VALUE_MAX_LAYERS; 1 is a linear value                                                    */
  int32_t width[MBD_VALUE_MAX_LAYERS]; /* entries [0, n_layers): 1 .. MBD_VALUE_MAX_WIDTH, the last one 1                     */
  int32_t act;           /* MBD_VALUE_RELU / MBD_VALUE_TANH: every hidden layer's; the last layer has none                    */
  int32_t flags;         /* MBD_VALUE_REL_XY (rigid-body envs only): link 0's x and y are subtracted from every link's        */
  float   scale;         /* finite: the weight of V in a candidate's reward (V is neither discounted nor divided by Hsample:
                            that is this number)                                                                              */
  int32_t reserved[5];   /* must be 0 */
} mbd_value;
/* The contract.  f32 throughout, every operation rounded; fma is the fused multiply-add, exp_ the library's exponential (the
 * primitive the weighting record's score uses).  Row b of a launch, s [n_in] its rollout's final state, W_l = W[l-1], b_l = b[l-1],
 * width_0 = n_in:
 *   REL_XY:  x0 = s[0], y0 = s[1];  for every link l:  s[13 l] = s[13 l] - x0,  s[13 l + 1] = s[13 l + 1] - y0
 *   x_0[j]  = (s[j] - center[j]) * in_scale[j]
 *   layer l = 1 .. n_layers, output o:  a = b_l[o];  for k = 0 .. width_{l-1} - 1 ascending:  a = fma(W_l[o][k], x_{l-1}[k], a)
 *   hidden: x_l[o] = act(a);   last: V = a
 *   relu(a) = a if a > 0;  +0 if a <= 0;  a if a is NaN
 *   tanh(a):  m = |a| if |a| < 44 else 44;  t = exp_((-2) * m);  y = (1 - t) / (1 + t);  a if a is NaN, else copysign(y, a)
 *   rews[b] = rews[b] + (scale * V)                                       (a product, then a sum; no fma)
 * rews[b] on the right is what the step would score without the record: the rollout's mean over Hsample, or what an objective
 * record left there.  The order is fixed within one (row, output) chain only; rows never meet, so a candidate whose final state is
 * not finite gets whatever this arithmetic gives — usually NaN, which a weighting record then drops — and leaves every other row's
 * bits alone.
 * Where the record applies: mbd_plan_sample_rollout (the rows of the local shard), mbd_plan_reverse_once, mbd_plan_run, episodes
 * and sessions, MBD and path-integral plans, lazy and materialised candidates, demo plans (the blend reads the rewards the record
 * leaves), sweeps (one net for all plans), and the three slots of a pick record, whose returns then include scale * V.  Unchanged,
 * as under an objective record: the rewards an episode reports, rew_final, the executed rows' rollouts, a delay record's
 * prediction.  Without a record no buffer is allocated, no final state is written and nothing is launched: every bit is as it was.
 * The set call copies the net (the weights transposed, for the kernel's coalesced reads), is synchronous and is to be called
 * between diffusion steps; rec == NULL clears.  Refused before any device access, the message naming the field.
 * MBD_ERR_INVALID: a NULL handle; non-zero reserved; n_in != state_size; n_layers outside 1 .. MBD_VALUE_MAX_LAYERS; a width
 * outside 1 .. MBD_VALUE_MAX_WIDTH; a last width other than 1; an unknown act; unknown flags; a NULL W or b of a layer in use; a
 * non-finite weight, bias, center, in_scale or scale.  MBD_ERR_UNSUPPORTED: MBD_VALUE_REL_XY on car2d (it has no links).
 * MBD_ERR_STATE: a plan that carries an ensemble record (an ensemble launch returns rewards only) — and mbd_plan_set_ensemble on a
 * plan that carries a value record —; a session open on the handle. */
int mbd_plan_set_value(mbd_plan* plan, const mbd_value* rec);
/* the last step's V per row (HOST [shard_count]; synchronises the device).  MBD_ERR_STATE without a record, or before a step has
 * run with one. */
int mbd_plan_peek_value(mbd_plan* plan, float* v_out);
/* V of states the caller gives: states HOST [B][state_size], v_out HOST [B], B >= 1 — the step's kernel on rows of the caller's (a
 * check of an imported net).  Synchronous.  MBD_ERR_STATE without a record; MBD_ERR_INVALID: NULL arguments, B < 1. */
int mbd_plan_eval_value(mbd_plan* plan, const float* states, int B, float* v_out);

/* ---- adapt: the shape of the sampling noise learnt from the weighted spread of the candidates (the diagonal covariance of CEM,
 * iCEM and CoVO-MPC; no counterpart in the reference, whose sigma_i is one scalar; DESIGN.md section 1 "N17 adapt") ---- */
/* An adapt record is a setting of a plan beside the noise shape.  The plan keeps a device table a [Hsample][action_size], all ones
 * at the start, and rewrites it behind every diffusion step from the weighted spread of that step's candidates; the samplers draw
 * under G = a * g (one product per element), g being the caller's noise shape in force at that step, ones where none is.  The rule
 * moves the SHAPE and leaves the scale alone: the sigma schedule, or a path-integral plan's carried sigma, still says how much noise
 * a step has; the table says where it goes — it narrows the elements where selection narrowed the candidates more than on average
 * and widens the others, within [a_min, a_max]. */
typedef struct mbd_adapt {
  float   rate;         /* 0 < rate <= 1: how far a step moves a towards its target                                    */
  float   a_min, a_max; /* finite, 0 < a_min <= 1 <= a_max: the clamp of every entry                                   */
  int32_t carry;        /* 0: a is all ones at the start of every tick; 1: at a tick boundary a is shifted exec_steps
                           rows forward with the mean, the appended rows take 1                                        */
  int32_t reserved[4];  /* must be 0 */
} mbd_adapt;
/* The update behind step i — f32 throughout, every operation rounded, the two fma explicit.  w [N]: the weights phase 2 of the step
 * used (the score's, or the weigh kernel's under a weighting record); Ybar_i: the mean the step sampled around; sigma: what it
 * sampled with (the schedule's sigma_i; the carried device scalar of an mppi plan); G: the table it sampled under.  For every
 * element e = (h, a):
 *   Y[n]   the candidate's value exactly as the weighted mean forms it: lazy plans clip((z[n][e] * sigma) + Ybar_i[e], -1, 1) from the
 *          shaped normal z, materialised plans the stored value
 *   d[n] = Y[n] - Ybar_i[e]
 *   m1 = sum_n w[n] d[n],  m2 = sum_n w[n] (d[n] * d[n])   both in the weighted mean's order ("wsum64"): 64 groups, group k a
 *          sequential chain acc = fma(w[n], x, acc) over n = k, k + 64, ... from +0 (x = d[n], or the rounded product d[n] * d[n]);
 *          the 64 partials added in group order, starting from group 0's
 *   var  = m2 - (m1 * m1);  var < 0 -> +0   (a NaN stays)
 *   active[e] = G[e] > 0;   s[e] = sqrt(var) / (sigma * G[e])   for active e.  An element the caller's shape froze (G[e] == 0)
 *          keeps its a[e] and takes no part below
 *   S = sqrt((sum over active e, ascending, of s[e] * s[e], from +0) / float(n_active))
 *   n_active == 0, or S not finite, or not S > 0: the step changes nothing and its log entry says skipped (all weight on one
 *          candidate makes every var zero, for instance)
 *   otherwise, for active e:  t = a[e] * (s[e] / S);   a'[e] = a[e] + (rate * (t - a[e])),  below a_min -> a_min, above a_max ->
 *          a_max;   G'[e] = a'[e] * g[e]  (no shape in force: a'[e])
 *   log: S as computed (NaN with no active element), skipped 0 / 1
 * Consequences.  Before the first update, and with a_min == a_max == 1 throughout, a is all ones and G == g bit for bit (x * 1 is
 * x): the plan has the bits of the plan without a record.  A frozen element stays frozen: G'[e] = a[e] * 0.
 * When the table changes otherwise: a is all ones after the set call, at the start of mbd_plan_run, at the start of every cold tick
 * of an episode or a session, and after mbd_plan_mpc_reset_mean; at the start of every other tick it follows `carry` (one small
 * launch, which also forms G under the shape in force in that tick: a shape set MBD_NOISE_WARM_TICKS enters G from tick 1 on;
 * behind an episode's last tick and at mbd_plan_mpc_close G is formed under the shape in force outside warm ticks again).
 * Between phase calls (mbd_plan_sample_rollout / mbd_plan_score_update, mbd_plan_reverse_once) the table persists.
 * A step's normals now depend on the previous step's result, so a plan with a record makes them in front of its rollout — the
 * path plans with shares_device take — and prepares nothing ahead: mbd_plan_prefetch_noise is a no-op for it.  The update is two
 * launches behind the step's update kernel on the step's stream; the tick's launch stands in front of the tick's first step.
 * Without a record nothing is launched and nothing changes.
 * Scope: MBD and mppi plans (update_method 0 and 1), rigid-body envs and car2d, lazy and materialised candidates, with or without
 * noise-shape, noise-basis, objective, weighting, value, ensemble, plant, delay, sigma and pick records; mbd_plan_run, the unsharded
 * phase calls, mbd_plan_run_mpc and sessions.  Sweeps take elite and to-go records (mbd_sweep_set_elites, mbd_sweep_set_togo), not yet
 * this one: their samplers are handed one shape for all plans.
 * The set call is synchronous (it waits for the device), discards normals prepared ahead as mbd_plan_set_noise_shape does, and is to
 * be called between diffusion steps; rec == NULL clears.  Refused before any device access, the message naming the field —
 * MBD_ERR_INVALID: a NULL handle, rate outside (0, 1] or non-finite, a_min / a_max non-finite or not 0 < a_min <= 1 <= a_max, carry
 * outside {0, 1}, non-zero reserved; MBD_ERR_UNSUPPORTED: update_method 2 or 3 (cma-es and cem adapt their own sigma), a plan
 * created with enable_demo; MBD_ERR_STATE: a sharded plan, a session open on the handle. */
int mbd_plan_set_adapt(mbd_plan* plan, const mbd_adapt* rec);
/* The table and the log (HOST; any of the outputs may be NULL; synchronises the device): a_out [Hsample][action_size] the current
 * table; ratio_out / skipped_out: S and the skipped flag of the steps since the last mbd_plan_run, mbd_plan_run_mpc or
 * mbd_plan_mpc_open began (the phase calls append), in the order the steps ran — the most recent min(count, capacity, 65536) of
 * them, oldest first.  The log lives on the device and the update's second kernel writes it.  *count_out: the steps there were.
 * MBD_ERR_STATE without a record; MBD_ERR_INVALID: a NULL handle, capacity < 0. */
int mbd_plan_peek_adapt(mbd_plan* plan, float* a_out, float* ratio_out, int32_t* skipped_out, int capacity, int* count_out);

/* ---- elites: a step's best candidates are candidates of the next step, and the step's mean may be one itself (the elite carry-over
 * of iCEM and CEM-MPC; the noise-free nominal of MPPI implementations and of predictive sampling; no counterpart in the reference,
 * whose every step draws N fresh candidates; DESIGN.md section 1 "N18 elites") ---- */
/* An elite record is a setting of a plan beside the adapt record.  The plan keeps, on the device, the rows E [n_elites][HNu] of the
 * best candidates its last diffusion step found, their returns R and indices src [n_elites], and one integer `count`, 0 <= count <=
 * n_elites, the number present.  Every step first overwrites its first candidates with them (injection), and behind its update takes
 * over its own best (selection).  No rollout kernel and no update kernel changes: an injected candidate is rolled out, scored and
 * averaged like any other. */
typedef struct mbd_elites {
  int32_t n_elites;   /* 0..32: how many of a step's best candidates the next step takes over              */
  int32_t nominal;    /* 0 / 1: candidate 0 of every step is the step's mean itself, clip(Ybar_i)          */
  int32_t carry;      /* 0: a tick starts without elites; 1: at a tick boundary they are shifted with the mean */
  int32_t reserved[5];  /* must be 0 */
} mbd_elites;
/* The contract — f32 throughout, every operation rounded.  slots = nominal + count.
 * INJECTION, in phase 1 of step i, behind the launch that made the step's normals z [N][HNu] (lazy plans: the MBD update on a
 * rigid-body env) or candidates Y0s [N][HNu] (materialised plans: car2d, mppi), in front of the rollout.  For every element e:
 *   nominal set, candidate 0:        lazy z[0][e] = +0;                  materialised Y0s[0][e] = clip(Ybar_i[e], -1, 1)
 *   elite j < count, candidate nominal + j:
 *                                    materialised Y0s[nominal+j][e] = E[j][e]
 *                                    lazy z[nominal+j][e] = g[e] == 0 ? +0 : (E[j][e] - Ybar_i[e]) / sigma_i   (the subtraction and
 *                                    the division each rounded)
 *   candidates from `slots` on keep every bit they were drawn with.
 * g is the shape the step's sampler was handed — the caller's noise shape in force in that step, or an adapt record's G —; with no
 * shape in force there is no test on g.  A frozen element therefore stays frozen.  What is rolled out and averaged for a lazy elite
 * is what the consumers of z form, clip((z * sigma_i) + Ybar_i, -1, 1): NOT E[j] bit for bit — the division and the product do not
 * undo each other exactly, and a frozen element takes Ybar_i's value.  The contract is the z above.  The rows are written behind a
 * noise basis where one is in force: they need not lie in the basis' span.
 * SELECTION, in phase 2 of step i, behind the step's update kernel (and an adapt record's launches), over r [N], the rewards the
 * score read — behind an objective, a value and an ensemble record:
 *   only finite entries (exponent bits not all ones) take part
 *   order: descending value, equal values (+0 == -0) lower index first — a total order on distinct indices
 *   count' = min(n_elites, number of finite entries);  src'[j] = the j-th entry in that order;  R'[j] = r[src'[j]]
 *   E'[j] = candidate src'[j] as mbd_plan_peek forms it: lazy clip((z[e] * sigma_i) + Ybar_i[e], -1, 1) from the step's normals —
 *           the injected rows included — and its Ybar_i; materialised the row as it stands
 *   log entry of the step: count', kept = the number of j with src'[j] < slots (the slots the step injected), top = R'[0], or the
 *           quiet NaN 0x7fc00000 when count' == 0
 * The injected candidates take part like any other, so an elite that is still among the best stays.  There is no sum in it: the
 * result is decided by an order and by gathers, whatever the algorithm.
 * LIFE CYCLE.  count = 0: at the set call, at the start of mbd_plan_run, at a cold tick of an episode or a session, behind
 * mbd_plan_mpc_reset_mean, and at the start of every other tick with carry == 0.  With carry == 1 the start of every other tick
 * shifts every present elite exec_steps rows forward with zeros behind it — the mean's own shift —, count stays, and R is stale until
 * the next selection rewrites it.  (One small launch in front of the tick's first sampler; behind an episode's last tick the elites
 * stay as that tick's last step selected them.)  The phase calls (mbd_plan_sample_rollout / mbd_plan_score_update,
 * mbd_plan_reverse_once) use the state as it stands.
 * A step's candidates now depend on the previous step's result, so a plan with a record takes the adapt record's route through the
 * noise ring: every step makes its normals in front of its rollout, nothing is prepared ahead or reused, and
 * mbd_plan_prefetch_noise is a no-op for it.  A step gains two launches, a tick one more.  Without a record nothing is launched and
 * every call keeps its bits.
 * Scope: MBD and mppi plans (update_method 0 and 1), rigid-body envs and car2d, lazy and materialised candidates, with or without
 * plant, delay, sigma, objective, weighting, value, ensemble, pick, adapt, noise-shape and noise-basis records (a pick record's best
 * candidate may then be an elite); mbd_plan_run, the unsharded phase calls, mbd_plan_run_mpc and sessions.  Sweeps: mbd_sweep_set_elites.
 * The set call is synchronous (it waits for the device), discards normals prepared ahead, and is to be called between diffusion
 * steps; rec == NULL clears.  Refused before any device access, the message naming the field — MBD_ERR_INVALID: a NULL handle,
 * n_elites outside [0, 32], nominal or carry outside {0, 1}, n_elites + nominal == 0, n_elites + nominal >= Nsample, non-zero
 * reserved; MBD_ERR_UNSUPPORTED: update_method 2 or 3 (cem keeps elites of its own kind, cma-es' spread would be biased by repeated
 * rows), a plan created with enable_demo (its score is not the return); MBD_ERR_STATE: a sharded plan, a session open on the
 * handle. */
int mbd_plan_set_elites(mbd_plan* plan, const mbd_elites* rec);
/* The elites and the log (HOST; any of the outputs may be NULL; synchronises the device): elites_out [n_elites][HNu], returns_out
 * and src_out [n_elites] as they stand — only the first *count_out entries mean anything —; log_count / log_kept / log_top: the
 * entries of the steps since the last mbd_plan_run, mbd_plan_run_mpc or mbd_plan_mpc_open began (the phase calls append), in the order
 * the steps ran — the most recent min(steps, capacity, 65536) of them, oldest first.  The log lives on the device and the selection
 * kernel writes it.  *n_log_out: the steps there were.  MBD_ERR_STATE without a record; MBD_ERR_INVALID: a NULL handle,
 * capacity < 0. */
int mbd_plan_peek_elites(mbd_plan* plan, float* elites_out, float* returns_out, int32_t* src_out, int32_t* count_out,
                         int32_t* log_count, int32_t* log_kept, float* log_top, int capacity, int* n_log_out);

/* ---- to-go: a horizon row is weighed by the return still ahead of it (the to-go return of PI^2, Theodorou, Buchli and Schaal 2010;
 * MPPI is PI^2 with this switched off; no counterpart in the reference, whose one weight per candidate multiplies all its rows;
 * DESIGN.md section 1 "N19 to-go") ---- */
/* A to-go record is a setting of a plan beside the adapt and elite records.  The horizon's rows fall into G groups of `block` rows,
 * and the rows of group j are what the step's ordinary update would give if the candidates' rewards were R_j, their mean reward from
 * the group's first row onwards.  No rollout kernel, sampler or launch choice changes: the rollouts already store rewss [N][H]. */
typedef struct mbd_togo {
  int32_t block;     /* >= 1: rows per group                                                            */
  int32_t min_tail;  /* 1..Hsample: a group starts only where at least this many rows are still ahead   */
  int32_t reserved[2];  /* must be 0 */
} mbd_togo;
/* The contract — f32 throughout, every operation rounded, no contraction.  H = Hsample, N = Nsample.
 * GROUPS.  The starts are s_0 = 0 and s_j = j * block for every j >= 1 with s_j < H and H - s_j >= min_tail; G is their number.
 * Group j owns rows [s_j, s_{j+1}), the last group [s_{G-1}, H).  block >= H or min_tail == H gives G = 1.
 * RETURNS.  R_0[n] = rews[n], the very array the step's score reads.  For the other groups one descending pass per candidate:
 *   acc = +0;  for t = H-1 down to s_1:  acc = acc + rewss[n][t];  whenever t is a start s_j (j >= 1):  R_j[n] = acc / float(H - s_j)
 * with rewss the rewards of the step's rollout.  Nothing is skipped: a NaN in step t reaches exactly the groups with s_j <= t, and
 * group 0 through rews.
 * UPDATE.  For every group j and every element e = (h, a) with h in group j, Ybar_{i-1}[e] is element e of the step's ordinary
 * update computed from R_j in place of rews: the score's standardisation and softmax with temp_sample and the std guard of MBD (none
 * for mppi), the wsum64 chain of the weighted mean over candidate values formed as today — clip((z * sigma_i) + Ybar_i, -1, 1) for
 * lazy plans, the stored value for materialised ones —, and the literal or identity score update.
 * UNCHANGED.  Everything else the update stores keeps its meaning and its bits: the step's mean reward is rews' mean in the score's
 * order, the weights mbd_plan_peek returns are group 0's, and the rows of group 0 are the rows of the plan without a record for the
 * same inputs.  G = 1 is no record, bit for bit.  Elite selection and a pick record keep reading rews.
 * A step's candidates do not depend on the previous result beyond what the mean already does: the noise prefetch stays.  With a
 * record a step launches two kernels (the returns, then score and weighted mean per group) where it launches one; without a record
 * every call keeps its launches and its bits.
 * Scope: MBD and mppi plans (update_method 0 and 1), rigid-body envs and car2d, lazy and materialised candidates; mbd_plan_run, the
 * unsharded phase calls, mbd_plan_reverse_once, mbd_plan_run_mpc and sessions; beside plant, delay, sigma, noise-shape, noise-basis,
 * pick and elite records.  Sweeps: mbd_sweep_set_togo.
 * The set call is synchronous (it waits for the device) and is to be called between diffusion steps; rec == NULL clears.  Refused
 * before any device access, the message naming the field or the record — MBD_ERR_INVALID: a NULL handle, block < 1, min_tail outside
 * [1, Hsample], non-zero reserved; MBD_ERR_UNSUPPORTED: update_method 2 or 3, a plan created with enable_demo, Nsample > 12288 (the
 * weights must fit LDS), a plan holding an objective, value, weighting, adapt or ensemble record (their per-row meaning is not
 * defined here; their set calls refuse a plan holding a to-go record in turn); MBD_ERR_STATE: a sharded plan, a session open on the
 * handle. */
int mbd_plan_set_togo(mbd_plan* plan, const mbd_togo* rec);
/* The last step's values (HOST; any output may be NULL; synchronises the device): starts_out [G] the groups' first rows, R_out and
 * W_out [G][Nsample] the groups' returns and weights (row 0: rews and the plan's weights), *n_groups_out = G.  The caller's arrays
 * hold G <= Hsample rows.  Before the record's first step R and W are all-ones bits (NaN).  MBD_ERR_STATE without a record;
 * MBD_ERR_INVALID: a NULL handle. */
int mbd_plan_peek_togo(mbd_plan* plan, int32_t* starts_out, float* R_out, float* W_out, int32_t* n_groups_out);

/* ---- zones: keep-out regions and goals for the env's tracked links (the obstacle and goal costs a sampling MPC is usually given; no
 * counterpart in the reference, whose plans maximise the env's reward alone; DESIGN.md section 1 "N20 zones") ---- */
/* A zone record is a setting of a plan beside the objective and value records.  The planning rollouts already write the tracked
 * links' world positions when they are handed a buffer; under a record they are handed one, and ONE launch between the rollout and
 * the score subtracts a penalty from each candidate's reward.  No rollout kernel, sampler, update kernel or launch choice changes;
 * without a record every call keeps its launches and its bits. */
#define MBD_MAX_ZONES 16
enum { MBD_ZONE_KEEP_OUT = 0, MBD_ZONE_GOAL = 1 };
typedef struct { int32_t kind; uint32_t links; float center[3]; float scale[3]; float radius, margin, weight; int32_t reserved; } mbd_zone;
typedef struct { int32_t n_zones; int32_t reserved[3]; mbd_zone zone[MBD_MAX_ZONES]; } mbd_zones;
/* links: a bit mask over the env's track slots — bit k is slot k, which is link track_link[k].  scale multiplies the three coordinate
 * differences before the distance is taken: (1,1,1) a sphere, (1,1,0) a vertical cylinder or a point goal on the ground plane,
 * (1,0,0) a slab.
 * The contract — f32 throughout, every operation rounded, no contraction.  H = Hsample; x the positions [B][H][n_track][3] of the
 * launch's rollout.
 * PENALTY of row b.  For step t, slot k ascending, zone z ascending, where bit k of zone z's links is set:
 *   e_i = (x_i - c_i) * s_i;  q = (e_0 e_0 + e_1 e_1) + e_2 e_2;  d = sqrt(q)
 *   keep-out: u = ((r + m) - d) / m        goal: u = (d - r) / m
 *   v = u < 0 ? 0 : (u > 1 ? 1 : u)  (a NaN stays a NaN);  term = w * (v * v)
 * s_t starts at +0 and adds the terms with k outer and z inner; pen starts at +0 and adds s_t in ascending t, then one division by
 * float(H); rews[b] = rews[b] - pen.  Nothing is skipped; a slot/zone pair outside the mask contributes no operation at all.
 * CLEARANCE.  clr_t is the minimum of d - r over the step's keep-out terms, +inf where there are none; clr the minimum of clr_t over
 * t.  A NaN wins and is stored as the canonical quiet NaN 0x7fc00000, so the order of the minimum cannot show.
 * WHERE.  The launch runs behind the objective's and in front of the value's: elite selection, weighting, adapt and every update
 * rule read the rews it wrote; rewss is not touched.  All four update methods, lazy and materialised candidates; mbd_plan_run, the
 * phase calls, mbd_plan_reverse_once, mbd_plan_run_mpc and sessions.
 * The set call is synchronous and is to be called between diffusion steps; rec == NULL clears.  Refused before any device access,
 * the message naming the field or the record — MBD_ERR_INVALID: a NULL handle; n_zones outside [1, MBD_MAX_ZONES]; a kind other
 * than 0 or 1; links zero or with a bit at or above n_track; a non-finite center; a scale entry non-finite or negative, or all three
 * zero; radius non-finite or negative; margin non-finite or not positive; weight non-finite or negative; non-zero reserved.
 * MBD_ERR_UNSUPPORTED: car2d; an env whose model tracks no link (compile planar models planar=False with track_names); a plan created
 * with enable_demo; a plan holding an ensemble, to-go or pick record — their set calls refuse a plan holding a zone record in turn.
 * MBD_ERR_STATE: a sharded plan; a session open on the handle.  At the run call of an episode, MBD_ERR_INVALID: a plant env whose
 * tracked links differ from the plan's (the demo record's rule). */
int mbd_plan_set_zones(mbd_plan* plan, const mbd_zones* rec);
/* Replaces the table of a plan that already holds a record: how a caller moves a goal or an obstacle between ticks.  Host state only
 * (the table travels as kernel arguments), so it is allowed while a session is open.  The record's own refusals as above;
 * MBD_ERR_STATE: a plan without a record, a session's tick in flight (collect it first). */
int mbd_plan_update_zones(mbd_plan* plan, const mbd_zones* rec);
/* the last step's pen and clr per candidate (HOST [Nsample] each, either may be NULL; synchronises the device).  MBD_ERR_STATE
 * without a record, or before a step has run with one. */
int mbd_plan_peek_zones(mbd_plan* plan, float* pen_out, float* clear_out);
/* An episode of mbd_plan_run_mpc under a record also logs, for every executed control step, s_t of the contract (its penalty before
 * the division by H) and clr_t, taken from the positions the executed rows' rollout wrote: HOST pen_out, clear_out [T * exec_steps],
 * either may be NULL.  The logged rewards stay the env's.  MBD_ERR_STATE without a record, or before an episode has run with one
 * (a session logs nothing executed: the caller owns the system). */
int mbd_plan_peek_mpc_zones(mbd_plan* plan, float* pen_out, float* clear_out);

/* ---- planning ahead of the plant: an episode whose plans take D ticks to arrive (the real-time iteration scheme; no
 * counterpart in the reference; DESIGN.md section 1 "N9 delay") ---- */
/* The episode of mbd_plan_run_mpc plans from s_t and executes that plan's first rows from the same s_t: planning takes no time.
 * A delay record gives it time.  While the system executes rows it is already committed to, the controller predicts — with the
 * PLAN's env — where those rows will leave the system, plans from that predicted state, and commits the new rows for D ticks
 * later.  A setting of a plan (of a sweep) beside the plant, ensemble and noise records, read by mbd_plan_run_mpc
 * (mbd_sweep_run_mpc) only: mbd_plan_run, mbd_sweep_run and the phase calls ignore it. */
#define MBD_MAX_MPC_DELAY 8
typedef struct mbd_mpc_delay {
  const float* rows0;   /* HOST [n_rows][action_size]: the rows the system is already committed to when the episode
                           starts; NULL = zeros (n_rows must then be 0).  Copied by the set call. */
  int32_t delay_ticks;  /* D, 1 .. MBD_MAX_MPC_DELAY: a plan made in tick t is first executed in tick t + D */
  int32_t n_rows;       /* 0, or D * exec_steps of the run that reads the record */
  int32_t reserved[4];  /* must be 0 */
} mbd_mpc_delay;
/* With a delay record, the episode of mbd_plan_run_mpc (above) becomes — everything not shown is unchanged, including the key
 * chains, the plant record's draws and the noise `when` modes (E = exec_steps, Nu = action_size):
 *   C = rows0 as D blocks of E rows (zeros if NULL)            the committed queue, [D][E][Nu]
 *   per tick t:  rng, k_t = split(rng)
 *                shat_t = final state of ONE rollout of the PLAN's env from s_t over the D*E rows of C, in queue order
 *                         (one candidate, horizon D*E; undisturbed rows; with an ensemble record still the plan's own env)
 *                M_t    = the plan from shat_t (i = i_start .. 1 from Ybar, key chain from k_t; ensemble, shape, basis as above)
 *                rows   = C[0]                    (plant record with act_std > 0: C[0] + act_std * eps[0:E*Nu], as above)
 *                rewards[tE .. tE+E), s' = rollout_PLANT(s_t, rows);  kick as above;  s_{t+1} = s'
 *                C = C[1:] ++ M_t[0:E]            (copied: -0.0 stays -0.0)
 *                Ybar = shift_E(M_t);  i_start = K
 * actions_out then holds the rows the plant was fed, means_out holds M_t — whose row 0 belongs to control step (t + D) E —,
 * states_out holds s_0 .. s_T, and mbd_plan_peek_mpc_predicted returns shat_0 .. shat_{T-1}.  Bit for bit:
 *  - no record, or a cleared record, leaves the episode as it is without one: same launches, same bits;
 *  - an episode of T ticks is a prefix of one of T + 1;
 *  - tick 0's mean is mbd_plan_run(k_0) of a plan whose state0 is shat_0;
 *  - with D = 1 and no disturbance (no plant record, or a record with plant NULL and both stds 0) the prediction launch and
 *    the execution launch have the same inputs, so shat_t == s_{t+1}, and the delayed episode of T + 1 ticks from s_0 equals the
 *    undelayed episode of T ticks that starts from s_1 with the same key, shifted by one tick: means_d[t] == means_u[t],
 *    states_d[t+1] == states_u[t], actions_d[(t+1)E ..] == actions_u[tE ..] and likewise the rewards, and
 *    actions_d[0:E] == rows0[0:E].
 * Still no host synchronisation between ticks: the queue lives on the device, and the tick boundary's kernel advances it.
 * The record is copied and stays until cleared (rec == NULL) or the handle is destroyed.  Refused with MBD_ERR_INVALID at the
 * set call, before any device access, the message naming the field: a NULL handle; delay_ticks outside
 * [1, MBD_MAX_MPC_DELAY]; non-zero reserved; rows0 NULL with n_rows != 0; rows0 non-NULL with n_rows < 1; a non-finite row
 * value.  Refused with MBD_ERR_INVALID at the run call, before any launch: n_rows != 0 && n_rows != D * exec_steps. */
int mbd_plan_set_mpc_delay(mbd_plan* plan, const mbd_mpc_delay* rec);
/* the predicted states of the last episode run with a record: HOST [T][state_size] (synchronises the device).  MBD_ERR_STATE
 * without a record, or before an episode has run with one. */
int mbd_plan_peek_mpc_predicted(mbd_plan* plan, float* predicted_out);

/* ---- the demo clock: an episode that follows a demonstration on the episode's own clock (mbd_planner.py:116-125 is the open-
 * loop demo step; the reference has no episode; DESIGN.md section 1 "N10 demo clock") ---- */
/* A demo plan (enable_demo) compares its kXrefRows = 50 planned steps with the env's 50 demo rows.  In an episode the demo has to
 * move with the system: a demo record carries a clip of any length and the row the episode starts at, and tick t plans under the
 * window of the clip that lies ahead of the system at that tick.  A setting of a plan (of a sweep) beside the plant, delay and
 * noise records, read by mbd_plan_run_mpc (mbd_sweep_run_mpc) only: mbd_plan_run, mbd_sweep_run and the phase calls ignore it. */
typedef struct mbd_mpc_demo {
  const float* clip;    /* HOST [n_track][n_rows][3] (car2d: [n_rows][2]); copied by the set call */
  int32_t n_rows;       /* L >= 1 */
  int32_t start_row;    /* c0 >= 0: the clip row the episode's first executed control step is compared with */
  float   rew_xref;     /* the demo's reward level in the blend (mbd_planner.py:121), constant over the episode */
  int32_t reserved[4];  /* must be 0 */
} mbd_mpc_demo;
/* With a demo record, tick t of the episode of mbd_plan_run_mpc (above) plans under (K = n_track, car2d 1; E = exec_steps; D =
 * the delay record's delay_ticks, 0 without one)
 *   window_t[k][h] = clip[k][min(c0 + (t + D) E + h, L - 1)]        h = 0 .. 49
 * — rows past the clip's end hold its last row (humanoidtrack.py:38-39); with a delay record the tick plans from the state
 * predicted for tick t + D, so its window starts there.  Every diffusion step of tick t is the demo step of mbd_plan_run with
 * window_t in place of the env's xref and rec.rew_xref in place of the env's rew_xref; everything else of the episode — the key
 * chains, the warm start, the shift, the executed rows, the plant, the delay queue, the noise shape and basis — is unchanged.
 * All T windows are built by ONE launch in front of the tick loop; a tick launches nothing new.  The rollouts of the executed
 * rows also write the tracked links' positions (car2d: x, y) of the E executed steps — the plant's, with a plant record — and
 * ONE launch behind the tick loop compares control step n = t E + j of the episode with the clip:
 *   err[n][k] = | x_k(n) - clip[k][min(c0 + n, L - 1)] |          (unclipped, f32: sqrtf(dx dx + dy dy + dz dz) in this order)
 * Bit for bit: with clip = the env's own xref, c0 = 0 and rew_xref = the env's, tick 0's mean is mbd_plan_run(k_0) of the demo
 * plan; an episode of T ticks is a prefix of one of T + 1, logs included; a plan without enable_demo is untouched.
 * The record is copied and stays until cleared (rec == NULL) or the handle is destroyed.  Refused with MBD_ERR_INVALID before any
 * launch, the message naming the field: a NULL handle; a NULL clip; n_rows < 1; start_row < 0; a non-finite rew_xref; non-zero
 * reserved; an env without xref; a plan whose config has enable_demo == 0 ("the plan does not use demos"); a non-finite clip
 * value.  A demo plan WITHOUT a record stays refused by the run call (MBD_ERR_UNSUPPORTED, enable_demo), and so does a demo plan
 * with an ensemble record.  At the run call, MBD_ERR_INVALID: a plant env whose n_track or tracked links differ from the plan's
 * env's. */
int mbd_plan_set_mpc_demo(mbd_plan* plan, const mbd_mpc_demo* rec);
/* the last episode run with a record (synchronises the device): HOST err_out [T*E][K] and windows_out [T][K][50][C] (C = 3,
 * car2d 2); either may be NULL.  MBD_ERR_STATE without a record, or before an episode has run with one. */
int mbd_plan_peek_mpc_track(mbd_plan* plan, float* err_out, float* windows_out);

/* ---- sessions: an episode the CALLER drives, one tick per call, from the state of a system the library does not own (no
 * counterpart in the reference; DESIGN.md section 1 "N11 session") ---- */
/* mbd_plan_run_mpc runs a whole episode and owns the plant.  A session is the same episode opened once and advanced one tick per
 * call from a state the caller hands in — a robot's, another simulator's: the caller is the plant.
 *   open:    rng = key; Ybar = zeros; i_start = Ndiffuse-1; t = 0; with a delay record C = rows0 or zeros   [D][E][Nu]
 *   tick(x): rng, k_t = split(rng)
 *            from = x                                   without a delay record
 *                 = final state of ONE rollout of the plan's env from x over the D*E rows of C      with one (predicted_out)
 *            Ybar = reverse_once(i, ., Ybar) from `from` for i = i_start .. 1, key chain from k_t  -> M_t   (mean_out)
 *            rows_out = M_t[0:E]                        (copied: -0.0 stays -0.0; unclipped, like actions_out)
 *            head_out = C[0];  C = C[1:] ++ M_t[0:E]    with a delay record (without one head_out = rows_out)
 *            Ybar = shift_E(M_t); i_start = K; t += 1
 * Without a delay record the caller executes rows_out now; with one it executes head_out now and rows_out in tick t + D.
 * Nothing is executed on the device: no rollout of the executed rows, no reward or state log, and mbd_plan_peek_mpc_track /
 * mbd_plan_peek_mpc_predicted do not serve sessions.  The noise shape, noise basis, ensemble, delay and demo records are read at
 * open, exactly as mbd_plan_run_mpc reads them; with a demo record tick t's window — the one mbd_plan_run_mpc's table holds for
 * that tick — is built by one small launch per tick.  mc->n_ticks is the most ticks the session serves; a session allocates
 * nothing per tick, so any value up to INT32_MAX costs nothing.
 * Bit for bit, because the batch episode and the session run ONE tick function:
 *  - a session fed states[t] of mbd_plan_run_mpc(key, T, K, E) returns mean_t == means[t] and rows_t == actions[tE .. tE+E); with
 *    a delay record head_t == actions[tE .. tE+E), predicted_t == predicted[t] and rows_t == means[t][0:E];
 *  - a session that executes rows_t on an env of its own equals the episode under a plant record naming that env, stds 0;
 *  - a handle that never opens a session behaves exactly as before: same launches, same bits. */
enum { MBD_TICK_ROWS_NONFINITE = 1, MBD_TICK_STATE_NONFINITE = 2, MBD_TICK_COLD = 4 };
typedef struct mbd_mpc_tick_info {
  int32_t tick;         /* t of the tick that produced the rows */
  int32_t flags;        /* the bits above: ROWS_NONFINITE — some element of rows_out is not finite (decided on the device, by
                           bits): a controller must never forward such rows; STATE_NONFINITE — the state handed in held a
                           non-finite value (checked on the host; the tick still runs); COLD — the tick ran Ndiffuse-1 steps */
  float   rew_mean;     /* rews.mean() of the tick's last diffusion step (what mbd_plan_run logs per step) */
  float   seconds;      /* host wall time submit -> rows on the host */
  int32_t reserved[4];  /* written 0 */
} mbd_mpc_tick_info;
/* A path-integral plan with a sigma record (mbd_mpc_sigma, above) opens a session like any other: tick(x) is then the record's
 * tick — n_it refinements from sigma, M_t = mu, the boundary formula for the next sigma — and mbd_plan_mpc_reset_mean makes the
 * next tick cold, sigma = sigma_cold included.  Between two ticks mbd_plan_get_sigma returns the sigma the next tick starts from.
 * open: everything mbd_plan_run_mpc refuses, with the same codes and messages (NULL plan / config / key -> MBD_ERR_INVALID
 * before any device access; the config's ranges; enable_demo without a demo record, a path-integral update without a sigma record ->
 * MBD_ERR_UNSUPPORTED; a sharded plan -> MBD_ERR_STATE; the delay record's n_rows against exec_steps -> MBD_ERR_INVALID); a
 * plant record set -> MBD_ERR_STATE (in a session the caller is the plant); a session already open -> MBD_ERR_STATE. */
int mbd_plan_mpc_open(mbd_plan* plan, const mbd_mpc_config* mc, const uint32_t key[2]);
/* submit: state HOST [state_size]; enqueues tick t and returns.  NULL plan / state -> MBD_ERR_INVALID; no session open, a tick
 * already in flight, or n_ticks ticks served -> MBD_ERR_STATE. */
int mbd_plan_mpc_submit(mbd_plan* plan, const float* state);
/* collect: waits for the tick in flight (an event behind its last kernel, which has written the outputs into pinned host
 * memory: a tick ends with no copy launch).  HOST outputs, each may be NULL: rows_out [E][Nu], mean_out [H][Nu], head_out
 * [E][Nu], predicted_out [state_size] (without a delay record: the state handed in), info_out.  NULL plan -> MBD_ERR_INVALID;
 * no session open or nothing in flight -> MBD_ERR_STATE. */
int mbd_plan_mpc_collect(mbd_plan* plan, float* rows_out, float* mean_out, float* head_out, float* predicted_out,
                         mbd_mpc_tick_info* info_out);
/* == submit then collect */
int mbd_plan_mpc_tick(mbd_plan* plan, const float* state, float* rows_out, float* mean_out, float* head_out,
                      float* predicted_out, mbd_mpc_tick_info* info_out);
/* the next tick is a cold one — Ybar = zeros, Ndiffuse-1 steps, sampled as tick 0 is, flagged COLD — and equals tick 0 of a
 * fresh session whose key is this session's rng at that tick; the delay queue is left as it is.  NULL plan -> MBD_ERR_INVALID;
 * no session open, or a tick in flight (collect it first) -> MBD_ERR_STATE. */
int mbd_plan_mpc_reset_mean(mbd_plan* plan);
/* close: waits for a tick in flight and drops it.  NULL plan -> MBD_ERR_INVALID; no session open -> MBD_ERR_STATE.
 * mbd_plan_destroy closes an open session.  While a session is open, these calls on the same handle return MBD_ERR_STATE, the
 * message naming the session: mbd_plan_run, _run_mpc, _eval, _set_state0, _reverse_once, _sample_rollout, _score_update and
 * every mbd_plan_set_* record call (plant, ensemble, noise shape, noise basis, delay, demo, sigma, objective, weighting, pick, value). */
int mbd_plan_mpc_close(mbd_plan* plan);

/* what the last step worked on, copied to HOST buffers (inspection / parity tests; synchronises the device): the
 * candidates Y0s [Nsample][H][Nu] (plans that keep normals instead form them here, from the normals, sigma_i and the
 * Ybar_i of the last step — between phase 1 and phase 2 the caller's d_Ybar_i must still be unchanged), the shard's
 * rewss [shard_count][H], the softmax weights [Nsample].  Any pointer may be NULL. */
int mbd_plan_peek(mbd_plan* plan, float* Y0s_out, float* rewss_out, float* weights_out);
/* timing of the dominant (rollout) kernel measured with hipEvents on the launch stream:
 * average milliseconds per launch since the last reset; count = launches. reset != 0 clears. */
int mbd_plan_kernel_time(mbd_plan* plan, float* avg_ms_out, int* count_out, int reset);
int mbd_plan_enable_timing(mbd_plan* plan, int enable);

/* ------------------------------------------------------------------------------------------------ */
/* sweeps — replaces the loops of mbd/scripts/run_mbd.py (:17-39 eight seeds, :42-64 eight           */
/* temperatures): P independent MBD plans of ONE env with the same (Nsample, Hsample, Ndiffuse,      */
/* beta0, betaT, enable_demo) advanced in lockstep, ONE rollout launch over the P * Nsample          */
/* candidates and ONE score + weighted-mean launch per diffusion step.  Seeds (keys, start states)   */
/* and temperatures may differ per plan.  Every plan's result is bit-identical to mbd_plan_run on    */
/* that plan alone.                                                                                  */
/* ------------------------------------------------------------------------------------------------ */
typedef struct mbd_sweep mbd_sweep;
#define MBD_SWEEP_MAX_PLANS 32
/* cfg: as for mbd_plan_create (unsharded; Nsample * 4 bytes <= 48 KB: larger plans fill the chip on their own — run
 * them as plans).  update_method 0: MBD plans; 1 / 2 / 3: the path-integral baselines mppi / cma-es / cem
 * (run_mbd.py:22-26,46-50 over path_integral.py:111-127; Ndiffuse plays Nrefine, no demos): one sampling launch, one rollout
 * launch and the update rule's kernels over all plans per refinement step.  temps: [n_plans] temp_sample per plan, or
 * NULL: cfg->temp_sample. */
int mbd_sweep_create(mbd_env* env, const mbd_plan_config* cfg, int n_plans, const float* temps, mbd_sweep** out);
int mbd_sweep_destroy(mbd_sweep* sweep);
/* state_init of plan k (HOST, state_size floats) */
int mbd_sweep_set_state0(mbd_sweep* sweep, int k, const float* state0);
/* the P reverse loops + final evaluations (mbd_planner.py:138-148,179-180).  keys: [n_plans][2] = rng_exp of each
 * plan (:150).  HOST outputs, any may be NULL: mu_0ts_out [n_plans][Ndiffuse-1][H][Nu], rew_means_out
 * [n_plans][Ndiffuse-1], rew_final_out [n_plans]; loop_seconds_out: wall time of the lockstep loop.  Synchronous.
 * Every plan's outputs are bit-identical to mbd_plan_run on its own WHATEVER the other plans do: a plan whose rollouts diverge
 * (non-finite rewards, a NaN mean) leaves the others' bits alone, whichever lanes their candidates share in the one launch. */
int mbd_sweep_run(mbd_sweep* sweep, const uint32_t* keys, float* mu_0ts_out, float* rew_means_out,
                  float* rew_final_out, double* loop_seconds_out);
/* ---- batched receding horizon (no counterpart in the reference, which plans open loop; DESIGN.md section 1 "N5 batched") ---- */
/* P closed-loop episodes in lockstep: episode k is EXACTLY mbd_plan_run_mpc's episode (above) on a plan of the sweep's config
 * with state0 = the state mbd_sweep_set_state0(k) set, key = keys[k] and temp_sample = the sweep's temps[k] — bit for bit —
 * and all episodes share mc (T, K, E).  Diffusion step i of tick t is ONE rollout launch over the P * Nsample candidates and
 * ONE score + weighted-mean launch, as in mbd_sweep_run; a tick boundary is one small kernel (blockIdx.y = episode) and one
 * rollout launch of the executed rows, one candidate per episode, which writes every episode's next state where the next
 * tick's rollouts read it.  No host synchronisation between ticks; the host waits as mbd_sweep_run does (see above).
 * keys: [n_plans][2].  HOST outputs, each may be NULL: actions_out [n_plans][T*E][Nu], rewards_out [n_plans][T*E], states_out
 * [n_plans][T+1][state_size], means_out [n_plans][T][H][Nu]; loop_seconds_out: wall time of the tick loop.  Synchronous; one
 * device->host copy per output at the end.  The sweep's start states are unchanged afterwards, whatever the outcome: a following
 * mbd_sweep_run equals a fresh sweep's.
 * The "bit for bit" above holds whatever the other episodes do: an episode that diverges — from its start state, or on its
 * plant — carries non-finite states and rewards from there on and leaves the other episodes' bits alone, in the planning
 * launches and in the launch that executes every episode's rows side by side.
 * Demo sweeps need a demo record, path-integral sweeps a sigma record (mbd_sweep_set_mpc_sigma below): NULL sweep / config /
 * keys and out-of-range fields -> MBD_ERR_INVALID (the NULL checks before any device access), enable_demo without a demo record
 * or a path-integral update without a sigma record -> MBD_ERR_UNSUPPORTED. */
int mbd_sweep_run_mpc(mbd_sweep* sweep, const mbd_mpc_config* mc, const uint32_t* keys, float* actions_out,
                      float* rewards_out, float* states_out, float* means_out, double* loop_seconds_out);
/* The plant record of episode k (mbd_mpc_plant, above; rec == NULL clears).  With records: episode k of mbd_sweep_run_mpc is
 * EXACTLY mbd_plan_run_mpc on a plan of its own carrying record k, bit for bit; the episodes may carry different plants, keys
 * and stds, or none.  The diffusion steps are unchanged; a tick boundary draws every episode's disturbances in one small
 * launch (blockIdx.y = episode), executes the rows in one rollout launch per maximal run of consecutive episodes that share
 * a plant handle (one shared plant: ONE launch), and applies the kicks in one launch, in the ticks that have any.  A sweep
 * without records runs exactly the launches described above.  Refusals as mbd_plan_set_mpc_plant's, against the sweep's env;
 * NULL sweep or k outside [0, n_plans) -> MBD_ERR_INVALID before any device access. */
int mbd_sweep_set_mpc_plant(mbd_sweep* sweep, int k, const mbd_mpc_plant* rec);
/* one noise shape (mbd_noise_shape, above) for all plans of the sweep: plan k of mbd_sweep_run, episode k of mbd_sweep_run_mpc,
 * is then the single plan's with the same record, bit for bit.  Refusals as mbd_plan_set_noise_shape's. */
int mbd_sweep_set_noise_shape(mbd_sweep* sweep, const mbd_noise_shape* rec);
/* one noise basis (mbd_noise_basis, above) for all plans of the sweep, with the same guarantee.  Refusals as
 * mbd_plan_set_noise_basis's. */
int mbd_sweep_set_noise_basis(mbd_sweep* sweep, const mbd_noise_basis* rec);
/* one objective record (mbd_objective, above) for all plans of the sweep — prev0 is every plan's —: plan k of mbd_sweep_run, episode
 * k of mbd_sweep_run_mpc and of a sweep's session is then the single plan's with the same record, bit for bit, whatever the other
 * plans do.  One launch over the n_plans * Nsample rows per step (blockIdx.y = plan), one launch per tick for every episode's
 * previous action.  Refusals as mbd_plan_set_objective's. */
int mbd_sweep_set_objective(mbd_sweep* sweep, const mbd_objective* rec);
/* plan k's ret_out [Nsample] and cost_out [Nsample] of the last step; as mbd_plan_peek_objective; k outside [0, n_plans) ->
 * MBD_ERR_INVALID */
int mbd_sweep_peek_objective(mbd_sweep* sweep, int k, float* ret_out, float* cost_out);
/* one weighting record (mbd_weighting, above) for all plans of the sweep, T0 being each plan's own temperature: plan k of
 * mbd_sweep_run, episode k of mbd_sweep_run_mpc and of a sweep's session equal the single plan with that record and temps[k], bit
 * for bit.  Refusals as mbd_plan_set_weighting's. */
int mbd_sweep_set_weighting(mbd_sweep* sweep, const mbd_weighting* rec);
/* plan k's log of the last run or the last tick; as mbd_plan_peek_weighting; k outside [0, n_plans) -> MBD_ERR_INVALID */
int mbd_sweep_peek_weighting(mbd_sweep* sweep, int k, float* temp_out, float* ess_out, int32_t* kept_out, int capacity, int* count_out);
/* one elite record (mbd_elites, above) for all plans of the sweep; NULL clears.  The contract is mbd_elites' per plan: plan k of
 * mbd_sweep_run, episode k of mbd_sweep_run_mpc and of a sweep's session equal the single plan with that record and temps[k], bit for
 * bit — plan k's, with its own E, R, src, count and log; what the other plans do or are fed makes no difference.  A step gains two
 * launches over the n_plans plans (blockIdx.y = plan), a tick one more; the counts stay on the device.  In a session's tick after
 * mbd_sweep_mpc_reset_mean(k) the episodes that idle through the steps above warm_steps take no part in the record's launches, and
 * mbd_sweep_mpc_reset_mean(k) empties episode k's elites.  Beside the sweep's plant, delay, sigma, pick, noise-shape, noise-basis,
 * objective, value, weighting and to-go records.  Refused before any device access, the message naming the field: the field checks
 * are mbd_plan_set_elites' on the sweep's config (MBD_ERR_UNSUPPORTED: update_method 2 or 3, enable_demo; MBD_ERR_INVALID: the
 * rest, n_elites + nominal >= Nsample among them, and a NULL handle); then MBD_ERR_STATE while a session is open. */
int mbd_sweep_set_elites(mbd_sweep* sweep, const mbd_elites* rec);
/* plan k's elites, count and log, as mbd_plan_peek_elites: the log holds the steps since the last mbd_sweep_run, mbd_sweep_run_mpc
 * or mbd_sweep_mpc_open began.  MBD_ERR_INVALID: a NULL handle, k outside [0, n_plans), capacity < 0; MBD_ERR_STATE without a record. */
int mbd_sweep_peek_elites(mbd_sweep* sweep, int k, float* elites_out, float* returns_out, int32_t* src_out, int32_t* count_out,
                          int32_t* log_count, int32_t* log_kept, float* log_top, int capacity, int* n_log_out);
/* one to-go record (mbd_togo, above) for all plans of the sweep; NULL clears.  The contract is mbd_togo's per plan — plan k's, with
 * its own R_j and W_j under temps[k] — and the guarantee mbd_sweep_set_elites gives.  A step launches the record's two kernels over
 * the n_plans plans where it launches the batch score and weighted mean.  Beside the sweep's plant, delay, sigma, pick, noise-shape,
 * noise-basis and elite records.  Refused before any device access, the message naming the field or the record: the field checks are
 * mbd_plan_set_togo's on the sweep's config; MBD_ERR_UNSUPPORTED beside the sweep's objective, value or weighting record — whose set
 * calls in turn refuse a sweep that carries a to-go record —; then MBD_ERR_STATE while a session is open. */
int mbd_sweep_set_togo(mbd_sweep* sweep, const mbd_togo* rec);
/* plan k's values of the last step, as mbd_plan_peek_togo.  MBD_ERR_INVALID: a NULL handle, k outside [0, n_plans); MBD_ERR_STATE
 * without a record. */
int mbd_sweep_peek_togo(mbd_sweep* sweep, int k, int32_t* starts_out, float* R_out, float* W_out, int32_t* n_groups_out);
/* one pick record (mbd_mpc_pick, above) for all episodes of the sweep: episode k of mbd_sweep_run_mpc and of a sweep's session
 * equals the single plan's with that record, bit for bit, logs included.  The gather and the choice are one launch each over the
 * n_plans episodes (blockIdx.y = episode), the rollout one launch over the 3 n_plans slots from the episodes' own states.  Refusals
 * as mbd_plan_set_mpc_pick's (sweeps take no ensemble). */
int mbd_sweep_set_mpc_pick(mbd_sweep* sweep, const mbd_mpc_pick* rec);
/* one value record (mbd_value, above) for all plans of the sweep — one net: plan k of mbd_sweep_run, episode k of mbd_sweep_run_mpc
 * and of a sweep's session is then the single plan's with the same record, bit for bit, whatever the other plans do.  One launch over
 * the n_plans * Nsample rows per step.  Refusals as mbd_plan_set_value's (sweeps take no ensemble). */
int mbd_sweep_set_value(mbd_sweep* sweep, const mbd_value* rec);
/* one zone record (mbd_zones, above) for all plans of the sweep — one table: plan k of mbd_sweep_run, episode k of mbd_sweep_run_mpc
 * and of a sweep's session is then the single plan's with the same record, bit for bit.  One launch over the n_plans * Nsample rows
 * per step, behind the objective's.  Refusals as mbd_plan_set_zones' on the sweep's config (sweeps take no ensemble and are never
 * sharded); MBD_ERR_UNSUPPORTED beside the sweep's to-go or pick record, whose set calls refuse a sweep with a zone record in turn. */
int mbd_sweep_set_zones(mbd_sweep* sweep, const mbd_zones* rec);
/* as mbd_plan_update_zones: the table of a sweep that already holds a record, allowed while a session is open but not while a tick
 * is in flight */
int mbd_sweep_update_zones(mbd_sweep* sweep, const mbd_zones* rec);
/* plan k's pen and clr of the last step, as mbd_plan_peek_zones; k outside [0, n_plans) -> MBD_ERR_INVALID */
int mbd_sweep_peek_zones(mbd_sweep* sweep, int k, float* pen_out, float* clear_out);
/* episode k's log of the last mbd_sweep_run_mpc, as mbd_plan_peek_mpc_zones; k outside [0, n_plans) -> MBD_ERR_INVALID */
int mbd_sweep_peek_mpc_zones(mbd_sweep* sweep, int k, float* pen_out, float* clear_out);
/* episode k's log; as mbd_plan_peek_mpc_pick; k outside [0, n_plans) -> MBD_ERR_INVALID */
int mbd_sweep_peek_mpc_pick(mbd_sweep* sweep, int k, int32_t* choice_out, float* rets_out, int32_t* best_out, int capacity,
                            int* count_out);
/* one delay record (mbd_mpc_delay, above) for all episodes of the sweep: episode k of mbd_sweep_run_mpc is then
 * mbd_plan_run_mpc on a plan of its own with the same record, bit for bit, whatever the other episodes do.  The prediction is
 * ONE rollout launch over the n_plans episodes, one candidate each, and the n_plans * Nsample planning candidates start from
 * the states it wrote.  Refusals as mbd_plan_set_mpc_delay's. */
int mbd_sweep_set_mpc_delay(mbd_sweep* sweep, const mbd_mpc_delay* rec);
/* the predicted states of the last batch run with a record: HOST [n_plans][T][state_size]; as mbd_plan_peek_mpc_predicted */
int mbd_sweep_peek_mpc_predicted(mbd_sweep* sweep, float* predicted_out);
/* one demo record (mbd_mpc_demo, above) for all episodes of the sweep — one clip and one clock: a rollout launch reads ONE demo
 * table for all its candidates, so per-episode clips or start rows would mean other rollout kernels.  Episode k of
 * mbd_sweep_run_mpc is then mbd_plan_run_mpc on a plan of its own with the same record, bit for bit.  Refusals as
 * mbd_plan_set_mpc_demo's. */
int mbd_sweep_set_mpc_demo(mbd_sweep* sweep, const mbd_mpc_demo* rec);
/* episode k's err_out [T*E][K] and the batch's windows_out [T][K][50][3] of the last batch run with a record; as
 * mbd_plan_peek_mpc_track; k outside [0, n_plans) -> MBD_ERR_INVALID */
int mbd_sweep_peek_mpc_track(mbd_sweep* sweep, int k, float* err_out, float* windows_out);
/* one sigma record (mbd_mpc_sigma, above) for all episodes of a path-integral sweep: episode k of mbd_sweep_run_mpc is then
 * mbd_plan_run_mpc on a path-integral plan of its own with the same record, keys[k] and temps[k], bit for bit.  A refinement of
 * a tick is mbd_sweep_run's lockstep step — one sampling launch, one rollout launch over the n_plans * Nsample candidates, the
 * update rule's kernels with blockIdx.y = episode — from the tick's slice of the state log (of the predicted states under a
 * delay record); the carried sigmas [n_plans] are logged and re-formed by ONE launch per tick boundary.  Plant records per
 * episode and the sweep's delay record compose through the boundary the MBD batches run.  Refusals as
 * mbd_plan_set_mpc_sigma's.  SESSIONS of path-integral sweeps stay refused by mbd_sweep_mpc_open (MBD_ERR_UNSUPPORTED,
 * update_method), record or not: a lockstep tick in which some episodes are cold and some are not would have to idle a carried
 * sigma. */
int mbd_sweep_set_mpc_sigma(mbd_sweep* sweep, const mbd_mpc_sigma* rec);
/* episode k's sigmas_out [T][2] of the last batch run with a record; as mbd_plan_peek_mpc_sigma; k outside [0, n_plans) ->
 * MBD_ERR_INVALID */
int mbd_sweep_peek_mpc_sigma(mbd_sweep* sweep, int k, float* sigmas_out);
/* ---- sessions of sweeps: P sessions in lockstep (mbd_plan_mpc_open, above; DESIGN.md section 1 "N11 session") ---- */
/* Episode k of a sweep's session is EXACTLY mbd_plan_mpc_open's session on a plan of the sweep's config with key = keys[k] and
 * temp_sample = the sweep's temps[k], fed states[k] — bit for bit, whatever the other episodes do or are fed (a non-finite state
 * included) — and all episodes share mc.  A diffusion step of a tick is ONE rollout launch over the n_plans * Nsample candidates,
 * the prediction of a delay record ONE launch over the episodes, and the tick ends with ONE boundary launch (blockIdx.y =
 * episode) that writes every episode's results into the mailbox.  The sweep's noise shape, noise basis, delay and demo records
 * are read at open; the sweep's start states are not used.
 * keys [n_plans][2]; states HOST [n_plans][state_size]; HOST outputs, each may be NULL: rows_out [n_plans][E][Nu], means_out
 * [n_plans][H][Nu], heads_out [n_plans][E][Nu], predicted_out [n_plans][state_size], infos_out [n_plans] (seconds: the tick's,
 * the same for every episode).
 * mbd_sweep_mpc_reset_mean(sweep, k): episode k's next tick is a cold one; the others' are not.  The lockstep loop then runs
 * Ndiffuse-1 steps, and an episode that is not cold idles through the steps above K — what they compute for it is discarded, its
 * key chain waits — and joins at step K from its shifted mean: its bits are a single session's.  One launch samples under one
 * noise shape and basis: such a mixed tick under a record in force in the warm ticks only -> MBD_ERR_UNSUPPORTED at submit.
 * Refusals as the plan calls', in their order: NULL sweep / config / keys / states -> MBD_ERR_INVALID before any device access;
 * open: mbd_sweep_run_mpc's refusals with its codes, an episode with a plant record -> MBD_ERR_STATE, a session already open ->
 * MBD_ERR_STATE; submit with no session, a tick in flight or n_ticks served, collect with nothing in flight, reset_mean / close
 * with no session -> MBD_ERR_STATE; reset_mean's k outside [0, n_plans) -> MBD_ERR_INVALID.  While a session is open
 * mbd_sweep_run, _run_mpc, _set_state0 and every mbd_sweep_set_* record call return MBD_ERR_STATE naming the session;
 * mbd_sweep_destroy closes an open session. */
int mbd_sweep_mpc_open(mbd_sweep* sweep, const mbd_mpc_config* mc, const uint32_t* keys);
int mbd_sweep_mpc_submit(mbd_sweep* sweep, const float* states);
int mbd_sweep_mpc_collect(mbd_sweep* sweep, float* rows_out, float* means_out, float* heads_out, float* predicted_out,
                          mbd_mpc_tick_info* infos_out);
int mbd_sweep_mpc_tick(mbd_sweep* sweep, const float* states, float* rows_out, float* means_out, float* heads_out,
                       float* predicted_out, mbd_mpc_tick_info* infos_out);
int mbd_sweep_mpc_reset_mean(mbd_sweep* sweep, int k);
int mbd_sweep_mpc_close(mbd_sweep* sweep);
/* path-integral sweeps: the carried sampling sigma of every plan after the last run (path_integral.py:113,131); HOST [n_plans] */
int mbd_sweep_get_sigmas(mbd_sweep* sweep, float* sigmas_out);
/* average milliseconds of the sweep's rollout launches since the last reset (hipEvents on the launch stream) */
int mbd_sweep_kernel_time(mbd_sweep* sweep, int enable, float* avg_ms_out, int* count_out);

/* ------------------------------------------------------------------------------------------------ */
/* in-library exchange — the ONE collective of a sharded diffusion step (the all-gather of the       */
/* per-candidate mean rewards between mbd_plan_sample_rollout and mbd_plan_score_update,             */
/* mbd_planner.py:109-111 with N sharded) WITHOUT a collective library: every rank owns a receive     */
/* window in device memory, peers write their slice into it directly (xGMI peer stores through       */
/* hipIpc mappings) and raise a flag per rank and epoch; a consumer kernel on the caller's stream    */
/* waits for the world's flags and hands over the gathered [rows][N] values.  Messages are <= 64 KB: */
/* the step pays two short kernels instead of a collective launch.  Results are the all-gather's.    */
/* ------------------------------------------------------------------------------------------------ */
typedef struct mbd_exchange mbd_exchange;
#define MBD_IPC_HANDLE_BYTES 64
#define MBD_EXCHANGE_MAX_RANKS 16
/* rank `rank` of `world` (<= MBD_EXCHANGE_MAX_RANKS) on `device`: rows x shard floats per rank and step.  The window is
 * FINE-GRAINED device memory (peers' stores and the owner's loads meet at system scope); a runtime without such a pool
 * gets MBD_ERR_UNSUPPORTED — keep the collective library's all-gather then (a coarse-grained window can hand the owner
 * a flag beside stale rewards). */
int mbd_exchange_create(int device, int rank, int world, int rows, int shard, mbd_exchange** out);
/* 1: the window is fine-grained memory (always, unless the test lever MBD_EXCHANGE_COARSE_OK allowed otherwise) */
int mbd_exchange_fine_grained(const mbd_exchange* x, int* out);
int mbd_exchange_destroy(mbd_exchange* x);
/* this rank's window as an IPC handle (MBD_IPC_HANDLE_BYTES bytes, HOST).  The caller passes the handles around by
 * any host channel (torch.distributed.all_gather_object, MPI, a file) and hands all of them to _connect. */
int mbd_exchange_local_handle(mbd_exchange* x, void* handle_out);
/* handles: [world][MBD_IPC_HANDLE_BYTES] HOST, rank-major (the own entry is not opened) */
int mbd_exchange_connect(mbd_exchange* x, const void* handles);
/* d_local [rows][shard] (device) -> every rank's window; *d_all_out: device pointer to [rows][world * shard], rank-major
 * = candidate order, valid until the next call.  Asynchronous on `stream`; every rank must call it once per step. */
int mbd_exchange_all_gather(mbd_exchange* x, const float* d_local, const float** d_all_out, void* stream);
/* MBD_OK, or MBD_ERR_STATE when a wait ran into its time limit (a peer that never arrived); synchronises the device */
int mbd_exchange_status(mbd_exchange* x);

#ifdef __cplusplus
}
#endif
#endif /* MBD_HIP_H */
