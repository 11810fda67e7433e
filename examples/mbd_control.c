/* mbd_control.c — the planner in the loop of a system the library does not own, from plain C through include/mbd_hip.h: a
 * session (mbd_plan_mpc_open) is opened once and advanced one tick per call from the state the caller's system is in.
 *
 *   gcc -O2 -I include examples/mbd_control.c -o mbd_control -L model-based-diffusion_amd/lib -lmbd_hip -Wl,-rpath,$PWD/model-based-diffusion_amd/lib -lm
 *   ./mbd_control hopper 256 20 10 3 20 [delay_ticks] [--rate_cost L] [--mppi] [--pick] [--value] [--elites] [--togo] [--zones]
 *                 env    N   H  Nd K ticks
 *
 * The "system" here is a second env the example owns, stepped with mbd_env_step — the env's rollout kernel at B = 1, H = 1 through
 * HOST pointers (mbd_env_rollout takes device pointers, which a program without the HIP runtime cannot make): replace plant_step by
 * your robot's or your simulator's step and plant state by what you measure (mbd_env_pipeline_init turns generalized coordinates
 * (q, qd) into a state).
 * With delay_ticks D > 0 the rows to execute NOW are head (what the system was already committed to); the rows the tick planned are
 * due D ticks later, and the tick planned from the state it predicted for then.
 * --mppi (last argument): the same loop with MPPI (path_integral.py) in the planner's place — a path-integral plan and the sigma
 * record that lets a session accept it: sigma 1.0 in the cold tick, 0.25 in every later one.
 *
 * --rate_cost L (in front of --mppi): an objective record (mbd_objective) whose rate cost L * sum_h |u_h - u_{h-1}|^2 keeps the
 * replanned rows from chattering; the command the system is executing when the session opens goes in as prev0 — here zeros, the
 * actuators at rest; on a robot, its current command — and from then on the library carries the last committed row itself.
 *
 * Every plan carries a weighting record (mbd_weighting) with rejection on: this is the example of driving a real system, and one
 * diverged candidate must not poison the plan.
 *
 * --pick (with --mppi, in either order, behind everything else): a pick record (mbd_mpc_pick) with all three candidates — a tick then
 * hands on the best of its new mean, the plan it was already committed to and the best candidate of its last step, as the planner's
 * model values them, and its line gains "choice C value V": which one (0 mean, 1 incumbent, 2 best candidate) and the value of the
 * plan handed on, a health signal for a loop around a real system.  (MBD_PICK_MEAN alone would report the value and change no row.)
 * One more small rollout per tick; without the flag no record is set and nothing changes.
 *
 * --value (among the trailing flags): a value record (mbd_value) — here the smallest net there is, a linear value on the height of
 * link 0 at the end of every candidate's rollout, weighing like one further reward row; a real controller loads a fitted net
 * (python -m mbd_hip.scripts.fit_value) into the same struct.  Rigid-body envs only (the state record's float 2 is link 0's z).
 *
 * --elites (among the trailing flags): an elite record (mbd_elites) — the four best candidates of every diffusion step are candidates
 * of the next one, candidate 0 of every step is the step's mean itself, and a tick boundary shifts the elites with the mean; the
 * tick's line gains "kept K top R": how many of the last step's elites had been injected, and the best return it saw.
 *
 * --togo (among the trailing flags): a to-go record (mbd_togo) — the horizon's rows in groups of five, each group updated under
 * weights from the candidates' mean reward from the group's first row onwards, no group starting with fewer than five rows ahead;
 * not beside --rate_cost or --value (the library refuses the pair).  The tick's line gains "groups G".
 *
 * --zones (among the trailing flags): a zone record (mbd_zones) on the env's model retracked to its root link — a keep-out pillar one
 * metre ahead of the start and a goal on the ground plane that this program moves with the system before every tick
 * (mbd_plan_update_zones: host state only, allowed while the session is open); rigid-body envs that are not planar (humanoidrun, ant;
 * not beside --pick or --togo).  The tick's line gains "pen P clear C": the mean penalty of the last step's candidates and the
 * smallest keep-out clearance among them.
 *
 * Prints one line per tick: "tick T reward R ms M flags F", then "mean_reward R ms_per_tick M". */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mbd_hip.h"

#define CHECK(call)                                                                    \
  do {                                                                                 \
    int rc_ = (call);                                                                  \
    if (rc_ != MBD_OK) {                                                               \
      fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, mbd_last_error());           \
      return 1;                                                                        \
    }                                                                                  \
  } while (0)

/* the caller's system: one control step from `state` under `action`, in place */
static int plant_step(mbd_env* plant, float* state, const float* action, float* scratch, int S, float* reward) {
  int rc = mbd_env_step(plant, state, action, scratch, reward, NULL);
  if (rc == MBD_OK) memcpy(state, scratch, sizeof(float) * (size_t)S);
  return rc;
}

int main(int argc, char** argv) {
  int mppi = 0, pick = 0, value = 0, elites = 0, togo = 0, zones = 0;
  while (argc > 1 && (strcmp(argv[argc - 1], "--mppi") == 0 || strcmp(argv[argc - 1], "--pick") == 0 ||
                      strcmp(argv[argc - 1], "--value") == 0 || strcmp(argv[argc - 1], "--elites") == 0 ||
                      strcmp(argv[argc - 1], "--togo") == 0 || strcmp(argv[argc - 1], "--zones") == 0)) { /* trailing flags */
    if (strcmp(argv[argc - 1], "--mppi") == 0) mppi = 1;
    else if (strcmp(argv[argc - 1], "--pick") == 0) pick = 1;
    else if (strcmp(argv[argc - 1], "--elites") == 0) elites = 1;
    else if (strcmp(argv[argc - 1], "--togo") == 0) togo = 1;
    else if (strcmp(argv[argc - 1], "--zones") == 0) zones = 1;
    else value = 1;
    argc -= 1;
  }
  float rate_cost = 0.0f;
  if (argc > 2 && strcmp(argv[argc - 2], "--rate_cost") == 0) {
    rate_cost = (float)atof(argv[argc - 1]);
    argc -= 2;
  }
  const char* env_name = argc > 1 ? argv[1] : "hopper";
  const int N = argc > 2 ? atoi(argv[2]) : 256, H = argc > 3 ? atoi(argv[3]) : 20, Nd = argc > 4 ? atoi(argv[4]) : 10;
  const int K = argc > 5 ? atoi(argv[5]) : 3, T = argc > 6 ? atoi(argv[6]) : 20, D = argc > 7 ? atoi(argv[7]) : 0;
  const int impl = MBD_PRNG_PARTITIONABLE, E = 1;
  mbd_env *env = NULL, *plant = NULL;
  if (zones) { /* the planner's model, tracking its root link: the rollouts then return that link's world positions */
    static mbd_model_t model;
    CHECK(mbd_builtin_model(env_name, &model));
    model.n_track = 1;
    model.track_link[0] = 0;
    CHECK(mbd_env_create_model(env_name, 0, &model, NULL, 0.0f, &env));
  } else {
    CHECK(mbd_env_create(env_name, 0, &env)); /* the planner's model */
  }
  CHECK(mbd_env_create(env_name, 0, &plant)); /* the system: here a second env, owned by this program */
  int Nu = 0, Nx = 0, S = 0;
  CHECK(mbd_env_info(env, &Nu, &Nx, &S, NULL, NULL, NULL));
  mbd_plan_config cfg;
  memset(&cfg, 0, sizeof(cfg));
  cfg.Nsample = N; cfg.Hsample = H; cfg.Ndiffuse = Nd; cfg.temp_sample = 0.1f;
  cfg.beta0 = 1e-4f; cfg.betaT = 1e-2f; cfg.prng_impl = impl; cfg.shard_begin = 0; cfg.shard_count = N;
  cfg.literal_score = 1;
  mbd_plan* plan = NULL;
  if (mppi) cfg.update_method = 1; /* 1 mppi, 2 cma-es, 3 cem: Ndiffuse plays Nrefine */
  CHECK(mbd_plan_create(env, &cfg, &plan));
  if (mppi) { /* without the record a path-integral plan is refused by mbd_plan_mpc_open */
    mbd_mpc_sigma sigma;
    memset(&sigma, 0, sizeof(sigma));
    sigma.sigma_cold = 1.0f; sigma.sigma_warm = 0.25f; sigma.gain = 0.0f;
    CHECK(mbd_plan_set_mpc_sigma(plan, &sigma));
  }
  float* command = (float*)calloc((size_t)Nu, sizeof(float)); /* what the system is executing now: at rest */
  if (!command) { /* (a NULL prev0 would silently mean "no previous action") */
    fprintf(stderr, "out of memory\n");
    return 1;
  }
  if (rate_cost > 0.0f) { /* the controller's own rate cost; the first difference of the first plan is taken against `command` */
    mbd_objective obj;
    memset(&obj, 0, sizeof(obj));
    obj.rate = rate_cost;
    obj.prev0 = command;
    obj.rows = H; obj.cols = Nu;
    CHECK(mbd_plan_set_objective(plan, &obj));
  }
  { /* a real system can leave the model's well-behaved region: a candidate whose rollout diverges (a NaN or infinite reward) is
     * left out of every step's weights instead of turning the whole plan into NaN.  With nothing dropped the plan's bits are
     * unchanged.  (ess_frac > 0 with a bracket would also choose every step's temperature by the effective sample size.) */
    mbd_weighting wt;
    memset(&wt, 0, sizeof(wt));
    wt.reject_nonfinite = 1;
    CHECK(mbd_plan_set_weighting(plan, &wt));
  }
  if (pick) { /* hand on the best of the mean, the incumbent and the best candidate; log the choice and the three values */
    mbd_mpc_pick rec;
    memset(&rec, 0, sizeof(rec));
    rec.candidates = MBD_PICK_MEAN | MBD_PICK_PREV | MBD_PICK_BEST;
    CHECK(mbd_plan_set_mpc_pick(plan, &rec));
  }
  if (value) { /* V(s_H) = z of link 0: one layer of one output, weighing like one more of the H reward rows */
    float* w = (float*)calloc((size_t)S, sizeof(float));
    const float bias = 0.0f;
    if (!w) {
      fprintf(stderr, "out of memory\n");
      return 1;
    }
    w[2] = 1.0f;
    mbd_value val;
    memset(&val, 0, sizeof(val));
    val.W[0] = w; val.b[0] = &bias;
    val.n_in = S; val.n_layers = 1; val.width[0] = 1;
    val.act = MBD_VALUE_RELU; val.scale = 1.0f / (float)H;
    CHECK(mbd_plan_set_value(plan, &val)); /* (copied: the tables may go) */
    free(w);
  }
  if (elites) { /* keep what a step found: its four best candidates and its mean are candidates of the next step, across ticks too */
    mbd_elites el;
    memset(&el, 0, sizeof(el));
    el.n_elites = 4; el.nominal = 1; el.carry = 1;
    CHECK(mbd_plan_set_elites(plan, &el));
  }
  if (togo) { /* weigh a row by the return still ahead of it: groups of five rows, the last one at least five long */
    mbd_togo tg;
    memset(&tg, 0, sizeof(tg));
    tg.block = 5; tg.min_tail = H < 5 ? H : 5;
    CHECK(mbd_plan_set_togo(plan, &tg));
  }
  mbd_zones zn;
  memset(&zn, 0, sizeof(zn));
  float* zone_pen = zones ? (float*)malloc(sizeof(float) * (size_t)N) : NULL;
  float* zone_clr = zones ? (float*)malloc(sizeof(float) * (size_t)N) : NULL;
  if (zones) { /* a pillar to keep out of and a goal on the ground plane, both for track slot 0 (the root link) */
    zn.n_zones = 2;
    zn.zone[0].kind = MBD_ZONE_KEEP_OUT; zn.zone[0].links = 1u;
    zn.zone[0].center[0] = 1.0f; zn.zone[0].scale[0] = 1.0f; zn.zone[0].scale[1] = 1.0f; /* (1, 1, 0): a vertical cylinder */
    zn.zone[0].radius = 0.3f; zn.zone[0].margin = 0.3f; zn.zone[0].weight = 5.0f;
    zn.zone[1].kind = MBD_ZONE_GOAL; zn.zone[1].links = 1u;
    zn.zone[1].center[0] = 2.0f; zn.zone[1].scale[0] = 1.0f; zn.zone[1].scale[1] = 1.0f;
    zn.zone[1].radius = 0.2f; zn.zone[1].margin = 4.0f; zn.zone[1].weight = 1.0f;
    CHECK(mbd_plan_set_zones(plan, &zn));
  }
  if (D > 0) { /* plans arrive D ticks late; the system starts committed to zeros */
    mbd_mpc_delay delay;
    memset(&delay, 0, sizeof(delay));
    delay.delay_ticks = D;
    CHECK(mbd_plan_set_mpc_delay(plan, &delay));
  }
  uint32_t key[2], k4[4];
  CHECK(mbd_prng_key(0, key));
  CHECK(mbd_prng_split(key, 2, impl, k4));
  const uint32_t rng_reset[2] = {k4[2], k4[3]}, rng_episode[2] = {k4[0], k4[1]};
  float* state = (float*)malloc(sizeof(float) * (size_t)S);
  float* scratch = (float*)malloc(sizeof(float) * (size_t)S);
  float* rows = (float*)malloc(sizeof(float) * (size_t)E * (size_t)Nu);
  float* head = (float*)malloc(sizeof(float) * (size_t)E * (size_t)Nu);
  CHECK(mbd_env_reset(plant, rng_reset, impl, state));
  mbd_mpc_config mc;
  memset(&mc, 0, sizeof(mc));
  mc.n_ticks = T; mc.warm_steps = K; mc.exec_steps = E;
  CHECK(mbd_plan_mpc_open(plan, &mc, rng_episode));
  double reward_sum = 0.0, seconds = 0.0;
  for (int t = 0; t < T; ++t) {
    mbd_mpc_tick_info info;
    if (zones) { /* the goal stays two metres ahead of the system, half a metre to its left: moved between two ticks */
      zn.zone[1].center[0] = state[0] + 2.0f;
      zn.zone[1].center[1] = state[1] + 0.5f;
      CHECK(mbd_plan_update_zones(plan, &zn));
    }
    CHECK(mbd_plan_mpc_tick(plan, state, rows, NULL, head, NULL, &info));
    /* never forward non-finite rows.  The flag speaks of `rows`, the NEW plan: plan afresh from the next state.  What goes to the
     * actuators is `head` — without a delay record the same rows; with one, the queue's head, which rows flagged D ticks ago have
     * reached by now (reset_mean leaves the queue as it is) — so `head` itself is what is checked before it is executed. */
    if (info.flags & MBD_TICK_ROWS_NONFINITE) CHECK(mbd_plan_mpc_reset_mean(plan));
    for (int k = 0; k < E * Nu; ++k)
      if (!isfinite(head[k])) head[k] = 0.0f; /* hold */
    float reward = 0.0f;
    for (int j = 0; j < E; ++j) CHECK(plant_step(plant, state, head + (size_t)j * Nu, scratch, S, &reward));
    printf("tick %d reward %.9g ms %.3f flags %d", info.tick, reward, 1e3 * info.seconds, info.flags);
    if (pick) {
      int32_t choice = 0;
      float rets[3] = {0.0f, 0.0f, 0.0f};
      CHECK(mbd_plan_peek_mpc_pick(plan, &choice, rets, NULL, 1, NULL)); /* (the most recent tick's entry) */
      printf(" choice %d value %.9g", (int)choice, rets[choice]);
    }
    if (elites) {
      int32_t kept = 0;
      float top = 0.0f;
      CHECK(mbd_plan_peek_elites(plan, NULL, NULL, NULL, NULL, NULL, &kept, &top, 1, NULL)); /* (the most recent step's entry) */
      printf(" kept %d top %.9g", (int)kept, top);
    }
    if (togo) {
      int32_t groups = 0;
      CHECK(mbd_plan_peek_togo(plan, NULL, NULL, NULL, &groups));
      printf(" groups %d", (int)groups);
    }
    if (zones) {
      double pen = 0.0;
      float clr = INFINITY;
      CHECK(mbd_plan_peek_zones(plan, zone_pen, zone_clr));
      for (int n = 0; n < N; ++n) {
        pen += zone_pen[n];
        if (!(zone_clr[n] >= clr)) clr = zone_clr[n];
      }
      printf(" pen %.6g clear %.6g", pen / N, clr);
    }
    printf("\n");
    reward_sum += reward;
    seconds += info.seconds;
  }
  printf("mean_reward %.9g ms_per_tick %.3f\n", reward_sum / T, 1e3 * seconds / T);
  CHECK(mbd_plan_mpc_close(plan));
  free(zone_clr);
  free(zone_pen);
  free(head);
  free(command);
  free(rows);
  free(scratch);
  free(state);
  CHECK(mbd_plan_destroy(plan));
  CHECK(mbd_env_destroy(plant));
  CHECK(mbd_env_destroy(env));
  return 0;
}
