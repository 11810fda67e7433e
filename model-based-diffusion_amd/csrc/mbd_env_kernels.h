// mbd_env_kernels.h — the kernels mbd_env.hip launches beside the rollout instantiations: the car2d rollout, the demo
// log-densities and the gather of the 3-D rollouts' per-lane constants.  Non-template and `static`, so every unit that sees
// them emits them: only mbd_env.hip includes this header.
#pragma once

#include "mbd_kernels.h"

namespace mbd {

// ---- car2d (mbd/envs/car2d.py): one candidate per lane -------------------------------------------------
struct Car2dParams {
  const float* q0;  // [3]
  const float* us;  // [B][H][2]
  float* rewss;     // [B][H] or nullptr
  float* rews;      // [B] or nullptr
  float* qs;        // [B][H][3] or nullptr
  float* q_final;   // [B][3] or nullptr
  int B, H;
};

__device__ __forceinline__ void car_dyn(const float x[3], float u0, float u1, float dx[3]) {
  float sn, cs;
  sincos_(x[2], &sn, &cs);
  dx[0] = u1 * sn * 3.0f;
  dx[1] = u1 * cs * 3.0f;
  dx[2] = u0 * 3.14159274101257324f / 3.0f * 2.0f;
}
__device__ __forceinline__ float car_reward(const float q[3]) {
  float dx = q[0] - 0.5f, dy = q[1] - 0.0f;
  // (sqrt_floor is the correctly rounded square root from 1e-30 up — exhaustive, probe_short — and its floor of 1e-15
  // below that leaves the reward at exactly 1, like the true root)
  float d = sqrt_floor(dx * dx + dy * dy);
  d = fclip(d, 0.0f, 0.2f);
  float t = d / 0.2f;
  return 1.0f - t * t;
}

static __global__ __launch_bounds__(64) void car2d_rollout_kernel(Car2dParams P) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= P.B) return;
  // obstacle centres (car2d.py:48-63): python float64 products cast to f32
  const float cx[11] = {(float)(0.3 * -3), (float)(0.3 * -2), (float)(0.3 * -1), 0.0f, 0.0f, 0.0f, 0.0f,
                        (float)(0.3 * -3), (float)(0.3 * -2), (float)(0.3 * -1), 0.0f};
  const float cy[11] = {(float)(0.3 * 2), (float)(0.3 * 2), (float)(0.3 * 2), (float)(0.3 * 2),
                        (float)(0.3 * 1), 0.0f, (float)(0.3 * -1), (float)(0.3 * -2), (float)(0.3 * -2),
                        (float)(0.3 * -2), (float)(0.3 * -2)};
  const float dt = (float)0.1, dt2 = (float)(0.1 / 2), dt6 = (float)(0.1 / 6);
  float q[3] = {P.q0[0], P.q0[1], P.q0[2]};
  float sum = 0.0f;
  for (int t = 0; t < P.H; ++t) {
    const float* u = P.us + ((size_t)b * P.H + t) * 2;
    float a0 = fclip(u[0], -1.0f, 1.0f), a1 = fclip(u[1], -1.0f, 1.0f);
    float k1[3], k2[3], k3[3], k4[3], x[3], qn[3];
    car_dyn(q, a0, a1, k1);
    for (int i = 0; i < 3; ++i) x[i] = q[i] + dt2 * k1[i];
    car_dyn(x, a0, a1, k2);
    for (int i = 0; i < 3; ++i) x[i] = q[i] + dt2 * k2[i];
    car_dyn(x, a0, a1, k3);
    for (int i = 0; i < 3; ++i) x[i] = q[i] + dt * k3[i];
    car_dyn(x, a0, a1, k4);
    for (int i = 0; i < 3; ++i) qn[i] = q[i] + dt6 * (k1[i] + 2.0f * k2[i] + 2.0f * k3[i] + k4[i]);
    bool collide = false;
    for (int i = 0; i < 11; ++i) {
      float dx = qn[0] - cx[i], dy = qn[1] - cy[i];
      // sqrtf(x) < 0.3f  <=>  x < 0x1.70a3d8p-4 (0.09000000357627869): the correctly rounded square root is monotonic and
      // that is the smallest float32 whose root rounds to >= 0.3f (tests/test_spec_math.py checks the window around it)
      collide = collide || (dx * dx + dy * dy < 0.09000000357627869f);
    }
    for (int i = 0; i < 3; ++i) q[i] = collide ? q[i] : qn[i];
    float rew = car_reward(q);
    sum = sum + rew;
    if (P.rewss) P.rewss[(size_t)b * P.H + t] = rew;
    if (P.qs) { float* o = P.qs + ((size_t)b * P.H + t) * 3; o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; }
  }
  if (P.rews) P.rews[b] = sum / (float)P.H;
  if (P.q_final) { P.q_final[b * 3] = q[0]; P.q_final[b * 3 + 1] = q[1]; P.q_final[b * 3 + 2] = q[2]; }
}

// ---- A5: demo log-densities ------------------------------------------------------------------------------
// HumanoidTrack.eval_xref_logpd (humanoidtrack.py:98-106): xpos [B][H][K][3], xref [K][H][3].  One workgroup per
// candidate: its K*H terms ((clip(|x - xref|, 0, .5) / .5)^2, the candidate's 3 K H floats are contiguous) are formed in
// parallel and parked in LDS; thread k then adds link k's H terms in t order (S_k), thread 0 the K sums in link order —
// the contract's order since round 6 (rounds 1-5: one chain over all K H terms), chosen so that the rollout kernels can
// accumulate S_k on the tracked link's lane as the control steps go by (RolloutParams::lp) and produce the same bits
// without this launch; the standalone entry (mbd_env_xref_logpd) and the instantiations that do not accumulate use this kernel.
// The clamp is fclip_nan: a NaN distance (a diverged candidate's positions) stays a NaN, as the reference's jnp.clip leaves it,
// here, in logpd_car2d_kernel and in the rollouts' accumulation alike (v_med3_f32 would turn it into a term of 0).
constexpr int kLogpdThreads = 256, kLogpdMaxTerms = MBD_MAX_TRACK * 64;
static __global__ __launch_bounds__(kLogpdThreads) void logpd_track_kernel(const float* __restrict__ xpos,
                                                                    const float* __restrict__ xref, int B, int H, int K,
                                                                    float* __restrict__ lp) {
  __shared__ float term[kLogpdMaxTerms];
  const int b = blockIdx.x;
  const int n = K * H;
  for (int i = threadIdx.x; i < n; i += kLogpdThreads) {
    const int t = i / K, k = i - t * K;  // (xpos order: t outer, k inner)
    const float* a = xpos + ((size_t)b * n + i) * 3;
    const float* c = xref + ((size_t)k * H + t) * 3;
    float ex = a[0] - c[0], ey = a[1] - c[1], ez = a[2] - c[2];
    float d = fsqrt(ex * ex + ey * ey + ez * ez);
    d = fclip_nan(d, 0.0f, 0.5f);
    float s = d / 0.5f;
    term[k * H + t] = s * s;
  }
  __shared__ float part[MBD_MAX_TRACK];
  __syncthreads();
  if ((int)threadIdx.x < K) {
    float a = 0.0f;
    for (int t = 0; t < H; ++t) a = a + term[threadIdx.x * H + t];
    part[threadIdx.x] = a;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  float acc = part[0];
  for (int k = 1; k < K; ++k) acc = acc + part[k];
  lp[b] = 0.0f - acc / (float)n;
}
// Car2d.eval_xref_logpd (car2d.py:95-102): qs [B][H][3], xref [H][2]
static __global__ __launch_bounds__(64) void logpd_car2d_kernel(const float* __restrict__ qs,
                                                         const float* __restrict__ xref, int B, int H,
                                                         float* __restrict__ lp) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  float acc = 0.0f;
  for (int t = 0; t < H; ++t) {
    const float* a = qs + ((size_t)b * H + t) * 3;
    float ex = a[0] - xref[2 * t], ey = a[1] - xref[2 * t + 1];
    float d = fsqrt(ex * ex + ey * ey);
    d = fclip_nan(d, 0.0f, 0.5f);
    float s = d / 0.5f;
    acc = acc + s * s;
  }
  lp[b] = 0.0f - acc / (float)H;
}

// ---- the per-lane constants of the 3-D rollouts (mbd_kernels.h LaneRec3), gathered once per env and layout ----
// lps lanes; dpp: the lane <-> link table of a DPP layout is in force (else lane = link); axi: axisymmetric inertia
// instantiation (the tensors are remapped to (a, a, c, u)).  The code of the former kernel prologue, unchanged.
static __global__ void lane_setup3_kernel(const mbd_model_t* __restrict__ M, const signed char* __restrict__ lane_tab, int LPS,
                                   int dpp, int axi, LaneRec3* __restrict__ out, int helpers = 0) {
  const int l_lane = threadIdx.x;
  if (l_lane >= LPS) return;
  const bool DPP = dpp != 0;
  LaneRec3 R;
  const int L = M->n_links, Nu = M->n_act, K = M->n_track;
  const int l_link = DPP ? (int)lane_tab[l_lane] : l_lane;  // the link this lane holds
  const bool link_ok = l_link >= 0 && l_link < L;
  const int l = link_ok ? l_link : 0;
  auto lane_of = [&](int link) { return DPP ? (int)lane_tab[16 + link] : link; };  // (relative to the group's first lane)
  const int lane = l_lane;
  const int parent = M->parent[l];
  const int nr = M->n_rot[l];
  const bool is_joint = link_ok && nr >= 0;
  const int ns = M->n_slide[l];  // (kernels without slide joints ignore everything slide-related)
  const bool world_parent = parent < 0;
  R.l = l; R.link_ok = link_ok; R.root_lane = link_ok && l == 0; R.parent = parent; R.nr = nr; R.is_joint = is_joint;
  R.ns = ns; R.world_parent = world_parent; R.nr_eff = is_joint ? nr : -1;
  R.plane_rel = parent >= 0 ? lane_of(parent) : lane;
  Inert<false> ic, ip;
  ic.inv_mass = M->inv_mass[l];
  ip.inv_mass = world_parent ? 0.0f : M->inv_mass[parent >= 0 ? parent : 0];
  for (int k = 0; k < 6; ++k) {
    ic.ib[k] = M->inv_inertia[l][k];
    ip.ib[k] = world_parent ? 0.0f : M->inv_inertia[parent >= 0 ? parent : 0][k];
  }
  if (axi) { axi_remap<false>(ic); axi_remap<false>(ip); }
  R.ic_inv_mass = ic.inv_mass; R.ip_inv_mass = ip.inv_mass;
  for (int k = 0; k < 6; ++k) { R.ic_ib[k] = ic.ib[k]; R.ip_ib[k] = ip.ib[k]; }
  for (int k = 0; k < 3; ++k) { R.ap_pos[k] = M->ap_pos[l][k]; R.ac_pos[k] = M->ac_pos[l][k]; }
  for (int k = 0; k < 4; ++k) { R.ap_rot[k] = M->ap_rot[l][k]; R.ac_rot[k] = M->ac_rot[l][k]; }
  const q4 ap_rot = q4{M->ap_rot[l][0], M->ap_rot[l][1], M->ap_rot[l][2], M->ap_rot[l][3]};
  // non-joint lanes (free root, padding) are masked through their scalars: every contribution they
  // compute is then an exact zero
  R.ang_damp = is_joint ? M->ang_damp[l] : 0.0f; R.vel_damp = is_joint ? M->vel_damp[l] : 0.0f;
  const int zero_lane = M->n_rot[0] < 0 ? lane_of(0) : (L < LPS ? L : -1);  // a lane contributing zeros
  R.need_child_mask = !(M->n_rot[0] < 0) && !(L < LPS);
  R.lane_of1_rel = lane_of(1);
  v3 saxis[3];
  int act_rot[3], act_sl[3];
  float gear_rot[3], gear_sl[3], alo_rot[3], ahi_rot[3], alo_sl[3], ahi_sl[3];
  for (int k = 0; k < 3; ++k) {
    R.lim_lo[k] = M->rot_lo[l][k]; R.lim_hi[k] = M->rot_hi[l][k];
    R.stiff[k] = M->rot_stiff[l][k]; R.damp[k] = M->rot_damp[l][k];
    saxis[k] = mk3(M->slide_axis[l][k][0], M->slide_axis[l][k][1], M->slide_axis[l][k][2]);
    R.sl_lo[k] = M->slide_lo[l][k]; R.sl_hi[k] = M->slide_hi[l][k]; R.sl_damp[k] = M->slide_damp[l][k];
    act_rot[k] = -1; act_sl[k] = -1;
    gear_rot[k] = gear_sl[k] = 0.0f; alo_rot[k] = alo_sl[k] = 0.0f; ahi_rot[k] = ahi_sl[k] = 0.0f;
  }
  for (int a = 0; a < Nu; ++a) {
    if (M->act_link[a] != l || !link_ok) continue;
    const int s = M->act_slot[a];
    for (int k = 0; k < 3; ++k) {
      if (s == k) { act_rot[k] = a; gear_rot[k] = M->act_gear[a]; alo_rot[k] = M->act_lo[a]; ahi_rot[k] = M->act_hi[a]; }
      if (s == 3 + k) { act_sl[k] = a; gear_sl[k] = M->act_gear[a]; alo_sl[k] = M->act_lo[a]; ahi_sl[k] = M->act_hi[a]; }
    }
  }
  // Slide slots a joint does not have are masked in the CONSTANTS, once: a zero axis makes the slot's velocity,
  // force, projection and limit terms exact zeros (everything it multiplies is finite).  Hinge slots are NOT
  // masked that way: the Euler angles of a slot the joint lacks are meaningless and can overflow near the gimbal
  // singularity, so they are discarded by selects (0 * inf would be NaN).
  for (int k = 0; k < 3; ++k) {
    const bool has_sl = is_joint && k < ns;
    saxis[k] = sel3(has_sl, saxis[k], mk3(0.0f, 0.0f, 0.0f));
    gear_sl[k] = has_sl ? gear_sl[k] : 0.0f;
    const v3 sw = rot(saxis[k], ap_rot);  // SLIDEW: the slide axes in the world frame, once
    R.saxis[k][0] = saxis[k].x; R.saxis[k][1] = saxis[k].y; R.saxis[k][2] = saxis[k].z;
    R.saxis_w[k][0] = sw.x; R.saxis_w[k][1] = sw.y; R.saxis_w[k][2] = sw.z;
    R.act_rot[k] = act_rot[k]; R.act_sl[k] = act_sl[k];
    R.gear_rot[k] = gear_rot[k]; R.gear_sl[k] = gear_sl[k];
    R.alo_rot[k] = alo_rot[k]; R.ahi_rot[k] = ahi_rot[k]; R.alo_sl[k] = alo_sl[k]; R.ahi_sl[k] = ahi_sl[k];
  }
  int child_lane[4] = {-1, -1, -1, -1};
  {
    int nc = 0;
    for (int c = l + 1; c < L; ++c)
      if (M->parent[c] == l && link_ok) {
        if (nc < 4) child_lane[nc] = lane_of(c);
        ++nc;
      }
  }
  for (int c = 0; c < 4; ++c) {
    R.child_lane_rel[c] = child_lane[c];
    R.child_src_rel[c] = child_lane[c] >= 0 ? child_lane[c] : (zero_lane >= 0 ? zero_lane : lane);
  }
  // DPP layout: 0/1 masks — rm[s]: this link has an s-th child (it sits at lane - Ds); pm[s]: this link is the
  // s-th child of its parent (which sits at lane + Ds)
  int myslot = -1;
  if (DPP && link_ok && parent >= 0) {
    myslot = 0;
    for (int c = 0; c < l; ++c) myslot += M->parent[c] == parent ? 1 : 0;
  }
  for (int k = 0; k < 4; ++k) {
    R.rm[k] = (DPP && child_lane[k] >= 0) ? 1.0f : 0.0f;
    R.pm[k] = (DPP && myslot == k) ? 1.0f : 0.0f;
  }
  {
    int nc = 0;
    for (int j = 0; j < 5; ++j) { R.col_has[j] = 0; R.col_rad[j] = 0.0f; R.col_pos[j][0] = R.col_pos[j][1] = R.col_pos[j][2] = 0.0f; }
    for (int k = 0; k < M->n_col; ++k)
      if (M->col_link[k] == l && link_ok) {
        if (nc < 5) {
          R.col_has[nc] = 1; R.col_rad[nc] = M->col_radius[k];
          R.col_pos[nc][0] = M->col_pos[k][0]; R.col_pos[nc][1] = M->col_pos[k][1]; R.col_pos[nc][2] = M->col_pos[k][2];
        }
        ++nc;
      }
  }
  R.help_src_rel = lane; R.help_from_rel[0] = R.help_from_rel[1] = lane; R.is_owner = 0; R.is_helper = 0;
  if (helpers && DPP) {
    // the one link with more than two colliders, its first two idle lanes (the host checked that all of this exists)
    int owner = -1;
    for (int c = 0; c < L && owner < 0; ++c) {
      int n = 0;
      for (int k = 0; k < M->n_col; ++k) n += M->col_link[k] == c ? 1 : 0;
      if (n > 2) owner = c;
    }
    int idle[2] = {-1, -1}, ni = 0;
    for (int q = 0; q < LPS && ni < 2; ++q)
      if ((int)lane_tab[q] < 0) idle[ni++] = q;
    if (owner >= 0 && ni == 2) {
      const int owner_lane = lane_of(owner);
      const int which = lane == idle[0] ? 0 : (lane == idle[1] ? 1 : -1);
      if (link_ok && l == owner) {
        R.is_owner = 1; R.help_from_rel[0] = idle[0]; R.help_from_rel[1] = idle[1];
        for (int j = 2; j < 5; ++j) R.col_has[j] = 0;  // (stage (4) of the owner runs slots 0, 1; the rest come from the helpers)
      } else if (which >= 0) {
        R.is_helper = 1; R.help_src_rel = owner_lane;
        int nc = 0;
        for (int k = 0; k < M->n_col; ++k)
          if (M->col_link[k] == owner) {
            const int slot = nc - 2 - 2 * which;  // helper 0: colliders 2, 3; helper 1: collider 4 (and 5)
            if (slot >= 0 && slot < 2) {
              R.col_has[slot] = 1; R.col_rad[slot] = M->col_radius[k];
              R.col_pos[slot][0] = M->col_pos[k][0]; R.col_pos[slot][1] = M->col_pos[k][1]; R.col_pos[slot][2] = M->col_pos[k][2];
            }
            ++nc;
          }
        R.ic_inv_mass = M->inv_mass[owner];
        for (int k = 0; k < 6; ++k) R.ic_ib[k] = M->inv_inertia[owner][k];
      }
    }
  }
  int track_k = -1;
  for (int k = 0; k < K; ++k)
    if (M->track_link[k] == l && link_ok) track_k = k;
  R.track_k = track_k;
  for (int k = 0; k < 3; ++k) R.com[k] = M->com[l][k];
  R.js_pos = is_joint ? M->joint_scale_pos : 0.0f; R.js_ang = is_joint ? M->joint_scale_ang : 0.0f;
  R.invm_sum = ip.inv_mass + ic.inv_mass;
  // isotropic models: the shares of an angular correction, (-ib_p, ib_c)/(ib_p + ib_c) * joint_scale_ang
  // (zero on non-joint lanes through js_ang)
  {
    const float ibs = ip.ib[0] + ic.ib[0];
    R.kang2[0] = -((ip.ib[0] / ibs) * R.js_ang); R.kang2[1] = (ic.ib[0] / ibs) * R.js_ang;
  }
  out[l_lane] = R;
}

}  // namespace mbd
