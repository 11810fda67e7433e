// mbd_planar.hip — translation unit of the planar rollouts (mbd_planar.h).  Its own file because it is built with its own
// scheduler strategy (-mllvm -amdgpu-sched-strategy=max-ilp, __graft_entry__.build): the planar substeps are short
// dependent chains around a few packed instructions, and the default strategy leaves 11-12 hazard s_nop per substep
// where max-ilp leaves 4-5 (hopper 342 -> 336 instructions per substep, halfcheetah 398 -> 391, walker2d 371 -> 363:
// a lone wavefront's time is its instruction count).  The 3-D kernels (mbd_env.hip) keep the default.
#define MBD_SHARED_ONLY 1
#include "mbd_planar.h"
#include "mbd_launch.h"

namespace mbd {

RolloutKernel planar_kernel(const EnvShape& s, int rk, int nfr, bool no_fl, bool early_out) {
  const int lps = s.lps, fam = s.dpp_family, max_col = s.max_col, fl = s.fl;
  if (early_out) {
    // the early-out instantiations (EO: P.cpw candidates per wavefront, mbd_planar.h): (lps, family, fl, rk, nfr) of the
    // built-in models with contacts — hopper, walker2d, halfcheetah
#if (MBD_TUNED_SPEC & 8) == 0  // (MBD_FLAG_CONTACT6_GAUSS_SEIDEL clear: stage (6) as a packed pair is Jacobi)
    if (no_fl || s.spec || max_col != 2) return nullptr;
    if (lps == 4 && fam == 2 && fl == 0 && rk == MBD_REW_HOPPER && nfr == 20) return rollout_planar_kernel<4, 2, 1, 0, 0, MBD_REW_HOPPER, 20, false, true>;
    if (lps == 8 && fam == 1 && fl == 0 && rk == MBD_REW_HOPPER && nfr == 20) return rollout_planar_kernel<8, 2, 1, -3, 0, MBD_REW_HOPPER, 20, false, true>;
    if (lps == 8 && fam == 1 && fl == 1 && rk == MBD_REW_HALFCHEETAH) return rollout_planar_kernel<8, 2, 1, -3, 1, MBD_REW_HALFCHEETAH, 0, false, true>;
#endif
    return nullptr;
  }
  if (max_col > 4) return nullptr;
  if (max_col > 2) {  // three or four spheres on a link (round 6: collide_all_capsules puts four on the halfcheetah's torso)
    if (s.spec) return rollout_planar_kernel<16, 4, 0, 0, -1, -1, 0, true>;
    if (lps == 8 && fam == 1) {
      if (fl == 1 && rk == MBD_REW_HALFCHEETAH && !no_fl && nfr == 16) return rollout_planar_kernel<8, 4, 1, -3, 1, MBD_REW_HALFCHEETAH, 16>;
      return rollout_planar_kernel<8, 4, 1, -3>;
    }
    if (lps == 4) return rollout_planar_kernel<4, 4, 0, 0>;
    if (lps == 8) return rollout_planar_kernel<8, 4, 0, 0>;
    return rollout_planar_kernel<16, 4, 0, 0>;
  }
  if (s.spec) return rollout_planar_kernel<16, 2, 0, 0, -1, -1, 0, true>;  // specification switches at run time
  // (... the reward kind: cartpole, hopper, walker2d, halfcheetah; and n_frames, for the values the built-in models have:
  // NFR; halfcheetah's 16 since round 6 — see below)
  if (lps == 4 && fam == 2) {
    if (max_col == 0) {
      if (fl == 2 && rk == MBD_REW_CARTPOLE && !no_fl && nfr == 4) return rollout_planar_kernel<4, 0, 1, 0, 2, MBD_REW_CARTPOLE, 4>;
      if (fl == 2 && rk == MBD_REW_CARTPOLE && !no_fl) return rollout_planar_kernel<4, 0, 1, 0, 2, MBD_REW_CARTPOLE>;
      return rollout_planar_kernel<4, 0, 1, 0>;
    }
    if (fl == 0 && rk == MBD_REW_HOPPER && !no_fl && nfr == 20) return rollout_planar_kernel<4, 2, 1, 0, 0, MBD_REW_HOPPER, 20>;
    if (fl == 0 && rk == MBD_REW_HOPPER && !no_fl) return rollout_planar_kernel<4, 2, 1, 0, 0, MBD_REW_HOPPER>;
    return rollout_planar_kernel<4, 2, 1, 0>;
  }
  if (lps == 8 && fam == 1) {
    if (fl == 0 && rk == MBD_REW_HOPPER && !no_fl && nfr == 20) return rollout_planar_kernel<8, 2, 1, -3, 0, MBD_REW_HOPPER, 20>;
    if (fl == 0 && rk == MBD_REW_HOPPER && !no_fl) return rollout_planar_kernel<8, 2, 1, -3, 0, MBD_REW_HOPPER>;
    // (round 6: n_frames = 16 as 2 x 8 substeps in line now pays, +0.7 % — without the renormalisation's two branches per
    // substep the body is shorter; rounds 2-5 measured -0.2 %)
    if (fl == 1 && rk == MBD_REW_HALFCHEETAH && !no_fl && nfr == 16) return rollout_planar_kernel<8, 2, 1, -3, 1, MBD_REW_HALFCHEETAH, 16>;
    if (fl == 1 && rk == MBD_REW_HALFCHEETAH && !no_fl) return rollout_planar_kernel<8, 2, 1, -3, 1, MBD_REW_HALFCHEETAH>;
    return rollout_planar_kernel<8, 2, 1, -3>;
  }
  if (lps == 8 && fam == 2) return rollout_planar_kernel<8, 2, 1, 0>;
  if (lps == 4) return rollout_planar_kernel<4, 2, 0, 0>;
  if (lps == 8) return rollout_planar_kernel<8, 2, 0, 0>;
  return rollout_planar_kernel<16, 2, 0, 0>;
}

}  // namespace mbd
