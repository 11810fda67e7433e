// mbd_hot3d.hip — translation unit of the 3-D rollout instantiations the built-in humanoids and ant run (the DPP families
// (+1, -4, -6) and (+1, -2, -4, -6) of mbd_kernels.h).  Its own file because it is built with its own scheduler strategy
// (-mllvm -amdgpu-sched-strategy=iterative-ilp, __graft_entry__.build): same-box A/B against the default strategy,
// profiles/r03_hot3d_sched_ab.txt — humanoidrun N=1024 0.5499 -> 0.5427 ms (+1.3 %), N=4096 +1.7 %, humanoidtrack +0.8 %.
// (The general instantiations stay in mbd_env.hip with the default: one of them crashes this compiler's register
// allocator under the iterative strategy.)
#define MBD_SHARED_ONLY 1
#include "mbd_kernels.h"
#include "mbd_launch.h"

namespace mbd {

RolloutKernel hot3d_kernel(const EnvShape& s, bool helpers, int rk, int nfr, bool unit) {
  constexpr int D0 = 1, D1 = -4, D2 = -6;
  if (s.humanoid_shape && s.dpp_family == 0 && s.max_col <= 1) {
    // (these two compile in the built-in humanoids' unit inverse inertia as well — mbd_kernels.h unit_inertia_form: -20 of
    // 823 instructions per substep; a model with another inertia runs the same instantiation with the inertia at run time)
    if (!unit) {
      if (rk == MBD_REW_HUMANOIDRUN && nfr == 7) return rollout_kernel_rtib<16, true, false, 3, 1, D0, D1, D2, 0, false, true, 3, false, false, MBD_REW_HUMANOIDRUN, 7>;
      if (rk == MBD_REW_HUMANOIDTRACK && nfr == 5) return rollout_kernel_rtib<16, true, false, 3, 1, D0, D1, D2, 0, false, true, 3, false, false, MBD_REW_HUMANOIDTRACK, 5>;
    }
    if (rk == MBD_REW_HUMANOIDRUN && nfr == 7) return rollout_kernel<16, true, false, 3, 1, D0, D1, D2, 0, false, true, 3, false, false, MBD_REW_HUMANOIDRUN, 7>;
    if (rk == MBD_REW_HUMANOIDTRACK && nfr == 5) return rollout_kernel<16, true, false, 3, 1, D0, D1, D2, 0, false, true, 3, false, false, MBD_REW_HUMANOIDTRACK, 5>;
    return rollout_kernel<16, true, false, 3, 1, D0, D1, D2, 0, false, true>;
  }
  if (s.humanoid_shape && s.dpp_family == 0 && s.max_col <= 5) {
    if (helpers) {  // humanoidstandup: the torso's colliders 2..4 run stage (4) on two of the candidate's idle lanes (HELP)
      if (rk == MBD_REW_HUMANOIDSTANDUP && nfr == 7) return rollout_kernel<16, true, false, 3, 5, D0, D1, D2, 0, false, true, 3, false, false, MBD_REW_HUMANOIDSTANDUP, 7, true, true>;
      return rollout_kernel<16, true, false, 3, 5, D0, D1, D2, 0, false, true, 3, false, false, -1, 0, true>;
    }
    if (rk == MBD_REW_HUMANOIDSTANDUP && nfr == 7) return rollout_kernel<16, true, false, 3, 5, D0, D1, D2, 0, false, true, 3, false, false, MBD_REW_HUMANOIDSTANDUP, 7>;
    return rollout_kernel<16, true, false, 3, 5, D0, D1, D2, 0, false, true>;
  }
  if (s.lps == 16 && s.iso && !s.slides && s.max_col <= 2 && s.dpp_family == 3 && s.max_rot <= 1) {
    // ant (the reference's default env_name): reward kind and n_frames compiled in, like the humanoids
    if (rk == MBD_REW_ANT && nfr == 10) return rollout_kernel<16, true, false, 4, 2, 1, -2, -4, -6, false, false, 3, false, false, MBD_REW_ANT, 10, false, true>;
    return rollout_kernel<16, true, false, 4, 2, 1, -2, -4, -6, false, false>;
  }
  return nullptr;
}

}  // namespace mbd
