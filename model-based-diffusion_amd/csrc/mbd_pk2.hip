// mbd_pk2.hip — translation unit of the two-candidates-per-lane rollouts (mbd_pk2.h).  Its own file because it is built
// with its own scheduler strategy (-mllvm -amdgpu-sched-strategy=iterative-ilp, __graft_entry__.build): a v_pk_*_f32
// result cannot be read by the very next instruction (the compiler inserts an s_nop), and these kernels are almost
// entirely dependent packed chains — the default strategy leaves 97 such wait states per substep, the iterative one 27.
// The one-candidate-per-lane kernels (mbd_env.hip) measured slower under that strategy and keep the default.
#define MBD_SHARED_ONLY 1
#include "mbd_pk2.h"
#include "mbd_launch.h"

namespace mbd {

RolloutKernel pk2_kernel(int fam, int max_col, int rk, int nfr, bool no_rk, int wpe, bool unit) {
  if (no_rk) nfr = 0;  // (the run-time forms read both)
  if (fam == 1) {  // ant (the reference's default env_name: mbd_planner.py:28, run_mbd.py:14)
    if (max_col > 2 || rk != MBD_REW_ANT) return nullptr;
    // (capped at 256 registers for two wavefronts per SIMD it is SLOWER here — 78 scratch accesses per control step:
    // N = 16384 2.71 -> 2.95 ms — so ant always runs the one-wavefront-per-SIMD form)
    if (rk == MBD_REW_ANT && nfr == 10) return rollout_pk2_kernel<2, MBD_REW_ANT, 10, 1, 1>;
    return rollout_pk2_kernel<2, -1, 0, 1, 1>;
  }
  if (max_col > 5) return nullptr;
  if (rk != MBD_REW_HUMANOIDRUN && rk != MBD_REW_HUMANOIDTRACK && rk != MBD_REW_HUMANOIDSTANDUP) return nullptr;
  if (max_col > 1) return rk == MBD_REW_HUMANOIDSTANDUP && nfr == 7 ? rollout_pk2_kernel<5, MBD_REW_HUMANOIDSTANDUP, 7>
                                                                    : rollout_pk2_kernel<5, -1, 0>;
  // (two wavefronts per SIMD: the reference's own humanoids with one collider per link; humanoidstandup's five
  // colliders do not fit 256 registers without spilling inside the substep loop — N = 16384: 4.36 -> 4.57 ms)
  // (the forms below with a reward kind and n_frames compiled in compile in the built-in humanoids' unit inverse inertia as
  // well — mbd_pk2.h unit_inertia_form_pk2; any other inertia: the same instantiation with the inertia at run time)
  if (!unit && rk == MBD_REW_HUMANOIDRUN && nfr == 7)
    return wpe == 2 ? rollout_pk2_kernel_rtib<1, MBD_REW_HUMANOIDRUN, 7, 2> : rollout_pk2_kernel_rtib<1, MBD_REW_HUMANOIDRUN, 7>;
  if (!unit && rk == MBD_REW_HUMANOIDTRACK && nfr == 5)
    return wpe == 2 ? rollout_pk2_kernel_rtib<1, MBD_REW_HUMANOIDTRACK, 5, 2> : rollout_pk2_kernel_rtib<1, MBD_REW_HUMANOIDTRACK, 5>;
  if (rk == MBD_REW_HUMANOIDRUN && nfr == 7)
    return wpe == 2 ? rollout_pk2_kernel<1, MBD_REW_HUMANOIDRUN, 7, 2> : rollout_pk2_kernel<1, MBD_REW_HUMANOIDRUN, 7>;
  if (rk == MBD_REW_HUMANOIDTRACK && nfr == 5)
    return wpe == 2 ? rollout_pk2_kernel<1, MBD_REW_HUMANOIDTRACK, 5, 2> : rollout_pk2_kernel<1, MBD_REW_HUMANOIDTRACK, 5>;
  return rollout_pk2_kernel<1, -1, 0>;
}

}  // namespace mbd
