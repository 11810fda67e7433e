// mbd_step_args.h — the kernel arguments that the records of mbd_internal.h keep by value: what a unit needs of the step
// kernels (mbd_step_kernels.h) without seeing, and so emitting, any of them.
#pragma once

#include <cstdint>

namespace mbd {

struct WeighRec {
  int reject;  // drop NaN and +-inf rewards
  float ess_frac, temp_min, temp_max;
  int iters;
};
// where a step's log entry goes: plan 0's slot of each of the three logs, plan k's `stride` entries further
struct WeighLog {
  float* temp;
  float* ess;
  int* kept;
  long long stride;
};
// What a tick's disturbance launches need of every episode (blockIdx.y = episode; a single plan is episode 0), passed like
// SweepKeys: d_t of the disturbance key chain, the action-noise std, and the kick std — which the host sets to 0 in the
// ticks that carry no kick, so that it doubles as the kick kernels' mask.  has[k] == 0: the episode has no record.
struct SweepPlant {
  uint32_t k[32][2];
  float act_std[32], kick_std[32];
  unsigned char has[32];
};

}  // namespace mbd
