// mbd_launch.h — what the translation units that hold rollout kernels share on the host side (mbd_env.hip, mbd_hot3d.hip,
// mbd_pk2.hip, mbd_planar.hip): the device-free facts of an env's model (EnvShape) and one lookup per unit that names the
// instantiation serving a model.  mbd_env.hip::choose_rollout asks them; launch_rollout launches what it chose.
#pragma once

#include <hip/hip_runtime.h>

#include "mbd_kernels.h"

namespace mbd {

// every rollout instantiation takes one RolloutParams: its host stub, or nullptr (no such instantiation)
using RolloutKernel = void (*)(RolloutParams);

// What the launch paths need to know of an env's model, derived once at env creation without a device (derive_shape).
struct EnvShape {
  int lps = 16, max_children = 0, max_col = 0, max_rot = 0;
  bool iso = false;          // mbd_model_t::iso_inertia
  bool unit_ib = false;      // iso, and every link's inverse inertia is exactly 1: the forms that compile it in (one-launch ensembles: of every member)
  bool diag_inertia = true;  // every body-frame inverse-inertia tensor is exactly diagonal
  bool axisym = true;        // ... with two equal entries: axisymmetric about a link axis (AXI instantiations)
  bool axi = false;          // diag_inertia && axisym && !iso
  bool slides = false;
  bool slide_limits = false;  // any slide dof with a finite range
  int max_slide = 0;          // largest slide-dof count of a joint
  bool slides_world_only = true;  // every joint with a slide dof hangs off the world
  bool has_weld = false;          // some joint has no hinge dof
  bool planar = false;            // MBD_FLAG_PLANAR: the planar restatement (mbd_planar.h)
  bool any_stiff = false;         // some hinge has a joint spring
  int fl = 0;  // the planar kernels' model switches: 1 joint springs | 2 slide limits | 4 elasticity
  // free root, isotropic inertia, no slide / weld joints, up to three children per link, multi-dof joints: the humanoids
  bool humanoid_shape = false;
  // DPP layout (kernels.h "lane exchange without the LDS"): lane <-> link tables when the tree fits the shifts
  int dpp_family = -1;  // index into kDppFamilies, -1: shuffles
  signed char lane_tab[32];
  bool helpers = false;  // one link with 3..5 colliders and two idle lanes to lend them to (HELP instantiations)
  bool spec = false;     // the model carries specification switches (MBD_SPEC_FLAGS): the general SPEC instantiations, 16 lanes
};

// The lookups.  rk: the model's reward kind, or -1 (lever MBD_NO_REWARD_CONST); nfr: n_frames, or 0 (run-time); unit: the
// forms with the unit inverse inertia compiled in may serve (EnvShape::unit_ib, unless lever MBD_NO_UNIT_CONST) — the ones
// with humanoidrun's / humanoidtrack's reward kind and n_frames compiled in; otherwise their rollout_kernel_rtib /
// rollout_pk2_kernel_rtib twins, which read the inertia from the lane record.
// mbd_hot3d.hip: the DPP instantiations the built-in humanoids and ant run (nullptr: the model is not one of those shapes);
// helpers: the humanoid form that lends colliders to idle lanes (EnvShape::helpers, unless lever MBD_NO_HELPERS)
RolloutKernel hot3d_kernel(const EnvShape& s, bool helpers, int rk, int nfr, bool unit);
// mbd_pk2.h, two candidates per lane: fam 0 the humanoid family, 1 ant; rk: the model's reward kind, no_rk: the run-time
// form whatever it is; wpe 2 asks for the form whose registers leave room for two wavefronts per SIMD (where there is
// one).  nullptr: no instantiation serves such a model.
RolloutKernel pk2_kernel(int fam, int max_col, int rk, int nfr, bool no_rk, int wpe, bool unit);
// mbd_planar.h: no_fl: the general instantiation (lever MBD_NO_PLANAR_FLAGS); early_out: the form that takes
// RolloutParams::cpw candidates per wavefront (nullptr where there is none)
RolloutKernel planar_kernel(const EnvShape& s, int rk, int nfr, bool no_fl, bool early_out);

}  // namespace mbd
