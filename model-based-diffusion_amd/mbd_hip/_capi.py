"""ctypes binding of libmbd_hip.so (include/mbd_hip.h) — the stub INTEGRATION.md shows a maintainer.

The library is the product: if it is missing, or no gfx950 device is visible, calls fail loudly
(``MbdError``); there is no Python/CPU fallback anywhere in this package.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .model import MbdModel

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "..", "lib", "libmbd_hip.so")

MBD_OK = 0
MBD_ERR_INVALID, MBD_ERR_UNSUPPORTED, MBD_ERR_HIP, MBD_ERR_NO_DEVICE, MBD_ERR_STATE = -1, -2, -3, -4, -5
PRNG_LEGACY, PRNG_PARTITIONABLE = 0, 1


class MbdError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libmbd_hip error {code}: {msg}")
        self.code = code


class PlanConfig(C.Structure):
    _fields_ = [("Nsample", C.c_int32), ("Hsample", C.c_int32), ("Ndiffuse", C.c_int32),
                ("temp_sample", C.c_float), ("beta0", C.c_float), ("betaT", C.c_float),
                ("enable_demo", C.c_int32), ("prng_impl", C.c_int32), ("shard_begin", C.c_int32),
                ("shard_count", C.c_int32), ("literal_score", C.c_int32), ("update_method", C.c_int32),
                ("shares_device", C.c_int32), ("reserved", C.c_int32 * 3)]


class MpcConfig(C.Structure):
    _fields_ = [("n_ticks", C.c_int32), ("warm_steps", C.c_int32), ("exec_steps", C.c_int32),
                ("reserved", C.c_int32 * 5)]


class MpcPlant(C.Structure):
    """mbd_mpc_plant (include/mbd_hip.h): the env that executes an episode's rows, and the episode's disturbances."""
    _fields_ = [("plant", C.c_void_p), ("key", C.c_uint32 * 2), ("act_std", C.c_float), ("kick_std", C.c_float),
                ("kick_every", C.c_int32), ("reserved", C.c_int32 * 3)]


MAX_ENSEMBLE = 8
RISK_MEAN, RISK_MIN = 0, 1
RISKS = {"mean": RISK_MEAN, "min": RISK_MIN}


class Ensemble(C.Structure):
    """mbd_ensemble (include/mbd_hip.h): the member envs every candidate of a plan is rolled out on, and the risk mode."""
    _fields_ = [("members", C.c_void_p * MAX_ENSEMBLE), ("n_members", C.c_int32), ("risk", C.c_int32),
                ("reserved", C.c_int32 * 6)]


NOISE_ALWAYS, NOISE_WARM_TICKS = 0, 1
NOISE_WHEN = {"always": NOISE_ALWAYS, "warm": NOISE_WARM_TICKS}


class NoiseShape(C.Structure):
    """mbd_noise_shape (include/mbd_hip.h): the table g [Hsample][action_size] the sampling noise is scaled by, and when."""
    _fields_ = [("scale", C.POINTER(C.c_float)), ("rows", C.c_int32), ("cols", C.c_int32), ("when", C.c_int32),
                ("reserved", C.c_int32 * 5)]


MAX_KNOTS = 16


class NoiseBasis(C.Structure):
    """mbd_noise_basis (include/mbd_hip.h): the table W [Hsample][n_knots] the sampling noise is correlated along the horizon
    through, and when."""
    _fields_ = [("basis", C.POINTER(C.c_float)), ("n_knots", C.c_int32), ("when", C.c_int32)]


MAX_MPC_DELAY = 8


class MpcDelay(C.Structure):
    """mbd_mpc_delay (include/mbd_hip.h): how many ticks a plan takes to arrive, and the rows the system is committed to when
    the episode starts."""
    _fields_ = [("rows0", C.POINTER(C.c_float)), ("delay_ticks", C.c_int32), ("n_rows", C.c_int32), ("reserved", C.c_int32 * 4)]


XREF_ROWS = 50  # csrc/mbd_kernels.h kXrefRows: the rows of a demo window


class MpcDemo(C.Structure):
    """mbd_mpc_demo (include/mbd_hip.h): the clip an episode follows, the row it starts at and the demo's reward level."""
    _fields_ = [("clip", C.POINTER(C.c_float)), ("n_rows", C.c_int32), ("start_row", C.c_int32), ("rew_xref", C.c_float),
                ("reserved", C.c_int32 * 4)]


class MpcSigma(C.Structure):
    """mbd_mpc_sigma (include/mbd_hip.h): the sigma a path-integral episode's cold and warm ticks start from, and the gain by
    which a warm tick's follows the sigma the last tick ended with."""
    _fields_ = [("sigma_cold", C.c_float), ("sigma_warm", C.c_float), ("gain", C.c_float), ("reserved", C.c_int32 * 5)]


class Objective(C.Structure):
    """mbd_objective (include/mbd_hip.h): the row weights, the actuator weights, the effort and rate costs a plan's rewards are
    shaped by, and the action executed before the first plan's row 0."""
    _fields_ = [("row_weight", C.POINTER(C.c_float)), ("act_weight", C.POINTER(C.c_float)), ("prev0", C.POINTER(C.c_float)),
                ("effort", C.c_float), ("rate", C.c_float), ("rows", C.c_int32), ("cols", C.c_int32), ("reserved", C.c_int32 * 5)]


class Weighting(C.Structure):
    """mbd_weighting (include/mbd_hip.h): whether candidates with a non-finite reward are left out of a step's weights, and the
    effective-sample-size target, bracket and bisection steps its temperature is chosen by."""
    _fields_ = [("reject_nonfinite", C.c_int32), ("ess_frac", C.c_float), ("temp_min", C.c_float), ("temp_max", C.c_float),
                ("iters", C.c_int32), ("reserved", C.c_int32 * 6)]


class Adapt(C.Structure):
    """mbd_adapt (include/mbd_hip.h): how fast the table that shapes a plan's sampling noise follows the weighted spread of its
    candidates, the clamp of its entries, and whether it is carried across tick boundaries."""
    _fields_ = [("rate", C.c_float), ("a_min", C.c_float), ("a_max", C.c_float), ("carry", C.c_int32), ("reserved", C.c_int32 * 4)]


class Elites(C.Structure):
    """mbd_elites (include/mbd_hip.h): how many of a step's best candidates the next step takes over, whether candidate 0 of every
    step is the step's mean itself, and whether the elites are carried across tick boundaries."""
    _fields_ = [("n_elites", C.c_int32), ("nominal", C.c_int32), ("carry", C.c_int32), ("reserved", C.c_int32 * 5)]


class Togo(C.Structure):
    """mbd_togo (include/mbd_hip.h): the horizon's rows in groups of ``block``, a group starting only where at least ``min_tail``
    rows are still ahead; group j's rows are updated under weights from the return from its first row onwards."""
    _fields_ = [("block", C.c_int32), ("min_tail", C.c_int32), ("reserved", C.c_int32 * 2)]


MAX_ZONES = 16
ZONE_KEEP_OUT, ZONE_GOAL = 0, 1


class Zone(C.Structure):
    """mbd_zone (include/mbd_hip.h): a keep-out region or a goal for the track slots of ``links`` — the distance is taken over
    the coordinate differences from ``center`` times ``scale``; a keep-out zone costs inside ``radius + margin``, a goal outside
    ``radius``."""
    _fields_ = [("kind", C.c_int32), ("links", C.c_uint32), ("center", C.c_float * 3), ("scale", C.c_float * 3),
                ("radius", C.c_float), ("margin", C.c_float), ("weight", C.c_float), ("reserved", C.c_int32)]


class Zones(C.Structure):
    """mbd_zones (include/mbd_hip.h): the table of a zone record."""
    _fields_ = [("n_zones", C.c_int32), ("reserved", C.c_int32 * 3), ("zone", Zone * MAX_ZONES)]


ELITES_MAX = 32
TOGO_MAX_N = 12288
PICK_MEAN, PICK_PREV, PICK_BEST = 1, 2, 4


class MpcPick(C.Structure):
    """mbd_mpc_pick (include/mbd_hip.h): which of a tick's three plans — its mean, the incumbent, the best candidate of its last
    step — the tick may hand on."""
    _fields_ = [("candidates", C.c_int32), ("reserved", C.c_int32 * 7)]


VALUE_MAX_LAYERS, VALUE_MAX_WIDTH = 4, 256
VALUE_RELU, VALUE_TANH = 0, 1
VALUE_REL_XY = 1


class Value(C.Structure):
    """mbd_value (include/mbd_hip.h): a small fully connected net over the env's state record, whose output at a rollout's final
    state is added, times ``scale``, to the candidate's reward."""
    _fields_ = [("W", C.POINTER(C.c_float) * VALUE_MAX_LAYERS), ("b", C.POINTER(C.c_float) * VALUE_MAX_LAYERS),
                ("center", C.POINTER(C.c_float)), ("in_scale", C.POINTER(C.c_float)), ("n_in", C.c_int32),
                ("n_layers", C.c_int32), ("width", C.c_int32 * VALUE_MAX_LAYERS), ("act", C.c_int32), ("flags", C.c_int32),
                ("scale", C.c_float), ("reserved", C.c_int32 * 5)]


TICK_ROWS_NONFINITE, TICK_STATE_NONFINITE, TICK_COLD = 1, 2, 4


class MpcTickInfo(C.Structure):
    """mbd_mpc_tick_info (include/mbd_hip.h): what a session's tick reports beside its rows."""
    _fields_ = [("tick", C.c_int32), ("flags", C.c_int32), ("rew_mean", C.c_float), ("seconds", C.c_float),
                ("reserved", C.c_int32 * 4)]


EXPORTS = [
    "mbd_last_error", "mbd_version", "mbd_tuned_spec", "mbd_device_count", "mbd_prng_key", "mbd_prng_split",
    "mbd_env_create", "mbd_env_name", "mbd_builtin_model", "mbd_env_get_model", "mbd_env_xref", "mbd_env_xref_logpd",
    "mbd_env_observe", "mbd_model_observe", "mbd_model_forward", "mbd_env_create_car2d", "mbd_env_create_model", "mbd_env_destroy", "mbd_env_info", "mbd_env_reset", "mbd_env_pipeline_init",
    "mbd_env_step", "mbd_env_rew_xref", "mbd_env_rollout", "mbd_plan_create", "mbd_plan_destroy",
    "mbd_plan_schedule", "mbd_plan_set_state0", "mbd_plan_sample_rollout", "mbd_plan_prefetch_noise", "mbd_plan_score_update",
    "mbd_plan_set_sigma", "mbd_plan_get_sigma", "mbd_plan_reverse_once", "mbd_plan_run", "mbd_plan_run_mpc", "mbd_plan_set_mpc_plant", "mbd_plan_set_ensemble", "mbd_plan_peek_ensemble", "mbd_plan_set_noise_shape", "mbd_plan_set_noise_basis", "mbd_plan_set_mpc_delay", "mbd_plan_peek_mpc_predicted", "mbd_plan_set_mpc_demo", "mbd_plan_peek_mpc_track", "mbd_plan_set_mpc_sigma", "mbd_plan_peek_mpc_sigma",
    "mbd_plan_set_objective", "mbd_plan_peek_objective", "mbd_sweep_set_objective", "mbd_sweep_peek_objective",
    "mbd_plan_set_weighting", "mbd_plan_peek_weighting", "mbd_sweep_set_weighting", "mbd_sweep_peek_weighting",
    "mbd_plan_set_mpc_pick", "mbd_plan_peek_mpc_pick", "mbd_sweep_set_mpc_pick", "mbd_sweep_peek_mpc_pick",
    "mbd_plan_set_value", "mbd_plan_peek_value", "mbd_plan_eval_value", "mbd_sweep_set_value",
    "mbd_plan_set_adapt", "mbd_plan_peek_adapt", "mbd_plan_set_elites", "mbd_plan_peek_elites",
    "mbd_plan_set_togo", "mbd_plan_peek_togo",
    "mbd_plan_set_zones", "mbd_plan_update_zones", "mbd_plan_peek_zones", "mbd_plan_peek_mpc_zones",
    "mbd_sweep_set_zones", "mbd_sweep_update_zones", "mbd_sweep_peek_zones", "mbd_sweep_peek_mpc_zones",
    "mbd_sweep_set_elites", "mbd_sweep_peek_elites", "mbd_sweep_set_togo", "mbd_sweep_peek_togo",
    "mbd_plan_mpc_open", "mbd_plan_mpc_submit", "mbd_plan_mpc_collect", "mbd_plan_mpc_tick", "mbd_plan_mpc_reset_mean",
    "mbd_plan_mpc_close", "mbd_plan_eval", "mbd_plan_peek", "mbd_plan_kernel_time",
    "mbd_plan_enable_timing",
    "mbd_sweep_create", "mbd_sweep_destroy", "mbd_sweep_set_state0", "mbd_sweep_run", "mbd_sweep_run_mpc", "mbd_sweep_set_mpc_plant", "mbd_sweep_set_noise_shape", "mbd_sweep_set_noise_basis", "mbd_sweep_set_mpc_delay", "mbd_sweep_peek_mpc_predicted", "mbd_sweep_set_mpc_demo", "mbd_sweep_peek_mpc_track", "mbd_sweep_set_mpc_sigma", "mbd_sweep_peek_mpc_sigma", "mbd_sweep_mpc_open", "mbd_sweep_mpc_submit", "mbd_sweep_mpc_collect", "mbd_sweep_mpc_tick", "mbd_sweep_mpc_reset_mean",
    "mbd_sweep_mpc_close", "mbd_sweep_kernel_time", "mbd_sweep_get_sigmas",
    "mbd_exchange_create", "mbd_exchange_destroy", "mbd_exchange_local_handle", "mbd_exchange_connect",
    "mbd_exchange_all_gather", "mbd_exchange_status", "mbd_exchange_fine_grained",
]

_lib = None
_vp, _i, _f = C.c_void_p, C.c_int, C.c_float
_u32p = C.POINTER(C.c_uint32)
_fp = C.POINTER(C.c_float)


def load() -> C.CDLL:
    """dlopen the in-tree library. Raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.path.abspath(os.environ.get("MBD_HIP_LIB") or LIB_PATH)  # override: kernel A/B builds only
    if not os.path.exists(path):
        raise MbdError(MBD_ERR_STATE, f"{path} is missing: run `python __graft_entry__.py` (build()) first; "
                                      "mbd_hip has no CPU fallback")
    # torch (device memory / streams / torch.distributed plumbing) bundles its own HIP runtime with the
    # same SONAME as the system one: it has to be the first one mapped, or two runtimes fight over the
    # device ("No HIP GPUs are available")
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    lib.mbd_last_error.restype = C.c_char_p
    lib.mbd_device_count.argtypes = [C.POINTER(_i)]
    lib.mbd_prng_key.argtypes = [C.c_uint64, _u32p]
    lib.mbd_prng_split.argtypes = [_u32p, _i, _i, _u32p]
    lib.mbd_env_create.argtypes = [C.c_char_p, _i, C.POINTER(_vp)]
    lib.mbd_env_name.argtypes = [_i]
    lib.mbd_env_name.restype = C.c_char_p
    lib.mbd_builtin_model.argtypes = [C.c_char_p, C.POINTER(MbdModel)]
    lib.mbd_env_get_model.argtypes = [_vp, C.POINTER(MbdModel)]
    lib.mbd_env_xref.argtypes = [_vp, _vp, _i, C.POINTER(_i)]
    lib.mbd_env_xref_logpd.argtypes = [_vp, _vp, _i, _i, _vp, _vp]
    lib.mbd_env_observe.argtypes = [_vp, _vp, _vp]
    lib.mbd_model_observe.argtypes = [C.POINTER(MbdModel), _vp, _vp, _vp, _vp]
    lib.mbd_env_create_car2d.argtypes = [_i, _vp, C.POINTER(_vp)]
    lib.mbd_env_create_model.argtypes = [C.c_char_p, _i, C.POINTER(MbdModel), _vp, _f, C.POINTER(_vp)]
    lib.mbd_env_destroy.argtypes = [_vp]
    lib.mbd_env_info.argtypes = [_vp] + [C.POINTER(_i)] * 5 + [_fp]
    lib.mbd_env_reset.argtypes = [_vp, _u32p, _i, _vp]
    lib.mbd_model_forward.argtypes = [_vp, _vp, _vp, _vp]
    lib.mbd_env_pipeline_init.argtypes = [_vp, _vp, _i, _vp, _i, _vp]
    lib.mbd_env_step.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp]
    lib.mbd_env_rew_xref.argtypes = [_vp, _fp]
    lib.mbd_env_rollout.argtypes = [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]
    lib.mbd_plan_create.argtypes = [_vp, C.POINTER(PlanConfig), C.POINTER(_vp)]
    lib.mbd_plan_destroy.argtypes = [_vp]
    lib.mbd_plan_schedule.argtypes = [_vp, _vp, _vp, _vp]
    lib.mbd_plan_set_state0.argtypes = [_vp, _vp]
    lib.mbd_plan_sample_rollout.argtypes = [_vp, _i, _u32p, _vp, _vp, _vp, _vp]
    lib.mbd_plan_prefetch_noise.argtypes = [_vp, _u32p, _vp]
    lib.mbd_plan_score_update.argtypes = [_vp, _i, _u32p, _vp, _vp, _vp, _vp, _vp, _vp]
    lib.mbd_plan_set_sigma.argtypes = [_vp, _f]
    lib.mbd_plan_get_sigma.argtypes = [_vp, _fp]
    lib.mbd_plan_reverse_once.argtypes = [_vp, _i, _u32p, _vp, _vp, _vp]
    lib.mbd_plan_run.argtypes = [_vp, _u32p, _vp, _vp, _fp, C.POINTER(C.c_double)]
    lib.mbd_plan_run_mpc.argtypes = [_vp, C.POINTER(MpcConfig), _u32p, _vp, _vp, _vp, _vp, C.POINTER(C.c_double)]
    lib.mbd_plan_set_mpc_plant.argtypes = [_vp, C.POINTER(MpcPlant)]
    lib.mbd_plan_set_ensemble.argtypes = [_vp, C.POINTER(Ensemble)]
    lib.mbd_plan_peek_ensemble.argtypes = [_vp, _vp, _vp]
    lib.mbd_plan_set_noise_shape.argtypes = [_vp, C.POINTER(NoiseShape)]
    lib.mbd_plan_set_noise_basis.argtypes = [_vp, C.POINTER(NoiseBasis)]
    lib.mbd_plan_set_mpc_delay.argtypes = [_vp, C.POINTER(MpcDelay)]
    lib.mbd_plan_peek_mpc_predicted.argtypes = [_vp, _vp]
    lib.mbd_plan_set_mpc_demo.argtypes = [_vp, C.POINTER(MpcDemo)]
    lib.mbd_plan_peek_mpc_track.argtypes = [_vp, _vp, _vp]
    lib.mbd_plan_set_mpc_sigma.argtypes = [_vp, C.POINTER(MpcSigma)]
    lib.mbd_plan_peek_mpc_sigma.argtypes = [_vp, _vp]
    lib.mbd_plan_set_objective.argtypes = [_vp, C.POINTER(Objective)]
    lib.mbd_plan_peek_objective.argtypes = [_vp, _vp, _vp]
    lib.mbd_sweep_set_objective.argtypes = [_vp, C.POINTER(Objective)]
    lib.mbd_sweep_peek_objective.argtypes = [_vp, _i, _vp, _vp]
    lib.mbd_plan_set_weighting.argtypes = [_vp, C.POINTER(Weighting)]
    lib.mbd_plan_peek_weighting.argtypes = [_vp, _vp, _vp, _vp, _i, C.POINTER(C.c_int)]
    lib.mbd_sweep_set_weighting.argtypes = [_vp, C.POINTER(Weighting)]
    lib.mbd_sweep_peek_weighting.argtypes = [_vp, _i, _vp, _vp, _vp, _i, C.POINTER(C.c_int)]
    lib.mbd_plan_set_mpc_pick.argtypes = [_vp, C.POINTER(MpcPick)]
    lib.mbd_plan_peek_mpc_pick.argtypes = [_vp, _vp, _vp, _vp, _i, C.POINTER(C.c_int)]
    lib.mbd_sweep_set_mpc_pick.argtypes = [_vp, C.POINTER(MpcPick)]
    lib.mbd_sweep_peek_mpc_pick.argtypes = [_vp, _i, _vp, _vp, _vp, _i, C.POINTER(C.c_int)]
    lib.mbd_plan_set_value.argtypes = [_vp, C.POINTER(Value)]
    lib.mbd_plan_peek_value.argtypes = [_vp, _vp]
    lib.mbd_plan_eval_value.argtypes = [_vp, _vp, _i, _vp]
    lib.mbd_sweep_set_value.argtypes = [_vp, C.POINTER(Value)]
    lib.mbd_plan_set_adapt.argtypes = [_vp, C.POINTER(Adapt)]
    lib.mbd_plan_set_elites.argtypes = [_vp, C.POINTER(Elites)]
    lib.mbd_plan_set_togo.argtypes = [_vp, C.POINTER(Togo)]
    lib.mbd_plan_peek_togo.argtypes = [_vp, _vp, _vp, _vp, _vp]
    lib.mbd_plan_peek_elites.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, C.POINTER(C.c_int)]
    lib.mbd_sweep_set_elites.argtypes = [_vp, C.POINTER(Elites)]
    lib.mbd_sweep_peek_elites.argtypes = [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, C.POINTER(C.c_int)]
    lib.mbd_sweep_set_togo.argtypes = [_vp, C.POINTER(Togo)]
    lib.mbd_sweep_peek_togo.argtypes = [_vp, _i, _vp, _vp, _vp, _vp]
    lib.mbd_plan_peek_adapt.argtypes = [_vp, _vp, _vp, _vp, _i, C.POINTER(C.c_int)]
    lib.mbd_plan_set_zones.argtypes = [_vp, C.POINTER(Zones)]
    lib.mbd_plan_update_zones.argtypes = [_vp, C.POINTER(Zones)]
    lib.mbd_plan_peek_zones.argtypes = [_vp, _vp, _vp]
    lib.mbd_plan_peek_mpc_zones.argtypes = [_vp, _vp, _vp]
    lib.mbd_sweep_set_zones.argtypes = [_vp, C.POINTER(Zones)]
    lib.mbd_sweep_update_zones.argtypes = [_vp, C.POINTER(Zones)]
    lib.mbd_sweep_peek_zones.argtypes = [_vp, _i, _vp, _vp]
    lib.mbd_sweep_peek_mpc_zones.argtypes = [_vp, _i, _vp, _vp]
    lib.mbd_plan_mpc_open.argtypes = [_vp, C.POINTER(MpcConfig), _u32p]
    lib.mbd_plan_mpc_submit.argtypes = [_vp, _vp]
    lib.mbd_plan_mpc_collect.argtypes = [_vp, _vp, _vp, _vp, _vp, C.POINTER(MpcTickInfo)]
    lib.mbd_plan_mpc_tick.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(MpcTickInfo)]
    lib.mbd_plan_mpc_reset_mean.argtypes = [_vp]
    lib.mbd_plan_mpc_close.argtypes = [_vp]
    lib.mbd_plan_eval.argtypes = [_vp, _vp, _fp]
    lib.mbd_plan_peek.argtypes = [_vp, _vp, _vp, _vp]
    lib.mbd_plan_kernel_time.argtypes = [_vp, _fp, C.POINTER(_i), _i]
    lib.mbd_plan_enable_timing.argtypes = [_vp, _i]
    lib.mbd_sweep_create.argtypes = [_vp, C.POINTER(PlanConfig), _i, _vp, C.POINTER(_vp)]
    lib.mbd_sweep_destroy.argtypes = [_vp]
    lib.mbd_sweep_set_state0.argtypes = [_vp, _i, _vp]
    lib.mbd_sweep_run.argtypes = [_vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_double)]
    lib.mbd_sweep_run_mpc.argtypes = [_vp, C.POINTER(MpcConfig), _vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_double)]
    lib.mbd_sweep_set_mpc_plant.argtypes = [_vp, _i, C.POINTER(MpcPlant)]
    lib.mbd_sweep_set_noise_shape.argtypes = [_vp, C.POINTER(NoiseShape)]
    lib.mbd_sweep_set_noise_basis.argtypes = [_vp, C.POINTER(NoiseBasis)]
    lib.mbd_sweep_set_mpc_delay.argtypes = [_vp, C.POINTER(MpcDelay)]
    lib.mbd_sweep_peek_mpc_predicted.argtypes = [_vp, _vp]
    lib.mbd_sweep_set_mpc_demo.argtypes = [_vp, C.POINTER(MpcDemo)]
    lib.mbd_sweep_peek_mpc_track.argtypes = [_vp, _i, _vp, _vp]
    lib.mbd_sweep_set_mpc_sigma.argtypes = [_vp, C.POINTER(MpcSigma)]
    lib.mbd_sweep_peek_mpc_sigma.argtypes = [_vp, _i, _vp]
    lib.mbd_sweep_mpc_open.argtypes = [_vp, C.POINTER(MpcConfig), _vp]
    lib.mbd_sweep_mpc_submit.argtypes = [_vp, _vp]
    lib.mbd_sweep_mpc_collect.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp]
    lib.mbd_sweep_mpc_tick.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp]
    lib.mbd_sweep_mpc_reset_mean.argtypes = [_vp, _i]
    lib.mbd_sweep_mpc_close.argtypes = [_vp]
    lib.mbd_sweep_kernel_time.argtypes = [_vp, _i, _fp, C.POINTER(_i)]
    lib.mbd_sweep_get_sigmas.argtypes = [_vp, _vp]
    lib.mbd_exchange_create.argtypes = [_i, _i, _i, _i, _i, C.POINTER(_vp)]
    lib.mbd_exchange_destroy.argtypes = [_vp]
    lib.mbd_exchange_local_handle.argtypes = [_vp, _vp]
    lib.mbd_exchange_connect.argtypes = [_vp, _vp]
    lib.mbd_exchange_all_gather.argtypes = [_vp, _vp, C.POINTER(_vp), _vp]
    lib.mbd_exchange_status.argtypes = [_vp]
    lib.mbd_exchange_fine_grained.argtypes = [_vp, C.POINTER(_i)]
    _lib = lib
    return lib


LEVERS = ("MBD_NO_DPP", "MBD_NO_NFR_CONST", "MBD_NO_REWARD_CONST", "MBD_NO_PLANAR_FLAGS", "MBD_NO_FAST_SLIDES",
          "MBD_NO_FUSED_NOISE", "MBD_NO_LAZY", "MBD_NO_PREFETCH", "MBD_NO_AUX", "MBD_WMEAN_SPLIT", "MBD_NO_FUSED_SCORE",
          "MBD_PK2", "MBD_WPB", "MBD_LDS_RESERVE", "MBD_NO_HELPERS", "MBD_ENS_SPLIT", "MBD_NO_UNIT_CONST",
          "MBD_VALUE_TILE")


def debug_set(name: str, value: int) -> None:
    """include/mbd_hip_debug.h: a test / A-B lever of the library (-1: not set).  The library reads the environment
    variables of the same names once, when it is first used; afterwards only this call changes a lever."""
    lib = load()
    lib.mbd_debug_set.argtypes = [C.c_char_p, _i]
    check(lib.mbd_debug_set(name.encode(), int(value)))


def debug_get(name: str) -> int:
    lib = load()
    lib.mbd_debug_get.argtypes = [C.c_char_p, C.POINTER(_i)]
    v = _i(0)
    check(lib.mbd_debug_get(name.encode(), C.byref(v)))
    return v.value


def debug_rollout_choice(model, n_cus: int, B: int, H: int, sweep_plan_N: int = 0, has_xref: bool = False) -> dict:
    """include/mbd_hip_debug.h: the rollout launch the library picks for `model` (an MbdModel) — no device needed."""
    lib = load()
    lib.mbd_debug_rollout_choice.argtypes = [C.POINTER(MbdModel), _i, _i, _i, _i, _i, C.c_char_p, _i, C.POINTER(_i)]
    name = C.create_string_buffer(512)
    out = (_i * 8)()
    check(lib.mbd_debug_rollout_choice(C.byref(model), n_cus, B, H, sweep_plan_N, int(has_xref), name, 512, out))
    keys = ("grid", "block", "lds", "cpw", "wpe", "xcd_pin", "fuses_noise", "fuses_logpd")
    return dict(zip(keys, list(out)), name=name.value.decode())


def debug_noise_shaped(key, impl: int, N: int, HNu: int, g, wide: bool, blocks: int) -> np.ndarray:
    """include/mbd_hip_debug.h: z [N, HNu] = normal(key, (N, HNu)) * g by the noise kernels' shaped loops, with 32-bit
    (``wide`` False) or 64-bit indices, on ``blocks`` workgroups."""
    lib = load()
    lib.mbd_debug_noise_shaped.argtypes = [_u32p, _i, _i, _i, _vp, _i, _i, _vp]
    g = np.ascontiguousarray(g, np.float32).reshape(HNu)
    out = np.empty((N, HNu), np.float32)
    check(lib.mbd_debug_noise_shaped(key_array(key), impl, N, HNu, np_ptr(g), int(wide), blocks, np_ptr(out)))
    return out


def debug_knot_noise(key, impl: int, N: int, H: int, Nu: int, W, g, blocks: int) -> np.ndarray:
    """include/mbd_hip_debug.h: z [N, H, Nu] of a step under the noise basis ``W`` [H, n_knots] (and the shape ``g`` [H, Nu], or
    None) by knot_noise_kernel alone, on ``blocks`` workgroups."""
    lib = load()
    lib.mbd_debug_knot_noise.argtypes = [_u32p, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp]
    W = np.ascontiguousarray(W, np.float32).reshape(H, -1)
    g = None if g is None else np.ascontiguousarray(g, np.float32).reshape(H * Nu)
    out = np.empty((N, H, Nu), np.float32)
    check(lib.mbd_debug_knot_noise(key_array(key), impl, N, H, Nu, W.shape[1], np_ptr(W), None if g is None else np_ptr(g), blocks,
                                   np_ptr(out)))
    return out


def debug_knot_noise_host(key, impl: int, N: int, H: int, Nu: int, W, g) -> np.ndarray:
    """include/mbd_hip_debug.h: ``debug_knot_noise``'s z by the kernel's per-column code run on the host (no device)."""
    lib = load()
    lib.mbd_debug_knot_noise_host.argtypes = [_u32p, _i, _i, _i, _i, _i, _vp, _vp, _vp]
    W = np.ascontiguousarray(W, np.float32).reshape(H, -1)
    g = None if g is None else np.ascontiguousarray(g, np.float32).reshape(H * Nu)
    out = np.full((N, H, Nu), np.nan, np.float32)
    check(lib.mbd_debug_knot_noise_host(key_array(key), impl, N, H, Nu, W.shape[1], np_ptr(W), None if g is None else np_ptr(g),
                                        np_ptr(out)))
    return out


def debug_check_mpc_delay(rec: "MpcDelay", action_size: int) -> int:
    """include/mbd_hip_debug.h: the refusals a delay record alone decides, for a handle of that action_size — no device
    needed.  Returns the code (the message: ``load().mbd_last_error()``)."""
    lib = load()
    lib.mbd_debug_check_mpc_delay.argtypes = [C.POINTER(MpcDelay), _i]
    return lib.mbd_debug_check_mpc_delay(C.byref(rec), int(action_size))


def debug_mpc_sigma_next(sigma_end, cold: float, warm: float, gain: float) -> np.ndarray:
    """include/mbd_hip_debug.h: the sigma a warm tick of a path-integral episode starts from, for every value of ``sigma_end``,
    by the boundary kernel's own function run on the host (no device)."""
    lib = load()
    lib.mbd_debug_mpc_sigma_next.argtypes = [_vp, _i, _f, _f, _f, _vp]
    x = np.ascontiguousarray(sigma_end, np.float32).reshape(-1)
    out = np.empty_like(x)
    check(lib.mbd_debug_mpc_sigma_next(np_ptr(x), x.size, cold, warm, gain, np_ptr(out)))
    return out


def debug_check_mpc_sigma(rec: "MpcSigma", update_method: int) -> int:
    """include/mbd_hip_debug.h: the refusals a sigma record alone decides for a handle of that update_method — no device
    needed.  Returns the code (the message: ``load().mbd_last_error()``)."""
    lib = load()
    lib.mbd_debug_check_mpc_sigma.argtypes = [C.POINTER(MpcSigma), _i]
    return lib.mbd_debug_check_mpc_sigma(C.byref(rec), int(update_method))


def debug_check_objective(rec: "Objective", Hsample: int, action_size: int) -> int:
    """include/mbd_hip_debug.h: the refusals an objective record alone decides, for a handle of that Hsample and action_size — no
    device needed.  Returns the code (the message: ``load().mbd_last_error()``)."""
    lib = load()
    lib.mbd_debug_check_objective.argtypes = [C.POINTER(Objective), _i, _i]
    return lib.mbd_debug_check_objective(C.byref(rec), int(Hsample), int(action_size))


def debug_objective_host(rewss, rews, cand, w=None, q=None, effort: float = 0.0, rate: float = 0.0, prev=None, lazy=None):
    """include/mbd_hip_debug.h: objective_kernel's arithmetic run on the host (no device).  ``rewss`` [B, H], ``rews`` [B],
    ``cand`` [N, H, Nu] (row b is candidate b % N), ``w`` [H] or None, ``q`` [Nu] or None (ones), ``prev`` [Nu] (clipped) or None;
    ``lazy`` None: cand holds values, else (sigma, ybar [H, Nu]): it holds normals.  Returns (rews_out [B], ret [B], cost [min(B, N)])."""
    lib = load()
    lib.mbd_debug_objective_host.argtypes = [_vp, _vp, _i, _i, _i, _i, _vp, _i, _f, _vp, _vp, _f, _vp, _f, _f, _vp, _vp, _vp, _vp]
    f32 = lambda x: np.ascontiguousarray(x, np.float32)
    rewss, rews, cand = f32(rewss), f32(rews), f32(cand)
    B, H = rewss.shape
    N, _, Nu = cand.shape
    wsum = np.float32(0)
    if w is not None:
        w = f32(w)
        for x in w:  # the f32 left-to-right sum the set call forms
            wsum = np.float32(wsum + x)
    q = np.ones(Nu, np.float32) if q is None else f32(q)
    prev = None if prev is None else f32(prev)
    sigma, ybar = (0.0, None) if lazy is None else (float(lazy[0]), f32(lazy[1]))
    out, ret, cost = np.full(B, np.nan, np.float32), np.full(B, np.nan, np.float32), np.full(min(B, N), np.nan, np.float32)
    opt = lambda a: None if a is None else np_ptr(a)
    check(lib.mbd_debug_objective_host(np_ptr(rewss), np_ptr(rews), B, N, H, Nu, np_ptr(cand), int(lazy is not None), sigma, opt(ybar),
                                       opt(w), float(wsum), np_ptr(q), float(effort), float(rate), opt(prev), np_ptr(out), np_ptr(ret),
                                       np_ptr(cost)))
    return out, ret, cost


def debug_check_value(rec: "Value", state_size: int, rigid_body: bool = True) -> int:
    """include/mbd_hip_debug.h: the refusals a value record alone decides, for an env of that state_size and kind — no device
    needed.  Returns the code (the message: ``load().mbd_last_error()``)."""
    lib = load()
    lib.mbd_debug_check_value.argtypes = [C.POINTER(Value), _i, _i]
    return lib.mbd_debug_check_value(C.byref(rec), int(state_size), int(bool(rigid_body)))


def debug_value_host(rec: "Value", states, rews=None, rigid_body: bool = True):
    """include/mbd_hip_debug.h: value_kernel's arithmetic run on the host (no device).  ``states`` [B, n_in], ``rews`` [B] or None.
    Returns V [B], or (V, rews + scale * V) when ``rews`` is given."""
    lib = load()
    lib.mbd_debug_value_host.argtypes = [C.POINTER(Value), _i, _vp, _vp, _i, _vp, _vp]
    states = np.ascontiguousarray(states, np.float32)
    B = states.shape[0]
    v = np.full(B, np.nan, np.float32)
    if rews is None:
        check(lib.mbd_debug_value_host(C.byref(rec), int(bool(rigid_body)), np_ptr(states), None, B, np_ptr(v), None))
        return v
    rews = np.ascontiguousarray(rews, np.float32)
    out = np.full(B, np.nan, np.float32)
    check(lib.mbd_debug_value_host(C.byref(rec), int(bool(rigid_body)), np_ptr(states), np_ptr(rews), B, np_ptr(v), np_ptr(out)))
    return v, out


def weighting_record(reject_nonfinite=True, ess_frac: float = 0.0, temp_min=None, temp_max=None, iters: int = 12) -> "Weighting":
    """The mbd_weighting of ``set_weighting``'s arguments (a bracket of None: zeros, which the library accepts with ess_frac == 0)."""
    rec = Weighting()
    rec.reject_nonfinite = int(reject_nonfinite)
    rec.ess_frac = float(ess_frac)
    rec.temp_min = 0.0 if temp_min is None else float(temp_min)
    rec.temp_max = 0.0 if temp_max is None else float(temp_max)
    rec.iters = int(iters)
    return rec


def debug_weighting_host(rews, temp: float, rec: "Weighting" = None, std_guard: int = 1):
    """include/mbd_hip_debug.h: weigh_kernel's arithmetic run on the host (no device).  ``rews`` [N], ``temp`` T0, ``rec`` a
    ``Weighting`` or None.  Returns (weights [N], rew_mean, T*, ess, kept)."""
    lib = load()
    lib.mbd_debug_weighting_host.argtypes = [_vp, _i, _f, _i, C.POINTER(Weighting), _vp, _vp, _vp, _vp, _vp]
    rews = np.ascontiguousarray(rews, np.float32)
    w = np.full(rews.shape[0], np.nan, np.float32)
    mean, T, ess, kept = np.zeros(1, np.float32), np.zeros(1, np.float32), np.zeros(1, np.float32), np.zeros(1, np.int32)
    check(lib.mbd_debug_weighting_host(np_ptr(rews), rews.shape[0], float(temp), int(std_guard), None if rec is None else C.byref(rec),
                                       np_ptr(w), np_ptr(mean), np_ptr(T), np_ptr(ess), np_ptr(kept)))
    return w, mean[0], T[0], ess[0], int(kept[0])


def peek_weighting(fn, handle, k, capacity: int) -> dict:
    """mbd_plan_peek_weighting (k None) or mbd_sweep_peek_weighting: {'temp', 'ess', 'kept'}, one entry per score step."""
    temp, ess, kept = np.zeros(capacity, np.float32), np.zeros(capacity, np.float32), np.zeros(capacity, np.int32)
    n = C.c_int(0)
    head = (handle,) if k is None else (handle, int(k))
    check(fn(*head, np_ptr(temp), np_ptr(ess), np_ptr(kept), int(capacity), C.byref(n)))
    m = min(n.value, capacity)
    return {"temp": temp[:m], "ess": ess[:m], "kept": kept[:m]}


def adapt_record(rate: float, a_min: float, a_max: float, carry=True) -> "Adapt":
    """The mbd_adapt of ``Plan.set_adapt``'s arguments."""
    rec = Adapt()
    rec.rate, rec.a_min, rec.a_max, rec.carry = float(rate), float(a_min), float(a_max), int(carry)
    return rec


def debug_check_adapt(rec: "Adapt", update_method: int = 0, enable_demo: bool = False) -> int:
    """include/mbd_hip_debug.h: the refusals an adapt record alone decides for a plan of that update_method and enable_demo; the
    return code (the message: ``mbd_last_error``)."""
    lib = load()
    lib.mbd_debug_check_adapt.argtypes = [C.POINTER(Adapt), _i, _i]
    return lib.mbd_debug_check_adapt(None if rec is None else C.byref(rec), int(update_method), int(bool(enable_demo)))


def _debug_adapt(device: bool, w, cand, ybar, sigma, lazy, a, g, rate, a_min, a_max, sigma_on_device=False):
    lib = load()
    w = np.ascontiguousarray(w, np.float32)
    cand = np.ascontiguousarray(cand, np.float32).reshape(w.shape[0], -1)
    N, HNu = cand.shape
    ybar = np.ascontiguousarray(ybar, np.float32).reshape(HNu)
    a = np.ascontiguousarray(a, np.float32).reshape(HNu)
    g = None if g is None else np.ascontiguousarray(g, np.float32).reshape(HNu)
    a_out, G_out = np.full(HNu, np.nan, np.float32), np.full(HNu, np.nan, np.float32)
    S, skipped = np.full(1, np.nan, np.float32), np.full(1, -1, np.int32)
    gp = None if g is None else np_ptr(g)
    tail = (np_ptr(a), gp, float(rate), float(a_min), float(a_max), np_ptr(a_out), np_ptr(G_out), np_ptr(S), np_ptr(skipped))
    if device:
        lib.mbd_debug_adapt_step.argtypes = [_vp, _vp, _i, _i, _vp, _f, _i, _i, _vp, _vp, _f, _f, _f, _vp, _vp, _vp, _vp]
        check(lib.mbd_debug_adapt_step(np_ptr(w), np_ptr(cand), N, HNu, np_ptr(ybar), float(sigma), int(bool(sigma_on_device)),
                                       int(bool(lazy)), *tail))
    else:
        lib.mbd_debug_adapt_host.argtypes = [_vp, _vp, _i, _i, _vp, _f, _i, _vp, _vp, _f, _f, _f, _vp, _vp, _vp, _vp]
        check(lib.mbd_debug_adapt_host(np_ptr(w), np_ptr(cand), N, HNu, np_ptr(ybar), float(sigma), int(bool(lazy)), *tail))
    return a_out, G_out, S[0], int(skipped[0])


def debug_adapt_host(w, cand, ybar, sigma, lazy, a, g, rate, a_min, a_max):
    """include/mbd_hip_debug.h: an adapt record's update on the host (no device).  ``w`` [N], ``cand`` [N, HNu] (values, or with
    ``lazy`` shaped normals), ``ybar`` [HNu], ``a`` [HNu], ``g`` [HNu] or None.  Returns (a' [HNu], G' [HNu], S, skipped)."""
    return _debug_adapt(False, w, cand, ybar, sigma, lazy, a, g, rate, a_min, a_max)


def debug_adapt_step(w, cand, ybar, sigma, lazy, a, g, rate, a_min, a_max, sigma_on_device=False):
    """The same by the launches a step makes, on the device; ``sigma_on_device``: the kernels read sigma from a device scalar."""
    return _debug_adapt(True, w, cand, ybar, sigma, lazy, a, g, rate, a_min, a_max, sigma_on_device)


def peek_adapt(fn, handle, HNu: int, capacity: int = None) -> dict:
    """mbd_plan_peek_adapt: {'a' [HNu], 'ratio' [n], 'skipped' [n], 'count'} — every step logged, or the most recent ``capacity``."""
    n = C.c_int(0)
    if capacity is None:
        check(fn(handle, None, None, None, 0, C.byref(n)))
        capacity = min(n.value, 65536)
    a = np.zeros(HNu, np.float32)
    ratio, skipped = np.zeros(max(capacity, 1), np.float32), np.zeros(max(capacity, 1), np.int32)
    check(fn(handle, np_ptr(a), np_ptr(ratio), np_ptr(skipped), int(capacity), C.byref(n)))
    m = min(n.value, capacity)
    return {"a": a, "ratio": ratio[:m], "skipped": skipped[:m], "count": n.value}


def elites_record(n_elites: int, nominal=False, carry=False) -> "Elites":
    """The mbd_elites of ``Plan.set_elites``'s arguments."""
    rec = Elites()
    rec.n_elites, rec.nominal, rec.carry = int(n_elites), int(nominal), int(carry)
    return rec


def debug_check_elites(rec: "Elites", Nsample: int, update_method: int = 0, enable_demo: bool = False) -> int:
    """include/mbd_hip_debug.h: the refusals an elite record alone decides for a plan of that Nsample, update_method and
    enable_demo; the return code (the message: ``mbd_last_error``)."""
    lib = load()
    lib.mbd_debug_check_elites.argtypes = [C.POINTER(Elites), _i, _i, _i]
    return lib.mbd_debug_check_elites(None if rec is None else C.byref(rec), int(Nsample), int(update_method), int(bool(enable_demo)))


def _elites_arrays(cand, ybar, g, n_elites, E_in):
    cand = np.ascontiguousarray(cand, np.float32)
    cand = cand.reshape(cand.shape[0], -1)
    N, HNu = cand.shape
    ybar = np.ascontiguousarray(ybar, np.float32).reshape(HNu)
    g = None if g is None else np.ascontiguousarray(g, np.float32).reshape(HNu)
    E_in = np.zeros((0, HNu), np.float32) if E_in is None else np.ascontiguousarray(E_in, np.float32).reshape(-1, HNu)
    return cand, N, HNu, ybar, g, E_in


def _elites_outputs(n_elites, HNu):
    k = max(int(n_elites), 1)
    return (np.zeros((k, HNu), np.float32), np.zeros(k, np.float32), np.zeros(k, np.int32), np.full(1, -1, np.int32),
            np.full(1, -1, np.int32), np.zeros(1, np.float32))


def _elites_result(n_elites, outs, cand_out=None):
    E, R, src, count, kept, top = outs
    res = dict(E=E[:n_elites], R=R[:n_elites], src=src[:n_elites], count=int(count[0]), kept=int(kept[0]), top=top[0])
    if cand_out is not None:
        res["cand"] = cand_out
    return res


def debug_elites_host(rews, cand, ybar, sigma, lazy, g, n_elites, nominal, E_in=None):
    """include/mbd_hip_debug.h: one step of an elite record on the host (no device) — the injection of ``E_in`` [count, HNu] (and the
    nominal) into a copy of ``cand`` [N, HNu] (values, or with ``lazy`` normals), then the selection over ``rews`` [N].  Returns
    dict(cand [N, HNu] behind the injection, E [n_elites, HNu], R, src [n_elites] — all bits set from ``count`` on —, count, kept,
    top)."""
    lib = load()
    cand, N, HNu, ybar, g, E_in = _elites_arrays(cand, ybar, g, n_elites, E_in)
    rews = np.ascontiguousarray(rews, np.float32).reshape(N)
    outs = _elites_outputs(n_elites, HNu)
    cand_out = np.zeros_like(cand)
    lib.mbd_debug_elites_host.argtypes = [_vp, _vp, _i, _i, _vp, _f, _i, _vp, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
    check(lib.mbd_debug_elites_host(np_ptr(rews), np_ptr(cand), N, HNu, np_ptr(ybar), float(sigma), int(bool(lazy)),
                                    None if g is None else np_ptr(g), int(n_elites), int(nominal),
                                    np_ptr(E_in) if E_in.shape[0] else None, int(E_in.shape[0]), np_ptr(cand_out),
                                    *[np_ptr(o) for o in outs]))
    return _elites_result(int(n_elites), outs, cand_out)


def debug_elites_inject(cand, ybar, sigma, lazy, g, n_elites, nominal, E_in=None):
    """elite_inject_kernel alone on the device over ``cand`` [N, HNu]: the candidates behind the injection."""
    lib = load()
    cand, N, HNu, ybar, g, E_in = _elites_arrays(cand, ybar, g, n_elites, E_in)
    cand_out = np.zeros_like(cand)
    lib.mbd_debug_elites_inject.argtypes = [_vp, _i, _i, _vp, _f, _i, _vp, _i, _i, _vp, _i, _vp]
    check(lib.mbd_debug_elites_inject(np_ptr(cand), N, HNu, np_ptr(ybar), float(sigma), int(bool(lazy)),
                                      None if g is None else np_ptr(g), int(n_elites), int(nominal),
                                      np_ptr(E_in) if E_in.shape[0] else None, int(E_in.shape[0]), np_ptr(cand_out)))
    return cand_out


def debug_elites_select(rews, cand, ybar, sigma, lazy, n_elites, nominal, count_in=0):
    """elite_select_kernel alone on the device over ``rews`` [N] and ``cand`` [N, HNu]; ``count_in``: the count word it finds.
    Returns ``debug_elites_host``'s dict without ``cand``."""
    lib = load()
    cand, N, HNu, ybar, _, _ = _elites_arrays(cand, ybar, None, n_elites, None)
    rews = np.ascontiguousarray(rews, np.float32).reshape(N)
    outs = _elites_outputs(n_elites, HNu)
    lib.mbd_debug_elites_select.argtypes = [_vp, _vp, _i, _i, _vp, _f, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]
    check(lib.mbd_debug_elites_select(np_ptr(rews), np_ptr(cand), N, HNu, np_ptr(ybar), float(sigma), int(bool(lazy)), int(n_elites),
                                      int(nominal), int(count_in), *[np_ptr(o) for o in outs]))
    return _elites_result(int(n_elites), outs)


def debug_sweep_elites_step(rews, cand, ybar, sigma, lazy, g, n_elites, nominal, E_in, count_in, mask=0xffffffff) -> dict:
    """include/mbd_hip_debug.h: an elite record's two batch launches alone on the device for P plans — ``rews`` [P, N], ``cand``
    [P, N, HNu], ``ybar`` [P, HNu], ``E_in`` [P, max(n_elites, 1), HNu], ``count_in`` [P]; ``mask``: the plans that take part.
    Returns dict(cand, E [P, max(n_elites, 1), HNu], R, src [P, max(n_elites, 1)], count, kept, top [P]): what no kernel wrote has
    all bits set (``count``: ``count_in``)."""
    lib = load()
    cand = np.ascontiguousarray(cand, np.float32)
    P, N = cand.shape[:2]
    cand = cand.reshape(P, N, -1)
    HNu, k = cand.shape[2], max(int(n_elites), 1)
    rews = np.ascontiguousarray(rews, np.float32).reshape(P, N)
    ybar = np.ascontiguousarray(ybar, np.float32).reshape(P, HNu)
    g = None if g is None else np.ascontiguousarray(g, np.float32).reshape(HNu)
    E_in = np.ascontiguousarray(E_in, np.float32).reshape(P, k, HNu)
    count_in = np.ascontiguousarray(count_in, np.int32).reshape(P)
    cand_out, E, R, src = np.zeros_like(cand), np.zeros((P, k, HNu), np.float32), np.zeros((P, k), np.float32), np.zeros((P, k), np.int32)
    count, kept, top = np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros(P, np.float32)
    lib.mbd_debug_sweep_elites_step.argtypes = [_i, C.c_uint32, _vp, _vp, _i, _i, _vp, _f, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp,
                                                _vp, _vp, _vp, _vp]
    check(lib.mbd_debug_sweep_elites_step(P, int(mask) & 0xffffffff, np_ptr(rews), np_ptr(cand), N, HNu, np_ptr(ybar), float(sigma),
                                          int(bool(lazy)), None if g is None else np_ptr(g), int(n_elites), int(nominal), np_ptr(E_in),
                                          np_ptr(count_in), np_ptr(cand_out), np_ptr(E), np_ptr(R), np_ptr(src), np_ptr(count),
                                          np_ptr(kept), np_ptr(top)))
    return dict(cand=cand_out, E=E, R=R, src=src, count=count, kept=kept, top=top)


def debug_sweep_togo_step(temps, cand, ybar, rews, rewss, Nu: int, block: int, min_tail: int, lazy, sigma: float, std_guard,
                          alpha_i: float, alpha_bar_i: float, alpha_bar_im1: float, literal, n_groups: int) -> dict:
    """include/mbd_hip_debug.h: a to-go record's two batch launches alone on the device for P plans under ``temps`` [P] — ``cand``
    [P, N, H * Nu], ``ybar`` [P, H * Nu], ``rews`` [P, N], ``rewss`` [P, N, H].  Returns dict(ybar [P, H, Nu], R, W [P, G, N],
    rew_mean [P])."""
    lib = load()
    rewss = np.ascontiguousarray(rewss, np.float32)
    P, N, H = rewss.shape
    temps = np.ascontiguousarray(temps, np.float32).reshape(P)
    cand = np.ascontiguousarray(cand, np.float32).reshape(P, N, H * int(Nu))
    ybar = np.ascontiguousarray(ybar, np.float32).reshape(P, H * int(Nu))
    rews = np.ascontiguousarray(rews, np.float32).reshape(P, N)
    G = int(n_groups)
    out, R, W = np.zeros((P, H, int(Nu)), np.float32), np.zeros((P, G, N), np.float32), np.zeros((P, G, N), np.float32)
    mean = np.zeros(P, np.float32)
    lib.mbd_debug_sweep_togo_step.argtypes = [_i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _i, _f, _f, _f, _i, _vp, _vp,
                                              _vp, _vp]
    check(lib.mbd_debug_sweep_togo_step(P, np_ptr(temps), np_ptr(cand), np_ptr(ybar), np_ptr(rews), np_ptr(rewss), N, H, int(Nu),
                                        int(block), int(min_tail), int(bool(lazy)), float(sigma), int(bool(std_guard)), float(alpha_i),
                                        float(alpha_bar_i), float(alpha_bar_im1), int(bool(literal)), np_ptr(out), np_ptr(R), np_ptr(W),
                                        np_ptr(mean)))
    return dict(ybar=out, R=R, W=W, rew_mean=mean)


def peek_elites(fn, handle, n_elites: int, HNu: int, capacity: int = None) -> dict:
    """mbd_plan_peek_elites: {'E' [count, HNu], 'R' [count], 'src' [count], 'count', 'log_count' / 'log_kept' / 'log_top' [n],
    'steps'} — every step logged, or the most recent ``capacity``."""
    n = C.c_int(0)
    if capacity is None:
        check(fn(handle, None, None, None, None, None, None, None, 0, C.byref(n)))
        capacity = min(n.value, 65536)
    k, cap = max(int(n_elites), 1), max(int(capacity), 1)
    E, R, src, count = np.zeros((k, HNu), np.float32), np.zeros(k, np.float32), np.zeros(k, np.int32), np.zeros(1, np.int32)
    lc, lk, lt = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.float32)
    check(fn(handle, np_ptr(E), np_ptr(R), np_ptr(src), np_ptr(count), np_ptr(lc), np_ptr(lk), np_ptr(lt), int(capacity), C.byref(n)))
    m, c = min(n.value, int(capacity)), int(count[0])
    return {"E": E[:c], "R": R[:c], "src": src[:c], "count": c, "log_count": lc[:m], "log_kept": lk[:m], "log_top": lt[:m],
            "steps": n.value}


_ZONE_KINDS = {"out": ZONE_KEEP_OUT, "keep_out": ZONE_KEEP_OUT, "goal": ZONE_GOAL, ZONE_KEEP_OUT: ZONE_KEEP_OUT, ZONE_GOAL: ZONE_GOAL}


def zone_entry(kind, center, radius: float, margin: float, weight: float = 1.0, links=None, axes: str = "xyz") -> dict:
    """One entry of a zone record as a plain dict: ``kind`` "out" / "goal" (or the C constants), ``center`` [3], ``links`` None
    (every track slot), a bit mask, or a list of track slots or link names (names are resolved against the env by
    ``zones_record``); ``axes``: which coordinate differences count — "xyz" a sphere, "xy" a vertical cylinder, "x" a slab."""
    if kind not in _ZONE_KINDS:
        raise ValueError(f"zone: kind={kind!r}: 'out' or 'goal'")
    if not axes or any(a not in "xyz" for a in axes) or len(set(axes)) != len(axes):
        raise ValueError(f"zone: axes={axes!r}: a subset of 'xyz'")
    c = [float(v) for v in np.asarray(center, np.float64).reshape(-1)]
    if len(c) != 3:
        raise ValueError(f"zone: center has {len(c)} entries, expected 3")
    return dict(kind=_ZONE_KINDS[kind], center=c, scale=[1.0 if a in axes else 0.0 for a in "xyz"], radius=float(radius),
                margin=float(margin), weight=float(weight), links=links)


def zones_record(zones, n_track: int, track_names=None) -> "Zones":
    """The mbd_zones of ``Plan.set_zones``'s argument: a list of ``zone_entry`` dicts (a dict may carry ``scale`` [3] of its own).
    ``track_names``: the link names of the env's track slots, for entries whose ``links`` name links."""
    zones = list(zones)
    if not 1 <= len(zones) <= MAX_ZONES:
        raise ValueError(f"zones: {len(zones)} entries: must lie in 1..{MAX_ZONES}")
    rec = Zones()
    rec.n_zones = len(zones)
    for z, e in enumerate(zones):
        links = e.get("links")
        if links is None:
            mask = (1 << int(n_track)) - 1
        elif isinstance(links, (int, np.integer)):
            mask = int(links)
        else:
            mask = 0
            for l in links:
                if isinstance(l, str):
                    if track_names is None or l not in track_names:
                        raise ValueError(f"zones: zone[{z}].links: {l!r} is not a tracked link ({list(track_names or ())})")
                    l = list(track_names).index(l)
                if not 0 <= int(l) < 32:
                    raise ValueError(f"zones: zone[{z}].links: slot {l} outside [0, 32)")
                mask |= 1 << int(l)
        zn = rec.zone[z]
        zn.kind, zn.links = int(e["kind"]), mask & 0xffffffff
        for i in range(3):
            zn.center[i], zn.scale[i] = float(e["center"][i]), float(e["scale"][i])
        zn.radius, zn.margin, zn.weight = float(e["radius"]), float(e["margin"]), float(e["weight"])
    return rec


def debug_check_zones(rec: "Zones", n_track: int) -> int:
    """include/mbd_hip_debug.h: the refusals a zone record alone decides for an env of that n_track; the return code (the message:
    ``mbd_last_error``)."""
    lib = load()
    lib.mbd_debug_check_zones.argtypes = [C.POINTER(Zones), _i]
    return lib.mbd_debug_check_zones(None if rec is None else C.byref(rec), int(n_track))


def _debug_zones(fn, rec, xpos, rews):
    xpos = np.ascontiguousarray(xpos, np.float32)
    B, H, K = xpos.shape[:3]
    rews = None if rews is None else np.ascontiguousarray(rews, np.float32)
    out = dict(rews=np.full(B, np.nan, np.float32), pen=np.full(B, np.nan, np.float32), clr=np.full(B, np.nan, np.float32),
               step_pen=np.full((B, H), np.nan, np.float32), step_clr=np.full((B, H), np.nan, np.float32))
    fn.argtypes = [C.POINTER(Zones), _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]
    check(fn(C.byref(rec), np_ptr(xpos), None if rews is None else np_ptr(rews), B, H, K,
             None if rews is None else np_ptr(out["rews"]), np_ptr(out["pen"]), np_ptr(out["clr"]), np_ptr(out["step_pen"]),
             np_ptr(out["step_clr"])))
    if rews is None:
        del out["rews"]
    return out


def debug_zones_host(rec: "Zones", xpos, rews=None) -> dict:
    """include/mbd_hip_debug.h: a zone record's launch on the host (no device) over ``xpos`` [B, H, K, 3] and ``rews`` [B].
    Returns dict(rews, pen, clr [B], step_pen, step_clr [B, H])."""
    return _debug_zones(load().mbd_debug_zones_host, rec, xpos, rews)


def debug_zones_step(rec: "Zones", xpos, rews=None) -> dict:
    """include/mbd_hip_debug.h: zones_kernel alone on the device, on the same arguments as ``debug_zones_host``."""
    return _debug_zones(load().mbd_debug_zones_step, rec, xpos, rews)


def peek_zones(fn, handle, k, N: int) -> dict:
    """mbd_*_peek_zones: {'pen' [N], 'clr' [N]} of the last step (``k`` None: a plan)."""
    pen, clr = np.zeros(N, np.float32), np.zeros(N, np.float32)
    args = (handle,) if k is None else (handle, int(k))
    check(fn(*args, np_ptr(pen), np_ptr(clr)))
    return dict(pen=pen, clr=clr)


def togo_record(block: int = 1, min_tail: int = 1) -> "Togo":
    """The mbd_togo of ``Plan.set_togo``'s arguments."""
    rec = Togo()
    rec.block, rec.min_tail = int(block), int(min_tail)
    return rec


def debug_check_togo(rec: "Togo", Hsample: int, Nsample: int, update_method: int = 0, enable_demo: bool = False) -> int:
    """include/mbd_hip_debug.h: the refusals a to-go record alone decides for a plan of that Hsample, Nsample, update_method and
    enable_demo; the return code (the message: ``mbd_last_error``)."""
    lib = load()
    lib.mbd_debug_check_togo.argtypes = [C.POINTER(Togo), _i, _i, _i, _i]
    return lib.mbd_debug_check_togo(None if rec is None else C.byref(rec), int(Hsample), int(Nsample), int(update_method),
                                    int(bool(enable_demo)))


def debug_togo_host(rews, rewss, block: int, min_tail: int) -> dict:
    """include/mbd_hip_debug.h: a to-go record's group layout and returns on the host (no device) from ``rews`` [N] and ``rewss``
    [N, H].  Returns dict(starts [G], R [G, N])."""
    lib = load()
    rewss = np.ascontiguousarray(rewss, np.float32)
    N, H = rewss.shape
    rews = np.ascontiguousarray(rews, np.float32).reshape(N)
    starts, R, G = np.full(H, -1, np.int32), np.zeros((H, N), np.float32), C.c_int32(0)
    lib.mbd_debug_togo_host.argtypes = [_vp, _vp, _i, _i, _i, _i, _vp, _vp, C.POINTER(C.c_int32)]
    check(lib.mbd_debug_togo_host(np_ptr(rews), np_ptr(rewss), N, H, int(block), int(min_tail), np_ptr(starts), np_ptr(R), C.byref(G)))
    return dict(starts=starts[:G.value].copy(), R=R.reshape(-1)[:G.value * N].reshape(G.value, N).copy())


def debug_togo_layout(H: int, block: int, min_tail: int) -> np.ndarray:
    """The group starts alone (``mbd_debug_togo_host`` without rewards; no device)."""
    lib = load()
    starts, G = np.full(max(int(H), 1), -1, np.int32), C.c_int32(0)
    lib.mbd_debug_togo_host.argtypes = [_vp, _vp, _i, _i, _i, _i, _vp, _vp, C.POINTER(C.c_int32)]
    check(lib.mbd_debug_togo_host(None, None, 1, int(H), int(block), int(min_tail), np_ptr(starts), None, C.byref(G)))
    return starts[:G.value].copy()


def debug_togo_step(cand, ybar, rews, rewss, Nu: int, block: int, min_tail: int, lazy, sigma: float, temp: float, std_guard,
                    alpha_i: float, alpha_bar_i: float, alpha_bar_im1: float, literal, n_groups: int) -> dict:
    """include/mbd_hip_debug.h: the step's two launches alone on the device over ``cand`` [N, H * Nu] (values, or with ``lazy``
    normals), ``ybar`` [H * Nu], ``rews`` [N] and ``rewss`` [N, H]; ``n_groups``: the layout's G (``debug_togo_layout``).  Returns
    dict(ybar [H, Nu], R, W [G, N], rew_mean)."""
    lib = load()
    rewss = np.ascontiguousarray(rewss, np.float32)
    N, H = rewss.shape
    cand = np.ascontiguousarray(cand, np.float32).reshape(N, H * int(Nu))
    ybar = np.ascontiguousarray(ybar, np.float32).reshape(H * int(Nu))
    rews = np.ascontiguousarray(rews, np.float32).reshape(N)
    G = int(n_groups)
    out, R, W, mean = np.zeros((H, int(Nu)), np.float32), np.zeros((G, N), np.float32), np.zeros((G, N), np.float32), np.zeros(1, np.float32)
    lib.mbd_debug_togo_step.argtypes = [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _f, _i, _f, _f, _f, _i, _vp, _vp, _vp, _vp]
    check(lib.mbd_debug_togo_step(np_ptr(cand), np_ptr(ybar), np_ptr(rews), np_ptr(rewss), N, H, int(Nu), int(block), int(min_tail),
                                  int(bool(lazy)), float(sigma), float(temp), int(bool(std_guard)), float(alpha_i), float(alpha_bar_i),
                                  float(alpha_bar_im1), int(bool(literal)), np_ptr(out), np_ptr(R), np_ptr(W), np_ptr(mean)))
    return dict(ybar=out, R=R, W=W, rew_mean=mean[0])


def peek_togo(fn, handle, H: int, N: int) -> dict:
    """mbd_plan_peek_togo: {'starts' [G], 'R' [G, N], 'W' [G, N]} of the last step."""
    G = C.c_int32(0)
    check(fn(handle, None, None, None, C.byref(G)))
    g = G.value
    starts, R, W = np.zeros(g, np.int32), np.zeros((g, N), np.float32), np.zeros((g, N), np.float32)
    check(fn(handle, np_ptr(starts), np_ptr(R), np_ptr(W), C.byref(G)))
    return {"starts": starts, "R": R, "W": W}


def pick_record(mean=True, prev=True, best=True) -> "MpcPick":
    """The mbd_mpc_pick of ``set_mpc_pick``'s arguments (none enabled goes to the library, which names the field)."""
    rec = MpcPick()
    rec.candidates = (PICK_MEAN if mean else 0) | (PICK_PREV if prev else 0) | (PICK_BEST if best else 0)
    return rec


def peek_mpc_pick(fn, handle, k, capacity: int = None) -> dict:
    """mbd_plan_peek_mpc_pick (k None) or mbd_sweep_peek_mpc_pick: {'choice' [n], 'rets' [n, 3], 'best' [n]}, one entry per tick —
    every tick served so far, or the most recent ``capacity`` of them, oldest first."""
    head = (handle,) if k is None else (handle, int(k))
    n = C.c_int(0)
    if capacity is None:
        check(fn(*head, None, None, None, 0, C.byref(n)))
        capacity = n.value
    capacity = max(int(capacity), 0)
    choice, rets, best = np.zeros(capacity, np.int32), np.zeros((capacity, 3), np.float32), np.zeros(capacity, np.int32)
    check(fn(*head, np_ptr(choice), np_ptr(rets), np_ptr(best), capacity, C.byref(n)))
    m = min(n.value, capacity)
    return {"choice": choice[:m], "rets": rets[:m], "best": best[:m]}


def has_mpc_pick(fn, handle, k) -> bool:
    """Whether the handle carries a pick record: the peek call's own answer (MBD_ERR_STATE: none)."""
    head = (handle,) if k is None else (handle, int(k))
    rc = fn(*head, None, None, None, 0, None)
    if rc == MBD_ERR_STATE:
        return False
    check(rc)
    return True


def debug_pick_best(rews) -> np.ndarray:
    """include/mbd_hip_debug.h: the pick record's argmax on the GPU.  ``rews`` [P, N] (or [N]); returns best [P] (or an int)."""
    lib = load()
    lib.mbd_debug_pick_best.argtypes = [_vp, _i, _i, _vp]
    r = np.ascontiguousarray(rews, np.float32)
    r2 = r.reshape(1, -1) if r.ndim == 1 else r
    best = np.full(r2.shape[0], -2, np.int32)
    check(lib.mbd_debug_pick_best(np_ptr(r2), r2.shape[0], r2.shape[1], np_ptr(best)))
    return int(best[0]) if r.ndim == 1 else best


RING_READ_ARGTYPES = [_vp, _i, C.c_longlong, C.c_longlong, C.c_longlong, _vp]


def debug_ring_read(ring, count: int, n: int) -> np.ndarray:
    """include/mbd_hip_debug.h: the device logs' reader alone on the GPU.  ``ring`` [cap, width] float32 or int32 (the dtype chooses
    the instantiation), a log that has seen ``count`` entries; returns the most recent min(n, count, cap) of them [m, width],
    oldest first.  What the reader did not write keeps all bits set."""
    lib = load()
    ring = np.ascontiguousarray(ring)
    if ring.dtype not in (np.float32, np.int32) or ring.ndim != 2:
        raise ValueError(f"ring of dtype {ring.dtype} and shape {ring.shape}: [cap, width] float32 or int32")
    fn = lib.mbd_debug_ring_read if ring.dtype == np.float32 else lib.mbd_debug_ring_read_i32
    fn.argtypes = RING_READ_ARGTYPES
    cap, width = ring.shape
    m = max(min(int(n), int(count), cap), 0)
    out = np.zeros((max(m, 1), width), ring.dtype)  # (room for one element where nothing is read: the entry refuses NULL)
    check(fn(np_ptr(ring), width, cap, int(count), int(n), np_ptr(out)))
    return out[:m]


SWEEP_UPDATE_ARGTYPES = [_vp, _i] + [_vp] * 10


def debug_sweep_update(handle, i: int, cand, ybar, rews, lp=None, sigma_in=None, sigma: bool = False, idx: bool = False) -> dict:
    """include/mbd_hip_debug.h: the update step of a sweep (``Sweep.h``) alone on uploaded arrays.  ``cand`` [P, N, H, Nu] (MBD
    sweeps: the normals), ``ybar`` [P, H, Nu], ``rews`` [P, N], ``lp`` [P, N] (demo sweeps), ``sigma_in`` [P] (cma-es).  Returns
    {'ybar' [P, H, Nu], 'weights' [P, N], 'rew_mean' [P]} and, asked for, 'sigma' [P] (cma-es) and 'idx' [P, min(N, 10)] (cem);
    every output starts as NaN (idx: -2), so one the library did not write shows."""
    lib = load()
    lib.mbd_debug_sweep_update.argtypes = SWEEP_UPDATE_ARGTYPES
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    cand, ybar, rews, lp, sigma_in = f32(cand), f32(ybar), f32(rews), f32(lp), f32(sigma_in)
    P, N = rews.shape
    assert cand.size == P * N * (ybar.size // P) and ybar.shape[0] == P, (cand.shape, ybar.shape, rews.shape)
    out = {"ybar": np.full(ybar.shape, np.nan, np.float32), "weights": np.full((P, N), np.nan, np.float32),
           "rew_mean": np.full(P, np.nan, np.float32)}
    if sigma:
        out["sigma"] = np.full(P, np.nan, np.float32)
    if idx:
        out["idx"] = np.full((P, min(N, 10)), -2, np.int32)
    opt = lambda a: None if a is None else np_ptr(a)
    check(lib.mbd_debug_sweep_update(handle, int(i), np_ptr(cand), np_ptr(ybar), np_ptr(rews), opt(lp), opt(sigma_in),
                                     np_ptr(out["ybar"]), np_ptr(out["weights"]), np_ptr(out["rew_mean"]), opt(out.get("sigma")),
                                     opt(out.get("idx"))))
    return out


def debug_math_ops() -> list:
    """include/mbd_hip_debug.h: the names of the primitives mbd_debug_eval_math evaluates."""
    lib = load()
    lib.mbd_debug_math_name.argtypes = [_i]
    lib.mbd_debug_math_name.restype = C.c_char_p
    names, k = [], 0
    while (n := lib.mbd_debug_math_name(k)) is not None:
        names.append(n.decode())
        k += 1
    return names


def debug_math_arity(op: str) -> tuple:
    """(inputs, outputs) per element of primitive `op` — no device needed."""
    lib = load()
    lib.mbd_debug_math_arity.argtypes = [C.c_char_p, C.POINTER(_i), C.POINTER(_i)]
    k_in, k_out = _i(0), _i(0)
    check(lib.mbd_debug_math_arity(op.encode(), C.byref(k_in), C.byref(k_out)))
    return k_in.value, k_out.value


def debug_eval_math(op: str, x) -> np.ndarray:
    """include/mbd_hip_debug.h: primitive `op` of csrc/mbd_math.h on the GPU, one thread per row of x ([n][k_in] float32,
    or [n] when k_in = 1); returns [n][k_out] ([n] when k_out = 1)."""
    lib = load()
    k_in, k_out = debug_math_arity(op)
    x = np.ascontiguousarray(x, np.float32).reshape(-1, k_in)
    out = np.empty((x.shape[0], k_out), np.float32)
    lib.mbd_debug_eval_math.argtypes = [C.c_char_p, C.c_longlong, _vp, _vp]
    check(lib.mbd_debug_eval_math(op.encode(), x.shape[0], x.ctypes.data, out.ctypes.data))
    return out[:, 0] if k_out == 1 else out


def check(rc: int) -> None:
    if rc != MBD_OK:
        raise MbdError(rc, load().mbd_last_error().decode())


def device_count() -> int:
    n = _i(0)
    check(load().mbd_device_count(C.byref(n)))
    return n.value


def key_array(key) -> "C.Array":
    k = np.ascontiguousarray(key, np.uint32).reshape(2)
    return (C.c_uint32 * 2)(int(k[0]), int(k[1]))


def prng_key(seed: int) -> np.ndarray:
    out = (C.c_uint32 * 2)()
    check(load().mbd_prng_key(int(seed), out))
    return np.array([out[0], out[1]], np.uint32)


def prng_split(key, num: int = 2, impl: int = PRNG_PARTITIONABLE) -> np.ndarray:
    out = (C.c_uint32 * (2 * num))()
    check(load().mbd_prng_split(key_array(key), num, impl, out))
    return np.array(list(out), np.uint32).reshape(num, 2)


def np_ptr(a: np.ndarray):
    return a.ctypes.data_as(_vp)
