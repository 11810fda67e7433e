"""Receding-horizon control on top of the planner (include/mbd_hip.h mbd_plan_run_mpc):
every control tick replans from the state the system reached, warm-started from the previous tick's plan, and executes the
first ``exec_steps`` rows of the new one — the whole episode on the device.  The reference plans open loop only
(mbd_planner.py); the reset and the episode key follow its seed chain (:40,79,150), so tick 0 is ``run_diffusion``'s plan.

    python -m mbd_hip.planners.mpc --env_name hopper --n_ticks 100 --warm_steps 20

prints one JSON line (timings of a second episode, after a warm-up one in the same process).  ``--n_episodes P`` runs the
seeds ``seed .. seed+P-1`` as ONE batch of lockstep episodes (mbd_sweep_run_mpc; ``run_mpc_batch``): a diffusion step of a tick
is one rollout launch over all the episodes' candidates, and every episode is the single one bit for bit.

The system need not be the model (include/mbd_hip.h mbd_mpc_plant; DESIGN.md section 1 "N5 plant"): ``--plant_mass``,
``--plant_friction``, ``--plant_gear`` execute the rows on a copy of the env whose links are that many times as heavy, whose
contact friction and actuator gears are multiplied (``Model.scaled``); ``--act_noise_std`` adds normal noise to every executed
action, ``--kick_std`` / ``--kick_every`` shove link 0 after every kick_every-th tick.  The disturbances are drawn on the device
from ``prng_key(disturb_seed)`` — that key as it is, folded with nothing else: episodes of different ``seed`` share their
disturbance chain unless ``disturb_seed`` differs too (the episodes of ``--n_episodes P`` all do: one noise realisation).  The planner keeps planning with the unperturbed model.  With every one
of these at its default no plant record is set at all and the JSON line is what it always was; with a record it also carries
the plant settings and ``nominal_episode_reward``: the same episode without the record, run in the same process.

    python -m mbd_hip.planners.mpc --env_name hopper --n_ticks 100 --plant_mass 1.3 --act_noise_std 0.2 --n_episodes 8

The planner can answer a wrong model with an ensemble (include/mbd_hip.h mbd_ensemble; DESIGN.md section 1 "N6 ensemble"):
``--ens_mass``, ``--ens_friction``, ``--ens_gear`` take comma lists, zipped into members (a single value broadcasts, an absent
list is all 1); member m is the env's model scaled by the m-th triple (``Model.scaled``), and every candidate is scored by its
mean — ``--ens_risk min``: its worst — return over the members.  Single episodes only.  With plant flags as well,
``nominal_episode_reward`` is the episode of the SAME planner — ensemble included — without the plant record: what the plant's
mismatch and disturbances cost that planner, not what the ensemble buys.

    python -m mbd_hip.planners.mpc --env_name hopper --plant_mass 1.25 --ens_mass 0.8,1,1.25,1.5 --ens_risk min

A warm tick restarts every row of the shifted mean at one sigma_K — the rows the shift has just appended, never optimised,
as much as the head rows refined over many ticks.  A noise shape (include/mbd_hip.h mbd_noise_shape; DESIGN.md section 1 "N7
noise shape") scales the sampling noise per horizon row and actuator: ``--tail_rows R --tail_sigma S`` ramp the last R rows
up to S times sigma_K (``tail_shape``) in the ticks t >= 1 only, so tick 0 stays ``run_diffusion``'s plan;
``--noise_shape FILE.npy`` loads a table [Hsample, Nu] (or anything that broadcasts to it, e.g. one value per actuator) that
is in force in every step, tick 0 included.  One or the other; a batch of episodes shares it.

    python -m mbd_hip.planners.mpc --env_name hopper --warm_steps 20 --tail_rows 5 --tail_sigma 4

The sampling noise is white along the horizon: Hsample independent normals per actuator, which the body low-pass filters.  A
noise basis (include/mbd_hip.h mbd_noise_basis; DESIGN.md section 1 "N8 noise basis") draws ``--noise_knots K`` normals per
actuator instead and spreads them over the rows (``knot_basis``): ``--noise_interp linear`` interpolates between K knots,
``hold`` keeps each for Hsample / K rows; every row keeps the variance sigma_i^2.  In force in every step, tick 0 included,
and composable with the tail ramp, which then scales the correlated noise.

    python -m mbd_hip.planners.mpc --env_name humanoidrun --warm_steps 20 --noise_knots 10 --noise_interp linear

Planning takes time.  ``--delay_ticks D`` (include/mbd_hip.h mbd_mpc_delay; DESIGN.md section 1 "N9 delay") runs the episode the
way a real-time controller has to: the plan made in tick t is first executed in tick t + D; meanwhile the system executes the
rows it is already committed to (zeros when the episode starts) and every tick plans from the state the planner's own model
predicts those rows will reach.  0, the default, sets no record.  It composes with ``--n_episodes`` (one D for the batch) and
with every plant, ensemble and noise flag; the saved episode then carries the predicted states.

    python -m mbd_hip.planners.mpc --env_name humanoidrun --warm_steps 20 --delay_ticks 1 --plant_mass 1.3

Every plan maximises the unweighted mean of the env's per-step rewards.  An objective record (include/mbd_hip.h mbd_objective;
DESIGN.md section 1 "N13 objective") shapes that: ``--discount G --terminal_weight W`` weigh horizon row h by G ** h and the last
row W times that (``discount_weights``); ``--effort_cost L`` and ``--rate_cost L`` subtract the controller's own costs on a
candidate's squared actions and on its squared step-to-step differences, the first difference taken against the last row the
previous tick committed — what keeps a replanning sampler from chattering; ``--act_weight FILE.npy`` weighs the two costs per
actuator.  With any of them the report gains ``action_rate``, the executed rows' mean squared step-to-step difference.  The
episode's rewards stay the env's own.

    python -m mbd_hip.planners.mpc --env_name hopper --warm_steps 20 --discount 0.98 --rate_cost 0.1

A plan scores its Hsample rows and nothing beyond them.  A value record (include/mbd_hip.h mbd_value; DESIGN.md section 1 "N16
value") adds what the state a candidate ends in is worth: ``--value FILE.npz`` loads a terminal value net over the state record
(``planners.value.ValueNet.save``; ``python -m mbd_hip.scripts.fit_value`` fits one to logged episodes) and ``--value_scale X`` lets
its V weigh like X further reward rows (the record's scale is X / Hsample).  With ``--value`` the report gains ``value`` and
``value_scale``; the episode's rewards stay the env's own.

    python -m mbd_hip.planners.mpc --env_name hopper --warm_steps 20 --Hsample 25 --value value.npz --value_scale 0.25

Every step weighs its candidates by a softmax of their standardised rewards at the env's ``temp_sample``, and one candidate whose
reward is NaN or infinite makes every weight NaN.  A weighting record (include/mbd_hip.h mbd_weighting; DESIGN.md section 1 "N14
weighting") changes both: ``--reject_nonfinite`` leaves such candidates out of the step, and ``--ess_frac F --temp_min A --temp_max
B --ess_iters I`` lets every step choose its temperature inside [A, B] by I bisection steps so that the effective sample size of
the weights is F times the candidates kept.  With either the report gains ``weighting_last_tick``: the temperature used, the ESS
and the kept count of each diffusion step of the LAST tick, which is what the device keeps of an episode it runs on its own; with
``--online``, where the script sees every tick, it gains ``weighting`` instead: one entry per tick, its last step's.

    python -m mbd_hip.planners.mpc --env_name hopper --warm_steps 20 --reject_nonfinite --ess_frac 0.25

Every tick hands on its new mean, which nobody has rolled out.  ``--pick mean,prev,best`` (any non-empty subset; include/mbd_hip.h
mbd_mpc_pick; DESIGN.md section 1 "N15 pick") evaluates the mean, the incumbent — the last tick's plan, shifted — and the best
candidate of the tick's last step on the planner's model and hands on the best of those named: the rows executed, the next tick's
warm start and ``means`` are the picked plan's.  ``--pick mean`` leaves the episode's bits alone and logs the value of every executed
plan.  The details gain ``pick`` = dict(choice, rets, best) per tick, the report ``pick_log``: the share of ticks per choice and the
mean value of the picked plan and of the mean.  ``--online`` and ``--n_episodes`` honour it.

    python -m mbd_hip.planners.mpc --env_name hopper --warm_steps 20 --pick mean,prev,best

The noise every step samples with has one shape: flat, or what ``--noise_shape`` / ``--tail_rows`` fix in advance.  An adapt record
(include/mbd_hip.h mbd_adapt; DESIGN.md section 1 "N17 adapt") lets the plan learn it: ``--adapt_rate R`` (0 < R <= 1) keeps a table
per horizon row and actuator, all ones at the start, which every diffusion step moves by R towards where the weighted spread of its
candidates says the noise should go — narrower where selection narrowed them more than on average, wider elsewhere —, every entry
within [``--adapt_min``, ``--adapt_max``]; the steps sample under the table times the noise shape in force.  ``--adapt_carry``
shifts the table across a tick boundary with the mean (otherwise every tick starts from ones).  MBD and mppi plans, single
episodes; ``--online`` honours it.  The details gain ``adapt`` = dict(a, ratio, skipped, count): the table behind the episode and
the log of its steps; the report ``adapt_table_min`` / ``adapt_table_max`` and ``adapt_steps_skipped``.

    python -m mbd_hip.planners.mpc --env_name hopper --warm_steps 20 --adapt_rate 0.3 --adapt_carry

Every step draws its candidates afresh and keeps only their weighted mean.  An elite record (include/mbd_hip.h mbd_elites; DESIGN.md
section 1 "N18 elites") carries candidates over: ``--elites K`` (0 to 32) makes the K best candidates of every diffusion step
candidates of the next one, ``--elite_nominal`` makes candidate 0 of every step the step's mean itself, noise-free, and
``--elite_carry`` shifts the elites across a tick boundary with the mean (otherwise every tick starts without elites).  MBD and mppi
plans; ``--online`` and ``--n_episodes`` honour it (one record for the batch; every episode has its own elites and log, and the
report's two fields then hold one list per episode).  The details gain ``elite_log`` = dict(E, R, src, count, log_count, log_kept,
log_top, steps): the elites behind the episode and the log of its steps; the report ``elites_kept`` and ``elites_top``, per tick the number of
selected candidates that had been injected (summed over the tick's steps) and the best return of the tick's last step.

    python -m mbd_hip.planners.mpc --env_name hopper --warm_steps 20 --elites 4 --elite_nominal --elite_carry

Every update weighs a candidate once: its whole return multiplies all its horizon rows, so the noise it drew in a late row is
credited with rewards of earlier rows it cannot have caused.  A to-go record (include/mbd_hip.h mbd_togo; DESIGN.md section 1 "N19
to-go") weighs a row by the return still ahead of it, the to-go return of PI^2: ``--togo_block B`` groups the rows B at a time and
updates each group under weights from the candidates' mean reward from the group's first row onwards; ``--togo_min_tail M`` starts a
group only where at least M rows are still ahead (the last group takes the rest).  There is no record unless ``--togo_block`` is
given.  MBD and mppi plans; ``--online`` and ``--n_episodes`` honour it (one record for the batch); not beside the objective, value, weighting, adapt or ensemble
flags.  The report gains ``togo_groups``, the groups' first rows.

    python -m mbd_hip.planners.mpc --env_name hopper --warm_steps 20 --togo_block 5 --togo_min_tail 10

None of the above says where the body may go.  A zone record (include/mbd_hip.h mbd_zones; DESIGN.md section 1 "N20 zones") does:
``--zone_links torso,left_shin`` retracks the built-in model (``get_env(name, track=...)``) so that the rollouts return those links'
world positions, and ``--zones`` lists keep-out regions and goals for them, ';' between entries, each
``kind:cx,cy,cz:radius:margin[:weight[:axes[:links]]]`` — kind ``out`` (a cost inside radius + margin, rising to ``weight`` at the
surface) or ``goal`` (a cost outside radius, rising to ``weight`` at radius + margin); axes a subset of ``xyz`` (``xy``: a vertical
cylinder, or a point goal on the ground plane); links a comma list of the tracked links the entry applies to (default: all).  Every
step subtracts the horizon mean of the penalties from each candidate's reward.  ``--online`` and ``--n_episodes`` honour the flags
(one record for the batch).  The report gains ``zone_pen_mean``, ``zone_clear_min`` and ``zone_hits`` — the executed control steps'
mean penalty, smallest keep-out clearance and the number of them inside a keep-out region; the saved episode ``zone_pen`` and
``zone_clear``.  The logged rewards stay the env's.

    python -m mbd_hip.planners.mpc --env_name humanoidrun --zone_links torso --zones "out:2,0,1:0.3:0.3:5;goal:6,0,1.2:0.2:6:1:xy"

A demo plan (``--enable_demo``) compares its 50 planned steps with the env's 50 demo rows; in an episode the demo has to move
with the system.  ``--demo_clip env|FILE.npy`` (include/mbd_hip.h mbd_mpc_demo; DESIGN.md section 1 "N10 demo clock") sets the
clip the episode follows — the env's own demo, or an array [n_track, L, 3] (car2d: [L, 2]) — and ``--demo_start c0`` the clip
row of the episode's first control step: tick t plans under the 50 rows from c0 + (t + delay_ticks) exec_steps on, rows past
the clip's end holding its last row.  ``--demo_period p`` first extends the clip periodically (``cycle_clip``) to the rows the
episode reaches, so that a long episode follows a gait that keeps moving instead of a pose frozen in world x.  The JSON line
then carries ``track_err_mean``, the mean distance of the executed steps' tracked positions from their clip rows; the saved
episode carries ``track_err`` and ``demo_windows``.  ``--enable_demo`` without a clip stays refused: an episode has no clock for
the env's 50 rows.  A batch of episodes shares one clip and one clock.

    python -m mbd_hip.planners.mpc --env_name humanoidtrack --enable_demo --demo_clip env --demo_period 20 --n_ticks 200

All of the above runs the whole episode in one call, on a plant the library owns.  ``--online`` (include/mbd_hip.h
mbd_plan_mpc_open; DESIGN.md section 1 "N11 session") runs it the way a user with a system of their own would: a session, one
``tick`` per control tick, with this script as the plant — ``env.rollout`` of the rows to execute, on the ``--plant_mass`` /
``--plant_friction`` / ``--plant_gear`` env if one is given — handing the state reached back to the next tick.  It saves the
episode (results/<env>/mpc_episode.npz) with the fields of the batch run and equal contents; its JSON line is its own — the ms per
tick the session itself took (the plant excluded), tick 0 and the warm ticks' min / median / max.
``--act_noise_std`` and ``--kick_std`` are refused with it: those are drawn by the plant record, and a session has none.  With a
demo clip the distances from the clip are not logged (a session executes nothing on the device).  Single episodes only.

    python -m mbd_hip.planners.mpc --env_name hopper --n_ticks 100 --warm_steps 20 --online --plant_mass 1.3

The controller need not be MBD.  ``--update_method mppi|cma-es|cem`` (include/mbd_hip.h mbd_mpc_sigma; DESIGN.md section 1 "N12
path-integral episodes") runs the reference's path-integral baselines (path_integral.py) as the planning loop of the same
episode — same plant, seeds, delay, mismatch and noise flags: a tick is ``warm_steps`` refinements (tick 0: Ndiffuse - 1) from the
shifted mean.  ``--sigma_cold`` is the sampling sigma tick 0 starts from (1.0: the reference's), ``--sigma_warm`` what every later
tick starts from; ``--sigma_gain G`` > 0 (cma-es only, whose sigma shrinks as it converges) starts a warm tick from
clamp(G * the sigma the last tick ended with, sigma_warm, sigma_cold) instead.  ``--n_episodes`` and ``--online`` work as for MBD;
ensembles and demos do not apply, and ``--online`` with ``--n_episodes`` > 1 ends with the library's refusal (sessions of
path-integral sweeps are not supported).  The JSON line and the saved episode then carry the settings and the ticks' ``sigmas``.

    python -m mbd_hip.planners.mpc --env_name hopper --n_ticks 100 --warm_steps 20 --update_method mppi --sigma_warm 0.25
"""
from __future__ import annotations

import os
from dataclasses import dataclass

import numpy as np

from .. import _capi
from ..envs import get_env
from ..envs.base import prng_impl
from .mbd_planner import Args, Plan, Sweep, apply_recommended
from .path_integral import UPDATE_METHODS as _PI_METHODS

UPDATE_METHODS = dict(mbd=0, **_PI_METHODS)  # mbd_plan_config.update_method

MAX_EPISODES = 32  # include/mbd_hip.h MBD_SWEEP_MAX_PLANS


@dataclass
class MpcArgs(Args):
    n_ticks: int = 50  # control ticks T of the episode
    warm_steps: int = 20  # diffusion steps K..1 of every tick after the first (the noise level it restarts from: sigma_K)
    exec_steps: int = 1  # control steps E executed per tick; the plan then shifts by E rows
    plant_mass: float = 1.0  # the plant's links are this many times as heavy as the model's
    plant_friction: float = 1.0  # the plant's contact friction, as a multiple of the model's
    plant_gear: float = 1.0  # the plant's actuator gears, as a multiple of the model's
    act_noise_std: float = 0.0  # std of the normal noise added to every executed action (before the env's clip)
    kick_std: float = 0.0  # std per component (m/s) of the velocity kick on link 0 ...
    kick_every: int = 1  # ... at the end of every kick_every-th tick
    disturb_seed: int = 0  # the disturbance key is prng_key(disturb_seed), folded with nothing else
    ens_mass: str = ""  # comma list: the ensemble members' link masses, as multiples of the model's
    ens_friction: str = ""  # ... their contact friction
    ens_gear: str = ""  # ... their actuator gears (the three lists are zipped; a single value broadcasts)
    ens_risk: str = "mean"  # a candidate's reward over the members: "mean" or "min"
    tail_rows: int = 0  # the last tail_rows horizon rows of every warm tick (t >= 1) sample with more noise ...
    tail_sigma: float = 1.0  # ... ramping up to tail_sigma times sigma_K at the last row (tail_shape)
    noise_shape: str = ""  # FILE.npy: a noise shape [Hsample, Nu] (or what broadcasts to it) in force in every step
    noise_knots: int = 0  # 0: white noise along the horizon; K: K knot normals per actuator in every step (knot_basis) ...
    noise_interp: str = "linear"  # ... interpolated between the knots ("linear") or held ("hold")
    delay_ticks: int = 0  # 0: plans are executed in the tick that made them; D: D ticks later, planned from a predicted state
    demo_clip: str = ""  # "": no demo record; "env": the env's own demo; FILE.npy: a clip [n_track, L, 3] (car2d [L, 2])
    demo_start: int = 0  # c0: the clip row the episode's first executed control step is compared with
    demo_period: int = 0  # p > 0: the clip is first extended periodically (cycle_clip) to the rows the episode reaches
    online: bool = False  # run the episode through a session (Plan.mpc_open), one tick per call, this script being the plant
    update_method: str = "mbd"  # the planning loop of a tick: "mbd", or the path-integral baselines "mppi", "cma-es", "cem"
    sigma_cold: float = 1.0  # path-integral methods: the sampling sigma tick 0 starts from (1.0: path_integral.py:131) ...
    sigma_warm: float = 1.0  # ... and every later tick,
    sigma_gain: float = 0.0  # or with G > 0 (cma-es only) clamp(G * the sigma the last tick ended with, sigma_warm, sigma_cold)
    discount: float = 1.0  # gamma: horizon row h of a plan weighs gamma ** h in what the plan maximises (discount_weights) ...
    terminal_weight: float = 1.0  # ... and the last row this many times that
    effort_cost: float = 0.0  # lambda_u: the controller's own cost on sum_h u^2 of a candidate (mbd_objective) ...
    rate_cost: float = 0.0  # ... lambda_du on sum_h (u_h - u_{h-1})^2, u_{-1} the last row committed before the plan begins
    act_weight: str = ""  # FILE.npy: the two costs' weights per actuator [Nu]
    reject_nonfinite: bool = False  # candidates whose reward is NaN or infinite get weight 0 and leave the statistics (mbd_weighting)
    ess_frac: float = 0.0  # F > 0: every step chooses its temperature so that the effective sample size is F times the candidates kept ...
    temp_min: float = 0.01  # ... inside [temp_min, temp_max] ...
    temp_max: float = 10.0
    ess_iters: int = 12  # ... by this many bisection steps
    pick: str = ""  # "mean,prev,best" or any non-empty subset: what a tick may hand on (mbd_mpc_pick); "": the mean, nothing evaluated
    value: str = ""  # FILE.npz: a terminal value net (planners.value.ValueNet.save; scripts.fit_value) over the state record ...
    value_scale: float = 1.0  # ... whose V at a candidate's final state weighs like this many further reward rows (scale = X / Hsample)
    adapt_rate: float = 0.0  # R > 0: an adapt record (mbd_adapt) — every step moves the noise table by R towards its target ...
    adapt_min: float = 0.25  # ... every entry within [adapt_min, adapt_max];
    adapt_max: float = 4.0
    adapt_carry: bool = False  # the table is shifted across a tick boundary with the mean (default: every tick starts from ones)
    elites: int = 0  # K > 0: an elite record (mbd_elites) — the K best candidates of a step are candidates of the next one ...
    elite_nominal: bool = False  # ... candidate 0 of every step is the step's mean itself (with --elites 0: the record is this alone)
    elite_carry: bool = False  # ... and a tick boundary shifts the elites with the mean (default: every tick starts without elites)
    togo_block: int = 0  # B > 0: a to-go record (mbd_togo) — the horizon's rows in groups of B, each under weights from the return ahead ...
    togo_min_tail: int = 1  # ... a group starting only where at least this many rows are still ahead
    zones: str = ""  # "kind:cx,cy,cz:radius:margin[:weight[:axes[:links]]];...": a zone record (mbd_zones) for the tracked links ...
    zone_links: str = ""  # ... comma list of link names or positions the built-in model is retracked to (get_env's track)


def zone(kind, center, radius: float, margin: float, weight: float = 1.0, links=None, axes: str = "xyz") -> dict:
    """One entry of a zone record (``Plan.set_zones``, include/mbd_hip.h mbd_zone): ``kind`` "out" — a keep-out region: a
    tracked link nearer than ``radius + margin`` to ``center`` costs ``weight * clip((radius + margin - d) / margin, 0, 1) ** 2``
    per step — or "goal": ``weight * clip((d - radius) / margin, 0, 1) ** 2``.  ``axes`` says which coordinate differences the
    distance d is taken over ("xyz" a sphere, "xy" a vertical cylinder or a point goal on the ground plane, "x" a slab);
    ``links`` which tracked links the entry applies to — None: all, else a list of track slots or link names, or a bit mask."""
    return _capi.zone_entry(kind, center, radius, margin, weight, links, axes)


def parse_zones(text: str) -> list:
    """The entries of ``--zones``: ';' between entries, each ``kind:cx,cy,cz:radius:margin[:weight[:axes[:links]]]``."""
    out = []
    for k, item in enumerate(x for x in text.split(";") if x.strip()):
        f = [x.strip() for x in item.split(":")]
        if not 4 <= len(f) <= 7:
            raise ValueError(f"zones: entry {k} {item!r}: kind:cx,cy,cz:radius:margin[:weight[:axes[:links]]]")
        try:
            center = [float(x) for x in f[1].split(",")]
            radius, margin = float(f[2]), float(f[3])
            weight = float(f[4]) if len(f) > 4 and f[4] else 1.0
        except ValueError:
            raise ValueError(f"zones: entry {k} {item!r}: center, radius, margin and weight are numbers") from None
        axes = f[5] if len(f) > 5 and f[5] else "xyz"
        links = None
        if len(f) > 6 and f[6]:
            links = [int(x) if x.lstrip("-").isdigit() else x for x in (y.strip() for y in f[6].split(","))]
        out.append(zone(f[0], center, radius, margin, weight, links, axes))
    if not out:
        raise ValueError(f"zones={text!r}: no entry")
    return out


def _has_zones(args: MpcArgs) -> bool:
    return bool(args.zones)


def _track_of(args: MpcArgs) -> tuple:
    """``get_env``'s track: the links of ``--zone_links`` (positions as ints)."""
    return tuple(int(x) if x.lstrip("-").isdigit() else x for x in (y.strip() for y in args.zone_links.split(",")) if x)


def _get_env(args: MpcArgs, device: int):
    """The env of the arguments: the built-in one, retracked where ``--zone_links`` says so (without the flag: today's call)."""
    track = _track_of(args)
    return get_env(args.env_name, device=device, track=track) if track else get_env(args.env_name, device=device)


def _zones_settings(args: MpcArgs) -> dict:
    return dict(zones=args.zones, zone_links=args.zone_links) if _has_zones(args) else {}


def zones_report(ep: dict) -> dict:
    """``zone_pen_mean``, ``zone_clear_min`` and ``zone_hits`` (the executed steps with negative clearance) of an episode's
    ``zone_pen`` / ``zone_clear`` logs, any leading episode axes included."""
    pen, clr = np.asarray(ep["zone_pen"], np.float64), np.asarray(ep["zone_clear"], np.float64)
    return dict(zone_pen_mean=float(pen.mean()), zone_clear_min=float(clr.min()), zone_hits=int((clr < 0).sum()))


def _online_zone_log(plan, xpos) -> tuple:
    """(s_t, clr_t) of executed steps from their tracked positions [E, K, 3]: the library's host text of the zone launch."""
    from .mbd_planner import _zones_record
    out = _capi.debug_zones_host(_zones_record(plan.env, plan._zone_entries), np.asarray(xpos, np.float32)[None])
    return out["step_pen"][0], out["step_clr"][0]


def _has_value(args: MpcArgs) -> bool:
    return bool(args.value)


def _value_of(args: MpcArgs):
    """``set_value``'s arguments: the net of ``--value`` and the record's scale."""
    from .value import ValueNet, terminal_scale
    return ValueNet.load(args.value), terminal_scale(args.value_scale, args.Hsample)


def _value_settings(args: MpcArgs) -> dict:
    return dict(value=args.value, value_scale=args.value_scale) if _has_value(args) else {}


_PLANT_FIELDS = ("plant_mass", "plant_friction", "plant_gear", "act_noise_std", "kick_std", "kick_every", "disturb_seed")


def _plant_settings(args: MpcArgs) -> dict:
    return {f: getattr(args, f) for f in _PLANT_FIELDS}


def _has_plant(args: MpcArgs) -> bool:
    """Whether the arguments ask for a plant record at all (every default: none is set)."""
    return any(getattr(args, f) != MpcArgs.__dataclass_fields__[f].default for f in _PLANT_FIELDS)


_ENS_FIELDS = ("ens_mass", "ens_friction", "ens_gear", "ens_risk")


def _has_ensemble(args: MpcArgs) -> bool:
    return any(getattr(args, f) != MpcArgs.__dataclass_fields__[f].default for f in _ENS_FIELDS)


def ensemble_triples(args: MpcArgs) -> list:
    """The members' (mass, friction, gear) triples: the three comma lists zipped, a single value broadcast, an absent list
    all 1.  [] without ensemble flags."""
    if not _has_ensemble(args):
        return []
    if args.ens_risk not in _capi.RISKS:
        raise ValueError(f"ens_risk={args.ens_risk!r}: one of {sorted(_capi.RISKS)}")
    lists = {f: [float(v) for v in str(getattr(args, f)).split(",") if v.strip()] or [1.0]
             for f in ("ens_mass", "ens_friction", "ens_gear")}
    M = max(len(v) for v in lists.values())
    for f, v in lists.items():
        if len(v) not in (1, M):
            raise ValueError(f"{f} lists {len(v)} values, another ensemble list {M}: equal lengths, or a single value")
    if not 1 <= M <= _capi.MAX_ENSEMBLE:
        raise ValueError(f"{M} ensemble members: 1 to {_capi.MAX_ENSEMBLE}")
    return [tuple(v[m] if len(v) > 1 else v[0] for v in lists.values()) for m in range(M)]


def _ensemble_envs(env, args: MpcArgs, device: int, cache: dict = None) -> list:
    """The member envs (None: the env itself, for the triple (1, 1, 1)), built with the plant's cache."""
    from dataclasses import replace
    return [_plant_env(env, replace(args, plant_mass=t[0], plant_friction=t[1], plant_gear=t[2]), device, cache)
            for t in ensemble_triples(args)]


def _ensemble_settings(args: MpcArgs) -> dict:
    return dict(ensemble=[dict(mass=t[0], friction=t[1], gear=t[2]) for t in ensemble_triples(args)], ens_risk=args.ens_risk)


_SHAPE_FIELDS = ("tail_rows", "tail_sigma", "noise_shape")


def tail_shape(H: int, Nu: int, rows: int, peak: float) -> np.ndarray:
    """The noise shape [H, Nu] of a warm replan: 1 for the rows h < H - rows, then the linear ramp
    1 + (peak - 1) (h - (H - rows) + 1) / rows up to ``peak`` at the last row — computed in float64, cast once to float32,
    the same for every actuator.  (With the default betas, Ndiffuse = 100 and warm_steps = 20, sigma_99 / sigma_20 = 4.2: a
    peak near 4 gives the last row the noise a cold plan starts with.)"""
    H, Nu, rows = int(H), int(Nu), int(rows)
    if not 0 <= rows <= H:
        raise ValueError(f"tail_rows={rows} outside [0, Hsample={H}]")
    if not (np.isfinite(peak) and peak >= 0):
        raise ValueError(f"tail_sigma={peak!r}: must be finite and >= 0")
    g = np.ones(H, np.float64)
    h = np.arange(H - rows, H, dtype=np.float64)
    g[H - rows:] = 1.0 + (float(peak) - 1.0) * (h - (H - rows) + 1.0) / max(rows, 1)
    return np.ascontiguousarray(np.broadcast_to(g.astype(np.float32)[:, None], (H, Nu)))


def _has_shape(args: MpcArgs) -> bool:
    """Whether the arguments ask for a noise shape at all (every default: none is set)."""
    return args.tail_rows != 0 or bool(args.noise_shape)


def _shape_of(args: MpcArgs, Nu: int):
    """(scale, when) of the arguments' noise shape: the tail ramp in the warm ticks, or the file's table in every step."""
    if args.tail_rows != 0 and args.noise_shape:
        raise ValueError("tail_rows and noise_shape both given: a plan has one noise shape")
    if args.noise_shape:
        return np.load(args.noise_shape), "always"
    return tail_shape(args.Hsample, Nu, args.tail_rows, args.tail_sigma), "warm"


def _shape_settings(args: MpcArgs) -> dict:
    return {f: getattr(args, f) for f in _SHAPE_FIELDS}


_BASIS_FIELDS = ("noise_knots", "noise_interp")
_BASIS_KINDS = ("linear", "hold")


def knot_basis(H: int, n_knots: int, kind: str = "linear", normalise: bool = True) -> np.ndarray:
    """The noise basis W [H, n_knots] of ``Plan.set_noise_basis``: "linear" — hat functions at the knots
    t_k = k (H - 1) / (n_knots - 1), so row h interpolates between the two knots around it and its weights sum to 1 (one
    knot: a constant column); "hold" — row h takes knot floor(h n_knots / H).  ``normalise`` divides every row by its
    Euclidean norm, so that every row keeps the variance sigma^2.  Computed in float64, cast once to float32."""
    H, K = int(H), int(n_knots)
    if H < 1:
        raise ValueError(f"Hsample={H}: must be >= 1")
    if not 1 <= K <= _capi.MAX_KNOTS:
        raise ValueError(f"noise_knots={K} outside [1, {_capi.MAX_KNOTS}]")
    if kind not in _BASIS_KINDS:
        raise ValueError(f"noise_interp={kind!r}: one of {list(_BASIS_KINDS)}")
    W = np.zeros((H, K), np.float64)
    h = np.arange(H, dtype=np.float64)
    if kind == "hold":
        W[np.arange(H), (np.arange(H) * K) // H] = 1.0
    elif K == 1 or H == 1:
        W[:, 0] = 1.0
    else:
        t = np.arange(K, dtype=np.float64) * (H - 1) / (K - 1)
        W = np.maximum(0.0, 1.0 - np.abs(h[:, None] - t[None, :]) * (K - 1) / (H - 1))
    if normalise:
        W = W / np.sqrt((W * W).sum(axis=1, keepdims=True))
    return np.ascontiguousarray(W.astype(np.float32))


def _has_basis(args: MpcArgs) -> bool:
    """Whether the arguments ask for a noise basis at all (the default: none)."""
    return args.noise_knots != 0


def _basis_of(args: MpcArgs):
    """(W, when) of the arguments' noise basis: in force in every step."""
    return knot_basis(args.Hsample, args.noise_knots, args.noise_interp), "always"


def _basis_settings(args: MpcArgs) -> dict:
    return {f: getattr(args, f) for f in _BASIS_FIELDS}


_OBJECTIVE_FIELDS = ("discount", "terminal_weight", "effort_cost", "rate_cost", "act_weight")


def discount_weights(H: int, gamma: float, terminal: float = 1.0) -> np.ndarray:
    """The row weights [H] of a discounted objective (include/mbd_hip.h mbd_objective.row_weight): w[h] = gamma ** h, the last row
    multiplied by ``terminal`` (it stands for everything behind the horizon) — in float64, rounded once to float32."""
    H = int(H)
    if H < 1:
        raise ValueError(f"Hsample={H}: must be >= 1")
    if not (np.isfinite(gamma) and gamma >= 0):
        raise ValueError(f"discount={gamma!r}: must be finite and >= 0")
    if not (np.isfinite(terminal) and terminal >= 0):
        raise ValueError(f"terminal_weight={terminal!r}: must be finite and >= 0")
    w = np.float64(gamma) ** np.arange(H, dtype=np.float64)
    w[-1] *= np.float64(terminal)
    return np.ascontiguousarray(w.astype(np.float32))


def action_rate(actions) -> float:
    """The executed rows' mean squared step-to-step difference, mean over steps and actuators of (u_n - u_{n-1})^2 (float64)."""
    a = np.asarray(actions, np.float64)
    return float(np.mean(np.diff(a, axis=-2) ** 2)) if a.shape[-2] > 1 else 0.0


def _has_objective(args: MpcArgs) -> bool:
    """Whether any objective flag differs from its default (then, and only then, the plan gets a record)."""
    return any(getattr(args, f) != MpcArgs.__dataclass_fields__[f].default for f in _OBJECTIVE_FIELDS)


def _objective_of(args: MpcArgs) -> dict:
    """``Plan.set_objective``'s arguments: the row weights only where a discount or a terminal weight is asked for."""
    weighted = args.discount != 1.0 or args.terminal_weight != 1.0
    return dict(row_weight=discount_weights(args.Hsample, args.discount, args.terminal_weight) if weighted else None,
                effort=args.effort_cost, rate=args.rate_cost, act_weight=np.load(args.act_weight) if args.act_weight else None)


def _objective_settings(args: MpcArgs) -> dict:
    return {f: getattr(args, f) for f in _OBJECTIVE_FIELDS} if _has_objective(args) else {}


def _has_weighting(args: MpcArgs) -> bool:
    """Whether the arguments ask for a weighting record at all (rejection, or an ESS target)."""
    return bool(args.reject_nonfinite) or args.ess_frac != 0.0


def _weighting_of(args: MpcArgs) -> dict:
    """``Plan.set_weighting``'s arguments (the bracket only with a target)."""
    ess = args.ess_frac != 0.0
    return dict(reject_nonfinite=args.reject_nonfinite, ess_frac=args.ess_frac, temp_min=args.temp_min if ess else None,
                temp_max=args.temp_max if ess else None, iters=args.ess_iters)


def _weighting_settings(args: MpcArgs) -> dict:
    return dict(reject_nonfinite=args.reject_nonfinite, ess_frac=args.ess_frac, temp_min=args.temp_min, temp_max=args.temp_max,
                ess_iters=args.ess_iters) if _has_weighting(args) else {}


def _has_adapt(args: MpcArgs) -> bool:
    """Whether the arguments ask for an adapt record at all (a rate)."""
    return args.adapt_rate != 0.0


def _adapt_of(args: MpcArgs) -> dict:
    """``Plan.set_adapt``'s arguments."""
    return dict(rate=args.adapt_rate, a_min=args.adapt_min, a_max=args.adapt_max, carry=bool(args.adapt_carry))


def _adapt_settings(args: MpcArgs) -> dict:
    return dict(adapt_rate=args.adapt_rate, adapt_min=args.adapt_min, adapt_max=args.adapt_max,
                adapt_carry=bool(args.adapt_carry)) if _has_adapt(args) else {}


def _adapt_log(log: dict) -> dict:
    """A peeked table and log as the report's three numbers."""
    return dict(adapt_table_min=float(log["a"].min()), adapt_table_max=float(log["a"].max()),
                adapt_steps_skipped=int(np.sum(log["skipped"])))


def _has_elites(args: MpcArgs) -> bool:
    """Whether the arguments ask for an elite record at all (elites, or the nominal)."""
    return args.elites != 0 or bool(args.elite_nominal)


def _elites_of(args: MpcArgs) -> dict:
    """``Plan.set_elites``'s arguments."""
    return dict(n_elites=args.elites, nominal=bool(args.elite_nominal), carry=bool(args.elite_carry))


def _elites_settings(args: MpcArgs) -> dict:
    return dict(elites=args.elites, elite_nominal=bool(args.elite_nominal), elite_carry=bool(args.elite_carry)) if _has_elites(args) else {}


def _elites_log(log: dict, Nd: int, K: int) -> dict:
    """A peeked step log as the report's two lists, one entry per tick: tick 0 ran Nd - 1 steps, every other tick K."""
    n = len(log["log_kept"])
    cuts = [0] + [min(c, n) for c in range(Nd - 1, n + K, K)] if n else [0]
    kept = [int(np.sum(log["log_kept"][a:b])) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
    top = [float(log["log_top"][b - 1]) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
    return dict(elites_kept=kept, elites_top=top)


def _has_togo(args: MpcArgs) -> bool:
    """Whether the arguments ask for a to-go record at all (a block)."""
    return args.togo_block != 0


def _togo_of(args: MpcArgs) -> dict:
    """``Plan.set_togo``'s arguments."""
    return dict(block=args.togo_block, min_tail=args.togo_min_tail)


def _togo_settings(args: MpcArgs) -> dict:
    return dict(togo_block=args.togo_block, togo_min_tail=args.togo_min_tail) if _has_togo(args) else {}


def _check_togo(args: MpcArgs) -> None:
    """What a to-go record refuses, decided from the arguments alone: the records whose per-row meaning is not defined."""
    if not _has_togo(args):
        return
    for name, has in (("objective", _has_objective), ("value", _has_value), ("weighting", _has_weighting), ("adapt", _has_adapt),
                      ("ensemble", _has_ensemble)):
        if has(args):
            raise ValueError(f"togo_block={args.togo_block!r} beside the {name} flags: a plan takes a to-go record or {name} record, "
                             "not both (what that record means per horizon row is not defined)")


_PICK_NAMES = ("mean", "prev", "best")


def _has_pick(args: MpcArgs) -> bool:
    return bool(args.pick)


def _pick_of(args: MpcArgs) -> dict:
    """``Plan.set_mpc_pick``'s arguments from ``pick``: a comma-separated non-empty subset of mean, prev, best."""
    names = [n.strip() for n in args.pick.split(",") if n.strip()]
    if not names or any(n not in _PICK_NAMES for n in names):
        raise ValueError(f"pick={args.pick!r}: a comma-separated non-empty subset of {', '.join(_PICK_NAMES)}")
    return {n: n in names for n in _PICK_NAMES}


def _pick_settings(args: MpcArgs) -> dict:
    return dict(pick=args.pick) if _has_pick(args) else {}


def _pick_log(log) -> dict:
    """A pick log (one episode's dict, or a batch's list of them) as JSON: the share of ticks per choice and the mean value of the
    picked plan and of the mean."""
    logs = log if isinstance(log, list) else [log]
    choice = np.concatenate([np.asarray(l["choice"]) for l in logs])
    rets = np.concatenate([np.asarray(l["rets"], np.float32).reshape(-1, 3) for l in logs])
    picked = rets[np.arange(len(choice)), choice] if len(choice) else rets[:, 0]
    with np.errstate(all="ignore"):
        return dict(share={n: float(np.mean(choice == k)) for k, n in enumerate(_PICK_NAMES)},
                    picked_value_mean=float(np.mean(picked)), mean_value_mean=float(np.mean(rets[:, 0])))


def _weighting_log(log: dict) -> dict:
    """A peeked log as JSON-ready lists."""
    return dict(temp=[float(x) for x in log["temp"]], ess=[float(x) for x in log["ess"]], kept=[int(x) for x in log["kept"]])


def _has_delay(args: MpcArgs) -> bool:
    """Whether the arguments ask for a delay record at all (the default: none)."""
    return args.delay_ticks != 0


def _delay_settings(args: MpcArgs) -> dict:
    return dict(delay_ticks=args.delay_ticks) if _has_delay(args) else {}


def cycle_clip(xref, n_rows: int, period: int) -> np.ndarray:
    """``xref`` [K, L0, 3] (or [L0, C]) extended periodically to ``n_rows`` rows: the rows < L0 are xref's own; row L0 + i
    repeats row L0 - period + (i mod period) of the last ``period`` rows, advanced by 1 + i // period times the displacement
    over one period, xref[:, L0-1] - xref[:, L0-1-period] — a gait cycle that keeps travelling.  Computed in float64, cast once
    to float32.  1 <= period <= L0 - 1."""
    x = np.asarray(xref, np.float64)
    flat = x.ndim == 2
    if flat:
        x = x[None]
    if x.ndim != 3:
        raise ValueError(f"clip of shape {np.shape(xref)}: must be [K, L0, C] or [L0, C]")
    L0, n_rows, period = x.shape[1], int(n_rows), int(period)
    if n_rows < 1:
        raise ValueError(f"n_rows={n_rows}: must be >= 1")
    if period < 1:
        raise ValueError(f"period={period}: must be >= 1")
    if period >= L0:
        raise ValueError(f"period={period}: must be < the clip's {L0} rows (the displacement over one period is taken inside it)")
    out = np.empty((x.shape[0], n_rows, x.shape[2]), np.float64)
    out[:, : min(L0, n_rows)] = x[:, :n_rows]
    if n_rows > L0:
        i = np.arange(n_rows - L0)
        disp = x[:, L0 - 1] - x[:, L0 - 1 - period]
        out[:, L0:] = x[:, L0 - period + i % period] + (1 + i // period)[None, :, None] * disp[:, None, :]
    out = np.ascontiguousarray(out.astype(np.float32))
    return out[0] if flat else out


_DEMO_FIELDS = ("demo_clip", "demo_start", "demo_period")


def _has_demo(args: MpcArgs) -> bool:
    """Whether the arguments ask for a demo record at all (the default: none)."""
    return bool(args.demo_clip)


def _demo_of(env, args: MpcArgs):
    """(clip, start_row) of the arguments' demo record: the env's demo or the file's array, extended by ``cycle_clip`` to the
    last row a window of the episode reads when ``demo_period`` > 0."""
    if args.demo_clip == "env":
        if getattr(env, "xref", None) is None:
            raise ValueError(f"demo_clip=env: env_name={args.env_name!r} has no demo")
        clip = np.asarray(env.xref, np.float32)
    else:
        clip = np.asarray(np.load(args.demo_clip), np.float32)
    if args.demo_period < 0:
        raise ValueError(f"demo_period={args.demo_period}: must be >= 0")
    if args.demo_period > 0:
        clip = cycle_clip(clip, args.demo_start + (args.n_ticks + args.delay_ticks) * args.exec_steps + args.Hsample, args.demo_period)
    return clip, args.demo_start


def _demo_settings(args: MpcArgs) -> dict:
    return {f: getattr(args, f) for f in _DEMO_FIELDS} if _has_demo(args) else {}


_SIGMA_FIELDS = ("update_method", "sigma_cold", "sigma_warm", "sigma_gain")


def _method(args: MpcArgs) -> int:
    """The update_method of the arguments' plans (ValueError on an unknown name)."""
    if args.update_method not in UPDATE_METHODS:
        raise ValueError(f"update_method={args.update_method!r}: one of {list(UPDATE_METHODS)}")
    return UPDATE_METHODS[args.update_method]


def _has_sigma(args: MpcArgs) -> bool:
    """Whether the arguments ask for a sigma record: whenever the method is not MBD."""
    return _method(args) != 0


def _sigma_of(args: MpcArgs) -> tuple:
    return args.sigma_cold, args.sigma_warm, args.sigma_gain


def _sigma_settings(args: MpcArgs) -> dict:
    return {f: getattr(args, f) for f in _SIGMA_FIELDS} if _has_sigma(args) else {}


def _plant_env(env, args: MpcArgs, device: int, cache: dict = None):
    """The env that executes the rows: None (the planner's own) unless mass / friction / gear differ from 1; one env per
    distinct triple in ``cache``."""
    triple = (float(args.plant_mass), float(args.plant_friction), float(args.plant_gear))
    if triple == (1.0, 1.0, 1.0):
        return None
    if not hasattr(env, "sys"):
        raise ValueError(f"env_name={args.env_name!r} has no rigid-body model to scale: plant_mass / plant_friction / "
                         "plant_gear need one")
    if cache is not None and triple in cache:
        return cache[triple]
    from ..envs.base import RigidBodyEnv
    plant = RigidBodyEnv(args.env_name, device=device, model=env.sys.scaled(*triple))
    if cache is not None:
        cache[triple] = plant
    return plant


def _record_kwargs(env, args: MpcArgs, device: int, cache: dict = None) -> dict:
    return dict(env=_plant_env(env, args, device, cache), key=_capi.prng_key(args.disturb_seed), act_std=args.act_noise_std,
                kick_std=args.kick_std, kick_every=args.kick_every)


def _reset_and_key(env, seed: int):
    """The reset state and the episode key of a seed, by the reference's chain."""
    rng = _capi.prng_key(seed)  # mbd_planner.py:40
    rng, rng_reset = _capi.prng_split(rng, 2, prng_impl())  # :79
    state_init = env.reset(rng_reset)  # :80
    rng_exp, rng = _capi.prng_split(rng, 2, prng_impl())  # :150
    return state_init, rng_exp


def _set_records(handle, env, args: MpcArgs, after_sigma=None, after_value=None) -> None:
    """The records a ``Plan`` and a ``Sweep`` both take, in the one order of their set calls (a sweep: one record for all episodes —
    ``_check_batch`` has held the fields equal).  ``after_sigma`` / ``after_value``: where a plan's set calls of what only a plan
    takes stand in that order — the plant and the ensemble record; the adapt record."""
    if _has_sigma(args):
        handle.set_mpc_sigma(*_sigma_of(args))
    if after_sigma:
        after_sigma()
    if _has_shape(args):
        handle.set_noise_shape(*_shape_of(args, env.action_size))
    if _has_basis(args):
        handle.set_noise_basis(*_basis_of(args))
    if _has_delay(args):
        handle.set_mpc_delay(args.delay_ticks)
    if _has_demo(args):
        handle.set_mpc_demo(*_demo_of(env, args))
    if _has_objective(args):
        handle.set_objective(**_objective_of(args))
    if _has_weighting(args):
        handle.set_weighting(**_weighting_of(args))
    if _has_pick(args):
        handle.set_mpc_pick(**_pick_of(args))
    if _has_value(args):
        handle.set_value(*_value_of(args))
    if after_value:
        after_value()
    if _has_elites(args):  # (a sweep: every episode has its own elites)
        handle.set_elites(**_elites_of(args))
    if _has_togo(args):
        handle.set_togo(**_togo_of(args))
    if _has_zones(args):
        handle.set_zones(parse_zones(args.zones))


def _setup(args: MpcArgs, device: int, online: bool = False):
    """``online``: no plant record is set — the caller executes the rows (``run_mpc_online``)."""
    _check_togo(args)
    apply_recommended(args)
    env = _get_env(args, device)
    state_init, rng_exp = _reset_and_key(env, args.seed)
    plan = Plan(env, args, update_method=_method(args))
    plan.set_state0(state_init)
    cache = {}

    def plant_and_ensemble():
        if _has_plant(args) and not online:
            plan.set_mpc_plant(**_record_kwargs(env, args, device, cache))
        if _has_ensemble(args):
            plan.set_ensemble(_ensemble_envs(env, args, device, cache), args.ens_risk)

    def adapt():
        if _has_adapt(args):
            plan.set_adapt(**_adapt_of(args))

    _set_records(plan, env, args, plant_and_ensemble, adapt)
    return env, plan, state_init, rng_exp


def _check_online(args: MpcArgs) -> None:
    """What ``--online`` refuses, decided from the arguments alone."""
    for f in ("act_noise_std", "kick_std"):
        if getattr(args, f) != MpcArgs.__dataclass_fields__[f].default:
            raise ValueError(f"{f}={getattr(args, f)!r} with online: the action noise and the kicks are drawn by the plant record, "
                             "and a session has none — the caller is the plant; disturb the plant you drive instead")


def _online_episode(env, plant, plan, state_init, key, args: MpcArgs) -> dict:
    """One episode through a session: tick, execute the rows on ``plant`` (None: ``env``) with ``env.rollout``, hand the state
    reached to the next tick.  Returns ``Plan.run_mpc``'s dict (``seconds``: the sum of the ticks' own) and ``tick_seconds`` [T]."""
    from ..envs.base import State
    pe = env if plant is None else plant
    T, E = args.n_ticks, args.exec_steps
    s = np.ascontiguousarray(state_init.pipeline_state, np.float32).reshape(-1)
    actions, rewards, states, means, predicted, secs, wlog, plog, zlog = [], [], [s], [], [], [], [], [], []
    with plan.mpc_open(key, args.warm_steps, E, T) as session:
        for _ in range(T):
            out = session.tick(s)
            if _has_weighting(args):  # (between ticks: the tick's last score step)
                wl = plan.peek_weighting()
                wlog.append((wl["temp"][-1], wl["ess"][-1], wl["kept"][-1]))
            if session.pick is not None:  # (a pick record: what the tick handed on)
                plog.append(session.pick)
            rows = out["head"]  # (the rows to execute now: the plan's own first rows, or under a delay record the queue's head)
            if _has_zones(args):  # (the executed steps' tracked positions: their penalties and clearances, on the host)
                rewss, xp, fin = pe.rollout(State(s, None, np.float32(0), np.float32(0), {}), rows[None], want_xpos=True, want_final=True)
                zlog.append(_online_zone_log(plan, xp[0].cpu().numpy()))
            else:
                rewss, fin = pe.rollout(State(s, None, np.float32(0), np.float32(0), {}), rows[None], want_final=True)
            s = fin[0].cpu().numpy().reshape(-1)
            actions.append(rows)
            rewards.append(rewss[0].cpu().numpy())
            states.append(s)
            means.append(out["mean"])
            predicted.append(out["predicted"])
            secs.append(out["seconds"])
        adapt = plan.peek_adapt() if _has_adapt(args) else None  # (the table behind the last tick, the log of the session's steps)
        elites = plan.peek_elites() if _has_elites(args) else None
        togo = plan.peek_togo() if _has_togo(args) else None
    ep = dict(actions=np.concatenate(actions), rewards=np.concatenate(rewards), states=np.stack(states), means=np.stack(means),
              seconds=float(np.sum(secs)), tick_seconds=np.asarray(secs, np.float64))
    if plan._has_delay:
        ep["predicted"] = np.stack(predicted)
    if wlog:  # per tick: the temperature, ESS and kept count of the tick's last step
        ep["weighting"] = dict(temp=np.array([w[0] for w in wlog], np.float32), ess=np.array([w[1] for w in wlog], np.float32),
                               kept=np.array([w[2] for w in wlog], np.int32))
    if adapt is not None:
        ep["adapt"] = adapt
    if elites is not None:
        ep["elite_log"] = elites
    if togo is not None:
        ep["togo"] = togo
    if zlog:
        ep["zone_pen"], ep["zone_clear"] = np.concatenate([z[0] for z in zlog]), np.concatenate([z[1] for z in zlog])
    if plog:
        ep["pick"] = dict(choice=np.array([x["choice"] for x in plog], np.int32), rets=np.stack([x["rets"] for x in plog]),
                          best=np.array([x["best"] for x in plog], np.int32))
    return ep


def run_mpc_online(args: MpcArgs, device: int = None, return_details: bool = False):
    """``run_mpc``'s episode through a session, the Python side being the plant (``--online``)."""
    _check_online(args)
    device = 0 if device is None else device
    env, plan, state_init, key = _setup(args, device, online=True)
    try:
        ep = _online_episode(env, _plant_env(env, args, device), plan, state_init, key, args)
    finally:
        plan.close()
    reward = float(ep["rewards"].mean())
    if not args.not_render:
        _save(args, ep)
    if return_details:
        return reward, dict(ep, state_init=state_init, key=key, dt=env.dt)
    return reward


def _check_batch(arg_list) -> None:
    """What a batch of lockstep episodes takes (the rule of scripts.run_mbd._batchable): up to 32 episodes of one rigid-body
    env with one set of sizes, schedule, (T, K, E) and delay_ticks; seeds, temperatures and the plant settings may differ.
    Decided from the arguments alone.  The episodes' OWN arguments: an elite or to-go record is the batch's, one for all episodes,
    and ``_check_batch_records`` takes those flags off the episodes before it asks this function."""
    from dataclasses import asdict

    from ..scripts.run_mbd import _resolved
    if not 1 <= len(arg_list) <= MAX_EPISODES:
        raise ValueError(f"{len(arg_list)} episodes: a batch holds 1 to {MAX_EPISODES}")
    for k, a in enumerate(arg_list):
        if _has_togo(a):
            raise ValueError(f"episode {k} carries togo_block={a.togo_block!r} of its own: a sweep takes one to-go record for all its "
                             "episodes (_check_batch_records)")
        if _has_elites(a):
            raise ValueError(f"episode {k} carries elites={a.elites!r} / elite_nominal={a.elite_nominal!r} of its own: a sweep takes "
                             "one elite record for all its episodes (_check_batch_records)")
        if _has_adapt(a):
            raise ValueError(f"episode {k} carries adapt_rate={a.adapt_rate!r}: sweeps take no adapt record (their samplers take one "
                             "shape for all plans); run the episodes one by one (run_mpc)")
        if _has_ensemble(a):
            raise ValueError(f"episode {k} carries ensemble flags ({', '.join(f for f in _ENS_FIELDS if getattr(a, f) != MpcArgs.__dataclass_fields__[f].default)}): "
                             "batches of lockstep episodes take no ensemble; run the episodes one by one (run_mpc)")
    ds = [asdict(_resolved(a)) for a in arg_list]
    for k, d in enumerate(ds):
        for f, v in d.items():
            if f not in ("seed", "temp_sample", "not_render") + _PLANT_FIELDS and v != ds[0][f]:
                raise ValueError(f"{f} differs between episodes 0 and {k} ({ds[0][f]!r}, {v!r}): the episodes of a batch "
                                 "may differ in seed, temp_sample and the plant settings only")
    if _has_shape(arg_list[0]) and arg_list[0].tail_rows != 0 and arg_list[0].noise_shape:
        raise ValueError("tail_rows and noise_shape both given: a sweep has one noise shape")
    if ds[0]["env_name"] in ("car2d", "pushT"):
        raise ValueError(f"env_name={ds[0]['env_name']!r}: batches run rigid-body envs; run its episodes one by one")
    if ds[0]["Nsample"] * 4 > 48 * 1024:
        raise ValueError(f"Nsample={ds[0]['Nsample']}: plans of more than 12288 candidates fill the chip on their own; "
                         "run their episodes one by one")
    if ds[0]["enable_demo"] and not _has_demo(arg_list[0]):
        raise ValueError("enable_demo: demos are time-indexed, an episode has no clock for them: give it one with demo_clip")
    if _has_demo(arg_list[0]) and not ds[0]["enable_demo"]:
        raise ValueError(f"demo_clip={arg_list[0].demo_clip!r} without enable_demo: the plans do not use demos")


_BATCH_RECORD_FIELDS = ("elites", "elite_nominal", "elite_carry", "togo_block", "togo_min_tail")


def _check_batch_records(arg_list) -> None:
    """``_check_batch`` for a batch that may carry an elite and a to-go record (mbd_sweep_set_elites, mbd_sweep_set_togo): the five
    flags are the batch's — equal in every episode, else ValueError naming the field —, ``_check_togo``'s refusals hold, and the
    episodes without those flags are what ``_check_batch`` takes.  An adapt record stays refused there."""
    from dataclasses import replace
    arg_list = list(arg_list)
    for k, a in enumerate(arg_list):
        _check_togo(a)
        for f in _BATCH_RECORD_FIELDS:
            if getattr(a, f) != getattr(arg_list[0], f):
                raise ValueError(f"{f} differs between episodes 0 and {k} ({getattr(arg_list[0], f)!r}, {getattr(a, f)!r}): a sweep takes "
                                 "one elite and one to-go record for all its episodes")
    none = {f: MpcArgs.__dataclass_fields__[f].default for f in _BATCH_RECORD_FIELDS}
    _check_batch([replace(a, **none) for a in arg_list])


def _setup_batch(arg_list, device: int):
    for a in arg_list:
        apply_recommended(a)
    a0 = arg_list[0]
    env = _get_env(a0, device)
    sweep = Sweep(env, a0, len(arg_list), temps=[a.temp_sample for a in arg_list], update_method=_method(a0))
    _set_records(sweep, env, a0)
    states, keys, plants = [], [], {}
    for k, a in enumerate(arg_list):
        state_init, rng_exp = _reset_and_key(env, a.seed)
        sweep.set_state0(k, state_init)
        if _has_plant(a):  # (one plant env per distinct (mass, friction, gear): episodes in a row that share it share a launch)
            sweep.set_mpc_plant(k, **_record_kwargs(env, a, device, plants))
        states.append(state_init)
        keys.append(rng_exp)
    return env, sweep, states, np.array(keys, np.uint32)


_LOGS = ("actions", "rewards", "states", "means")


def run_mpc_batch(arg_list, device: int = None, return_details: bool = False):
    """The episodes of ``arg_list`` (MpcArgs that differ in ``seed``, ``temp_sample`` and the plant settings only, else ValueError
    naming the field)
    as ONE batch in lockstep.  Episode k is ``run_mpc(arg_list[k])`` bit for bit.  Returns the list of the episodes' mean
    rewards; ``return_details`` adds the list of their detail dicts (as ``run_mpc``'s; ``seconds`` is the whole batch's).
    Unless the first episode says ``not_render``: results/<env>/mpc_episode.npz, its arrays with a leading episode axis when
    there is more than one episode."""
    arg_list = list(arg_list)
    _check_batch_records(arg_list)
    env, sweep, states, keys = _setup_batch(arg_list, 0 if device is None else device)
    try:
        ep = sweep.run_mpc(keys, arg_list[0].n_ticks, arg_list[0].warm_steps, arg_list[0].exec_steps)
        _peek_batch_records(sweep, arg_list[0], ep)
    finally:
        sweep.close()
    rewards = [float(r.mean()) for r in ep["rewards"]]
    if not arg_list[0].not_render:
        _save(arg_list[0], ep if len(arg_list) > 1 else {k: ep[k][0] for k in _logs(ep)})
    if return_details:
        shape = _shape_settings(arg_list[0]) if _has_shape(arg_list[0]) else {}
        if _has_basis(arg_list[0]):
            shape = dict(shape, **_basis_settings(arg_list[0]))
        shape = dict(shape, **_delay_settings(arg_list[0]), **_demo_settings(arg_list[0]), **_sigma_settings(arg_list[0]),
                     **_objective_settings(arg_list[0]), **_weighting_settings(arg_list[0]), **_elites_settings(arg_list[0]),
                     **_togo_settings(arg_list[0]), **_zones_settings(arg_list[0]))
        windows = {"demo_windows": ep["demo_windows"]} if "demo_windows" in ep else {}  # (one table: every episode's)
        pick = (lambda k: {f: ep[f][k] for f in ("pick", "elite_log", "togo") if f in ep})
        return rewards, [dict({f: ep[f][k] for f in _logs(ep)}, **windows, **pick(k), seconds=ep["seconds"], state_init=states[k], key=keys[k], dt=env.dt,
                              **_plant_settings(arg_list[k]), **shape) for k in range(len(arg_list))]
    return rewards


def _peek_batch_records(sweep, a0: MpcArgs, ep: dict) -> None:
    """Every episode's elites and step log, and its last step's returns and weights per group, as ``run_mpc`` reports them."""
    if _has_elites(a0):
        ep["elite_log"] = [sweep.peek_elites(k) for k in range(sweep.P)]
    if _has_togo(a0):
        ep["togo"] = [sweep.peek_togo(k) for k in range(sweep.P)]


def _logs(ep: dict) -> tuple:
    """The episode's logs: the four every episode has, the predicted states of one with a delay record, the distances from
    the clip of one with a demo record, the ticks' sigmas of a path-integral one."""
    return _LOGS + tuple(k for k in ("predicted", "track_err", "sigmas", "zone_pen", "zone_clear") if k in ep)


def _save(args: MpcArgs, ep: dict) -> None:
    path = os.path.join(os.getcwd(), "results", args.env_name)
    os.makedirs(path, exist_ok=True)
    extra = {"demo_windows": ep["demo_windows"]} if "demo_windows" in ep else {}  # (one table, whatever the episodes)
    np.savez_compressed(os.path.join(path, "mpc_episode.npz"), **{k: ep[k] for k in _logs(ep)}, **extra)


def run_mpc(args: MpcArgs, device: int = None, return_details: bool = False):
    """One closed-loop episode of ``args.n_ticks`` ticks.  Returns the episode's mean reward (over its T * E executed control
    steps); ``return_details`` adds a dict with the episode's actions, rewards, states (s_0 .. s_T), per-tick means, the
    loop's wall time (seconds), the reset state, the episode key and the control dt.  Unless ``not_render``:
    results/<env>/mpc_episode.npz."""
    env, plan, state_init, key = _setup(args, 0 if device is None else device)
    try:
        ep = plan.run_mpc(key, args.n_ticks, args.warm_steps, args.exec_steps)
        if _has_weighting(args):  # (the device log holds the last tick's score steps: their temperature, ESS and kept count)
            ep["weighting_last_tick"] = plan.peek_weighting()
        if _has_adapt(args):  # (the table behind the last tick and the log of the episode's steps)
            ep["adapt"] = plan.peek_adapt()
        if _has_elites(args):  # (the elites behind the last tick and the log of the episode's steps)
            ep["elite_log"] = plan.peek_elites()
        if _has_togo(args):  # (the layout, and the last step's returns and weights per group)
            ep["togo"] = plan.peek_togo()
    finally:
        plan.close()
    reward = float(ep["rewards"].mean())
    if not args.not_render:
        _save(args, ep)
    if return_details:
        ens = _ensemble_settings(args) if _has_ensemble(args) else {}
        shape = _shape_settings(args) if _has_shape(args) else {}
        if _has_basis(args):
            shape = dict(shape, **_basis_settings(args))
        shape = dict(shape, **_delay_settings(args), **_demo_settings(args), **_sigma_settings(args), **_objective_settings(args),
                     **_weighting_settings(args), **_adapt_settings(args), **_elites_settings(args), **_togo_settings(args),
                     **_zones_settings(args))
        return reward, dict(ep, state_init=state_init, key=key, dt=env.dt, **_plant_settings(args), **ens, **shape)
    return reward


def _main(argv=None) -> dict:
    """The CLI: a warm-up episode, an open-loop run_diffusion loop of the same plan (its ms per diffusion step, for
    comparison) and the timed episode, all in one process; returns what it prints."""
    import argparse
    import contextlib
    import json
    import sys

    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    for f in MpcArgs.__dataclass_fields__.values():
        if f.type in ("bool", bool):
            p.add_argument(f"--{f.name}", action="store_true")
        else:
            p.add_argument(f"--{f.name}", type=type(f.default), default=f.default)
    p.add_argument("--n_episodes", type=int, default=1, help="seeds seed .. seed+P-1 as one batch of lockstep episodes")
    ns = vars(p.parse_args(argv))
    n_episodes = ns.pop("n_episodes")
    args = MpcArgs(**ns)
    if args.online:
        if n_episodes != 1 and _has_sigma(args):  # (the library's own refusal: sessions of path-integral sweeps)
            from dataclasses import replace
            arg_list = [replace(args, seed=args.seed + k) for k in range(n_episodes)]
            _check_batch_records(arg_list)
            _, sweep, _, keys = _setup_batch(arg_list, 0)
            try:
                sweep.mpc_open(keys, args.warm_steps, args.exec_steps, args.n_ticks).close()
            finally:
                sweep.close()
        if n_episodes != 1:
            raise ValueError(f"n_episodes={n_episodes} with online: a session drives one episode")
        return _main_online(args)
    if n_episodes != 1:
        return _main_batch(args, n_episodes)
    with contextlib.redirect_stdout(sys.stderr):  # (stdout carries the JSON line only)
        env, plan, state_init, key = _setup(args, 0)
        T, K, E, Nd = args.n_ticks, args.warm_steps, args.exec_steps, args.Ndiffuse
        plan.run_mpc(key, T, K, E)  # warm-up
        _, _, _, open_secs = plan.run(key)
        ep = plan.run_mpc(key, T, K, E)
        wlog = plan.peek_weighting() if _has_weighting(args) else None
        alog = plan.peek_adapt() if _has_adapt(args) else None
        elog = plan.peek_elites() if _has_elites(args) else None
        tlog = plan.peek_togo() if _has_togo(args) else None
        nominal = None
        if _has_plant(args):  # what the perturbation cost: the same episode without the record
            plan.clear_mpc_plant()
            nominal = float(plan.run_mpc(key, T, K, E)["rewards"].mean())
        plan.close()
    steps = (Nd - 1) + (T - 1) * K  # diffusion steps the episode ran
    secs = ep["seconds"]
    open_ms = 1e3 * open_secs / (Nd - 1)
    res = dict(env=args.env_name, Nsample=args.Nsample, Hsample=args.Hsample, Ndiffuse=Nd, n_ticks=T, warm_steps=K,
               exec_steps=E, ms_per_tick=1e3 * secs / T, ticks_per_s=T / secs, ms_per_diffusion_step=1e3 * secs / steps,
               open_loop_ms_per_diffusion_step=open_ms,
               # what a tick costs beyond its diffusion steps at the open-loop rate: the boundary launches (two; three with a plant record)
               boundary_ms_per_tick=(1e3 * secs - steps * open_ms) / T,
               real_time_factor=T * E * env.dt / secs, episode_reward=float(ep["rewards"].mean()))
    if nominal is not None:  # (without a record the line is what it always was)
        res.update(_plant_settings(args), nominal_episode_reward=nominal)
    if _has_ensemble(args):
        res.update(_ensemble_settings(args))
    if _has_shape(args):
        res.update(_shape_settings(args))
    if _has_basis(args):
        res.update(_basis_settings(args))
    res.update(_delay_settings(args))  # (without a record the line is what it always was)
    res.update(_sigma_settings(args))
    if _has_objective(args):  # (the executed rows' mean squared step-to-step difference, from actions_out on the host)
        res.update(_objective_settings(args), action_rate=action_rate(ep["actions"]))
    if _has_demo(args):
        res.update(_demo_settings(args), track_err_mean=float(ep["track_err"].mean()))
    if wlog is not None:  # (the last tick's score steps)
        res.update(_weighting_settings(args), weighting_last_tick=_weighting_log(wlog))
    if "pick" in ep:
        res.update(_pick_settings(args), pick_log=_pick_log(ep["pick"]))
    res.update(_value_settings(args))  # (without --value the line is what it always was)
    if alog is not None:
        res.update(_adapt_settings(args), **_adapt_log(alog))
    if elog is not None:
        res.update(_elites_settings(args), **_elites_log(elog, args.Ndiffuse, K))
    if tlog is not None:
        res.update(_togo_settings(args), togo_groups=[int(x) for x in tlog["starts"]])
    if "zone_pen" in ep:  # (the executed control steps' penalties and keep-out clearances)
        res.update(_zones_settings(args), **zones_report(ep))
    if not args.not_render:
        _save(args, ep)
    print(json.dumps(res), flush=True)
    return res


def _main_online(args: MpcArgs) -> dict:
    """``--online``: the episode through a session after a warm-up one, in one process; the times are the session's own."""
    import contextlib
    import json
    import sys

    _check_online(args)
    with contextlib.redirect_stdout(sys.stderr):  # (stdout carries the JSON line only)
        env, plan, state_init, key = _setup(args, 0, online=True)
        plant = _plant_env(env, args, 0)
        _online_episode(env, plant, plan, state_init, key, args)  # warm-up
        ep = _online_episode(env, plant, plan, state_init, key, args)
        plan.close()
    T, E = args.n_ticks, args.exec_steps
    ms = 1e3 * ep["tick_seconds"]
    warm = ms[1:] if T > 1 else ms  # (tick 0 is the cold plan: Ndiffuse-1 steps)
    res = dict(env=args.env_name, Nsample=args.Nsample, Hsample=args.Hsample, Ndiffuse=args.Ndiffuse, n_ticks=T,
               warm_steps=args.warm_steps, exec_steps=E, online=True, ms_per_tick=float(ms.mean()), tick0_ms=float(ms[0]),
               warm_tick_ms_min=float(warm.min()), warm_tick_ms_median=float(np.median(warm)), warm_tick_ms_max=float(warm.max()),
               real_time_factor=T * E * env.dt / ep["seconds"], episode_reward=float(ep["rewards"].mean()))
    if _has_plant(args):
        res.update(_plant_settings(args))
    res.update(_delay_settings(args))
    res.update(_sigma_settings(args))
    if _has_objective(args):
        res.update(_objective_settings(args), action_rate=action_rate(ep["actions"]))
    if "weighting" in ep:  # (per tick)
        res.update(_weighting_settings(args), weighting=_weighting_log(ep["weighting"]))
    if "pick" in ep:
        res.update(_pick_settings(args), pick_log=_pick_log(ep["pick"]))
    res.update(_value_settings(args))  # (without --value the line is what it always was)
    if "adapt" in ep:
        res.update(_adapt_settings(args), **_adapt_log(ep["adapt"]))
    if "elite_log" in ep:
        res.update(_elites_settings(args), **_elites_log(ep["elite_log"], args.Ndiffuse, args.warm_steps))
    if "togo" in ep:
        res.update(_togo_settings(args), togo_groups=[int(x) for x in ep["togo"]["starts"]])
    if "zone_pen" in ep:
        res.update(_zones_settings(args), **zones_report(ep))
    if not args.not_render:
        _save(args, ep)
    print(json.dumps(res), flush=True)
    return res


def _main_batch(args: MpcArgs, P: int) -> dict:
    """``--n_episodes P``: the batch after a warm-up batch, the sweep's and one plan's open-loop loops, and ONE sequential episode
    of the first seed (what the batch replaces P times) after a warm-up one, all in one process."""
    import contextlib
    import json
    import sys
    from dataclasses import replace

    arg_list = [replace(args, seed=args.seed + k) for k in range(P)]
    _check_batch_records(arg_list)
    with contextlib.redirect_stdout(sys.stderr):  # (stdout carries the JSON line only)
        env, sweep, states, keys = _setup_batch(arg_list, 0)
        a0 = arg_list[0]
        T, K, E, Nd = a0.n_ticks, a0.warm_steps, a0.exec_steps, a0.Ndiffuse
        sweep.run_mpc(keys, T, K, E)  # warm-up
        _, _, _, open_secs = sweep.run(keys, outputs=False)
        ep = sweep.run_mpc(keys, T, K, E)
        _peek_batch_records(sweep, a0, ep)
        nominal = None
        if _has_plant(a0):  # what the perturbation cost: the same batch without the records
            for k in range(P):
                sweep.clear_mpc_plant(k)
            nominal = [float(r.mean()) for r in sweep.run_mpc(keys, T, K, E)["rewards"]]
        sweep.close()
        plan = Plan(env, a0, update_method=_method(a0))
        plan.set_state0(states[0])

        def plant():
            if _has_plant(a0):
                plan.set_mpc_plant(**_record_kwargs(env, a0, 0))

        _set_records(plan, env, a0, plant)
        plan.run_mpc(keys[0], T, K, E)  # warm-up
        _, _, _, open_secs_1 = plan.run(keys[0])
        seq = plan.run_mpc(keys[0], T, K, E)
        plan.close()
    steps = (Nd - 1) + (T - 1) * K  # diffusion steps every episode ran
    secs = ep["seconds"]
    open_ms, open_ms_1 = 1e3 * open_secs / (Nd - 1), 1e3 * open_secs_1 / (Nd - 1)
    rews = [float(r.mean()) for r in ep["rewards"]]
    res = dict(env=a0.env_name, Nsample=a0.Nsample, Hsample=a0.Hsample, Ndiffuse=Nd, n_ticks=T, warm_steps=K, exec_steps=E,
               n_episodes=P, ms_per_tick=1e3 * secs / T, ticks_per_s=T / secs, episode_ticks_per_s=P * T / secs,
               ms_per_diffusion_step=1e3 * secs / steps, open_loop_ms_per_diffusion_step=open_ms,
               # what a tick of the batch costs beyond its diffusion steps at the sweep's open-loop rate: the boundary launches
               boundary_ms_per_tick=(1e3 * secs - steps * open_ms) / T,
               real_time_factor=T * E * env.dt / secs, episode_reward=float(np.mean(rews)), episode_rewards=rews,
               episode_reward_mean=float(np.mean(rews)), episode_reward_std=float(np.std(rews)),
               # one episode of the first seed on a plan of its own, and what P of them one after another cost against the batch
               sequential_episode_seconds=seq["seconds"], single_open_loop_ms_per_diffusion_step=open_ms_1,
               speedup=P * seq["seconds"] / secs, open_loop_ratio=P * open_ms_1 / open_ms)
    if nominal is not None:  # (without records the line is what it always was)
        res.update(_plant_settings(a0), nominal_episode_reward=float(np.mean(nominal)))
    if _has_shape(a0):
        res.update(_shape_settings(a0))
    if _has_basis(a0):
        res.update(_basis_settings(a0))
    res.update(_delay_settings(a0))
    res.update(_sigma_settings(a0))
    if _has_objective(a0):
        res.update(_objective_settings(a0), action_rate=action_rate(ep["actions"]))
    res.update(_weighting_settings(a0))
    if "pick" in ep:
        res.update(_pick_settings(a0), pick_log=_pick_log(ep["pick"]))
    res.update(_value_settings(a0))
    if "elite_log" in ep:  # (per episode)
        logs = [_elites_log(lg, Nd, K) for lg in ep["elite_log"]]
        res.update(_elites_settings(a0), elites_kept=[lg["elites_kept"] for lg in logs], elites_top=[lg["elites_top"] for lg in logs])
    if "togo" in ep:  # (one layout for the batch)
        res.update(_togo_settings(a0), togo_groups=[int(x) for x in ep["togo"][0]["starts"]])
    if _has_demo(a0):
        res.update(_demo_settings(a0), track_err_mean=float(ep["track_err"].mean()))
    if "zone_pen" in ep:  # (over all episodes)
        res.update(_zones_settings(a0), **zones_report(ep))
    if not a0.not_render:
        _save(a0, ep)
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    _main()
