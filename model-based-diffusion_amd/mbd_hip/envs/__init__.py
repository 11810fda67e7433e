"""Env registry — drop-in for ``mbd.envs.get_env`` (mbd/envs/__init__.py:13-33) on the hot path."""
from __future__ import annotations

from . import specs
from .base import Car2d, RigidBodyEnv, State

__all__ = ["get_env", "builtin_model", "State", "Car2d", "RigidBodyEnv"]


def builtin_model(env_name: str):
    """The compiled model the library embeds under ``env_name`` as a ``Model`` (host only: no device is looked for)."""
    import ctypes as C

    from .. import _capi
    from ..model import MbdModel, Model
    from .base import _names
    st = MbdModel()
    _capi.check(_capi.load().mbd_builtin_model(env_name.encode(), C.byref(st)))
    return Model.from_struct(st, *_names(env_name), env_name=env_name)


def get_env(env_name: str, device: int = 0, track=()):
    """Same contract as the reference: a string in, an env object out, ``ValueError`` on an unknown
    name.  Every name the reference's registry knows resolves — car2d, humanoidrun, humanoidtrack, humanoidstandup, hopper,
    halfcheetah, walker2d, cartpole, ant — except pushT (Brax's generalized backend: another physics engine).
    ``track``: link names or positions — the built-in model retracked (``Model.tracked``), what a zone record measures; car2d and
    the planar models raise ``ValueError``.  Empty: the built-in env as it is."""
    track = tuple(track)
    if env_name == "car2d":
        if track:
            raise ValueError("car2d has no links to track")
        return Car2d(device=device)
    if env_name in specs.SPECS:
        if track:
            return RigidBodyEnv(env_name, device=device, model=builtin_model(env_name).tracked(track))
        return RigidBodyEnv(env_name, device=device)
    if env_name in specs.OUT_OF_SCOPE:
        raise ValueError(f"Environment {env_name!r} is known to the reference but outside the MI355X "
                         f"hot-path scope of mbd_hip (SURVEY.md §2)")
    raise ValueError(f"Unknown environment: {env_name}")
