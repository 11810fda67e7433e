"""Which models run the instantiations with the unit inverse inertia compiled in: csrc/mbd_env.hip::choose_rollout through
mbd_debug_rollout_choice, no device, 256 compute units.

The instantiations of rollout_kernel and rollout_pk2_kernel that compile in humanoidrun's or humanoidtrack's reward kind and
n_frames compile in that model's inv_inertia = (1, 1, 1, 0, 0, 0) as well (mbd_kernels.h unit_inertia_form): the built-in
models get them, one candidate per lane (B = 1024) and two (B = 8192).  A model whose inverse inertia is anything else —
every link scaled, or one link's diagonal alone — gets the same instantiation of rollout_kernel_rtib / rollout_pk2_kernel_rtib,
which reads it from the lane records, and so does every model under the lever MBD_NO_UNIT_CONST.  (The elasticity is NOT part
of the choice: the kernels read it at run time in both forms.)"""
import numpy as np
import pytest

from conftest import load_model

N_CUS, H = 256, 50
HUMANOIDS = {"humanoidrun": "0, 7", "humanoidtrack": "3, 5"}  # reward kind, n_frames as the instantiations spell them


def _names(rk_nfr, unit):
    """(3-D, two-per-lane) instantiation of a built-in humanoid at B = 1024 and B = 8192."""
    twin = "" if unit else "_rtib"
    targs = f"16, true, false, 3, 1, 1, -4, -6, 0, false, true, 3, false, false, {rk_nfr}, false, false, false"
    return (f"void mbd::rollout_kernel{twin}<{targs}>(mbd::RolloutParams)",
            f"void mbd::rollout_pk2_kernel{twin}<1, {rk_nfr}, 1, 0>(mbd::RolloutParams)")


def _choice(m, B):
    from mbd_hip import _capi
    return _capi.debug_rollout_choice(m.to_struct(), N_CUS, B, H)["name"]


def _one_link_halved(name):
    m = load_model(name)
    ib = np.array(m.fields["inv_inertia"], np.float32)
    ib[m.n_links // 2, 0:3] = 0.5
    m.fields["inv_inertia"] = ib
    return m


def _elastic(name):
    m = load_model(name)
    m.fields["elasticity"] = 0.25
    return m


@pytest.mark.parametrize("name", sorted(HUMANOIDS))
def test_the_builtin_humanoids_have_unit_inverse_inertia(name):
    m = load_model(name)
    ib = np.asarray(m.fields["inv_inertia"], np.float32)[:m.n_links]
    assert int(m.fields["iso_inertia"]) == 1 and np.all(ib[:, :3] == 1.0) and not ib[:, 3:].any()


@pytest.mark.parametrize("name", sorted(HUMANOIDS))
def test_stock_humanoids_run_the_unit_forms(lib, name):
    want3d, want_pk2 = _names(HUMANOIDS[name], unit=True)
    m = load_model(name)
    assert _choice(m, 1024) == want3d
    assert _choice(m, 8192) == want_pk2


@pytest.mark.parametrize("name", sorted(HUMANOIDS))
def test_an_elastic_humanoid_still_runs_the_unit_forms(lib, name):
    """Only the inverse inertia is compiled in; the restitution term reads the model's elasticity in both forms."""
    want3d, want_pk2 = _names(HUMANOIDS[name], unit=True)
    assert _choice(_elastic(name), 1024) == want3d
    assert _choice(_elastic(name), 8192) == want_pk2


@pytest.mark.parametrize("name", sorted(HUMANOIDS))
@pytest.mark.parametrize("variant", ["scaled", "one_link"])
def test_other_inertias_run_the_general_forms(lib, name, variant):
    want3d, want_pk2 = _names(HUMANOIDS[name], unit=False)
    m = load_model(name).scaled(mass=1.25) if variant == "scaled" else _one_link_halved(name)
    assert _choice(m, 1024) == want3d
    assert _choice(m, 8192) == want_pk2


@pytest.mark.parametrize("name", sorted(HUMANOIDS))
def test_the_lever_gives_the_general_forms(lib, levers, name):
    from mbd_hip import _capi
    assert "MBD_NO_UNIT_CONST" in _capi.LEVERS and _capi.debug_get("MBD_NO_UNIT_CONST") == -1
    want3d, want_pk2 = _names(HUMANOIDS[name], unit=False)
    levers(MBD_NO_UNIT_CONST=1)
    for m in (load_model(name), load_model(name).scaled(mass=1.25), _one_link_halved(name), _elastic(name)):
        assert _choice(m, 1024) == want3d
        assert _choice(m, 8192) == want_pk2
    levers(MBD_NO_UNIT_CONST=0)  # (only 1 switches the forms off)
    assert _choice(load_model(name), 1024) == _names(HUMANOIDS[name], unit=True)[0]
