"""Fused XPBD rollout on the device: the specialised tile of 16 compiles its contact lanes for listed and described contacts only
(contact_item's LISTED mode; the context flags xpbd_spec_tile_fits fixes are constants there).  Every case
compares the specialised launch bit for bit with the generic instance of the same tile (NT_XPBD_CFG), which keeps every form of
contact_item, and with the call-by-call loop `clear_forces; collide; step; swap`: state, body_f, per-world contact counts, and ids + the
17 record floats of every live contact.  Scenes: tests/joint_axes_cases.py (CONTACT_SCENES: the builders of tests/record_solve_cases.py
at 17 / 20 worlds and 3 substeps); the emulated twin is tests/test_spec_contact_text_emu.py."""
import numpy as np
import pytest

import joint_axes_cases as cases
import test_gpu_record_solve as rs  # (its launch helpers; none of its tests are collected here)
from joint_axes_cases import CFG_GENERIC, CFG_SPEC, CONTACT_SUBSTEPS

pytestmark = pytest.mark.gpu
ITERATIONS = 2
_sims, _loops = {}, {}


def _sim(name):
    if name not in _sims:
        scene, n = cases.CONTACT_SCENES[name]
        _sims[name] = rs._Sim(scene(n, device="cuda:0"), ITERATIONS)
    return _sims[name]


def _reference(name, substeps=CONTACT_SUBSTEPS):
    if (name, substeps) not in _loops:
        _loops[name, substeps] = _sim(name).loop(substeps)  # (computed once, never modified)
    return _loops[name, substeps]


@pytest.mark.parametrize("name", sorted(cases.CONTACT_SCENES))
def test_specialised_rollout_equals_generic_and_loop(name):
    sim, ref = _sim(name), _reference(name)
    assert sim.takes_spec(None) and sim.takes_spec(CFG_SPEC) and not sim.takes_spec(CFG_GENERIC)  # (the specialised instance runs)
    rs._assert_same(sim.rollout(CFG_GENERIC, CONTACT_SUBSTEPS), ref)
    rs._assert_same(sim.rollout(CFG_SPEC, CONTACT_SUBSTEPS), ref)
    rs._assert_same(sim.rollout(None, CONTACT_SUBSTEPS), ref)  # (the default dispatch)


def test_the_scenes_are_what_they_are_for():
    """more live contacts than slot lanes; a live pair without a static side; worlds that gain contacts for the second and for the third
    substep beside worlds without any, and a live contact on the kinematic platform"""
    from newton_amd.enums import BodyFlags

    n = cases.CONTACT_SCENES["disc_chain"][1]
    assert (rs._per_env(_reference("disc_chain")[2])[:n] == 36).all() and 36 > rs.NSLOT
    model, ct = _sim("mixed_pairs").model, _reference("mixed_pairs")[2]
    body = np.asarray(model.shape_body)
    s0, s1 = ct.rigid_contact_shape0.cpu().numpy(), ct.rigid_contact_shape1.cpu().numpy()
    live = s0 >= 0
    assert ((body[s0[live]] >= 0) & (body[s1[live]] >= 0)).any()
    model, n = _sim("gaining").model, cases.CONTACT_SCENES["gaining"][1]
    counts = [rs._per_env(_reference("gaining", s)[2])[:n].copy() for s in (1, 2, 3)]
    assert (counts[0] == 0).any() and (counts[0] >= 3).any()
    assert (counts[1] > counts[0]).any() and (counts[2] > counts[1]).any()
    flags, nb = np.asarray(model.env.body_flags), model.body_count // n
    kin = int(np.flatnonzero(flags & int(BodyFlags.KINEMATIC))[0])
    ct, body = _reference("gaining")[2], np.asarray(model.shape_body)
    s0, s1 = ct.rigid_contact_shape0.cpu().numpy(), ct.rigid_contact_shape1.cpu().numpy()
    live = (s0 >= 0) & (s1 >= 0)
    assert ((body[s0[live]] % nb == kin) | (body[s1[live]] % nb == kin)).any()
