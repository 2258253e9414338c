"""Fused XPBD rollout, emulated kernels: the specialised tile of 16 compiles its contact lanes for listed and described contacts only
(contact_item's LISTED mode; the context flags xpbd_spec_tile_fits fixes are constants there).  Every case
compares the specialised launch bit for bit with the generic instance of the same tile (NT_XPBD_CFG), which keeps every form of
contact_item, and with the call-by-call loop `clear_forces; collide; step; swap`: state, body_f, per-world contact counts, and ids + the
17 record floats of every live contact.  Scenes: tests/joint_axes_cases.py (CONTACT_SCENES: the builders of tests/record_solve_cases.py
at 17 / 20 worlds and 3 substeps); the device twin is tests/test_gpu_spec_contact_text.py."""
import numpy as np
import pytest

import joint_axes_cases as cases
import test_record_solve_emu as rs  # (its launch helpers; none of its tests are collected here)
from joint_axes_cases import CFG_GENERIC, CFG_SPEC, CONTACT_SUBSTEPS

ITERATIONS = 2


@pytest.fixture(scope="module")
def H():
    import harness

    harness.lib()
    return harness


_models, _loops = {}, {}


def _model(name):
    if name not in _models:
        scene, n = cases.CONTACT_SCENES[name]
        _models[name] = scene(n)
    return _models[name]


def _reference(H, name, substeps=CONTACT_SUBSTEPS):
    if (name, substeps) not in _loops:
        _loops[name, substeps] = rs._loop(H, _model(name), substeps, ITERATIONS)  # (computed once, never modified)
    return _loops[name, substeps]


@pytest.mark.parametrize("name", sorted(cases.CONTACT_SCENES))
def test_specialised_rollout_equals_generic_and_loop(H, name):
    model, ref = _model(name), _reference(H, name)
    assert rs._takes_spec(H, model, None, ITERATIONS) and rs._takes_spec(H, model, CFG_SPEC, ITERATIONS)  # (the specialised instance runs)
    assert not rs._takes_spec(H, model, CFG_GENERIC, ITERATIONS)
    rs._assert_same(rs._rollout(H, model, CFG_GENERIC, CONTACT_SUBSTEPS, ITERATIONS), ref)
    rs._assert_same(rs._rollout(H, model, CFG_SPEC, CONTACT_SUBSTEPS, ITERATIONS), ref)
    rs._assert_same(rs._rollout(H, model, None, CONTACT_SUBSTEPS, ITERATIONS), ref)  # (the default dispatch)


def test_disc_chain_has_more_live_contacts_than_slot_lanes(H):
    n = cases.CONTACT_SCENES["disc_chain"][1]
    assert n == 17  # one full tile and a ragged tile with a single valid world
    assert (_reference(H, "disc_chain")["env_count"][:n] == 36).all() and 36 > rs.NSLOT  # (a contact lane takes two contacts)


def test_mixed_pairs_store_both_orientations_and_a_dynamic_dynamic_pair(H):
    import record_solve_cases
    from newton_amd.enums import GeoType

    model, n = _model("mixed_pairs"), cases.CONTACT_SCENES["mixed_pairs"][1]
    pairs = record_solve_cases.stored_pair_types(model)
    cyl, plane, sphere = int(GeoType.CYLINDER), int(GeoType.PLANE), int(GeoType.SPHERE)
    assert any(ta == cyl and tb == plane for ta, tb, _, _ in pairs)  # stored against the type order: exchanged
    assert any(ta == plane and tb == cyl for ta, tb, _, _ in pairs)  # stored in type order
    assert any(ta == sphere and tb == sphere and ba >= 0 and bb >= 0 for ta, tb, ba, bb in pairs)  # no static side
    ref = _reference(H, "mixed_pairs")
    body = np.asarray(model.shape_body)
    live = ref["shape0"] >= 0
    assert ((body[ref["shape0"][live]] >= 0) & (body[ref["shape1"][live]] >= 0)).any()  # the dynamic-dynamic pair is live
    assert n == 20 and ref["env_count"][:n].min() >= 12


def test_worlds_gain_contacts_inside_the_launch_and_a_kinematic_body_is_in_contact(H):
    from newton_amd.enums import BodyFlags

    model, n = _model("gaining"), cases.CONTACT_SCENES["gaining"][1]
    counts = [_reference(H, "gaining", s)["env_count"][:n] for s in (1, 2, 3)]
    assert (counts[0] == 0).any() and (counts[0] >= 3).any()  # worlds without a live contact beside worlds with several, in one tile
    assert (counts[1] > counts[0]).any() and (counts[2] > counts[1]).any()  # contacts that appear for the second and the third substep
    flags = np.asarray(model.env.body_flags)
    assert (flags & int(BodyFlags.KINEMATIC) != 0).sum() == 1
    kin = int(np.flatnonzero(flags & int(BodyFlags.KINEMATIC))[0])
    ref, nb = _reference(H, "gaining"), model.body_count // n
    body = np.asarray(model.shape_body)
    live = (ref["shape0"] >= 0) & (ref["shape1"] >= 0)
    b0, b1 = body[ref["shape0"][live]], body[ref["shape1"][live]]
    assert ((b0 % nb == kin) | (b1 % nb == kin)).any()  # the platform carries its rider: a live contact with a kinematic body
