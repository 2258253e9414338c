"""Fused XPBD rollout, emulated kernels: what gather_axes (nt_xpbd.hpp) makes of a joint's axes -- limits, drives, targets -- on the three
paths that must agree.  Every case compares the specialised launch of the tile of 16 bit for bit with the generic instance of the same
tile (NT_XPBD_CFG) and with the call-by-call loop `clear_forces; collide; step; swap`: state, body_f, per-world contact counts, and ids
+ the 17 record floats of every live contact.  No tolerance anywhere.  Scenes: tests/joint_axes_cases.py -- every count of axes, axes
that point the negative way, every mix of stiffness and damping, velocity targets, targets that differ from world to world, a disabled
joint, a world-attached parent; the device twin is tests/test_gpu_joint_axes.py, which adds the captured graph and which alone sees
what contraction makes of the kernels' arithmetic.

These are the scenes on which keeping a joint lane's AxisData in LDS for a launch ("joint axis rows") left the
generic instance by ulps on the device while this file passed (profiles/axis_rows_bisect.txt); the rows were dropped, the scenes stay
for whoever takes gather_axes off the per-call path next.  The emulated tiles poison their LDS: a row read before it is written, or by a
lane that does not own it, shows here."""
import copy

import numpy as np
import pytest

import joint_axes_cases as cases
import test_joint_roles_emu as jr  # (its simulation helpers; none of its tests are collected here)
from joint_axes_cases import CFG_GENERIC

_Sim, _assert_same, _bits, _three, _compare, _takes_spec, _shape = (jr._Sim, jr._assert_same, jr._bits, jr._three, jr._compare, jr._takes_spec,
                                                                    jr._shape)


@pytest.fixture(scope="module")
def H():
    import harness

    harness.lib()
    return harness


_models = {}


def _model(name):
    if name not in _models:
        _models[name] = cases.SCENES[name][0](cases.SCENES[name][1])
    return _models[name]


def test_the_scene_holds_what_gather_axes_tells_apart():
    model, n = _model("axes"), cases.SCENES["axes"][1]
    for fact, holds in cases.describe(model.env).items():
        assert holds, fact
    d = cases.drive_mixes(model, n)
    assert d.pop("mixes") == {(True, True), (True, False), (False, True), (False, False)}
    for fact, holds in d.items():
        assert holds, fact


@pytest.mark.parametrize("name", sorted(cases.SCENES))
def test_specialised_rollout_equals_generic_and_loop(H, name):
    """(asserts that the specialised instance ran, and that a joint of every live type corrected something)"""
    _compare(H, _model(name), cases.SCENES[name][2])


def test_targets_that_differ_from_world_to_world(H):
    """every world drives every axis to a target of its own (position and velocity): a row shared by the worlds of a tile by mistake
    would give all of them the first world's"""
    model, (n, substeps) = _model("axes"), cases.SCENES["axes"][1:]
    f, tq, tqd = cases.controls(model, n, 0)
    nd = model.joint_dof_count // n
    assert len(np.unique(tqd.reshape(n, nd)[:, 0])) == n and len(np.unique(tq.reshape(n, -1)[:, 0])) == n
    sims = _three(H, model)
    for s in sims:
        s.set_controls(f, tq, tqd)
    ref, generic, spec = (s.launch(substeps) for s in sims)
    _assert_same(generic, ref)
    _assert_same(spec, ref)
    same = _Sim(H, model, CFG_GENERIC)  # the first world's targets in every world: something else
    same.set_controls(f, np.tile(tq.reshape(n, -1)[0], n), np.tile(tqd.reshape(n, nd)[0], n))
    assert not np.array_equal(_bits(same.launch(substeps)["body_qd"]), _bits(ref["body_qd"]))


def test_two_launches_with_other_targets(H):
    """the second launch of a model runs with other targets: nothing of the first launch's lives on"""
    model, (n, substeps) = _model("axes"), cases.SCENES["axes"][1:]
    sims = _three(H, model)
    second = None
    for v in (0, 1):
        for s in sims:
            s.set_controls(*cases.controls(model, n, v))
        ref, generic, spec = (s.launch(substeps) for s in sims)
        _assert_same(generic, ref)
        _assert_same(spec, ref)
        second = ref
    stale = _Sim(H, model, CFG_GENERIC)  # what a launch that kept the first controls would give: something else
    stale.set_controls(*cases.controls(model, n, 0))
    stale.launch(substeps)
    assert not np.array_equal(_bits(stale.launch(substeps)["body_qd"]), _bits(second["body_qd"]))


def test_uniform_edits_of_a_limit_and_a_stiffness_equal_a_fresh_model(H):
    """A joint limit moved, then a drive's stiffness changed, the same in every world, a launch after each.  Each launch equals, bit for
    bit, the launch of a model built anew with those values from the same state; and each edit alone reaches the kernels: the model
    without it gives something else."""
    n, substeps = cases.SCENES["axes"][1:]
    model = cases.axes_scene(n)  # (a model of its own: edited in place)
    sims = _three(H, model)
    ref, generic, spec = (s.launch(substeps) for s in sims)
    _assert_same(generic, ref)
    _assert_same(spec, ref)
    for k, which in enumerate(cases.AXIS_EDITS):
        lagging = _Sim(H, copy.deepcopy(model), CFG_GENERIC)  # (the model without this edit, on the state the others start from)
        lagging.copy_state(sims[1])
        cases.edit_axes(model, n, which)
        fresh_model = cases.axes_scene(n)
        for w in cases.AXIS_EDITS[: k + 1]:
            cases.edit_axes(fresh_model, n, w)
        fresh = _Sim(H, fresh_model, CFG_GENERIC)
        fresh.copy_state(sims[1])
        for s in sims:
            s.set_model(model)
        assert _takes_spec(H, model, None)
        ref, generic, spec = (s.launch(substeps) for s in sims)
        _assert_same(generic, ref)
        _assert_same(spec, ref)
        _assert_same(spec, fresh.launch(substeps))
        assert not np.array_equal(_bits(lagging.launch(substeps)["body_qd"]), _bits(ref["body_qd"])), which


def test_seventeen_joints_take_the_generic_instance_and_sixteen_the_specialised(H):
    """16 joints fill the 32 joint lanes of the tile; a loop-closing 17th keeps the generic instance, and asking for the specialised one is
    refused"""
    closed, open_ = cases.ring_scene(cases.RING_WORLDS, closed=True), cases.ring_scene(cases.RING_WORLDS, closed=False)
    assert (closed.env.nj, open_.env.nj) == (17, 16)
    shape = _shape(H, closed, None)
    assert shape[:4] == [16, 512, 1, 1] and not shape[4] & cases.SPEC_BIT
    with pytest.raises(Exception):
        _Sim(H, closed, cases.CFG_SPEC).launch(cases.RING_SUBSTEPS)
    loop, rollout = _Sim(H, closed, None, loop=True), _Sim(H, closed, None)
    _assert_same(rollout.launch(cases.RING_SUBSTEPS), loop.launch(cases.RING_SUBSTEPS))
    _compare(H, open_, cases.RING_SUBSTEPS)  # (asserts that the specialised instance is taken)
