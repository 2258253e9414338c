"""Fused XPBD rollout on the device: what gather_axes (nt_xpbd.hpp) makes of a joint's axes -- limits, drives, targets -- on the three
paths that must agree.  Every case compares the specialised launch of the tile of 16 bit for bit with the generic instance of the same
tile (NT_XPBD_CFG) and with the call-by-call loop `clear_forces; collide; step; swap`: state, body_f, per-world contact counts, and ids
+ the 17 record floats of every live contact.  No tolerance anywhere.

THIS file decides bit equality: gather_axes contracts `tp += wa * target_pos`, the joint items contract around what it returns, and
which product of a sum is fused is the device compiler's choice per instance; the emulated twin (tests/test_joint_axes_emu.py)
compiles without contraction.  Keeping a joint lane's AxisData in LDS for a launch passed there and failed here
(profiles/axis_rows_bisect.txt).  Scenes: tests/joint_axes_cases.py."""
import numpy as np
import pytest

import joint_axes_cases as cases
import test_gpu_joint_roles as jr  # (its simulation helpers; none of its tests are collected here)
from joint_axes_cases import CFG_GENERIC, CFG_SPEC, DT, FLAT

pytestmark = pytest.mark.gpu
_Sim, _assert_same, _three, _compare, _cfg = jr._Sim, jr._assert_same, jr._three, jr._compare, jr._cfg
_models = {}


def _model(name):
    if name not in _models:
        _models[name] = cases.SCENES[name][0](cases.SCENES[name][1], device="cuda:0")
    return _models[name]


@pytest.mark.parametrize("name", sorted(cases.SCENES))
def test_specialised_rollout_equals_generic_and_loop(name):
    """(asserts that the specialised instance ran, and that a joint of every live type corrected something)"""
    _compare(_model(name), cases.SCENES[name][2])


def test_targets_that_differ_from_world_to_world():
    """every world drives every axis to a target of its own (position and velocity): a row shared by the worlds of a tile by mistake
    would give all of them the first world's"""
    model, (n, substeps) = _model("axes"), cases.SCENES["axes"][1:]
    f, tq, tqd = cases.controls(model, n, 0)
    nd = model.joint_dof_count // n
    sims = _three(model)
    for s in sims:
        s.set_controls(f, tq, tqd)
    ref, generic, spec = (s.launch(substeps) for s in sims)
    _assert_same(generic, ref)
    _assert_same(spec, ref)
    same = _Sim(model, CFG_GENERIC)  # the first world's targets in every world: something else
    same.set_controls(f, np.tile(tq.reshape(n, -1)[0], n), np.tile(tqd.reshape(n, nd)[0], n))
    assert not np.array_equal(same.launch(substeps)["body_qd"], ref["body_qd"])


def test_two_launches_with_other_targets():
    """the second launch of a model runs with other targets: nothing of the first launch's lives on"""
    model, (n, substeps) = _model("axes"), cases.SCENES["axes"][1:]
    sims = _three(model)
    second = None
    for v in (0, 1):
        for s in sims:
            s.set_controls(*cases.controls(model, n, v))
        ref, generic, spec = (s.launch(substeps) for s in sims)
        _assert_same(generic, ref)
        _assert_same(spec, ref)
        second = ref
    stale = _Sim(model, CFG_GENERIC)  # what a launch that kept the first controls would give: something else
    stale.set_controls(*cases.controls(model, n, 0))
    stale.launch(substeps)
    assert not np.array_equal(stale.launch(substeps)["body_qd"], second["body_qd"])


def test_captured_graph_replayed_after_the_targets_were_changed_in_place():
    """one captured launch of the specialised instance, replayed with the first targets and then with others written into the same
    device buffers: each replay equals the generic instance's eager launch with those targets"""
    import torch

    import newton_amd as nt

    model, (n, substeps) = _model("axes"), cases.SCENES["axes"][1:]
    assert substeps % 2 == 1  # (the launch leaves the state in s1: each frame swaps, as the eager sims do)
    generic, spec = _Sim(model, CFG_GENERIC), _Sim(model, CFG_SPEC)
    for s in (generic, spec):
        s.set_controls(*cases.controls(model, n, 0))

    def frame():  # s0 -> s1, then s1 back into s0: the captured buffers are the same in every replay
        spec.solver.rollout(spec.s0, spec.s1, spec.ctrl, spec.ct, DT, substeps)
        spec.s0.assign(spec.s1)

    with _cfg(CFG_SPEC):
        assert spec.takes_spec(CFG_SPEC)
        g = nt.graph.capture(frame, warmup=0, contacts=spec.ct)  # (the capture launches nothing: the replays do)
        for v in (0, 1):
            for s in (generic, spec):
                s.set_controls(*cases.controls(model, n, v))
            g.launch()
            torch.cuda.synchronize()
            ref, got = generic.launch(substeps), spec.snapshot()
            for k in ("body_q", "body_qd", "env_count", "count", *FLAT):
                assert np.array_equal(got[k], ref[k]), (v, k)


def test_uniform_edits_of_a_limit_and_a_stiffness_equal_a_fresh_model():
    """A joint limit moved, then a drive's stiffness changed, the same in every world, each through notify_model_changed with a launch
    after it.  Each launch equals, bit for bit, the launch of a model built anew with those values (set before it first reaches the
    device) from the same state; and each edit alone reaches the device: a model one edit behind gives something else."""
    n, substeps = cases.SCENES["axes"][1:]
    model, lag_model = cases.axes_scene(n, device="cuda:0"), cases.axes_scene(n, device="cuda:0")  # (edited in place)
    sims, lagging = _three(model), _Sim(lag_model, CFG_GENERIC)
    ref, generic, spec = (s.launch(substeps) for s in sims)
    _assert_same(generic, ref)
    _assert_same(spec, ref)
    for k, which in enumerate(cases.AXIS_EDITS):
        if k:  # (the lagging model follows one edit behind)
            cases.edit_axes(lag_model, n, cases.AXIS_EDITS[k - 1])
            jr._notify(lagging)
        fresh_model = cases.axes_scene(n, device="cuda:0")
        for w in cases.AXIS_EDITS[: k + 1]:
            cases.edit_axes(fresh_model, n, w)
        fresh = _Sim(fresh_model, CFG_GENERIC)
        for s in (lagging, fresh):
            s.s0.assign(sims[1].s0)
        cases.edit_axes(model, n, which)
        jr._notify(sims[0])
        assert sims[2].takes_spec(None)
        ref, generic, spec = (s.launch(substeps) for s in sims)
        _assert_same(generic, ref)
        _assert_same(spec, ref)
        _assert_same(spec, fresh.launch(substeps))
        assert not np.array_equal(lagging.launch(substeps)["body_qd"], ref["body_qd"]), which


def test_seventeen_joints_take_the_generic_instance_and_sixteen_the_specialised():
    """16 joints fill the 32 joint lanes of the tile; a loop-closing 17th keeps the generic instance, and asking for the specialised one is
    refused"""
    closed = cases.ring_scene(cases.RING_WORLDS, device="cuda:0", closed=True)
    open_ = cases.ring_scene(cases.RING_WORLDS, device="cuda:0", closed=False)
    assert (closed.env.nj, open_.env.nj) == (17, 16)
    loop, rollout = _Sim(closed, None, loop=True), _Sim(closed, None)
    shape = rollout.shape(None)
    assert shape[:4] == [16, 512, 1, 1] and not shape[4] & cases.SPEC_BIT
    with pytest.raises(Exception):
        _Sim(closed, CFG_SPEC).launch(cases.RING_SUBSTEPS)
    _assert_same(rollout.launch(cases.RING_SUBSTEPS), loop.launch(cases.RING_SUBSTEPS))
    _compare(open_, cases.RING_SUBSTEPS)  # (asserts that the specialised instance is taken)
