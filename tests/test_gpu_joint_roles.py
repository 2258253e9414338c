"""Fused XPBD rollout on the device: on the specialised tile of 16 a joint lane keeps the launch-invariant operands of its joint in
registers (lane roles, nt_ctx.hpp: JointRole).  Every case compares the specialised launch bit for bit with the
generic instance of the same tile (NT_XPBD_CFG) and with the call-by-call loop `clear_forces; collide; step; swap`: state, body_f,
per-world contact counts, and ids + the 17 record floats of every live contact.  No tolerance anywhere.

THIS file decides bit equality.  The emulated twin (tests/test_joint_roles_emu.py) compiles the kernels without contraction and agreed
with the generic instance for a joint role that, on the device, left it by an ulp: which product of a sum of two products is fused is
the device compiler's choice per instance.  Scenes: tests/lane_roles_cases.py and tests/joint_roles_cases.py."""
import ctypes as C
import os

import numpy as np
import pytest

import joint_roles_cases as cases
from joint_roles_cases import CFG_GENERIC, CFG_SPEC, DT, FLAT, SPEC_BIT

pytestmark = pytest.mark.gpu


class _cfg:
    def __init__(self, cfg):
        self.cfg = cfg

    def __enter__(self):
        self.old = os.environ.pop("NT_XPBD_CFG", None)
        if self.cfg:
            os.environ["NT_XPBD_CFG"] = self.cfg

    def __exit__(self, *exc):
        os.environ.pop("NT_XPBD_CFG", None)
        if self.old is not None:
            os.environ["NT_XPBD_CFG"] = self.old


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


class _Sim:
    """one model's states, Contacts and Control, stepped launch after launch on path `cfg` (loop: the call-by-call loop)"""

    def __init__(self, model, cfg, loop=False, iterations=2):
        import newton_amd as nt

        self.model, self.cfg, self.loop = model, cfg, loop
        self.solver, self.pipe = nt.solvers.SolverXPBD(model, iterations=iterations), nt.CollisionPipeline(model)
        self.ctrl, self.ct = model.control(), self.pipe.contacts()
        self.s0, self.s1 = model.state(), model.state()
        f = np.ones((model.body_count, 6), dtype=np.float32)
        self.s0.body_f, self.s1.body_f = f, 2.0 * f  # (the launch leaves both as clear_forces does, whatever they held)

    def set_controls(self, f, tq, tqd):  # (in place: the device buffers a captured graph holds stay where they are)
        self.ctrl.joint_f, self.ctrl.joint_target_q, self.ctrl.joint_target_qd = f, tq, tqd

    def launch(self, substeps):
        if self.loop:
            for _ in range(substeps):
                self.s0.clear_forces()
                self.pipe.collide(self.s0, self.ct)
                self.solver.step(self.s0, self.s1, self.ctrl, self.ct, DT)
                self.s0, self.s1 = self.s1, self.s0
            self.s0.clear_forces()
            self.s1.clear_forces()
        else:
            with _cfg(self.cfg):
                out = self.solver.rollout(self.s0, self.s1, self.ctrl, self.ct, DT, substeps)
            if out is self.s1:
                self.s0, self.s1 = self.s1, self.s0
        return self.snapshot()

    def snapshot(self):
        r = {"body_q": _bits(self.s0.body_q), "body_qd": _bits(self.s0.body_qd), "count": _bits(self.ct.rigid_contact_count),
             "env_count": self.ct.rigid_contact_count_per_env.cpu().numpy().copy(),
             "body_f": np.stack([self.s0.body_f.cpu().numpy(), self.s1.body_f.cpu().numpy()])}
        for k in FLAT:
            r[k] = _bits(getattr(self.ct, "rigid_contact_" + k))
        return r

    def shape(self, cfg):
        dm, out, p = self.model.device_model(), (C.c_int32 * 5)(), self.solver._params()
        with _cfg(cfg):
            assert dm.lib.nt_xpbd_rollout_shape(C.byref(dm.desc), C.byref(p), None, out) == 0
        return list(out)

    def takes_spec(self, cfg):
        out = self.shape(cfg)
        return out[:4] == [16, 512, 1, 1] and bool(out[4] & SPEC_BIT)


def _assert_same(got, ref):
    assert np.isfinite(ref["body_q"].view(np.float32)).all()
    for k in ("body_q", "body_qd", "env_count", "count", *FLAT):
        assert np.array_equal(got[k], ref[k]), k
    assert not got["body_f"].any() and not ref["body_f"].any()


def _joint_corrections(model, iterations, substeps):
    """[worlds, 6, nj]: the largest magnitude, over `substeps` reporting steps from the scene's first state, of the child-side
    corrections a step accumulates per joint (default control: no joint_f, so the feed-forward part is zero).  A state with
    body_parent_f makes the step kernel keep them."""
    import newton_amd as nt

    requested = set(model.get_requested_state_attributes())
    model.request_state_attributes("body_parent_f")
    try:
        s0, s1 = model.state(), model.state()
    finally:
        model._requested_state_attributes = requested
    solver, pipe = nt.solvers.SolverXPBD(model, iterations=iterations), nt.CollisionPipeline(model)
    ct, ctrl, t, seen = pipe.contacts(), model.control(), model.env, 0.0
    for _ in range(substeps):
        s0.clear_forces()
        pipe.collide(s0, ct)
        solver.step(s0, s1, ctrl, ct, DT)
        s0, s1 = s1, s0
        seen = np.maximum(seen, np.abs(solver._joint_impulse.cpu().numpy()))
    return seen[:, : t.nj, : t.env_count].transpose(2, 0, 1)


_models = {}


def _model(name):
    if name not in _models:
        _models[name] = cases.SCENES[name][0](cases.SCENES[name][1], device="cuda:0")
    return _models[name]


def _three(model, iterations=2):
    """(loop, generic, specialised) -- and the specialised instance is really the one the last of them runs"""
    sims = _Sim(model, None, loop=True, iterations=iterations), _Sim(model, CFG_GENERIC, iterations=iterations), _Sim(model, CFG_SPEC, iterations=iterations)
    assert sims[2].takes_spec(None) and sims[2].takes_spec(CFG_SPEC) and not sims[2].takes_spec(CFG_GENERIC)
    return sims


def _compare(model, substeps, iterations=2):
    cases.assert_every_live_type_corrects(model.env, _joint_corrections(model, iterations, substeps))  # (the joint lanes have work)
    loop, generic, spec = _three(model, iterations)
    ref = loop.launch(substeps)
    _assert_same(generic.launch(substeps), ref)
    _assert_same(spec.launch(substeps), ref)
    _assert_same(_Sim(model, None, iterations=iterations).launch(substeps), ref)  # (the default dispatch)


@pytest.mark.parametrize("name", sorted(cases.SCENES))
def test_specialised_rollout_equals_generic_and_loop(name):
    _compare(_model(name), cases.SCENES[name][2])


@pytest.mark.parametrize("iterations", [1, 2, 3])
def test_chain_of_five_at_one_two_and_three_iterations(iterations):
    """(the drift of the first joint role showed on this chain after two substeps)"""
    _compare(_model("chain5"), cases.SCENES["chain5"][2], iterations)


def test_two_launches_with_other_targets():
    """the second launch of a model runs with other joint_f / joint_target_q / joint_target_qd: nothing of the first launch's lives on"""
    model, (n, substeps) = _model("zoo"), cases.SCENES["zoo"][1:]
    sims = _three(model)
    second = None
    for v in (0, 1):
        for s in sims:
            s.set_controls(*cases.base.controls(model, n, v))
        ref, generic, spec = (s.launch(substeps) for s in sims)
        _assert_same(generic, ref)
        _assert_same(spec, ref)
        second = ref
    stale = _Sim(model, CFG_GENERIC)  # what a launch that kept the first controls would give: something else
    stale.set_controls(*cases.base.controls(model, n, 0))
    stale.launch(substeps)
    assert not np.array_equal(stale.launch(substeps)["body_qd"], second["body_qd"])


def _notify(sim):
    import newton_amd as nt

    F = nt.ModelFlags
    sim.solver.notify_model_changed(F.JOINT_PROPERTIES | F.JOINT_DOF_PROPERTIES)


def test_a_joint_edit_between_launches_equals_a_fresh_model_with_that_edit():
    """The prismatic joint disabled, then enabled again, then a joint limit moved, each through notify_model_changed with a launch
    after it.  Each launch equals, bit for bit, the launch of a model built anew with the same edits (made before it first reaches
    the device) from the same state: the record is refilled per launch.  And each edit alone reaches the device: a model one edit
    behind gives something else."""
    n, substeps = cases.SCENES["zoo"][1:]
    model, lag_model = cases.base.zoo_scene(n, device="cuda:0"), cases.base.zoo_scene(n, device="cuda:0")  # (edited in place)
    sims, lagging = _three(model), _Sim(lag_model, CFG_GENERIC)
    ref, generic, spec = (s.launch(substeps) for s in sims)
    _assert_same(generic, ref)
    _assert_same(spec, ref)
    for k, which in enumerate(cases.JOINT_EDITS):
        if k:  # (the lagging model follows one edit behind)
            cases.edit_joint(lag_model, n, cases.JOINT_EDITS[k - 1])
            _notify(lagging)
        fresh_model = cases.base.zoo_scene(n, device="cuda:0")
        for w in cases.JOINT_EDITS[: k + 1]:
            cases.edit_joint(fresh_model, n, w)
        fresh = _Sim(fresh_model, CFG_GENERIC)
        assert int(fresh_model.env.joint_enabled[cases.ZOO_PRISMATIC_JOINT]) == (0 if which == "disable_prismatic" else 1)
        for s in (lagging, fresh):
            s.s0.assign(sims[1].s0)
        cases.edit_joint(model, n, which)
        _notify(sims[0])
        assert sims[2].takes_spec(None)
        ref, generic, spec = (s.launch(substeps) for s in sims)
        _assert_same(generic, ref)
        _assert_same(spec, ref)
        _assert_same(spec, fresh.launch(substeps))
        assert not np.array_equal(lagging.launch(substeps)["body_qd"], ref["body_qd"]), which


def test_captured_graph_replayed_after_a_change_of_targets():
    """one captured launch of the specialised instance, replayed with the first controls and then with others written into the same
    device buffers: each replay equals the generic instance's eager launch with those controls"""
    import torch

    import newton_amd as nt

    model, (n, substeps) = _model("zoo"), cases.SCENES["zoo"][1:]
    assert substeps % 2 == 1  # (the launch leaves the state in s1: each frame swaps, as the eager sims do)
    generic, spec = _Sim(model, CFG_GENERIC), _Sim(model, CFG_SPEC)
    for s in (generic, spec):
        s.set_controls(*cases.base.controls(model, n, 0))

    def frame():  # s0 -> s1, then s1 back into s0: the captured buffers are the same in every replay
        spec.solver.rollout(spec.s0, spec.s1, spec.ctrl, spec.ct, DT, substeps)
        spec.s0.assign(spec.s1)

    with _cfg(CFG_SPEC):
        assert spec.takes_spec(CFG_SPEC)
        g = nt.graph.capture(frame, warmup=0, contacts=spec.ct)  # (the capture launches nothing: the replays do)
        for v in (0, 1):
            for s in (generic, spec):
                s.set_controls(*cases.base.controls(model, n, v))
            g.launch()
            torch.cuda.synchronize()
            ref, got = generic.launch(substeps), spec.snapshot()
            for k in ("body_q", "body_qd", "env_count", "count", *FLAT):
                assert np.array_equal(got[k], ref[k]), (v, k)


def test_seventeen_joints_take_the_generic_instance_and_sixteen_the_specialised():
    """xpbd_spec_tile_fits: wave_up(nj) + nj <= nslot, so that a joint lane makes one trip and its record is its joint's.  16 joints fill
    the 32 slots; a loop-closing 17th (nb stays 16: every other fact holds) keeps the generic instance, and asking for the specialised
    one is refused."""
    closed = cases.ring_scene(cases.RING_WORLDS, device="cuda:0", closed=True)
    open_ = cases.ring_scene(cases.RING_WORLDS, device="cuda:0", closed=False)
    assert (closed.env.nj, closed.env.nb, open_.env.nj) == (17, 16, 16)
    cases.assert_every_live_type_corrects(closed.env, _joint_corrections(closed, 2, cases.RING_SUBSTEPS))  # (the closing joint pulls)
    loop, rollout = _Sim(closed, None, loop=True), _Sim(closed, None)
    shape = rollout.shape(None)
    assert shape[:4] == [16, 512, 1, 1] and not shape[4] & SPEC_BIT
    with pytest.raises(Exception):
        _Sim(closed, CFG_SPEC).launch(cases.RING_SUBSTEPS)
    _assert_same(rollout.launch(cases.RING_SUBSTEPS), loop.launch(cases.RING_SUBSTEPS))
    _compare(open_, cases.RING_SUBSTEPS)  # (asserts that the specialised instance is taken)
