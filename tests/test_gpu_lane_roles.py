"""Fused XPBD rollout on the device: on the specialised tile of 16 an apply lane keeps the launch-invariant operands of its body in
registers (lane roles); the scenes also cover what a joint lane's record would hold.  Every case compares the
specialised launch bit for bit with the generic instance of the same tile (NT_XPBD_CFG) and with the call-by-call loop
`clear_forces; collide; step; swap`: state, body_f, per-world contact counts, and ids + the 17 record floats of every live contact.
Scenes: tests/lane_roles_cases.py; the emulated twin is tests/test_lane_roles_emu.py."""
import ctypes as C
import os

import numpy as np
import pytest

import lane_roles_cases as cases
from lane_roles_cases import CFG_GENERIC, CFG_SPEC, DT, FLAT, SPEC_BIT

pytestmark = pytest.mark.gpu

ITERATIONS = 2


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

    def __init__(self, model, cfg, loop=False):
        import newton_amd as nt

        self.model, self.cfg, self.loop = model, cfg, loop
        self.solver, self.pipe = nt.solvers.SolverXPBD(model, iterations=ITERATIONS), nt.CollisionPipeline(model)
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

    def takes_spec(self, cfg):
        dm, out, p = self.model.device_model(), (C.c_int32 * 5)(), self.solver._params()
        with _cfg(cfg):
            assert dm.lib.nt_xpbd_rollout_shape(C.byref(dm.desc), C.byref(p), None, out) == 0
        return list(out)[:4] == [16, 512, 1, 1] and bool(out[4] & SPEC_BIT)


def _assert_same(got, ref):
    assert np.isfinite(ref["body_q"].view(np.float32)).all()
    for k in ("body_q", "body_qd", "env_count", "count", *FLAT):
        assert np.array_equal(got[k], ref[k]), k
    assert not got["body_f"].any() and not ref["body_f"].any()


_models = {}


def _model(name):
    if name not in _models:
        _models[name] = cases.SCENES[name][0](cases.SCENES[name][1], device="cuda:0")
    return _models[name]


def _three(model):
    sims = _Sim(model, None, loop=True), _Sim(model, CFG_GENERIC), _Sim(model, CFG_SPEC)
    assert sims[2].takes_spec(None) and sims[2].takes_spec(CFG_SPEC) and not sims[2].takes_spec(CFG_GENERIC)
    return sims


@pytest.mark.parametrize("name", sorted(cases.SCENES))
def test_specialised_rollout_equals_generic_and_loop(name):
    model, substeps = _model(name), cases.SCENES[name][2]
    loop, generic, spec = _three(model)
    ref = loop.launch(substeps)
    assert ref["env_count"][: cases.SCENES[name][1]].min() > 0  # live contacts in every world: the contact applies have records to sum
    _assert_same(generic.launch(substeps), ref)
    _assert_same(spec.launch(substeps), ref)
    _assert_same(_Sim(model, None).launch(substeps), ref)  # (the default dispatch)


def test_two_launches_with_other_controls():
    """the second launch of a model runs with other joint_f / joint_target_q / joint_target_qd: nothing of the first launch's lives on"""
    model, (n, substeps) = _model("zoo"), cases.SCENES["zoo"][1:]
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


def _notify(sim):
    import newton_amd as nt

    F = nt.ModelFlags
    sim.solver.notify_model_changed(F.JOINT_DOF_PROPERTIES | F.BODY_INERTIAL_PROPERTIES | F.SHAPE_PROPERTIES)


def test_launches_with_one_parameter_edit_between_each():
    """a joint limit, then a body mass, then a shape scale change between launches (uniformly: the model keeps the specialised tile);
    notify_model_changed refreshes the device tables.  After each edit a launch from the same state with a model that lacks THAT edit
    gives something else: each edit alone reaches the device, the body mass through the apply lanes' inverse mass"""
    n, substeps = cases.SCENES["zoo"][1:]
    model, lag_model = cases.zoo_scene(n, device="cuda:0"), cases.zoo_scene(n, device="cuda:0")  # (models of their own: edited in place)
    sims, lagging = _three(model), _Sim(lag_model, CFG_GENERIC)
    ref, generic, spec = (s.launch(substeps) for s in sims)
    _assert_same(generic, ref)
    _assert_same(spec, ref)
    for k, which in enumerate(cases.EDITS):
        if k:  # (the lagging model follows one edit behind)
            cases.edit_parameters(lag_model, n, cases.EDITS[k - 1])
            _notify(lagging)
        lagging.s0.assign(sims[1].s0)
        cases.edit_parameters(model, n, which)
        _notify(sims[0])
        assert sims[2].takes_spec(None)
        ref, generic, spec = (s.launch(substeps) for s in sims)
        _assert_same(generic, ref)
        _assert_same(spec, ref)
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
        s.set_controls(*cases.controls(model, n, 0))

    def frame():  # s0 -> s1, then s1 back into s0: the captured buffers are the same in every replay
        spec.solver.rollout(spec.s0, spec.s1, spec.ctrl, spec.ct, DT, substeps)
        spec.s0.assign(spec.s1)

    with _cfg(CFG_SPEC):
        g = nt.graph.capture(frame, warmup=0, contacts=spec.ct)  # (the capture launches nothing: the replays do)
        for v in (0, 1):
            for s in (generic, spec):
                s.set_controls(*cases.controls(model, n, v))
            g.launch()
            torch.cuda.synchronize()
            ref, got = generic.launch(substeps), spec.snapshot()
            for k in ("body_q", "body_qd", "env_count", "count", *FLAT):
                assert np.array_equal(got[k], ref[k]), (v, k)
