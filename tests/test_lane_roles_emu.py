"""Fused XPBD rollout, emulated kernels: on the specialised tile of 16 an apply lane keeps the launch-invariant operands of its body in
registers (lane roles); the scenes also cover what a joint lane's record would hold.  Every case compares the
specialised launch bit for bit with the generic instance of the same tile (NT_XPBD_CFG) and with the call-by-call loop
`clear_forces; collide; step; swap`: state, body_f, per-world contact counts, and ids + the 17 record floats of every live contact.
Scenes: tests/lane_roles_cases.py; the device twin is tests/test_gpu_lane_roles.py (which adds the captured graph, and which alone
sees what contraction makes of the kernels' arithmetic)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))

import lane_roles_cases as cases  # noqa: E402
from lane_roles_cases import CFG_GENERIC, CFG_SPEC, DT, FLAT, SPEC_BIT, SPW  # noqa: E402

ITERATIONS = 2


@pytest.fixture(scope="module")
def H():
    import harness

    harness.lib()
    return harness


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


def _bits(x):
    return x.view(np.int32) if x.dtype == np.float32 else x


def _result(out, other, ct):
    n = ct.em.t.env_count
    r = {"body_q": out.body_q.copy(), "body_qd": out.body_qd.copy(), "env_count": ct.env_count.copy(),
         "body_f": np.stack([out.body_f[..., :n], other.body_f[..., :n]])}
    r.update(ct.export())
    return r


class _Sim:
    """one model's states, Contacts and Control, stepped launch after launch on path `cfg` (None: the call-by-call loop)"""

    def __init__(self, H, model, cfg, loop=False):
        self.H, self.cfg, self.loop = H, cfg, loop
        self.em = H.EmuModel(model)
        self.a, self.b, self.ct = H.EmuState(self.em), H.EmuState(self.em), H.EmuContacts(self.em)
        self.a.body_f[:], self.b.body_f[:] = 1.0, 2.0  # (the launch leaves both as clear_forces does, whatever they held)
        self.ctrl = H.EmuControl(self.em)

    def set_controls(self, f, tq, tqd):
        self.ctrl = self.H.EmuControl(self.em, joint_f=f, joint_target_q=tq, joint_target_qd=tqd)

    def set_model(self, model):  # (edited parameters: the descriptor is rebuilt from the host arrays, the state stays)
        self.em = self.H.EmuModel(model)
        for s in (self.a, self.b, self.ct):
            s.em = self.em

    def copy_state(self, other):
        self.a.body_q[:], self.a.body_qd[:] = other.a.body_q, other.a.body_qd

    def launch(self, substeps):
        H = self.H
        if self.loop:
            for _ in range(substeps):
                d = self.a.desc()
                H.check(H.lib().nt_clear_forces(C.byref(self.em.desc), C.byref(d), None), "nt_clear_forces")
                H.collide(self.em, self.a, self.ct)
                H.xpbd_step(self.em, self.a, self.b, self.ctrl, self.ct, DT, iterations=ITERATIONS)
                self.a, self.b = self.b, self.a
            for s in (self.a, self.b):
                d = s.desc()
                H.check(H.lib().nt_clear_forces(C.byref(self.em.desc), C.byref(d), None), "nt_clear_forces")
        else:
            with _cfg(self.cfg):
                out = H.xpbd_rollout(self.em, self.a, self.b, self.ctrl, self.ct, DT, substeps, iterations=ITERATIONS)
            if out is self.b:
                self.a, self.b = self.b, self.a
        return _result(self.a, self.b, self.ct)


def _assert_same(got, ref):
    assert np.isfinite(ref["body_q"]).all()
    for k in ("body_q", "body_qd", "env_count", "count", *FLAT):
        assert np.array_equal(_bits(got[k]), _bits(ref[k])), k
    assert not got["body_f"].any() and not ref["body_f"].any()


def _takes_spec(H, model, cfg):
    em = H.EmuModel(model)
    p, out = H.xpbd_params(iterations=ITERATIONS), (C.c_int32 * 5)()
    with _cfg(cfg):
        H.check(H.lib().nt_xpbd_rollout_shape(C.byref(em.desc), C.byref(p), None, out), "nt_xpbd_rollout_shape")
    return list(out)[:4] == [16, 512, 1, 1] and bool(out[4] & SPEC_BIT)


_models = {}


def _model(name):
    if name not in _models:
        _models[name] = cases.SCENES[name][0](cases.SCENES[name][1])
    return _models[name]


def _three(H, model):
    assert _takes_spec(H, model, None) and _takes_spec(H, model, CFG_SPEC) and not _takes_spec(H, model, CFG_GENERIC)
    return _Sim(H, model, None, loop=True), _Sim(H, model, CFG_GENERIC), _Sim(H, model, CFG_SPEC)


@pytest.mark.parametrize("name", sorted(cases.SCENES))
def test_specialised_rollout_equals_generic_and_loop(H, name):
    model, substeps = _model(name), cases.SCENES[name][2]
    loop, generic, spec = _three(H, model)
    ref = loop.launch(substeps)
    assert ref["env_count"][: cases.SCENES[name][1]].min() > 0  # live contacts in every world: the contact applies have records to sum
    _assert_same(generic.launch(substeps), ref)
    _assert_same(spec.launch(substeps), ref)
    _assert_same(_Sim(H, model, None).launch(substeps), ref)  # (the default dispatch)


def test_zoo_covers_every_branch_the_records_replace(H):
    import newton_amd as nt
    from newton_amd.enums import BodyFlags

    model = _model("zoo")
    t, J = model.env, nt.JointType
    types = set(int(x) for x in t.joint_type)
    assert {int(J.REVOLUTE), int(J.PRISMATIC), int(J.FIXED), int(J.BALL), int(J.D6), int(J.DISTANCE), int(J.FREE)} <= types
    assert (np.asarray(t.joint_enabled) == 0).sum() == 1 and (np.asarray(t.joint_parent) < 0).sum() >= 5  # one disabled; world parents
    assert int(t.joint_parent[0]) < 0 and int(t.joint_type[0]) == int(J.REVOLUTE)  # a SOLVED joint with a world-attached parent
    start = np.asarray(t.body_joint_start)
    assert (np.diff(start)[cases.HUB]) >= 5  # more incident joints than apply_item fetches as one batch (NT_APPLY_JOINTS = 4)
    pstart = np.asarray(t.body_pair_start)
    assert np.diff(pstart)[cases.FREE_A] >= 2  # a body with several pairs: the record's first entry, then the list
    flags, inv_mass = np.asarray(t.body_flags), np.asarray(model.body_inv_mass)[: t.nb]
    assert flags[cases.KIN] & int(BodyFlags.KINEMATIC) and not flags[cases.ZERO] & int(BodyFlags.KINEMATIC) and inv_mass[cases.ZERO] == 0
    assert cases.SCENES["zoo"][1] % 16 == 1  # a ragged tile with one valid world


@pytest.mark.parametrize("name,gap", [("chain5", 3), ("chain7", 1), ("chain8", 0)])
def test_chain_sizes_sit_below_and_on_the_lane_ranges(name, gap):
    t = _model(name).env
    for n in (t.nb, t.nj, t.ns, t.np):
        assert -(-n // SPW) * SPW - n == gap  # inert lanes between the first population and the second (A0, B0, I0, S0)


def test_two_launches_with_other_controls(H):
    """the second launch of a model runs with other joint_f / joint_target_q / joint_target_qd: nothing of the first launch's lives on"""
    model, (n, substeps) = _model("zoo"), cases.SCENES["zoo"][1:]
    sims = _three(H, model)
    first = []
    for v in (0, 1):
        f, tq, tqd = cases.controls(model, n, v)
        for s in sims:
            s.set_controls(f, tq, tqd)
        ref, generic, spec = (s.launch(substeps) for s in sims)
        _assert_same(generic, ref)
        _assert_same(spec, ref)
        first.append(ref)
    stale = _Sim(H, model, CFG_GENERIC)  # what a launch that kept the first controls would give: something else
    stale.set_controls(*cases.controls(model, n, 0))
    stale.launch(substeps)
    assert not np.array_equal(_bits(stale.launch(substeps)["body_qd"]), _bits(first[1]["body_qd"]))


def test_launches_with_one_parameter_edit_between_each(H):
    """a joint limit, then a body mass, then a shape scale change between launches (uniformly: the model keeps the specialised tile).
    After each edit a launch from the same state with the model as it was before THAT edit gives something else: each edit alone
    reaches the kernels, the body mass through the apply lanes' inverse mass"""
    import copy

    n, substeps = cases.SCENES["zoo"][1:]
    model = cases.zoo_scene(n)  # (a model of its own: edited in place)
    sims = _three(H, model)
    lagging = _Sim(H, model, CFG_GENERIC)
    ref, generic, spec = (s.launch(substeps) for s in sims)
    _assert_same(generic, ref)
    _assert_same(spec, ref)
    for which in cases.EDITS:
        lagging.set_model(copy.deepcopy(model))  # (the model without this edit, on the state the others start from)
        lagging.copy_state(sims[1])
        cases.edit_parameters(model, n, which)
        for s in sims:
            s.set_model(model)
        assert _takes_spec(H, model, None)
        ref, generic, spec = (s.launch(substeps) for s in sims)
        _assert_same(generic, ref)
        _assert_same(spec, ref)
        assert not np.array_equal(_bits(lagging.launch(substeps)["body_qd"]), _bits(ref["body_qd"])), which
