"""Fused XPBD rollout, emulated kernels: on the specialised tile of 16 a joint lane keeps the launch-invariant operands of its joint in
registers (lane roles, nt_ctx.hpp: JointRole).  Every case compares the specialised launch bit for bit with the
generic instance of the same tile (NT_XPBD_CFG) and with the call-by-call loop `clear_forces; collide; step; swap`: state, body_f,
per-world contact counts, and ids + the 17 record floats of every live contact.  No tolerance anywhere.
Scenes: tests/lane_roles_cases.py and tests/joint_roles_cases.py; the device twin is tests/test_gpu_joint_roles.py, which adds the
captured graph and which alone sees what contraction makes of the kernels' arithmetic."""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))

import joint_roles_cases as cases  # noqa: E402
from joint_roles_cases import CFG_GENERIC, CFG_SPEC, DT, FLAT, SPEC_BIT, SPW  # noqa: E402


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


class _Sim:
    """one model's states, Contacts and Control, stepped launch after launch on path `cfg` (loop: the call-by-call loop, which can
    report the per-joint corrections of its last step)"""

    def __init__(self, H, model, cfg, loop=False, iterations=2):
        self.H, self.cfg, self.loop, self.iterations = H, cfg, loop, iterations
        self.em = H.EmuModel(model)
        self.a, self.b, self.ct = H.EmuState(self.em, parent_f=loop), H.EmuState(self.em, parent_f=loop), H.EmuContacts(self.em)
        self.a.body_f[:], self.b.body_f[:] = 1.0, 2.0  # (the launch leaves both as clear_forces does, whatever they held)
        self.ctrl = H.EmuControl(self.em)
        self.joint_impulse = None

    def set_controls(self, f, tq, tqd):
        self.ctrl = self.H.EmuControl(self.em, joint_f=f, joint_target_q=tq, joint_target_qd=tqd)

    def set_model(self, model):  # (edited parameters: the descriptor is rebuilt from the host arrays, the state stays)
        self.em = self.H.EmuModel(model)
        for s in (self.a, self.b, self.ct):
            s.em = self.em

    def copy_state(self, other):
        self.a.body_q[:], self.a.body_qd[:] = other.a.body_q, other.a.body_qd

    def launch(self, substeps):
        H, L, t = self.H, self.H.L, self.em.t
        if self.loop:
            ji = np.zeros((6, max(t.nj, 1), t.env_stride), np.float32)
            ci = np.zeros((6, max(t.np * t.cpp, 1), t.env_stride), np.float32)
            rep = L.nt_xpbd_report(ci.ctypes.data, ji.ctypes.data)
            seen = np.zeros_like(ji)  # (each step starts its accumulator anew: the largest magnitude over the launch's steps)
            for _ in range(substeps):
                d = self.a.desc()
                H.check(H.lib().nt_clear_forces(C.byref(self.em.desc), C.byref(d), None), "nt_clear_forces")
                H.collide(self.em, self.a, self.ct)
                H.xpbd_step(self.em, self.a, self.b, self.ctrl, self.ct, DT, report=rep, iterations=self.iterations)
                self.a, self.b = self.b, self.a
                seen = np.maximum(seen, np.abs(ji))
            for s in (self.a, self.b):
                d = s.desc()
                H.check(H.lib().nt_clear_forces(C.byref(self.em.desc), C.byref(d), None), "nt_clear_forces")
            self.joint_impulse = seen[:, : t.nj, : t.env_count].transpose(2, 0, 1).copy()
        else:
            with _cfg(self.cfg):
                out = H.xpbd_rollout(self.em, self.a, self.b, self.ctrl, self.ct, DT, substeps, iterations=self.iterations)
            if out is self.b:
                self.a, self.b = self.b, self.a
        n = t.env_count
        r = {"body_q": self.a.body_q.copy(), "body_qd": self.a.body_qd.copy(), "env_count": self.ct.env_count.copy(),
             "body_f": np.stack([self.a.body_f[..., :n], self.b.body_f[..., :n]])}
        r.update(self.ct.export())
        return r


def _assert_same(got, ref):
    assert np.isfinite(ref["body_q"]).all()
    for k in ("body_q", "body_qd", "env_count", "count", *FLAT):
        assert np.array_equal(_bits(got[k]), _bits(ref[k])), k
    assert not got["body_f"].any() and not ref["body_f"].any()


def _shape(H, model, cfg, iterations=2):
    em = H.EmuModel(model)
    p, out = H.xpbd_params(iterations=iterations), (C.c_int32 * 5)()
    with _cfg(cfg):
        H.check(H.lib().nt_xpbd_rollout_shape(C.byref(em.desc), C.byref(p), None, out), "nt_xpbd_rollout_shape")
    return list(out)


def _takes_spec(H, model, cfg, iterations=2):
    out = _shape(H, model, cfg, iterations)
    return out[:4] == [16, 512, 1, 1] and bool(out[4] & SPEC_BIT)


_models = {}


def _model(name):
    if name not in _models:
        _models[name] = cases.SCENES[name][0](cases.SCENES[name][1])
    return _models[name]


def _three(H, model, iterations=2):
    """(loop, generic, specialised) -- and the specialised instance is really the one the last of them runs"""
    assert _takes_spec(H, model, None, iterations) and _takes_spec(H, model, CFG_SPEC, iterations)
    assert not _takes_spec(H, model, CFG_GENERIC, iterations)
    return (_Sim(H, model, None, loop=True, iterations=iterations), _Sim(H, model, CFG_GENERIC, iterations=iterations),
            _Sim(H, model, CFG_SPEC, iterations=iterations))


def _compare(H, model, substeps, iterations=2):
    loop, generic, spec = _three(H, model, iterations)
    ref = loop.launch(substeps)
    cases.assert_every_live_type_corrects(model.env, loop.joint_impulse)  # (the joint lanes had something to do, in every type)
    _assert_same(generic.launch(substeps), ref)
    _assert_same(spec.launch(substeps), ref)
    _assert_same(_Sim(H, model, None, iterations=iterations).launch(substeps), ref)  # (the default dispatch)
    return ref


@pytest.mark.parametrize("name", sorted(cases.SCENES))
def test_specialised_rollout_equals_generic_and_loop(H, name):
    _compare(H, _model(name), cases.SCENES[name][2])


@pytest.mark.parametrize("iterations", [1, 2, 3])
def test_chain_of_five_at_one_two_and_three_iterations(H, iterations):
    """(the drift of the first joint role showed on this chain after two substeps)"""
    _compare(H, _model("chain5"), cases.SCENES["chain5"][2], iterations)


def test_zoo_holds_what_a_joint_record_holds():
    import newton_amd as nt

    t, J = _model("zoo").env, nt.JointType
    types = set(int(x) for x in t.joint_type)
    assert {int(J.REVOLUTE), int(J.PRISMATIC), int(J.FIXED), int(J.BALL), int(J.D6), int(J.DISTANCE), int(J.FREE)} <= types
    assert (np.asarray(t.joint_enabled) == 0).sum() == 1
    assert int(t.joint_parent[0]) < 0 and int(t.joint_type[0]) == int(J.REVOLUTE)  # a SOLVED joint with a world-attached parent
    assert np.diff(np.asarray(t.body_joint_start))[cases.base.HUB] == 6  # the hub
    assert np.asarray(_model("zoo").body_inv_mass)[cases.base.ZERO] == 0  # (its free joint is never solved and still is a record)
    assert int(t.joint_type[cases.ZOO_PRISMATIC_JOINT]) == int(J.PRISMATIC) and int(t.joint_enabled[cases.ZOO_PRISMATIC_JOINT])
    # the angular joint lanes start at A0 = nj rounded up to a wave of slots: three below, one below and on the boundary
    for name, gap in (("chain5", 3), ("chain7", 1), ("chain8", 0)):
        nj = _model(name).env.nj
        assert -(-nj // SPW) * SPW - nj == gap


def test_two_launches_with_other_targets(H):
    """the second launch of a model runs with other joint_f / joint_target_q / joint_target_qd: nothing of the first launch's lives on"""
    model, (n, substeps) = _model("zoo"), cases.SCENES["zoo"][1:]
    sims = _three(H, model)
    second = None
    for v in (0, 1):
        f, tq, tqd = cases.base.controls(model, n, v)
        for s in sims:
            s.set_controls(f, tq, tqd)
        ref, generic, spec = (s.launch(substeps) for s in sims)
        _assert_same(generic, ref)
        _assert_same(spec, ref)
        second = ref
    stale = _Sim(H, model, CFG_GENERIC)  # what a launch that kept the first controls would give: something else
    stale.set_controls(*cases.base.controls(model, n, 0))
    stale.launch(substeps)
    assert not np.array_equal(_bits(stale.launch(substeps)["body_qd"]), _bits(second["body_qd"]))


def test_a_joint_edit_between_launches_equals_a_fresh_model_with_that_edit(H):
    """The prismatic joint disabled, then enabled again, then a joint limit moved, a launch after each.  Each launch equals, bit for
    bit, the launch of a model built anew and given the same edits, started from the same state: the record is refilled per launch.
    And each edit alone reaches the kernels: the model without it gives something else."""
    n, substeps = cases.SCENES["zoo"][1:]
    model = cases.base.zoo_scene(n)  # (a model of its own: edited in place)
    sims = _three(H, model)
    ref, generic, spec = (s.launch(substeps) for s in sims)
    _assert_same(generic, ref)
    _assert_same(spec, ref)
    for k, which in enumerate(cases.JOINT_EDITS):
        lagging = _Sim(H, copy.deepcopy(model), CFG_GENERIC)  # (the model without this edit, on the state the others start from)
        lagging.copy_state(sims[1])
        cases.edit_joint(model, n, which)
        fresh_model = cases.base.zoo_scene(n)
        for w in cases.JOINT_EDITS[: k + 1]:
            cases.edit_joint(fresh_model, n, w)
        fresh = _Sim(H, fresh_model, CFG_GENERIC)
        fresh.copy_state(sims[1])
        for s in sims:
            s.set_model(model)
        assert _takes_spec(H, model, None)
        assert int(model.env.joint_enabled[cases.ZOO_PRISMATIC_JOINT]) == (0 if which == "disable_prismatic" else 1)
        ref, generic, spec = (s.launch(substeps) for s in sims)
        _assert_same(generic, ref)
        _assert_same(spec, ref)
        _assert_same(spec, fresh.launch(substeps))
        assert not np.array_equal(_bits(lagging.launch(substeps)["body_qd"]), _bits(ref["body_qd"])), which


def test_seventeen_joints_take_the_generic_instance_and_sixteen_the_specialised(H):
    """xpbd_spec_tile_fits: wave_up(nj) + nj <= nslot, so that a joint lane makes one trip and its record is its joint's.  16 joints fill
    the 32 slots; a loop-closing 17th (nb stays 16: every other fact holds) keeps the generic instance, and asking for the specialised
    one is refused."""
    closed, open_ = cases.ring_scene(cases.RING_WORLDS, closed=True), cases.ring_scene(cases.RING_WORLDS, closed=False)
    assert (closed.env.nj, closed.env.nb, open_.env.nj) == (17, 16, 16)
    shape = _shape(H, closed, None)
    assert shape[:4] == [16, 512, 1, 1] and not shape[4] & SPEC_BIT
    with pytest.raises(Exception):
        _Sim(H, closed, CFG_SPEC).launch(cases.RING_SUBSTEPS)
    loop, rollout = _Sim(H, closed, None, loop=True), _Sim(H, closed, None)
    ref = loop.launch(cases.RING_SUBSTEPS)
    cases.assert_every_live_type_corrects(closed.env, loop.joint_impulse)  # (the closing joint pulls)
    _assert_same(rollout.launch(cases.RING_SUBSTEPS), ref)
    _compare(H, open_, cases.RING_SUBSTEPS)  # (asserts that the specialised instance is taken)
