"""Fused XPBD rollout on the device: the specialised tile of 16 makes each contact record on the lane that solves it and its pair lanes
take the type-sorted shapes from pair_desc.  Every case compares the specialised launch bit for bit with the
generic instance of the same tile (NT_XPBD_CFG) and with the call-by-call loop `clear_forces; collide; step; swap`: state, body_f,
per-world contact counts, and ids + the 17 record floats of every live contact.  Scenes: tests/record_solve_cases.py; the emulated twin
is tests/test_record_solve_emu.py."""
import ctypes as C
import os

import numpy as np
import pytest

import record_solve_cases as cases
from record_solve_cases import CFG_GENERIC, CFG_SPEC, DT, FLAT, NSLOT, SPEC_BIT

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
    def __init__(self, model, iterations, joint_f=None):
        import newton_amd as nt

        self.model, self.solver, self.pipe = model, nt.solvers.SolverXPBD(model, iterations=iterations), nt.CollisionPipeline(model)
        self.ctrl = model.control()
        if joint_f is not None:
            self.ctrl.joint_f = np.asarray(joint_f, dtype=np.float32)

    def _fresh(self):
        s0, s1 = self.model.state(), self.model.state()
        f = np.ones((self.model.body_count, 6), dtype=np.float32)
        s0.body_f, s1.body_f = f, 2.0 * f  # (the launch leaves both as clear_forces does, whatever they held)
        return s0, s1, self.pipe.contacts()

    def rollout(self, cfg, substeps):
        s0, s1, ct = self._fresh()
        with _cfg(cfg):
            out = self.solver.rollout(s0, s1, self.ctrl, ct, DT, substeps)
        assert out is (s1 if substeps % 2 else s0)
        return out, (s0 if out is s1 else s1), ct

    def loop(self, substeps):
        s0, s1, ct = self._fresh()
        for _ in range(substeps):
            s0.clear_forces()
            self.pipe.collide(s0, ct)
            self.solver.step(s0, s1, self.ctrl, ct, DT)
            s0, s1 = s1, s0
        s0.clear_forces()
        s1.clear_forces()
        return s0, s1, ct

    def takes_spec(self, cfg):
        dm, out, p = self.model.device_model(), (C.c_int32 * 5)(), self.solver._params()
        with _cfg(cfg):
            assert dm.lib.nt_xpbd_rollout_shape(C.byref(dm.desc), C.byref(p), None, out) == 0
        return list(out)[:4] == [16, 512, 1, 1] and bool(out[4] & SPEC_BIT)


def _per_env(ct):
    return ct.rigid_contact_count_per_env.cpu().numpy()


def _assert_same(got, ref):
    (go, gother, gct), (ro, rother, rct) = got, ref
    assert np.isfinite(ro.body_q.cpu().numpy()).all()
    assert np.array_equal(_bits(go.body_q), _bits(ro.body_q)) and np.array_equal(_bits(go.body_qd), _bits(ro.body_qd))
    assert np.array_equal(_bits(gct.rigid_contact_count), _bits(rct.rigid_contact_count))
    for k in FLAT:
        assert np.array_equal(_bits(getattr(gct, "rigid_contact_" + k)), _bits(getattr(rct, "rigid_contact_" + k))), k
    assert np.array_equal(_per_env(gct), _per_env(rct))
    for s in (go, gother, ro, rother):
        assert not s.body_f.cpu().numpy().any()


_models, _sims, _loops = {}, {}, {}


def _model(name):
    if name not in _models:
        scene, n = cases.SCENES[name]
        _models[name] = scene(n, device="cuda:0")
    return _models[name]


def _sim(name, iterations):
    if (name, iterations) not in _sims:
        _sims[name, iterations] = _Sim(_model(name), iterations)
    return _sims[name, iterations]


def _reference(name, substeps, iterations):
    key = (name, substeps, iterations)
    if key not in _loops:
        _loops[key] = _sim(name, iterations).loop(substeps)  # (computed once, never modified)
    return _loops[key]


@pytest.mark.parametrize("iterations", [1, 2])
@pytest.mark.parametrize("substeps", [1, 10])
@pytest.mark.parametrize("name", sorted(cases.SCENES))
def test_specialised_rollout_equals_generic_and_loop(name, substeps, iterations):
    sim, ref = _sim(name, iterations), _reference(name, substeps, iterations)
    assert sim.takes_spec(None) and sim.takes_spec(CFG_SPEC) and not sim.takes_spec(CFG_GENERIC)
    _assert_same(sim.rollout(CFG_GENERIC, substeps), ref)
    _assert_same(sim.rollout(CFG_SPEC, substeps), ref)
    _assert_same(sim.rollout(None, substeps), ref)


@pytest.mark.parametrize("substeps", [1, 10])
def test_joint_forces_in_some_worlds_of_a_tile(substeps):
    """the joint-force lanes skip the frames of a joint whose joint_f rows are all zero: worlds with forces on every dof, with -0.0
    everywhere, with one driven joint between undriven neighbours, and with none, in one tile"""
    model, n = _model("disc_chain"), cases.SCENES["disc_chain"][1]
    if "forced" not in _sims:
        _sims["forced"] = _Sim(model, 2, cases.mixed_joint_f(model, n))
    sim = _sims["forced"]
    assert sim.takes_spec(None)
    ref = sim.loop(substeps)
    assert not np.array_equal(_bits(ref[0].body_qd), _bits(_reference("disc_chain", substeps, 2)[0].body_qd))  # (the forces act)
    _assert_same(sim.rollout(CFG_GENERIC, substeps), ref)
    _assert_same(sim.rollout(CFG_SPEC, substeps), ref)


def test_disc_chain_has_more_live_contacts_than_slot_lanes():
    n = cases.SCENES["disc_chain"][1]
    assert n == 17  # one full tile and a ragged tile with a single valid world
    for substeps in (1, 10):
        assert (_per_env(_reference("disc_chain", substeps, 2)[2])[:n] == 36).all() and 36 > NSLOT


def test_mixed_pairs_store_both_orientations():
    from newton_amd.enums import GeoType

    model = _model("mixed_pairs")
    pairs = cases.stored_pair_types(model)
    cyl, plane, sphere = int(GeoType.CYLINDER), int(GeoType.PLANE), int(GeoType.SPHERE)
    assert any(ta == cyl and tb == plane for ta, tb, _, _ in pairs)  # stored against the type order: exchanged
    assert any(ta == plane and tb == cyl for ta, tb, _, _ in pairs)  # stored in type order
    assert any(ta == sphere and tb == sphere and ba >= 0 and bb >= 0 for ta, tb, ba, bb in pairs)  # no static side
    ct = _reference("mixed_pairs", 10, 2)[2]
    s0, s1 = ct.rigid_contact_shape0.cpu().numpy(), ct.rigid_contact_shape1.cpu().numpy()
    body, live = np.asarray(model.shape_body), s0 >= 0
    assert ((body[s0[live]] >= 0) & (body[s1[live]] >= 0)).any()  # the dynamic-dynamic pair is live
    assert _per_env(ct)[:16].min() >= 12


def test_dropped_worlds_gain_contacts_inside_the_launch():
    from newton_amd.enums import BodyFlags

    first, last = _per_env(_reference("dropped", 1, 2)[2])[:16], _per_env(_reference("dropped", 10, 2)[2])[:16]
    assert (first == 0).any() and (first >= 3).any()  # worlds without a live contact beside worlds with several, in one tile
    assert (last > first).any()                         # contacts that appear in the middle of the launch
    assert (np.asarray(_model("dropped").env.body_flags) & int(BodyFlags.KINEMATIC) != 0).sum() == 1  # one kinematic body per world
