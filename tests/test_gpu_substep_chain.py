"""Fused XPBD rollout on the device: the launch equals the call-by-call loop `clear_forces; collide; step; swap` bit for bit on every
path the substep chain takes -- the pose snapshot filled by the integrate lane (specialised and generic tile of
16), the paths that keep the copy pass or take no snapshot (convex pairs, iterations=0), kinematic and zero-mass bodies, the step
kernel across a step boundary, and the launch's outputs stored behind the substep loop (Contacts, per-env counts, body_f of both
states).  The emulated twin is tests/test_substep_chain_emu.py."""
import ctypes as C
import os

import numpy as np
import pytest

import substep_chain_cases as cases
from substep_chain_cases import CFG_GENERIC, CFG_SPEC, DT, FLAT, SPEC_BIT

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
    def __init__(self, model, joint_f=0.3, **solver_kw):
        import newton_amd as nt

        solver_kw.setdefault("iterations", 2)
        self.model, self.solver, self.pipe = model, nt.solvers.SolverXPBD(model, **solver_kw), nt.CollisionPipeline(model)
        self.ctrl = model.control()
        self.ctrl.joint_f = np.full(model.joint_dof_count, joint_f, dtype=np.float32)

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
        s0.clear_forces()  # (a step never writes body_f: the loop's next clear_forces does what the launch has done for both states)
        s1.clear_forces()
        return s0, s1, ct

    def shape(self, cfg=None):
        dm, out, p = self.model.device_model(), (C.c_int32 * 5)(), self.solver._params()
        with _cfg(cfg):
            assert dm.lib.nt_xpbd_rollout_shape(C.byref(dm.desc), C.byref(p), None, out) == 0
        return list(out)


def _count(ct):
    return int(ct.rigid_contact_count.cpu().numpy()[0])


def _assert_same(got, ref, min_contacts):
    (go, gother, gct), (ro, rother, rct) = got, ref
    assert np.isfinite(ro.body_q.cpu().numpy()).all()
    assert np.array_equal(_bits(go.body_q), _bits(ro.body_q)) and np.array_equal(_bits(go.body_qd), _bits(ro.body_qd))
    assert _count(gct) == _count(rct) and _count(rct) >= min_contacts  # (no pass on empty Contacts)
    for k in FLAT:
        assert np.array_equal(_bits(getattr(gct, "rigid_contact_" + k)), _bits(getattr(rct, "rigid_contact_" + k))), k
    assert np.array_equal(_bits(gct.rigid_contact_count_per_env), _bits(rct.rigid_contact_count_per_env))
    for s in (go, gother, ro, rother):
        assert not s.body_f.cpu().numpy().any()


_cache = {}


def _quadrupeds():
    if "sim" not in _cache:
        from scenes import quadruped_scene

        _cache["sim"] = _Sim(cases.lowered(quadruped_scene, 40, device="cuda:0"))  # two full workgroups of 16 and a ragged third
    return _cache["sim"]


def _quadruped_loop(substeps):
    if substeps not in _cache:
        _cache[substeps] = _quadrupeds().loop(substeps)  # (computed once, never modified)
    return _cache[substeps]


# (odd and even counts: both store targets; 1: the first substep is the last; 10: the headline's frame)
@pytest.mark.parametrize("substeps", [1, 2, 3, 10])
@pytest.mark.parametrize("cfg", [None, CFG_SPEC, CFG_GENERIC], ids=["default", "specialised", "generic"])
def test_lowered_quadruped_rollout_equals_the_loop(substeps, cfg):
    sim, ref = _quadrupeds(), _quadruped_loop(substeps)
    assert int(ref[2].rigid_contact_count_per_env.cpu().numpy()[:40].min()) >= 1
    assert bool(sim.shape(cfg)[4] & SPEC_BIT) == (cfg != CFG_GENERIC)
    _assert_same(sim.rollout(cfg, substeps), ref, min_contacts=40)


def test_kinematic_and_zero_mass_bodies():
    n, substeps = 24, 10
    model = cases.kinematic_scene(n, device="cuda:0")
    sim = _Sim(model, joint_f=0.0)
    assert sim.shape() == [16, 512, 1, 1, SPEC_BIT]  # the tile of 16 with the pose snapshot, specialised instance
    ref = sim.loop(substeps)
    for cfg in (None, CFG_GENERIC):
        _assert_same(sim.rollout(cfg, substeps), ref, min_contacts=2 * n)
    # the early-return paths carry live contacts at the end of the rollout, in every world
    ct = ref[2]
    touched = cases.bodies_in_contact(model, ct.rigid_contact_shape0.cpu().numpy(), ct.rigid_contact_shape1.cpu().numpy())
    for w in range(n):
        assert {w * cases.NB_KIN + b for b in (cases.KIN, cases.RIDER, cases.FIXED, cases.TOP)} <= touched, w
    q0 = np.asarray(model.body_q, dtype=np.float32).reshape(n, cases.NB_KIN, 7)
    q1 = ref[0].body_q.cpu().numpy().reshape(n, cases.NB_KIN, 7)
    assert np.array_equal(q1[:, cases.KIN], q0[:, cases.KIN])        # the kinematic platform passes through
    assert not np.array_equal(q1[:, cases.FIXED], q0[:, cases.FIXED])  # the zero-mass body drifts with its velocity


def test_convex_quadruped_rollout_equals_the_loop():
    """convex pairs: the pair lanes convert their records inside the pair interval -- the snapshot keeps its copy pass"""
    from scenes import quadruped_convex_scene

    sim = _Sim(cases.lowered(quadruped_convex_scene, 24, device="cuda:0"))
    assert sim.shape()[4] & 1 and not sim.shape()[4] & SPEC_BIT
    _assert_same(sim.rollout(None, 3), sim.loop(3), min_contacts=24)


def test_no_iterations_rollout_equals_the_loop():
    """iterations=0: integrate_bodies rebuilds the body origins itself and keeps its own interval"""
    sim = _Sim(_quadrupeds().model, iterations=0)
    ref = sim.loop(3)
    for cfg in (None, CFG_GENERIC):
        _assert_same(sim.rollout(cfg, 3), ref, min_contacts=40)


def test_two_steps_equal_a_rollout_of_two():
    """nt_xpbd_step against the launch across a step boundary, on the per-environment tile (one heavier link in one world)"""
    from scenes import quadruped_scene

    sim = _Sim(cases.one_heavier_link(quadruped_scene, 24, device="cuda:0"))
    assert sim.shape()[3] == 0  # (no uniform-parameter tile)
    _assert_same(sim.rollout(None, 2), sim.loop(2), min_contacts=24)
