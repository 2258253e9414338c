"""Fused XPBD rollout, emulated kernels: the launch equals the call-by-call loop `clear_forces; collide; step; swap` bit for bit on every
path the substep chain takes -- the pose snapshot filled by the integrate lane (specialised and generic tile of
16), the paths that keep the copy pass or take no snapshot (convex pairs, iterations=0), kinematic and zero-mass bodies (the early
returns of integrate_bodies and apply_body_deltas), the step kernel across a step boundary (W is not rebuilt by a step's last apply),
and the launch's outputs stored behind the substep loop (Contacts, per-env counts, body_f of both states).  The device twin is
tests/test_gpu_substep_chain.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))

import substep_chain_cases as cases  # noqa: E402
from substep_chain_cases import CFG_GENERIC, CFG_SPEC, DT, FLAT, SPEC_BIT  # noqa: E402


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
    """what a frame hands over: state, the nine flat Contacts fields + total count, per-env counts, body_f of both states (the
    worlds' columns: the padding of the env stride belongs to nobody)"""
    n = ct.em.t.env_count
    r = {"body_q": out.body_q.copy(), "body_qd": out.body_qd.copy(), "env_count": ct.env_count.copy(),
         "body_f": np.stack([out.body_f[..., :n], other.body_f[..., :n]])}
    r.update(ct.export())
    return r


def _setup(H, model, joint_f):
    em = H.EmuModel(model)
    ctrl = H.EmuControl(em)
    ctrl.joint_f[:] = joint_f
    return em, H.EmuState(em), H.EmuState(em), H.EmuContacts(em), ctrl


def _rollout(H, model, cfg, substeps, joint_f=0.3, **params):
    em, a, b, ct, ctrl = _setup(H, model, joint_f)
    a.body_f[:], b.body_f[:] = 1.0, 2.0  # (the launch leaves both as clear_forces does, whatever they held)
    with _cfg(cfg):
        out = H.xpbd_rollout(em, a, b, ctrl, ct, DT, substeps, **params)
    assert out is (b if substeps % 2 else a)
    return _result(out, a if out is b else b, ct)


def _loop(H, model, substeps, joint_f=0.3, **params):
    em, a, b, ct, ctrl = _setup(H, model, joint_f)
    a.body_f[:], b.body_f[:] = 1.0, 2.0
    for _ in range(substeps):
        d = a.desc()
        H.check(H.lib().nt_clear_forces(C.byref(em.desc), C.byref(d), None), "nt_clear_forces")
        H.collide(em, a, ct)
        H.xpbd_step(em, a, b, ctrl, ct, DT, **params)
        a, b = b, a
    for s in (a, b):  # (a step never writes body_f: the loop's next clear_forces does what the launch has done for both states)
        d = s.desc()
        H.check(H.lib().nt_clear_forces(C.byref(em.desc), C.byref(d), None), "nt_clear_forces")
    return _result(a, b, ct)


def _assert_same(got, ref):
    assert np.isfinite(ref["body_q"]).all()
    for k in ("body_q", "body_qd", "env_count", "count", *FLAT):
        assert np.array_equal(_bits(got[k]), _bits(ref[k])), k
    assert not got["body_f"].any() and not ref["body_f"].any()


def _shape(H, model, cfg=None, **params):
    params.setdefault("iterations", 2)
    em = H.EmuModel(model)
    p, out = H.xpbd_params(**params), (C.c_int32 * 5)()
    with _cfg(cfg):
        H.check(H.lib().nt_xpbd_rollout_shape(C.byref(em.desc), C.byref(p), None, out), "nt_xpbd_rollout_shape")
    return list(out)


@pytest.fixture(scope="module")
def quadrupeds():
    from scenes import quadruped_scene

    return cases.lowered(quadruped_scene, 40)  # two full workgroups of 16 and a ragged third


_loops = {}


def _quadruped_loop(H, quadrupeds, substeps):
    if substeps not in _loops:
        _loops[substeps] = _loop(H, quadrupeds, substeps)
    return _loops[substeps]


# (odd and even counts: both store targets; 1: the first substep is the last; 10: the headline's frame)
@pytest.mark.parametrize("substeps", [1, 2, 3, 10])
@pytest.mark.parametrize("cfg", [None, CFG_SPEC, CFG_GENERIC], ids=["default", "specialised", "generic"])
def test_lowered_quadruped_rollout_equals_the_loop(H, quadrupeds, substeps, cfg):
    ref = _quadruped_loop(H, quadrupeds, substeps)
    assert ref["env_count"][:40].min() >= 1 and ref["count"][0] >= 40  # (no pass on empty Contacts)
    assert bool(_shape(H, quadrupeds, cfg)[4] & SPEC_BIT) == (cfg != CFG_GENERIC)
    _assert_same(_rollout(H, quadrupeds, cfg, substeps), ref)


def test_kinematic_and_zero_mass_bodies(H):
    n, substeps = 24, 10
    model = cases.kinematic_scene(n)
    assert _shape(H, model) == [16, 512, 1, 1, SPEC_BIT]  # the tile of 16 with the pose snapshot, specialised instance
    ref = _loop(H, model, substeps, joint_f=0.0)
    for cfg in (None, CFG_GENERIC):
        _assert_same(_rollout(H, model, cfg, substeps, joint_f=0.0), ref)
    # the early-return paths carry live contacts at the end of the rollout, in every world
    touched = cases.bodies_in_contact(model, ref["shape0"], ref["shape1"])
    for w in range(n):
        assert {w * cases.NB_KIN + b for b in (cases.KIN, cases.RIDER, cases.FIXED, cases.TOP)} <= touched, w
    q0 = np.asarray(model.body_q, dtype=np.float32).reshape(n, cases.NB_KIN, 7)
    q1 = H.EmuModel(model).to_aos(ref["body_q"], 7, cases.NB_KIN).reshape(n, cases.NB_KIN, 7)
    assert np.array_equal(q1[:, cases.KIN], q0[:, cases.KIN])        # the kinematic platform passes through
    assert not np.array_equal(q1[:, cases.FIXED], q0[:, cases.FIXED])  # the zero-mass body drifts with its velocity


def test_convex_quadruped_rollout_equals_the_loop(H):
    """convex pairs: the pair lanes convert their records inside the pair interval -- the snapshot keeps its copy pass"""
    from scenes import quadruped_convex_scene

    model = cases.lowered(quadruped_convex_scene, 24)
    assert _shape(H, model)[4] & 1 and not _shape(H, model)[4] & SPEC_BIT
    ref = _loop(H, model, 3)
    assert ref["env_count"][:24].min() >= 1
    _assert_same(_rollout(H, model, None, 3), ref)


def test_no_iterations_rollout_equals_the_loop(H, quadrupeds):
    """iterations=0: integrate_bodies rebuilds the body origins itself and keeps its own interval"""
    ref = _loop(H, quadrupeds, 3, iterations=0)
    assert ref["env_count"][:40].min() >= 1
    for cfg in (None, CFG_GENERIC):
        _assert_same(_rollout(H, quadrupeds, cfg, 3, iterations=0), ref)


def test_two_steps_equal_a_rollout_of_two(H):
    """nt_xpbd_step against the launch across a step boundary, on the per-environment tile (one heavier link in one world)"""
    from scenes import quadruped_scene

    model = cases.one_heavier_link(quadruped_scene, 24)
    assert _shape(H, model)[3] == 0  # (no uniform-parameter tile)
    ref = _loop(H, model, 2)
    assert ref["env_count"][:24].min() >= 1
    _assert_same(_rollout(H, model, None, 2), ref)
