"""Specialised instance of the fused XPBD rollout (NT_SPEC) on the device: the replicated quadruped takes it;
bit for bit the generic instance of the same shape (NT_XPBD_CFG's sixth field forces either), the call-by-call loop
`clear_forces; collide; step; swap`, and its own graph replay.  40 worlds: a ragged last workgroup; 272: 17 full ones.
The emulated twin with the dispatch cases is tests/test_spec_tile_emu.py."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SPEC, GENERIC = "16,512,1,1,0,1", "16,512,1,1,0,0"
FLAT = ("shape0", "shape1", "point0", "point1", "offset0", "offset1", "normal", "margin0", "margin1")
DT, SUBSTEPS = 1e-3, 10


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


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


_scenes = {}


def _scene(n):
    """model, solver, pipeline, control and the forced-generic rollout of the scene (computed once, never modified)"""
    if n not in _scenes:
        import newton_amd as nt
        from scenes import quadruped_scene

        model = quadruped_scene(n, device="cuda:0", seed=5)
        model.joint_q.reshape(n, -1)[:, 2] -= 0.24  # feet in the ground: live contacts
        model.body_q, model.body_qd = nt.articulation.eval_fk_numpy(model, model.joint_q, model.joint_qd)
        solver, pipe, ctrl = nt.solvers.SolverXPBD(model, iterations=2), nt.CollisionPipeline(model), model.control()
        ctrl.joint_f = np.full(model.joint_dof_count, 0.3, dtype=np.float32)
        _scenes[n] = (model, solver, pipe, ctrl, _rollout(model, solver, pipe, ctrl, GENERIC))
    return _scenes[n]


def _rollout(model, solver, pipe, ctrl, cfg, substeps=SUBSTEPS):
    s0, s1, ct = model.state(), model.state(), pipe.contacts()
    with _cfg(cfg):
        out = solver.rollout(s0, s1, ctrl, ct, DT, substeps)
    assert out is (s1 if substeps % 2 else s0)
    return out, ct


def _assert_same(got, ref, min_contacts):
    (go, gct), (ro, rct) = got, ref
    assert np.isfinite(ro.body_q.cpu().numpy()).all()
    assert _same(go.body_q, ro.body_q) and _same(go.body_qd, ro.body_qd)
    n = int(rct.rigid_contact_count.cpu().numpy()[0])
    assert int(gct.rigid_contact_count.cpu().numpy()[0]) == n and n >= min_contacts
    for k in FLAT:
        assert _same(getattr(gct, "rigid_contact_" + k), getattr(rct, "rigid_contact_" + k)), k
    assert _same(gct.rigid_contact_count_per_env, rct.rigid_contact_count_per_env)


def _shape(model, solver, cfg=None):
    dm, out, p = model.device_model(), (C.c_int32 * 5)(), solver._params()
    with _cfg(cfg):
        assert dm.lib.nt_xpbd_rollout_shape(C.byref(dm.desc), C.byref(p), None, out) == 0
    return list(out)


@pytest.mark.parametrize("n", [40, 272])
def test_quadruped_takes_the_specialised_instance(n):
    model, solver = _scene(n)[:2]
    assert _shape(model, solver) == [16, 512, 1, 1, 4]
    assert _shape(model, solver, SPEC)[4] == 4 and _shape(model, solver, GENERIC)[4] == 0


@pytest.mark.parametrize("n", [40, 272])
def test_specialised_instance_is_bitwise_the_generic_one(n):
    model, solver, pipe, ctrl, generic = _scene(n)
    _assert_same(_rollout(model, solver, pipe, ctrl, SPEC), generic, min_contacts=n)
    _assert_same(_rollout(model, solver, pipe, ctrl, None), generic, min_contacts=n)  # (the default dispatch)


@pytest.mark.parametrize("n", [40, 272])
def test_specialised_rollout_equals_the_call_by_call_loop(n):
    model, solver, pipe, ctrl, _ = _scene(n)
    l0, l1, lct = model.state(), model.state(), pipe.contacts()
    for _ in range(SUBSTEPS):
        l0.clear_forces()
        pipe.collide(l0, lct)
        solver.step(l0, l1, ctrl, lct, DT)
        l0, l1 = l1, l0
    got = _rollout(model, solver, pipe, ctrl, SPEC)
    _assert_same(got, (l0, lct), min_contacts=n)
    assert not got[0].body_f.cpu().numpy().any()


def test_captured_specialised_rollout_replays_the_direct_launch():
    import torch

    import newton_amd as nt

    if getattr(torch.cuda, "_newton_emulated", False):
        pytest.skip("hipGraph capture needs the device (not emulated)")
    model, solver, pipe, ctrl, _ = _scene(40)
    with _cfg(SPEC):
        d0, d1, dct = model.state(), model.state(), pipe.contacts()
        for _ in range(2):
            assert solver.rollout(d0, d1, ctrl, dct, DT, SUBSTEPS) is d0
        g0, g1, gct = model.state(), model.state(), pipe.contacts()
        # (the direct calls above were the warm-up: the capture pass records the frame without running it)
        graph = nt.graph.capture(lambda: solver.rollout(g0, g1, ctrl, gct, DT, SUBSTEPS), warmup=0, contacts=gct)
        for _ in range(2):
            graph.launch()
        torch.cuda.synchronize()
    _assert_same((g0, gct), (d0, dct), min_contacts=40)
