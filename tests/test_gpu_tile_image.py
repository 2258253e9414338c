"""The tile image (nt_model.tile_image_words, found at nt_model.body_flags) on the device (the block-shared region of the kernels' LDS tile as one host-packed image, DESIGN.md section
3.1): the fused XPBD rollout with the image against the same launch under NT_TILE_IMAGE=0 (table-by-table staging), against the
call-by-call loop and through one captured graph, bit for bit; and Model.notify_model_changed, which rewrites the image in place,
against a rebuilt model.  The CPU twin with the word-for-word checks of the image is tests/test_tile_image_emu.py."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SUBSTEPS, DT = 10, 1e-3


@contextmanager
def _image(on):
    """NT_TILE_IMAGE is read by the launch code at every launch"""
    old = os.environ.get("NT_TILE_IMAGE")
    try:
        if on:
            os.environ.pop("NT_TILE_IMAGE", None)
        else:
            os.environ["NT_TILE_IMAGE"] = "0"
        yield
    finally:
        if old is None:
            os.environ.pop("NT_TILE_IMAGE", None)
        else:
            os.environ["NT_TILE_IMAGE"] = old


def _quadrupeds(n, mass_factor=None):
    import newton_amd as nt
    from scenes import quadruped_scene

    model = quadruped_scene(n, seed=5, device="cuda:0")
    model.joint_q.reshape(n, -1)[:, 2] -= 0.24  # feet in the ground: live contacts
    model.body_q, model.body_qd = nt.articulation.eval_fk_numpy(model, model.joint_q, model.joint_qd)
    if mass_factor is not None:
        _scale_mass(model, mass_factor)
    return model


def _scale_mass(model, factor):
    """every link of every world `factor` times heavier: mass, inertia and their inverses"""
    for k, f in (("body_mass", factor), ("body_inertia", factor), ("body_inv_mass", 1.0 / factor), ("body_inv_inertia", 1.0 / factor)):
        setattr(model, k, (np.array(getattr(model, k), copy=True) * np.float32(f)).astype(np.float32))


def _setup(model):
    import newton_amd as nt

    pipe = nt.CollisionPipeline(model)
    solver = nt.solvers.SolverXPBD(model, iterations=2)
    ctrl = model.control()
    ctrl.joint_f = np.full(model.joint_dof_count, 0.3, dtype=np.float32)
    return pipe, solver, ctrl


def _result(state, contacts):
    import torch

    torch.cuda.synchronize()
    n = int(contacts.rigid_contact_count.cpu().numpy()[0])
    return (state.body_q.cpu().numpy().copy(), state.body_qd.cpu().numpy().copy(), n,
            contacts.rigid_contact_shape0.cpu().numpy()[:n].copy(), contacts.rigid_contact_point0.cpu().numpy()[:n].copy(),
            contacts.rigid_contact_normal.cpu().numpy()[:n].copy())


def _same(a, b):
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x, y.view(np.int32) if y.dtype == np.float32 else y)
        else:
            assert x == y


def _rollout(model, pipe, solver, ctrl, image=True):
    s0, s1, contacts = model.state(), model.state(), pipe.contacts()
    with _image(image):
        out = solver.rollout(s0, s1, ctrl, contacts, DT, SUBSTEPS)
    return _result(out, contacts)


@pytest.mark.parametrize("n", [40, 272])  # three workgroups of 16 with a ragged last one; 17 workgroups
def test_rollout_with_image_is_bitwise_staged_loop_and_graph(n):
    import torch

    import newton_amd as nt

    model = _quadrupeds(n)
    dm = model.device_model()
    assert dm.desc.tile_image_words > 0 and dm.desc.body_flags % 16 == 0 and dm.desc.params_uniform == 1
    pipe, solver, ctrl = _setup(model)
    got = _rollout(model, pipe, solver, ctrl, image=True)
    assert np.isfinite(got[0]).all() and np.abs(got[1]).max() > 0.0 and got[2] >= n  # moving, every robot in contact
    # 1. the table-by-table staging of the same library
    _same(got, _rollout(model, pipe, solver, ctrl, image=False))
    # 2. the call-by-call loop (collide and step stage the same image, each launch)
    s0, s1, contacts = model.state(), model.state(), pipe.contacts()
    for _ in range(SUBSTEPS):
        s0.clear_forces()
        pipe.collide(s0, contacts)
        solver.step(s0, s1, ctrl, contacts, DT)
        s0, s1 = s1, s0
    _same(got, _result(s0, contacts))
    # 3. one replay of the captured launch
    if not getattr(torch.cuda, "_newton_emulated", False):  # (hipGraph capture needs the device)
        st, contacts = [model.state(), model.state()], pipe.contacts()
        g = nt.graph.capture(lambda: solver.rollout(st[0], st[1], ctrl, contacts, DT, SUBSTEPS), warmup=0)
        g.launch()
        _same(got, _result(st[0], contacts))


def test_notify_model_changed_rewrites_the_image():
    import newton_amd as nt

    n = 40
    model = _quadrupeds(n)
    pipe, solver, ctrl = _setup(model)
    before = _rollout(model, pipe, solver, ctrl)
    _scale_mass(model, 2.0)
    solver.notify_model_changed(nt.ModelFlags.BODY_INERTIAL_PROPERTIES)
    assert model.device_model().desc.params_uniform == 1 and model.device_model().desc.tile_image_words > 0
    edited = _rollout(model, pipe, solver, ctrl)
    _same(edited, _rollout(model, pipe, solver, ctrl, image=False))  # image and tables were refreshed together
    rebuilt_model = _quadrupeds(n, mass_factor=2.0)
    rebuilt = _rollout(rebuilt_model, *_setup(rebuilt_model))
    _same(edited, rebuilt)
    assert not np.array_equal(edited[1], before[1])  # the edit reached the kernels
