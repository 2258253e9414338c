"""Specialised instance of the fused XPBD rollout (NT_SPEC): the uniform-parameter tile of 16 with the facts the
launch code verified (nt_kernels.hip: xpbd_spec_tile_fits) compiled in as constants.  Emulated kernels: bitwise against the generic
instance of the same shape, plus the dispatch -- the quadruped takes the instance, every model or option that breaks one of the facts
keeps the generic one.  NT_XPBD_CFG's sixth field is the handle: 0 forces the generic instance, 1 asks for the specialised one.  The
GPU twin is tests/test_gpu_spec_tile.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))

SPEC, GENERIC = "16,512,1,1,0,1", "16,512,1,1,0,0"
SPEC_BIT = 4  # nt_xpbd_rollout_shape: out[4]


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


def _rollout(H, model, cfg, substeps=6, **params):
    params.setdefault("iterations", 2)
    em = H.EmuModel(model)
    a, b, ct, ctrl = H.EmuState(em), H.EmuState(em), H.EmuContacts(em), H.EmuControl(em)
    ctrl.joint_f[:] = 0.3
    with _cfg(cfg):
        H.xpbd_rollout(em, a, b, ctrl, ct, 1e-3, substeps, **params)
    out = a if substeps % 2 == 0 else b
    return {"body_q": out.body_q.copy(), "body_qd": out.body_qd.copy(), "shape0": ct.shape0.copy(), "shape1": ct.shape1.copy(),
            "env_count": ct.env_count.copy(), "data": ct.data.copy()}


def _shape(H, model, cfg=None, **params):
    params.setdefault("iterations", 2)
    em = H.EmuModel(model)
    p, out = H.xpbd_params(**params), (C.c_int32 * 5)()
    with _cfg(cfg):
        H.check(H.lib().nt_xpbd_rollout_shape(C.byref(em.desc), C.byref(p), None, out), "nt_xpbd_rollout_shape")
    return list(out)


def _bits(x):
    return x.view(np.int32) if x.dtype == np.float32 else x


def _assert_same(r0, r1):
    for k in ("body_q", "body_qd", "shape0", "shape1", "env_count"):
        assert np.array_equal(_bits(r0[k]), _bits(r1[k])), k
    # records of the live slots (a dead slot keeps what an earlier launch left there: these tiles write the last substep's only)
    live = np.broadcast_to((r0["shape0"] >= 0)[None, ...], r0["data"].shape)
    assert np.array_equal(_bits(r0["data"])[live], _bits(r1["data"])[live])


def _lowered_quadrupeds(n=40, scene=None, drop=0.24):
    from scenes import quadruped_scene

    import newton_amd as nt

    model = (scene or quadruped_scene)(n, seed=5)  # 40 worlds: ragged last workgroup; seed: per-world STATE jitter, same parameters
    model.joint_q.reshape(n, -1)[:, 2] -= drop  # feet in the ground: live contacts
    model.body_q, model.body_qd = nt.articulation.eval_fk_numpy(model, model.joint_q, model.joint_qd)
    return model


@pytest.fixture(scope="module")
def quadrupeds():
    return _lowered_quadrupeds()


@pytest.mark.parametrize("substeps", [6, 5])  # (5: the odd output state, and another last substep for the Contacts export)
def test_specialised_instance_is_bitwise_the_generic_one(H, quadrupeds, substeps):
    r0 = _rollout(H, quadrupeds, GENERIC, substeps)
    r1 = _rollout(H, quadrupeds, SPEC, substeps)
    _assert_same(r0, r1)
    assert r0["env_count"][:40].min() > 0 and (r0["shape0"] >= 0).any() and np.abs(r0["body_qd"]).max() > 0.0


def test_replicated_quadruped_takes_the_specialised_instance(H, quadrupeds):
    assert _shape(H, quadrupeds)[:4] == [16, 512, 1, 1]
    assert _shape(H, quadrupeds)[4] & SPEC_BIT
    assert _shape(H, quadrupeds, SPEC)[4] & SPEC_BIT
    assert not _shape(H, quadrupeds, GENERIC)[4] & SPEC_BIT
    assert not _shape(H, quadrupeds, "32,512,1,1")[4] & SPEC_BIT  # (the other tiles have no such instance)
    _assert_same(_rollout(H, quadrupeds, None), _rollout(H, quadrupeds, GENERIC))


def _one_heavier_link():
    model = _lowered_quadrupeds()
    model.body_mass = np.array(model.body_mass, copy=True)
    model.body_mass[13 * 3 + 2] *= 1.25  # one link of world 3
    model.body_inv_mass = np.where(model.body_mass > 0, 1.0 / np.maximum(model.body_mass, 1e-30), 0.0).astype(np.float32)
    return model


def _jointless():
    """Analytic pairs, uniform parameters, no joint at all: spheres as free links on the ground."""
    import newton_amd as nt

    env = nt.ModelBuilder()
    for k in range(3):
        b = env.add_link(xform=[0.4 * k, 0.0, 0.095 + 0.01 * k, 0.0, 0.0, 0.0, 1.0])
        env.add_shape_sphere(b, radius=0.1)
    scene = nt.ModelBuilder()
    scene.replicate(env, 40)
    scene.add_ground_plane()
    return scene.finalize()


def _convex():
    from scenes import quadruped_convex_scene

    return _lowered_quadrupeds(scene=quadruped_convex_scene)


# each line breaks ONE fact of xpbd_spec_tile_fits: (model, solver options, an override the model can take with the generic instance
# forced, does the uniform tile of 16 itself still fit the model and options)
BREAKERS = {
    "restitution": (_lowered_quadrupeds, {"enable_restitution": True}, "8,256,2,0,0,0", False),
    "velocity_from_position_delta": (_lowered_quadrupeds, {"compute_body_velocity_from_position_delta": True}, "8,256,2,0,0,0", False),
    "no_iterations": (_lowered_quadrupeds, {"iterations": 0}, GENERIC, True),
    "one_heavier_link": (_one_heavier_link, {}, "16,512,1,0,0,0", False),
    "no_joints": (_jointless, {}, GENERIC, True),
    "convex_pairs": (_convex, {}, "16,512,1,1,1,0", False),
}


@pytest.mark.parametrize("name", list(BREAKERS))
def test_a_broken_fact_keeps_the_generic_instance(H, name):
    make, params, generic_cfg, uni16 = BREAKERS[name]
    model = make()
    shape = _shape(H, model, **params)
    assert not shape[4] & SPEC_BIT, shape
    if uni16:  # only the fact under test stands between this model and the instance: same shape, and asking for it is refused
        assert shape[:4] == [16, 512, 1, 1]
        with pytest.raises(Exception):
            _rollout(H, model, SPEC, **params)
    r0 = _rollout(H, model, generic_cfg, **params)
    _assert_same(r0, _rollout(H, model, None, **params))
    assert np.isfinite(r0["body_q"]).all()
