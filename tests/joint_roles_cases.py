"""Scenes and edits shared by tests/test_joint_roles_emu.py and tests/test_gpu_joint_roles.py (on the specialised
tile of 16 a joint lane keeps the launch-invariant operands of its joint in registers for the whole launch).  The scenes of
tests/lane_roles_cases.py are used as they are; this file adds the ring of 16 links that sits on and one past the bound on `nj`, the
joint edits and the bookkeeping of which joint types a scene solves."""
import numpy as np

import lane_roles_cases as base
from lane_roles_cases import CFG_GENERIC, CFG_SPEC, DT, FLAT, SPEC_BIT, SPW  # noqa: F401  (re-exported to the two test files)

# name -> (builder, worlds, substeps): the scenes of the lane-role tests
SCENES = base.SCENES
RING_LINKS, RING_WORLDS, RING_SUBSTEPS = 16, 17, 2


def ring_scene(n, device=None, closed=True):
    """A chain of 16 spheres on the ground (free joint + 15 revolute joints: nb = nj = ns = 16, np = 8, the joint lanes fill the tile's
    32 slots exactly) and, when `closed`, a distance joint from the last link back to the first, 1 cm shorter than the chain is long, so
    that it pulls: a loop-closing joint, outside the articulation, nj = 17 with nb = 16."""
    import newton_amd as nt
    from newton_amd import _np_math as nm

    env = nt.ModelBuilder()
    pitch, z = 0.25, base.R - 0.001
    bodies, shapes, joints = [], [], []
    for k in range(RING_LINKS):
        bodies.append(env.add_link(xform=[pitch * k, 0.0, z, 0.0, 0.0, 0.0, 1.0]))
        # (every second link collides: 16 pairs of 4 contact records each are more than the tile's record rows hold)
        cfg = nt.ModelBuilder.ShapeConfig(density=800.0 + 50.0 * k, has_shape_collision=k % 2 == 0)
        shapes.append(env.add_shape_sphere(bodies[-1], radius=base.R, cfg=cfg))
    joints.append(env.add_joint_free(bodies[0]))
    for k in range(1, RING_LINKS):
        joints.append(env.add_joint_revolute(bodies[k - 1], bodies[k], axis=[0.0, 1.0, 0.0], parent_xform=nm.transform([0.5 * pitch, 0.0, 0.0]),
                                             child_xform=nm.transform([-0.5 * pitch, 0.0, 0.0]), target_ke=30.0 + 5.0 * k, target_kd=0.5,
                                             limit_lower=-0.3, limit_upper=0.3))
    env.add_articulation(joints)
    if closed:
        length = pitch * (RING_LINKS - 1)
        env.add_joint_distance(bodies[-1], bodies[0], parent_xform=nm.transform([0.0, 0.0, 0.0]), child_xform=nm.transform([0.0, 0.0, 0.0]),
                               min_distance=0.0, max_distance=length - 0.01)
    base._filter_all(env, shapes)
    model = base._finish(env, n, device, -0.0004 * (np.arange(n) % 5))
    rng = np.random.default_rng(RING_LINKS + int(closed))
    model.joint_qd = rng.normal(0.0, 0.4, size=model.joint_qd.shape).astype(np.float32)
    model.body_q, model.body_qd = nt.articulation.eval_fk_numpy(model, model.joint_q, model.joint_qd)
    t = model.env
    assert (t.nb, t.nj, t.ns, t.np) == (RING_LINKS, RING_LINKS + int(closed), RING_LINKS, RING_LINKS // 2)
    return model


# joint edits of zoo_scene, applied in this order, each on top of the ones before it
JOINT_EDITS = ("disable_prismatic", "enable_prismatic", "joint_limit")
ZOO_PRISMATIC_JOINT = 2  # HUB -prismatic-> PRI (lane_roles_cases.zoo_scene: joints in builder order)


def edit_joint(model, n, which):
    """One joint edit of zoo_scene in place, the same in every world: the prismatic joint's `enabled` flag cleared or set again, or the
    lower limit of HUB -> REV.  On a host-only model the per-world table the emulated descriptor is built from follows here; on the
    device notify_model_changed does that."""
    nj = len(np.asarray(model.joint_enabled)) // n
    if which in ("disable_prismatic", "enable_prismatic"):
        on = which == "enable_prismatic"
        np.asarray(model.joint_enabled).reshape(n, nj)[:, ZOO_PRISMATIC_JOINT] = on
        if not model.is_gpu:
            model.env.joint_enabled = np.array(model.env.joint_enabled, copy=True)
            model.env.joint_enabled[ZOO_PRISMATIC_JOINT] = int(on)
    else:
        assert which == "joint_limit"
        base.edit_parameters(model, n, "joint_limit")


def live_joint_types(t):
    """{joint type: [joints of that type that the joint lanes solve]} of one world's tables: enabled, not FREE, and not between two
    bodies without mass (joint_live, nt_xpbd.hpp)"""
    import newton_amd as nt

    out = {}
    for j in range(t.nj):
        if int(t.joint_enabled[j]) and int(t.joint_type[j]) != int(nt.JointType.FREE):
            out.setdefault(int(t.joint_type[j]), []).append(j)
    return out


def assert_every_live_type_corrects(t, joint_impulse):
    """joint_impulse [worlds, 6, nj]: the child-side corrections a reporting step accumulated per joint (no joint_f in the launch: the
    feed-forward part is zero).  Every joint type the scene solves has a joint with a non-zero correction."""
    live = live_joint_types(t)
    assert live
    for jt, joints in live.items():
        assert np.any(joint_impulse[:, :, joints] != 0.0), f"no joint of type {jt} corrected anything"
