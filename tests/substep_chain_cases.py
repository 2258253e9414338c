"""Scenes shared by tests/test_substep_chain_emu.py and tests/test_gpu_substep_chain.py (the pose snapshot
without its copy pass, the step's last apply without the W rebuild, the launch's outputs stored behind the substep loop)."""
import numpy as np

DT = 1e-3
CFG_SPEC, CFG_GENERIC = "16,512,1,1,0,1", "16,512,1,1,0,0"
SPEC_BIT = 4  # nt_xpbd_rollout_shape: out[4]
FLAT = ("shape0", "shape1", "point0", "point1", "offset0", "offset1", "normal", "margin0", "margin1")

# bodies of one world of kinematic_scene, in builder order
KIN, RIDER, FIXED, TOP, LOOSE = range(5)
NB_KIN = 5


def lowered(scene, n, drop=0.24, device=None, **kw):
    """n quadrupeds with the feet in the ground (live contacts); seed: per-world STATE jitter, same parameters in every world"""
    import newton_amd as nt

    model = scene(n, device=device, seed=5, **kw)
    model.joint_q.reshape(n, -1)[:, 2] -= drop
    model.body_q, model.body_qd = nt.articulation.eval_fk_numpy(model, model.joint_q, model.joint_qd)
    return model


def one_heavier_link(scene, n, device=None):
    """per-environment parameters: the model leaves the uniform-parameter tiles"""
    model = lowered(scene, n, device=device)
    model.body_mass = np.array(model.body_mass, copy=True)
    model.body_mass[13 * 3 + 2] *= 1.25  # one link of world 3
    model.body_inv_mass = np.where(model.body_mass > 0, 1.0 / np.maximum(model.body_mass, 1e-30), 0.0).astype(np.float32)
    return model


def kinematic_scene(n, device=None):
    """Uniform-parameter analytic worlds on the ground plane with the two kinds of body that leave integrate_bodies / apply_body_deltas
    early: a kinematic platform (sliding and yawing: its velocity feeds the friction rows) carrying a dynamic box, and a body of zero
    mass that is NOT kinematic (drifting: integrate_bodies moves it, the last apply gives it its origin back) carrying a dynamic
    sphere; a third dynamic body lies on the ground."""
    import newton_amd as nt

    env = nt.ModelBuilder()
    kin = env.add_body(xform=[0.0, 0.0, 0.3, 0.0, 0.0, 0.0, 1.0], is_kinematic=True)
    env.add_shape_box(kin, hx=0.4, hy=0.4, hz=0.05)
    rider = env.add_body(xform=[0.05, 0.0, 0.449, 0.0, 0.0, 0.0, 1.0])
    env.add_shape_sphere(rider, radius=0.1)
    fixed = env.add_body(xform=[1.5, 0.0, 0.3, 0.0, 0.0, 0.0, 1.0])  # (one box per world: a box-box pair would be a convex pair)
    env.add_shape_sphere(fixed, radius=0.3, cfg=nt.ModelBuilder.ShapeConfig(density=0.0))
    top = env.add_body(xform=[1.5, 0.0, 0.679, 0.0, 0.0, 0.0, 1.0])
    env.add_shape_sphere(top, radius=0.08)
    loose = env.add_body(xform=[0.0, 1.5, 0.079, 0.0, 0.0, 0.0, 1.0])
    env.add_shape_sphere(loose, radius=0.08)
    assert (kin, rider, fixed, top, loose) == (KIN, RIDER, FIXED, TOP, LOOSE)
    sc = nt.ModelBuilder()
    sc.replicate(env, n)
    sc.add_ground_plane()
    model = sc.finalize(device=device)
    assert model.body_count == n * NB_KIN
    inv_mass = np.asarray(model.body_inv_mass).reshape(n, NB_KIN)
    assert (inv_mass[:, FIXED] == 0).all() and (inv_mass[:, [RIDER, TOP, LOOSE]] > 0).all()
    qd = model.body_qd.reshape(n, NB_KIN, 6)
    qd[:, KIN, 0], qd[:, KIN, 5] = 0.5, 0.3
    qd[:, FIXED, 1], qd[:, FIXED, 5] = 0.05, 0.2
    return model


def bodies_in_contact(model, shape0, shape1):
    """set of global body indices that own a shape of a live contact (flat Contacts arrays)"""
    live = shape0 >= 0
    body = np.asarray(model.shape_body)
    return set(body[shape0[live]].tolist()) | set(body[shape1[live]].tolist())
