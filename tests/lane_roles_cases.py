"""Scenes shared by tests/test_lane_roles_emu.py and tests/test_gpu_lane_roles.py (on the specialised tile of 16
an apply lane keeps the launch-invariant operands of its body in registers for the whole launch).  Every scene has uniform
parameters, analytic pairs only and fits the specialised tile; the worlds of a scene differ in their STATE alone."""
import numpy as np

from substep_chain_cases import CFG_GENERIC, CFG_SPEC, DT, FLAT, SPEC_BIT  # noqa: F401  (re-exported to the two test files)

R = 0.1  # [m] sphere radius of every link
SPW = 4  # slots per wave of the tile of 16: the second population of a shared interval starts at a multiple of it


def _finish(env, n, device, lift):
    """n copies of env on the ground plane; world w is raised by lift[w] through its FIRST free joint (state only) and FK'd"""
    import newton_amd as nt

    sc = nt.ModelBuilder()
    sc.replicate(env, n)
    sc.add_ground_plane()
    model = sc.finalize(device=device)
    nc = model.joint_coord_count // n
    q0 = int(np.asarray(model.env.joint_q_start)[list(np.asarray(model.env.joint_type)).index(int(nt.JointType.FREE))])
    model.joint_q.reshape(n, nc)[:, q0 + 2] += np.asarray(lift, dtype=np.float32)
    model.body_q, model.body_qd = nt.articulation.eval_fk_numpy(model, model.joint_q, model.joint_qd)
    assert model.env.np_analytic == model.env.np and model.env.cpp == 4
    return model


def _filter_all(env, shapes, keep=()):
    for i, a in enumerate(shapes):
        for b in shapes[i + 1:]:
            if (a, b) not in keep:
                env.add_shape_collision_filter_pair(a, b)


# bodies of one world of zoo_scene, in builder order
HUB, REV, PRI, BALL, FIX, D6, DIST, LOOSE_JOINT, FREE_A, FREE_B, KIN, ZERO = range(12)


def zoo_scene(n, device=None):
    """One articulation with every joint type the XPBD joint lanes tell apart, hung on a hub with six incident joints:
        world -revolute-> HUB (a world-attached parent: id_p < 0), HUB -revolute-> REV, HUB -prismatic-> PRI, HUB -ball-> BALL,
        HUB -fixed-> FIX, HUB -D6(linear x, angular z)-> D6, REV -distance-> DIST, PRI -revolute (DISABLED)-> LOOSE_JOINT,
    then four free bodies: FREE_A and FREE_B (overlapping spheres on the ground: FREE_A owns two pairs and is their first body),
    KIN (a kinematic box, sliding) and ZERO (a sphere of zero mass that is not kinematic, drifting).  Limits, drives and velocity
    targets on the axes; no two links of the articulation have the same mass.  Spheres rest 1 mm inside the ground; the worlds differ
    in joint coordinates and velocities."""
    import newton_amd as nt
    from newton_amd import _np_math as nm

    B = nt.ModelBuilder
    env = B()
    X = lambda p, q=(0.0, 0.0, 0.0, 1.0): nm.transform(p, q)  # noqa: E731
    z = R - 0.001
    pos = {HUB: (0.0, 0.0), REV: (0.3, 0.0), PRI: (-0.3, 0.0), BALL: (0.0, 0.3), FIX: (0.0, -0.3), D6: (0.25, 0.25), DIST: (0.6, 0.0),
           LOOSE_JOINT: (-0.6, 0.0)}
    links, shapes = [], []
    for k in range(8):
        links.append(env.add_link(xform=[pos[k][0], pos[k][1], z, 0.0, 0.0, 0.0, 1.0]))
        shapes.append(env.add_shape_sphere(links[-1], radius=R, cfg=B.ShapeConfig(density=800.0 + 150.0 * k)))  # (no two masses equal)
    assert links == list(range(8))

    def anchors(a, b):  # the joint sits halfway between the two links
        pa, pb = np.array(pos[a]), np.array(pos[b])
        h = 0.5 * (pb - pa)
        return X([h[0], h[1], 0.0]), X([-h[0], -h[1], 0.0])

    D = B.JointDofConfig
    joints = [env.add_joint_revolute(-1, HUB, axis=[0.0, 0.0, 1.0], parent_xform=X([0.0, 0.0, z]), child_xform=X([0.0, 0.0, 0.0]),
                                     target_ke=40.0, target_kd=2.0)]
    p, c = anchors(HUB, REV)
    joints.append(env.add_joint_revolute(HUB, REV, axis=[0.0, 1.0, 0.0], parent_xform=p, child_xform=c, limit_lower=-0.2, limit_upper=0.3,
                                         target_ke=100.0, target_kd=1.0))
    p, c = anchors(HUB, PRI)
    joints.append(env.add_joint_prismatic(HUB, PRI, axis=[1.0, 0.0, 0.0], parent_xform=p, child_xform=c, limit_lower=-0.05, limit_upper=0.08,
                                          target_ke=200.0, target_kd=5.0))
    p, c = anchors(HUB, BALL)
    joints.append(env.add_joint_ball(HUB, BALL, parent_xform=p, child_xform=c))
    p, c = anchors(HUB, FIX)
    joints.append(env.add_joint_fixed(HUB, FIX, parent_xform=X(p[:3], nm.quat_rpy(0.0, 0.0, 0.2)), child_xform=c))
    p, c = anchors(HUB, D6)
    joints.append(env.add_joint_d6(HUB, D6, linear_axes=[D(axis=0, limit_lower=-0.04, limit_upper=0.04)],
                                   angular_axes=[D(axis=2, target_ke=20.0, target_kd=0.5, target_vel=0.3)], parent_xform=p, child_xform=c))
    joints.append(env.add_joint_distance(REV, DIST, parent_xform=X([0.05, 0.0, 0.0]), child_xform=X([-0.05, 0.0, 0.0]), min_distance=0.05,
                                         max_distance=0.15))
    p, c = anchors(PRI, LOOSE_JOINT)
    joints.append(env.add_joint_revolute(PRI, LOOSE_JOINT, axis=[0.0, 1.0, 0.0], parent_xform=p, child_xform=c, enabled=False))
    env.add_articulation(joints)
    a = env.add_body(xform=[0.0, 1.0, z, 0.0, 0.0, 0.0, 1.0])
    sa = env.add_shape_sphere(a, radius=R)
    b = env.add_body(xform=[2.0 * R - 0.004, 1.0, z, 0.0, 0.0, 0.0, 1.0])
    sb = env.add_shape_sphere(b, radius=R)
    kin = env.add_body(xform=[1.5, 1.0, 0.049, 0.0, 0.0, 0.0, 1.0], is_kinematic=True)
    sk = env.add_shape_box(kin, hx=0.2, hy=0.2, hz=0.05)
    zero = env.add_body(xform=[-1.5, 1.0, z, 0.0, 0.0, 0.0, 1.0])
    sz = env.add_shape_sphere(zero, radius=R, cfg=B.ShapeConfig(density=0.0))
    assert (a, b, kin, zero) == (FREE_A, FREE_B, KIN, ZERO)
    _filter_all(env, shapes + [sa, sb, sk, sz], keep={(sa, sb)})
    # per-world state: the root revolute and the hub's joints a little off their rest pose, everything moving
    model = _finish(env, n, device, -0.0003 * (np.arange(n) % 4))
    rng = np.random.default_rng(11)
    t = model.env
    jq = model.joint_q.reshape(n, -1).copy()
    for j in range(8):
        qs, jt = int(t.joint_q_start[j]), int(t.joint_type[j])
        if jt in (int(nt.JointType.REVOLUTE), int(nt.JointType.PRISMATIC), int(nt.JointType.D6)):
            k = int(t.joint_lin_count[j] + t.joint_ang_count[j])
            jq[:, qs:qs + k] = rng.uniform(-0.06, 0.06, size=(n, k))
    model.joint_q = jq.reshape(-1).astype(np.float32)
    model.joint_qd = rng.normal(0.0, 0.3, size=model.joint_qd.shape).astype(np.float32)
    model.body_q, model.body_qd = nt.articulation.eval_fk_numpy(model, model.joint_q, model.joint_qd)
    qd = model.body_qd.reshape(n, 12, 6)
    qd[:, KIN, :] = 0.0
    qd[:, KIN, 0], qd[:, KIN, 5] = 0.4, 0.2  # the platform slides and yaws
    qd[:, ZERO, :] = 0.0
    qd[:, ZERO, 1], qd[:, ZERO, 5] = 0.05, 0.2  # integrate_bodies moves the massless body; the last apply gives it its origin back
    return model


def chain_scene(n, device=None, links=8):
    """`links` spheres in a row on the ground, the first on a free joint, each linked to the next by a revolute joint with a drive:
    nb = nj = ns = np = links, so `links` = 8 puts every second lane range (A0, B0, I0, S0) right behind the first population, 7 leaves
    one inert lane between them and 5 three."""
    import newton_amd as nt
    from newton_amd import _np_math as nm

    env = nt.ModelBuilder()
    pitch, z = 0.25, R - 0.001
    bodies, shapes, joints = [], [], []
    for k in range(links):
        bodies.append(env.add_link(xform=[pitch * k, 0.0, z, 0.0, 0.0, 0.0, 1.0]))
        shapes.append(env.add_shape_sphere(bodies[-1], radius=R, cfg=nt.ModelBuilder.ShapeConfig(density=800.0 + 150.0 * k)))
    joints.append(env.add_joint_free(bodies[0]))
    for k in range(1, links):
        joints.append(env.add_joint_revolute(bodies[k - 1], bodies[k], axis=[0.0, 1.0, 0.0], parent_xform=nm.transform([0.5 * pitch, 0.0, 0.0]),
                                             child_xform=nm.transform([-0.5 * pitch, 0.0, 0.0]), target_ke=30.0 + 5.0 * k, target_kd=0.5,
                                             limit_lower=-0.3, limit_upper=0.3))
    env.add_articulation(joints)
    _filter_all(env, shapes)
    model = _finish(env, n, device, -0.0004 * (np.arange(n) % 5))
    rng = np.random.default_rng(links)
    model.joint_qd = rng.normal(0.0, 0.4, size=model.joint_qd.shape).astype(np.float32)
    model.body_q, model.body_qd = nt.articulation.eval_fk_numpy(model, model.joint_q, model.joint_qd)
    t = model.env
    assert (t.nb, t.nj, t.ns, t.np) == (links, links, links, links)
    return model


# name -> (builder, worlds, substeps).  17 and 20 worlds: one full tile and a ragged one with 1 / 4 valid worlds
SCENES = {"zoo": (zoo_scene, 17, 3), "chain5": (lambda n, device=None: chain_scene(n, device, 5), 20, 2),
          "chain7": (lambda n, device=None: chain_scene(n, device, 7), 20, 2), "chain8": (lambda n, device=None: chain_scene(n, device, 8), 17, 2)}


def controls(model, n, variant):
    """(joint_f [n nd], joint_target_q [n ntq], joint_target_qd [n nd]) of control set `variant` (0, 1): both drive every axis, differently
    in every world, and differ from each other in all three arrays"""
    nd, ntq = model.joint_dof_count // n, len(np.asarray(model.joint_target_q)) // n
    rng = np.random.default_rng(100 + variant)
    f = rng.uniform(-0.3, 0.3, size=(n, nd)).astype(np.float32)
    tq = np.asarray(model.joint_target_q, dtype=np.float32).reshape(n, ntq).copy()
    tq += rng.uniform(-0.1, 0.1, size=tq.shape).astype(np.float32) * (0.5 + variant)
    tqd = rng.uniform(-0.5, 0.5, size=(n, nd)).astype(np.float32)
    return f.reshape(-1), tq.reshape(-1), tqd.reshape(-1)


EDITS = ("joint_limit", "body_mass", "shape_scale")


def edit_parameters(model, n, which):
    """One edit of zoo_scene in place, the same in every world (the model stays uniform): a joint limit, a body's mass or a shape's scale"""
    nd, nb, ns = model.joint_dof_count // n, model.body_count // n, (model.shape_count - 1) // n
    if which == "joint_limit":
        lo = np.asarray(model.joint_limit_lower).reshape(n, nd)
        lo[:, 1] = 0.01  # HUB -> REV: the lower limit moves inside the current angles of some worlds
    elif which == "body_mass":  # (a body in contact with the ground: the contact apply scales its correction by the inverse mass)
        mass = np.asarray(model.body_mass).reshape(n, nb)
        mass[:, BALL] *= 1.5
        model.body_inv_mass = np.where(model.body_mass > 0, 1.0 / np.maximum(model.body_mass, 1e-30), 0.0).astype(np.float32)
    else:
        assert which == "shape_scale"
        scale = np.asarray(model.shape_scale)[: n * ns].reshape(n, ns, 3)
        scale[:, FREE_B, 0] = R + 0.02  # (deep enough to be in the ground wherever the earlier launches left the sphere)
