"""Scenes and edits shared by tests/test_joint_axes_emu.py and tests/test_gpu_joint_axes.py (what gather_axes makes of a joint's axes,
on the specialised tile of 16, its generic instance and the call-by-call loop) and by tests/test_spec_contact_text_emu.py and
tests/test_gpu_spec_contact_text.py (the contact lanes of the specialised tile: DESIGN.md section 3.1).  The scenes of
tests/joint_roles_cases.py are used as they are (the ring of 16 and 17 joints); this file adds the model that runs every count of axes
gather_axes knows, with axes that point the negative way, every mix of stiffness and damping, velocity targets, a disabled joint and a
world-attached parent, and the contact scenes of tests/record_solve_cases.py at 17 / 20 worlds."""
import numpy as np

import joint_roles_cases as roles
import lane_roles_cases as base
from lane_roles_cases import CFG_GENERIC, CFG_SPEC, DT, FLAT, SPEC_BIT  # noqa: F401  (re-exported to the two test files)

R = base.R
# bodies of one world of axes_scene, in builder order
HUB, REV, PRI, BALL, FIX, D6A, D6B, DIST, LOOSE, FREE = range(10)
# joints in builder order (the free body's joint follows the articulation's)
J_ROOT, J_REV, J_PRI, J_BALL, J_FIX, J_D6A, J_D6B, J_DIST, J_LOOSE, J_FREE = range(10)


def axes_scene(n, device=None):
    """One articulation on a hub:
        world -revolute (axis -z; ke > 0, kd = 0)-> HUB          a world-attached parent
        HUB -revolute (axis (0.6, -0.8, 0); ke = 0, kd > 0, velocity target, limits)-> REV
        HUB -prismatic (axis -x; ke, kd, velocity target, limits)-> PRI
        HUB -ball-> BALL                                        three angular axes, stiffness and damping both zero
        HUB -fixed-> FIX
        HUB -D6 (2 linear, 3 angular axes)-> D6A, HUB -D6 (3 linear, 2 angular axes)-> D6B
        REV -distance-> DIST, PRI -revolute (DISABLED)-> LOOSE
    and a free body.  The D6 axes mix the three kinds of drive (ke alone, kd alone, neither), carry velocity targets and limits, and half
    of them point along a negative coordinate axis: axis * lower > axis * upper there, so that gather_axes' vmin / vmax exchange the two
    ends; the limit pairs lie both ways round zero (lower > -upper and lower < -upper).  Spheres rest 1 mm inside the ground; the worlds
    differ in joint coordinates and velocities."""
    import newton_amd as nt
    from newton_amd import _np_math as nm

    B = nt.ModelBuilder
    D = B.JointDofConfig
    env = B()
    X = lambda p, q=(0.0, 0.0, 0.0, 1.0): nm.transform(p, q)  # noqa: E731
    z = R - 0.001
    pos = {HUB: (0.0, 0.0), REV: (0.3, 0.0), PRI: (-0.3, 0.0), BALL: (0.0, 0.3), FIX: (0.0, -0.3), D6A: (0.25, 0.25), D6B: (-0.25, -0.25),
           DIST: (0.6, 0.0), LOOSE: (-0.6, 0.0)}
    links, shapes = [], []
    for k in range(9):
        links.append(env.add_link(xform=[pos[k][0], pos[k][1], z, 0.0, 0.0, 0.0, 1.0]))
        shapes.append(env.add_shape_sphere(links[-1], radius=R, cfg=B.ShapeConfig(density=800.0 + 150.0 * k)))  # (no two masses equal)
    assert links == list(range(9))

    def anchors(a, b):  # the joint sits halfway between the two links
        h = 0.5 * (np.array(pos[b]) - np.array(pos[a]))
        return X([h[0], h[1], 0.0]), X([-h[0], -h[1], 0.0])

    joints = [env.add_joint_revolute(-1, HUB, axis=[0.0, 0.0, -1.0], parent_xform=X([0.0, 0.0, z]), child_xform=X([0.0, 0.0, 0.0]),
                                     target_ke=40.0, target_kd=0.0)]
    p, c = anchors(HUB, REV)
    joints.append(env.add_joint_revolute(HUB, REV, axis=[0.6, -0.8, 0.0], parent_xform=p, child_xform=c, limit_lower=-0.2, limit_upper=0.3,
                                         target_ke=0.0, target_kd=1.5, target_vel=0.4))
    p, c = anchors(HUB, PRI)
    joints.append(env.add_joint_prismatic(HUB, PRI, axis=[-1.0, 0.0, 0.0], parent_xform=p, child_xform=c, limit_lower=-0.05, limit_upper=0.08,
                                          target_ke=200.0, target_kd=5.0, target_vel=-0.1))
    p, c = anchors(HUB, BALL)
    joints.append(env.add_joint_ball(HUB, BALL, parent_xform=p, child_xform=c))
    p, c = anchors(HUB, FIX)
    joints.append(env.add_joint_fixed(HUB, FIX, parent_xform=X(p[:3], nm.quat_rpy(0.0, 0.0, 0.2)), child_xform=c))
    p, c = anchors(HUB, D6A)
    joints.append(env.add_joint_d6(
        HUB, D6A, parent_xform=p, child_xform=c,
        linear_axes=[D(axis=[0.0, -1.0, 0.0], limit_lower=-0.04, limit_upper=0.03, target_ke=50.0),
                     D(axis=2, limit_lower=-0.02, limit_upper=0.05, target_kd=2.0, target_vel=0.05)],
        angular_axes=[D(axis=[-1.0, 0.0, 0.0], limit_lower=-0.3, limit_upper=0.2, target_ke=20.0, target_kd=0.5, target_vel=0.3),
                      D(axis=1, target_kd=0.4, target_vel=-0.2), D(axis=[0.0, 0.0, -1.0], limit_lower=-0.1, limit_upper=0.25)]))
    p, c = anchors(HUB, D6B)
    joints.append(env.add_joint_d6(
        HUB, D6B, parent_xform=p, child_xform=c,
        linear_axes=[D(axis=[-1.0, 0.0, 0.0], limit_lower=-0.01, limit_upper=0.06), D(axis=1, limit_lower=-0.05, limit_upper=0.05, target_ke=80.0),
                     D(axis=[0.0, 0.0, -1.0], limit_lower=-0.03, limit_upper=0.02, target_kd=1.0, target_vel=0.1)],
        angular_axes=[D(axis=[0.0, -1.0, 0.0], limit_lower=-0.15, limit_upper=0.4, target_ke=15.0),
                      D(axis=2, target_kd=0.3, target_vel=0.25)]))
    joints.append(env.add_joint_distance(REV, DIST, parent_xform=X([0.05, 0.0, 0.0]), child_xform=X([-0.05, 0.0, 0.0]), min_distance=0.05,
                                         max_distance=0.15))
    p, c = anchors(PRI, LOOSE)
    joints.append(env.add_joint_revolute(PRI, LOOSE, axis=[0.0, 1.0, 0.0], parent_xform=p, child_xform=c, enabled=False))
    env.add_articulation(joints)
    free = env.add_body(xform=[0.0, 1.0, z, 0.0, 0.0, 0.0, 1.0])
    sf = env.add_shape_sphere(free, radius=R)
    assert free == FREE and joints == list(range(9))
    base._filter_all(env, shapes + [sf])
    model = base._finish(env, n, device, -0.0003 * (np.arange(n) % 4))
    rng = np.random.default_rng(23)
    t = model.env
    jq = model.joint_q.reshape(n, -1).copy()
    for j in range(9):
        qs, jt = int(t.joint_q_start[j]), int(t.joint_type[j])
        if jt in (int(nt.JointType.REVOLUTE), int(nt.JointType.PRISMATIC), int(nt.JointType.D6)):
            k = int(t.joint_lin_count[j] + t.joint_ang_count[j])
            jq[:, qs:qs + k] = rng.uniform(-0.06, 0.06, size=(n, k))
    model.joint_q = jq.reshape(-1).astype(np.float32)
    model.joint_qd = rng.normal(0.0, 0.3, size=model.joint_qd.shape).astype(np.float32)
    model.body_q, model.body_qd = nt.articulation.eval_fk_numpy(model, model.joint_q, model.joint_qd)
    assert (t.nb, t.nj) == (10, 10)
    return model


# name -> (builder, worlds, substeps).  17 and 20 worlds: one full tile and a ragged one
SCENES = {"axes": (axes_scene, 17, 3), "axes20": (axes_scene, 20, 2)}
RING_WORLDS, RING_SUBSTEPS, ring_scene = roles.RING_WORLDS, roles.RING_SUBSTEPS, roles.ring_scene
controls = base.controls
assert_every_live_type_corrects = roles.assert_every_live_type_corrects


def describe(t):
    """what the model holds of the list in the module docstring, from one world's tables: {fact: bool}"""
    import newton_amd as nt

    J = nt.JointType
    ty, lin, ang = (np.asarray(x) for x in (t.joint_type, t.joint_lin_count, t.joint_ang_count))
    d6 = ty == int(J.D6)
    return {"every joint type": {int(J.REVOLUTE), int(J.PRISMATIC), int(J.BALL), int(J.FIXED), int(J.DISTANCE), int(J.FREE), int(J.D6)} <= set(ty.tolist()),
            "D6 with 2 and 3 linear axes": {2, 3} <= set(lin[d6].tolist()), "D6 with 2 and 3 angular axes": {2, 3} <= set(ang[d6].tolist()),
            "one disabled joint": int((np.asarray(t.joint_enabled) == 0).sum()) == 1,
            "a solved joint with a world-attached parent": int(t.joint_parent[J_ROOT]) < 0 and int(t.joint_enabled[J_ROOT]) == 1}


def drive_mixes(model, n):
    """the (ke > 0, kd > 0) combinations among the axes of the solved, non-free joints of one world, and facts on their axes and limits"""
    import newton_amd as nt

    t, nd = model.env, model.joint_dof_count // n
    ke, kd = np.asarray(model.joint_target_ke)[:nd], np.asarray(model.joint_target_kd)[:nd]
    lo, up = np.asarray(model.joint_limit_lower)[:nd], np.asarray(model.joint_limit_upper)[:nd]
    axis = np.asarray(model.joint_axis).reshape(-1, 3)[:nd]
    tv = np.asarray(model.joint_target_qd)[:nd]
    dofs = []
    for j in range(t.nj):
        if int(t.joint_enabled[j]) and int(t.joint_type[j]) not in (int(nt.JointType.FREE), int(nt.JointType.DISTANCE)):
            s = int(t.joint_qd_start[j])
            dofs += list(range(s, s + int(t.joint_lin_count[j]) + int(t.joint_ang_count[j])))
    dofs = np.array(dofs)
    limited = dofs[(lo[dofs] > -1e3) & (up[dofs] < 1e3)]
    return {"mixes": set(zip((ke[dofs] > 0).tolist(), (kd[dofs] > 0).tolist())),
            "negative axis component": bool((axis[dofs] < 0).any()),
            "lower > -upper": bool((lo[limited] > -up[limited]).any()), "lower < -upper": bool((lo[limited] < -up[limited]).any()),
            "velocity targets": bool((tv[dofs] != 0).any())}


# uniform edits of axes_scene, applied in this order, each on top of the ones before it: the upper limit of HUB -> REV moves inside the
# current angles of some worlds; the drive of the second linear axis of D6B gets another stiffness
AXIS_EDITS = ("limit", "ke")


def edit_axes(model, n, which):
    nd = model.joint_dof_count // n
    t = model.env
    if which == "limit":
        np.asarray(model.joint_limit_upper).reshape(n, nd)[:, int(t.joint_qd_start[J_REV])] = 0.01
    else:
        assert which == "ke"
        np.asarray(model.joint_target_ke).reshape(n, nd)[:, int(t.joint_qd_start[J_D6B]) + 1] = 140.0


# ---- contact scenes of tests/test_spec_contact_text_emu.py and tests/test_gpu_spec_contact_text.py: the builders of
# tests/record_solve_cases.py at 17 or 20 worlds and 3 substeps
CONTACT_SUBSTEPS = 3


def gaining_scene(n, device=None):
    """record_solve_cases.dropped_scene (a kinematic platform carrying a sphere; two revolute-linked spheres falling) with the heights
    set so that worlds reach the ground INSIDE a launch of three substeps: a sphere is admitted 0.2 m above the ground and starts 1 mm
    inside it, so a lift of 0.201 m is the edge; falling from rest covers 10, 30, 60 um after one, two, three steps of 1 ms.  By world
    (mod 8): 0 and 4 touch from the start, 1 reaches the ground for the second substep's collide, 3 for the third's, 5 only after the
    launch, 2 (also off its platform), 6 and 7 as in dropped_scene."""
    import newton_amd as nt
    import record_solve_cases as rs

    model = rs.dropped_scene(n, device)
    nc = model.joint_coord_count // n
    was = np.array([0.0, 0.2012, 0.5, 0.2011, 0.0, 0.20135, 0.3, 0.1])[np.arange(n) % 8]
    now = np.array([0.0, 0.201005, 0.5, 0.20102, 0.0, 0.2011, 0.3, 0.1])[np.arange(n) % 8]
    model.joint_q.reshape(n, nc)[:, 2] += (now - was).astype(np.float32)
    model.body_q, model.body_qd = nt.articulation.eval_fk_numpy(model, model.joint_q, model.joint_qd)
    nb = model.body_count // n
    model.body_qd.reshape(n, nb, 6)[:, 2, 0] = 0.4  # (the platform slides, as in dropped_scene)
    return model


def _rs(name):
    def build(n, device=None):
        import record_solve_cases as rs

        return rs.SCENES[name][0](n, device)

    return build


# name -> (builder, worlds)
CONTACT_SCENES = {"disc_chain": (_rs("disc_chain"), 17), "mixed_pairs": (_rs("mixed_pairs"), 20), "gaining": (gaining_scene, 17)}
