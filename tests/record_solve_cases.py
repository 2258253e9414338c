"""Scenes shared by tests/test_record_solve_emu.py and tests/test_gpu_record_solve.py (the contact record made
by the lane that solves it, the pair lane's shapes taken type-sorted from pair_desc).  Every scene has uniform parameters, analytic
pairs only and fits the specialised tile of 16; the worlds of a scene differ in their STATE alone."""
import numpy as np

from substep_chain_cases import CFG_GENERIC, CFG_SPEC, DT, FLAT, SPEC_BIT  # noqa: F401  (re-exported to the two test files)

NSLOT = 32  # slot lanes per world of the tile of 16 with 512 threads


def _finish(env, n, device, lift):
    """n copies of env on the ground plane; world w is raised by lift[w] (state only) and FK'd"""
    import newton_amd as nt

    sc = nt.ModelBuilder()
    sc.replicate(env, n)
    sc.add_ground_plane()
    model = sc.finalize(device=device)
    nc = model.joint_coord_count // n
    model.joint_q.reshape(n, nc)[:, 2] += np.asarray(lift, dtype=np.float32)
    model.body_q, model.body_qd = nt.articulation.eval_fk_numpy(model, model.joint_q, model.joint_qd)
    assert model.env.np_analytic == model.env.np and model.env.cpp == 4
    return model


def _filter_all(env, shapes):
    for i, a in enumerate(shapes):
        for b in shapes[i + 1:]:
            env.add_shape_collision_filter_pair(a, b)


TILT = 0.02  # [rad] a disc resting on its cap a little off level: plane_cylinder's flat mode gives the deepest rim point + three


def disc_chain_scene(n, device=None, discs=9):
    """`discs` flat cylinders in a row, each resting on an end cap on the ground plane and linked to the next by a revolute joint:
    four live contacts per disc, 36 per world -- more than the 32 slot lanes, so a contact lane takes two contacts.  The worlds sink
    into the ground by different depths."""
    import newton_amd as nt
    from newton_amd import _np_math as nm

    r, hh, pitch = 0.1, 0.03, 0.25
    q = nm.quat_from_axis_angle([1.0, 0.0, 0.0], TILT)
    env = nt.ModelBuilder()
    links, shapes, joints = [], [], []
    for k in range(discs):
        links.append(env.add_link(xform=[pitch * k, 0.0, hh + 0.002, *q]))
        shapes.append(env.add_shape_cylinder(links[-1], radius=r, half_height=hh))
    joints.append(env.add_joint_free(links[0]))
    for k in range(1, discs):
        joints.append(env.add_joint_revolute(links[k - 1], links[k], axis=[1.0, 0.0, 0.0], parent_xform=nm.transform([0.5 * pitch, 0.0, 0.0]),
                                             child_xform=nm.transform([-0.5 * pitch, 0.0, 0.0])))
    env.add_articulation(joints)
    _filter_all(env, shapes)  # (cylinder-cylinder is a convex pair)
    return _finish(env, n, device, -0.0004 * (np.arange(n) % 5))


def mixed_pairs_scene(n, device=None):
    """Both orientations of a stored pair and a pair without a static side: a cylinder in front of a world-local plane (stored
    (cylinder, plane): the pair lane's exchange), one behind it (stored (plane, cylinder): none), and two revolute-linked bodies whose
    spheres overlap (sphere-sphere, dynamic on both sides; parent filtering off).  All of them also meet the global ground plane."""
    import newton_amd as nt
    from newton_amd import _np_math as nm

    q = nm.quat_from_axis_angle([1.0, 0.0, 0.0], TILT)
    env = nt.ModelBuilder()
    a = env.add_body(xform=[0.0, 0.0, 0.031, *q])
    ca = env.add_shape_cylinder(a, radius=0.1, half_height=0.03)
    env.add_shape_plane(body=-1, width=0.0, length=0.0)
    b = env.add_body(xform=[0.4, 0.0, 0.031, *q])
    cb = env.add_shape_cylinder(b, radius=0.1, half_height=0.03)
    l0 = env.add_link(xform=[0.0, 0.6, 0.099, 0.0, 0.0, 0.0, 1.0])
    s0 = env.add_shape_sphere(l0, radius=0.1)
    l1 = env.add_link(xform=[0.19, 0.6, 0.099, 0.0, 0.0, 0.0, 1.0])
    s1 = env.add_shape_sphere(l1, radius=0.1)
    j0 = env.add_joint_free(l0)
    j1 = env.add_joint_revolute(l0, l1, axis=[0.0, 1.0, 0.0], parent_xform=nm.transform([0.095, 0.0, 0.0]),
                                child_xform=nm.transform([-0.095, 0.0, 0.0]), collision_filter_parent=False)
    env.add_articulation([j0, j1])
    _filter_all(env, [ca, cb])
    for c in (ca, cb):  # (sphere-cylinder takes MPR / GJK)
        for s in (s0, s1):
            env.add_shape_collision_filter_pair(min(c, s), max(c, s))
    return _finish(env, n, device, np.zeros(n))


def dropped_scene(n, device=None):
    """Worlds at different heights in one tile: some touch the ground from the first substep, some reach it in the middle of a
    10-substep launch, some never do.  A kinematic platform carries a sphere in every world; two revolute-linked spheres fall."""
    import newton_amd as nt
    from newton_amd import _np_math as nm

    env = nt.ModelBuilder()
    l0 = env.add_link(xform=[0.0, 0.0, 0.099, 0.0, 0.0, 0.0, 1.0])
    env.add_shape_sphere(l0, radius=0.1)
    l1 = env.add_link(xform=[0.3, 0.0, 0.099, 0.0, 0.0, 0.0, 1.0])
    env.add_shape_sphere(l1, radius=0.1)
    j0 = env.add_joint_free(l0)
    j1 = env.add_joint_revolute(l0, l1, axis=[0.0, 1.0, 0.0], parent_xform=nm.transform([0.15, 0.0, 0.0]), child_xform=nm.transform([-0.15, 0.0, 0.0]))
    env.add_articulation([j0, j1])
    kin = env.add_body(xform=[0.0, 1.0, 0.5, 0.0, 0.0, 0.0, 1.0], is_kinematic=True)
    env.add_shape_box(kin, hx=0.3, hy=0.3, hz=0.05)
    rider = env.add_body(xform=[0.0, 1.0, 0.649, 0.0, 0.0, 0.0, 1.0])
    env.add_shape_sphere(rider, radius=0.1)
    # the gap of a default shape is 0.1 per side: a sphere is admitted 0.2 above the ground, and the spheres start 1 mm inside it.
    # Falling from rest they travel g t^2 / 2 = 0.5 mm in the 10 ms of a launch: lifts of 0.201 m + a fraction of that put the first
    # contact inside the launch.  Worlds 2 (mod 8) also raise the rider off its platform: no live contact at all
    lift = np.array([0.0, 0.2012, 0.5, 0.2011, 0.0, 0.20135, 0.3, 0.1])[np.arange(n) % 8]
    model = _finish(env, n, device, lift)
    nb, nc = model.body_count // n, model.joint_coord_count // n
    model.joint_q.reshape(n, nc)[np.arange(n) % 8 == 2, 7 + 1 + 7 + 2] += 0.5  # (the rider's free joint follows l0's, l1's and the platform's)
    model.body_q, model.body_qd = nt.articulation.eval_fk_numpy(model, model.joint_q, model.joint_qd)
    model.body_qd.reshape(n, nb, 6)[:, 2, 0] = 0.4  # the platform slides: its velocity feeds the rider's friction row
    return model


SCENES = {"disc_chain": (disc_chain_scene, 17), "mixed_pairs": (mixed_pairs_scene, 16), "dropped": (dropped_scene, 16)}


def mixed_joint_f(model, n):
    """Feed-forward joint forces [n * nd] for a disc_chain model, by world (mod 4): 0 none, 1 every dof, 2 all -0.0, 3 one revolute joint
    of the chain driven and its two neighbours not (and the free root joint not)."""
    nd = model.joint_dof_count // n
    f = np.zeros((n, nd), dtype=np.float32)
    w = np.arange(n) % 4
    f[w == 1] = np.linspace(-0.4, 0.5, nd, dtype=np.float32)
    f[w == 2] = -0.0
    f[w == 3, 6 + 3] = 0.35  # (dofs 0..5 are the root's; revolute k of the chain is dof 6 + k)
    assert np.signbit(f[w == 2]).all() and not f[w == 0].any() and (f[w == 1] != 0).all()
    return f.reshape(-1)


def stored_pair_types(model):
    """(type of pair_a's shape, type of pair_b's shape, body of pair_a's shape, body of pair_b's shape) per pair of a world"""
    t = model.env
    ty, body = np.asarray(t.shape_type), np.asarray(t.shape_body)
    return [(int(ty[a]), int(ty[b]), int(body[a]), int(body[b])) for a, b in zip(t.pair_a, t.pair_b)]
