"""A float64 reference for the wrench of ONE D6 joint with two or three angular axes under SolverSemiImplicit, the case tables
that exercise it, and a way to read the wrench off any implementation of the solver's step.  Holds no tests; shared by
tests/test_d6_angular_emu.py (CPU oracle, emulated kernels) and tests/test_gpu_d6_angular.py (HIP path).

The reference (`d6_wrench`) restates eval_body_joints (semi_implicit/kernels_body.py:55-520) for a D6 joint in numpy float64: the
joint frames, x_err, r_err = inverse(q_p) * q_c, v_err, w_err, the linear rows, the attach terms and the branch for two or three
angular axes.  Its decomposition of r_err into the intrinsic X-Y'-Z'' angles is scipy's `Rotation.as_euler("XYZ")` -- the piece that
is independent of the kernels' and the oracle's quat_decompose, which were written by one hand.

The read-out (`read_wrench`): the semi-implicit integrator is linear in the applied wrench, so one step of dt = 1e-3 with
angular_damping = 0 and zero gravity (run A) next to the same step on a twin model whose D6 joint is disabled (run B) gives the
joint's wrench on every body as tau = R I R^T (w_A - w_B) / dt and f = m (v_A - v_B) / dt, I and m from the model in float64.  The
parent receives (f_total, t_total + r_p x f_total), the child the negated (f_total, t_total + r_c x f_total).

Cases are worlds, not test parameters: a table is one model with one joint per world (parameters, poses and velocities differ per
world; the topology is the same), so a whole table costs two launches."""
import functools
import warnings

import numpy as np
from scipy.spatial.transform import Rotation

import newton_amd as nt
from newton_amd import _np_math as nm

DT = 1.0e-3
ATTACH_KE, ATTACH_KD = 1.0e4, 1.0e2  # SolverSemiImplicit's defaults
ANGULAR_DAMPING_SCALE = 0.01
EPS32 = float(np.finfo(np.float32).eps)
N_PERTURBATIONS = 64


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------------
def joint_force(q, qd, target_q, target_qd, target_ke, target_kd, limit_lower, limit_upper, limit_ke, limit_kd, damping):
    """joint_force (kernels_body.py:17-52): PD drive, replaced by the limit spring and damper outside [lower, upper], plus the
    passive damping."""
    limit_f = damping_f = 0.0
    target_f = target_ke * (target_q - q) + target_kd * (target_qd - qd)
    if q < limit_lower:
        limit_f = limit_ke * (limit_lower - q)
        damping_f = -limit_kd * qd
        target_f = 0.0
    elif q > limit_upper:
        limit_f = limit_ke * (limit_upper - q)
        damping_f = -limit_kd * qd
        target_f = 0.0
    return limit_f + damping_f + target_f - damping * qd


def euler_xyz(q):
    """(a, b, c) with q = Rx(a) Ry(b) Rz(c): scipy's intrinsic "XYZ" angles.  scipy warns at gimbal lock (it then sets c = 0); the
    warning is silenced here only."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        return Rotation.from_quat(q).as_euler("XYZ")


def joint_params(model, j):
    """Float64 copies of everything eval_body_joints reads for joint j."""
    f64 = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    lin, ang = (int(x) for x in np.asarray(model.joint_dof_dim).reshape(-1, 2)[j])
    d0, t0 = int(model.joint_qd_start[j]), int(model.joint_target_q_start[j])
    n = lin + ang
    parent, child = int(model.joint_parent[j]), int(model.joint_child[j])
    P = dict(parent=parent, child=child, lin=lin, ang=ang, X_p=f64(model.joint_X_p)[j].copy(), X_c=f64(model.joint_X_c)[j].copy(),
             com_c=f64(model.body_com)[child], com_p=f64(model.body_com)[parent] if parent >= 0 else None,
             axis=f64(model.joint_axis).reshape(-1, 3)[d0:d0 + n], target_q=f64(model.joint_target_q)[t0:t0 + n])
    for k, name in (("target_qd", "joint_target_qd"), ("joint_f", "joint_f"), ("target_ke", "joint_target_ke"),
                    ("target_kd", "joint_target_kd"), ("limit_lower", "joint_limit_lower"), ("limit_upper", "joint_limit_upper"),
                    ("limit_ke", "joint_limit_ke"), ("limit_kd", "joint_limit_kd"), ("damping", "joint_damping")):
        P[k] = f64(getattr(model, name))[d0:d0 + n]
    return P


def _dof_force(P, k, q, qd):
    return joint_force(q, qd, P["target_q"][k], P["target_qd"][k], P["target_ke"][k], P["target_kd"][k], P["limit_lower"][k],
                       P["limit_upper"][k], P["limit_ke"][k], P["limit_kd"][k], P["damping"][k])


def d6_wrench(P, bq_c, bqd_c, bq_p=None, bqd_p=None, attach_ke=ATTACH_KE, attach_kd=ATTACH_KD):
    """The wrenches (f, tau about the COM, world frame) a D6 joint with >= 2 angular axes applies to its parent and to its child:
    (w_parent or None, w_child), each a 6-vector.

    The "fixed" third axis of a joint with TWO angular axes: the reference solver calls joint_force for it with the attach gains
    as drive gains, target 0 -- and with limits (0, 0) and zero limit gains.  Every angle other than exactly 0 is outside those
    limits, the limit branch replaces the drive by a limit spring of stiffness 0, and the force on the third axis is ZERO for
    every non-zero angle.  That is the reference solver's behaviour (kernels_body.py:495-515), which this project mirrors; it is
    restated here as it stands and the two-axis cases with a non-zero third angle pin it."""
    X_wp = P["X_p"]
    r_p = w_p = v_p = np.zeros(3)
    if bq_p is not None:
        X_wp = nm.transform_mul(bq_p, X_wp)
        r_p = X_wp[:3] - nm.transform_point(bq_p, P["com_p"])
        w_p = bqd_p[3:]
        v_p = bqd_p[:3] + np.cross(w_p, r_p)
    X_wc = nm.transform_mul(bq_c, P["X_c"])
    r_c = X_wc[:3] - nm.transform_point(bq_c, P["com_c"])
    w_c = bqd_c[3:]
    v_c = bqd_c[:3] + np.cross(w_c, r_c)
    x_err = X_wc[:3] - X_wp[:3]
    r_err = nm.quat_mul(nm.quat_inverse(X_wp[3:]), X_wc[3:])
    v_err, w_err = v_c - v_p, w_c - w_p
    lin, ang = P["lin"], P["ang"]
    assert ang in (2, 3)
    to_world = lambda v: nm.quat_rotate(X_wp[3:], v)  # noqa: E731

    f_total, t_total = np.zeros(3), np.zeros(3)
    pos, vel = np.zeros(3), np.zeros(3)
    for k in range(lin):  # the linear rows: a drive / limit along each free axis, the attach spring on the rest
        axis_k = to_world(P["axis"][k])
        qk, qdk = np.dot(x_err, axis_k), np.dot(v_err, axis_k)
        f_total += axis_k * (-P["joint_f"][k] - _dof_force(P, k, qk, qdk))
        pos += qk * axis_k
        vel += qdk * axis_k
    f_total += (x_err - pos) * attach_ke + (v_err - vel) * attach_kd

    # the angular rows: decompose the relative rotation, transport the axes like FK does (axis 1 turned by the first rotation,
    # axis 2 by the first two), then into the world with the parent anchor
    angles = euler_xyz(r_err)
    orig = [P["axis"][lin], P["axis"][lin + 1]]
    orig.append(P["axis"][lin + 2] if ang == 3 else np.cross(orig[0], orig[1]))
    q_0 = nm.quat_from_axis_angle(orig[0], angles[0])
    axis_1 = nm.quat_rotate(q_0, orig[1])
    q_1 = nm.quat_from_axis_angle(axis_1, angles[1])
    axes = [to_world(orig[0]), to_world(axis_1), to_world(nm.quat_rotate(nm.quat_mul(q_1, q_0), orig[2]))]
    for k in range(3):
        qd = np.dot(axes[k], w_err)
        if k < ang:
            t_total += axes[k] * (-P["joint_f"][lin + k] - _dof_force(P, lin + k, angles[k], qd))
        else:  # see the docstring: zero for every non-zero angle
            t_total += axes[k] * -joint_force(angles[k], qd, 0.0, 0.0, attach_ke, attach_kd * ANGULAR_DAMPING_SCALE, 0.0, 0.0, 0.0,
                                              0.0, 0.0)
    w_child = -np.concatenate([f_total, t_total + np.cross(r_c, f_total)])
    w_parent = np.concatenate([f_total, t_total + np.cross(r_p, f_total)]) if bq_p is not None else None
    return w_parent, w_child


def read_wrench(model, qd_a, qd_b, dt=DT):
    """[B, 6] (f, tau): the wrench that turns run B's velocities into run A's in one semi-implicit step from model.body_q."""
    bq = np.asarray(model.body_q, dtype=np.float64).reshape(-1, 7)
    d = (np.asarray(qd_a, dtype=np.float64).reshape(-1, 6) - np.asarray(qd_b, dtype=np.float64).reshape(-1, 6)) / dt
    out = np.zeros_like(d)
    for b in range(len(bq)):
        R = nm.quat_to_matrix(bq[b, 3:] / np.linalg.norm(bq[b, 3:]))
        out[b, :3] = float(model.body_mass[b]) * d[b, :3]
        out[b, 3:] = R @ np.asarray(model.body_inertia, dtype=np.float64).reshape(-1, 3, 3)[b] @ R.T @ d[b, 3:]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the table for the direct comparison
# ---------------------------------------------------------------------------------------------------------------------------------
PI = np.pi
AXIS_SETS = {  # 3 axes: as listed; 2 axes: the first two, the third is their cross product
    "xyz": ([1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]),
    "xzy": ([1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0]),
    "yzx": ([0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]),
    "tilted": ([0.6, 0.8, 0.0], [-0.8, 0.6, 0.0], [0.0, 0.0, 1.0]),
}
ANGLE_ROWS = [  # (a, b, c) of r_err = Rx(a) Ry(b) Rz(c); at least 1e-3 from +-pi
    (0.4, -0.3, 0.7), (-1.3, 0.9, -2.2), (2.4, -1.1, 1.6), (-0.05, 0.02, 0.1), (1.9, 0.6, -0.8),
    (PI - 1e-3, 0.5, -0.6), (-(PI - 1e-3), -0.7, 1.2), (0.8, 0.4, PI - 1e-3), (-1.7, -0.2, -(PI - 1e-3)),
    (0.9, PI / 2 - 0.05, -0.4), (-2.1, -(PI / 2 - 0.05), 0.3), (1.2, PI / 2 - 0.01, 2.0), (-0.6, -(PI / 2 - 0.01), -1.5),
]
MODES = ("drive", "below", "above", "damped", "feedforward")


def direct_cases(ang, parent):
    """One case per (axis set, angle row): per-axis modes rotate with the case index so that every mode meets every axis, in
    changing combinations across the three axes."""
    rng = np.random.default_rng(100 * ang + (7 if parent == "free" else 0))
    cases = []
    for name, axes in AXIS_SETS.items():
        for angles in ANGLE_ROWS:
            i = len(cases)
            cases.append(dict(axes=axes[:ang], angles=angles, modes=[MODES[(i + 2 * k + i // 5) % 5] for k in range(ang)],
                              u=rng.uniform(size=(4, 8)), n=rng.normal(size=(4, 6)), axis_set=name))
    return cases


def _dof(axis, angle, mode, u):
    """One angular axis whose current coordinate is `angle`."""
    D = nt.ModelBuilder.JointDofConfig
    kw = dict(axis=list(axis), target_ke=20.0 + 60.0 * u[0], target_kd=0.5 + 1.5 * u[1],
              target_pos=angle + (0.1 + 0.3 * u[2]) * (1.0 if u[3] > 0.5 else -1.0), target_vel=0.3 + u[4])
    if mode == "below":  # the angle is 0.2 below the lower limit
        kw.update(limit_lower=angle + 0.2, limit_upper=angle + 1.2, limit_ke=50.0 + 100.0 * u[5], limit_kd=0.5 + 1.5 * u[6])
        kw["target_pos"] = angle + 0.7  # (the builder keeps target_pos within the limits)
    elif mode == "above":
        kw.update(limit_lower=angle - 1.2, limit_upper=angle - 0.2, limit_ke=50.0 + 100.0 * u[5], limit_kd=0.5 + 1.5 * u[6])
        kw["target_pos"] = angle - 0.7
    elif mode == "damped":
        kw.update(damping=0.5 + 1.5 * u[5])
    return D(**kw)


@functools.lru_cache(maxsize=None)
def _direct_host(ang, parent, enabled):
    return direct_model(ang, parent, enabled)


def direct_model(ang, parent, enabled=True, device=None):
    """The table as a model: world i holds case i.  parent == "world": the joint hangs from a rotated, offset parent_xform.
    parent == "free": from a FREE floating body that moves and spins; the joint then also has a driven linear axis, a rotated
    child_xform, anchors off both COMs and a few mm apart (x_err, v_err != 0).  enabled=False: the twin for run B."""
    D = nt.ModelBuilder.JointDofConfig
    cfg = nt.ModelBuilder.ShapeConfig(has_shape_collision=False)
    scene = nt.ModelBuilder(gravity=0.0)
    poses, ffs = [], []
    for case in direct_cases(ang, parent):
        u, n = case["u"], case["n"]
        env = nt.ModelBuilder(gravity=0.0)
        X_p = nm.transform(0.2 * n[0, :3], nm.quat_rpy(*(1.5 * n[1, :3])))
        X_c = nm.transform([-0.07, 0.02, 0.03], nm.quat_rpy(*(0.8 * n[1, 3:]))) if parent == "free" else nm.transform([-0.07, 0.02, 0.03])
        joints, lin_axes = [], []
        if parent == "free":
            pb = env.add_link(xform=[*(0.2 * n[2, :3]), *nm.quat_rpy(*(1.2 * n[2, 3:]))])
            env.add_shape_box(pb, xform=nm.transform([0.01, -0.02, 0.015]), hx=0.07, hy=0.05, hz=0.04, cfg=cfg)
            joints.append(env.add_joint_free(pb))
            lin_axes = [D(axis=0, target_ke=150.0, target_kd=3.0, target_pos=0.01, target_vel=-0.2)]
        child = env.add_link()
        env.add_shape_box(child, xform=nm.transform([0.02, -0.01, 0.015]), hx=0.06, hy=0.05, hz=0.04, cfg=cfg)
        dofs = [_dof(case["axes"][k], case["angles"][k], case["modes"][k], u[k]) for k in range(ang)]
        joints.append(env.add_joint_d6(pb if parent == "free" else -1, child, linear_axes=lin_axes, angular_axes=dofs, parent_xform=X_p,
                                       child_xform=X_c, enabled=enabled))
        env.add_articulation(joints)
        scene.add_world(env)
        # the child's pose from the wanted relative rotation (and a few mm between the anchors of the free-parent joint)
        bq_p = np.asarray(env.body_q[0], dtype=np.float64) if parent == "free" else nm.transform()
        X_wp = nm.transform_mul(bq_p, X_p)
        x_err = nm.quat_rotate(X_wp[3:], 0.003 * n[3, :3]) if parent == "free" else np.zeros(3)
        X_wc = np.array([*(X_wp[:3] + x_err), *nm.quat_mul(X_wp[3:], Rotation.from_euler("XYZ", case["angles"]).as_quat())])
        poses += ([bq_p] if parent == "free" else []) + [nm.transform_mul(X_wc, nm.transform_inverse(X_c))]
        ffs.append([(u[k, 7] - 0.5) * 4.0 if case["modes"][k] == "feedforward" else 0.0 for k in range(ang)])
    model = scene.finalize(device=device)
    model.body_q = np.asarray(poses, dtype=np.float32)
    rng = np.random.default_rng(11 + ang)
    model.body_qd = rng.normal(0.0, 1.0, size=(model.body_count, 6)).astype(np.float32)
    jf = np.zeros(model.joint_dof_count, dtype=np.float32).reshape(model.world_count, -1)
    jf[:, -ang:] = np.asarray(ffs, dtype=np.float32)
    if parent == "free":
        jf[:, -ang - 1] = 0.8  # the linear axis
    model.joint_f = jf.reshape(-1)
    return model


def _d6_joints(model):
    return [j for j in range(model.joint_count) if int(model.joint_type[j]) == int(nt.JointType.D6)]


def _ulp_step(x, sign):
    x32 = np.asarray(x, dtype=np.float32)
    return np.nextafter(x32, np.where(sign > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)).astype(np.float64)


@functools.lru_cache(maxsize=None)
def direct_reference(ang, parent):
    """(ref [B, 6], allow [B, 2]): the reference wrench on every body of the table, evaluated on the model's float32-rounded inputs,
    and per body the allowance for (f, tau): the largest change of the reference over N_PERTURBATIONS seeded perturbations of the
    input quaternions (both bodies', both anchors') by +-1 float32 ulp per component -- the reference's own sensitivity to the
    rounding of its inputs."""
    model = _direct_host(ang, parent, True)
    bq = np.asarray(model.body_q, dtype=np.float64).reshape(-1, 7)
    bqd = np.asarray(model.body_qd, dtype=np.float64).reshape(-1, 6)
    ref, allow = np.zeros((model.body_count, 6)), np.zeros((model.body_count, 2))
    rng = np.random.default_rng(2024)
    for j in _d6_joints(model):
        P = joint_params(model, j)
        p, c = P["parent"], P["child"]

        def wrench(P, qc, qp):
            return d6_wrench(P, qc, bqd[c], qp, bqd[p] if p >= 0 else None)

        w_p, w_c = wrench(P, bq[c], bq[p] if p >= 0 else None)
        ref[c] = w_c
        if p >= 0:
            ref[p] = w_p
        for _ in range(N_PERTURBATIONS):
            Q, qc, qp = dict(P), bq[c].copy(), bq[p].copy() if p >= 0 else None
            Q["X_p"], Q["X_c"] = P["X_p"].copy(), P["X_c"].copy()
            for t in (Q["X_p"], Q["X_c"], qc) + ((qp,) if p >= 0 else ()):
                t[3:] = _ulp_step(t[3:], rng.integers(0, 2, size=4) * 2 - 1)
            v_p, v_c = wrench(Q, qc, qp)
            for b, v, w in ((c, v_c, w_c),) + (((p, v_p, w_p),) if p >= 0 else ()):
                allow[b, 0] = max(allow[b, 0], np.linalg.norm(v[:3] - w[:3]))
                allow[b, 1] = max(allow[b, 1], np.linalg.norm(v[3:] - w[3:]))
    return ref, allow


def direct_ratios(step, ang, parent, device=None):
    """Runs A and B through `step(model) -> body_qd after one step of DT` and returns per body the error of the read-off wrench
    over the allowance, [B, 2] for (f, tau), together with the read-off wrench itself."""
    if device is None:
        m_a, m_b = _direct_host(ang, parent, True), _direct_host(ang, parent, False)
    else:
        m_a, m_b = direct_model(ang, parent, True, device), direct_model(ang, parent, False, device)
    got = read_wrench(m_a, step(m_a), step(m_b))
    ref, allow = direct_reference(ang, parent)
    assert np.isfinite(got).all() and np.all(allow > 0.0)
    err = np.stack([np.linalg.norm(got[:, :3] - ref[:, :3], axis=1), np.linalg.norm(got[:, 3:] - ref[:, 3:], axis=1)], axis=1)
    return err / allow, got


# ---------------------------------------------------------------------------------------------------------------------------------
# the gimbal band: the decomposition checked as a decomposition
# ---------------------------------------------------------------------------------------------------------------------------------
GIMBAL_B = (PI / 2, -PI / 2, PI / 2 - 1e-4, -(PI / 2 - 1e-4), PI / 2 - 3e-4, PI / 2 - 1e-3, -(PI / 2 - 1e-3), PI / 2 - 1e-2, 0.3)
GIMBAL_AC = ((0.4, -0.7), (-2.0, 1.1), (2.6, 2.9))
GIMBAL_KE = 50.0


def gimbal_cases():
    return [(a, b, c) for b in GIMBAL_B for (a, c) in GIMBAL_AC]


def gimbal_model(k, device=None):
    """One body at rest per world on a D6 with angular axes X, Y, Z from a rotated parent_xform, anchors at the COM; a position
    drive (stiffness GIMBAL_KE, target 0, no damping) on axis k only, so the child's torque is -GIMBAL_KE * a_k * A_k."""
    D = nt.ModelBuilder.JointDofConfig
    cfg = nt.ModelBuilder.ShapeConfig(has_shape_collision=False)
    scene = nt.ModelBuilder(gravity=0.0)
    q_p = nm.quat_rpy(0.3, -0.5, 0.8)
    poses = []
    for angles in gimbal_cases():
        env = nt.ModelBuilder(gravity=0.0)
        link = env.add_link()
        env.add_shape_box(link, hx=0.06, hy=0.05, hz=0.04, cfg=cfg)
        j = env.add_joint_d6(-1, link, angular_axes=[D(axis=a, target_ke=GIMBAL_KE if a == k else 0.0) for a in range(3)],
                             parent_xform=[0.25, -0.5, 1.0, *q_p])
        env.add_articulation([j])
        scene.add_world(env)
        poses.append([0.25, -0.5, 1.0, *nm.quat_mul(q_p, Rotation.from_euler("XYZ", angles).as_quat())])
    model = scene.finalize(device=device)
    model.body_q = np.asarray(poses, dtype=np.float32)
    model.body_qd = np.zeros((model.body_count, 6), dtype=np.float32)
    return model


def gimbal_bound(b):
    """Allowed rotation angle [rad] between Rx(a_0) Ry(a_1) Rz(a_2) and r_err: asin near 1 amplifies a rounding delta of the matrix
    entry sin(b) to sqrt(2 delta) (2e-3 at the pole for a few ulp), 16 eps32 / |cos b| away from it, plus 4e-6 for the read-out."""
    cb = abs(np.cos(b))
    return (min(2e-3, 16.0 * EPS32 / cb) if cb > 0.0 else 2e-3) + 4e-6


def gimbal_readout(step, device=None):
    """Three read-outs from rest (drive on axis 0, 1, 2 only): a_0 = -tau . A_0 / ke, A_1 built from a_0 gives a_1, A_2 built
    from both gives a_2.  Returns per case (angles read [3], rotation angle between Rx(a_0) Ry(a_1) Rz(a_2) and r_err, bound)."""
    models = [gimbal_model(k, device) for k in range(3)]
    taus = []
    for m in models:
        qd = np.asarray(step(m), dtype=np.float64).reshape(-1, 6)
        assert np.isfinite(qd).all()
        taus.append(read_wrench(m, qd, np.zeros_like(qd))[:, 3:])
    m = models[0]
    bq = np.asarray(m.body_q, dtype=np.float64).reshape(-1, 7)
    out = []
    for i, (_, b, _) in enumerate(gimbal_cases()):
        q_p = np.asarray(m.joint_X_p, dtype=np.float64)[i, 3:]
        r_err = nm.quat_mul(nm.quat_inverse(q_p), bq[i, 3:])
        e = np.eye(3)
        a0 = -np.dot(taus[0][i], nm.quat_rotate(q_p, e[0])) / GIMBAL_KE
        q_0 = nm.quat_from_axis_angle(e[0], a0)
        axis_1 = nm.quat_rotate(q_0, e[1])
        a1 = -np.dot(taus[1][i], nm.quat_rotate(q_p, axis_1)) / GIMBAL_KE
        q_1 = nm.quat_from_axis_angle(axis_1, a1)
        a2 = -np.dot(taus[2][i], nm.quat_rotate(q_p, nm.quat_rotate(nm.quat_mul(q_1, q_0), e[2]))) / GIMBAL_KE
        angle = (Rotation.from_euler("XYZ", [a0, a1, a2]).inv() * Rotation.from_quat(r_err)).magnitude()
        out.append((np.array([a0, a1, a2]), float(angle), gimbal_bound(b)))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the checks, shared by the oracle / emulator module and the device module
# ---------------------------------------------------------------------------------------------------------------------------------
# x the reference's own sensitivity to float32 rounding of its input quaternions.  Fixed from the CPU oracle's worst error / allowance
# ratio (3.77 on the force of one case, see tests/test_d6_angular_emu.py) with about 4x headroom, before the emulator or the device were looked at: the rest of
# the error is the fp32 arithmetic of the joint phase itself (anchor positions of 0.1 .. 1 m times the attach stiffness 1e4) and of the
# read-out (velocities of 1 m/s over dt = 1e-3), which a perturbation of the quaternions alone does not excite.
MARGIN = 16.0
TABLES = [(2, "world"), (3, "world"), (2, "free"), (3, "free")]
STEPWISE = {"xpbd": (1e-3, 1e-5, 1e-3), "semi": (1e-4, 1e-5, 3e-4), "fs": (1e-3, 1e-5, 3e-4)}  # dt, tol_q, tol_qd: the joint zoo's


def check_direct(step, ang, parent, device=None, tag=""):
    ratios, got = direct_ratios(step, ang, parent, device)
    cases = direct_cases(ang, parent)
    per_case = ratios.reshape(len(cases), -1, 2)
    worst = per_case.max(axis=1)
    print(f"[d6 direct {tag}] ang={ang} parent={parent}: worst error / allowance force {worst[:, 0].max():.2f} torque {worst[:, 1].max():.2f}"
          f" (|tau| {np.linalg.norm(got[:, 3:], axis=1).min():.2g} .. {np.linalg.norm(got[:, 3:], axis=1).max():.2g})")
    bad = [(i, cases[i]["axis_set"], cases[i]["angles"], cases[i]["modes"], worst[i]) for i in range(len(cases)) if worst[i].max() > MARGIN]
    assert not bad, bad
    return worst.max(axis=0)


def check_gimbal(step, device=None, tag=""):
    res = gimbal_readout(step, device)
    cases = gimbal_cases()
    worst = max(angle / bound for _, angle, bound in res)
    print(f"[d6 gimbal {tag}] worst rotation angle / bound {worst:.3f}; worst angle {max(a for _, a, _ in res):.2e} rad")
    for (a, b, c), (read, angle, bound) in zip(cases, res):
        assert np.isfinite(read).all()
        assert angle <= bound, (a, b, c, read, angle, bound)
        if abs(np.cos(b)) <= 1e-4:  # the gimbal branch folds the third angle into the first
            assert abs(read[2]) <= 1e-6, (a, b, c, read)
    return worst


def rel_error(a, b, floor=1.0):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), floor)))


def fk_residual(model, body_q, joint_q):
    """Largest difference between every joint's relative transform inverse(X_wp) * X_wc, composed in float64 from body_q, and the joint
    transform its joint_q stands for -- for a D6, scipy's intrinsic Euler rotation about the listed axes (the way
    tests/test_kinematics.py checks the host FK).  Quaternions up to sign."""
    from scipy.spatial.transform import Rotation

    import newton_amd as nt
    from newton_amd import _np_math as nm

    t = model.env
    E = t.env_count
    bq = np.asarray(body_q, dtype=np.float64).reshape(E, t.nb, 7)
    jq = np.asarray(joint_q, dtype=np.float64).reshape(E, t.nc)
    X_p = np.asarray(model.joint_X_p, dtype=np.float64).reshape(E, t.nj, 7)
    X_c = np.asarray(model.joint_X_c, dtype=np.float64).reshape(E, t.nj, 7)
    axis = np.asarray(model.joint_axis, dtype=np.float64).reshape(E, t.nd, 3)
    worst = 0.0
    for e in range(E):
        for j in range(t.nj):
            qs, ds, jt = int(t.joint_q_start[j]), int(t.joint_qd_start[j]), int(t.joint_type[j])
            lin, ang = int(t.joint_lin_count[j]), int(t.joint_ang_count[j])
            if jt == nt.JointType.FREE:
                want = jq[e, qs:qs + 7]
            else:
                p = sum((jq[e, qs + k] * axis[e, ds + k] for k in range(lin)), np.zeros(3))
                rot = Rotation.identity()
                for k in range(ang):  # intrinsic: each rotation about its axis as carried along by the earlier ones
                    rot = rot * Rotation.from_rotvec(jq[e, qs + lin + k] * axis[e, ds + lin + k])
                want = np.array([*p, *rot.as_quat()])
            parent = int(t.joint_parent[j])
            X_wp = X_p[e, j] if parent < 0 else nm.transform_mul(bq[e, parent], X_p[e, j])
            rel = nm.transform_mul(nm.transform_inverse(X_wp), nm.transform_mul(bq[e, int(t.joint_child[j])], X_c[e, j]))
            worst = max(worst, min(np.abs(rel[3:] - want[3:]).max(), np.abs(rel[3:] + want[3:]).max()), np.abs(rel[:3] - want[:3]).max())
    return float(worst)
