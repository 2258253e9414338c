"""float64 reference for newton_amd.eval_inverse_dynamics (contract: include/newton_hip_kinematics.h) that shares no S' formula with the
code under test: the velocity-dependent part of the link accelerations is a central difference of the float64 Jacobian reference of
tests/test_eval_jacobian_host.py along the motion.

With q+- = retract(q, +-h qd) -- the dof-space update of ik.IKSolver.retract_numpy, restated here -- the link accelerations at qdd = 0
are (J(q+) qd - J(q-) qd) / 2h: qd is held constant, and for constant qd that retraction is the exact trajectory of every joint type
(coordinates add; a BALL turns by exp(h w) in the parent anchor frame; a FREE / DISTANCE child's COM translates and the child turns
about it, both in the parent anchor frame).  J qdd is added, then the definition's f_l = I_l a_l + v_l x* (I_l v_l) - (m_l g, c_l x m_l g)
and tau = sum_l J_l^T f_l, all about the world origin.  J and I at q itself come from the body_q the code under test is given (the same
fp32 inputs); body_q at q+- from the float64 forward kinematics CARRYING that body_q: what the given poses deviate from eval_fk(joint_q)
-- the rounding of body_q to fp32, or the joint violation a maximal-coordinate solver leaves -- is absorbed into the child anchors as a
constant transform per joint (carried_model), so that the trajectory passes through the given poses at q (up to the normalisation of
their fp32 quaternions), every link still turns about its parent's anchor axes, and the parent poses the contract takes pivots and
axes from are the given ones.  h = 1e-4: the truncation error is O(h^2 |qd|^3), ~1e-8 of the scale;
tests/test_inverse_dynamics_host.py checks that halving h moves the result by less than 1e-7 of it."""
import copy

import numpy as np

from newton_amd.articulation import _eval_fk_float64, _qmul, _qrot, _xinv, _xmul
from newton_amd.enums import JointType as JT
from test_eval_jacobian_host import reference

H_STEP = 1e-4


def _exp_quat(d):
    n = np.linalg.norm(d, axis=1, keepdims=True)
    safe = np.where(n > 0.0, n, 1.0)
    return np.concatenate([np.where(n > 0.0, d * np.sin(0.5 * n) / safe, 0.5 * d), np.cos(0.5 * n)], axis=1)


def _unit(q):
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def retract(model, joint_q, delta):
    """joint_q (+) delta in float64, [E, nc] from [E, nc] and [E, nd] (homogeneous model)."""
    t = model.env
    E = t.env_count
    q = np.asarray(joint_q, dtype=np.float64).reshape(E, t.nc)
    d = np.asarray(delta, dtype=np.float64).reshape(E, t.nd)
    out = q.copy()
    com = np.asarray(model.body_com, dtype=np.float64).reshape(E, t.nb, 3)
    X_c = np.asarray(model.joint_X_c, dtype=np.float64).reshape(E, t.nj, 7)
    for j in range(t.nj):
        jt, qs, ds = int(t.joint_type[j]), int(t.joint_q_start[j]), int(t.joint_qd_start[j])
        if jt in (JT.PRISMATIC, JT.REVOLUTE, JT.D6):
            n = int(t.joint_lin_count[j] + t.joint_ang_count[j]) if jt == JT.D6 else 1
            out[:, qs:qs + n] = q[:, qs:qs + n] + d[:, ds:ds + n]
        elif jt == JT.BALL:
            out[:, qs:qs + 4] = _unit(_qmul(_exp_quat(d[:, ds:ds + 3]), q[:, qs:qs + 4]))
        elif jt in (JT.FREE, JT.DISTANCE):
            c = com[:, int(t.joint_child[j])]
            Y = _xmul(q[:, qs:qs + 7], _xinv(X_c[:, j]))
            qy = _unit(_qmul(_exp_quat(d[:, ds + 3:ds + 6]), Y[:, 3:]))
            cy = Y[:, :3] + _qrot(Y[:, 3:], c) + d[:, ds:ds + 3]
            out[:, qs:qs + 7] = _xmul(np.concatenate([cy - _qrot(qy, c), qy], axis=1), X_c[:, j])
    return out


def carried_model(model, body_q, joint_q):
    """A copy of the model whose child anchors X_c absorb what body_q deviates from eval_fk(joint_q): its float64 forward kinematics
    gives body_q (quaternions normalised) at joint_q.  Per joint, X_j = (F_p X_p)^-1 F_c X_c from the plain forward kinematics F, and
    the new anchor is X_c' = B_c^-1 (B_p X_p) X_j for the given poses B."""
    t = model.env
    E = t.env_count

    def unit(X):  # (fp32 quaternions are unit to 6e-8 only; the transform algebra below wants them unit)
        X = np.asarray(X, dtype=np.float64).reshape(E, -1, 7).copy()
        X[..., 3:] /= np.linalg.norm(X[..., 3:], axis=-1, keepdims=True)
        return X

    B, X_p, X_c = unit(body_q), unit(model.joint_X_p), unit(model.joint_X_c)
    out = copy.copy(model)
    out.joint_X_p, out.joint_X_c = X_p.reshape(-1, 7), X_c.reshape(-1, 7)
    F, _ = _eval_fk_float64(out, np.asarray(joint_q, dtype=np.float64).reshape(-1), np.zeros(E * t.nd))
    X_c = X_c.copy()
    for j in range(t.nj):
        p, c = int(t.joint_parent[j]), int(t.joint_child[j])
        Fa, Ba = (X_p[:, j], X_p[:, j]) if p < 0 else (_xmul(F[:, p], X_p[:, j]), _xmul(B[:, p], X_p[:, j]))
        X_j = _xmul(_xinv(Fa), _xmul(F[:, c], X_c[:, j]))
        X_c[:, j] = _xmul(_xinv(B[:, c]), _xmul(Ba, X_j))
    out.joint_X_c = unit(X_c).reshape(-1, 7)
    return out


def art_dof_ranges(model):
    """Per articulation: (first, last + 1) flat dof index."""
    d_edges = np.concatenate([np.asarray(model.joint_qd_start), [model.joint_dof_count]])
    return [(int(d_edges[b]), int(d_edges[e])) for b, e in zip(np.asarray(model.articulation_start), np.asarray(model.articulation_end))]


def pad_dofs(model, flat, D):
    """Flat per-dof values -> the public [articulation_count, D] layout (zero padding)."""
    flat = np.asarray(flat, dtype=np.float64).reshape(-1)
    out = np.zeros((int(model.articulation_count), D))
    for a, (lo, hi) in enumerate(art_dof_ranges(model)):
        out[a, :hi - lo] = flat[lo:hi]
    return out


def inverse_dynamics_reference(model, body_q, joint_q, joint_qd, joint_qdd=None, gravity=True, velocity_terms=True, h=H_STEP):
    """tau [articulation_count, D] in float64.  joint_qdd: the public [articulation_count, D] layout or None.  Homogeneous model."""
    t = model.env
    E = t.env_count
    q = np.asarray(joint_q, dtype=np.float64).reshape(E, t.nc)
    qd = np.asarray(joint_qd, dtype=np.float64).reshape(E, t.nd) if velocity_terms else np.zeros((E, t.nd))
    ref = reference(model, body_q, q.reshape(-1))
    A, D = int(model.articulation_count), ref.D
    qd_pad = pad_dofs(model, qd, D)
    qdd_pad = np.zeros((A, D)) if joint_qdd is None else np.asarray(joint_qdd, dtype=np.float64).reshape(A, D)
    zero = np.zeros(t.nd * E)
    carried = carried_model(model, body_q, q)

    def J_at(qq):
        bq, _ = _eval_fk_float64(carried, qq.reshape(-1), zero)
        return reference(carried, bq.reshape(-1, 7), qq.reshape(-1)).J

    Jp, Jm = J_at(retract(carried, q, h * qd)), J_at(retract(carried, q, -h * qd))
    v = np.einsum("arc,ac->ar", ref.J, qd_pad)
    acc = np.einsum("arc,ac->ar", ref.J, qdd_pad) + np.einsum("arc,ac->ar", Jp - Jm, qd_pad) / (2.0 * h)
    g_all = np.asarray(model.gravity, dtype=np.float64).reshape(-1, 3)
    world = np.asarray(model.articulation_world)
    starts, ends, jch = np.asarray(model.articulation_start), np.asarray(model.articulation_end), np.asarray(model.joint_child)
    tau = np.zeros((A, D))
    for a in range(A):
        g = g_all[int(world[a])] if gravity else np.zeros(3)
        for i, j in enumerate(range(int(starts[a]), int(ends[a]))):
            Il = ref.I[int(jch[j])]
            vl, al = v[a, 6 * i:6 * i + 6], acc[a, 6 * i:6 * i + 6].copy()
            al[:3] -= g  # I (g, 0) = (m g, c x m g)
            mom = Il @ vl
            f = Il @ al
            f[:3] += np.cross(vl[3:], mom[:3])
            f[3:] += np.cross(vl[3:], mom[3:]) + np.cross(vl[:3], mom[:3])
            tau[a] += ref.J[a, 6 * i:6 * i + 6].T @ f
    return tau


def id_error(tau, tau_ref, scale_ref=None):
    """The error measure of every gate: max |tau - tau_ref| / max(1, max|tau_ref| of the articulation).  scale_ref: the result the
    scale is taken from when tau is one PART of it (gravity or velocity terms alone): the fp32 kernel forms the parts from the same
    intermediate terms, whose size the whole result shows and a small part does not."""
    got = np.asarray(tau.detach().cpu().numpy() if hasattr(tau, "detach") else tau, dtype=np.float64)
    scale = np.maximum(1.0, np.abs(tau_ref if scale_ref is None else scale_ref).max(axis=1, keepdims=True))
    return float((np.abs(got - tau_ref) / scale).max())


def random_rates(model, seed, D):
    """qd ~ U(-2, 2) flat per dof and qdd ~ U(-5, 5) in the public layout (zero in the padding), float32, seeded."""
    rng = np.random.default_rng(seed)
    qd = rng.uniform(-2.0, 2.0, size=model.joint_dof_count).astype(np.float32)
    qdd = pad_dofs(model, rng.uniform(-5.0, 5.0, size=model.joint_dof_count), D).astype(np.float32)
    return qd, qdd
