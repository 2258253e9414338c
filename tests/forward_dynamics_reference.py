"""float64 reference for newton_amd.eval_forward_dynamics (contract: include/newton_hip_kinematics.h) that shares no solve with the code
under test:
  H_ref        the mass-matrix reference of tests/test_eval_jacobian_host.py (sum_l J_l^T I_l J_l from the definition)
  h_ref        inverse_dynamics_reference(qdd=None): a finite difference of the Jacobian reference along the motion
  tau_ext_ref  sum_l J_ref,l^T w_l, the wrench (F, T) at the link's COM carried to the world origin in float64: (F, T + c_l x F)
  b_ref        joint_f + tau_ext_ref - h_ref
  qdd_ref      numpy.linalg.solve(H_ref, b_ref), articulation by articulation (LU with pivoting: not a Cholesky)

Error measure of every gate, per articulation: the normwise backward error
  eta = |H_ref qdd - b_ref|_inf / (|H_ref|_inf |qdd|_inf + max(1, |joint_f|_inf, |h_ref|_inf, |tau_ext_ref|_inf))
which a correct fp32 Cholesky keeps near D 2^-24 whatever the conditioning (cond(H) reaches 4e4 on the scenes: the plain forward error
of an fp32 solve is ~1e-4 of max|qdd| with no defect anywhere, so it is printed and never asserted).  The second term of the denominator
is the scale on which eval_inverse_dynamics is accurate: where joint_f cancels h, |b_ref| alone would under-scale the kernel's h."""
import numpy as np

from inverse_dynamics_reference import art_dof_ranges, inverse_dynamics_reference, pad_dofs
from newton_amd.articulation import _qrot
from test_eval_jacobian_host import reference


class FdReference:
    """H [A, D, D], h, tau_ext, b, qdd [A, D] in float64, nda [A] and cond [A] (2-norm condition number of the live block)."""


def external_torque_reference(model, body_q, ref, body_f):
    """sum_l J_ref,l^T (F_l, T_l + c_l x F_l) per articulation, [A, D] in float64."""
    bq = np.asarray(body_q, dtype=np.float64).reshape(-1, 7)
    com = np.asarray(model.body_com, dtype=np.float64).reshape(-1, 3)
    w = np.asarray(body_f, dtype=np.float64).reshape(-1, 6)
    cw = bq[:, :3] + _qrot(bq[:, 3:], com)
    starts, ends, jch = np.asarray(model.articulation_start), np.asarray(model.articulation_end), np.asarray(model.joint_child)
    out = np.zeros((len(starts), ref.D))
    for a in range(len(starts)):
        for i, j in enumerate(range(int(starts[a]), int(ends[a]))):
            b = int(jch[j])
            out[a] += ref.J[a, 6 * i:6 * i + 6].T @ np.concatenate([w[b, :3], w[b, 3:] + np.cross(cw[b], w[b, :3])])
    return out


def forward_dynamics_reference(model, body_q, joint_q, joint_qd, joint_f=None, body_f=None, gravity=True, velocity_terms=True):
    """Homogeneous model.  joint_f: the public [articulation_count, D] layout or None; body_f [body_count, 6] or None."""
    ref = reference(model, body_q, np.asarray(joint_q, dtype=np.float64).reshape(-1))
    A, D = int(model.articulation_count), ref.D
    out = FdReference()
    out.H = ref.H
    out.h = inverse_dynamics_reference(model, body_q, joint_q, joint_qd, None, gravity, velocity_terms)
    out.joint_f = np.zeros((A, D)) if joint_f is None else np.asarray(joint_f, dtype=np.float64).reshape(A, D)
    out.tau_ext = np.zeros((A, D)) if body_f is None else external_torque_reference(model, body_q, ref, body_f)
    out.b = out.joint_f + out.tau_ext - out.h
    out.nda = np.array([hi - lo for lo, hi in art_dof_ranges(model)])
    out.qdd, out.cond = np.zeros((A, D)), np.ones(A)
    for a, n in enumerate(out.nda):
        if n:
            out.qdd[a, :n] = np.linalg.solve(ref.H[a, :n, :n], out.b[a, :n])
            out.cond[a] = np.linalg.cond(ref.H[a, :n, :n])
    return out


def _np64(x):
    return np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x, dtype=np.float64)


def fd_denominator(ref, qdd):
    """[A]: |H_ref|_inf |qdd|_inf + max(1, |joint_f|_inf, |h_ref|_inf, |tau_ext_ref|_inf)."""
    q = _np64(qdd)
    H_norm = np.abs(ref.H).sum(axis=2).max(axis=1)
    scale = np.maximum(1.0, np.maximum(np.abs(ref.joint_f).max(axis=1), np.maximum(np.abs(ref.h).max(axis=1), np.abs(ref.tau_ext).max(axis=1))))
    return H_norm * np.abs(q).max(axis=1) + scale


def fd_eta(qdd, ref):
    """The largest backward error over the articulations (NaN if qdd holds one)."""
    q = _np64(qdd)
    res = np.abs(np.einsum("aij,aj->ai", ref.H, q) - ref.b).max(axis=1)
    eta = res / fd_denominator(ref, q)
    return float(eta.max()) if np.all(np.isfinite(eta)) else float("nan")


def fd_forward_error(qdd, ref):
    """|qdd - qdd_ref|_inf / max(1, |qdd_ref|_inf), the largest over the articulations: for the record, nothing asserts on it."""
    q = _np64(qdd)
    return float((np.abs(q - ref.qdd).max(axis=1) / np.maximum(1.0, np.abs(ref.qdd).max(axis=1))).max())


def random_forces(model, seed, D):
    """joint_f ~ U(-10, 10) in the public layout (zero in the padding) and body_f [body_count, 6]: force ~ U(-20, 20), torque
    ~ U(-2, 2); float32, seeded."""
    rng = np.random.default_rng(seed)
    joint_f = pad_dofs(model, rng.uniform(-10.0, 10.0, size=model.joint_dof_count), D).astype(np.float32)
    body_f = np.concatenate([rng.uniform(-20.0, 20.0, size=(model.body_count, 3)), rng.uniform(-2.0, 2.0, size=(model.body_count, 3))],
                            axis=1).astype(np.float32)
    return joint_f, body_f
