"""One-iteration parity of nt_ik_solve with the float64 host path (shared by tests/test_ik_solver_emu.py and test_gpu_ik_solver.py).

Metric: |delta_dev - delta_ref|_inf / max(1, |delta_ref|_inf), delta recovered from joint_q_out through the tangent map of the
retraction, divided by 2^-24 * cond_2(A_ref) per problem (A_ref = J^T J + lambda I of the reference).  PARITY_GATE is 4 x the largest
ratio measured (fp32 summation order differs between scenes); the measured maxima are in DESIGN.md section 3.4."""
import ctypes as C

import numpy as np

from newton_amd import _lib as L
from newton_amd import ik
from newton_amd.articulation import _qinv, _qmul, _qrot, _xinv, _xmul

JT = ik.JointType
MEASURED_MAX = 0.321  # the largest ratio measured: MI355X 0.321, emulator 0.312 (both multi_art)
PARITY_GATE = 4.0 * MEASURED_MAX


class device_problem:
    """nt_ik_problem over host arrays (the emulator takes numpy arrays where the product passes device pointers)."""

    def __init__(self, solver):
        p = L.nt_ik_problem()
        p.count = len(solver.objectives)
        p.lambda_factor, p.lambda_min, p.lambda_max, p.rho_min = solver.lambda_factor, solver.lambda_min, solver.lambda_max, solver.rho_min
        self.keep = []
        for k, o in enumerate(solver.objectives):
            tgt = np.ascontiguousarray(getattr(o, o._target_name), dtype=np.float32)
            self.keep.append(tgt)
            d = p.obj[k]
            d.weight, d.target = o.weight, tgt.ctypes.data_as(C.c_void_p).value
            if isinstance(o, ik.IKObjectivePosition):
                d.type, d.link, d.offset[:3] = L.NT_IK_POSITION, o.link_index, [float(x) for x in o.link_offset]
            elif isinstance(o, ik.IKObjectiveRotation):
                d.type, d.link, d.offset[:] = L.NT_IK_ROTATION, o.link_index, [float(x) for x in o.link_offset_rotation]
                d.flags = L.NT_IK_CANONICALIZE if o.canonicalize_quat_err else 0
            else:
                d.type = L.NT_IK_JOINT_LIMIT
        self.desc = p


def _log_quat(q):
    """Rotation vector of a unit quaternion (the inverse of ik._exp_quat), shortest rotation."""
    q = q * np.where(q[:, 3:4] < 0.0, -1.0, 1.0)
    n = np.linalg.norm(q[:, :3], axis=1, keepdims=True)
    ang = 2.0 * np.arctan2(n, q[:, 3:4])
    return np.where(n > 0.0, q[:, :3] / np.where(n > 0.0, n, 1.0) * ang, 2.0 * q[:, :3])


def tangent(solver, q0, q1):
    """delta [E, nd] with q1 = q0 (+) delta: the inverse of IKSolver.retract_numpy."""
    model, t = solver.model, solver.model.env
    E = t.env_count
    q0, q1 = solver._q64(q0), solver._q64(q1)
    d = np.zeros((E, t.nd))
    com = np.asarray(model.body_com, dtype=np.float64).reshape(E, t.nb, 3)
    X_c = np.asarray(model.joint_X_c, dtype=np.float64).reshape(E, t.nj, 7)
    for j in range(t.nj):
        jt, qs, ds = int(t.joint_type[j]), int(t.joint_q_start[j]), int(t.joint_qd_start[j])
        if jt in (JT.PRISMATIC, JT.REVOLUTE, JT.D6):
            n = int(t.joint_lin_count[j] + t.joint_ang_count[j]) if jt == JT.D6 else 1
            d[:, ds:ds + n] = q1[:, qs:qs + n] - q0[:, qs:qs + n]
        elif jt == JT.BALL:
            d[:, ds:ds + 3] = _log_quat(_qmul(q1[:, qs:qs + 4], _qinv(q0[:, qs:qs + 4])))
        elif jt in (JT.FREE, JT.DISTANCE):
            c = com[:, int(t.joint_child[j])]
            Y0, Y1 = _xmul(q0[:, qs:qs + 7], _xinv(X_c[:, j])), _xmul(q1[:, qs:qs + 7], _xinv(X_c[:, j]))
            d[:, ds:ds + 3] = (Y1[:, :3] + _qrot(Y1[:, 3:], c)) - (Y0[:, :3] + _qrot(Y0[:, 3:], c))
            d[:, ds + 3:ds + 6] = _log_quat(_qmul(Y1[:, 3:], _qinv(Y0[:, 3:])))
    return d


def reference_iteration(solver, start, step=1.0):
    """One iteration of the float64 host path from ``start`` with lambda = lambda_initial: delta, A, rho, accept, cost.  Asserts the
    construction: every problem's rho is at least 0.1 away from rho_min, so that an fp32 rounding cannot flip the decision."""
    E = solver.n_problems
    lam = np.full(E, solver.lambda_initial)
    trace = []
    r0, _ = solver.evaluate_numpy(start, jacobian=False)
    q, lam1, cost, _ = solver._solve_numpy(solver._q64(start), lam, 1, step, trace)
    tr = trace[0]
    assert np.all(tr["ok"]) and np.all(np.abs(tr["rho"] - solver.rho_min) >= 0.1), "test construction: rho too close to rho_min"
    A = tr["A"] + lam[:, None, None] * np.eye(solver.model.env.nd)
    return dict(delta=tr["delta"], A=A, cond=np.linalg.cond(A), accept=tr["accept"], cost=cost, q=q, cost_in=0.5 * np.sum(r0 * r0, axis=1),
                step=step)


def one_iteration_ratio(solver, start, ref, q_out):
    """The parity metric per problem (accepted problems; a rejected problem must return its input bit for bit)."""
    acc = ref["accept"]
    q_in32 = np.asarray(start, dtype=np.float32).reshape(len(acc), -1)
    q_out = np.asarray(q_out, dtype=np.float32).reshape(len(acc), -1)
    assert np.array_equal(q_out[~acc], q_in32[~acc])
    assert acc.any()
    got = tangent(solver, q_in32, q_out) / ref["step"]
    err = np.abs(got - ref["delta"]).max(axis=1) / np.maximum(1.0, np.abs(ref["delta"]).max(axis=1))
    ratio = err / (2.0 ** -24 * ref["cond"])
    return ratio[acc]


def mirror_cost(solver, q_out):
    """(the cost the float64 host path evaluates at q_out [E], the fp32 evaluation error allowed on it).  Each of the m residual rows
    carries the rounding of fp32 FK along the chain, 1e-6 (metres; 2 vec(q_err) alike) in absolute terms, so 0.5 |r|^2 moves by at most
    |r| 1e-6 sqrt(m) + m 1e-12 / 2, plus 1e-6 relative for the fp32 sum itself."""
    r, _ = solver.evaluate_numpy(q_out, jacobian=False)
    want = 0.5 * np.sum(r * r, axis=1)
    m = r.shape[1]
    return want, np.sqrt(2.0 * want) * 1e-6 * np.sqrt(m) + 0.5 * m * 1e-12 + 1e-6 * want


def long_chain(links, device=None):
    """One world, a chain of `links` revolute joints: nd (nd + 1) / 2 rows of J^T J alone exceed the LDS of a CU from nd = 286."""
    import newton_amd as nt

    env = nt.ModelBuilder()
    cfg = nt.ModelBuilder.ShapeConfig(has_shape_collision=False)
    parent, joints = -1, []
    for k in range(links):
        b = env.add_link(xform=[0.1 * k, 0.0, 1.0, 0, 0, 0, 1])
        env.add_shape_box(b, hx=0.05, hy=0.02, hz=0.02, cfg=cfg)
        joints.append(env.add_joint_revolute(parent, b, axis=[0.0, 1.0, 0.0]))
        parent = b
    env.add_articulation(joints)
    return env.finalize(device=device)


def rejected_only_case(E, device=None):
    """An unreachable target with lambda_max = lambda_initial = 1e-5 and rho_min = 10: every step is refused."""
    from ik_cases import OFFSET, ik_case

    model, q_star, targets, start = ik_case("joint_zoo", E, 9, device=device)
    far = np.tile(np.array([[30.0, -20.0, 25.0]], dtype=np.float32), (E, 1))
    obj = [ik.IKObjectivePosition(model.env.nb - 1, OFFSET, far)]
    return model, ik.IKSolver(model, obj, lambda_initial=1e-5, lambda_max=1e-5, rho_min=10.0), start
