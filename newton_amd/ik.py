"""Batched inverse kinematics: position / rotation / joint-limit objectives solved by Levenberg-Marquardt, one problem per world of a
replicated model (the capability of the reference's ``newton.ik.IKSolver``; the reference takes ``n_problems`` beside a
single-articulation model -- here the problems ARE the worlds, and the variables are all dofs of a world).

On a GPU model ``IKSolver.step`` is one launch of ik_solve_kernel (nt_ik_solve, include/newton_hip_kinematics.h -- the contract is
written there): all iterations inside it, no allocation, no synchronisation, recordable by ``newton_amd.graph.capture``.  On a host
model the same algorithm runs in numpy, float64 inside, vectorised over the worlds; that path is the reference the kernel is tested
against.  Not provided: samplers / multiple seeds, L-BFGS, autodiff Jacobians, per-problem masks."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .articulation import (_eval_fk_float64, _host_array, _motion_subspace_numpy, _path_matrix, _qinv, _qmul, _qrot, _xinv, _xmul,
                           check_ik_supported)
from .enums import MAXVAL, JointType

MAX_OBJECTIVES = 8  # NT_IK_MAX_OBJECTIVES


def predicted_reduction(step_size, lam, delta_dot_delta, g_dot_delta):
    """C - m(s delta) of the quadratic model m(p) = C + g.p + p.J^T J p / 2 for the scaled step, with (J^T J + lambda I) delta = -g:
    s (s lambda delta.delta - (2 - s) g.delta) / 2; for s = 1 it is delta.(lambda delta - g) / 2.  The kernel evaluates the same
    expression (ik_solve_kernel)."""
    return 0.5 * step_size * (step_size * lam * delta_dot_delta - (2.0 - step_size) * g_dot_delta)


def _exp_quat(d):
    """exp of a rotation vector as a quaternion (xyzw): (d sin(|d| / 2) / |d|, cos(|d| / 2)); (d / 2, 1) at d = 0."""
    a = np.linalg.norm(d, axis=-1, keepdims=True)
    s = np.where(a > 0.0, np.sin(0.5 * a) / np.where(a > 0.0, a, 1.0), 0.5)
    return np.concatenate([d * s, np.where(a > 0.0, np.cos(0.5 * a), 1.0)], axis=-1)


def _unit(q):
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def _target_array(values):
    """A private copy of the caller's targets: float32; a float64 numpy array keeps its precision (host models only -- a GPU model
    rounds it to float32 when the solver takes the objective)."""
    a = _host_array(values)
    return np.array(a, dtype=np.float64 if getattr(a, "dtype", None) == np.float64 else np.float32)


def _resident(values, shape, what):
    a = np.array(_host_array(values), dtype=np.float32)
    if a.size != int(np.prod(shape)):
        raise ValueError(f"{what} must have shape {tuple(shape)}, got {tuple(np.shape(values))}")
    return np.ascontiguousarray(a.reshape(shape))


def _assign(dst, values, what):
    """In-place copy into the resident array (numpy on a host model, a device tensor on a GPU model): the storage stays."""
    if hasattr(dst, "copy_"):
        import torch  # noqa: PLC0415

        src = values if hasattr(values, "data_ptr") else torch.from_numpy(np.ascontiguousarray(_host_array(values), dtype=np.float32))
        if src.numel() != dst.numel():
            raise ValueError(f"{what} must have shape {tuple(dst.shape)}")
        dst.copy_(src.reshape(dst.shape))
    else:
        src = np.asarray(_host_array(values), dtype=dst.dtype)
        if src.size != dst.size:
            raise ValueError(f"{what} must have shape {dst.shape}")
        dst[...] = src.reshape(dst.shape)


def _cholesky_solve(A, b):
    """x [E, n] with A x = b by Cholesky, batched over the worlds, and ok [E]: False (x = 0) where A has a non-positive pivot.  numpy's
    batched factorisation raises when ANY matrix fails; only then the worlds are factored one by one to find which."""
    ok = np.ones(len(A), dtype=bool)
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        L = np.broadcast_to(np.eye(A.shape[1]), A.shape).copy()
        for e in range(len(A)):
            try:
                L[e] = np.linalg.cholesky(A[e])
            except np.linalg.LinAlgError:
                ok[e] = False
    y = np.linalg.solve(L, b[:, :, None])
    x = np.linalg.solve(np.swapaxes(L, 1, 2), y)[:, :, 0]
    return np.where(ok[:, None], x, 0.0), ok


class IKObjectivePosition:
    """Brings the point ``link_offset`` (link frame) of body ``link_index`` (world-local) to ``target_positions`` [n_problems, 3].
    Residual ``w (p + rot(q, offset) - target)``, Jacobian rows ``w (v + omega x (p + rot(q, offset)))``."""

    def __init__(self, link_index, link_offset, target_positions, weight=1.0):
        self.link_index, self.weight = int(link_index), float(weight)
        self.link_offset = np.asarray(_host_array(link_offset), dtype=np.float32).reshape(-1)
        if self.link_offset.shape != (3,):
            raise ValueError("link_offset must have 3 components")
        self.target_positions = _target_array(target_positions)
        if self.target_positions.ndim != 2 or self.target_positions.shape[1] != 3:
            raise ValueError("target_positions must have shape [n_problems, 3]")

    def set_target_positions(self, x):
        _assign(self.target_positions, x, "target_positions")

    _target_name = "target_positions"


class IKObjectiveRotation:
    """Brings ``q * link_offset_rotation`` of body ``link_index`` to ``target_rotations`` [n_problems, 4] (xyzw).  Residual
    ``w * 2 * vec(q_err)``, ``q_err = (q * offset) * conj(target)``, negated when its w < 0 with ``canonicalize_quat_err``.  The
    Jacobian rows are ``w omega``: the Gauss-Newton approximation, exact at zero rotation error (it drops the factor that maps an
    angular velocity onto the rate of ``2 vec(q_err)``, which tends to the identity as the error vanishes)."""

    def __init__(self, link_index, link_offset_rotation, target_rotations, canonicalize_quat_err=True, weight=1.0):
        self.link_index, self.weight = int(link_index), float(weight)
        self.canonicalize_quat_err = bool(canonicalize_quat_err)
        self.link_offset_rotation = np.asarray(_host_array(link_offset_rotation), dtype=np.float32).reshape(-1)
        if self.link_offset_rotation.shape != (4,):
            raise ValueError("link_offset_rotation must have 4 components (xyzw)")
        self.target_rotations = _target_array(target_rotations)
        if self.target_rotations.ndim != 2 or self.target_rotations.shape[1] != 4:
            raise ValueError("target_rotations must have shape [n_problems, 4]")

    def set_target_rotations(self, q):
        _assign(self.target_rotations, q, "target_rotations")

    _target_name = "target_rotations"


class IKObjectiveJointLimit:
    """One row per dof of a PRISMATIC / REVOLUTE / D6 joint with ``lower < upper``, both finite:
    ``w (max(0, q - upper) - max(0, lower - q))``.  ``None``: the model's own limits; else arrays of ``joint_dof_count`` entries."""

    def __init__(self, joint_limit_lower=None, joint_limit_upper=None, weight=1.0):
        self.joint_limit_lower, self.joint_limit_upper, self.weight = joint_limit_lower, joint_limit_upper, float(weight)
        self.limits = None  # [n_problems, 2 nd] (lower, upper) once bound to a solver

    _target_name = "limits"


class IKSolver:
    """Levenberg-Marquardt over the stacked objectives.  Per iteration: ``A = J^T J + lambda I``, ``g = J^T r``, ``A delta = -g`` by
    Cholesky, ``q' = q (+) step_size delta``; accepted when the predicted reduction (:func:`predicted_reduction`) is positive, the cost
    fell and ``rho = (C - C') / pred > rho_min`` -- then ``lambda <- max(lambda / lambda_factor, lambda_min)``, otherwise ``q`` stays bit
    for bit and ``lambda <- min(lambda lambda_factor, lambda_max)`` (a non-positive pivot is a rejection).  ``lambdas`` persist across
    ``step`` calls (``reset`` restores ``lambda_initial``); ``costs`` holds the cost ``|r|^2 / 2`` at the returned ``joint_q_out``.

    Refused with NotImplementedError: heterogeneous models, worlds with a body that is no joint's child or a joint outside any
    articulation, a multi-axis D6 that ``check_ik_supported`` refuses, more than ``MAX_OBJECTIVES`` objectives, and (at ``step``) a
    tile that does not fit the LDS."""

    def __init__(self, model, objectives, lambda_initial=0.1, lambda_factor=2.0, lambda_min=1e-5, lambda_max=1e10, rho_min=1e-3):
        if getattr(model, "is_heterogeneous", False):
            raise NotImplementedError("IKSolver: heterogeneous models are unsupported (one problem is one world of a replicated model)")
        t = model.env
        if t.nj == 0 or t.na == 0 or t.nd == 0 or np.any(np.asarray(model.joint_articulation) == -1):
            raise NotImplementedError("IKSolver: needs articulations that cover every world's joints (unsupported)")
        if set(int(b) for b in t.joint_child) != set(range(t.nb)):
            raise NotImplementedError("IKSolver: a world has a body that is no joint's child (unsupported)")
        check_ik_supported(model)
        objectives = list(objectives)
        if len(objectives) > MAX_OBJECTIVES:
            raise NotImplementedError(f"IKSolver: more than {MAX_OBJECTIVES} objectives are unsupported")
        self.model, self.objectives = model, objectives
        self.lambda_initial, self.lambda_factor = float(lambda_initial), float(lambda_factor)
        self.lambda_min, self.lambda_max, self.rho_min = float(lambda_min), float(lambda_max), float(rho_min)
        E = self.n_problems
        self._gpu = bool(getattr(model, "is_gpu", False))
        for o in objectives:
            if isinstance(o, IKObjectiveJointLimit):
                lim = []
                for given, own in ((o.joint_limit_lower, model.joint_limit_lower), (o.joint_limit_upper, model.joint_limit_upper)):
                    lim.append(_resident(own if given is None else given, (E, t.nd), "joint limits"))
                o.limits = np.ascontiguousarray(np.concatenate(lim, axis=1))
            elif isinstance(o, (IKObjectivePosition, IKObjectiveRotation)):
                if not 0 <= o.link_index < t.nb:
                    raise ValueError(f"link_index {o.link_index} is outside the world's {t.nb} bodies")
                tgt = getattr(o, o._target_name)
                if tgt.shape[0] != E:  # (a device tensor too: an objective taken over from another solver)
                    raise ValueError(f"{o._target_name} has {tgt.shape[0]} rows, the model has {E} worlds")
            else:
                raise TypeError(f"IKSolver: {type(o).__name__} is not an IK objective")
        # host-side tables
        self._on = _path_matrix(t)
        self._dof_joint = np.searchsorted(t.joint_qd_start, np.arange(t.nd), side="right") - 1
        self._link_joint = {int(b): j for j, b in enumerate(t.joint_child)}
        limited = np.isin(np.asarray(t.joint_type)[self._dof_joint], [int(JointType.PRISMATIC), int(JointType.REVOLUTE), int(JointType.D6)])
        self._limit_types = limited
        self._dof_coord = np.where(limited, np.asarray(t.joint_q_start)[self._dof_joint] + np.arange(t.nd)
                                   - np.asarray(t.joint_qd_start)[self._dof_joint], 0)
        if self._gpu:
            import torch  # noqa: PLC0415

            from . import _lib  # noqa: PLC0415

            dev = model.device_model().device
            for o in objectives:
                cur = getattr(o, o._target_name)
                if not hasattr(cur, "copy_"):
                    setattr(o, o._target_name, torch.from_numpy(np.asarray(cur, dtype=np.float32)).to(dev).contiguous())
            self.lambdas = torch.full((E,), self.lambda_initial, dtype=torch.float32, device=dev)
            self.costs = torch.zeros(E, dtype=torch.float32, device=dev)
            p = _lib.nt_ik_problem()
            p.count = len(objectives)
            p.lambda_factor, p.lambda_min, p.lambda_max, p.rho_min = self.lambda_factor, self.lambda_min, self.lambda_max, self.rho_min
            for k, o in enumerate(objectives):
                d = p.obj[k]
                d.weight, d.target = o.weight, getattr(o, o._target_name).data_ptr()
                if isinstance(o, IKObjectivePosition):
                    d.type, d.link, d.offset[:3] = _lib.NT_IK_POSITION, o.link_index, [float(x) for x in o.link_offset]
                elif isinstance(o, IKObjectiveRotation):
                    d.type, d.link, d.offset[:] = _lib.NT_IK_ROTATION, o.link_index, [float(x) for x in o.link_offset_rotation]
                    d.flags = _lib.NT_IK_CANONICALIZE if o.canonicalize_quat_err else 0
                else:
                    d.type = _lib.NT_IK_JOINT_LIMIT
            self._problem = p
        else:
            self.lambdas = np.full(E, self.lambda_initial, dtype=np.float32)
            self.costs = np.zeros(E, dtype=np.float32)

    @property
    def n_problems(self):
        return int(self.model.env.env_count)

    def reset(self):
        """lambdas back to lambda_initial (in place)."""
        if hasattr(self.lambdas, "fill_"):
            self.lambdas.fill_(self.lambda_initial)
        else:
            self.lambdas[...] = self.lambda_initial

    # -----------------------------------------------------------------------------------------------------------------------------
    # the float64 host mathematics (the reference of the kernel): residuals, Jacobian, retraction
    # -----------------------------------------------------------------------------------------------------------------------------
    def _q64(self, joint_q):
        t = self.model.env
        q = np.asarray(_host_array(joint_q), dtype=np.float64)
        if q.size != t.env_count * t.nc:
            raise ValueError(f"joint_q must have {t.env_count * t.nc} entries ([joint_coord_count] or [n_problems, {t.nc}])")
        return q.reshape(t.env_count, t.nc)

    def evaluate_numpy(self, joint_q, jacobian=True):
        """(r [E, m], J [E, m, nd] or None) in float64 at ``joint_q``; the rows in objective order (a joint-limit objective has one
        row per dof, zero for dofs without limits)."""
        t = self.model.env
        E, nd = t.env_count, t.nd
        q = self._q64(joint_q)
        bq, _ = _eval_fk_float64(self.model, q, np.zeros(E * nd))
        S = _motion_subspace_numpy(self.model, bq, q) if jacobian else None
        rs, Js = [], []
        for o in self.objectives:
            w = o.weight
            tgt = np.asarray(_host_array(getattr(o, o._target_name)), dtype=np.float64)
            if isinstance(o, IKObjectiveJointLimit):
                lo, hi = tgt[:, :nd], tgt[:, nd:]
                active = self._limit_types[None, :] & (lo < hi) & (np.abs(lo) < MAXVAL) & (np.abs(hi) < MAXVAL)
                qd = q[:, self._dof_coord]
                r = np.where(active, w * (np.maximum(0.0, qd - hi) - np.maximum(0.0, lo - qd)), 0.0)
                rs.append(r)
                if jacobian:
                    J = np.zeros((E, nd, nd))
                    J[:, np.arange(nd), np.arange(nd)] = np.where(r != 0.0, w, 0.0)
                    Js.append(J)
                continue
            X = bq[:, o.link_index]
            mask = self._on[self._link_joint[o.link_index], self._dof_joint].astype(np.float64)
            if isinstance(o, IKObjectivePosition):
                P = X[:, :3] + _qrot(X[:, 3:], np.asarray(o.link_offset, dtype=np.float64))
                rs.append(w * (P - tgt))
                if jacobian:
                    Js.append(np.swapaxes(w * (S[:, :, :3] + np.cross(S[:, :, 3:], P[:, None, :])) * mask[None, :, None], 1, 2))
            else:
                qe = _qmul(_qmul(X[:, 3:], np.asarray(o.link_offset_rotation, dtype=np.float64)), _qinv(tgt))
                if o.canonicalize_quat_err:
                    qe = qe * np.where(qe[:, 3:4] < 0.0, -1.0, 1.0)
                rs.append(2.0 * w * qe[:, :3])
                if jacobian:
                    Js.append(np.swapaxes(w * S[:, :, 3:] * mask[None, :, None], 1, 2))
        r = np.concatenate(rs, axis=1) if rs else np.zeros((E, 0))
        return r, (np.concatenate(Js, axis=1) if rs else np.zeros((E, 0, nd))) if jacobian else None

    def retract_numpy(self, joint_q, delta):
        """``joint_q (+) delta`` in float64: [E, nc] from [E, nc] and [E, nd]."""
        model, t = self.model, self.model.env
        E = t.env_count
        q = self._q64(joint_q)
        d = np.asarray(delta, dtype=np.float64).reshape(E, t.nd)
        out = q.copy()
        com = np.asarray(model.body_com, dtype=np.float64).reshape(E, t.nb, 3)
        X_c = np.asarray(model.joint_X_c, dtype=np.float64).reshape(E, t.nj, 7)
        for j in range(t.nj):
            jt, qs, ds = int(t.joint_type[j]), int(t.joint_q_start[j]), int(t.joint_qd_start[j])
            if jt in (JointType.PRISMATIC, JointType.REVOLUTE, JointType.D6):
                n = int(t.joint_lin_count[j] + t.joint_ang_count[j]) if jt == JointType.D6 else 1
                out[:, qs:qs + n] = q[:, qs:qs + n] + d[:, ds:ds + n]
            elif jt == JointType.BALL:
                out[:, qs:qs + 4] = _unit(_qmul(_exp_quat(d[:, ds:ds + 3]), q[:, qs:qs + 4]))
            elif jt in (JointType.FREE, JointType.DISTANCE):
                # the child pose in the parent anchor frame Y = X_j X_c^-1: its COM translates, it rotates about the COM; X_j' = Y' X_c
                c = com[:, int(t.joint_child[j])]
                Y = _xmul(q[:, qs:qs + 7], _xinv(X_c[:, j]))
                qy = _unit(_qmul(_exp_quat(d[:, ds + 3:ds + 6]), Y[:, 3:]))
                cy = Y[:, :3] + _qrot(Y[:, 3:], c) + d[:, ds:ds + 3]
                out[:, qs:qs + 7] = _xmul(np.concatenate([cy - _qrot(qy, c), qy], axis=1), X_c[:, j])
        return out

    # -----------------------------------------------------------------------------------------------------------------------------
    def step(self, joint_q_in, joint_q_out, iterations=10, step_size=1.0):
        """``iterations`` Levenberg-Marquardt iterations from ``joint_q_in`` into ``joint_q_out`` (Newton's flat order,
        [joint_coord_count] or [n_problems, nc]; they may be the same array).  GPU model: float32 tensors on the model's device, one
        kernel launch on the model's stream.  Host model: numpy arrays, float32 (float64 arrays are taken and filled unrounded)."""
        iterations = int(iterations)
        if iterations < 0:
            raise ValueError("iterations must be >= 0")
        if not float(step_size) > 0.0:
            raise ValueError("step_size must be positive")
        t = self.model.env
        n = t.env_count * t.nc
        if self._gpu:
            import torch  # noqa: PLC0415

            from . import _lib  # noqa: PLC0415

            for x, what in ((joint_q_in, "joint_q_in"), (joint_q_out, "joint_q_out")):
                if not (hasattr(x, "data_ptr") and x.dtype == torch.float32 and x.is_cuda and x.is_contiguous() and x.numel() == n):
                    raise ValueError(f"{what} must be a contiguous float32 tensor of {n} entries on the model's device")
            dm = self.model.device_model()
            st = dm.lib.nt_ik_solve(C.byref(dm.desc), C.byref(self._problem), joint_q_in.data_ptr(), joint_q_out.data_ptr(),
                                    self.lambdas.data_ptr(), self.costs.data_ptr(), iterations, float(step_size), dm.stream())
            if st == -3:  # NT_ERR_UNSUPPORTED
                raise NotImplementedError("IKSolver.step: nt_ik_solve answered NT_ERR_UNSUPPORTED (the tile of one world does not fit the "
                                          "LDS, or the library is a build without this kernel)")
            _lib.check(st, "nt_ik_solve")
            return
        for x, what in ((joint_q_in, "joint_q_in"), (joint_q_out, "joint_q_out")):
            if not isinstance(x, np.ndarray) or x.size != n or x.dtype not in (np.float32, np.float64):
                raise ValueError(f"{what} must be a float32 numpy array of {n} entries")
        q, lam, cost, _ = self._solve_numpy(self._q64(joint_q_in), self.lambdas.astype(np.float64), iterations, float(step_size))
        joint_q_out[...] = q.reshape(joint_q_out.shape)
        self.lambdas[...] = lam
        self.costs[...] = cost

    def _solve_numpy(self, q, lam, iterations, s, trace=None):
        """The iteration in float64.  ``trace`` (a list) receives one dict per iteration: delta, g, A (without lambda), lam (used), pred, rho,
        accept, cost (after the decision)."""
        nd = self.model.env.nd
        r, J = self.evaluate_numpy(q)
        cost = 0.5 * np.sum(r * r, axis=1)
        eye = np.eye(nd)
        for _ in range(iterations):
            JT = np.swapaxes(J, 1, 2)
            A0 = JT @ J
            g = (JT @ r[:, :, None])[:, :, 0]
            A = A0 + lam[:, None, None] * eye
            delta, ok = _cholesky_solve(A, -g)
            q2 = self.retract_numpy(q, s * delta)
            r2, J2 = self.evaluate_numpy(q2)
            cost2 = 0.5 * np.sum(r2 * r2, axis=1)
            pred = predicted_reduction(s, lam, np.sum(delta * delta, axis=1), np.sum(g * delta, axis=1))
            with np.errstate(divide="ignore", invalid="ignore"):
                rho = (cost - cost2) / pred
                accept = ok & (pred > 0.0) & (cost2 < cost) & (rho > self.rho_min)
            lam_used = lam
            q = np.where(accept[:, None], q2, q)
            r = np.where(accept[:, None], r2, r)
            J = np.where(accept[:, None, None], J2, J)
            cost = np.where(accept, cost2, cost)
            lam = np.where(accept, np.maximum(lam / self.lambda_factor, self.lambda_min), np.minimum(lam * self.lambda_factor, self.lambda_max))
            if trace is not None:
                trace.append(dict(delta=delta, g=g, A=A0, lam=lam_used, pred=pred, rho=rho, accept=accept, cost=cost.copy(), ok=ok))
        return q, lam, cost, r
