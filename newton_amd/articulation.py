"""eval_fk: joint coordinates -> maximal coordinates (newton/_src/sim/articulation.py:236-573), and eval_ik, its inverse.

Host implementations (numpy, vectorised over environments): eval_fk_numpy seeds ``body_q`` / ``body_qd`` before stepping, it is
model-preparation code, not part of the per-substep hot path; eval_ik_numpy is the host mirror of the device kernel behind
``eval_ik`` (nt_eval_ik, include/newton_hip_kinematics.h) and serves host models only.
"""
from __future__ import annotations

import numpy as np

from .enums import JointType


def _qmul(a, b):
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bx + bw * ax + ay * bz - by * az, aw * by + bw * ay + az * bx - bz * ax,
                     aw * bz + bw * az + ax * by - bx * ay, aw * bw - ax * bx - ay * by - az * bz], axis=-1)


def _qrot(q, v):
    qv, w = q[..., :3], q[..., 3:4]
    return v * (2.0 * w * w - 1.0) + np.cross(qv, v) * w * 2.0 + qv * np.sum(qv * v, axis=-1, keepdims=True) * 2.0


def _qinv(q):
    return q * np.array([-1.0, -1.0, -1.0, 1.0])


def _quat_axis_angle(axis, angle):
    h = 0.5 * np.asarray(angle)[..., None]
    return np.concatenate([axis * np.sin(h), np.cos(h)], axis=-1)


def _quat_from_cols(c0, c1, c2):
    """wp.quat_from_matrix(wp.matrix_from_cols(c0, c1, c2)) for a batch of (near-)orthonormal column triples."""
    m = np.stack([c0, c1, c2], axis=-1)  # [..., row, col]
    out = np.zeros(m.shape[:-2] + (4,))
    for idx in np.ndindex(m.shape[:-2]):
        a = m[idx]
        tr = a[0, 0] + a[1, 1] + a[2, 2]
        if tr >= 0.0:
            h = np.sqrt(tr + 1.0)
            w = 0.5 * h
            h = 0.5 / h
            x, y, z = (a[2, 1] - a[1, 2]) * h, (a[0, 2] - a[2, 0]) * h, (a[1, 0] - a[0, 1]) * h
        else:
            k = int(np.argmax(np.diag(a)))
            i, j = (k + 1) % 3, (k + 2) % 3
            h = np.sqrt((a[k, k] - (a[i, i] + a[j, j])) + 1.0)
            v = [0.0, 0.0, 0.0]
            v[k] = 0.5 * h
            h = 0.5 / h
            v[i] = (a[k, i] + a[i, k]) * h
            v[j] = (a[j, k] + a[k, j]) * h
            w = (a[j, i] - a[i, j]) * h
            x, y, z = v
        q = np.array([x, y, z, w])
        out[idx] = q / np.linalg.norm(q)
    return out


def _xmul(a, b):
    return np.concatenate([_qrot(a[..., 3:], b[..., :3]) + a[..., :3], _qmul(a[..., 3:], b[..., 3:])], axis=-1)


def _xinv(t):
    qi = _qinv(t[..., 3:])
    return np.concatenate([-_qrot(qi, t[..., :3]), qi], axis=-1)


def eval_fk_numpy(model, joint_q, joint_qd):
    """Returns (body_q [B,7], body_qd [B,6]) as float32 arrays."""
    if getattr(model, "is_heterogeneous", False):  # worlds differ: FK per world group, world-major concatenation (hetero.py)
        parts = model.world_groups.parts
        jq = np.split(np.asarray(joint_q, dtype=np.float32), np.cumsum([p.joint_coord_count for p in parts])[:-1])
        jqd = np.split(np.asarray(joint_qd, dtype=np.float32), np.cumsum([p.joint_dof_count for p in parts])[:-1])
        res = [eval_fk_numpy(p, a, b) for p, a, b in zip(parts, jq, jqd)]
        return np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res])
    body_q, body_qd = _eval_fk_float64(model, joint_q, joint_qd)
    return body_q.reshape(-1, 7).astype(np.float32), body_qd.reshape(-1, 6).astype(np.float32)


def _eval_fk_float64(model, joint_q, joint_qd):
    """eval_fk_numpy before the rounding: (body_q [E, nb, 7], body_qd [E, nb, 6]) in float64 (homogeneous models)."""
    t = model.env
    E, nb, nj = t.env_count, t.nb, t.nj
    jq = np.asarray(joint_q, dtype=np.float64).reshape(E, t.nc)
    jqd = np.asarray(joint_qd, dtype=np.float64).reshape(E, t.nd)
    body_q = np.asarray(model.body_q, dtype=np.float64).reshape(E, nb, 7).copy()
    body_qd = np.asarray(model.body_qd, dtype=np.float64).reshape(E, nb, 6).copy()
    com = np.asarray(model.body_com, dtype=np.float64).reshape(E, nb, 3)
    X_p = np.asarray(model.joint_X_p, dtype=np.float64).reshape(E, nj, 7)
    X_c = np.asarray(model.joint_X_c, dtype=np.float64).reshape(E, nj, 7)
    axis_all = np.asarray(model.joint_axis, dtype=np.float64).reshape(E, t.nd, 3)
    art = np.asarray(model.joint_articulation).reshape(E, nj)[0] if nj else []
    ident = np.tile(np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]), (E, 1))
    for j in range(nj):
        if art[j] == -1:
            continue
        jt = int(t.joint_type[j])
        parent, child = int(t.joint_parent[j]), int(t.joint_child[j])
        qs, qds = int(t.joint_q_start[j]), int(t.joint_qd_start[j])
        lin, ang = int(t.joint_lin_count[j]), int(t.joint_ang_count[j])
        X_j = ident.copy()
        v_lin = np.zeros((E, 3))
        v_ang = np.zeros((E, 3))
        if jt == JointType.PRISMATIC:
            ax = axis_all[:, qds]
            X_j[:, :3] = ax * jq[:, qs:qs + 1]
            v_lin = ax * jqd[:, qds:qds + 1]
        elif jt == JointType.REVOLUTE:
            ax = axis_all[:, qds]
            h = 0.5 * jq[:, qs:qs + 1]
            X_j[:, 3:6] = ax * np.sin(h)
            X_j[:, 6:7] = np.cos(h)
            v_ang = ax * jqd[:, qds:qds + 1]
        elif jt == JointType.BALL:
            X_j[:, 3:7] = jq[:, qs:qs + 4]
            v_ang = jqd[:, qds:qds + 3]
        elif jt in (JointType.FREE, JointType.DISTANCE):
            X_j = jq[:, qs:qs + 7].copy()
            v_lin = jqd[:, qds:qds + 3]
            v_ang = jqd[:, qds + 3:qds + 6]
        elif jt == JointType.D6:
            pos = np.zeros((E, 3))
            for k in range(lin):
                pos += axis_all[:, qds + k] * jq[:, qs + k:qs + k + 1]
                v_lin = v_lin + axis_all[:, qds + k] * jqd[:, qds + k:qds + k + 1]
            X_j[:, :3] = pos
            if ang == 1:
                ax = axis_all[:, qds + lin]
                h = 0.5 * jq[:, qs + lin:qs + lin + 1]
                X_j[:, 3:6] = ax * np.sin(h)
                X_j[:, 6:7] = np.cos(h)
                v_ang = ax * jqd[:, qds + lin:qds + lin + 1]
            elif ang == 2:  # compute_2d_rotational_dofs (articulation.py:36-83)
                ax0, ax1 = axis_all[:, qds + lin], axis_all[:, qds + lin + 1]
                q_off = _quat_from_cols(ax0, ax1, np.cross(ax0, ax1))
                a0 = _qrot(q_off, np.broadcast_to([1.0, 0.0, 0.0], (E, 3)))
                local_1 = _qrot(q_off, np.broadcast_to([0.0, 1.0, 0.0], (E, 3)))
                q_0 = _quat_axis_angle(a0, jq[:, qs + lin])
                a1 = _qrot(q_0, local_1)
                q_1 = _quat_axis_angle(a1, jq[:, qs + lin + 1])
                X_j[:, 3:7] = _qmul(q_1, q_0)
                v_ang = a0 * jqd[:, qds + lin:qds + lin + 1] + a1 * jqd[:, qds + lin + 1:qds + lin + 2]
            elif ang == 3:  # compute_3d_rotational_dofs (articulation.py:127-178)
                ax0, ax1, ax2 = (axis_all[:, qds + lin + k] for k in range(3))
                q_0 = _quat_axis_angle(ax0, jq[:, qs + lin])
                a1 = _qrot(q_0, ax1)
                q_1 = _quat_axis_angle(a1, jq[:, qs + lin + 1])
                q_10 = _qmul(q_1, q_0)
                a2 = _qrot(q_10, ax2)
                q_2 = _quat_axis_angle(a2, jq[:, qs + lin + 2])
                X_j[:, 3:7] = _qmul(q_2, q_10)
                v_ang = (ax0 * jqd[:, qds + lin:qds + lin + 1] + a1 * jqd[:, qds + lin + 1:qds + lin + 2]
                         + a2 * jqd[:, qds + lin + 2:qds + lin + 3])
        elif jt == JointType.FIXED:
            pass
        else:
            continue
        X_wpj = X_p[:, j]
        if parent >= 0:
            X_wp = body_q[:, parent]
            X_wpj = _xmul(X_wp, X_wpj)
        X_wcj = _xmul(X_wpj, X_j)
        X_wc = _xmul(X_wcj, _xinv(X_c[:, j]))
        x_child = X_wc[:, :3]
        v_parent = np.zeros((E, 3))
        w_parent = np.zeros((E, 3))
        if parent >= 0:
            qd_p = body_qd[:, parent]
            w_parent = qd_p[:, 3:]
            r = x_child - (X_wp[:, :3] + _qrot(X_wp[:, 3:], com[:, parent]))
            v_parent = np.cross(w_parent, r) + qd_p[:, :3]
        lin_w = _qrot(X_wpj[:, 3:], v_lin)
        ang_w = _qrot(X_wpj[:, 3:], v_ang)
        com_w = _qrot(X_wc[:, 3:], com[:, child])
        if jt in (JointType.FREE, JointType.DISTANCE):
            lin_origin = lin_w - np.cross(ang_w, com_w)
        else:
            lin_origin = lin_w + np.cross(ang_w, x_child - X_wcj[:, :3])
        v_o = v_parent + lin_origin
        w_o = w_parent + ang_w
        body_q[:, child] = X_wc
        body_qd[:, child, :3] = np.cross(w_o, com_w) + v_o
        body_qd[:, child, 3:] = w_o
    return body_q, body_qd


def _host_array(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _articulation_selection(model, mask, indices, what):
    """bool [articulation_count] from ``mask`` (bool per articulation) or ``indices`` (articulation ids); all when neither is given."""
    A = int(model.articulation_count)
    if mask is not None and indices is not None:
        raise ValueError(f"{what}: 'mask' and 'indices' cannot be used together")
    art_sel = np.ones(A, dtype=bool)
    if mask is not None:
        art_sel = np.asarray(mask.detach().cpu().numpy() if hasattr(mask, "detach") else mask).astype(bool).reshape(-1)
        if art_sel.shape[0] != A:
            raise ValueError(f"{what}: mask has {art_sel.shape[0]} entries, the model has {A} articulations")
    if indices is not None:
        idx = np.asarray(indices.detach().cpu().numpy() if hasattr(indices, "detach") else indices, dtype=np.int64).reshape(-1)
        art_sel = np.zeros(A, dtype=bool)
        art_sel[idx] = True
    return art_sel


def _fk_body_selection(model, mask, indices, body_flag_filter):
    """bool [body_count]: bodies whose inbound joint belongs to a selected articulation and whose flags pass the filter."""
    art_sel = _articulation_selection(model, mask, indices, "eval_fk")
    joint_art = np.asarray(model.joint_articulation)
    sel = np.zeros(model.body_count, dtype=bool)
    ok = joint_art >= 0
    sel[np.asarray(model.joint_child)[ok]] = art_sel[joint_art[ok]]
    if body_flag_filter is not None:
        sel &= (np.asarray(model.body_flags) & int(body_flag_filter)) != 0
    return sel


def eval_fk(model, joint_q, joint_qd, state, mask=None, indices=None, body_flag_filter=None):
    """newton.eval_fk(model, joint_q, joint_qd, state, mask=None, indices=None, body_flag_filter=BodyFlags.ALL)
    (newton/_src/sim/articulation.py:500-573): writes state.body_q / state.body_qd.  ``mask`` (bool per articulation) or
    ``indices`` (articulation ids) restrict the update to some articulations, ``body_flag_filter`` to bodies whose flags
    match (e.g. BodyFlags.KINEMATIC to re-pose only the prescribed bodies).  ``state`` may be a State or the Model itself (as
    in example_basic_urdf.py:88)."""
    if mask is not None or indices is not None or body_flag_filter is not None:
        sel = _fk_body_selection(model, mask, indices, body_flag_filter)
        if sel.all():
            return eval_fk(model, joint_q, joint_qd, state)
        from .state import State as _State  # noqa: PLC0415

        scratch = _State(model) if isinstance(state, _State) else None
        if scratch is not None and getattr(model, "is_gpu", False):
            # full FK into a scratch state (one kernel launch), then copy the selected bodies
            import torch  # noqa: PLC0415

            eval_fk(model, joint_q, joint_qd, scratch)
            rows = torch.as_tensor(np.flatnonzero(sel), device=scratch.body_q.device)
            for name in ("body_q", "body_qd"):
                cur, new = getattr(state, name), getattr(scratch, name)
                cur[rows] = new[rows]
                setattr(state, name, cur)
            return
        bq, bqd = eval_fk_numpy(model, _host_array(joint_q), _host_array(joint_qd))
        cur_q = np.array(_host_array(state.body_q), dtype=np.float32).reshape(-1, 7)
        cur_qd = np.array(_host_array(state.body_qd), dtype=np.float32).reshape(-1, 6)
        cur_q[sel], cur_qd[sel] = bq[sel], bqd[sel]
        state.body_q, state.body_qd = cur_q, cur_qd
        return

    def host(x):
        return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)

    from .state import State, pack_soa  # noqa: PLC0415

    t = model.env
    on_device = getattr(model, "is_gpu", False) and isinstance(state, State) and t.nj > 0
    if on_device and not np.any(np.asarray(model.joint_articulation) == -1):
        # device path: one launch of eval_fk_kernel through the C ABI (nt_eval_fk)
        import ctypes as C  # noqa: PLC0415

        from . import _lib  # noqa: PLC0415

        dm = model.device_model()
        jq = pack_soa(model, joint_q, 1, t.nc)
        jqd = pack_soa(model, joint_qd, 1, t.nd)
        d = state._desc()
        _lib.check(dm.lib.nt_eval_fk(C.byref(dm.desc), jq.data_ptr(), jqd.data_ptr(), C.byref(d), dm.stream()), "nt_eval_fk")
        return

    bq, bqd = eval_fk_numpy(model, host(joint_q), host(joint_qd))
    state.body_q = bq
    state.body_qd = bqd


# ---------------------------------------------------------------------------------------------------------------------------------
# eval_ik
# ---------------------------------------------------------------------------------------------------------------------------------
_D6_ORTHOGONAL_TOL = 1e-4


def check_ik_supported(model):
    """eval_ik recovers the angles of a D6 joint with two or three angular axes as Euler angles in the frame of those axes: they must be
    mutually orthogonal.  Raises NotImplementedError (the C ABI's NT_ERR_UNSUPPORTED) otherwise; checked once per model."""
    if getattr(model, "_ik_checked", False):
        return
    jt = np.asarray(model.joint_type)
    dd = np.asarray(model.joint_dof_dim).reshape(-1, 2)
    axis = np.asarray(model.joint_axis, dtype=np.float64).reshape(-1, 3)
    qds = np.asarray(model.joint_qd_start)
    for j in np.flatnonzero((jt == int(JointType.D6)) & (dd[:, 1] >= 2)):
        a = axis[qds[j] + dd[j, 0]:qds[j] + dd[j, 0] + dd[j, 1]]
        g = a @ a.T
        if np.abs(g - np.diag(np.diag(g))).max() > _D6_ORTHOGONAL_TOL:
            raise NotImplementedError(f"eval_ik: joint {j} is a D6 joint with {dd[j, 1]} angular axes that are not mutually orthogonal "
                                      "(unsupported)")
    model._ik_checked = True


def _wrap_pi(a):
    a = np.where(a > np.pi, a - 2.0 * np.pi, a)
    return np.where(a <= -np.pi, a + 2.0 * np.pi, a)


def _twist_angle(axis, q):
    return _wrap_pi(2.0 * np.arctan2(np.sum(axis * q[..., :3], axis=-1), q[..., 3]))


def _d6_angles(ang, e, q_j):
    """Intrinsic Euler angles of q_j in the frame whose columns are the axes e[0..ang-1] (mutually orthogonal)."""
    e2 = e[2] if ang == 3 else np.cross(e[0], e[1])
    r0, r1, r2 = _qrot(q_j, e[0]), _qrot(q_j, e[1]), _qrot(q_j, e2)

    def d(a, b):
        return np.sum(a * b, axis=-1)

    if ang == 2:
        return [np.arctan2(d(e2, r1), d(e[1], r1)), np.arctan2(d(e[0], r2), d(e[0], r0))]
    s = np.where(d(np.cross(e[0], e[1]), e2) < 0.0, -1.0, 1.0)
    m00, m01, m02 = d(e[0], r0), d(e[0], r1), d(e[0], r2)
    return [s * np.arctan2(-d(e[1], r2), d(e2, r2)), s * np.arctan2(m02, np.sqrt(m00 * m00 + m01 * m01)), s * np.arctan2(-m01, m00)]


def eval_ik_numpy(model, body_q, body_qd, joint_q=None, joint_qd=None, art_sel=None):
    """Host mirror of eval_ik_kernel: returns (joint_q, joint_qd) as float32 arrays in Newton's flat order.  ``joint_q`` / ``joint_qd``
    (default: the model's) supply the entries that stay untouched: FIXED joints have none, and with ``art_sel`` (bool per articulation)
    the joints of unselected articulations and joints outside any articulation keep theirs."""
    if getattr(model, "is_heterogeneous", False):  # per world group, world-major concatenation (hetero.py)
        parts = model.world_groups.parts
        cut = lambda a, key: np.split(np.asarray(a, dtype=np.float32), np.cumsum([getattr(p, key) for p in parts])[:-1])  # noqa: E731
        bq, bqd = cut(np.asarray(body_q).reshape(-1, 7), "body_count"), cut(np.asarray(body_qd).reshape(-1, 6), "body_count")
        jq = cut(model.joint_q if joint_q is None else joint_q, "joint_coord_count")
        jqd = cut(model.joint_qd if joint_qd is None else joint_qd, "joint_dof_count")
        sel = [None] * len(parts) if art_sel is None else np.split(np.asarray(art_sel, dtype=bool),
                                                                  np.cumsum([p.articulation_count for p in parts])[:-1])
        res = [eval_ik_numpy(p, *args) for p, *args in zip(parts, bq, bqd, jq, jqd, sel)]
        return np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res])
    check_ik_supported(model)
    t = model.env
    E, nb, nj = t.env_count, t.nb, t.nj
    bq = np.asarray(body_q, dtype=np.float64).reshape(E, nb, 7)
    bqd = np.asarray(body_qd, dtype=np.float64).reshape(E, nb, 6)
    out_q = np.array(model.joint_q if joint_q is None else joint_q, dtype=np.float32).reshape(E, t.nc)
    out_qd = np.array(model.joint_qd if joint_qd is None else joint_qd, dtype=np.float32).reshape(E, t.nd)
    com = np.asarray(model.body_com, dtype=np.float64).reshape(E, nb, 3)
    X_p = np.asarray(model.joint_X_p, dtype=np.float64).reshape(E, nj, 7)
    X_c = np.asarray(model.joint_X_c, dtype=np.float64).reshape(E, nj, 7)
    axis_all = np.asarray(model.joint_axis, dtype=np.float64).reshape(E, t.nd, 3)
    art = np.asarray(model.joint_articulation).reshape(E, nj) if nj else np.zeros((E, 0), dtype=np.int64)
    handled = (JointType.PRISMATIC, JointType.REVOLUTE, JointType.BALL, JointType.FREE, JointType.DISTANCE, JointType.D6)
    for j in range(nj):
        jt = int(t.joint_type[j])
        if jt not in [int(h) for h in handled]:
            continue
        rows = np.ones(E, dtype=bool)
        if art_sel is not None:
            rows = (art[:, j] >= 0) & np.asarray(art_sel, dtype=bool)[np.maximum(art[:, j], 0)]
            if not rows.any():
                continue
        parent, child = int(t.joint_parent[j]), int(t.joint_child[j])
        qs, qds = int(t.joint_q_start[j]), int(t.joint_qd_start[j])
        lin, ang = int(t.joint_lin_count[j]), int(t.joint_ang_count[j])
        X_wpj = X_p[:, j]
        if parent >= 0:
            X_wp = bq[:, parent]
            X_wpj = _xmul(X_wp, X_wpj)
        X_wc = bq[:, child]
        X_wcj = _xmul(X_wc, X_c[:, j])
        q_pinv = _qinv(X_wpj[:, 3:])
        x_j = _qrot(q_pinv, X_wcj[:, :3] - X_wpj[:, :3])
        q_j = _qmul(q_pinv, X_wcj[:, 3:])
        w_o = bqd[:, child, 3:]
        com_w = _qrot(X_wc[:, 3:], com[:, child])
        v_o = bqd[:, child, :3] - np.cross(w_o, com_w)
        w_parent = np.zeros((E, 3))
        v_parent = np.zeros((E, 3))
        if parent >= 0:
            w_parent = bqd[:, parent, 3:]
            v_parent = np.cross(w_parent, X_wc[:, :3] - (X_wp[:, :3] + _qrot(X_wp[:, 3:], com[:, parent]))) + bqd[:, parent, :3]
        ang_w, lin_origin = w_o - w_parent, v_o - v_parent
        if jt in (JointType.FREE, JointType.DISTANCE):
            lin_w = lin_origin + np.cross(ang_w, com_w)
        else:
            lin_w = lin_origin - np.cross(ang_w, X_wc[:, :3] - X_wcj[:, :3])
        v_lin, v_ang = _qrot(q_pinv, lin_w), _qrot(q_pinv, ang_w)

        def dot(a, b):
            return np.sum(a * b, axis=-1)

        q_new, qd_new = [], []
        if jt == JointType.PRISMATIC:
            q_new, qd_new = [dot(axis_all[:, qds], x_j)], [dot(axis_all[:, qds], v_lin)]
        elif jt == JointType.REVOLUTE:
            q_new, qd_new = [_twist_angle(axis_all[:, qds], q_j)], [dot(axis_all[:, qds], v_ang)]
        elif jt == JointType.BALL:
            q_new, qd_new = list(q_j.T), list(v_ang.T)
        elif jt in (JointType.FREE, JointType.DISTANCE):
            q_new, qd_new = list(x_j.T) + list(q_j.T), list(v_lin.T) + list(v_ang.T)
        else:  # D6
            for k in range(lin):
                q_new.append(dot(axis_all[:, qds + k], x_j))
                qd_new.append(dot(axis_all[:, qds + k], v_lin))
            e = [axis_all[:, qds + lin + k] for k in range(ang)]
            if ang == 1:
                q_new.append(_twist_angle(e[0], q_j))
                qd_new.append(dot(e[0], v_ang))
            elif ang >= 2:
                th = _d6_angles(ang, e, q_j)
                # eval_fk's transported axes at the recovered angles; v_ang = sum a_k qd_k (Cramer)
                a0 = e[0]
                a1 = _qrot(_quat_axis_angle(a0, th[0]), e[1])
                q_new += th
                if ang == 2:
                    g00, g01, g11, b0, b1 = dot(a0, a0), dot(a0, a1), dot(a1, a1), dot(a0, v_ang), dot(a1, v_ang)
                    det = g00 * g11 - g01 * g01
                    qd_new += [(b0 * g11 - b1 * g01) / det, (g00 * b1 - g01 * b0) / det]
                else:
                    q_10 = _qmul(_quat_axis_angle(a1, th[1]), _quat_axis_angle(a0, th[0]))
                    a2 = _qrot(q_10, e[2])
                    a12 = np.cross(a1, a2)
                    det = dot(a0, a12)
                    qd_new += [dot(v_ang, a12) / det, dot(a0, np.cross(v_ang, a2)) / det, dot(a0, np.cross(a1, v_ang)) / det]
        for k, v in enumerate(q_new):
            out_q[rows, qs + k] = v[rows]
        for k, v in enumerate(qd_new):
            out_qd[rows, qds + k] = v[rows]
    return out_q.reshape(-1), out_qd.reshape(-1)


def _fill(dst, values):
    """Write ``values`` (flat, Newton order) into the caller's tensor / array in place."""
    if hasattr(dst, "copy_"):
        dst.copy_(values.reshape(dst.shape) if hasattr(values, "device") else dst.new_tensor(np.asarray(values)).reshape(dst.shape))
    else:
        dst[...] = (values.detach().cpu().numpy() if hasattr(values, "detach") else np.asarray(values)).reshape(dst.shape)


def _eval_ik_device(model, state, joint_q, joint_qd, art_mask):
    """One launch of eval_ik_kernel on the model's stream.  art_mask: uint8 device tensor [env_count * na] or None."""
    import ctypes as C  # noqa: PLC0415

    from . import _lib  # noqa: PLC0415
    from .state import pack_soa  # noqa: PLC0415

    t = model.env
    dm = model.device_model()
    d = state._desc()
    # the state's own SoA buffers (no copy), or SoA twins of the caller's arrays (they supply the entries that stay untouched)
    soa_q = state._soa["joint_q"] if joint_q is None else pack_soa(model, joint_q, 1, t.nc)
    soa_qd = state._soa["joint_qd"] if joint_qd is None else pack_soa(model, joint_qd, 1, t.nd)
    _lib.check(dm.lib.nt_eval_ik(C.byref(dm.desc), C.byref(d), soa_q.data_ptr(), soa_qd.data_ptr(),
                                 None if art_mask is None else art_mask.data_ptr(), dm.stream()), "nt_eval_ik")
    for dst, soa, n in ((joint_q, soa_q, t.nc), (joint_qd, soa_qd, t.nd)):
        if dst is None or n == 0:
            continue
        import torch  # noqa: PLC0415

        flat = torch.empty(t.env_count * n, dtype=torch.float32, device=dm.device)
        _lib.check(dm.lib.nt_unpack_aos(soa.data_ptr(), flat.data_ptr(), 1, n, t.env_count, t.env_stride, dm.stream()), "nt_unpack_aos")
        _fill(dst, flat)


def eval_ik(model, state, joint_q=None, joint_qd=None, mask=None, indices=None):
    """newton.eval_ik(model, state, joint_q, joint_qd, mask=None, indices=None) (newton/_src/sim/articulation.py): joint coordinates and
    velocities from ``state.body_q`` / ``state.body_qd`` -- the inverse of :func:`eval_fk`.  The maximal-coordinate solvers (SolverXPBD,
    SolverSemiImplicit) never touch ``state.joint_q`` / ``state.joint_qd``: step, call ``eval_ik``, then read them (or an
    ``ArticulationView``).

    With ``joint_q`` / ``joint_qd`` left ``None`` the state's own arrays are written in place: on a GPU model, without ``mask`` /
    ``indices``, that is one kernel launch on the model's stream, no copy, no allocation, no synchronisation -- it records into
    ``newton_amd.graph.capture``.  Only that path is: a selection uploads its byte mask on every call (one allocation and one
    host-to-device copy; ``nt_eval_ik`` itself takes a resident mask and stays capturable), given tensors / arrays are filled in
    Newton's flat order through staging buffers.  Every joint of the model is evaluated, inside an articulation or not; ``mask`` (bool per articulation) or
    ``indices`` (articulation ids) restrict the update: the joints of unselected articulations and joints outside any articulation
    are left untouched.  FIXED joints have no coordinates.  A D6 joint with two or three angular axes needs them mutually orthogonal
    (the angles are Euler angles in the frame of the axes); any other is refused as unsupported (NotImplementedError).  Joints that the
    solver left slightly violated are projected onto their coordinates."""
    art_sel = None
    if mask is not None or indices is not None:
        art_sel = _articulation_selection(model, mask, indices, "eval_ik")
        if art_sel.all() and not np.any(np.asarray(model.joint_articulation) == -1):
            art_sel = None
    if getattr(model, "is_heterogeneous", False):
        return _eval_ik_groups(model, state, joint_q, joint_qd, art_sel)
    check_ik_supported(model)
    t = model.env
    if getattr(model, "is_gpu", False):
        from .state import State  # noqa: PLC0415

        if not isinstance(state, State):
            raise TypeError("eval_ik: a GPU model needs a State (the body state is read on the device)")
        if t.nj == 0:
            return
        if art_sel is not None and t.na == 0:
            raise NotImplementedError("eval_ik: mask / indices need articulations that cover every world's joints in order")
        _eval_ik_device(model, state, joint_q, joint_qd, _device_art_mask(model, art_sel, "eval_ik"))
        return
    jq, jqd = eval_ik_numpy(model, _host_array(state.body_q), _host_array(state.body_qd),
                            _host_array(state.joint_q if joint_q is None else joint_q),
                            _host_array(state.joint_qd if joint_qd is None else joint_qd), art_sel)
    if joint_q is None:
        state.joint_q = jq
    else:
        _fill(joint_q, jq)
    if joint_qd is None:
        state.joint_qd = jqd
    else:
        _fill(joint_qd, jqd)


def _eval_ik_groups(model, state, joint_q, joint_qd, art_sel):
    """Heterogeneous model: one eval_ik per world group into the parts of the GroupedState, the groups on their sibling streams."""
    groups = model.world_groups
    parts = groups.parts

    def cut(value, key):
        if value is None:
            return [None] * len(parts)
        sizes = [getattr(p, key) for p in parts]
        if hasattr(value, "split") and hasattr(value, "device"):
            return list(value.reshape(-1).split(sizes))
        return np.split(np.asarray(value).reshape(-1), np.cumsum(sizes)[:-1])  # (views: filled in place)

    if joint_q is not None and not hasattr(joint_q, "device") and not isinstance(joint_q, np.ndarray):
        raise TypeError("eval_ik: joint_q must be a tensor or a numpy array")
    if joint_qd is not None and not hasattr(joint_qd, "device") and not isinstance(joint_qd, np.ndarray):
        raise TypeError("eval_ik: joint_qd must be a tensor or a numpy array")
    qs, qds = cut(joint_q, "joint_coord_count"), cut(joint_qd, "joint_dof_count")
    sels = [None] * len(parts) if art_sel is None else np.split(art_sel, np.cumsum([p.articulation_count for p in parts])[:-1])

    def go(i, p):
        eval_ik(p, state.parts[i], qs[i], qds[i], mask=sels[i])

    if getattr(model, "is_gpu", False):
        groups.run(go)
    else:
        for i, p in enumerate(parts):
            go(i, p)


# ---------------------------------------------------------------------------------------------------------------------------------
# eval_jacobian / eval_mass_matrix
# ---------------------------------------------------------------------------------------------------------------------------------
def _articulated(model, what):
    t = model.env
    if t.nj == 0 or t.na == 0:
        raise NotImplementedError(f"{what}: needs articulations that cover every world's joints in order (unsupported)")
    return t


def _joint_ancestors(t):
    """Per env-local joint: the joint of the same articulation whose child is its parent body (-1: none)."""
    art = np.searchsorted(t.art_start[1:], np.arange(t.nj), side="right")
    anc = -np.ones(t.nj, dtype=np.int64)
    for j in range(t.nj):
        p = int(t.joint_parent[j])
        if p >= 0:
            for k in range(int(t.art_start[art[j]]), int(t.art_start[art[j] + 1])):
                if int(t.joint_child[k]) == p:
                    anc[j] = k
    return art, anc


def _path_matrix(t):
    """bool [nj, nj]: entry (l, a) -- joint a is joint l or on its joint_parent chain inside the articulation."""
    _, anc = _joint_ancestors(t)
    on = np.zeros((t.nj, t.nj), dtype=bool)
    for j in range(t.nj):
        k, n = j, 0
        while k >= 0 and n <= t.nj:
            on[j, k] = True
            k, n = anc[k], n + 1
    return on


def _motion_subspace_numpy(model, body_q, joint_q):
    """S [E, nd, 6] in float64: the column of every dof as an origin-referenced world twist (linear, angular) -- the closed forms of
    include/newton_hip_kinematics.h."""
    t = model.env
    E, nb, nj = t.env_count, t.nb, t.nj
    bq = np.asarray(body_q, dtype=np.float64).reshape(E, nb, 7)
    jq = np.asarray(joint_q, dtype=np.float64).reshape(E, t.nc)
    com = np.asarray(model.body_com, dtype=np.float64).reshape(E, nb, 3)
    X_p = np.asarray(model.joint_X_p, dtype=np.float64).reshape(E, nj, 7)
    axis_all = np.asarray(model.joint_axis, dtype=np.float64).reshape(E, t.nd, 3)
    S = np.zeros((E, t.nd, 6))
    eye = np.eye(3)
    for j in range(nj):
        jt = int(t.joint_type[j])
        parent, child = int(t.joint_parent[j]), int(t.joint_child[j])
        qs, ds = int(t.joint_q_start[j]), int(t.joint_qd_start[j])
        lin, ang = int(t.joint_lin_count[j]), int(t.joint_ang_count[j])
        X_wpj = X_p[:, j]
        if parent >= 0:
            X_wpj = _xmul(bq[:, parent], X_wpj)
        p, qR = X_wpj[:, :3], X_wpj[:, 3:]

        def linear(d, a):
            S[:, d, :3] = _qrot(qR, a)

        def angular(d, a, pivot):
            w = _qrot(qR, a)
            S[:, d, :3], S[:, d, 3:] = np.cross(pivot, w), w

        unit = lambda k: np.broadcast_to(eye[k], (E, 3))  # noqa: E731
        if jt == JointType.PRISMATIC:
            linear(ds, axis_all[:, ds])
        elif jt == JointType.REVOLUTE:
            angular(ds, axis_all[:, ds], p)
        elif jt == JointType.BALL:
            for k in range(3):
                angular(ds + k, unit(k), p)
        elif jt in (JointType.FREE, JointType.DISTANCE):
            c_child = bq[:, child, :3] + _qrot(bq[:, child, 3:], com[:, child])
            for k in range(3):
                linear(ds + k, unit(k))
                angular(ds + 3 + k, unit(k), c_child)
        elif jt == JointType.D6:
            pos = np.zeros((E, 3))
            for k in range(lin):
                linear(ds + k, axis_all[:, ds + k])
                pos += axis_all[:, ds + k] * jq[:, qs + k:qs + k + 1]
            p_j = p + _qrot(qR, pos)
            e = [axis_all[:, ds + lin + k] for k in range(ang)]
            if ang == 1:
                a = [e[0]]
            elif ang == 2:  # compute_2d_rotational_dofs, as eval_fk_numpy
                q_off = _quat_from_cols(e[0], e[1], np.cross(e[0], e[1]))
                a0 = _qrot(q_off, unit(0))
                a = [a0, _qrot(_quat_axis_angle(a0, jq[:, qs + lin]), _qrot(q_off, unit(1)))]
            elif ang == 3:
                q_0 = _quat_axis_angle(e[0], jq[:, qs + lin])
                a1 = _qrot(q_0, e[1])
                a = [e[0], a1, _qrot(_qmul(_quat_axis_angle(a1, jq[:, qs + lin + 1]), q_0), e[2])]
            else:
                a = []
            for k in range(ang):
                angular(ds + lin + k, a[k], p_j)
    return S


def _spatial_inertia_numpy(model, body_q):
    """[E, nb, 6, 6] in float64: each body's world-frame spatial inertia about the origin, (linear, angular) ordering."""
    t = model.env
    E, nb = t.env_count, t.nb
    bq = np.asarray(body_q, dtype=np.float64).reshape(E, nb, 7)
    com = np.asarray(model.body_com, dtype=np.float64).reshape(E, nb, 3)
    mass = np.asarray(model.body_mass, dtype=np.float64).reshape(E, nb)
    Ib = np.asarray(model.body_inertia, dtype=np.float64).reshape(E, nb, 3, 3)
    q = bq.reshape(-1, 7)[:, 3:]
    R = np.stack([_qrot(q, np.broadcast_to(np.eye(3)[k], (E * nb, 3))) for k in range(3)], axis=-1).reshape(E, nb, 3, 3)
    c = bq[:, :, :3] + _qrot(q, com.reshape(-1, 3)).reshape(E, nb, 3)
    cx = np.zeros((E, nb, 3, 3))
    cx[..., 0, 1], cx[..., 0, 2], cx[..., 1, 0] = -c[..., 2], c[..., 1], c[..., 2]
    cx[..., 1, 2], cx[..., 2, 0], cx[..., 2, 1] = -c[..., 0], -c[..., 1], c[..., 0]
    m = mass[..., None, None]
    out = np.zeros((E, nb, 6, 6))
    out[..., :3, :3] = m * np.eye(3)
    out[..., :3, 3:] = -m * cx
    out[..., 3:, :3] = m * cx
    out[..., 3:, 3:] = R @ Ib @ np.swapaxes(R, -1, -2) - m * (cx @ cx)
    return out


def _art_dims(model):
    return int(model.max_joints_per_articulation), int(model.max_dofs_per_articulation)


def _art_ranges(t):
    """Per env-local articulation: (first joint, joint count, first dof, dof count)."""
    dof_edges = np.concatenate([t.joint_qd_start, [t.nd]])
    return [(int(t.art_start[k]), int(t.art_start[k + 1] - t.art_start[k]), int(dof_edges[t.art_start[k]]),
             int(dof_edges[t.art_start[k + 1]] - dof_edges[t.art_start[k]])) for k in range(t.na)]


def _new_or_checked(out, shape, what):
    if out is None:
        return np.zeros(shape, dtype=np.float32)
    if not isinstance(out, np.ndarray) or out.dtype != np.float32 or tuple(out.shape) != tuple(shape):
        raise ValueError(f"{what} must be a float32 numpy array of shape {tuple(shape)}")
    return out


def eval_jacobian_numpy(model, body_q, joint_q, J=None, joint_S_s=None, art_sel=None):
    """Host mirror of eval_jacobian_kernel (float64 inside, float32 out): fills and returns J [articulation_count, 6 L, D]; the slices
    of articulations ``art_sel`` (bool per articulation) leaves out stay untouched, in ``joint_S_s`` [joint_dof_count, 6] too."""
    L, D = _art_dims(model)
    J = _new_or_checked(J, (int(model.articulation_count), 6 * L, D), "J")
    if joint_S_s is not None:
        joint_S_s = _new_or_checked(joint_S_s, (int(model.joint_dof_count), 6), "joint_S_s")
    if getattr(model, "is_heterogeneous", False):
        parts = model.world_groups.parts
        bqs = np.split(np.asarray(body_q).reshape(-1, 7), np.cumsum([p.body_count for p in parts])[:-1])
        jqs = np.split(np.asarray(joint_q).reshape(-1), np.cumsum([p.joint_coord_count for p in parts])[:-1])
        a0 = d0 = 0
        for p, bq, jq in zip(parts, bqs, jqs):
            a1, d1 = a0 + p.articulation_count, d0 + p.joint_dof_count
            if p.articulation_count:
                sel = None if art_sel is None else np.asarray(art_sel, dtype=bool)[a0:a1]
                Lp, Dp = _art_dims(p)
                Jp = np.array(J[a0:a1, :6 * Lp, :Dp])  # (a copy: the slice is cleared below)
                eval_jacobian_numpy(p, bq, jq, Jp, None if joint_S_s is None else joint_S_s[d0:d1], sel)
                rows = slice(a0, a1) if sel is None else a0 + np.flatnonzero(sel)
                J[rows] = 0.0
                J[rows, :6 * Lp, :Dp] = Jp if sel is None else Jp[sel]
            a0, d0 = a1, d1
        return J
    t = _articulated(model, "eval_jacobian")
    E = t.env_count
    S = _motion_subspace_numpy(model, body_q, joint_q)
    on = _path_matrix(t)
    dof_joint = np.searchsorted(t.joint_qd_start, np.arange(t.nd), side="right") - 1 if t.nd else np.zeros(0, dtype=np.int64)
    sel = np.ones((E, t.na), dtype=bool) if art_sel is None else np.asarray(art_sel, dtype=bool).reshape(E, t.na)
    Jv = J.reshape(E, t.na, 6 * L, D)
    for k, (j0, nja, d0, nda) in enumerate(_art_ranges(t)):
        blk = np.zeros((E, 6 * L, D))
        for i in range(nja):
            cols = on[j0 + i, dof_joint[d0:d0 + nda]]
            blk[:, 6 * i:6 * i + 6, :nda] = np.swapaxes(S[:, d0:d0 + nda], 1, 2) * cols
        Jv[sel[:, k], k] = blk[sel[:, k]].astype(np.float32)
        if joint_S_s is not None:
            joint_S_s.reshape(E, t.nd, 6)[sel[:, k], d0:d0 + nda] = S[sel[:, k], d0:d0 + nda].astype(np.float32)
    return J


def eval_mass_matrix_numpy(model, body_q, joint_q, H=None, body_I_s=None, art_sel=None):
    """Host mirror of eval_mass_matrix_kernel: H [articulation_count, D, D] = sum over links of J_l^T I_l J_l, in float64 from the
    definition (the kernel composes inertias along the tree), float32 out; ``body_I_s`` [body_count, 6, 6] optional."""
    L, D = _art_dims(model)
    H = _new_or_checked(H, (int(model.articulation_count), D, D), "H")
    if body_I_s is not None:
        body_I_s = _new_or_checked(body_I_s, (int(model.body_count), 6, 6), "body_I_s")
    if getattr(model, "is_heterogeneous", False):
        parts = model.world_groups.parts
        bqs = np.split(np.asarray(body_q).reshape(-1, 7), np.cumsum([p.body_count for p in parts])[:-1])
        jqs = np.split(np.asarray(joint_q).reshape(-1), np.cumsum([p.joint_coord_count for p in parts])[:-1])
        a0 = b0 = 0
        for p, bq, jq in zip(parts, bqs, jqs):
            a1, b1 = a0 + p.articulation_count, b0 + p.body_count
            if p.articulation_count:
                sel = None if art_sel is None else np.asarray(art_sel, dtype=bool)[a0:a1]
                Dp = _art_dims(p)[1]
                Hp = np.array(H[a0:a1, :Dp, :Dp])
                eval_mass_matrix_numpy(p, bq, jq, Hp, None if body_I_s is None else body_I_s[b0:b1], sel)
                rows = slice(a0, a1) if sel is None else a0 + np.flatnonzero(sel)
                H[rows] = 0.0
                H[rows, :Dp, :Dp] = Hp if sel is None else Hp[sel]
            a0, b0 = a1, b1
        return H
    t = _articulated(model, "eval_mass_matrix")
    E = t.env_count
    blocks, I_s = _mass_matrix_float64(model, body_q, joint_q)
    sel = np.ones((E, t.na), dtype=bool) if art_sel is None else np.asarray(art_sel, dtype=bool).reshape(E, t.na)
    Hv = H.reshape(E, t.na, D, D)
    for k, (j0, nja, _d0, _nda) in enumerate(_art_ranges(t)):
        if body_I_s is not None:
            for i in range(nja):
                b = int(t.joint_child[j0 + i])
                body_I_s.reshape(E, t.nb, 6, 6)[sel[:, k], b] = I_s[sel[:, k], b].astype(np.float32)
        Hv[sel[:, k], k] = blocks[sel[:, k], k].astype(np.float32)
    return H


def _mass_matrix_float64(model, body_q, joint_q):
    """(H [E, na, D, D], the links' spatial inertias [E, nb, 6, 6]) in float64, before any rounding (homogeneous model)."""
    t = model.env
    E, D = t.env_count, _art_dims(model)[1]
    S = _motion_subspace_numpy(model, body_q, joint_q)
    I_s = _spatial_inertia_numpy(model, body_q)
    on = _path_matrix(t)
    dof_joint = np.searchsorted(t.joint_qd_start, np.arange(t.nd), side="right") - 1 if t.nd else np.zeros(0, dtype=np.int64)
    out = np.zeros((E, t.na, D, D))
    for k, (j0, nja, d0, nda) in enumerate(_art_ranges(t)):
        blk = np.zeros((E, D, D))
        for i in range(nja):
            Jl = np.swapaxes(S[:, d0:d0 + nda], 1, 2) * on[j0 + i, dof_joint[d0:d0 + nda]]  # [E, 6, nda]
            blk[:, :nda, :nda] += np.swapaxes(Jl, 1, 2) @ I_s[:, int(t.joint_child[j0 + i])] @ Jl
        out[:, k] = 0.5 * (blk + np.swapaxes(blk, 1, 2))  # (symmetric bit for bit, like the kernel's one value per pair)
    return out, I_s


def _device_art_mask(model, art_sel, what):
    if art_sel is None:
        return None
    import torch  # noqa: PLC0415

    t = model.env
    if t.na * t.env_count != art_sel.shape[0]:
        raise NotImplementedError(f"{what}: mask needs articulations that cover every world's joints in order")
    return torch.from_numpy(art_sel.astype(np.uint8)).to(model.device_model().device)


def _device_out(model, out, shape, what):
    """The caller's float32 device tensor (checked), or a new one."""
    import torch  # noqa: PLC0415

    dev = model.device_model().device
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=dev)
    if not (hasattr(out, "data_ptr") and out.dtype == torch.float32 and out.is_cuda and out.is_contiguous()
            and tuple(out.shape) == tuple(shape)):
        raise ValueError(f"{what} must be a contiguous float32 tensor of shape {tuple(shape)} on the model's device")
    return out


def _mask_selection(model, mask, what):
    art_sel = None
    if mask is not None:
        art_sel = _articulation_selection(model, mask, None, what)
        if art_sel.all():
            art_sel = None
    return art_sel


def _eval_jm_device(model, state, what, out, out_name, shape, aux, aux_name, aux_shape, art_sel):
    """Device path of eval_jacobian / eval_mass_matrix (``what``): one launch of nt_<what> on the model's stream into ``out`` (the
    caller's, checked, or a new tensor: zeroed first where a mask leaves slices unwritten) and the optional ``aux``.  Returns ``out``."""
    import ctypes as C  # noqa: PLC0415

    from . import _lib  # noqa: PLC0415

    _articulated(model, what)
    dm = model.device_model()
    fresh = out is None
    out = _device_out(model, out, shape, out_name)
    if aux is not None:
        aux = _device_out(model, aux, aux_shape, aux_name)
    if fresh and art_sel is not None:
        out.zero_()
    art_mask = _device_art_mask(model, art_sel, what)
    d = state._desc()
    _lib.check(getattr(dm.lib, "nt_" + what)(C.byref(dm.desc), C.byref(d), out.data_ptr(), None if aux is None else aux.data_ptr(),
                                             None if art_mask is None else art_mask.data_ptr(), dm.stream()), "nt_" + what)
    return out


def eval_jacobian(model, state, J=None, joint_S_s=None, mask=None):
    """newton.eval_jacobian(model, state, J=None, joint_S_s=None, mask=None) (newton/_src/sim/articulation.py): the articulation
    Jacobian ``J`` [articulation_count, 6 L, D] float32, L = ``model.max_joints_per_articulation``, D =
    ``model.max_dofs_per_articulation``.  Row block i of articulation a is the child body of its joint i, an origin-referenced world
    twist (linear first); column k is its dof k, with respect to the public ``joint_qd`` (a FREE / DISTANCE joint carries the COM
    velocity).  With ``(v, w) = J[a, 6 i:6 i + 6] @ joint_qd[dofs of a]`` the body velocity :func:`eval_fk` produces is
    ``(v + w x c, w)``, c the link's world COM.  Padding and the entries of dofs off a link's root path are written as zero on every
    call.  ``joint_S_s`` [joint_dof_count, 6] (optional) receives the column of each dof; ``mask`` (bool per articulation) leaves the
    slices of unselected articulations untouched.

    Reads ``state.body_q`` (parent poses, COMs) and ``state.joint_q`` (the joint's own displacement) -- eval_fk's composition: after a
    maximal-coordinate step (SolverXPBD, SolverSemiImplicit) call :func:`eval_ik` first.  Outputs left ``None`` are allocated and
    returned: torch tensors on a GPU model, numpy arrays on a host model.  On a GPU model with ``J`` (and ``joint_S_s``, if wanted)
    supplied and no ``mask`` the call is one kernel launch on the model's stream (nt_eval_jacobian): no allocation, no
    synchronisation, it records into ``newton_amd.graph.capture``.  A mask uploads its bytes on every call."""
    art_sel = _mask_selection(model, mask, "eval_jacobian")
    if getattr(model, "is_heterogeneous", False):
        return _eval_jm_groups(model, state, "jacobian", J, joint_S_s, art_sel)
    L, D = _art_dims(model)
    if not getattr(model, "is_gpu", False):
        return eval_jacobian_numpy(model, _host_array(state.body_q), _host_array(state.joint_q), J, joint_S_s, art_sel)
    t = model.env
    return _eval_jm_device(model, state, "eval_jacobian", J, "J", (t.env_count * t.na, 6 * L, D),
                           joint_S_s, "joint_S_s", (t.env_count * t.nd, 6), art_sel)


def eval_mass_matrix(model, state, H=None, J=None, body_I_s=None, joint_S_s=None, mask=None):
    """newton.eval_mass_matrix(model, state, H=None, J=None, body_I_s=None, joint_S_s=None, mask=None)
    (newton/_src/sim/articulation.py): the joint-space inertia ``H`` [articulation_count, D, D] float32, ``H = sum_l J_l^T I_l J_l``
    with I_l the link's world-frame spatial inertia -- ``qd^T H qd / 2`` is the articulation's kinetic energy for the ``body_qd``
    :func:`eval_fk` produces.  Symmetric bit for bit, both triangles written, padding zero.  No armature is added: this is NOT the
    matrix SolverFeatherstone factorises (that one carries the dof armature and the solver's internal FREE-joint convention).
    ``body_I_s`` [body_count, 6, 6] (optional) receives each link's spatial inertia about the world origin.  ``J`` / ``joint_S_s``, if
    given, are filled by an additional :func:`eval_jacobian` launch; H itself is one launch of its own (nt_eval_mass_matrix) and never
    reads J.  Inputs, allocation, ``mask`` and capture behaviour as for :func:`eval_jacobian` (after a maximal-coordinate step call
    :func:`eval_ik` first)."""
    art_sel = _mask_selection(model, mask, "eval_mass_matrix")
    if J is not None or joint_S_s is not None:
        eval_jacobian(model, state, J, joint_S_s, mask)
    if getattr(model, "is_heterogeneous", False):
        return _eval_jm_groups(model, state, "mass_matrix", H, body_I_s, art_sel)
    D = _art_dims(model)[1]
    if not getattr(model, "is_gpu", False):
        return eval_mass_matrix_numpy(model, _host_array(state.body_q), _host_array(state.joint_q), H, body_I_s, art_sel)
    t = model.env
    return _eval_jm_device(model, state, "eval_mass_matrix", H, "H", (t.env_count * t.na, D, D),
                           body_I_s, "body_I_s", (t.env_count * t.nb, 6, 6), art_sel)


def _eval_jm_groups(model, state, which, out, aux, art_sel):
    """Heterogeneous model: one call per world group; a group's articulations are a slice of the global outputs, padded to the
    maxima over the groups (L, D)."""
    groups = model.world_groups
    parts = groups.parts
    L, D = _art_dims(model)
    A = int(model.articulation_count)
    gpu = getattr(model, "is_gpu", False)
    shape = (A, 6 * L, D) if which == "jacobian" else (A, D, D)
    aux_key, aux_shape = (("joint_dof_count", (int(model.joint_dof_count), 6)) if which == "jacobian"
                          else ("body_count", (int(model.body_count), 6, 6)))
    if not gpu:
        fn = eval_jacobian_numpy if which == "jacobian" else eval_mass_matrix_numpy
        return fn(model, _host_array(state.body_q), _host_array(state.joint_q), out, aux, art_sel)
    import torch  # noqa: PLC0415

    dev = parts[0].device_model().device
    if out is None:
        out = torch.zeros(shape, dtype=torch.float32, device=dev)
    elif not (hasattr(out, "data_ptr") and out.dtype == torch.float32 and tuple(out.shape) == shape):
        raise ValueError(f"the output must be a float32 tensor of shape {shape}")
    if aux is not None and not (hasattr(aux, "data_ptr") and aux.dtype == torch.float32 and tuple(aux.shape) == aux_shape):
        raise ValueError(f"the optional output must be a float32 tensor of shape {aux_shape}")
    a_edges = np.concatenate([[0], np.cumsum([p.articulation_count for p in parts])])
    x_edges = np.concatenate([[0], np.cumsum([getattr(p, aux_key) for p in parts])])
    call = eval_jacobian if which == "jacobian" else eval_mass_matrix

    def go(i, p):
        if not p.articulation_count:
            return
        a0, a1 = int(a_edges[i]), int(a_edges[i + 1])
        sel = None if art_sel is None else art_sel[a0:a1]
        Lp, Dp = _art_dims(p)
        xs = None if aux is None else aux[int(x_edges[i]):int(x_edges[i + 1])]
        same = (Lp, Dp) == (L, D) if which == "jacobian" else Dp == D
        if same:  # the group's slice has the global shape: written in place
            call(p, state.parts[i], out[a0:a1], xs, mask=sel) if which == "jacobian" else call(p, state.parts[i], out[a0:a1],
                                                                                                 body_I_s=xs, mask=sel)
            return
        got = call(p, state.parts[i], None, xs, mask=sel) if which == "jacobian" else call(p, state.parts[i], None, body_I_s=xs, mask=sel)
        rows = torch.arange(a0, a1, device=dev) if sel is None else torch.as_tensor(a0 + np.flatnonzero(sel), device=dev)
        pick = slice(None) if sel is None else torch.as_tensor(np.flatnonzero(sel), device=dev)
        out[rows] = 0.0
        if which == "jacobian":
            out[rows, :6 * Lp, :Dp] = got[pick]
        else:
            out[rows, :Dp, :Dp] = got[pick]

    groups.run(go)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# eval_inverse_dynamics
# ---------------------------------------------------------------------------------------------------------------------------------
NT_ID_GRAVITY, NT_ID_VELOCITY = 1, 2  # include/newton_hip_kinematics.h


def _parent_first(model, what):
    """The walk down a link's root path takes the dofs in ascending order: a joint's ancestor must come before it."""
    t = model.env
    ok = getattr(t, "_parent_first", None)
    if ok is None:
        _, anc = _joint_ancestors(t)
        ok = bool(np.all(anc < np.arange(t.nj)))
        try:
            t._parent_first = ok
        except AttributeError:
            pass
    if not ok:
        raise NotImplementedError(f"{what}: the joints of an articulation must come parent before child (unsupported)")


def _joint_pivots_numpy(model, body_q, joint_q):
    """[E, nj, 3] in float64: the point the angular columns of each joint pass through (_motion_subspace_numpy's)."""
    t = model.env
    E, nb, nj = t.env_count, t.nb, t.nj
    bq = np.asarray(body_q, dtype=np.float64).reshape(E, nb, 7)
    jq = np.asarray(joint_q, dtype=np.float64).reshape(E, t.nc)
    com = np.asarray(model.body_com, dtype=np.float64).reshape(E, nb, 3)
    X_p = np.asarray(model.joint_X_p, dtype=np.float64).reshape(E, nj, 7)
    axis_all = np.asarray(model.joint_axis, dtype=np.float64).reshape(E, t.nd, 3)
    piv = np.zeros((E, nj, 3))
    for j in range(nj):
        jt, parent, child = int(t.joint_type[j]), int(t.joint_parent[j]), int(t.joint_child[j])
        qs, ds, lin = int(t.joint_q_start[j]), int(t.joint_qd_start[j]), int(t.joint_lin_count[j])
        X_wpj = X_p[:, j] if parent < 0 else _xmul(bq[:, parent], X_p[:, j])
        if jt in (JointType.FREE, JointType.DISTANCE):
            piv[:, j] = bq[:, child, :3] + _qrot(bq[:, child, 3:], com[:, child])
        elif jt == JointType.D6:
            pos = np.zeros((E, 3))
            for k in range(lin):
                pos += axis_all[:, ds + k] * jq[:, qs + k:qs + k + 1]
            piv[:, j] = X_wpj[:, :3] + _qrot(X_wpj[:, 3:], pos)
        else:
            piv[:, j] = X_wpj[:, :3]
    return piv


def _world_gravity(model):
    """[E, 3] float64: the gravity row of each world (the row of its first body, as the device tables)."""
    t = model.env
    g = np.asarray(model.gravity, dtype=np.float64).reshape(-1, 3)
    world = np.asarray(model.body_world).reshape(t.env_count, t.nb)[:, 0] if t.nb else np.zeros(t.env_count, dtype=np.int64)
    return g[world]


def _split_parts(parts, value, key, width=None):
    sizes = np.cumsum([getattr(p, key) for p in parts])[:-1]
    a = np.asarray(value)
    return np.split(a.reshape(-1) if width is None else a.reshape(-1, width), sizes)


def eval_inverse_dynamics_numpy(model, body_q, joint_q, joint_qd, joint_qdd=None, tau=None, gravity=True, velocity_terms=True, art_sel=None):
    """Host mirror of eval_inverse_dynamics_kernel: tau [articulation_count, D] = sum over links of J_l^T f_l with
    f_l = I_l a_l + v_l x* (I_l v_l) - (m_l g, c_l x m_l g), in float64 from the definition of include/newton_hip_kinematics.h (about the
    world origin, link by link; the kernel works about the root link), float32 out.  ``joint_qdd`` [articulation_count, D] or None (zero);
    the slices of articulations ``art_sel`` leaves out stay untouched."""
    D = _art_dims(model)[1]
    A = int(model.articulation_count)
    tau = _new_or_checked(tau, (A, D), "tau")
    if joint_qdd is not None:
        joint_qdd = np.asarray(joint_qdd)
        if joint_qdd.shape != (A, D):
            raise ValueError(f"joint_qdd must have shape {(A, D)}")
    if getattr(model, "is_heterogeneous", False):
        parts = model.world_groups.parts
        bqs, jqs = _split_parts(parts, body_q, "body_count", 7), _split_parts(parts, joint_q, "joint_coord_count")
        jqds = _split_parts(parts, joint_qd, "joint_dof_count")
        a0 = 0
        for p, bq, jq, jqd in zip(parts, bqs, jqs, jqds):
            a1 = a0 + p.articulation_count
            if p.articulation_count:
                sel = None if art_sel is None else np.asarray(art_sel, dtype=bool)[a0:a1]
                Dp = _art_dims(p)[1]
                tp = np.array(tau[a0:a1, :Dp])
                eval_inverse_dynamics_numpy(p, bq, jq, jqd, None if joint_qdd is None else joint_qdd[a0:a1, :Dp], tp, gravity,
                                            velocity_terms, sel)
                rows = slice(a0, a1) if sel is None else a0 + np.flatnonzero(sel)
                tau[rows] = 0.0
                tau[rows, :Dp] = tp if sel is None else tp[sel]
            a0 = a1
        return tau
    t = _articulated(model, "eval_inverse_dynamics")
    check_ik_supported(model)
    _parent_first(model, "eval_inverse_dynamics")
    E = t.env_count
    blocks = _inverse_dynamics_float64(model, body_q, joint_q, joint_qd, joint_qdd, gravity, velocity_terms)
    sel = np.ones((E, t.na), dtype=bool) if art_sel is None else np.asarray(art_sel, dtype=bool).reshape(E, t.na)
    tv = tau.reshape(E, t.na, D)
    for k in range(t.na):
        tv[sel[:, k], k] = blocks[sel[:, k], k].astype(np.float32)
    return tau


def _inverse_dynamics_float64(model, body_q, joint_q, joint_qd, joint_qdd, gravity, velocity_terms, link_wrench=None):
    """tau [E, na, D] in float64, before any rounding (homogeneous model).  ``link_wrench`` [E, nb, 6] (optional): an external wrench
    on each link about the world origin, subtracted from f_l -- tau then holds h - sum_l J_l^T w_l."""
    t = model.env
    E, nd, D = t.env_count, t.nd, _art_dims(model)[1]
    S = _motion_subspace_numpy(model, body_q, joint_q)
    I_s = _spatial_inertia_numpy(model, body_q)
    piv = _joint_pivots_numpy(model, body_q, joint_q)
    on = _path_matrix(t)
    dof_joint = np.searchsorted(t.joint_qd_start, np.arange(nd), side="right") - 1 if nd else np.zeros(0, dtype=np.int64)
    qd = np.asarray(joint_qd, dtype=np.float64).reshape(E, nd) if velocity_terms else np.zeros((E, nd))
    qdd = np.zeros((E, nd))
    ranges = _art_ranges(t)
    if joint_qdd is not None:
        for k, (_j0, _nja, d0, nda) in enumerate(ranges):
            qdd[:, d0:d0 + nda] = np.asarray(joint_qdd, dtype=np.float64).reshape(E, t.na, D)[:, k, :nda]
    g = _world_gravity(model) if gravity else np.zeros((E, 3))
    out = np.zeros((E, t.na, D))
    for k, (j0, nja, d0, nda) in enumerate(ranges):
        blk = np.zeros((E, D))
        for j in range(j0, j0 + nja):
            # v_l and a_l = J_l qdd + sum S'_d qd_d down the root path (the running twist is the twist of the frame that carries the
            # next dof's pivot; its angular part the rate of a D6's axis frame, every other joint's axes ride on the parent link)
            v, w, al, aw, w_parent = (np.zeros((E, 3)) for _ in range(5))
            for d in range(d0, d0 + nda):
                jd = int(dof_joint[d])
                if not on[j, jd]:
                    continue
                jt, i = int(t.joint_type[jd]), d - int(t.joint_qd_start[jd])
                if i == 0:
                    w_parent = w.copy()
                angular = (jt in (JointType.REVOLUTE, JointType.BALL) or (jt in (JointType.FREE, JointType.DISTANCE) and i >= 3)
                           or (jt == JointType.D6 and i >= int(t.joint_lin_count[jd])))
                sv, sw = S[:, d, :3], S[:, d, 3:]
                w_frame = w if jt == JointType.D6 else w_parent
                if angular:
                    p_dot = v + np.cross(w, piv[:, jd])
                    dbottom = np.cross(w_frame, sw)
                    dtop = np.cross(p_dot, sw) + np.cross(piv[:, jd], dbottom)
                else:
                    dtop, dbottom = np.cross(w_frame, sv), np.zeros((E, 3))
                al = al + sv * qdd[:, d:d + 1] + dtop * qd[:, d:d + 1]
                aw = aw + sw * qdd[:, d:d + 1] + dbottom * qd[:, d:d + 1]
                v = v + sv * qd[:, d:d + 1]
                w = w + sw * qd[:, d:d + 1]
            Il = I_s[:, int(t.joint_child[j])]
            vl, acc = np.concatenate([v, w], axis=1), np.concatenate([al - g, aw], axis=1)
            mom = np.einsum("eij,ej->ei", Il, vl)
            f = np.einsum("eij,ej->ei", Il, acc)
            f[:, :3] += np.cross(w, mom[:, :3])
            f[:, 3:] += np.cross(w, mom[:, 3:]) + np.cross(v, mom[:, :3])
            if link_wrench is not None:
                f -= link_wrench[:, int(t.joint_child[j])]
            cols = on[j, dof_joint[d0:d0 + nda]]
            blk[:, :nda] += np.einsum("edi,ei->ed", S[:, d0:d0 + nda], f) * cols
        out[:, k] = blk
    return out


def _device_in(model, value, shape, what):
    """A resident float32 tensor as it is (checked); anything else is uploaded (one allocation and one host-to-device copy)."""
    import torch  # noqa: PLC0415

    if hasattr(value, "data_ptr"):
        return _device_out(model, value, shape, what)
    a = np.ascontiguousarray(value, dtype=np.float32)
    if a.shape != tuple(shape):
        raise ValueError(f"{what} must have shape {tuple(shape)}")
    return torch.from_numpy(a).to(model.device_model().device)


def eval_inverse_dynamics(model, state, joint_qdd=None, tau=None, gravity=True, velocity_terms=True, mask=None):
    """Inverse dynamics in the convention of :func:`eval_jacobian` / :func:`eval_mass_matrix`: the joint torques ``tau``
    [articulation_count, D] float32 (D = ``model.max_dofs_per_articulation``, the rows of ``H``) that produce the joint acceleration
    ``joint_qdd`` [articulation_count, D] at the state's ``joint_q`` / ``joint_qd``:

        ``tau = H joint_qdd + h(q, qd)``,  ``h = C(q, qd) qd + g(q)``, the bias forces

    with eval_mass_matrix's ``H`` -- ``torch.bmm(H, joint_qdd[..., None])`` lines up.  ``joint_qdd=None`` is zero: the call returns
    ``h``; with ``velocity_terms=False`` the generalized gravity forces alone (what holds the robot still), with ``gravity=False`` the
    Coriolis / centrifugal forces alone; both off and no ``joint_qdd``: exactly zero.  ``tau . joint_qd`` is power with respect to the
    public ``joint_qd`` (a FREE / DISTANCE joint carries the COM velocity).  The rigid-body term only, like ``H``: no armature, no joint
    limits, no drives, no friction -- and not the bias force SolverFeatherstone forms internally (its FREE-joint convention differs; for
    chains of 1-dof joints the two coincide, so ``control.joint_f = h`` cancels gravity and velocity terms there).  The padding of
    ``tau`` is written as zero on every call; ``mask`` (bool per articulation) leaves the slices of unselected articulations untouched.

    Reads ``state.body_q``, ``state.joint_q`` and ``state.joint_qd``: after a maximal-coordinate step (SolverXPBD, SolverSemiImplicit)
    call :func:`eval_ik` first.  A ``tau`` left ``None`` is allocated and returned: a torch tensor on a GPU model, a numpy array on a
    host model.  On a GPU model with ``tau`` (and ``joint_qdd``, if used) supplied as resident float32 tensors and no ``mask`` the call
    is one kernel launch on the model's stream (nt_eval_inverse_dynamics): no allocation, no synchronisation, it records into
    ``newton_amd.graph.capture`` -- ``joint_qdd`` is read at launch time, an in-place update followed by a replay takes effect.  A mask
    uploads its bytes on every call, a ``joint_qdd`` that is not a device tensor is uploaded.  Multi-axis D6 joints as for
    :func:`eval_ik`."""
    art_sel = _mask_selection(model, mask, "eval_inverse_dynamics")
    if getattr(model, "is_heterogeneous", False):
        return _eval_id_groups(model, state, joint_qdd, tau, gravity, velocity_terms, art_sel)
    D = _art_dims(model)[1]
    if not getattr(model, "is_gpu", False):
        return eval_inverse_dynamics_numpy(model, _host_array(state.body_q), _host_array(state.joint_q), _host_array(state.joint_qd),
                                           None if joint_qdd is None else _host_array(joint_qdd), tau, gravity, velocity_terms, art_sel)
    import ctypes as C  # noqa: PLC0415

    from . import _lib  # noqa: PLC0415

    t = _articulated(model, "eval_inverse_dynamics")
    check_ik_supported(model)
    _parent_first(model, "eval_inverse_dynamics")
    dm = model.device_model()
    shape = (t.env_count * t.na, D)
    fresh = tau is None
    tau = _device_out(model, tau, shape, "tau")
    if joint_qdd is not None:
        joint_qdd = _device_in(model, joint_qdd, shape, "joint_qdd")
    if fresh and art_sel is not None:
        tau.zero_()
    art_mask = _device_art_mask(model, art_sel, "eval_inverse_dynamics")
    d = state._desc()
    flags = (NT_ID_GRAVITY if gravity else 0) | (NT_ID_VELOCITY if velocity_terms else 0)
    _lib.check(dm.lib.nt_eval_inverse_dynamics(C.byref(dm.desc), C.byref(d), None if joint_qdd is None else joint_qdd.data_ptr(), flags,
                                               tau.data_ptr(), None if art_mask is None else art_mask.data_ptr(), dm.stream()),
               "nt_eval_inverse_dynamics")
    return tau


def _eval_id_groups(model, state, joint_qdd, tau, gravity, velocity_terms, art_sel):
    """Heterogeneous model: one call per world group (_eval_jm_groups' pattern); a group's articulations are a slice of the global
    [articulation_count, D] arrays, padded to the widest group's D."""
    groups = model.world_groups
    parts = groups.parts
    D = _art_dims(model)[1]
    A = int(model.articulation_count)
    if not getattr(model, "is_gpu", False):
        return eval_inverse_dynamics_numpy(model, _host_array(state.body_q), _host_array(state.joint_q), _host_array(state.joint_qd),
                                           None if joint_qdd is None else _host_array(joint_qdd), tau, gravity, velocity_terms, art_sel)
    import torch  # noqa: PLC0415

    dev = parts[0].device_model().device
    if tau is None:
        tau = torch.zeros((A, D), dtype=torch.float32, device=dev)
    elif not (hasattr(tau, "data_ptr") and tau.dtype == torch.float32 and tuple(tau.shape) == (A, D)):
        raise ValueError(f"tau must be a float32 tensor of shape {(A, D)}")
    if joint_qdd is not None:
        if not hasattr(joint_qdd, "data_ptr"):
            joint_qdd = torch.from_numpy(np.ascontiguousarray(joint_qdd, dtype=np.float32)).to(dev)
        if joint_qdd.dtype != torch.float32 or tuple(joint_qdd.shape) != (A, D):
            raise ValueError(f"joint_qdd must be a float32 tensor of shape {(A, D)}")
    a_edges = np.concatenate([[0], np.cumsum([p.articulation_count for p in parts])])

    def go(i, p):
        if not p.articulation_count:
            return
        a0, a1 = int(a_edges[i]), int(a_edges[i + 1])
        sel = None if art_sel is None else art_sel[a0:a1]
        Dp = _art_dims(p)[1]
        kw = dict(gravity=gravity, velocity_terms=velocity_terms, mask=sel)
        if Dp == D:  # the group's slice has the global shape: read and written in place
            eval_inverse_dynamics(p, state.parts[i], None if joint_qdd is None else joint_qdd[a0:a1], tau[a0:a1], **kw)
            return
        got = eval_inverse_dynamics(p, state.parts[i], None if joint_qdd is None else joint_qdd[a0:a1, :Dp].contiguous(), None, **kw)
        rows = torch.arange(a0, a1, device=dev) if sel is None else torch.as_tensor(a0 + np.flatnonzero(sel), device=dev)
        pick = slice(None) if sel is None else torch.as_tensor(np.flatnonzero(sel), device=dev)
        tau[rows] = 0.0
        tau[rows, :Dp] = got[pick]

    groups.run(go)
    return tau


# ---------------------------------------------------------------------------------------------------------------------------------
# eval_forward_dynamics
# ---------------------------------------------------------------------------------------------------------------------------------
NT_FD_GRAVITY, NT_FD_VELOCITY, NT_FD_BODY_F = 1, 2, 4  # include/newton_hip_kinematics.h


def _new_or_checked_info(info, count):
    if info is None:
        return None
    if not isinstance(info, np.ndarray) or info.dtype != np.int32 or info.shape != (count,):
        raise ValueError(f"info must be an int32 numpy array of shape {(count,)}")
    return info


def eval_forward_dynamics_numpy(model, body_q, joint_q, joint_qd, joint_f=None, body_f=None, joint_qdd=None, gravity=True,
                                velocity_terms=True, info=None, art_sel=None):
    """Host mirror of eval_forward_dynamics_kernel: joint_qdd [articulation_count, D] from H joint_qdd = joint_f + sum_l J_l^T w_l - h,
    in float64 from the parts of eval_mass_matrix_numpy, eval_inverse_dynamics_numpy and eval_jacobian_numpy before their rounding, one
    Cholesky solve per articulation, float32 out.  ``joint_f`` [articulation_count, D] or None (zero); ``body_f`` [body_count, 6]
    (world-frame force and torque about each link's COM) or None (no external wrench).  A pivot that is not > 0: the articulation's
    entries are NaN and its ``info`` (int32 [articulation_count], optional) the 1-based column, otherwise 0.  The slices of
    articulations ``art_sel`` leaves out stay untouched, in ``info`` too."""
    D = _art_dims(model)[1]
    A = int(model.articulation_count)
    joint_qdd = _new_or_checked(joint_qdd, (A, D), "joint_qdd")
    info = _new_or_checked_info(info, A)
    if joint_f is not None:
        joint_f = np.asarray(joint_f)
        if joint_f.shape != (A, D):
            raise ValueError(f"joint_f must have shape {(A, D)}")
    if body_f is not None:
        body_f = np.asarray(body_f)
        if body_f.shape != (int(model.body_count), 6):
            raise ValueError(f"body_f must have shape {(int(model.body_count), 6)}")
    if getattr(model, "is_heterogeneous", False):
        parts = model.world_groups.parts
        bqs, jqs = _split_parts(parts, body_q, "body_count", 7), _split_parts(parts, joint_q, "joint_coord_count")
        jqds = _split_parts(parts, joint_qd, "joint_dof_count")
        bfs = [None] * len(parts) if body_f is None else _split_parts(parts, body_f, "body_count", 6)
        a0 = 0
        for p, bq, jq, jqd, bf in zip(parts, bqs, jqs, jqds, bfs):
            a1 = a0 + p.articulation_count
            if p.articulation_count:
                sel = None if art_sel is None else np.asarray(art_sel, dtype=bool)[a0:a1]
                Dp = _art_dims(p)[1]
                out = np.array(joint_qdd[a0:a1, :Dp])
                eval_forward_dynamics_numpy(p, bq, jq, jqd, None if joint_f is None else joint_f[a0:a1, :Dp], bf, out, gravity,
                                            velocity_terms, None if info is None else info[a0:a1], sel)
                rows = slice(a0, a1) if sel is None else a0 + np.flatnonzero(sel)
                joint_qdd[rows] = 0.0
                joint_qdd[rows, :Dp] = out if sel is None else out[sel]
            a0 = a1
        return joint_qdd
    t = _articulated(model, "eval_forward_dynamics")
    check_ik_supported(model)
    _parent_first(model, "eval_forward_dynamics")
    E = t.env_count
    wrench = None
    if body_f is not None:  # (F, T) at the COM -> (F, T + c x F) about the world origin: what J_l^T takes
        bq = np.asarray(body_q, dtype=np.float64).reshape(E, t.nb, 7)
        cw = bq[..., :3] + _qrot(bq[..., 3:], np.asarray(model.body_com, dtype=np.float64).reshape(E, t.nb, 3))
        w = np.asarray(body_f, dtype=np.float64).reshape(E, t.nb, 6)
        wrench = np.concatenate([w[..., :3], w[..., 3:] + np.cross(cw, w[..., :3])], axis=-1)
    H, _ = _mass_matrix_float64(model, body_q, joint_q)
    b = -_inverse_dynamics_float64(model, body_q, joint_q, joint_qd, None, gravity, velocity_terms, wrench)
    if joint_f is not None:
        b += np.asarray(joint_f, dtype=np.float64).reshape(E, t.na, D)
    sel = np.ones((E, t.na), dtype=bool) if art_sel is None else np.asarray(art_sel, dtype=bool).reshape(E, t.na)
    out, inf = joint_qdd.reshape(E, t.na, D), None if info is None else info.reshape(E, t.na)
    for k, (_j0, _nja, _d0, nda) in enumerate(_art_ranges(t)):
        for e in np.flatnonzero(sel[:, k]):
            row, bad = np.zeros(D), 0
            A_, L = H[e, k, :nda, :nda], np.zeros((nda, nda))
            for j in range(nda):  # column by column, the kernel's order: the first pivot that is not > 0 is reported
                p = A_[j, j] - L[j, :j] @ L[j, :j]
                if not p > 0.0:
                    bad = j + 1
                    break
                L[j, j] = np.sqrt(p)
                L[j + 1:, j] = (A_[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
            if bad:
                row[:nda] = np.nan
            elif nda:
                y = np.linalg.solve(L, b[e, k, :nda])  # (triangular systems)
                row[:nda] = np.linalg.solve(L.T, y)
            out[e, k] = row.astype(np.float32)
            if inf is not None:
                inf[e, k] = bad
    return joint_qdd


def eval_forward_dynamics(model, state, joint_f=None, joint_qdd=None, body_f=False, gravity=True, velocity_terms=True, info=None, mask=None):
    """Forward dynamics in the convention of :func:`eval_mass_matrix` / :func:`eval_inverse_dynamics`: the joint accelerations
    ``joint_qdd`` [articulation_count, D] float32 that the joint forces ``joint_f`` [articulation_count, D] (``None``: zero) produce at
    the state's ``joint_q`` / ``joint_qd``:

        ``H joint_qdd = joint_f + sum_l J_l^T w_l - h(q, qd)``

    with eval_mass_matrix's ``H``, eval_jacobian's ``J`` and eval_inverse_dynamics's bias forces ``h`` -- so
    ``eval_inverse_dynamics(joint_qdd=eval_forward_dynamics(joint_f))`` returns ``joint_f`` (``body_f`` off).  ``body_f=True`` reads the
    external link wrenches ``w_l`` from ``state.body_f`` -- what collide and the contact evaluation leave there: world-frame force and
    torque about each link's COM, the convention the steppers consume.  ``gravity`` / ``velocity_terms`` select the parts of ``h``; all
    three off and no ``joint_f``: exactly zero.  The rigid-body terms only: no armature, no joint limits, no drives, no friction -- not
    the acceleration SolverFeatherstone integrates (for fixed-base chains of 1-dof joints without armature the two coincide).

    An articulation whose ``H`` is not positive definite (a massless leaf link, a non-finite input) gets NaN in its entries and the
    1-based column of the failing pivot in ``info`` (int32 [articulation_count], optional; 0 otherwise); no other articulation is
    affected.  The padding of ``joint_qdd`` is written as zero on every call; ``mask`` (bool per articulation) leaves the slices of
    unselected articulations untouched, in ``info`` too.

    Reads ``state.body_q``, ``state.joint_q``, ``state.joint_qd`` (after a maximal-coordinate step call :func:`eval_ik` first) and, with
    ``body_f=True``, ``state.body_f``.  A ``joint_qdd`` left ``None`` is allocated and returned: a torch tensor on a GPU model, a numpy
    array (computed in float64) on a host model.  On a GPU model with ``joint_qdd`` (and ``joint_f`` / ``info``, if used) supplied as
    resident tensors and no ``mask`` the call is one kernel launch on the model's stream (nt_eval_forward_dynamics): no allocation, no
    synchronisation, it records into ``newton_amd.graph.capture`` -- ``joint_f`` is read at launch time, an in-place update followed by
    a replay takes effect.  Multi-axis D6 joints as for :func:`eval_ik`."""
    art_sel = _mask_selection(model, mask, "eval_forward_dynamics")
    if getattr(model, "is_heterogeneous", False) and getattr(model, "is_gpu", False):
        return _eval_fd_groups(model, state, joint_f, joint_qdd, body_f, gravity, velocity_terms, info, art_sel)
    D = _art_dims(model)[1]
    if not getattr(model, "is_gpu", False):
        return eval_forward_dynamics_numpy(model, _host_array(state.body_q), _host_array(state.joint_q), _host_array(state.joint_qd),
                                           None if joint_f is None else _host_array(joint_f),
                                           _host_array(state.body_f) if body_f else None, joint_qdd, gravity, velocity_terms, info, art_sel)
    import ctypes as C  # noqa: PLC0415

    import torch  # noqa: PLC0415

    from . import _lib  # noqa: PLC0415

    t = _articulated(model, "eval_forward_dynamics")
    check_ik_supported(model)
    _parent_first(model, "eval_forward_dynamics")
    dm = model.device_model()
    shape = (t.env_count * t.na, D)
    fresh = joint_qdd is None
    joint_qdd = _device_out(model, joint_qdd, shape, "joint_qdd")
    if joint_f is not None:
        joint_f = _device_in(model, joint_f, shape, "joint_f")
    if info is not None and not (hasattr(info, "data_ptr") and info.dtype == torch.int32 and info.is_cuda and info.is_contiguous()
                                 and tuple(info.shape) == (shape[0],)):
        raise ValueError(f"info must be a contiguous int32 tensor of shape {(shape[0],)} on the model's device")
    if fresh and art_sel is not None:
        joint_qdd.zero_()
    art_mask = _device_art_mask(model, art_sel, "eval_forward_dynamics")
    d = state._desc()
    flags = (NT_FD_GRAVITY if gravity else 0) | (NT_FD_VELOCITY if velocity_terms else 0) | (NT_FD_BODY_F if body_f else 0)
    _lib.check(dm.lib.nt_eval_forward_dynamics(C.byref(dm.desc), C.byref(d), None if joint_f is None else joint_f.data_ptr(), flags,
                                               joint_qdd.data_ptr(), None if info is None else info.data_ptr(),
                                               None if art_mask is None else art_mask.data_ptr(), dm.stream()),
               "nt_eval_forward_dynamics")
    return joint_qdd


def _eval_fd_groups(model, state, joint_f, joint_qdd, body_f, gravity, velocity_terms, info, art_sel):
    """Heterogeneous model on the device: one call per world group (_eval_id_groups' pattern); a group's articulations are a slice of
    the global [articulation_count, D] arrays, padded to the widest group's D."""
    import torch  # noqa: PLC0415

    groups = model.world_groups
    parts = groups.parts
    D = _art_dims(model)[1]
    A = int(model.articulation_count)
    dev = parts[0].device_model().device
    if joint_qdd is None:
        joint_qdd = torch.zeros((A, D), dtype=torch.float32, device=dev)
    elif not (hasattr(joint_qdd, "data_ptr") and joint_qdd.dtype == torch.float32 and tuple(joint_qdd.shape) == (A, D)):
        raise ValueError(f"joint_qdd must be a float32 tensor of shape {(A, D)}")
    if joint_f is not None:
        if not hasattr(joint_f, "data_ptr"):
            joint_f = torch.from_numpy(np.ascontiguousarray(joint_f, dtype=np.float32)).to(dev)
        if joint_f.dtype != torch.float32 or tuple(joint_f.shape) != (A, D):
            raise ValueError(f"joint_f must be a float32 tensor of shape {(A, D)}")
    if info is not None and not (hasattr(info, "data_ptr") and info.dtype == torch.int32 and tuple(info.shape) == (A,)):
        raise ValueError(f"info must be an int32 tensor of shape {(A,)}")
    a_edges = np.concatenate([[0], np.cumsum([p.articulation_count for p in parts])])

    def go(i, p):
        if not p.articulation_count:
            return
        a0, a1 = int(a_edges[i]), int(a_edges[i + 1])
        sel = None if art_sel is None else art_sel[a0:a1]
        Dp = _art_dims(p)[1]
        kw = dict(body_f=body_f, gravity=gravity, velocity_terms=velocity_terms, info=None if info is None else info[a0:a1], mask=sel)
        if Dp == D:  # the group's slice has the global shape: read and written in place
            eval_forward_dynamics(p, state.parts[i], None if joint_f is None else joint_f[a0:a1], joint_qdd[a0:a1], **kw)
            return
        got = eval_forward_dynamics(p, state.parts[i], None if joint_f is None else joint_f[a0:a1, :Dp].contiguous(), None, **kw)
        rows = torch.arange(a0, a1, device=dev) if sel is None else torch.as_tensor(a0 + np.flatnonzero(sel), device=dev)
        pick = slice(None) if sel is None else torch.as_tensor(np.flatnonzero(sel), device=dev)
        joint_qdd[rows] = 0.0
        joint_qdd[rows, :Dp] = got[pick]

    groups.run(go)
    return joint_qdd
