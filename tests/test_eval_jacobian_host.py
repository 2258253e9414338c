"""newton_amd.eval_jacobian / eval_mass_matrix on the host: a float64 closed-form reference of the contract
(include/newton_hip_kinematics.h), validated against eval_fk_numpy (column by column, kinetic energy) and against the closed forms of a
single and a double pendulum; the numpy paths against it; selection; padding; the C header against the ctypes table.

The reference, the scenes and the gates below are shared with tests/test_eval_jacobian_emu.py and tests/test_gpu_eval_jacobian.py.
Gates (errors against the float64 reference evaluated on the same fp32 inputs):
  J, joint_S_s   1e-5 * max(1, R) per entry, R the largest anchor / COM distance from the origin in that world -- the standing
                 single-call kinematics gate (an entry is a unit axis or its cross product with a point of that size)
  H              1e-5 * max|H_ref| of that articulation
  body_I_s       1e-5 * max|I_ref| of that body (a handful of fp32 products and sums per entry, 6e-8 each, relative to m |c|^2)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import newton_amd as nt
from newton_amd import _lib
from newton_amd import _np_math as nm
from newton_amd.articulation import eval_fk_numpy, eval_jacobian_numpy, eval_mass_matrix_numpy
from test_eval_ik_host import SCENES as IK_SCENES
from test_eval_ik_host import random_joint_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "newton_hip_kinematics.h")
JT = nt.JointType
GATE = 1e-5
POISON = 7.0


def multi_art_scene(world_count, device=None):
    """Three articulations of different widths per world: two free spheres (1 joint, 6 dofs each) and a two-link pendulum (2 joints,
    2 dofs): L = 2, D = 6 -- every articulation is padded, in rows or in columns."""
    env = nt.ModelBuilder()
    cfg = nt.ModelBuilder.ShapeConfig(has_shape_collision=False)
    for k in range(2):
        b = env.add_body(xform=[0.4 * k, -0.3, 1.2 + 0.1 * k, 0.0, 0.0, 0.0, 1.0])
        env.add_shape_sphere(b, xform=nm.transform([0.02, -0.01 * k, 0.015]), radius=0.1 + 0.02 * k, cfg=cfg)
    a, b = env.add_link(xform=[0.0, 0.5, 1.0, 0, 0, 0, 1]), env.add_link(xform=[0.4, 0.5, 1.0, 0, 0, 0, 1])
    for k, link in enumerate((a, b)):
        env.add_shape_box(link, xform=nm.transform([0.03, 0.0, 0.01 * k]), hx=0.2, hy=0.05, hz=0.04 + 0.01 * k, cfg=cfg)
    j0 = env.add_joint_revolute(-1, a, axis=[0.0, 1.0, 0.0], parent_xform=nm.transform([0.0, 0.5, 1.0], nm.quat_rpy(0.1, 0.0, 0.3)),
                                child_xform=nm.transform([-0.2, 0.0, 0.0]))
    j1 = env.add_joint_revolute(a, b, axis=[0.6, 0.0, 0.8], parent_xform=nm.transform([0.2, 0.01, 0.0]),
                                child_xform=nm.transform([-0.2, 0.0, 0.02], nm.quat_rpy(0.0, 0.2, 0.0)))
    env.add_articulation([j0, j1])
    scene = nt.ModelBuilder()
    scene.replicate(env, world_count)
    return scene.finalize(device=device)


SCENES = dict(IK_SCENES)
SCENES["multi_art"] = lambda E, device=None: multi_art_scene(E, device=device)


def fk_case(name, E, seed):
    """model, the random (joint_q, joint_qd) and eval_fk's fp32 body state for them."""
    model = SCENES[name](E)
    jq, jqd = random_joint_state(model, seed)
    bq, bqd = eval_fk_numpy(model, jq, jqd)
    return model, jq, jqd, bq, bqd


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 reference: one articulation at a time over the model's flat arrays (homogeneous or not)
# ---------------------------------------------------------------------------------------------------------------------------------
def _R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _axis_angle_R(axis, angle):
    a = np.asarray(axis) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _skew(c):
    return np.array([[0, -c[2], c[1]], [c[2], 0, -c[0]], [-c[1], c[0], 0]])


class Reference:
    """J [A, 6 L, D], S [dofs, 6], H [A, D, D], I [bodies, 6, 6] in float64, and R [A]: the largest anchor / COM distance from the
    origin in the articulation's world."""


def jacobian_reference(model, body_q, joint_q):
    bq = np.asarray(body_q, dtype=np.float64).reshape(-1, 7)
    jq = np.asarray(joint_q, dtype=np.float64).reshape(-1)
    com = np.asarray(model.body_com, dtype=np.float64).reshape(-1, 3)
    X_p = np.asarray(model.joint_X_p, dtype=np.float64).reshape(-1, 7)
    axes = np.asarray(model.joint_axis, dtype=np.float64).reshape(-1, 3)
    jtype, jpar, jch = np.asarray(model.joint_type), np.asarray(model.joint_parent), np.asarray(model.joint_child)
    qs_all, ds_all = np.asarray(model.joint_q_start), np.asarray(model.joint_qd_start)
    dd = np.asarray(model.joint_dof_dim).reshape(-1, 2)
    d_edges = np.concatenate([ds_all, [model.joint_dof_count]])
    starts, ends = np.asarray(model.articulation_start), np.asarray(model.articulation_end)
    world = np.asarray(model.articulation_world)
    A = int(model.articulation_count)
    L, D = int((ends - starts).max()), int((d_edges[ends] - d_edges[starts]).max())
    ref = Reference()
    ref.L, ref.D = L, D
    ref.J, ref.S = np.zeros((A, 6 * L, D)), np.zeros((model.joint_dof_count, 6))
    reach = np.zeros(A)
    for a in range(A):
        j0, j1 = int(starts[a]), int(ends[a])
        d0 = int(d_edges[j0])
        child_joint = {int(jch[j]): j for j in range(j0, j1)}
        for j in range(j0, j1):
            p, c, ty = int(jpar[j]), int(jch[j]), int(jtype[j])
            qs, ds, lin, ang = int(qs_all[j]), int(ds_all[j]), int(dd[j, 0]), int(dd[j, 1])
            Rp, pp = _R(X_p[j, 3:]), X_p[j, :3]
            if p >= 0:
                Rb = _R(bq[p, 3:])
                pp, Rp = bq[p, :3] + Rb @ pp, Rb @ Rp
            c_child = bq[c, :3] + _R(bq[c, 3:]) @ com[c]
            reach[a] = max(reach[a], np.linalg.norm(pp), np.linalg.norm(c_child))
            cols = []  # (linear axis | None, angular axis | None, pivot) in the parent anchor frame
            if ty == JT.PRISMATIC:
                cols = [(axes[ds], None, None)]
            elif ty == JT.REVOLUTE:
                cols = [(None, axes[ds], pp)]
            elif ty == JT.BALL:
                cols = [(None, np.eye(3)[k], pp) for k in range(3)]
            elif ty in (JT.FREE, JT.DISTANCE):
                cols = [(np.eye(3)[k], None, None) for k in range(3)] + [(None, np.eye(3)[k], c_child) for k in range(3)]
            elif ty == JT.D6:
                cols = [(axes[ds + k], None, None) for k in range(lin)]
                pj = pp + Rp @ sum((axes[ds + k] * jq[qs + k] for k in range(lin)), np.zeros(3))
                reach[a] = max(reach[a], np.linalg.norm(pj))
                e = [axes[ds + lin + k] for k in range(ang)]
                th = [jq[qs + lin + k] for k in range(ang)]
                if ang == 1:
                    rot = [e[0]]
                elif ang == 2:  # the second axis turned by the first rotation (axes orthonormalised as the builder's frame)
                    a0 = e[0] / np.linalg.norm(e[0])
                    rot = [a0, _axis_angle_R(a0, th[0]) @ e[1]]
                elif ang == 3:
                    R0 = _axis_angle_R(e[0], th[0])
                    a1 = R0 @ e[1]
                    rot = [e[0], a1, _axis_angle_R(a1, th[1]) @ R0 @ e[2]]
                else:
                    rot = []
                cols += [(None, r, pj) for r in rot]
            else:
                assert ty == JT.FIXED
            for k, (al, aa, pivot) in enumerate(cols):
                if aa is None:
                    ref.S[ds + k, :3] = Rp @ al
                else:
                    w = Rp @ aa
                    ref.S[ds + k, :3], ref.S[ds + k, 3:] = np.cross(pivot, w), w
        for j in range(j0, j1):  # link of joint j: its own columns and those of the joints up its parent chain
            k = j
            while k is not None:
                lo, hi = int(d_edges[k]), int(d_edges[k + 1])
                ref.J[a, 6 * (j - j0):6 * (j - j0) + 6, lo - d0:hi - d0] = ref.S[lo:hi].T
                k = child_joint.get(int(jpar[k])) if jpar[k] >= 0 else None
    ref.R = np.array([reach[world == world[a]].max() for a in range(A)])
    return ref


def mass_matrix_reference(model, body_q, ref):
    """Adds H = sum_l J_l^T I_l J_l and I (about the world origin) to a jacobian_reference."""
    bq = np.asarray(body_q, dtype=np.float64).reshape(-1, 7)
    com = np.asarray(model.body_com, dtype=np.float64).reshape(-1, 3)
    mass = np.asarray(model.body_mass, dtype=np.float64).reshape(-1)
    Ib = np.asarray(model.body_inertia, dtype=np.float64).reshape(-1, 3, 3)
    ref.I = np.zeros((model.body_count, 6, 6))
    for b in range(model.body_count):
        Rb = _R(bq[b, 3:])
        cx = _skew(bq[b, :3] + Rb @ com[b])
        ref.I[b] = np.block([[mass[b] * np.eye(3), -mass[b] * cx], [mass[b] * cx, Rb @ Ib[b] @ Rb.T - mass[b] * cx @ cx]])
    starts, ends, jch = np.asarray(model.articulation_start), np.asarray(model.articulation_end), np.asarray(model.joint_child)
    ref.H = np.zeros((len(starts), ref.D, ref.D))
    for a in range(len(starts)):
        for i, j in enumerate(range(int(starts[a]), int(ends[a]))):
            Jl = ref.J[a, 6 * i:6 * i + 6]
            ref.H[a] += Jl.T @ ref.I[int(jch[j])] @ Jl
    return ref


def reference(model, body_q, joint_q):
    return mass_matrix_reference(model, body_q, jacobian_reference(model, body_q, joint_q))


def jm_errors(model, ref, J=None, H=None, S=None, I=None):  # noqa: E741
    """Largest error over its gate scale, per quantity given: {"J": ..., "H": ..., "S": ..., "I": ...} (<= GATE passes)."""
    out = {}
    f64 = lambda x: np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x, dtype=np.float64)  # noqa: E731
    if J is not None:
        out["J"] = float((np.abs(f64(J) - ref.J) / np.maximum(1.0, ref.R)[:, None, None]).max())
    if H is not None:
        out["H"] = float((np.abs(f64(H) - ref.H) / np.abs(ref.H).max(axis=(1, 2), keepdims=True)).max())
    if S is not None:
        d_edges = np.concatenate([np.asarray(model.joint_qd_start), [model.joint_dof_count]])
        starts, ends = np.asarray(model.articulation_start), np.asarray(model.articulation_end)
        scale = np.ones(model.joint_dof_count)
        for a in range(len(starts)):
            scale[d_edges[starts[a]]:d_edges[ends[a]]] = max(1.0, ref.R[a])
        out["S"] = float((np.abs(f64(S) - ref.S) / scale[:, None]).max()) if model.joint_dof_count else 0.0
    if I is not None:
        links = np.asarray(model.joint_child)
        out["I"] = float((np.abs(f64(I) - ref.I)[links] / np.abs(ref.I[links]).max(axis=(1, 2), keepdims=True)).max())
    return out


def within_gates(errs):
    return all(v <= GATE for v in errs.values())


def structure_ok(model, ref, J, H):
    """Padding and non-ancestor entries exactly zero (where the reference has structural zeros), H symmetric bit for bit."""
    J, H = np.asarray(J), np.asarray(H)
    d_edges = np.concatenate([np.asarray(model.joint_qd_start), [model.joint_dof_count]])
    starts, ends, jpar, jch = (np.asarray(getattr(model, k)) for k in ("articulation_start", "articulation_end", "joint_parent", "joint_child"))
    for a in range(len(starts)):
        nja, nda = int(ends[a] - starts[a]), int(d_edges[ends[a]] - d_edges[starts[a]])
        zero = np.ones((6 * ref.L, ref.D), dtype=bool)
        child_joint = {int(jch[j]): j for j in range(int(starts[a]), int(ends[a]))}
        for j in range(int(starts[a]), int(ends[a])):
            k = j
            while k is not None:
                zero[6 * (j - starts[a]):6 * (j - starts[a]) + 6, d_edges[k] - d_edges[starts[a]]:d_edges[k + 1] - d_edges[starts[a]]] = False
                k = child_joint.get(int(jpar[k])) if jpar[k] >= 0 else None
        assert not zero[:6 * nja, :nda].all() or nda == 0 or nja == 1
        if not np.all(J[a][zero] == 0.0):
            return False
        if not (np.all(H[a, nda:, :] == 0.0) and np.all(H[a, :, nda:] == 0.0)):
            return False
    return bool(np.array_equal(H, np.swapaxes(H, 1, 2)))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the reference against eval_fk_numpy and against closed forms
# ---------------------------------------------------------------------------------------------------------------------------------
def _link_identity_error(model, ref, bq, jqd, bqd):
    """max over links of |(v + w x c, w) - body_qd| / max(1, R), (v, w) = J_l qd."""
    bq, bqd = np.asarray(bq, dtype=np.float64).reshape(-1, 7), np.asarray(bqd, dtype=np.float64).reshape(-1, 6)
    com = np.asarray(model.body_com, dtype=np.float64).reshape(-1, 3)
    d_edges = np.concatenate([np.asarray(model.joint_qd_start), [model.joint_dof_count]])
    starts, ends, jch = np.asarray(model.articulation_start), np.asarray(model.articulation_end), np.asarray(model.joint_child)
    worst = 0.0
    for a in range(len(starts)):
        qd = np.zeros(ref.D)
        nda = d_edges[ends[a]] - d_edges[starts[a]]
        qd[:nda] = np.asarray(jqd, dtype=np.float64)[d_edges[starts[a]]:d_edges[ends[a]]]
        for i, j in enumerate(range(int(starts[a]), int(ends[a]))):
            b = int(jch[j])
            vw = ref.J[a, 6 * i:6 * i + 6] @ qd
            c = bq[b, :3] + _R(bq[b, 3:]) @ com[b]
            got = np.concatenate([vw[:3] + np.cross(vw[3:], c), vw[3:]])
            worst = max(worst, np.abs(got - bqd[b]).max() / max(1.0, ref.R[a]))
    return worst


@pytest.mark.parametrize("name", sorted(SCENES))
def test_reference_columns_match_eval_fk_with_unit_velocities(name):
    model = SCENES[name](3)
    jq, _ = random_joint_state(model, 13)
    bq, _ = eval_fk_numpy(model, jq, np.zeros(model.joint_dof_count, np.float32))
    ref = jacobian_reference(model, bq, jq)
    nd, worst = model.env.nd, 0.0
    for d in range(nd):  # dof d of every world at unit rate
        jqd = np.zeros((3, nd), np.float32)
        jqd[:, d] = 1.0
        bq2, bqd = eval_fk_numpy(model, jq, jqd.reshape(-1))
        assert np.array_equal(bq2, bq)
        worst = max(worst, _link_identity_error(model, ref, bq, jqd.reshape(-1), bqd))
    print(f"[eval_jacobian reference] {name}: {nd} columns, identity err / max(1, R) {worst:.3e}")
    assert worst <= 1e-6  # eval_fk_numpy computes in float64 and rounds body_qd to fp32: 6e-8 of an O(R) value


def kinetic_energy(model, bq, bqd):
    """Per articulation: sum over its links of m |v_com|^2 / 2 + w^T R I R^T w / 2."""
    bq, bqd = np.asarray(bq, dtype=np.float64).reshape(-1, 7), np.asarray(bqd, dtype=np.float64).reshape(-1, 6)
    mass = np.asarray(model.body_mass, dtype=np.float64).reshape(-1)
    Ib = np.asarray(model.body_inertia, dtype=np.float64).reshape(-1, 3, 3)
    starts, ends, jch = np.asarray(model.articulation_start), np.asarray(model.articulation_end), np.asarray(model.joint_child)
    ke = np.zeros(len(starts))
    for a in range(len(starts)):
        for j in range(int(starts[a]), int(ends[a])):
            b = int(jch[j])
            Rb = _R(bq[b, 3:])
            ke[a] += 0.5 * mass[b] * bqd[b, :3] @ bqd[b, :3] + 0.5 * bqd[b, 3:] @ (Rb @ Ib[b] @ Rb.T) @ bqd[b, 3:]
    return ke


def energy_error(model, H, jqd, ke):
    """max over articulations of |qd^T H qd / 2 - ke| / ke."""
    d_edges = np.concatenate([np.asarray(model.joint_qd_start), [model.joint_dof_count]])
    starts, ends = np.asarray(model.articulation_start), np.asarray(model.articulation_end)
    H, jqd = np.asarray(H, dtype=np.float64), np.asarray(jqd, dtype=np.float64)
    worst = 0.0
    for a in range(len(starts)):
        qd = jqd[d_edges[starts[a]]:d_edges[ends[a]]]
        worst = max(worst, abs(0.5 * qd @ H[a, :len(qd), :len(qd)] @ qd - ke[a]) / ke[a])
    return worst


@pytest.mark.parametrize("name", sorted(SCENES))
def test_reference_mass_matrix_gives_the_kinetic_energy(name):
    model, jq, jqd, bq, bqd = fk_case(name, 5, 17)
    ref = reference(model, bq, jq)
    err = energy_error(model, ref.H, jqd, kinetic_energy(model, bq, bqd))
    print(f"[eval_mass_matrix reference] {name}: kinetic energy rel err {err:.3e}")
    assert err <= 1e-5  # body_qd is fp32: 6e-8 relative per term, squared and summed over a dozen links
    assert np.allclose(ref.H, np.swapaxes(ref.H, 1, 2), rtol=0, atol=1e-12 * np.abs(ref.H).max())
    assert all(np.linalg.eigvalsh(h[:n, :n]).min() > 0.0 for h, n in zip(ref.H, _art_dofs(model)))


def _art_dofs(model):
    d_edges = np.concatenate([np.asarray(model.joint_qd_start), [model.joint_dof_count]])
    return d_edges[np.asarray(model.articulation_end)] - d_edges[np.asarray(model.articulation_start)]


def planar_pendulum(links, device=None, worlds=1):
    """`links` box links in a chain, revolute about y, COM at the link origin, l_c = 0.3 from the joint, the next joint 0.5 along."""
    env = nt.ModelBuilder()
    cfg = nt.ModelBuilder.ShapeConfig(has_shape_collision=False)
    joints, prev = [], -1
    for k in range(links):
        b = env.add_link(xform=[0.3 + 0.5 * k, 0.0, 2.0, 0, 0, 0, 1])
        env.add_shape_box(b, hx=0.3, hy=0.04, hz=0.05 + 0.01 * k, cfg=cfg)
        joints.append(env.add_joint_revolute(prev, b, axis=[0.0, 1.0, 0.0], parent_xform=nm.transform([0.0, 0.0, 2.0] if k == 0 else [0.2, 0.0, 0.0]),
                                             child_xform=nm.transform([-0.3, 0.0, 0.0])))
        prev = b
    env.add_articulation(joints)
    scene = nt.ModelBuilder()
    scene.replicate(env, worlds)
    return scene.finalize(device=device)


def pendulum_closed_form(model, q):
    """Textbook H of the planar single / double pendulum above (angles q, both about y)."""
    m = np.asarray(model.body_mass, dtype=np.float64)
    Iyy = np.asarray(model.body_inertia, dtype=np.float64).reshape(-1, 3, 3)[:, 1, 1]
    lc, l1 = 0.3, 0.5
    if len(q) == 1:
        return np.array([[Iyy[0] + m[0] * lc * lc]])
    c2 = np.cos(q[1])
    h22 = Iyy[1] + m[1] * lc * lc
    h12 = h22 + m[1] * l1 * lc * c2
    return np.array([[Iyy[0] + m[0] * lc * lc + Iyy[1] + m[1] * (l1 * l1 + lc * lc + 2 * l1 * lc * c2), h12], [h12, h22]])


@pytest.mark.parametrize("links", [1, 2])
def test_reference_mass_matrix_matches_pendulum_closed_forms(links):
    model = planar_pendulum(links)
    assert np.allclose(np.asarray(model.body_com), 0.0)
    jq = np.array([0.7, -1.1][:links], np.float32)
    bq, _ = eval_fk_numpy(model, jq, np.zeros(links, np.float32))
    ref = reference(model, bq, jq)
    want = pendulum_closed_form(model, jq.astype(np.float64))
    assert np.abs(ref.H[0] - want).max() <= 1e-6 * np.abs(want).max()  # (body_q is fp32)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the numpy paths
# ---------------------------------------------------------------------------------------------------------------------------------
def _host_state(model, bq, bqd, jq, jqd):
    s = model.state()
    s.body_q, s.body_qd, s.joint_q, s.joint_qd = bq, bqd, jq, jqd
    return s


@pytest.mark.parametrize("name", sorted(SCENES))
def test_numpy_paths_match_reference(name):
    model, jq, jqd, bq, bqd = fk_case(name, 7, 5)
    ref = reference(model, bq, jq)
    s = _host_state(model, bq, bqd, jq, jqd)
    S = np.full((model.joint_dof_count, 6), POISON, np.float32)
    I = np.full((model.body_count, 6, 6), POISON, np.float32)  # noqa: E741
    J = nt.eval_jacobian(model, s, joint_S_s=S)
    H = nt.eval_mass_matrix(model, s, body_I_s=I)
    assert J.dtype == np.float32 and H.dtype == np.float32
    assert J.shape == (model.articulation_count, 6 * model.max_joints_per_articulation, model.max_dofs_per_articulation)
    assert H.shape == (model.articulation_count, model.max_dofs_per_articulation, model.max_dofs_per_articulation)
    assert model.max_dofs_per_articulation == model.env.max_art_dofs == ref.D and model.max_joints_per_articulation == ref.L
    errs = jm_errors(model, ref, J, H, S, I)
    print(f"[eval_jacobian numpy] {name}: error / gate scale {errs}")
    assert within_gates(errs), errs
    assert structure_ok(model, ref, J, H)
    err = energy_error(model, H, jqd, kinetic_energy(model, bq, bqd))
    assert err <= 1e-5, err
    # eval_mass_matrix(J=..., joint_S_s=...) fills them through eval_jacobian
    J2, S2 = np.full_like(J, POISON), np.full_like(S, POISON)
    H2 = nt.eval_mass_matrix(model, s, J=J2, joint_S_s=S2)
    assert np.array_equal(J2, J) and np.array_equal(S2, S) and np.array_equal(H2, H)


def test_outputs_into_caller_arrays_and_poisoned_padding():
    model, jq, jqd, bq, bqd = fk_case("multi_art", 4, 2)
    s = _host_state(model, bq, bqd, jq, jqd)
    J, H = nt.eval_jacobian(model, s), nt.eval_mass_matrix(model, s)
    J2, H2 = np.full_like(J, POISON), np.full_like(H, POISON)
    assert nt.eval_jacobian(model, s, J2) is J2 and nt.eval_mass_matrix(model, s, H2) is H2
    assert np.array_equal(J2, J) and np.array_equal(H2, H)  # padding and non-ancestor entries are written (zero) on every call
    assert model.env.na == 3 and J.shape == (12, 12, 6) and np.all(J[0, 6:] == 0.0) and np.all(J[2, :, 2:] == 0.0)
    with pytest.raises(ValueError, match="J must be a float32 numpy array of shape"):
        nt.eval_jacobian(model, s, np.zeros((12, 12, 5), np.float32))


def _hetero_case():
    from test_heterogeneous_worlds import mixed_model

    model = mixed_model((("quadruped", 2), ("boxes3", 1), ("pendulum", 2), ("quadruped", 1)))
    assert model.is_heterogeneous
    states = [random_joint_state(p, 2 + i) for i, p in enumerate(model.world_groups.parts)]
    jq, jqd = np.concatenate([a for a, _ in states]), np.concatenate([b for _, b in states])
    bq, bqd = eval_fk_numpy(model, jq, jqd)
    return model, jq, jqd, bq, bqd


def test_heterogeneous_model():
    model, jq, jqd, bq, bqd = _hetero_case()
    ref = reference(model, bq, jq)
    assert (ref.L, ref.D) == (model.max_joints_per_articulation, model.max_dofs_per_articulation) == (13, 18)
    S = np.zeros((model.joint_dof_count, 6), np.float32)
    I = np.zeros((model.body_count, 6, 6), np.float32)  # noqa: E741
    J = eval_jacobian_numpy(model, bq, jq, None, S)
    H = eval_mass_matrix_numpy(model, bq, jq, None, I)
    errs = jm_errors(model, ref, J, H, S, I)
    print(f"[eval_jacobian numpy] heterogeneous: error / gate scale {errs}")
    assert within_gates(errs), errs
    assert structure_ok(model, ref, J, H)
    # selection over the global articulation ids into poisoned outputs
    sel = np.arange(model.articulation_count) % 2 == 0
    s = model.state()
    s.body_q, s.body_qd, s.joint_q, s.joint_qd = bq, bqd, jq, jqd
    Jm, Hm = np.full_like(J, POISON), np.full_like(H, POISON)
    nt.eval_jacobian(model, s, Jm, mask=sel)
    nt.eval_mass_matrix(model, s, Hm, mask=sel)
    assert np.array_equal(Jm[sel], J[sel]) and np.all(Jm[~sel] == POISON)
    assert np.array_equal(Hm[sel], H[sel]) and np.all(Hm[~sel] == POISON)


def test_mask_leaves_unselected_slices_untouched_bit_for_bit():
    model, jq, jqd, bq, bqd = fk_case("multi_art", 6, 4)
    s = _host_state(model, bq, bqd, jq, jqd)
    S, I = np.zeros((model.joint_dof_count, 6), np.float32), np.zeros((model.body_count, 6, 6), np.float32)  # noqa: E741
    J, H = nt.eval_jacobian(model, s, joint_S_s=S), nt.eval_mass_matrix(model, s, body_I_s=I)
    sel = np.random.default_rng(3).random(model.articulation_count) < 0.5
    assert sel.any() and not sel.all()
    Jm, Hm, Sm, Im = (np.full_like(x, POISON) for x in (J, H, S, I))
    nt.eval_jacobian(model, s, Jm, Sm, mask=sel)
    nt.eval_mass_matrix(model, s, Hm, body_I_s=Im, mask=sel)
    assert np.array_equal(Jm[sel], J[sel]) and np.all(Jm[~sel] == POISON)
    assert np.array_equal(Hm[sel], H[sel]) and np.all(Hm[~sel] == POISON)
    d_edges = np.concatenate([np.asarray(model.joint_qd_start), [model.joint_dof_count]])
    dsel = np.concatenate([np.full(d_edges[e] - d_edges[b], sel[a]) for a, (b, e) in enumerate(zip(model.articulation_start, model.articulation_end))])
    bsel = np.zeros(model.body_count, dtype=bool)
    bsel[np.asarray(model.joint_child)] = np.repeat(sel, np.asarray(model.articulation_end) - np.asarray(model.articulation_start))
    assert np.array_equal(Sm[dsel], S[dsel]) and np.all(Sm[~dsel] == POISON)
    assert np.array_equal(Im[bsel], I[bsel]) and np.all(Im[~bsel] == POISON)
    with pytest.raises(ValueError, match="mask has 3 entries"):
        nt.eval_jacobian(model, s, mask=[True, False, True])


def test_articulation_view_world_mask():
    model, jq, jqd, bq, bqd = fk_case("multi_art", 4, 8)
    s = _host_state(model, bq, bqd, jq, jqd)
    labels = list(model.articulation_label)[:3]
    view = nt.selection.ArticulationView(model, str(labels[2]))  # the pendulum: third articulation of every world
    Jv, Hv = view.eval_jacobian(s), view.eval_mass_matrix(s)
    J, H = nt.eval_jacobian(model, s), nt.eval_mass_matrix(model, s)
    assert Jv.shape == (4, 12, 6) and Hv.shape == (4, 6, 6)
    assert np.array_equal(Jv, J.reshape(4, 3, 12, 6)[:, 2]) and np.array_equal(Hv, H.reshape(4, 3, 6, 6)[:, 2])
    Jm, Hm = np.full_like(J, POISON), np.full_like(H, POISON)
    got_J = view.eval_jacobian(s, Jm, mask=[True, False, True, False])
    got_H = view.eval_mass_matrix(s, Hm, mask=[True, False, True, False])
    assert np.array_equal(got_J[[0, 2]], Jv[[0, 2]]) and np.all(got_J[[1, 3]] == POISON)
    assert np.array_equal(got_H[[0, 2]], Hv[[0, 2]]) and np.all(got_H[[1, 3]] == POISON)
    assert np.all(Jm.reshape(4, 3, 12, 6)[[1, 3]] == POISON)  # every articulation of an unselected world
    with pytest.raises(ValueError, match="one entry per world"):
        view.eval_jacobian(s, mask=[True, False])


def test_model_without_articulations_is_refused():
    env = nt.ModelBuilder()
    b = env.add_link(xform=[0.0, 0.0, 1.0, 0, 0, 0, 1])
    env.add_shape_box(b, hx=0.1, hy=0.05, hz=0.05)
    env.add_joint_revolute(-1, b, axis=[0.0, 1.0, 0.0])
    model = env.finalize()
    assert model.max_joints_per_articulation == 0 and model.max_dofs_per_articulation == 0
    with pytest.raises(NotImplementedError, match="needs articulations"):
        nt.eval_jacobian(model, model.state())


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the C ABI: header vs ctypes table, argument errors
# ---------------------------------------------------------------------------------------------------------------------------------
def _declaration(name):
    text = open(HEADER).read()
    m = re.search(r"nt_status\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/newton_hip_kinematics.h"
    return [" ".join(re.sub(r"/\*.*?\*/", "", a).split()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("name,out,aux", [("nt_eval_jacobian", "J", "joint_S_s"), ("nt_eval_mass_matrix", "H", "body_I_s")])
def test_header_and_ctypes_table_agree(name, out, aux):
    args = _declaration(name)
    assert args == ["const nt_model* m", "const nt_state* in", f"float* {out}", f"float* {aux}", "const uint8_t* art_mask", "void* stream"]
    restype, argtypes = _lib.SYMBOLS[name]
    assert restype is C.c_int32
    assert argtypes == [C.POINTER(_lib.nt_model), C.POINTER(_lib.nt_state), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert _declaration(name + "_tile") == args[:5] + ["int32_t envs_per_block", "void* stream"]
    assert _lib.SYMBOLS[name + "_tile"] == (C.c_int32, argtypes[:5] + [C.c_int32, C.c_void_p])
    assert re.search(r"^ \*\s+" + name + r"\s+<-", open(HEADER).read(), re.M)  # the entry-point table
    import __graft_entry__ as g

    assert not any("newton_hip_kinematics.h" in d for d in g.UNITS["nt_kernels.hip"])  # the headline unit keeps its id


@pytest.mark.parametrize("name", ["nt_eval_jacobian", "nt_eval_mass_matrix"])
def test_argument_errors(name):
    """Null pointers NT_ERR_INVALID_ARG (-1); no joints / no articulations NT_ERR_UNSUPPORTED (-3): decided before any launch, so the
    compiled library answers without a device."""
    lib = _lib.load()
    fn, tile = getattr(lib, name), getattr(lib, name + "_tile")
    m, s = _lib.nt_model(), _lib.nt_state()
    m.env_count, m.env_stride, m.nb, m.nj, m.cpp, m.na, m.max_art_dofs = 4, 64, 2, 1, 4, 1, 1
    buf = (C.c_float * 16)()
    ptr = C.cast(buf, C.c_void_p)
    m.art_start = ptr
    s.body_q, s.joint_q = ptr, ptr
    ok = (C.byref(m), C.byref(s), ptr, None, None, None)
    assert fn(None, *ok[1:]) == -1
    assert fn(ok[0], None, *ok[2:]) == -1
    assert fn(ok[0], ok[1], None, None, None, None) == -1
    for missing in ("body_q", "joint_q"):
        s2 = _lib.nt_state()
        s2.body_q, s2.joint_q = ptr, ptr
        setattr(s2, missing, None)
        assert fn(ok[0], C.byref(s2), *ok[2:]) == -1
    m.nj = 0
    assert fn(*ok) == -3 and tile(*ok[:5], 0, None) == -3
    m.nj, m.na = 1, 0
    assert fn(*ok) == -3 and tile(*ok[:5], 16, None) == -3
