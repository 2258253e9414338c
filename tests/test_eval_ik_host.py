"""newton_amd.eval_ik on the host: a float64 reference of the contract (include/newton_hip_kinematics.h), validated by round trip
through eval_fk_numpy; eval_ik_numpy against it; selection; the C header against the ctypes table.

The reference, the scenes, the random inputs and the gates below are shared with tests/test_eval_ik_emu.py and
tests/test_gpu_eval_ik.py.  Gates: coordinates 1e-5 absolute (eval_fk's fp32-rounded output perturbs O(1) quantities by 6e-8 through a
short chain); rates 1e-5 * max(1, V), V the larger body-velocity magnitude of the joint's two bodies (a rate is a difference of terms
of that size)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import newton_amd as nt
from newton_amd import _lib
from newton_amd import _np_math as nm
from newton_amd.articulation import eval_fk_numpy, eval_ik_numpy
from scenes import free_child_scene, joint_zoo_scene, pendulum_scene, quadruped_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "newton_hip_kinematics.h")
JT = nt.JointType
Q_GATE, QD_GATE = 1e-5, 1e-5


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 reference of the contract (one joint at a time, all worlds at once)
# ---------------------------------------------------------------------------------------------------------------------------------
def _qm(a, b):
    av, aw, bv, bw = a[:, :3], a[:, 3:], b[:, :3], b[:, 3:]
    return np.concatenate([aw * bv + bw * av + np.cross(av, bv), aw * bw - np.sum(av * bv, axis=1, keepdims=True)], axis=1)


def _qc(q):
    return q * np.array([-1.0, -1.0, -1.0, 1.0])


def _rot(q, v):
    qv = np.concatenate([v, np.zeros((len(v), 1))], axis=1)
    return _qm(_qm(q, qv), _qc(q))[:, :3]


def _aa(axis, angle):
    return np.concatenate([axis * np.sin(0.5 * angle)[:, None], np.cos(0.5 * angle)[:, None]], axis=1)


def _wrap(a):
    return np.pi - np.mod(np.pi - a, 2.0 * np.pi)  # (-pi, pi]


def ik_reference(model, body_q, body_qd):
    """(joint_q, joint_qd, written_q, written_qd) in float64: the coordinates of every joint, and which entries the call writes."""
    t = model.env
    E, nb, nj = t.env_count, t.nb, t.nj
    bq = np.asarray(body_q, dtype=np.float64).reshape(E, nb, 7)
    bqd = np.asarray(body_qd, dtype=np.float64).reshape(E, nb, 6)
    com = np.asarray(model.body_com, dtype=np.float64).reshape(E, nb, 3)
    X_p = np.asarray(model.joint_X_p, dtype=np.float64).reshape(E, nj, 7)
    X_c = np.asarray(model.joint_X_c, dtype=np.float64).reshape(E, nj, 7)
    axes = np.asarray(model.joint_axis, dtype=np.float64).reshape(E, t.nd, 3)
    jq, jqd = np.zeros((E, t.nc)), np.zeros((E, t.nd))
    wq, wqd = np.zeros(t.nc, dtype=bool), np.zeros(t.nd, dtype=bool)
    dot = lambda a, b: np.sum(a * b, axis=1)  # noqa: E731
    for j in range(nj):
        jt, p, c = int(t.joint_type[j]), int(t.joint_parent[j]), int(t.joint_child[j])
        qs, ds, lin, ang = int(t.joint_q_start[j]), int(t.joint_qd_start[j]), int(t.joint_lin_count[j]), int(t.joint_ang_count[j])
        if jt == JT.FIXED:
            continue
        p_wpj, q_wpj = X_p[:, j, :3], X_p[:, j, 3:]
        w_p, v_par = np.zeros((E, 3)), np.zeros((E, 3))
        if p >= 0:
            p_wpj, q_wpj = bq[:, p, :3] + _rot(bq[:, p, 3:], p_wpj), _qm(bq[:, p, 3:], q_wpj)
            w_p = bqd[:, p, 3:]
            v_par = bqd[:, p, :3] + np.cross(w_p, bq[:, c, :3] - (bq[:, p, :3] + _rot(bq[:, p, 3:], com[:, p])))
        x_c, q_c = bq[:, c, :3], bq[:, c, 3:]
        p_wcj, q_wcj = x_c + _rot(q_c, X_c[:, j, :3]), _qm(q_c, X_c[:, j, 3:])
        x_j, q_j = _rot(_qc(q_wpj), p_wcj - p_wpj), _qm(_qc(q_wpj), q_wcj)
        w_o, com_w = bqd[:, c, 3:], _rot(q_c, com[:, c])
        v_o = bqd[:, c, :3] - np.cross(w_o, com_w)
        ang_w, lin_o = w_o - w_p, v_o - v_par
        lin_w = lin_o + np.cross(ang_w, com_w) if jt in (JT.FREE, JT.DISTANCE) else lin_o - np.cross(ang_w, x_c - p_wcj)
        v_lin, v_ang = _rot(_qc(q_wpj), lin_w), _rot(_qc(q_wpj), ang_w)
        twist = lambda ax: _wrap(2.0 * np.arctan2(dot(ax, q_j[:, :3]), q_j[:, 3]))  # noqa: E731
        if jt == JT.PRISMATIC:
            q, qd = [dot(axes[:, ds], x_j)], [dot(axes[:, ds], v_lin)]
        elif jt == JT.REVOLUTE:
            q, qd = [twist(axes[:, ds])], [dot(axes[:, ds], v_ang)]
        elif jt == JT.BALL:
            q, qd = list(q_j.T), list(v_ang.T)
        elif jt in (JT.FREE, JT.DISTANCE):
            q, qd = list(x_j.T) + list(q_j.T), list(v_lin.T) + list(v_ang.T)
        else:
            assert jt == JT.D6
            q = [dot(axes[:, ds + k], x_j) for k in range(lin)]
            qd = [dot(axes[:, ds + k], v_lin) for k in range(lin)]
            e = [axes[:, ds + lin + k] for k in range(ang)]
            if ang == 1:
                q.append(twist(e[0]))
                qd.append(dot(e[0], v_ang))
            elif ang >= 2:
                # M = B^T R(q_j) B with B = [e0 e1 e2]: R_x(s t0) R_y(s t1) R_z(s t2), s = det B
                B = np.stack([e[0], e[1], e[2] if ang == 3 else np.cross(e[0], e[1])], axis=2)  # [E, row, col]
                Rcols = np.stack([_rot(q_j, B[:, :, k]) for k in range(3)], axis=2)
                M = np.einsum("eki,ekj->eij", B, Rcols)
                s = np.sign(np.linalg.det(B))
                if ang == 2:
                    th = [np.arctan2(M[:, 2, 1], M[:, 1, 1]), np.arctan2(M[:, 0, 2], M[:, 0, 0])]
                else:
                    th = [s * np.arctan2(-M[:, 1, 2], M[:, 2, 2]), s * np.arctan2(M[:, 0, 2], np.hypot(M[:, 0, 0], M[:, 0, 1])),
                          s * np.arctan2(-M[:, 0, 1], M[:, 0, 0])]
                q += th
                # rates over eval_fk's rotated axes a_k (least squares = the exact solve for a consistent v_ang)
                a = [e[0], _rot(_aa(e[0], th[0]), e[1])]
                if ang == 3:
                    a.append(_rot(_qm(_aa(a[1], th[1]), _aa(e[0], th[0])), e[2]))
                A = np.stack(a, axis=2)
                qd += list(np.stack([np.linalg.lstsq(A[i], v_ang[i], rcond=None)[0] for i in range(E)]).T)
        for k, v in enumerate(q):
            jq[:, qs + k], wq[qs + k] = v, True
        for k, v in enumerate(qd):
            jqd[:, ds + k], wqd[ds + k] = v, True
    return jq.reshape(-1), jqd.reshape(-1), np.tile(wq, E), np.tile(wqd, E)


def rate_scale(model, body_qd):
    """Per dof: max(1, V), V the larger of the linear / angular speeds of the joint's two bodies."""
    t = model.env
    E = t.env_count
    bqd = np.asarray(body_qd, dtype=np.float64).reshape(E, t.nb, 6)
    speed = np.maximum(np.linalg.norm(bqd[:, :, :3], axis=2), np.linalg.norm(bqd[:, :, 3:], axis=2))
    out = np.ones((E, t.nd))
    edges = np.concatenate([t.joint_qd_start, [t.nd]])
    for j in range(t.nj):
        v = speed[:, int(t.joint_child[j])]
        if t.joint_parent[j] >= 0:
            v = np.maximum(v, speed[:, int(t.joint_parent[j])])
        out[:, edges[j]:edges[j + 1]] = np.maximum(1.0, v)[:, None]
    return out.reshape(-1)


def ik_errors(model, got_q, got_qd, ref_q, ref_qd, body_qd):
    """(max coordinate error, max rate error over its scale); quaternion coordinates are compared up to sign."""
    t = model.env
    E = t.env_count
    g, r = np.asarray(got_q, dtype=np.float64).reshape(E, t.nc).copy(), np.asarray(ref_q, dtype=np.float64).reshape(E, t.nc)
    for j in range(t.nj):
        jt, qs = int(t.joint_type[j]), int(t.joint_q_start[j])
        o = qs + 3 if jt in (JT.FREE, JT.DISTANCE) else qs if jt == JT.BALL else -1
        if o >= 0:
            g[:, o:o + 4] *= np.where(np.sum(g[:, o:o + 4] * r[:, o:o + 4], axis=1, keepdims=True) < 0.0, -1.0, 1.0)
    eq = float(np.abs(g - r).max()) if t.nc else 0.0
    eqd = float((np.abs(np.asarray(got_qd, dtype=np.float64) - ref_qd) / rate_scale(model, body_qd)).max()) if t.nd else 0.0
    return eq, eqd


def within_gates(errors):
    eq, eqd = errors
    return eq <= Q_GATE and eqd <= QD_GATE


# ---------------------------------------------------------------------------------------------------------------------------------
# scenes and inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def d6_zoo_scene(world_count, device=None):
    """world -revolute-> 0 -prismatic-> 1 -ball-> 2 -fixed-> 3 -D6(1 lin, 1 ang)-> 4 -D6(2 ang)-> 5 -D6(2 lin, 3 ang, left-handed
    triple)-> 6 -D6(3 ang, tilted right-handed triple)-> 7; off-centre COMs, anchors rotated and off the axes on both sides."""
    env = nt.ModelBuilder()
    cfg = nt.ModelBuilder.ShapeConfig(has_shape_collision=False)
    links = []
    for k in range(8):
        b = env.add_link(xform=[0.3 * k, 0.05 * (k % 3), 1.0 + 0.02 * k, 0.0, 0.0, 0.0, 1.0])
        env.add_shape_box(b, xform=nm.transform([0.02 * (k - 3), 0.015, -0.01 * k]), hx=0.12, hy=0.05 + 0.01 * k, hz=0.04, cfg=cfg)
        links.append(b)
    X = lambda p, rpy=(0.0, 0.0, 0.0): nm.transform(p, nm.quat_rpy(*rpy))  # noqa: E731
    D = nt.ModelBuilder.JointDofConfig
    tilt = nm.quat_rpy(0.3, -0.5, 0.7)
    tri = [nm.quat_rotate(tilt, np.eye(3)[k]) for k in range(3)]
    joints = [
        env.add_joint_revolute(-1, links[0], axis=[0.0, 1.0, 0.0], parent_xform=X([0.0, 0.1, 1.0], (0.2, 0.1, -0.3)),
                               child_xform=X([-0.15, 0.02, 0.01], (0.0, 0.3, 0.1))),
        env.add_joint_prismatic(links[0], links[1], axis=[0.6, 0.0, 0.8], parent_xform=X([0.15, 0.0, 0.03], (0.1, 0.0, 0.2)),
                                child_xform=X([-0.15, 0.01, 0.0])),
        env.add_joint_ball(links[1], links[2], parent_xform=X([0.15, 0.02, 0.0], (0.0, 0.2, 0.0)), child_xform=X([-0.15, 0.0, 0.02])),
        env.add_joint_fixed(links[2], links[3], parent_xform=X([0.15, 0.0, 0.0], (0.1, 0.0, 0.2)), child_xform=X([-0.15, 0.0, 0.0])),
        env.add_joint_d6(links[3], links[4], linear_axes=[D(axis=0)], angular_axes=[D(axis=2)],
                         parent_xform=X([0.15, 0.0, 0.01], (0.0, -0.1, 0.3)), child_xform=X([-0.15, 0.03, 0.0])),
        env.add_joint_d6(links[4], links[5], angular_axes=[D(axis=1), D(axis=2)],
                         parent_xform=X([0.15, 0.01, 0.0], (0.2, 0.0, 0.0)), child_xform=X([-0.15, 0.0, 0.02], (0.0, 0.1, 0.1))),
        env.add_joint_d6(links[5], links[6], linear_axes=[D(axis=1), D(axis=2)], angular_axes=[D(axis=0), D(axis=2), D(axis=1)],
                         parent_xform=X([0.15, 0.0, 0.0], (0.0, 0.2, -0.1)), child_xform=X([-0.15, 0.02, 0.0])),
        env.add_joint_d6(links[6], links[7], angular_axes=[D(axis=tri[0]), D(axis=tri[1]), D(axis=tri[2])],
                         parent_xform=X([0.15, 0.0, 0.02]), child_xform=X([-0.15, 0.0, 0.0], (0.3, 0.0, 0.0))),
    ]
    env.add_articulation(joints)
    scene = nt.ModelBuilder()
    scene.replicate(env, world_count)
    return scene.finalize(device=device)


def random_joint_state(model, seed):
    """Angles uniform in +-3 rad (the middle angle of a three-axis D6 within +-1.2), linear coordinates +-0.3 about the model's, unit
    random quaternions, qd ~ N(0, 1)."""
    rng = np.random.default_rng(seed)
    t = model.env
    E = t.env_count
    jq = np.asarray(model.joint_q, dtype=np.float64).reshape(E, t.nc).copy()

    def quats():
        q = rng.normal(size=(E, 4))
        return q / np.linalg.norm(q, axis=1, keepdims=True)

    for j in range(t.nj):
        jt, qs, lin, ang = int(t.joint_type[j]), int(t.joint_q_start[j]), int(t.joint_lin_count[j]), int(t.joint_ang_count[j])
        if jt == JT.PRISMATIC:
            jq[:, qs] += rng.uniform(-0.3, 0.3, E)
        elif jt == JT.REVOLUTE:
            jq[:, qs] = rng.uniform(-3.0, 3.0, E)
        elif jt == JT.BALL:
            jq[:, qs:qs + 4] = quats()
        elif jt in (JT.FREE, JT.DISTANCE):
            jq[:, qs:qs + 3] += rng.uniform(-0.3, 0.3, (E, 3))
            jq[:, qs + 3:qs + 7] = quats()
        elif jt == JT.D6:
            jq[:, qs:qs + lin] += rng.uniform(-0.3, 0.3, (E, lin))
            jq[:, qs + lin:qs + lin + ang] = rng.uniform(-3.0, 3.0, (E, ang))
            if ang == 3:
                jq[:, qs + lin + 1] = rng.uniform(-1.2, 1.2, E)
    jqd = rng.normal(0.0, 1.0, size=(E * t.nd,))
    return jq.reshape(-1).astype(np.float32), jqd.astype(np.float32)


SCENES = {
    "d6_zoo": lambda E, device=None: d6_zoo_scene(E, device=device),
    "joint_zoo": lambda E, device=None: joint_zoo_scene(E, device=device, seed=None),
    "joint_zoo_free_root": lambda E, device=None: joint_zoo_scene(E, device=device, seed=None, free_root=True),
    "free_child": lambda E, device=None: free_child_scene(E, device=device, seed=None),
    "free_child_free_root": lambda E, device=None: free_child_scene(E, device=device, seed=None, free_root=True),
    "quadruped": lambda E, device=None: quadruped_scene(E, device=device),
    "pendulum": lambda E, device=None: pendulum_scene(E, device=device),
}


def fk_case(name, E, seed):
    """model, the random (joint_q, joint_qd) and eval_fk's fp32 body state for them."""
    model = SCENES[name](E)
    jq, jqd = random_joint_state(model, seed)
    bq, bqd = eval_fk_numpy(model, jq, jqd)
    return model, jq, jqd, bq, bqd


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the reference: ik(fk(q, qd)) == (q, qd)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENES))
def test_reference_inverts_eval_fk(name):
    model, jq, jqd, bq, bqd = fk_case(name, 9, 11)
    rq, rqd, wq, wqd = ik_reference(model, bq, bqd)
    t = model.env
    types = set(int(x) for x in t.joint_type)
    assert wq.all() and wqd.all()  # FIXED joints carry no coordinates: every entry belongs to a joint that writes
    eq, eqd = ik_errors(model, rq, rqd, jq.astype(np.float64), jqd.astype(np.float64), bqd)
    print(f"[eval_ik reference] {name}: types {sorted(types)} coord err {eq:.3e} rate err/scale {eqd:.3e}")
    assert eq <= Q_GATE and eqd <= QD_GATE


def test_scenes_cover_every_joint_type_the_builder_makes():
    seen, d6_ang = set(), set()
    for name in SCENES:
        t = SCENES[name](1).env
        seen |= set(int(x) for x in t.joint_type)
        d6_ang |= set(int(a) for a, ty in zip(t.joint_ang_count, t.joint_type) if ty == JT.D6)
    assert seen >= {int(JT.PRISMATIC), int(JT.REVOLUTE), int(JT.BALL), int(JT.FIXED), int(JT.FREE), int(JT.DISTANCE), int(JT.D6)}
    assert d6_ang >= {1, 2, 3}


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. eval_ik_numpy / nt.eval_ik on host models
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENES))
def test_eval_ik_numpy_matches_reference(name):
    model, _jq, _jqd, bq, bqd = fk_case(name, 7, 5)
    rq, rqd, _, _ = ik_reference(model, bq, bqd)
    gq, gqd = eval_ik_numpy(model, bq, bqd)
    assert gq.dtype == np.float32 and gqd.dtype == np.float32
    eq, eqd = ik_errors(model, gq, gqd, rq, rqd, bqd)
    print(f"[eval_ik_numpy] {name}: coord err {eq:.3e} rate err/scale {eqd:.3e}")
    assert eq <= Q_GATE and eqd <= QD_GATE


def test_eval_ik_numpy_heterogeneous_model():
    """Worlds that differ: eval_ik_numpy cuts the flat arrays per world group and concatenates world-major, selection included."""
    from test_heterogeneous_worlds import mixed_model

    model = mixed_model((("quadruped", 2), ("boxes3", 1), ("pendulum", 2), ("quadruped", 1)))
    assert model.is_heterogeneous
    parts = model.world_groups.parts
    states = [random_joint_state(p, 2 + i) for i, p in enumerate(parts)]
    jq, jqd = np.concatenate([a for a, _ in states]), np.concatenate([b for _, b in states])
    bq, bqd = eval_fk_numpy(model, jq, jqd)
    gq, gqd = eval_ik_numpy(model, bq, bqd)
    assert gq.shape == (model.joint_coord_count,) and gqd.shape == (model.joint_dof_count,)
    cut = lambda a, key, w: np.split(np.asarray(a).reshape(-1, w) if w > 1 else np.asarray(a),  # noqa: E731
                                     np.cumsum([getattr(p, key) for p in parts])[:-1])
    worst = [0.0, 0.0]
    for p, pbq, pbqd, pq, pqd in zip(parts, cut(bq, "body_count", 7), cut(bqd, "body_count", 6), cut(gq, "joint_coord_count", 1),
                                    cut(gqd, "joint_dof_count", 1)):
        rq, rqd, _, _ = ik_reference(p, pbq, pbqd)
        e = ik_errors(p, pq, pqd, rq, rqd, pbqd)
        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
    print(f"[eval_ik_numpy] heterogeneous: coord err {worst[0]:.3e} rate err/scale {worst[1]:.3e}")
    assert within_gates(worst), worst
    # selection over the global articulation ids; the given arrays supply what stays
    sel = np.arange(model.articulation_count) % 2 == 0
    fill_q, fill_qd = np.full(model.joint_coord_count, 7.0, np.float32), np.full(model.joint_dof_count, -7.0, np.float32)
    sq, sqd = eval_ik_numpy(model, bq, bqd, fill_q, fill_qd, art_sel=sel)
    art = np.asarray(model.joint_articulation)
    q_edges = np.concatenate([np.asarray(model.joint_q_start), [model.joint_coord_count]])
    d_edges = np.concatenate([np.asarray(model.joint_qd_start), [model.joint_dof_count]])
    on = [art[j] >= 0 and sel[art[j]] for j in range(len(art))]
    q_sel = np.concatenate([np.full(q_edges[j + 1] - q_edges[j], on[j]) for j in range(len(art))])
    d_sel = np.concatenate([np.full(d_edges[j + 1] - d_edges[j], on[j]) for j in range(len(art))])
    assert q_sel.any() and not q_sel.all()
    assert np.array_equal(sq[q_sel], gq[q_sel]) and np.all(sq[~q_sel] == 7.0)
    assert np.array_equal(sqd[d_sel], gqd[d_sel]) and np.all(sqd[~d_sel] == -7.0)


def _host_state(model, bq, bqd, fill):
    s = model.state()
    s.body_q, s.body_qd = bq, bqd
    s.joint_q = np.full(model.joint_coord_count, fill, dtype=np.float32)
    s.joint_qd = np.full(model.joint_dof_count, -fill, dtype=np.float32)
    return s


def test_eval_ik_in_place_and_into_arrays():
    model, _jq, _jqd, bq, bqd = fk_case("quadruped", 5, 3)
    rq, rqd, _, _ = ik_reference(model, bq, bqd)
    s = _host_state(model, bq, bqd, 7.0)
    nt.eval_ik(model, s)
    assert within_gates(ik_errors(model, s.joint_q, s.joint_qd, rq, rqd, bqd))
    assert np.array_equal(s.body_q, bq) and np.array_equal(s.body_qd, bqd)
    s2 = _host_state(model, bq, bqd, 7.0)
    out_q, out_qd = np.zeros(model.joint_coord_count, np.float32), np.zeros(model.joint_dof_count, np.float32)
    nt.eval_ik(model, s2, out_q, out_qd)
    assert np.array_equal(out_q, s.joint_q) and np.array_equal(out_qd, s.joint_qd)
    assert np.all(s2.joint_q == 7.0) and np.all(s2.joint_qd == -7.0)  # the state's own arrays stay as they were


def test_mask_and_indices_leave_unselected_entries_untouched_bit_for_bit():
    model, _jq, _jqd, bq, bqd = fk_case("free_child", 6, 4)
    full = _host_state(model, bq, bqd, 7.0)
    nt.eval_ik(model, full)
    sel = np.array([True, False, False, True, True, False])
    for kw in ({"mask": sel}, {"indices": np.flatnonzero(sel)}):
        s = _host_state(model, bq, bqd, 7.0)
        nt.eval_ik(model, s, **kw)
        q, qd = s.joint_q.reshape(6, -1), s.joint_qd.reshape(6, -1)
        assert np.array_equal(q[sel], full.joint_q.reshape(6, -1)[sel]) and np.array_equal(qd[sel], full.joint_qd.reshape(6, -1)[sel])
        assert np.all(q[~sel] == 7.0) and np.all(qd[~sel] == -7.0)
    with pytest.raises(ValueError, match="'mask' and 'indices' cannot be used together"):
        nt.eval_ik(model, full, mask=sel, indices=[0])
    with pytest.raises(ValueError, match="mask has 3 entries, the model has 6 articulations"):
        nt.eval_ik(model, full, mask=[True, False, True])


def test_articulation_view_world_mask():
    model, _jq, _jqd, bq, bqd = fk_case("quadruped", 4, 8)
    view = nt.selection.ArticulationView(model, "*")
    full = _host_state(model, bq, bqd, 7.0)
    view.eval_ik(full)
    s = _host_state(model, bq, bqd, 7.0)
    view.eval_ik(s, mask=[True, False, True, False])
    got, want = view.get_dof_positions(s), view.get_dof_positions(full)
    assert np.array_equal(got[[0, 2]], want[[0, 2]]) and np.all(got[[1, 3]] == 7.0)
    assert np.all(view.get_dof_velocities(s)[[1, 3]] == -7.0)
    with pytest.raises(ValueError, match="one entry per world"):
        view.eval_ik(s, mask=[True, False])


def test_fixed_joints_and_joints_outside_articulations():
    """FIXED joints write nothing; without a selection joints outside any articulation are evaluated, with one they are not."""
    env = nt.ModelBuilder()
    cfg = nt.ModelBuilder.ShapeConfig(has_shape_collision=False)
    a, b = env.add_link(xform=[0.0, 0.0, 1.0, 0, 0, 0, 1]), env.add_link(xform=[0.4, 0.0, 1.0, 0, 0, 0, 1])
    for link in (a, b):
        env.add_shape_box(link, hx=0.1, hy=0.05, hz=0.05, cfg=cfg)
    j0 = env.add_joint_revolute(-1, a, axis=[0.0, 1.0, 0.0], parent_xform=nm.transform([0.0, 0.0, 1.0]))
    env.add_joint_revolute(a, b, axis=[0.0, 0.0, 1.0], parent_xform=nm.transform([0.2, 0.0, 0.0]), child_xform=nm.transform([-0.2, 0.0, 0.0]))
    env.add_articulation([j0])  # the second joint belongs to no articulation
    scene = nt.ModelBuilder()
    scene.replicate(env, 3)
    model = scene.finalize()
    jq, jqd = random_joint_state(model, 1)
    # eval_fk skips joints outside articulations: pose the second body through a twin model whose articulation holds both joints
    env2 = nt.ModelBuilder()
    a2, b2 = env2.add_link(xform=[0.0, 0.0, 1.0, 0, 0, 0, 1]), env2.add_link(xform=[0.4, 0.0, 1.0, 0, 0, 0, 1])
    for link in (a2, b2):
        env2.add_shape_box(link, hx=0.1, hy=0.05, hz=0.05, cfg=cfg)
    k0 = env2.add_joint_revolute(-1, a2, axis=[0.0, 1.0, 0.0], parent_xform=nm.transform([0.0, 0.0, 1.0]))
    k1 = env2.add_joint_revolute(a2, b2, axis=[0.0, 0.0, 1.0], parent_xform=nm.transform([0.2, 0.0, 0.0]), child_xform=nm.transform([-0.2, 0.0, 0.0]))
    env2.add_articulation([k0, k1])
    scene2 = nt.ModelBuilder()
    scene2.replicate(env2, 3)
    bq, bqd = eval_fk_numpy(scene2.finalize(), jq, jqd)
    s = _host_state(model, bq, bqd, 7.0)
    nt.eval_ik(model, s)
    assert within_gates(ik_errors(model, s.joint_q, s.joint_qd, jq.astype(np.float64), jqd.astype(np.float64), bqd))
    s = _host_state(model, bq, bqd, 7.0)
    nt.eval_ik(model, s, mask=[True, True, True])
    q = s.joint_q.reshape(3, 2)
    assert np.abs(q[:, 0] - jq.reshape(3, 2)[:, 0]).max() <= Q_GATE and np.all(q[:, 1] == 7.0)


def test_non_orthogonal_multi_axis_d6_is_refused():
    env = nt.ModelBuilder()
    cfg = nt.ModelBuilder.ShapeConfig(has_shape_collision=False)
    a = env.add_link(xform=[0.0, 0.0, 1.0, 0, 0, 0, 1])
    env.add_shape_box(a, hx=0.1, hy=0.05, hz=0.05, cfg=cfg)
    D = nt.ModelBuilder.JointDofConfig
    j = env.add_joint_d6(-1, a, angular_axes=[D(axis=[1.0, 0.0, 0.0]), D(axis=[0.6, 0.8, 0.0])])
    env.add_articulation([j])
    model = env.finalize()
    with pytest.raises(NotImplementedError, match="not mutually orthogonal"):
        nt.eval_ik(model, model.state())


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the C ABI: header vs ctypes table, argument errors
# ---------------------------------------------------------------------------------------------------------------------------------
def _declaration(name):
    text = open(HEADER).read()
    m = re.search(r"nt_status\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/newton_hip_kinematics.h"
    return [" ".join(re.sub(r"/\*.*?\*/", "", a).split()) for a in m.group(1).split(",")]


def test_header_and_ctypes_table_agree_on_nt_eval_ik():
    args = _declaration("nt_eval_ik")
    assert args == ["const nt_model* m", "const nt_state* in", "float* joint_q", "float* joint_qd", "const uint8_t* art_mask", "void* stream"]
    restype, argtypes = _lib.SYMBOLS["nt_eval_ik"]
    assert restype is C.c_int32
    assert argtypes == [C.POINTER(_lib.nt_model), C.POINTER(_lib.nt_state), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    tile = _declaration("nt_eval_ik_tile")
    assert tile == args[:5] + ["int32_t envs_per_block", "void* stream"]
    assert _lib.SYMBOLS["nt_eval_ik_tile"] == (C.c_int32, argtypes[:5] + [C.c_int32, C.c_void_p])
    assert re.search(r"^ \*\s+nt_eval_ik\s+<-", open(HEADER).read(), re.M)  # the entry-point table at the top
    import __graft_entry__ as g

    assert "newton_hip_kinematics.h" in open(g.__file__).read()  # part of source_hash() and of the unit's dependencies
    assert any("newton_hip_kinematics.h" in d for d in g.UNITS["nt_featherstone.hip"])
    assert not any("newton_hip_kinematics.h" in d for d in g.UNITS["nt_kernels.hip"])  # the headline unit keeps its id


def test_argument_errors():
    """Null pointers NT_ERR_INVALID_ARG (-1), a model without joints NT_ERR_UNSUPPORTED (-3): decided before any launch, so the compiled
    library answers without a device."""
    lib = _lib.load()
    m, s = _lib.nt_model(), _lib.nt_state()
    m.env_count, m.env_stride, m.nb, m.nj, m.cpp = 4, 64, 2, 1, 4
    buf = (C.c_float * 16)()
    ptr = C.cast(buf, C.c_void_p)
    s.body_q, s.body_qd = ptr, ptr
    ok = (C.byref(m), C.byref(s), ptr, ptr, None, None)
    assert lib.nt_eval_ik(None, *ok[1:]) == -1
    assert lib.nt_eval_ik(ok[0], None, *ok[2:]) == -1
    assert lib.nt_eval_ik(ok[0], ok[1], None, *ok[3:]) == -1
    assert lib.nt_eval_ik(ok[0], ok[1], ok[2], None, None, None) == -1
    s2 = _lib.nt_state()
    s2.body_q = ptr
    assert lib.nt_eval_ik(ok[0], C.byref(s2), *ok[2:]) == -1
    m.nj = 0
    assert lib.nt_eval_ik(*ok) == -3
    assert lib.nt_eval_ik_tile(ok[0], ok[1], ok[2], ok[3], None, 0, None) == -3
