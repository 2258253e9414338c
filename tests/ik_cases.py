"""Shared construction of the IK test problems (tests/test_ik_solver_host.py, _emu.py, test_gpu_ik_solver.py): the target configuration
q* is drawn by random_joint_state and moved inside the joint limits, the targets are eval_fk(q*) in float64, the start is q* perturbed
by at most 0.2 per scalar coordinate and by a rotation of at most 0.2 rad per quaternion coordinate."""
import numpy as np

import newton_amd as nt
from newton_amd import ik
from newton_amd.articulation import _eval_fk_float64, _qmul, _qrot
from newton_amd.enums import MAXVAL
from test_eval_ik_host import random_joint_state
from test_eval_jacobian_host import SCENES

JT = nt.JointType
PERTURB = 0.2


def inside_limits(model, jq):
    """Limited PRISMATIC / REVOLUTE / D6 coordinates moved into the middle 80 % of [lower, upper]."""
    t = model.env
    E = t.env_count
    q = np.asarray(jq, dtype=np.float64).reshape(E, t.nc).copy()
    lo = np.asarray(model.joint_limit_lower, dtype=np.float64).reshape(E, t.nd)
    hi = np.asarray(model.joint_limit_upper, dtype=np.float64).reshape(E, t.nd)
    for j in range(t.nj):
        if int(t.joint_type[j]) not in (JT.PRISMATIC, JT.REVOLUTE, JT.D6):
            continue
        qs, ds = int(t.joint_q_start[j]), int(t.joint_qd_start[j])
        n = int(t.joint_lin_count[j] + t.joint_ang_count[j]) if int(t.joint_type[j]) == JT.D6 else 1
        for k in range(n):
            a, b = lo[:, ds + k], hi[:, ds + k]
            lim = (a < b) & (np.abs(a) < MAXVAL) & (np.abs(b) < MAXVAL)
            q[:, qs + k] = np.where(lim, np.clip(q[:, qs + k], a + 0.1 * (b - a), b - 0.1 * (b - a)), q[:, qs + k])
    return q


def perturbed(model, q, seed):
    rng = np.random.default_rng(seed)
    t = model.env
    E = t.env_count
    out = q.copy()

    def rotate(cols):
        v = rng.normal(size=(E, 3))
        v *= (rng.uniform(0.0, PERTURB, E) / np.linalg.norm(v, axis=1))[:, None]
        out[:, cols] = _qmul(ik._exp_quat(v), q[:, cols])

    for j in range(t.nj):
        jt, qs = int(t.joint_type[j]), int(t.joint_q_start[j])
        qe = int(t.joint_q_start[j + 1]) if j + 1 < t.nj else t.nc
        if jt == JT.BALL:
            rotate(slice(qs, qs + 4))
        elif jt in (JT.FREE, JT.DISTANCE):
            out[:, qs:qs + 3] += rng.uniform(-PERTURB, PERTURB, (E, 3))
            rotate(slice(qs + 3, qs + 7))
        else:
            out[:, qs:qe] += rng.uniform(-PERTURB, PERTURB, (E, qe - qs))
    return out


def link_pose(model, q, link, offset=None, offset_rotation=None):
    bq, _ = _eval_fk_float64(model, q, np.zeros(model.env.env_count * model.env.nd))
    X = bq[:, link]
    if offset is not None:
        return X[:, :3] + _qrot(X[:, 3:], np.asarray(offset, dtype=np.float64))
    return _qmul(X[:, 3:], np.asarray(offset_rotation, dtype=np.float64))


OFFSET = np.array([0.05, -0.02, 0.03], dtype=np.float32)
S, C_ = np.sin(0.15), np.cos(0.15)
OFFSET_ROT = np.array([S * 0.6, 0.0, S * 0.8, C_], dtype=np.float32)


LIMITED_SCENES = ("joint_zoo", "joint_zoo_free_root")


def violated_limit_rows(solver, q):
    """Per problem the number of non-zero joint-limit residual rows at q (float64 host evaluation)."""
    r, _ = solver.evaluate_numpy(q, jacobian=False)
    at, count = 0, np.zeros(len(r), dtype=np.int64)
    for o in solver.objectives:
        n = solver.model.env.nd if isinstance(o, ik.IKObjectiveJointLimit) else 3
        if isinstance(o, ik.IKObjectiveJointLimit):
            count += np.count_nonzero(r[:, at:at + n], axis=1)
        at += n
    return count


def objective_specs(name, model):
    """[(kind, link)] of the scene's objectives: the quadruped's four feet, base rotation and joint limits (its joints carry none: the
    rows are zero); one position per articulation of multi_art; position and rotation of the last link elsewhere, and on the scenes
    with finite limits (LIMITED_SCENES) the joint-limit objective, violated at the start."""
    t = model.env
    if name == "quadruped":
        leaves = [int(t.joint_child[j]) for j in range(t.nj) if not np.any(t.joint_parent == t.joint_child[j])]
        assert len(leaves) == 4
        root = int(t.joint_child[0])
        return [("position", b) for b in leaves] + [("rotation", root), ("limit", -1)]
    if name == "multi_art":
        return [("position", int(t.joint_child[int(t.art_start[k + 1]) - 1])) for k in range(t.na)]
    specs = [("position", t.nb - 1), ("rotation", t.nb - 1)]
    if name in LIMITED_SCENES:  # finite limits (-0.05 .. 0.1, -0.2 .. 0.4): narrower than the start's perturbation
        specs.append(("limit", -1))
    return specs


def targets_at(name, model, q, dtype):
    out = []
    for kind, link in objective_specs(name, model):
        if kind == "position":
            out.append(link_pose(model, q, link, offset=OFFSET).astype(dtype))
        elif kind == "rotation":
            out.append(link_pose(model, q, link, offset_rotation=OFFSET_ROT).astype(dtype))
        else:
            out.append(None)
    return out


def make_objectives(name, model, targets, weights=None):
    objs = []
    for i, ((kind, link), tg) in enumerate(zip(objective_specs(name, model), targets)):
        w = 1.0 if weights is None else weights[i]
        if kind == "position":
            objs.append(ik.IKObjectivePosition(link, OFFSET, tg, weight=w))
        elif kind == "rotation":
            objs.append(ik.IKObjectiveRotation(link, OFFSET_ROT, tg, weight=w))
        else:
            objs.append(ik.IKObjectiveJointLimit(weight=w))
    return objs


def ik_case(name, E, seed, device=None, dtype=np.float32):
    """model, q* [E, nc] (float64), the targets at q* in ``dtype``, the start [E, nc] (float64, exactly representable in float32)."""
    model = SCENES[name](E, device=device)
    jq, _ = random_joint_state(model, seed)
    q_star = inside_limits(model, jq)
    start = perturbed(model, q_star, seed + 1000).astype(np.float32).astype(np.float64)
    return model, q_star, targets_at(name, model, q_star, dtype), start


def pose_errors(name, model, q, targets):
    """(max position error [E] in metres, max rotation error [E] in radians) of the objectives at q against ``targets``."""
    E = model.env.env_count
    pos, rot = np.zeros(E), np.zeros(E)
    for (kind, link), tg in zip(objective_specs(name, model), targets):
        if kind == "position":
            pos = np.maximum(pos, np.linalg.norm(link_pose(model, q, link, offset=OFFSET) - np.asarray(tg, dtype=np.float64), axis=1))
        elif kind == "rotation":
            qe = _qmul(link_pose(model, q, link, offset_rotation=OFFSET_ROT), np.asarray(tg, dtype=np.float64) * [-1.0, -1.0, -1.0, 1.0])
            rot = np.maximum(rot, 2.0 * np.arctan2(np.linalg.norm(qe[:, :3], axis=1), np.abs(qe[:, 3])))
    return pos, rot
