"""newton_amd.ik on host models: the float64 numpy path that is the reference of the device kernel (nt_ik_solve,
include/newton_hip_kinematics.h).  Derivative consistency of residuals, Jacobian rows and retraction; one iteration against
numpy.linalg.solve; convergence of every problem of every scene; the interface."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import newton_amd as nt
from ik_cases import OFFSET, OFFSET_ROT, SCENES, ik_case, make_objectives, objective_specs, pose_errors
from newton_amd import _lib, ik

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "newton_hip_kinematics.h")
E = 5
_CASES = {}


def _case(name):
    """model, q*, float64 targets, start, solver (computed once per scene; the tests reset the solver before use)."""
    if name not in _CASES:
        model, q_star, targets, start = ik_case(name, E, 5, dtype=np.float64)
        _CASES[name] = (model, q_star, targets, start, ik.IKSolver(model, make_objectives(name, model, targets)))
    return _CASES[name]


def _rotation_rows(name, model):
    rows, at = [], 0
    for kind, _ in objective_specs(name, model):
        n = model.env.nd if kind == "limit" else 3
        if kind == "rotation":
            rows += list(range(at, at + n))
        at += n
    return np.array(rows, dtype=np.int64), at


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. r(q (+) eps delta) - r(q) = eps J delta + O(eps^2): residuals, Jacobian rows, retraction and the FREE-joint COM convention
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENES))
def test_derivative_consistency(name):
    model, q_star, targets, start, solver = _case(name)
    nd = model.env.nd
    rng = np.random.default_rng(3)
    delta = rng.normal(size=(E, nd))
    delta /= np.linalg.norm(delta, axis=1, keepdims=True)
    rot_rows, m = _rotation_rows(name, model)
    # at q* every row (the rotation error is zero there: the Gauss-Newton rows are exact); at the start all but the rotation rows
    for q, keep in ((q_star, np.arange(m)), (start, np.setdiff1d(np.arange(m), rot_rows))):
        q = solver.retract_numpy(q, np.zeros((E, nd)))  # (unit quaternions in float64: the drawn ones are fp32-rounded)
        r0, J = solver.evaluate_numpy(q)
        lin = np.einsum("emd,ed->em", J, delta)

        def defect(eps):
            r1, _ = solver.evaluate_numpy(solver.retract_numpy(q, eps * delta), jacobian=False)
            return np.linalg.norm((r1 - r0 - eps * lin)[:, keep], axis=1)

        d1, d2 = defect(1e-4), defect(0.5e-4)
        print(f"[ik host] {name}: defect(1e-4) max {d1.max():.3e}, defect(5e-5) max {d2.max():.3e}, |J delta| min {np.linalg.norm(lin, axis=1).min():.3e}")
        assert np.all(d1 <= 1e-6)  # O(eps^2) = 1e-8 times a curvature of order <= 100 (first order would be 1e-4)
        big = d1 > 1e-12  # above float64 rounding of the difference
        assert np.all(np.abs(d1[big] / d2[big] - 4.0) <= 0.2)
        assert np.linalg.norm(lin, axis=1).min() > 1e-3  # (the comparison is not vacuous)


def test_joint_limit_rows():
    """A violated limit: residual, Jacobian row and derivative; dofs without limits have zero rows."""
    model, q_star, targets, start, _ = _case("joint_zoo")
    t = model.env
    lo = np.asarray(model.joint_limit_lower, dtype=np.float64).reshape(E, t.nd)
    hi = np.asarray(model.joint_limit_upper, dtype=np.float64).reshape(E, t.nd)
    limited = (lo < hi) & (np.abs(lo) < 1e10) & (np.abs(hi) < 1e10)
    assert limited.any() and not limited.all()
    solver = ik.IKSolver(model, [ik.IKObjectiveJointLimit(weight=2.0)])
    q = q_star.copy()
    d = int(np.flatnonzero(limited[0])[0])
    coord = int(solver._dof_coord[d])
    q[:, coord] = hi[:, d] + 0.05
    r, J = solver.evaluate_numpy(q)
    assert np.allclose(r[:, d], 2.0 * 0.05) and np.all(J[:, d, d] == 2.0)
    assert np.count_nonzero(r) == E and np.count_nonzero(J) == E
    q[:, coord] = lo[:, d] - 0.1
    r, J = solver.evaluate_numpy(q)
    assert np.allclose(r[:, d], -2.0 * 0.1) and np.all(J[:, d, d] == 2.0)
    # one step brings the coordinate back inside
    out = np.zeros_like(q)
    solver.step(q, out, iterations=20)
    assert np.all(out[:, coord] >= lo[:, d] - 1e-6) and np.all(solver.costs <= 1e-10)
    # custom limits replace the model's
    wide = ik.IKSolver(model, [ik.IKObjectiveJointLimit(np.full(E * t.nd, -50.0), np.full(E * t.nd, 50.0))])
    assert np.all(wide.evaluate_numpy(q)[0] == 0.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. one iteration against numpy.linalg.solve on normal equations assembled here
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step_size", [1.0, 0.6])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_one_iteration_against_linalg_solve(name, step_size):
    """The normal equations are assembled here from the solver's own r and J (``evaluate_numpy``; J is pinned independently by
    test_derivative_consistency); the solve (LU here, Cholesky there), the predicted reduction from the model's definition, the
    candidate's cost and the decision are independent of ``step``."""
    model, q_star, targets, start, solver = _case(name)
    solver.reset()
    nd = model.env.nd
    r, J = solver.evaluate_numpy(start)
    lam = float(np.float32(0.1))  # (lambdas are float32 resident)
    out = np.zeros_like(start)
    solver.step(start, out, iterations=1, step_size=step_size)
    accepted = 0
    for e in range(E):
        A = J[e].T @ J[e] + lam * np.eye(nd)
        g = J[e].T @ r[e]
        delta = np.linalg.solve(A, -g)
        p = step_size * delta
        pred = -(g @ p) - 0.5 * p @ (J[e].T @ J[e]) @ p  # the reduction of the quadratic model, from its definition
        assert abs(ik.predicted_reduction(step_size, lam, delta @ delta, g @ delta) - pred) <= 1e-12 * max(1.0, abs(pred))
        cand = solver.retract_numpy(np.tile(start[e], (E, 1)), np.tile(p, (E, 1)))[0]
        r2 = solver.evaluate_numpy(np.tile(cand, (E, 1)), jacobian=False)[0][e]
        c0, c2 = 0.5 * r[e] @ r[e], 0.5 * r2 @ r2
        ok = pred > 0.0 and c2 < c0 and (c0 - c2) / pred > solver.rho_min
        accepted += ok
        want = cand if ok else start[e]
        # Cholesky (the solver) against LU (here): both backward stable, the solutions differ by at most ~ n eps cond(A) |delta| each
        tol = 2.0 * nd * 2.0 ** -52 * np.linalg.cond(A) * max(1.0, np.abs(delta).max())
        assert np.abs(out[e] - want).max() <= tol, (name, e, np.abs(out[e] - want).max(), tol)
        assert solver.lambdas[e] == np.float32(0.05 if ok else 0.2)
        assert abs(solver.costs[e] - (c2 if ok else c0)) <= 1e-6 * max(c0, 1e-30)
    assert accepted > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. convergence of every problem, monotone costs, the lambda rule, reset
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENES))
def test_every_problem_converges_within_50_iterations(name):
    model, q_star, targets, start, solver = _case(name)
    solver.reset()
    trace = []
    lam0 = solver.lambdas.astype(np.float64)
    q, lam, cost, _ = solver._solve_numpy(start, lam0, 50, 1.0, trace)
    pos, rot = pose_errors(name, model, q, targets)
    print(f"[ik host] {name}: position error max {pos.max():.3e} m, rotation error max {rot.max():.3e} rad, cost max {cost.max():.3e}")
    assert np.all(pos <= 1e-8) and np.all(rot <= 1e-7)
    costs = np.array([0.5 * np.sum(solver.evaluate_numpy(start, jacobian=False)[0] ** 2, axis=1)] + [tr["cost"] for tr in trace])
    assert np.all(np.diff(costs, axis=0) <= 0.0)
    cur = lam0
    for tr in trace:
        assert np.array_equal(tr["lam"], cur)
        cur = np.where(tr["accept"], np.maximum(cur / solver.lambda_factor, solver.lambda_min), np.minimum(cur * solver.lambda_factor, solver.lambda_max))
    assert np.array_equal(cur, lam)
    # the public call: the same iterate; lambdas persist across calls; reset restores them
    out = np.zeros_like(start)
    solver.step(start, out, iterations=20)
    solver.step(out, out, iterations=30)
    assert np.abs(out - q).max() <= 1e-9 and np.array_equal(solver.lambdas, lam.astype(np.float32))
    assert np.allclose(solver.costs, cost, rtol=1e-5, atol=1e-30)
    solver.reset()
    assert np.all(solver.lambdas == np.float32(0.1))
    # float32 arrays: rounded output, flat shape
    flat_in, flat_out = start.astype(np.float32).reshape(-1), np.zeros(start.size, np.float32)
    solver.step(flat_in, flat_out, iterations=50)
    p32, r32 = pose_errors(name, model, flat_out.astype(np.float64).reshape(start.shape), targets)
    assert np.all(p32 <= 1e-5) and np.all(r32 <= 1e-5)  # fp32 coordinates: 6e-8 relative each, along the chain


def test_cholesky_solve_marks_a_non_positive_pivot():
    A = np.tile(np.eye(3), (4, 1, 1)) * np.array([2.0, 1.0, 4.0, 3.0])[:, None, None]
    A[1, 2, 2] = -1.0
    x, ok = ik._cholesky_solve(A, np.ones((4, 3)))
    assert np.array_equal(ok, [True, False, True, True]) and np.all(x[1] == 0.0)
    assert np.allclose(x[[0, 2, 3]], 1.0 / np.array([2.0, 4.0, 3.0])[:, None])


def test_zero_iterations_and_rejected_steps_keep_the_input_bit_for_bit():
    from ik_parity import rejected_only_case

    model, solver, start = rejected_only_case(E)
    q_in = start.astype(np.float32)
    out = np.full_like(q_in, 7.0)
    solver.step(q_in, out, iterations=0)
    assert np.array_equal(out.view(np.uint32), q_in.view(np.uint32)) and np.all(solver.costs > 100.0)
    solver.step(q_in, out, iterations=30)
    assert np.array_equal(out.view(np.uint32), q_in.view(np.uint32)) and np.all(solver.lambdas == np.float32(1e-5))


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the interface
# ---------------------------------------------------------------------------------------------------------------------------------
def test_argument_and_shape_errors():
    model, q_star, targets, start, solver = _case("joint_zoo")
    nb = model.env.nb
    with pytest.raises(ValueError):
        ik.IKObjectivePosition(0, [0.0, 0.0], np.zeros((E, 3)))
    with pytest.raises(ValueError):
        ik.IKObjectivePosition(0, [0.0, 0.0, 0.0], np.zeros((E, 4)))
    with pytest.raises(ValueError):
        ik.IKObjectiveRotation(0, [0.0, 0.0, 0.0, 1.0], np.zeros((E, 3)))
    with pytest.raises(ValueError):
        ik.IKSolver(model, [ik.IKObjectivePosition(nb, [0.0, 0.0, 0.0], np.zeros((E, 3)))])
    with pytest.raises(ValueError):
        ik.IKSolver(model, [ik.IKObjectivePosition(0, [0.0, 0.0, 0.0], np.zeros((E + 1, 3)))])
    with pytest.raises(ValueError):
        ik.IKSolver(model, [ik.IKObjectiveJointLimit(np.zeros(3), None)])
    with pytest.raises(TypeError):
        ik.IKSolver(model, ["position"])
    out = np.zeros_like(start, dtype=np.float32)
    with pytest.raises(ValueError):
        solver.step(start.astype(np.float32)[:-1], out)
    with pytest.raises(ValueError):
        solver.step(start.astype(np.float32), out, iterations=-1)
    with pytest.raises(ValueError):
        solver.step(start.astype(np.float32), out, step_size=0.0)
    with pytest.raises(ValueError):
        solver.step(start.astype(np.int32), out)
    with pytest.raises(ValueError):
        solver.objectives[0].set_target_positions(np.zeros((E, 2)))
    assert solver.n_problems == E and solver.costs.dtype == np.float32 and solver.lambdas.shape == (E,)
    assert nt.ik is ik


def test_refusals():
    from test_heterogeneous_worlds import mixed_model

    tgt = np.zeros((1, 3), np.float32)
    with pytest.raises(NotImplementedError, match="heterogeneous"):
        ik.IKSolver(mixed_model((("quadruped", 1), ("pendulum", 1))), [])
    env = nt.ModelBuilder()
    b = env.add_link(xform=[0.0, 0.0, 1.0, 0, 0, 0, 1])
    env.add_shape_box(b, hx=0.1, hy=0.05, hz=0.05)
    env.add_joint_revolute(-1, b, axis=[0.0, 1.0, 0.0])
    with pytest.raises(NotImplementedError, match="articulations"):
        ik.IKSolver(env.finalize(), [ik.IKObjectivePosition(0, [0.0, 0.0, 0.0], tgt)])
    env = nt.ModelBuilder()
    cfg = nt.ModelBuilder.ShapeConfig(has_shape_collision=False)
    a, loose = env.add_link(xform=[0.0, 0.0, 1.0, 0, 0, 0, 1]), env.add_link(xform=[0.0, 1.0, 1.0, 0, 0, 0, 1])
    for link in (a, loose):
        env.add_shape_box(link, hx=0.1, hy=0.05, hz=0.05, cfg=cfg)
    env.add_articulation([env.add_joint_revolute(-1, a, axis=[0.0, 1.0, 0.0])])
    with pytest.raises(NotImplementedError, match="no joint's child"):
        ik.IKSolver(env.finalize(), [ik.IKObjectivePosition(0, [0.0, 0.0, 0.0], tgt)])
    env = nt.ModelBuilder()
    a = env.add_link(xform=[0.0, 0.0, 1.0, 0, 0, 0, 1])
    env.add_shape_box(a, hx=0.1, hy=0.05, hz=0.05, cfg=cfg)
    D = nt.ModelBuilder.JointDofConfig
    env.add_articulation([env.add_joint_d6(-1, a, angular_axes=[D(axis=[1.0, 0.0, 0.0]), D(axis=[0.6, 0.8, 0.0])])])
    with pytest.raises(NotImplementedError, match="not mutually orthogonal"):
        ik.IKSolver(env.finalize(), [ik.IKObjectivePosition(0, [0.0, 0.0, 0.0], tgt)])
    model = _case("joint_zoo")[0]
    many = [ik.IKObjectivePosition(0, [0.0, 0.0, 0.0], np.zeros((E, 3), np.float32)) for _ in range(ik.MAX_OBJECTIVES + 1)]
    with pytest.raises(NotImplementedError, match="objectives"):
        ik.IKSolver(model, many)


def test_set_target_writes_in_place():
    model, q_star, targets, start, _ = _case("joint_zoo")
    pos = ik.IKObjectivePosition(model.env.nb - 1, OFFSET, np.zeros((E, 3), np.float32))
    rot = ik.IKObjectiveRotation(model.env.nb - 1, OFFSET_ROT, np.tile([0.0, 0.0, 0.0, 1.0], (E, 1)).astype(np.float32))
    solver = ik.IKSolver(model, [pos, rot])
    store_p, store_r = pos.target_positions, rot.target_rotations
    at_p, at_r = store_p.ctypes.data, store_r.ctypes.data
    pos.set_target_positions(targets[0])
    rot.set_target_rotations(targets[1].reshape(-1))
    assert pos.target_positions is store_p and store_p.ctypes.data == at_p and rot.target_rotations is store_r and store_r.ctypes.data == at_r
    assert np.array_equal(store_p, targets[0].astype(np.float32)) and store_p.dtype == np.float32
    out = np.zeros_like(start)
    solver.step(start, out, iterations=50)
    p, r = pose_errors("joint_zoo", model, out, [None if t is None else t.astype(np.float32) for t in targets])
    assert np.all(p <= 1e-6) and np.all(r <= 1e-6)  # (float32 targets: reachable to their own rounding)


def _declaration(name):
    text = open(HEADER).read()
    m = re.search(r"nt_status\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/newton_hip_kinematics.h"
    return [" ".join(re.sub(r"/\*.*?\*/", "", a).split()) for a in m.group(1).split(",")]


def test_header_and_ctypes_table_agree():
    args = _declaration("nt_ik_solve")
    assert args == ["const nt_model* m", "const nt_ik_problem* p", "const float* joint_q_in", "float* joint_q_out", "float* lambda",
                    "float* cost", "int32_t iterations", "float step_size", "void* stream"]
    P = C.c_void_p
    assert _lib.SYMBOLS["nt_ik_solve"] == (C.c_int32, [C.POINTER(_lib.nt_model), C.POINTER(_lib.nt_ik_problem), P, P, P, P, C.c_int32,
                                                         C.c_float, P])
    assert _declaration("nt_ik_solve_tile") == args[:8] + ["int32_t envs_per_block", "void* stream"]
    assert _lib.SYMBOLS["nt_ik_solve_tile"] == (C.c_int32, _lib.SYMBOLS["nt_ik_solve"][1][:8] + [C.c_int32, P])
    text = open(HEADER).read()
    assert re.search(r"^ \*\s+nt_ik_solve\s+<-", text, re.M)  # the entry-point table
    assert int(re.search(r"#define NT_IK_MAX_OBJECTIVES (\d+)", text).group(1)) == _lib.NT_IK_MAX_OBJECTIVES == ik.MAX_OBJECTIVES
    enum = re.search(r"enum \{ NT_IK_POSITION = (\d), NT_IK_ROTATION = (\d), NT_IK_JOINT_LIMIT = (\d) \}", text)
    assert tuple(int(x) for x in enum.groups()) == (_lib.NT_IK_POSITION, _lib.NT_IK_ROTATION, _lib.NT_IK_JOINT_LIMIT)
    # the struct mirrors: field order and sizes as the header declares them (natural alignment)
    fields = re.search(r"typedef struct nt_ik_objective \{(.*?)\} nt_ik_objective;", text, re.S).group(1)
    names = re.findall(r"(\w+)(?:\[\d+\])?;", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert names == [f[0] for f in _lib.nt_ik_objective._fields_]
    assert C.sizeof(_lib.nt_ik_objective) == 40 and C.sizeof(_lib.nt_ik_problem) == 24 + 40 * _lib.NT_IK_MAX_OBJECTIVES
    import __graft_entry__ as g

    assert not any("newton_hip_kinematics.h" in d for d in g.UNITS["nt_kernels.hip"])  # the headline unit keeps its id
