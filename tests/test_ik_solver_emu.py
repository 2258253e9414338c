"""ik_solve_kernel (nt_ik_solve, include/newton_hip_kinematics.h) on the emulator: the kernel SOURCES executed on the CPU (tests/emu),
without a GPU, against the float64 host path of newton_amd.ik on identical fp32 inputs.  37 worlds (not a multiple of any tile), one
environment per workgroup and the default tile."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import tolerances  # noqa: E402
from ik_cases import LIMITED_SCENES, OFFSET, ik_case, make_objectives, violated_limit_rows  # noqa: E402
from ik_parity import (PARITY_GATE, device_problem, long_chain, mirror_cost, one_iteration_ratio, reference_iteration, rejected_only_case)  # noqa: E402
from newton_amd import ik  # noqa: E402

N_WORLDS = 37
EMU_SCENES = ["quadruped", "joint_zoo_free_root", "d6_zoo", "multi_art"]


@pytest.fixture(scope="module")
def H(oracle_lib):
    import harness

    harness.lib()  # builds tests/emu/_build/libnewton_emu.so on first use
    return harness


def _solve(H, em, prob, q_in, lam, iterations, step=1.0, epb=0, out=None):
    """One nt_ik_solve_tile on host arrays: (joint_q_out, lambda, cost)."""
    q_in = np.ascontiguousarray(q_in, dtype=np.float32)
    q_out = np.full_like(q_in, 7.0) if out is None else out
    lam = np.ascontiguousarray(lam, dtype=np.float32).copy()
    cost = np.full(len(lam), 7.0, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    H.check(H.lib().nt_ik_solve_tile(C.byref(em.desc), C.byref(prob.desc), p(q_in), p(q_out), p(lam), p(cost), iterations, step, epb, None),
            "nt_ik_solve_tile")
    return q_out, lam, cost


_CASES = {}


def _case(name):
    if name not in _CASES:
        model, q_star, targets, start = ik_case(name, N_WORLDS, 5)
        solver = ik.IKSolver(model, make_objectives(name, model, targets))
        if name in LIMITED_SCENES:  # test construction: the joint-limit rows are not all zero -- every world violates a limit
            assert np.all(violated_limit_rows(solver, start) > 0)
        _CASES[name] = (model, solver, start, reference_iteration(solver, start))
    return _CASES[name]


@pytest.mark.parametrize("epb", [1, 0])
@pytest.mark.parametrize("name", EMU_SCENES)
def test_one_iteration_parity(H, name, epb):
    model, solver, start, ref = _case(name)
    em = H.EmuModel(model)
    q_out, lam, cost = _solve(H, em, device_problem(solver), start, solver.lambdas, 1, epb=epb)
    ratio = one_iteration_ratio(solver, start, ref, q_out)
    print(f"[ik emu] {name} epb {epb}: max |d delta| / max(1, |delta|) / (2^-24 cond A) = {ratio.max():.3f} (nd^2 = {model.env.nd ** 2})")
    tolerances.record(f"ik_solver_emu_{name}_epb{epb}", {"delta_over_eps_cond": {"max": float(ratio.max())}}, {"delta_over_eps_cond": PARITY_GATE})
    assert ratio.max() <= model.env.nd ** 2  # beyond the textbook worst case of a Cholesky solve: a defect, not a number to adopt
    assert ratio.max() <= PARITY_GATE
    assert np.array_equal(lam, np.where(ref["accept"], 0.05, 0.2).astype(np.float32))
    want, allowed = mirror_cost(solver, q_out)
    assert np.all(np.abs(cost - want) <= allowed)


def test_one_iteration_parity_with_a_scaled_step(H):
    """step_size 0.6 on the scene with violated joint limits: the (2 - s) term of the predicted reduction and the scaled retraction."""
    name, s = "joint_zoo_free_root", 0.6
    model, solver, start, _ = _case(name)
    ref = reference_iteration(solver, start, s)
    em = H.EmuModel(model)
    q_out, lam, cost = _solve(H, em, device_problem(solver), start, solver.lambdas, 1, step=s)
    ratio = one_iteration_ratio(solver, start, ref, q_out)
    print(f"[ik emu] {name} step {s}: max |d delta| / max(1, |delta|) / (2^-24 cond A) = {ratio.max():.3f}")
    tolerances.record(f"ik_solver_emu_{name}_step06", {"delta_over_eps_cond": {"max": float(ratio.max())}}, {"delta_over_eps_cond": PARITY_GATE})
    assert ratio.max() <= PARITY_GATE
    assert np.array_equal(lam, np.where(ref["accept"], 0.05, 0.2).astype(np.float32))
    want, allowed = mirror_cost(solver, q_out)
    assert np.all(np.abs(cost - want) <= allowed)
    # not the full step's result: the scaled step is really taken
    full, _, _ = _solve(H, em, device_problem(solver), start, solver.lambdas, 1)
    assert not np.array_equal(full, q_out)


@pytest.mark.parametrize("name", EMU_SCENES)
def test_thirty_iterations(H, name):
    model, solver, start, _ = _case(name)
    em = H.EmuModel(model)
    _, _, cost_in = _solve(H, em, device_problem(solver), start, solver.lambdas, 0)
    q_out, lam, cost = _solve(H, em, device_problem(solver), start, solver.lambdas, 30)
    want, allowed = mirror_cost(solver, q_out)
    print(f"[ik emu] {name}: cost in max {cost_in.max():.3e}, out max {cost.max():.3e}, |cost - mirror| max {np.abs(cost - want).max():.3e}")
    assert np.all(np.abs(cost - want) <= allowed)
    assert np.all(cost <= cost_in)
    assert np.all(np.isfinite(q_out)) and np.all(q_out != 7.0)


def test_zero_iterations_copy_and_cost(H):
    model, solver, start, ref = _case("quadruped")
    em = H.EmuModel(model)
    q_out, lam, cost = _solve(H, em, device_problem(solver), start, solver.lambdas, 0)
    assert np.array_equal(q_out, start.astype(np.float32)) and np.array_equal(lam, solver.lambdas)
    assert np.all(np.abs(cost - ref["cost_in"]) <= 1e-5 * ref["cost_in"])


@pytest.mark.parametrize("epb", [1, 0])
def test_rejected_only_problem_returns_its_input_bit_for_bit(H, epb):
    model, solver, start = rejected_only_case(N_WORLDS)
    em = H.EmuModel(model)
    q_in = start.astype(np.float32)
    q_out, lam, cost = _solve(H, em, device_problem(solver), q_in, solver.lambdas, 30, epb=epb)
    assert np.array_equal(q_out.view(np.uint32), q_in.view(np.uint32))
    assert np.all(lam == np.float32(1e-5))
    # in place
    buf = q_in.copy()
    _solve(H, em, device_problem(solver), buf, solver.lambdas, 3, epb=epb, out=buf)
    assert np.array_equal(buf.view(np.uint32), q_in.view(np.uint32))


def test_too_many_objectives_and_bad_arguments(H):
    model, solver, start, _ = _case("multi_art")
    em = H.EmuModel(model)
    prob = device_problem(solver)
    q = start.astype(np.float32)
    lam, cost = solver.lambdas.copy(), np.zeros(N_WORLDS, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    lib = H.lib()
    assert lib.nt_ik_solve(C.byref(em.desc), C.byref(prob.desc), None, p(q), p(lam), p(cost), 1, 1.0, None) == -1
    assert lib.nt_ik_solve(C.byref(em.desc), C.byref(prob.desc), p(q), p(q), p(lam), p(cost), -1, 1.0, None) == -1
    assert lib.nt_ik_solve_tile(C.byref(em.desc), C.byref(prob.desc), p(q), p(q), p(lam), p(cost), 1, 1.0, 3, None) == -3
    prob.desc.count = 9
    assert lib.nt_ik_solve(C.byref(em.desc), C.byref(prob.desc), p(q), p(q), p(lam), p(cost), 1, 1.0, None) == -3


def test_a_tile_that_does_not_fit_the_lds_is_unsupported(H):
    """300 dofs: the packed J^T J of ONE world is 45 150 rows = 176 KB, more than the 160 KB of a CU: refused before any launch."""
    model = long_chain(300)
    solver = ik.IKSolver(model, [ik.IKObjectivePosition(299, OFFSET, np.zeros((1, 3), np.float32))])
    em = H.EmuModel(model)
    prob = device_problem(solver)
    q, lam, cost = np.zeros(300, np.float32), solver.lambdas.copy(), np.full(1, 7.0, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for epb in (0, 1):
        assert H.lib().nt_ik_solve_tile(C.byref(em.desc), C.byref(prob.desc), p(q), p(q), p(lam), p(cost), 1, 1.0, epb, None) == -3
    assert cost[0] == 7.0
