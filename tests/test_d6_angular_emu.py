"""D6 joints with two and three angular axes, without a GPU: the CPU oracle and the kernel SOURCES on the emulator (tests/emu).

Part A -- the `ang >= 2` branch of SolverSemiImplicit's joint phase (si_joint_item in nt_semi_implicit.hpp, quat_decompose in
nt_math.hpp; oracle_semi_implicit.cpp, wp_builtins.h) against the float64 reference of tests/d6_reference.py, whose decomposition is
scipy's.  Direct comparison: the joint wrench read off one step (run A minus run B, see d6_reference) against the reference on
the same float32-rounded inputs; the allowance per case and body is the reference's own largest change under +-1 ulp perturbations of
the input quaternions, times MARGIN.  Gimbal band: three read-outs from rest recover (a_0, a_1, a_2) and Rx(a_0) Ry(a_1) Rz(a_2)
must be r_err within d6_reference.gimbal_bound.

MARGIN (d6_reference.MARGIN = 16) was fixed from the CPU oracle's worst error / allowance ratio with about 4x headroom, before the
emulator or the device were looked at.  Measured worst ratios (force, torque) over all four tables (2 | 3 axes) x (world | free parent):
    CPU oracle   3.77   2.99
    emulator     3.77   2.99       (envs_per_block 1 and 8: the oracle's bits)
    MI355X       3.77   3.03
Gimbal band, worst rotation angle / bound: 0.297 (5.96e-4 rad against 2.004e-3) on the oracle, the emulator and the MI355X alike; with
the branch test on sin(a1) this work replaced it was 449 (0.9 rad, the pose a = -2, b = pi/2, c = 1.1).

What these tests cannot see, shown by mutating the kernel: dropping the `a >= pi` wrap of quat_decompose (atan2f never exceeds
float32(pi), so the wrap acts on that single value, and the tables stay 1e-3 away from +-pi where fp32 and fp64 land on different
sides), and negating the cross product that stands in for the locked third axis of a two-axis joint (its force is zero for every
non-zero angle, see d6_reference.d6_wrench).  A wrong sign of R12, an untransported second axis and the old branch test all fail here.

Part B -- a chain of such joints (scenes.d6_angular_scene: two angular axes, linear + two angular, three angular in the order
x, z, y) under all three solvers, emulated kernels vs the oracle step by step with the loop and tolerances of
tests/test_gpu_parity_joint_zoo.py; SolverFeatherstone's body_q additionally against a float64 FK of its own joint_q composed with
scipy, since the oracle shares the kernels' formulas."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import d6_reference as R  # noqa: E402
from d6_reference import STEPWISE, TABLES, check_direct, check_gimbal, fk_residual, rel_error  # noqa: E402


@pytest.fixture(scope="module")
def H(oracle_lib):
    import harness

    harness.lib()
    return harness


def oracle_step(model):
    from oracle_bridge import Oracle, OracleState

    o = Oracle(model)
    s0, s1 = OracleState(model), OracleState(model)
    o.semi_implicit_step(s0, s1, o.control(), None, R.DT, angular_damping=0.0)
    return s1.body_qd


def emu_step(H, epb):
    def step(model):
        em = H.EmuModel(model)
        s0, s1 = H.EmuState(em), H.EmuState(em)
        H.semi_implicit_step(em, s0, s1, H.EmuControl(em), None, R.DT, epb=epb, angular_damping=0.0)
        return s1.aos("body_qd")

    return step


@pytest.mark.parametrize("ang,parent", TABLES)
def test_wrench_against_float64_reference_oracle(oracle_lib, ang, parent):
    check_direct(oracle_step, ang, parent, tag="oracle")


@pytest.mark.parametrize("epb", [1, 8])
@pytest.mark.parametrize("ang,parent", TABLES)
def test_wrench_against_float64_reference_emu(H, ang, parent, epb):
    check_direct(emu_step(H, epb), ang, parent, tag=f"emu epb={epb}")


def test_gimbal_band_decomposition_oracle(oracle_lib):
    check_gimbal(oracle_step, tag="oracle")


@pytest.mark.parametrize("epb", [1, 8])
def test_gimbal_band_decomposition_emu(H, epb):
    check_gimbal(emu_step(H, epb), tag=f"emu epb={epb}")


# ---------------------------------------------------------------------------------------------------------------------------------
# Part B: the chain under the three solvers
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("free_root", [False, True])
@pytest.mark.parametrize("solver", sorted(STEPWISE))
def test_chain_stepwise_emu(H, solver, free_root):
    from oracle_bridge import Oracle, OracleState
    from scenes import d6_angular_scene

    dt, tol_q, tol_qd = STEPWISE[solver]
    model = d6_angular_scene(5, free_root=free_root)
    assert [int(a) for a in model.env.joint_ang_count[1:]] == [2, 2, 3]
    jf = np.random.default_rng(9).normal(0, 0.5, size=model.joint_dof_count).astype(np.float32)
    em, o = H.EmuModel(model), Oracle(model)
    ctrl, c = H.EmuControl(em, joint_f=jf), o.control(joint_f=jf)
    os0, os1 = OracleState(model), OracleState(model)
    for _ in range(5):
        s0 = H.EmuState(em, body_q=os0.body_q, body_qd=os0.body_qd, joint_q=os0.joint_q, joint_qd=os0.joint_qd)
        s1 = H.EmuState(em)
        os0.body_f[:] = 0
        if solver == "xpbd":
            H.xpbd_step(em, s0, s1, ctrl, None, dt, iterations=3)
            o.xpbd_step(os0, os1, c, None, dt, iterations=3)
        elif solver == "semi":
            H.semi_implicit_step(em, s0, s1, ctrl, None, dt)
            o.semi_implicit_step(os0, os1, c, None, dt)
        else:
            H.featherstone_step(em, s0, s1, ctrl, None, dt)
            o.featherstone_step(os0, os1, c, None, dt)
        assert np.all(np.isfinite(os1.body_q))
        assert rel_error(s1.aos("body_q"), os1.body_q) <= tol_q
        assert rel_error(s1.aos("body_qd"), os1.body_qd) <= tol_qd
        if solver == "fs":
            assert rel_error(s1.aos("joint_q"), os1.joint_q) <= tol_q
            assert rel_error(s1.aos("joint_qd"), os1.joint_qd) <= tol_qd
        os0, os1 = os1, os0
    assert np.abs(os0.body_q - np.asarray(model.body_q)).max() > 1e-5  # it moved
    if solver == "fs":  # independent of the oracle: the kernels' body_q is the float64 FK of the kernels' own joint_q
        assert fk_residual(model, s1.aos("body_q"), s1.aos("joint_q")) <= 1e-6  # (the bound of tests/test_kinematics.py)
