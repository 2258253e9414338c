"""D6 joints with two and three angular axes on the device: the checks of tests/test_d6_angular_emu.py (which documents them and
records the measured error / allowance ratios) through the public API -- SolverSemiImplicit.step against the float64 reference of
tests/d6_reference.py (direct comparison and gimbal band, the same tables and the same MARGIN), and the chain of
scenes.d6_angular_scene under the three solvers against the CPU oracle step by step (11 worlds, 25 steps, the loop and tolerances of
tests/test_gpu_parity_joint_zoo.py), SolverFeatherstone's poses also against a float64 FK of its own joint_q."""
import numpy as np
import pytest

import d6_reference as R
from d6_reference import STEPWISE, TABLES, check_direct, check_gimbal, fk_residual
from d6_reference import rel_error as _rel

pytestmark = pytest.mark.gpu


def hip_step(model):
    import newton_amd as nt

    solver = nt.solvers.SolverSemiImplicit(model, angular_damping=0.0)
    s0, s1 = model.state(), model.state()
    s0.clear_forces()
    solver.step(s0, s1, model.control(), None, R.DT)
    return s1.body_qd.cpu().numpy()


@pytest.mark.parametrize("ang,parent", TABLES)
def test_wrench_against_float64_reference_hip(ang, parent):
    check_direct(hip_step, ang, parent, device="cuda:0", tag="hip")


def test_gimbal_band_decomposition_hip():
    check_gimbal(hip_step, device="cuda:0", tag="hip")


@pytest.mark.parametrize("free_root", [False, True])
@pytest.mark.parametrize("solver", sorted(STEPWISE))
def test_chain_stepwise_hip(solver, free_root):
    import newton_amd as nt
    from oracle_bridge import Oracle, OracleState
    from scenes import d6_angular_scene

    dt, tol_q, tol_qd = STEPWISE[solver]
    model = d6_angular_scene(11, device="cuda:0", free_root=free_root)
    o = Oracle(model)
    jf = np.random.default_rng(9).normal(0, 0.5, size=model.joint_dof_count).astype(np.float32)
    s0, s1 = model.state(), model.state()
    ctrl = model.control()
    ctrl.joint_f = jf
    if solver == "xpbd":
        hip = nt.solvers.SolverXPBD(model, iterations=3)
    elif solver == "semi":
        hip = nt.solvers.SolverSemiImplicit(model)
    else:
        hip = nt.solvers.SolverFeatherstone(model)
    os0, os1 = OracleState(model), OracleState(model)
    c = o.control(joint_f=jf)
    for _ in range(25):
        s0.body_q, s0.body_qd = os0.body_q, os0.body_qd
        s0.joint_q, s0.joint_qd = os0.joint_q, os0.joint_qd
        s0.clear_forces()
        hip.step(s0, s1, ctrl, None, dt)
        os0.body_f[:] = 0
        if solver == "xpbd":
            o.xpbd_step(os0, os1, c, None, dt, iterations=3)
        elif solver == "semi":
            o.semi_implicit_step(os0, os1, c, None, dt)
        else:
            o.featherstone_step(os0, os1, c, None, dt)
        assert np.all(np.isfinite(os1.body_q))
        assert _rel(s1.body_q.cpu().numpy(), os1.body_q) <= tol_q
        assert _rel(s1.body_qd.cpu().numpy(), os1.body_qd) <= tol_qd
        if solver == "fs":
            assert _rel(s1.joint_q.cpu().numpy(), os1.joint_q) <= tol_q
            assert _rel(s1.joint_qd.cpu().numpy(), os1.joint_qd) <= tol_qd
        os0, os1 = os1, os0
    assert np.abs(os0.body_q - np.asarray(model.body_q)).max() > 1e-4  # it moved
    if solver == "fs":  # independent of the oracle
        assert fk_residual(model, s1.body_q.cpu().numpy(), s1.joint_q.cpu().numpy()) <= 1e-6  # (the bound of tests/test_kinematics.py)
