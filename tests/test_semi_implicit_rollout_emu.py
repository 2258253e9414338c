"""SolverSemiImplicit's fused rollout (nt_semi_implicit_rollout / semi_implicit_rollout_kernel) on the emulator: the kernel SOURCES
executed on the CPU (tests/emu), without a GPU.

The criterion is the project's exact one: N substeps in one launch == the loop `body_f = 0; collide; semi_implicit_step; swap`
launch by launch, bit for bit, on every body of every world -- state, the zeroed body_f of both states, the untouched joint
coordinates and the Contacts the last substep's collide leaves.  One case checks the rollout against the CPU oracle with the
tolerances of tests/test_gpu_parity_semi_implicit.py (same scene, same step count, same dt)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import newton_amd as nt  # noqa: E402
from newton_amd import _lib as L  # noqa: E402

NT_ERR_INVALID_ARG, NT_ERR_UNSUPPORTED = -1, -3
N_WORLDS = 37  # not a multiple of any tile


@pytest.fixture(scope="module")
def H(oracle_lib):
    import harness

    harness.lib()  # builds tests/emu/_build/libnewton_emu.so on first use
    return harness


def _rollout_status(H, em, s0, s1, control, contacts, dt, substeps, epb=0):
    p, cp = L.nt_semi_implicit_params(0.05, 1.0, 1.0e4, 1.0e2), L.nt_collide_params(0, epb)
    d0, d1, dc, dct = s0.desc(), s1.desc(), control.desc(), contacts.desc()
    return H.lib().nt_semi_implicit_rollout(C.byref(em.desc), C.byref(p), C.byref(cp), C.byref(d0), C.byref(d1), C.byref(dc),
                                            C.byref(dct), float(dt), int(substeps), None)


def _rollout(H, em, s0, s1, control, contacts, dt, substeps, epb=0):
    H.check(_rollout_status(H, em, s0, s1, control, contacts, dt, substeps, epb), "nt_semi_implicit_rollout")
    return s1 if substeps % 2 else s0


def _loop(H, em, s0, s1, control, contacts, dt, substeps, epb=0):
    for _ in range(substeps):
        s0.body_f[:] = 0
        H.collide(em, s0, contacts, epb=epb)
        H.semi_implicit_step(em, s0, s1, control, contacts, dt, epb=epb)
        s0, s1 = s1, s0
    return s0


def _pendulum():
    from scenes import pendulum_scene

    return pendulum_scene(N_WORLDS, seed=11), None, 1e-3


def _quadruped():
    from scenes import quadruped_scene

    model = quadruped_scene(N_WORLDS)
    model.joint_q.reshape(N_WORLDS, -1)[:, 2] -= 0.26  # lowered into contact
    model.body_q, model.body_qd = nt.articulation.eval_fk_numpy(model, model.joint_q, model.joint_qd)
    rng = np.random.default_rng(3)
    model.body_qd = (model.body_qd + rng.normal(0, 0.3, size=model.body_qd.shape)).astype(np.float32)
    return model, rng.normal(0, 1.0, size=model.joint_dof_count).astype(np.float32), 1e-4


def _box_stack():
    from scenes import box_stack_scene

    model = box_stack_scene(N_WORLDS)
    assert model.env.np_analytic < model.env.np  # the convex (MPR / GJK) variant of the kernel
    return model, None, 1e-4


def _d6_angular():
    from scenes import d6_angular_scene

    model = d6_angular_scene(N_WORLDS, seed=13, free_root=True)  # D6 joints with two and three angular axes
    return model, np.random.default_rng(4).normal(0, 0.5, size=model.joint_dof_count).astype(np.float32), 1e-4


SCENES = {"pendulum": _pendulum, "quadruped": _quadruped, "box_stack": _box_stack, "d6_angular": _d6_angular}


@pytest.mark.parametrize("epb", [1, 8])
@pytest.mark.parametrize("substeps", [6, 7])
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_rollout_equals_loop_bitwise(H, scene, substeps, epb):
    model, jf, dt = SCENES[scene]()
    em = H.EmuModel(model)
    ctrl = H.EmuControl(em, joint_f=jf)
    rng = np.random.default_rng(5)

    def states():  # body_f starts dirty in both: clear_forces is part of the frame
        a, b = H.EmuState(em), H.EmuState(em)
        a.body_f[:] = rng.normal(0, 1.0, size=a.body_f.shape).astype(np.float32)
        b.body_f[:] = a.body_f
        return a, b

    r0, r1 = states()
    rct = H.EmuContacts(em)
    jq, jqd = r0.joint_q.copy(), r0.joint_qd.copy()
    out = _rollout(H, em, r0, r1, ctrl, rct, dt, substeps, epb)
    assert out is (r1 if substeps % 2 else r0)
    rexp = rct.export()

    l0, l1 = states()
    lct = H.EmuContacts(em)
    ref = _loop(H, em, l0, l1, ctrl, lct, dt, substeps, epb)
    lexp = lct.export()  # (the loop's last collide is the last thing that wrote lct)

    E = model.env.env_count
    assert np.isfinite(ref.body_q[:, :, :E]).all() and not np.array_equal(ref.aos("body_q"), np.asarray(model.body_q, np.float32))
    # 1. state, every body of every world, bit for bit
    assert np.array_equal(out.aos("body_q").view(np.uint32), ref.aos("body_q").view(np.uint32))
    assert np.array_equal(out.aos("body_qd").view(np.uint32), ref.aos("body_qd").view(np.uint32))
    # 2. body_f of both states zero, the Contacts are the last collide's
    assert not r0.aos("body_f").any() and not r1.aos("body_f").any()
    n = int(lexp["count"][0])
    assert int(rexp["count"][0]) == n and (scene in ("pendulum", "d6_angular") or n > 0)
    for k, v in lexp.items():
        assert np.array_equal(rexp[k], v), k
    assert np.array_equal(rct.env_count[:E], lct.env_count[:E])
    # 3. this solver does not write generalized coordinates
    for s in (r0, r1):
        assert np.array_equal(s.joint_q, jq) and np.array_equal(s.joint_qd, jqd)


def _rel(a, b, floor=1.0):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), floor)))


def test_pendulum_rollout_against_oracle(H):
    """100 substeps at dt = 1e-3 in one launch vs the oracle's collide + step loop: tolerances of
    tests/test_gpu_parity_semi_implicit.py::test_pendulum_single_step_and_rollout."""
    from oracle_bridge import Oracle, OracleState
    from scenes import pendulum_scene

    model = pendulum_scene(N_WORLDS, seed=11)
    em = H.EmuModel(model)
    out = _rollout(H, em, H.EmuState(em), H.EmuState(em), H.EmuControl(em), H.EmuContacts(em), 1e-3, 100)
    o = Oracle(model)
    os0, os1, oc, c = OracleState(model), OracleState(model), o.contacts(), o.control()
    for _ in range(100):
        os0.body_f[:] = 0
        o.collide(os0.body_q, oc)
        o.semi_implicit_step(os0, os1, c, oc, 1e-3)
        os0, os1 = os1, os0
    assert _rel(out.aos("body_q"), os0.body_q) <= 1e-4
    assert _rel(out.aos("body_qd"), os0.body_qd, floor=1.0) <= 1e-3


def test_argument_checks(H):
    from scenes import hull_bin_scene, pendulum_scene

    model = pendulum_scene(3)
    em = H.EmuModel(model)
    s0, s1, ctrl, ct = H.EmuState(em), H.EmuState(em), H.EmuControl(em), H.EmuContacts(em)
    before = s0.body_q.copy()
    assert _rollout_status(H, em, s0, s1, ctrl, ct, 1e-3, 0) == NT_ERR_INVALID_ARG
    assert _rollout_status(H, em, s0, s1, ctrl, ct, 1e-3, -2) == NT_ERR_INVALID_ARG
    assert np.array_equal(s0.body_q, before)
    # pair-heavy models keep their contact records in HBM: XPBD / collide only, like nt_semi_implicit_step
    model = hull_bin_scene(1, 40)
    em = H.EmuModel(model)
    assert em.desc.contact_scratch_in_hbm == 1
    s0, s1, ctrl, ct = H.EmuState(em), H.EmuState(em), H.EmuControl(em), H.EmuContacts(em)
    assert _rollout_status(H, em, s0, s1, ctrl, ct, 1e-4, 2) == NT_ERR_UNSUPPORTED
