"""newton_amd.eval_jacobian / eval_mass_matrix on the device (nt_eval_jacobian / nt_eval_mass_matrix,
include/newton_hip_kinematics.h) against the float64 reference of tests/test_eval_jacobian_host.py evaluated on the same fp32 inputs.
Gates (see there): J and joint_S_s 1e-5 * max(1, R) per entry, H 1e-5 * max|H_ref| per articulation, body_I_s 1e-5 * max|I_ref| per
body."""
import ctypes as C

import numpy as np
import pytest

import tolerances
from test_eval_ik_host import random_joint_state
from test_eval_jacobian_host import (GATE, POISON, SCENES, _link_identity_error, energy_error, jm_errors, kinetic_energy, reference,
                                     structure_ok, within_gates)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_WORLDS = 37


def _emulated():
    import torch

    return getattr(torch.cuda, "_newton_emulated", False)


def _needs_device():
    import torch

    if not torch.cuda.is_available() or _emulated():
        pytest.skip("needs the device (not emulated)")


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


_CASES = {}


def _posed(name, E=N_WORLDS, seed=31):
    """GPU model, a state posed by the device eval_fk from random joint coordinates, and the reference on its fp32 arrays (computed
    once per case and shared by the tests; nothing below writes the state)."""
    if (name, E, seed) not in _CASES:
        import newton_amd as nt

        model = SCENES[name](E, device=DEV)
        jq, jqd = random_joint_state(model, seed)
        s = model.state()
        s.joint_q, s.joint_qd = jq, jqd
        nt.eval_fk(model, jq, jqd, s)
        bq, bqd = _np(s.body_q), _np(s.body_qd)
        _CASES[(name, E, seed)] = (nt, model, s, jq, jqd, bq, bqd, reference(model, bq, jq))
    return _CASES[(name, E, seed)]


def _outputs(model, fill=POISON):
    import torch

    L, D, A = model.max_joints_per_articulation, model.max_dofs_per_articulation, model.articulation_count
    mk = lambda *shape: torch.full(shape, fill, dtype=torch.float32, device=DEV)  # noqa: E731
    return mk(A, 6 * L, D), mk(A, D, D), mk(model.joint_dof_count, 6), mk(model.body_count, 6, 6)


@pytest.mark.parametrize("name,E", [(n, N_WORLDS) for n in sorted(SCENES)] + [("multi_art", 1), ("quadruped", 1)])
def test_device_matches_reference(name, E):
    nt, model, s, jq, jqd, bq, bqd, ref = _posed(name, E)
    J, H, S, I = _outputs(model)  # noqa: E741
    assert nt.eval_jacobian(model, s, J, S) is J and nt.eval_mass_matrix(model, s, H, body_I_s=I) is H
    errs = jm_errors(model, ref, J, H, S, I)
    if E == N_WORLDS:
        tolerances.record(f"eval_jacobian_{name}", {"J_over_max_1_R": {"max": errs["J"]}, "S_over_max_1_R": {"max": errs["S"]}},
                          {"J_over_max_1_R": GATE, "S_over_max_1_R": GATE})
        tolerances.record(f"eval_mass_matrix_{name}", {"H_over_max_H": {"max": errs["H"]}, "I_over_max_I": {"max": errs["I"]}},
                          {"H_over_max_H": GATE, "I_over_max_I": GATE})
    assert within_gates(errs), (name, errs)
    assert structure_ok(model, ref, _np(J), _np(H))  # the poison is gone: padding / non-ancestor entries written as zero, H symmetric
    assert np.array_equal(_np(s.body_q), bq) and np.array_equal(_np(s.joint_q), jq)
    # allocating form: same bits
    assert np.array_equal(_np(nt.eval_jacobian(model, s)), _np(J)) and np.array_equal(_np(nt.eval_mass_matrix(model, s)), _np(H))


@pytest.mark.parametrize("name", sorted(SCENES))
def test_identities_with_the_device_eval_fk(name):
    """J @ joint_qd reproduces the state's own body_qd (device eval_fk), and qd^T H qd / 2 its kinetic energy."""
    nt, model, s, jq, jqd, bq, bqd, ref = _posed(name)
    J, H = nt.eval_jacobian(model, s), nt.eval_mass_matrix(model, s)

    class Got:
        pass

    got = Got()
    got.J, got.R, got.D = _np(J).astype(np.float64), ref.R, ref.D
    e_id = _link_identity_error(model, got, bq, jqd, bqd)
    ke = kinetic_energy(model, bq, bqd)
    e_ke = energy_error(model, _np(H), jqd, ke)
    print(f"[eval_jacobian gpu] {name}: |J qd - body_qd| / max(1, R) {e_id:.3e}, kinetic energy rel err {e_ke:.3e}")
    # a row of J carries an entry error of <= GATE * max(1, R) per column, times |qd|: |qd|_1 in all; the device eval_fk's own body_qd
    # is within the same gate (one more term); the angular part is carried to the COM (a factor <= 1 + R, 2 after the division by
    # max(1, R)).  Energy: H's entry error GATE * max|H_ref| summed over the quadratic form is GATE * max|H_ref| * |qd|_1^2 / 2, plus
    # GATE relative for the fp32 body_qd the energy itself is taken from
    qd_l1 = np.abs(jqd.reshape(model.env.env_count, -1)).sum(axis=1).max()
    assert e_id <= GATE * (qd_l1 + 1.0) * 2.0
    d_edges = np.concatenate([np.asarray(model.joint_qd_start), [model.joint_dof_count]])
    for a, (b, e) in enumerate(zip(model.articulation_start, model.articulation_end)):
        qd = jqd[d_edges[b]:d_edges[e]].astype(np.float64)
        got = 0.5 * qd @ _np(H)[a, :len(qd), :len(qd)].astype(np.float64) @ qd
        assert abs(got - ke[a]) <= 0.5 * GATE * np.abs(ref.H[a]).max() * np.abs(qd).sum() ** 2 + GATE * ke[a], (name, a)


@pytest.mark.parametrize("name", ["d6_zoo", "multi_art", "quadruped"])
def test_all_tiles_give_the_same_bits(name):
    nt, model, s, *_ = _posed(name)
    dm = model.device_model()
    d = s._desc()
    base = None
    for epb in (0, 1, 4, 8, 16):
        J, H, S, I = _outputs(model)  # noqa: E741
        st = dm.lib.nt_eval_jacobian_tile(C.byref(dm.desc), C.byref(d), J.data_ptr(), S.data_ptr(), None, epb, dm.stream())
        st2 = dm.lib.nt_eval_mass_matrix_tile(C.byref(dm.desc), C.byref(d), H.data_ptr(), I.data_ptr(), None, epb, dm.stream())
        assert st == 0 and st2 == 0, (epb, st, st2)
        got = [_np(x) for x in (J, H, S, I)]
        if base is None:
            base = got
        assert all(np.array_equal(a, b) for a, b in zip(base, got)), epb


def test_masked_call_into_poisoned_outputs():
    nt, model, s, *_ = _posed("multi_art")
    full = _outputs(model)
    nt.eval_jacobian(model, s, full[0], full[2])
    nt.eval_mass_matrix(model, s, full[1], body_I_s=full[3])
    sel = np.random.default_rng(1).random(model.articulation_count) < 0.5
    part = _outputs(model)
    nt.eval_jacobian(model, s, part[0], part[2], mask=sel)
    nt.eval_mass_matrix(model, s, part[1], body_I_s=part[3], mask=sel)
    dsel = np.repeat(sel, np.tile([6, 6, 2], N_WORLDS))
    bsel = np.repeat(sel, np.tile([1, 1, 2], N_WORLDS))
    for f, p, m in zip(full, part, (sel, sel, dsel, bsel)):
        f, p = _np(f), _np(p)
        assert np.array_equal(p[m], f[m]) and np.all(p[~m] == POISON)
    # the view's world mask
    view = nt.selection.ArticulationView(model, str(list(model.articulation_label)[2]))
    wsel = np.arange(N_WORLDS) % 3 == 0
    J2, H2 = _outputs(model)[:2]
    gJ, gH = _np(view.eval_jacobian(s, J2, mask=wsel)), _np(view.eval_mass_matrix(s, H2, mask=wsel))
    fJ, fH = _np(full[0]).reshape(N_WORLDS, 3, *full[0].shape[1:])[:, 2], _np(full[1]).reshape(N_WORLDS, 3, *full[1].shape[1:])[:, 2]
    assert np.array_equal(gJ[wsel], fJ[wsel]) and np.all(gJ[~wsel] == POISON)
    assert np.array_equal(gH[wsel], fH[wsel]) and np.all(gH[~wsel] == POISON)


def test_caller_tensors_no_allocation_no_synchronisation():
    _needs_device()
    import torch

    nt, model, s, *_ = _posed("quadruped")
    J, H, S, I = _outputs(model)  # noqa: E741
    nt.eval_jacobian(model, s, J, S)
    nt.eval_mass_matrix(model, s, H, body_I_s=I)
    torch.cuda.synchronize()
    want = [_np(x).copy() for x in (J, H, S, I)]
    for x in (J, H, S, I):
        x.fill_(POISON)
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        nt.eval_jacobian(model, s, J, S)
        nt.eval_mass_matrix(model, s, H, body_I_s=I)
        nt.eval_mass_matrix(model, s, H, J=J, body_I_s=I, joint_S_s=S)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.cuda.memory_stats(DEV)["allocation.all.allocated"] == before
    torch.cuda.synchronize()
    assert all(np.array_equal(a, _np(b)) for a, b in zip(want, (J, H, S, I)))


@pytest.mark.parametrize("backend", ["torch", "abi"])
def test_captured_frame_replays_bit_identically(backend):
    """{eval_fk; eval_jacobian; eval_mass_matrix} recorded once; joint_q changed; the replay equals the direct calls bit for bit."""
    _needs_device()
    import torch

    import newton_amd as nt

    model = SCENES["quadruped"](64, device=DEV)
    jq, jqd = random_joint_state(model, 3)
    s = model.state()
    s.joint_q, s.joint_qd = jq, jqd
    dm = model.device_model()
    J, H, S, I = _outputs(model)  # noqa: E741

    def frame():
        d = s._desc()
        st = dm.lib.nt_eval_fk(C.byref(dm.desc), s._soa["joint_q"].data_ptr(), s._soa["joint_qd"].data_ptr(), C.byref(d), dm.stream())
        assert st == 0
        nt.eval_jacobian(model, s, J, S)
        nt.eval_mass_matrix(model, s, H, body_I_s=I)

    g = nt.graph.capture(frame, warmup=1, backend=backend)
    torch.cuda.synchronize()
    first = _np(J).copy()
    s._soa["joint_q"][0, 7:, :] += 0.25  # the twelve leg angles of every world
    g.launch()
    torch.cuda.synchronize()
    replay = [_np(x).copy() for x in (J, H, S, I, s.body_q)]
    assert np.abs(replay[0] - first).max() > 1e-2
    for x in (J, H, S, I):
        x.fill_(POISON)
    frame()
    torch.cuda.synchronize()
    assert all(np.array_equal(a, _np(b)) for a, b in zip(replay, (J, H, S, I, s.body_q)))


def test_heterogeneous_model():
    """quadrupeds | box stacks | pendulums: one launch per world group into its slice of the global outputs, padded to the global L, D."""
    import newton_amd as nt
    from test_heterogeneous_worlds import mixed_model

    model = mixed_model((("quadruped", 2), ("boxes3", 1), ("pendulum", 2), ("quadruped", 1)), device=DEV)
    assert model.is_heterogeneous
    states = [random_joint_state(p, 2 + i) for i, p in enumerate(model.world_groups.parts)]
    jq, jqd = np.concatenate([a for a, _ in states]), np.concatenate([b for _, b in states])
    s = model.state()
    s.joint_q, s.joint_qd = jq, jqd
    s.body_q, s.body_qd = nt.articulation.eval_fk_numpy(model, jq, jqd)
    bq = _np(s.body_q)
    ref = reference(model, bq, jq)
    J, H, S, I = _outputs(model)  # noqa: E741
    nt.eval_jacobian(model, s, J, S)
    nt.eval_mass_matrix(model, s, H, body_I_s=I)
    errs = jm_errors(model, ref, J, H, S, I)
    tolerances.record("eval_jacobian_heterogeneous", {"J_over_max_1_R": {"max": errs["J"]}, "S_over_max_1_R": {"max": errs["S"]}},
                      {"J_over_max_1_R": GATE, "S_over_max_1_R": GATE})
    tolerances.record("eval_mass_matrix_heterogeneous", {"H_over_max_H": {"max": errs["H"]}, "I_over_max_I": {"max": errs["I"]}},
                      {"H_over_max_H": GATE, "I_over_max_I": GATE})
    assert within_gates(errs), errs
    assert structure_ok(model, ref, _np(J), _np(H))
    sel = np.arange(model.articulation_count) % 2 == 0
    Jm, Hm = _outputs(model)[:2]
    nt.eval_jacobian(model, s, Jm, mask=sel)
    nt.eval_mass_matrix(model, s, Hm, mask=sel)
    assert np.array_equal(_np(Jm)[sel], _np(J)[sel]) and np.all(_np(Jm)[~sel] == POISON)
    assert np.array_equal(_np(Hm)[sel], _np(H)[sel]) and np.all(_np(Hm)[~sel] == POISON)


def test_after_xpbd_steps_of_lowered_quadrupeds():
    """Step, eval_ik, eval_jacobian.  The solver leaves the joints slightly violated and eval_ik projects, so J joint_qd reproduces the
    stepped body_qd of the leaf links (the feet) only up to that violation.  The violation is measured independently of the kernels
    under test: the residual of the identity with the float64 reference Jacobian on the same state.  The device residual may exceed it
    by what the entry gate allows over a row: GATE * max(1, R) per entry times |qd|_1, the angular part carried to the COM (a factor
    1 + R)."""
    import newton_amd as nt
    from scenes import quadruped_scene

    E = N_WORLDS
    model = quadruped_scene(E, device=DEV)
    model.joint_q.reshape(E, -1)[:, 2] -= 0.26
    model.body_q, model.body_qd = nt.articulation.eval_fk_numpy(model, model.joint_q, model.joint_qd)
    pipe = nt.CollisionPipeline(model)
    contacts, solver = pipe.contacts(), nt.solvers.SolverXPBD(model, iterations=2)
    s0, s1, ctrl = model.state(), model.state(), model.control()
    ctrl.joint_f = np.random.default_rng(2).normal(0, 2.0, size=model.joint_dof_count).astype(np.float32)
    solver.rollout(s0, s1, ctrl, contacts, 1e-3, 6)  # (even: the result is in s0)
    nt.eval_ik(model, s0)
    J = _np(nt.eval_jacobian(model, s0)).astype(np.float64)
    bq, bqd, jq, jqd = (_np(getattr(s0, k)) for k in ("body_q", "body_qd", "joint_q", "joint_qd"))
    ref = reference(model, bq, jq)
    errs = jm_errors(model, ref, J)
    tolerances.record("eval_jacobian_after_xpbd_steps", {"J_over_max_1_R": {"max": errs["J"]}}, {"J_over_max_1_R": GATE})
    assert within_gates(errs), errs
    t = model.env
    leaves = [j for j in range(t.nj) if not np.any(t.joint_parent == t.joint_child[j])]
    assert len(leaves) == 4 and all(int(t.joint_type[j]) == int(nt.JointType.REVOLUTE) for j in leaves)
    com = np.asarray(model.body_com, dtype=np.float64).reshape(E, t.nb, 3)
    B, Bd, qd = bq.astype(np.float64).reshape(E, t.nb, 7), bqd.astype(np.float64).reshape(E, t.nb, 6), jqd.astype(np.float64).reshape(E, t.nd)
    from newton_amd.articulation import _qrot

    def residual(Jx):
        worst = np.zeros(E)
        for j in leaves:
            b = int(t.joint_child[j])
            vw = np.einsum("erc,ec->er", Jx[:, 6 * j:6 * j + 6, :], qd)
            c = B[:, b, :3] + _qrot(B[:, b, 3:], com[:, b])
            got = np.concatenate([vw[:, :3] + np.cross(vw[:, 3:], c), vw[:, 3:]], axis=1)
            worst = np.maximum(worst, np.abs(got - Bd[:, b]).max(axis=1))
        return worst

    violation, device = residual(ref.J), residual(J)
    allowance = GATE * np.maximum(1.0, ref.R) * np.abs(qd).sum(axis=1) * (1.0 + ref.R)
    print(f"[eval_jacobian gpu] after 6 XPBD substeps: joint violation (reference residual) max {violation.max():.3e}, device residual "
          f"max {device.max():.3e}, allowance over the violation max {allowance.max():.3e}, largest excess {np.max(device - violation):.3e}")
    assert np.all(device <= violation + allowance)
