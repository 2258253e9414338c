"""newton_amd.eval_ik on the device (nt_eval_ik, include/newton_hip_kinematics.h) against the float64 reference of
tests/test_eval_ik_host.py on identical fp32 body states.  Gates (see there): 1e-5 on coordinates, 1e-5 * max(1, V) on rates -- the
standing single-call kinematics gate of test_eval_fk_device_matches_oracle."""
import numpy as np
import pytest

import tolerances
from test_eval_ik_host import Q_GATE, QD_GATE, SCENES, ik_errors, ik_reference, random_joint_state, within_gates

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATES = {"coord": Q_GATE, "rate_over_scale": QD_GATE}


def _emulated():
    import torch

    return getattr(torch.cuda, "_newton_emulated", False)


def _needs_device():
    import torch

    if not torch.cuda.is_available() or _emulated():
        pytest.skip("needs the device (not emulated)")


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _posed(name, E, seed, fill=7.0):
    """GPU model + a state whose body arrays are eval_fk of random joint coordinates and whose joint arrays hold a fill value."""
    import newton_amd as nt

    model = SCENES[name](E, device=DEV)
    jq, jqd = random_joint_state(model, seed)
    s = model.state()
    nt.eval_fk(model, jq, jqd, s)
    s.joint_q = np.full(model.joint_coord_count, fill, np.float32)
    s.joint_qd = np.full(model.joint_dof_count, -fill, np.float32)
    return nt, model, s, jq, jqd


def _check(name, model, s, bq, bqd):
    rq, rqd, _, _ = ik_reference(model, bq, bqd)
    errs = ik_errors(model, _np(s.joint_q), _np(s.joint_qd), rq, rqd, bqd)
    tolerances.record(name, {"coord": {"max": errs[0]}, "rate_over_scale": {"max": errs[1]}}, GATES)
    assert within_gates(errs), (name, errs)


@pytest.mark.parametrize("name,E", [(n, 37) for n in sorted(SCENES)] + [("quadruped", 4096)])
def test_device_matches_reference(name, E):
    if E > 1000 and _emulated():
        pytest.skip("4096 worlds: hours in emulation")
    nt, model, s, jq, jqd = _posed(name, E, 31)
    bq, bqd = _np(s.body_q), _np(s.body_qd)
    nt.eval_ik(model, s)
    _check(f"eval_ik_{name}_{E}", model, s, bq, bqd)
    # the in-place path reads the body state only
    assert np.array_equal(_np(s.body_q), bq) and np.array_equal(_np(s.body_qd), bqd)
    # round trip: what eval_fk was given
    assert within_gates(ik_errors(model, _np(s.joint_q), _np(s.joint_qd), jq.astype(np.float64), jqd.astype(np.float64), bqd))


def test_into_tensors_and_arrays():
    import torch

    nt, model, s, _jq, _jqd = _posed("d6_zoo", 37, 4)
    ref = model.state()
    ref.assign(s)
    nt.eval_ik(model, ref)
    out_q = torch.zeros(model.joint_coord_count, dtype=torch.float32, device=DEV)
    out_qd = np.zeros(model.joint_dof_count, dtype=np.float32)
    nt.eval_ik(model, s, out_q, out_qd)
    assert np.array_equal(_np(out_q), _np(ref.joint_q)) and np.array_equal(out_qd, _np(ref.joint_qd))
    assert np.all(_np(s.joint_q) == 7.0) and np.all(_np(s.joint_qd) == -7.0)


def _lowered_quadrupeds(E):
    import newton_amd as nt
    from scenes import quadruped_scene

    model = quadruped_scene(E, device=DEV)
    model.joint_q.reshape(E, -1)[:, 2] -= 0.26
    model.body_q, model.body_qd = nt.articulation.eval_fk_numpy(model, model.joint_q, model.joint_qd)
    return nt, model


def test_articulation_view_after_xpbd_steps():
    """The dof getters return the initial pose after XPBD steps; after eval_ik they match the reference on the stepped body state."""
    nt, model = _lowered_quadrupeds(37)
    pipe = nt.CollisionPipeline(model)
    contacts, solver = pipe.contacts(), nt.solvers.SolverXPBD(model, iterations=2)
    s0, s1, ctrl = model.state(), model.state(), model.control()
    ctrl.joint_f = np.random.default_rng(2).normal(0, 2.0, size=model.joint_dof_count).astype(np.float32)
    view = nt.selection.ArticulationView(model, "*")
    before = _np(view.get_dof_positions(s0)).copy()
    solver.rollout(s0, s1, ctrl, contacts, 1e-3, 20)
    assert np.array_equal(_np(view.get_dof_positions(s0)), before)  # the solver does not advance joint_q
    bq, bqd = _np(s0.body_q), _np(s0.body_qd)
    view.eval_ik(s0)
    assert np.abs(_np(view.get_dof_positions(s0)) - before).max() > 1e-3
    assert np.abs(_np(view.get_root_velocities(s0))).max() > 0.0
    _check("eval_ik_after_xpbd_rollout", model, s0, bq, bqd)
    rq, _, _, _ = ik_reference(model, bq, bqd)
    assert np.abs(_np(view.get_dof_positions(s0))[:, 7:] - rq.reshape(37, -1)[:, 7:]).max() <= Q_GATE
    # world mask
    s1.assign(s0)
    s1.joint_q = np.full(model.joint_coord_count, 7.0, np.float32)
    sel = np.arange(37) % 3 == 0
    view.eval_ik(s1, mask=sel)
    got = _np(view.get_dof_positions(s1))
    assert np.array_equal(got[sel], _np(view.get_dof_positions(s0))[sel]) and np.all(got[~sel] == 7.0)


def test_reproduces_featherstone_joint_state():
    """Independent cross-check: SolverFeatherstone advances joint_q / joint_qd itself and rebuilds the bodies from them."""
    nt, model = _lowered_quadrupeds(37)
    pipe = nt.CollisionPipeline(model)
    contacts, solver = pipe.contacts(), nt.solvers.SolverFeatherstone(model)
    s0, s1, ctrl = model.state(), model.state(), model.control()
    for _ in range(10):
        s0.clear_forces()
        pipe.collide(s0, contacts)
        solver.step(s0, s1, ctrl, contacts, 1e-3)
        s0, s1 = s1, s0
    want_q, want_qd, bqd = _np(s0.joint_q).astype(np.float64), _np(s0.joint_qd).astype(np.float64), _np(s0.body_qd)
    nt.eval_ik(model, s0)
    errs = ik_errors(model, _np(s0.joint_q), _np(s0.joint_qd), want_q, want_qd, bqd)
    tolerances.record("eval_ik_vs_featherstone_joint_state", {"coord": {"max": errs[0]}, "rate_over_scale": {"max": errs[1]}}, GATES)
    assert within_gates(errs), errs


def test_mask_and_indices():
    nt, model, s, _jq, _jqd = _posed("free_child", 37, 9)
    full = model.state()
    full.assign(s)
    nt.eval_ik(model, full)
    fq, fqd = _np(full.joint_q).reshape(37, -1), _np(full.joint_qd).reshape(37, -1)
    sel = np.random.default_rng(1).random(37) < 0.5
    for kw in ({"mask": sel}, {"indices": np.flatnonzero(sel)}):
        part = model.state()
        part.assign(s)
        nt.eval_ik(model, part, **kw)
        q, qd = _np(part.joint_q).reshape(37, -1), _np(part.joint_qd).reshape(37, -1)
        assert np.array_equal(q[sel], fq[sel]) and np.array_equal(qd[sel], fqd[sel])
        assert np.all(q[~sel] == 7.0) and np.all(qd[~sel] == -7.0)
    with pytest.raises(ValueError, match="'mask' and 'indices' cannot be used together"):
        nt.eval_ik(model, s, mask=sel, indices=[0])


def test_heterogeneous_model():
    """quadrupeds | box stacks | pendulums: one launch per world group into the GroupedState."""
    import newton_amd as nt
    from test_heterogeneous_worlds import LAYOUT, mixed_model

    layout = (("quadruped", 1), ("boxes3", 2), ("pendulum", 1), ("boxes2", 1)) if _emulated() else LAYOUT
    model = mixed_model(layout, device=DEV)
    assert model.is_heterogeneous
    pipe = nt.CollisionPipeline(model)
    contacts, solver = pipe.contacts(), nt.solvers.SolverXPBD(model, iterations=2)
    s0, s1, ctrl = model.state(), model.state(), model.control()
    for _ in range(6):
        s0.clear_forces()
        pipe.collide(s0, contacts)
        solver.step(s0, s1, ctrl, contacts, 1e-3)
        s0, s1 = s1, s0
    bq, bqd = _np(s0.body_q), _np(s0.body_qd)
    nt.eval_ik(model, s0)
    gq, gqd = _np(s0.joint_q), _np(s0.joint_qd)
    assert np.array_equal(_np(s0.body_q), bq)
    parts = model.world_groups.parts
    cut = lambda a, key, w: np.split(a.reshape(-1, w) if w > 1 else a, np.cumsum([getattr(p, key) for p in parts])[:-1])  # noqa: E731
    worst = [0.0, 0.0]
    for p, pbq, pbqd, pq, pqd in zip(parts, cut(bq, "body_count", 7), cut(bqd, "body_count", 6), cut(gq, "joint_coord_count", 1),
                                    cut(gqd, "joint_dof_count", 1)):
        rq, rqd, _, _ = ik_reference(p, pbq, pbqd)
        e = ik_errors(p, pq, pqd, rq, rqd, pbqd)
        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
    tolerances.record("eval_ik_heterogeneous", {"coord": {"max": worst[0]}, "rate_over_scale": {"max": worst[1]}}, GATES)
    assert within_gates(worst), worst
    # selection over the global articulation ids
    sel = np.arange(model.articulation_count) % 2 == 0
    s1.assign(s0)
    s1.joint_q = np.full(model.joint_coord_count, 7.0, np.float32)
    nt.eval_ik(model, s1, mask=sel)
    art = np.asarray(model.joint_articulation)
    q_edges = np.concatenate([np.asarray(model.joint_q_start), [model.joint_coord_count]])
    coord_sel = np.concatenate([np.full(q_edges[j + 1] - q_edges[j], art[j] >= 0 and sel[art[j]]) for j in range(len(art))])
    got = _np(s1.joint_q)
    assert np.array_equal(got[coord_sel], gq[coord_sel]) and np.all(got[~coord_sel] == 7.0)


def test_no_host_synchronisation():
    _needs_device()
    import torch

    nt, model, s, _jq, _jqd = _posed("quadruped", 64, 5)
    nt.eval_ik(model, s)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        nt.eval_ik(model, s)
        nt.selection.ArticulationView(model, "*").eval_ik(s)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()


@pytest.mark.parametrize("backend", ["torch", "abi"])
def test_captured_frame_replays_bit_identically(backend):
    """One frame {rollout; eval_ik} recorded with newton_amd.graph.capture and replayed twice == the eager calls, bit for bit.  A
    capture refuses host synchronisation and (backend "abi") allocation inside the frame."""
    _needs_device()
    import torch

    substeps, frames = 4, 3
    out = {}
    for mode in ("eager", "graph"):
        nt, model = _lowered_quadrupeds(64)
        pipe = nt.CollisionPipeline(model)
        contacts, solver = pipe.contacts(), nt.solvers.SolverXPBD(model, iterations=2)
        s0, s1, ctrl = model.state(), model.state(), model.control()

        def frame():
            solver.rollout(s0, s1, ctrl, contacts, 1e-3, substeps)  # (even: the result is in s0)
            nt.eval_ik(model, s0)

        if mode == "eager":
            for _ in range(frames):
                frame()
        else:
            g = nt.graph.capture(frame, warmup=1, backend=backend, contacts=contacts)  # the warm-up frame is the eager run's first
            for _ in range(frames - 1):
                g.launch()
        torch.cuda.synchronize()
        out[mode] = [_np(getattr(s0, k)).copy() for k in ("body_q", "body_qd", "joint_q", "joint_qd")]
    assert np.abs(out["eager"][2] - np.asarray(model.joint_q)).max() > 1e-4
    for a, b in zip(out["eager"], out["graph"]):
        assert np.array_equal(a, b)
