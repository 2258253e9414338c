"""newton_amd.eval_inverse_dynamics on the device (nt_eval_inverse_dynamics, include/newton_hip_kinematics.h) against the float64
finite-difference reference of tests/inverse_dynamics_reference.py evaluated on the same fp32 inputs.  Gate (see
tests/test_inverse_dynamics_host.py): |tau - tau_ref| / max(1, max|tau_ref| of the articulation) <= ID_GATE, 4 x the largest per-scene
maximum measured on the emulator.

Measured on the MI355X: see DESIGN.md (the per-scene table) and the test log; the bias-compensation ratios are recorded through
tests/tolerances."""
import ctypes as C

import numpy as np
import pytest

import tolerances
from inverse_dynamics_reference import id_error, inverse_dynamics_reference, random_rates
from test_eval_ik_host import random_joint_state
from test_eval_jacobian_host import POISON, SCENES
from test_inverse_dynamics_host import ID_GATE, compensation_scene, compensation_state, id_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_WORLDS = 37
BOTH = 3  # NT_ID_GRAVITY | NT_ID_VELOCITY


def _emulated():
    import torch

    return getattr(torch.cuda, "_newton_emulated", False)


def _needs_device():
    import torch

    if not torch.cuda.is_available() or _emulated():
        pytest.skip("needs the device (not emulated)")


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


_POSED = {}


def _posed(name, E=N_WORLDS, seed=21):
    """The shared case on a GPU model: a State holding eval_fk_numpy's fp32 body state and the case's joint_q / joint_qd, joint_qdd as a
    resident tensor (made once per case; nothing below writes them unless it says so)."""
    if (name, E, seed) not in _POSED:
        import torch

        import newton_amd as nt

        c = id_case(name, E, seed, device=DEV)
        s = c.model.state()
        s.body_q, s.body_qd, s.joint_q, s.joint_qd = c.bq, c.bqd, c.jq, c.qd
        _POSED[(name, E, seed)] = (nt, c, s, torch.from_numpy(c.qdd).to(DEV))
    return _POSED[(name, E, seed)]


def _tau(model, fill=POISON):
    import torch

    return torch.full((model.articulation_count, model.max_dofs_per_articulation), fill, dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("name,E", [(n, N_WORLDS) for n in sorted(SCENES)] + [("multi_art", 1), ("quadruped", 1)])
def test_device_matches_reference(name, E):
    nt, c, s, qdd = _posed(name, E)
    tau = _tau(c.model)
    assert nt.eval_inverse_dynamics(c.model, s, qdd, tau) is tau
    err = id_error(tau, c.ref())
    print(f"[eval_inverse_dynamics gpu] {name} E {E}: max |tau - tau_ref| / max(1, max|tau_ref|) {err:.3e}")
    if E == N_WORLDS:
        tolerances.record(f"eval_inverse_dynamics_{name}", {"tau_over_max_1_tau": {"max": err}}, {"tau_over_max_1_tau": ID_GATE})
    assert err <= ID_GATE, (name, err)
    got = _np(tau)
    assert all(np.all(got[a, hi - lo:] == 0.0) for a, (lo, hi) in enumerate(c.dof_ranges))  # the poison is gone from the padding
    assert np.array_equal(_np(s.body_q), c.bq) and np.array_equal(_np(s.joint_qd), c.qd)  # the state is only read
    assert np.array_equal(_np(nt.eval_inverse_dynamics(c.model, s, qdd)), got)  # allocating form: same bits
    assert np.array_equal(_np(nt.eval_inverse_dynamics(c.model, s, c.qdd)), got)  # joint_qdd from the host: uploaded
    # the bias forces and their parts, on the scale of the whole result; both flags off: exactly zero
    for kw in (dict(), dict(velocity_terms=False), dict(gravity=False)):
        h = nt.eval_inverse_dynamics(c.model, s, **kw)
        assert id_error(h, c.ref(qdd=False, **kw), scale_ref=c.ref()) <= ID_GATE, (name, kw)
    assert np.all(_np(nt.eval_inverse_dynamics(c.model, s, tau=_tau(c.model), gravity=False, velocity_terms=False)) == 0.0)


@pytest.mark.parametrize("name", ["d6_zoo", "multi_art", "quadruped"])
def test_all_tiles_give_the_same_bits(name):
    nt, c, s, qdd = _posed(name)
    dm = c.model.device_model()
    d = s._desc()
    base = None
    for epb in (0, 1, 4, 8, 16):
        tau = _tau(c.model)
        st = dm.lib.nt_eval_inverse_dynamics_tile(C.byref(dm.desc), C.byref(d), qdd.data_ptr(), BOTH, tau.data_ptr(), None, epb, dm.stream())
        assert st == 0, (epb, st)
        got = _np(tau)
        if base is None:
            base = got
            assert np.array_equal(base, _np(nt.eval_inverse_dynamics(c.model, s, qdd)))
        assert np.array_equal(base, got), epb


def test_replicated_worlds_give_equal_bits():
    import torch

    nt, c, _s, _qdd = _posed("quadruped")
    t = c.model.env
    E = t.env_count
    rep = lambda x, n: np.tile(np.asarray(x).reshape(E, n, -1)[0], (E, 1, 1)).reshape(np.asarray(x).shape)  # noqa: E731
    s = c.model.state()
    s.body_q, s.body_qd, s.joint_q, s.joint_qd = rep(c.bq, t.nb), rep(c.bqd, t.nb), rep(c.jq, t.nc), rep(c.qd, t.nd)
    qdd = torch.from_numpy(np.ascontiguousarray(rep(c.qdd, t.na))).to(DEV)
    tau = _np(nt.eval_inverse_dynamics(c.model, s, qdd)).reshape(E, t.na, -1)
    assert np.all(tau == tau[:1]) and np.abs(tau).max() > 1.0


def test_masked_call_into_poisoned_output():
    nt, c, s, qdd = _posed("multi_art")
    full = _np(nt.eval_inverse_dynamics(c.model, s, qdd))
    sel = np.random.default_rng(1).random(c.model.articulation_count) < 0.5
    part = _np(nt.eval_inverse_dynamics(c.model, s, qdd, _tau(c.model), mask=sel))
    assert sel.any() and not sel.all()
    assert np.array_equal(part[sel], full[sel]) and np.all(part[~sel] == POISON)
    view = nt.selection.ArticulationView(c.model, str(list(c.model.articulation_label)[2]))
    wsel = np.arange(N_WORLDS) % 3 == 0
    got = _np(view.eval_inverse_dynamics(s, qdd, _tau(c.model), mask=wsel))
    want = full.reshape(N_WORLDS, 3, -1)[:, 2]
    assert np.array_equal(got[wsel], want[wsel]) and np.all(got[~wsel] == POISON)


def test_heterogeneous_model():
    """quadrupeds | box stacks | pendulums: one launch per world group into its slice of the global tau, padded to the global D."""
    import newton_amd as nt
    from test_heterogeneous_worlds import mixed_model

    model = mixed_model((("quadruped", 2), ("boxes3", 1), ("pendulum", 2), ("quadruped", 1)), device=DEV)
    assert model.is_heterogeneous
    parts = model.world_groups.parts
    jq = np.concatenate([random_joint_state(p, 2 + i)[0] for i, p in enumerate(parts)])
    D = int(model.max_dofs_per_articulation)
    qd, qdd = random_rates(model, 9, D)
    s = model.state()
    s.joint_q, s.joint_qd = jq, qd
    s.body_q, s.body_qd = nt.articulation.eval_fk_numpy(model, jq, qd)
    bq = _np(s.body_q)
    tau = nt.eval_inverse_dynamics(model, s, qdd, _tau(model))
    want = np.zeros((model.articulation_count, D))
    b0 = c0 = d0 = a0 = 0
    for p in parts:
        b1, c1, d1, a1 = b0 + p.body_count, c0 + p.joint_coord_count, d0 + p.joint_dof_count, a0 + p.articulation_count
        if p.articulation_count:
            Dp = int(p.max_dofs_per_articulation)
            want[a0:a1, :Dp] = inverse_dynamics_reference(p, bq[b0:b1], jq[c0:c1], qd[d0:d1], qdd[a0:a1, :Dp])
        b0, c0, d0, a0 = b1, c1, d1, a1
    err = id_error(tau, want)
    tolerances.record("eval_inverse_dynamics_heterogeneous", {"tau_over_max_1_tau": {"max": err}}, {"tau_over_max_1_tau": ID_GATE})
    assert err <= ID_GATE, err
    got = _np(tau)
    assert np.all(got[np.abs(want).max(axis=1) == 0.0] == 0.0)
    sel = np.arange(model.articulation_count) % 2 == 0
    part = _np(nt.eval_inverse_dynamics(model, s, qdd, _tau(model), mask=sel))
    assert np.array_equal(part[sel], got[sel]) and np.all(part[~sel] == POISON)


def test_caller_tensors_no_allocation_no_synchronisation():
    _needs_device()
    import torch

    nt, c, s, qdd = _posed("quadruped")
    tau = _tau(c.model)
    nt.eval_inverse_dynamics(c.model, s, qdd, tau)
    torch.cuda.synchronize()
    want = _np(tau).copy()
    tau.fill_(POISON)
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        nt.eval_inverse_dynamics(c.model, s, qdd, tau)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.cuda.memory_stats(DEV)["allocation.all.allocated"] == before
    torch.cuda.synchronize()
    assert np.array_equal(want, _np(tau))


@pytest.mark.parametrize("backend", ["torch", "abi"])
def test_captured_call_replays_bit_identically(backend):
    """eval_inverse_dynamics into a caller tensor recorded once; joint_qdd and the state changed in place; the replay equals the direct
    call bit for bit."""
    _needs_device()
    import torch

    import newton_amd as nt

    model = SCENES["quadruped"](64, device=DEV)
    jq, _ = random_joint_state(model, 3)
    D = int(model.max_dofs_per_articulation)
    qd, qdd_host = random_rates(model, 5, D)
    s = model.state()
    s.joint_q, s.joint_qd = jq, qd
    nt.eval_fk(model, jq, qd, s)
    qdd, tau = torch.from_numpy(qdd_host).to(DEV), _tau(model)

    def frame():
        nt.eval_inverse_dynamics(model, s, qdd, tau)

    g = nt.graph.capture(frame, warmup=1, backend=backend)
    torch.cuda.synchronize()
    first = _np(tau).copy()
    qdd.mul_(-0.5)
    s._soa["joint_qd"][0, 6:, :] += 0.25  # the twelve leg rates of every world
    s._soa["joint_q"][0, 7:, :] += 0.25  # and the leg angles (body_q stays: the links' own columns move with joint_q only for D6)
    g.launch()
    torch.cuda.synchronize()
    replay = _np(tau).copy()
    assert np.abs(replay - first).max() > 1e-2
    tau.fill_(POISON)
    frame()
    torch.cuda.synchronize()
    assert np.array_equal(replay, _np(tau))


def test_after_xpbd_steps_of_lowered_quadrupeds():
    """Step, eval_ik, eval_inverse_dynamics: the state a control loop sees.  The reference is evaluated on the same stepped fp32 arrays
    (body_q, and the joint_q / joint_qd eval_ik projected out of it)."""
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
    D = int(model.max_dofs_per_articulation)
    _, qdd = random_rates(model, 4, D)
    tau = nt.eval_inverse_dynamics(model, s0, qdd)
    bq, jq, jqd = (_np(getattr(s0, k)) for k in ("body_q", "joint_q", "joint_qd"))
    want = inverse_dynamics_reference(model, bq, jq, jqd, qdd)
    # The solver leaves the joints slightly violated (up to a centimetre here) and eval_ik projects: body_q is not eval_fk(joint_q) any
    # more.  The kernel takes every pivot and axis from body_q; so does the reference, whose trajectory carries the given poses
    # (inverse_dynamics_reference.carried_model): the plain gate holds.
    err = id_error(tau, want)
    print(f"[eval_inverse_dynamics gpu] after 6 XPBD substeps + eval_ik: {err:.3e} (max|tau_ref| {np.abs(want).max():.1f})")
    tolerances.record("eval_inverse_dynamics_after_xpbd_steps", {"tau_over_max_1_tau": {"max": err}}, {"tau_over_max_1_tau": ID_GATE})
    assert err <= ID_GATE, err


@pytest.mark.parametrize("kind", ["pendulum3", "rpr"])
def test_bias_forces_cancel_in_the_featherstone_step(kind):
    """control.joint_f = h(q, qd): the solver's qdd = (H + armature)^-1 (tau - h) is zero up to the fp32 rounding of tau (~1e-6
    relative), so one step moves joint_qd at most 1e-3 of what it moves without the compensation.  Fixed-base chains of 1-dof joints:
    the case where the solver's convention and the public one coincide.  Measured ratios: tests/tolerances records them (CPU oracle,
    tests/test_inverse_dynamics_host.py: pendulum3 3.4e-06, rpr 4.5e-06)."""
    import newton_amd as nt

    model = compensation_scene(kind, 5, device=DEV)
    q, qd = compensation_state(model, 7)
    s_in, s_out = model.state(), model.state()
    s_in.joint_q, s_in.joint_qd = q, qd
    nt.eval_fk(model, q, qd, s_in)
    h = nt.eval_inverse_dynamics(model, s_in)  # [5, 3]: the dofs in order
    solver = nt.solvers.SolverFeatherstone(model, angular_damping=0.0)
    moved = []
    for joint_f in (_np(h).reshape(-1), np.zeros_like(qd)):
        ctrl = model.control()
        ctrl.joint_f = joint_f
        solver.step(s_in, s_out, ctrl, None, 1e-3)
        moved.append(float(np.abs(_np(s_out.joint_qd).astype(np.float64) - qd).max()))
    ratio = moved[0] / moved[1]
    print(f"[eval_inverse_dynamics gpu] {kind}: max|d qd| over one Featherstone step with joint_f = h {moved[0]:.3e}, with joint_f = 0 "
          f"{moved[1]:.3e}, ratio {ratio:.3e}")
    tolerances.record(f"eval_inverse_dynamics_compensation_{kind}", {"dqd_ratio": {"max": ratio}}, {"dqd_ratio": 1e-3})
    assert moved[1] > 1e-3 and moved[0] <= 1e-3 * moved[1]
