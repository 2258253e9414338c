"""newton_amd.eval_forward_dynamics on the device (nt_eval_forward_dynamics, include/newton_hip_kinematics.h) against the float64
reference of tests/forward_dynamics_reference.py evaluated on the same fp32 inputs.  Gate (see tests/test_forward_dynamics_host.py):
the normwise backward error eta <= FD_GATE, 4 x the largest per-scene maximum measured on the emulator.  The plain forward error and
cond(H_ref) are printed for the record; nothing asserts on them.

Measured on the MI355X: see DESIGN.md (the per-scene table) and the test log; tests/tolerances records every figure."""
import ctypes as C

import numpy as np
import pytest

import tolerances
from forward_dynamics_reference import fd_denominator, fd_eta, forward_dynamics_reference, random_forces
from inverse_dynamics_reference import random_rates
from test_eval_ik_host import random_joint_state
from test_eval_jacobian_host import POISON, SCENES
from test_forward_dynamics_host import (FD_GATE, FS_BOUND, FS_DT, N_WORLDS, fd_case, featherstone_ratio, massless_leaf_model, report)
from test_inverse_dynamics_host import ID_GATE, compensation_scene, compensation_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = 7  # NT_FD_GRAVITY | NT_FD_VELOCITY | NT_FD_BODY_F
INFO_POISON = -7


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
    """The shared case on a GPU model: a State holding eval_fk_numpy's fp32 body state, the case's joint_q / joint_qd and body_f;
    joint_f as a resident tensor (made once per case; nothing below writes them unless it says so)."""
    if (name, E, seed) not in _POSED:
        import torch

        import newton_amd as nt

        c = fd_case(name, E, seed, device=DEV)
        _POSED[(name, E, seed)] = (nt, c, _state(c, c.model), torch.from_numpy(c.joint_f).to(DEV))
    return _POSED[(name, E, seed)]


def _state(c, model, body_f=None):
    s = model.state()
    s.body_q, s.body_qd, s.joint_q, s.joint_qd = c.id.bq, c.id.bqd, c.id.jq, c.id.qd
    s.body_f = c.body_f if body_f is None else body_f
    return s


def _out(model, fill=POISON):
    import torch

    return torch.full((model.articulation_count, model.max_dofs_per_articulation), fill, dtype=torch.float32, device=DEV)


def _info(model):
    import torch

    return torch.full((model.articulation_count,), INFO_POISON, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("name,E", [(n, N_WORLDS) for n in sorted(SCENES)] + [("multi_art", 1), ("quadruped", 1)])
def test_device_matches_reference(name, E):
    nt, c, s, joint_f = _posed(name, E)
    qdd, info = _out(c.model), _info(c.model)
    assert nt.eval_forward_dynamics(c.model, s, joint_f, qdd, body_f=True, info=info) is qdd
    eta = report(f"gpu E {E}", name, qdd, c.ref())
    if E == N_WORLDS:
        tolerances.record(f"eval_forward_dynamics_{name}", {"eta": {"max": eta}}, {"eta": FD_GATE})
    assert eta <= FD_GATE, (name, eta)
    got = _np(qdd)
    assert np.all(_np(info) == 0)
    assert all(np.all(got[a, n:] == 0.0) for a, n in enumerate(c.nda))  # the poison is gone from the padding
    assert np.array_equal(_np(s.body_q), c.id.bq) and np.array_equal(_np(s.joint_qd), c.id.qd) and np.array_equal(_np(s.body_f), c.body_f)
    assert np.array_equal(_np(joint_f), c.joint_f)  # the inputs are only read
    assert np.array_equal(_np(nt.eval_forward_dynamics(c.model, s, joint_f, body_f=True)), got)  # allocating form: same bits
    assert np.array_equal(_np(nt.eval_forward_dynamics(c.model, s, c.joint_f, body_f=True)), got)  # joint_f from the host: uploaded
    # each part off against the reference with the same part removed; everything off: exactly zero
    for kw in (dict(gravity=False), dict(velocity_terms=False), dict(body_f=False)):
        part = nt.eval_forward_dynamics(c.model, s, joint_f, **{**dict(body_f=True), **kw})
        assert fd_eta(part, c.ref(**kw)) <= FD_GATE, (name, kw)
    assert fd_eta(nt.eval_forward_dynamics(c.model, s, None, body_f=True), c.ref(joint_f=False)) <= FD_GATE
    assert np.all(_np(nt.eval_forward_dynamics(c.model, s, None, _out(c.model), gravity=False, velocity_terms=False)) == 0.0)


def test_heterogeneous_model():
    """quadrupeds | box stacks | pendulums: one launch per world group into its slice of the global arrays, padded to the global D."""
    import newton_amd as nt
    from test_heterogeneous_worlds import mixed_model

    model = mixed_model((("quadruped", 2), ("boxes3", 1), ("pendulum", 2), ("quadruped", 1)), device=DEV)
    assert model.is_heterogeneous
    parts = model.world_groups.parts
    jq = np.concatenate([random_joint_state(p, 2 + i)[0] for i, p in enumerate(parts)])
    D = int(model.max_dofs_per_articulation)
    qd, _ = random_rates(model, 9, D)
    joint_f, body_f = random_forces(model, 10, D)
    s = model.state()
    s.joint_q, s.joint_qd, s.body_f = jq, qd, body_f
    s.body_q, s.body_qd = nt.articulation.eval_fk_numpy(model, jq, qd)
    bq = _np(s.body_q)
    info = _info(model)
    qdd = _np(nt.eval_forward_dynamics(model, s, joint_f, _out(model), body_f=True, info=info))
    assert np.all(_np(info) == 0)
    b0 = c0 = d0 = a0 = 0
    worst = 0.0
    for p in parts:
        b1, c1, d1, a1 = b0 + p.body_count, c0 + p.joint_coord_count, d0 + p.joint_dof_count, a0 + p.articulation_count
        if p.articulation_count:
            Dp = int(p.max_dofs_per_articulation)
            ref = forward_dynamics_reference(p, bq[b0:b1], jq[c0:c1], qd[d0:d1], joint_f[a0:a1, :Dp], body_f[b0:b1])
            worst = max(worst, fd_eta(qdd[a0:a1, :Dp], ref))
            assert np.all(qdd[a0:a1, Dp:] == 0.0)
        b0, c0, d0, a0 = b1, c1, d1, a1
    print(f"[eval_forward_dynamics gpu] heterogeneous: eta {worst:.3e}")
    tolerances.record("eval_forward_dynamics_heterogeneous", {"eta": {"max": worst}}, {"eta": FD_GATE})
    assert worst <= FD_GATE, worst
    sel = np.arange(model.articulation_count) % 2 == 0
    pinfo = _info(model)
    part = _np(nt.eval_forward_dynamics(model, s, joint_f, _out(model), body_f=True, info=pinfo, mask=sel))
    assert np.array_equal(part[sel], qdd[sel]) and np.all(part[~sel] == POISON)
    assert np.all(_np(pinfo)[sel] == 0) and np.all(_np(pinfo)[~sel] == INFO_POISON)


def test_after_xpbd_steps_of_lowered_quadrupeds():
    """Step, eval_ik, eval_forward_dynamics with body_f=True reading what the state holds: the state a control loop sees (joints
    violated by up to a centimetre).  The reference is evaluated on the same stepped fp32 arrays."""
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
    solver.rollout(s0, s1, ctrl, contacts, 1e-3, 6)  # (even: the result is in s0; the rollout leaves body_f cleared)
    nt.eval_ik(model, s0)
    D = int(model.max_dofs_per_articulation)
    joint_f, body_f = random_forces(model, 4, D)
    s0.body_f = body_f  # the wrenches a contact evaluation would have left
    info = _info(model)
    qdd = nt.eval_forward_dynamics(model, s0, joint_f, body_f=True, info=info)
    bq, jq, jqd, bf = (_np(getattr(s0, k)) for k in ("body_q", "joint_q", "joint_qd", "body_f"))
    assert np.array_equal(bf, body_f) and np.all(_np(info) == 0)
    ref = forward_dynamics_reference(model, bq, jq, jqd, joint_f, bf)
    eta = report("gpu", "after 6 XPBD substeps + eval_ik", qdd, ref)
    tolerances.record("eval_forward_dynamics_after_xpbd_steps", {"eta": {"max": eta}}, {"eta": FD_GATE})
    assert eta <= FD_GATE, eta


@pytest.mark.parametrize("name", ["quadruped", "joint_zoo_free_root", "d6_zoo"])
def test_device_round_trip_through_inverse_dynamics(name):
    """eval_inverse_dynamics(qdd = eval_forward_dynamics(joint_f)) against joint_f on the denominator of eta: each call is allowed its
    own gate on that scale."""
    nt, c, s, joint_f = _posed(name)
    qdd = nt.eval_forward_dynamics(c.model, s, joint_f)
    back = _np(nt.eval_inverse_dynamics(c.model, s, qdd)).astype(np.float64)
    err = float((np.abs(back - c.joint_f).max(axis=1) / fd_denominator(c.ref(body_f=False), qdd)).max())
    print(f"[eval_forward_dynamics gpu] {name}: ID(FD(joint_f)) - joint_f over the denominator {err:.3e}")
    tolerances.record(f"eval_forward_dynamics_round_trip_{name}", {"round_trip": {"max": err}}, {"round_trip": FD_GATE + ID_GATE})
    assert err <= FD_GATE + ID_GATE, err


@pytest.mark.parametrize("name", ["d6_zoo", "multi_art", "quadruped"])
def test_all_tiles_give_the_same_bits(name):
    nt, c, s, joint_f = _posed(name)
    dm = c.model.device_model()
    d = s._desc()
    base = None
    for epb in (0, 1, 4, 8, 16):
        qdd, info = _out(c.model), _info(c.model)
        st = dm.lib.nt_eval_forward_dynamics_tile(C.byref(dm.desc), C.byref(d), joint_f.data_ptr(), ALL, qdd.data_ptr(), info.data_ptr(), None,
                                                  epb, dm.stream())
        assert st == 0, (epb, st)
        got = _np(qdd)
        if base is None:
            base = got
            assert np.array_equal(base, _np(nt.eval_forward_dynamics(c.model, s, joint_f, body_f=True)))
        assert np.array_equal(base, got) and np.all(_np(info) == 0), epb


def test_replicated_worlds_give_equal_bits():
    import torch

    nt, c, _s, _f = _posed("quadruped")
    t = c.model.env
    E = t.env_count
    rep = lambda x, n: np.tile(np.asarray(x).reshape(E, n, -1)[0], (E, 1, 1)).reshape(np.asarray(x).shape)  # noqa: E731
    s = c.model.state()
    s.body_q, s.body_qd, s.joint_q, s.joint_qd = rep(c.id.bq, t.nb), rep(c.id.bqd, t.nb), rep(c.id.jq, t.nc), rep(c.id.qd, t.nd)
    s.body_f = rep(c.body_f, t.nb)
    joint_f = torch.from_numpy(np.ascontiguousarray(rep(c.joint_f, t.na))).to(DEV)
    qdd = _np(nt.eval_forward_dynamics(c.model, s, joint_f, body_f=True)).reshape(E, t.na, -1)
    assert np.all(qdd == qdd[:1]) and np.abs(qdd).max() > 1.0


def test_masked_call_into_poisoned_output():
    nt, c, s, joint_f = _posed("multi_art")
    full = _np(nt.eval_forward_dynamics(c.model, s, joint_f, body_f=True))
    sel = np.random.default_rng(1).random(c.model.articulation_count) < 0.5
    info = _info(c.model)
    part = _np(nt.eval_forward_dynamics(c.model, s, joint_f, _out(c.model), body_f=True, info=info, mask=sel))
    assert sel.any() and not sel.all()
    assert np.array_equal(part[sel], full[sel]) and np.all(part[~sel] == POISON)
    assert np.all(_np(info)[sel] == 0) and np.all(_np(info)[~sel] == INFO_POISON)
    view = nt.selection.ArticulationView(c.model, str(list(c.model.articulation_label)[2]))
    wsel = np.arange(N_WORLDS) % 3 == 0
    got = _np(view.eval_forward_dynamics(s, joint_f, _out(c.model), mask=wsel, body_f=True))
    want = full.reshape(N_WORLDS, 3, -1)[:, 2]
    assert np.array_equal(got[wsel], want[wsel]) and np.all(got[~wsel] == POISON)


def test_caller_tensors_no_allocation():
    _needs_device()
    import torch

    nt, c, s, joint_f = _posed("quadruped")
    qdd, info = _out(c.model), _info(c.model)
    nt.eval_forward_dynamics(c.model, s, joint_f, qdd, body_f=True, info=info)
    torch.cuda.synchronize()
    want = _np(qdd).copy()
    qdd.fill_(POISON)
    torch.cuda.synchronize()
    before, count = torch.cuda.memory_allocated(DEV), torch.cuda.memory_stats(DEV)["allocation.all.allocated"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            nt.eval_forward_dynamics(c.model, s, joint_f, qdd, body_f=True, info=info)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.cuda.memory_allocated(DEV) == before and torch.cuda.memory_stats(DEV)["allocation.all.allocated"] == count
    torch.cuda.synchronize()
    assert np.array_equal(want, _np(qdd))


@pytest.mark.parametrize("backend", ["torch", "abi"])
def test_captured_call_replays_bit_identically(backend):
    """One call into caller tensors recorded once (torch: torch.cuda.graph); joint_f updated in place; the replay equals the direct
    call bit for bit."""
    _needs_device()
    import torch

    import newton_amd as nt

    model = SCENES["quadruped"](64, device=DEV)
    jq, _ = random_joint_state(model, 3)
    D = int(model.max_dofs_per_articulation)
    qd, _ = random_rates(model, 5, D)
    f_host, body_f = random_forces(model, 6, D)
    s = model.state()
    s.joint_q, s.joint_qd, s.body_f = jq, qd, body_f
    nt.eval_fk(model, jq, qd, s)
    joint_f, qdd, info = torch.from_numpy(f_host).to(DEV), _out(model), _info(model)

    def frame():
        nt.eval_forward_dynamics(model, s, joint_f, qdd, body_f=True, info=info)

    g = nt.graph.capture(frame, warmup=1, backend=backend)
    torch.cuda.synchronize()
    first = _np(qdd).copy()
    g.launch()
    torch.cuda.synchronize()
    assert np.array_equal(first, _np(qdd))  # the replay of unchanged inputs: the same bits
    joint_f.mul_(-0.5)
    g.launch()
    torch.cuda.synchronize()
    replay = _np(qdd).copy()
    assert np.abs(replay - first).max() > 1e-2
    qdd.fill_(POISON)
    frame()
    torch.cuda.synchronize()
    assert np.array_equal(replay, _np(qdd)) and np.all(_np(info) == 0)


@pytest.mark.parametrize("name", ["multi_art", "quadruped"])
def test_world_isolation(name):
    """Run B multiplies joint_f and body_f by 1e6 (finite) and zeroes a leaf's mass and inertia in the worlds w % 3 == 1; every other
    world's joint_qdd and info carry run A's bits, and inside the edited worlds only the edited articulation reports."""
    nt, c, s, joint_f = _posed(name, seed=3)
    t = c.model.env
    qdd_a, info_a = _out(c.model), _info(c.model)
    nt.eval_forward_dynamics(c.model, s, joint_f, qdd_a, body_f=True, info=info_a)
    model, bad = massless_leaf_model(name, N_WORLDS, device=DEV)
    aggressor = np.arange(N_WORLDS) % 3 == 1
    f_b = c.joint_f.copy().reshape(N_WORLDS, t.na, -1)
    f_b[aggressor] *= np.float32(1e6)
    bf_b = c.body_f.copy().reshape(N_WORLDS, t.nb, 6)
    bf_b[aggressor] *= np.float32(1e6)
    assert np.all(np.isfinite(f_b)) and np.all(np.isfinite(bf_b))
    s_b = _state(c, model, bf_b.reshape(-1, 6))
    qdd_b, info_b = _out(model), _info(model)
    nt.eval_forward_dynamics(model, s_b, f_b.reshape(c.joint_f.shape), qdd_b, body_f=True, info=info_b)
    a, b = _np(qdd_a).reshape(N_WORLDS, t.na, -1), _np(qdd_b).reshape(N_WORLDS, t.na, -1)
    ia, ib = _np(info_a).reshape(N_WORLDS, t.na), _np(info_b).reshape(N_WORLDS, t.na)
    assert np.all(ia == 0) and np.all(np.isfinite(a))
    assert np.array_equal(a[~aggressor], b[~aggressor]) and np.array_equal(ia[~aggressor], ib[~aggressor])
    bad = bad.reshape(N_WORLDS, t.na)
    assert np.array_equal(ib > 0, bad)
    for w, k in zip(*np.nonzero(bad)):
        n = c.nda[w * t.na + k]
        assert np.all(np.isnan(b[w, k, :n])) and np.all(b[w, k, n:] == 0.0)
    assert np.all(np.isfinite(b[~bad]))


@pytest.mark.parametrize("kind", ["pendulum3", "rpr"])
def test_featherstone_step_moves_joint_qd_by_qdd_dt(kind):
    """SolverFeatherstone.step on the device, fixed-base chains of 1-dof joints without armature, limits, drives, damping or friction:
    (qd1 - qd0) / dt against joint_qdd, the bound of the bias-compensation test on the same scenes (the rounding of qd1 alone explains
    2^-24 max|qd| / dt ~ 1.5e-4)."""
    import newton_amd as nt

    model = compensation_scene(kind, 5, device=DEV)
    q, qd = compensation_state(model, 7)
    joint_f = np.random.default_rng(11).uniform(-10.0, 10.0, size=(5, 3)).astype(np.float32)
    s_in, s_out = model.state(), model.state()
    s_in.joint_q, s_in.joint_qd = q, qd
    nt.eval_fk(model, q, qd, s_in)
    qdd = _np(nt.eval_forward_dynamics(model, s_in, joint_f))
    ctrl = model.control()
    ctrl.joint_f = joint_f.reshape(-1)
    nt.solvers.SolverFeatherstone(model, angular_damping=0.0).step(s_in, s_out, ctrl, None, FS_DT)
    ratio = featherstone_ratio(qd, _np(s_out.joint_qd), qdd)
    print(f"[eval_forward_dynamics gpu] {kind}: max |(qd1 - qd0) / dt - qdd| / max(1, max|qdd|) over one Featherstone step {ratio:.3e}")
    tolerances.record(f"eval_forward_dynamics_featherstone_{kind}", {"acc_ratio": {"max": ratio}}, {"acc_ratio": FS_BOUND})
    assert np.abs(qdd).max() > 1.0 and ratio <= FS_BOUND
