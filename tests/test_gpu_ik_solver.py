"""newton_amd.ik.IKSolver on the device (nt_ik_solve, include/newton_hip_kinematics.h) against the float64 host path of newton_amd.ik
on the same fp32 inputs: one-iteration parity (tests/ik_parity.py), convergence, tile widths, graph capture, round trip with the
stepper.  37 worlds unless stated."""
import ctypes as C

import numpy as np
import pytest

import tolerances
from ik_cases import (LIMITED_SCENES, OFFSET, SCENES, ik_case, make_objectives, objective_specs, pose_errors, targets_at,
                      violated_limit_rows)
from ik_parity import PARITY_GATE, long_chain, mirror_cost, one_iteration_ratio, reference_iteration

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_WORLDS = 37
POS_BOUND, ROT_BOUND = 1e-4, 1e-3  # fp32 FK along <= 13 links of ~1 m reach carries ~1e-6 m; two decades cover LM's last stalled steps
_CASES = {}


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _case(name, E=N_WORLDS):
    """GPU model + solver, the host twin (model + solver on the same fp32 targets), the start; computed once, solvers reset by users."""
    if (name, E) not in _CASES:
        import torch

        from newton_amd import ik

        model, q_star, targets, start = ik_case(name, E, 5, device=DEV)
        host_model = SCENES[name](E)
        if name in LIMITED_SCENES:  # test construction: the joint-limit rows are not all zero at the start
            probe = ik.IKSolver(host_model, make_objectives(name, host_model, targets))
            assert np.all(violated_limit_rows(probe, start) > 0) if name == "joint_zoo_free_root" else np.any(violated_limit_rows(probe, start) > 0)
        _CASES[(name, E)] = dict(model=model, solver=ik.IKSolver(model, make_objectives(name, model, targets)), host_model=host_model,
                                 host=ik.IKSolver(host_model, make_objectives(name, host_model, targets)), targets=targets,
                                 start=start, q_in=torch.from_numpy(start.astype(np.float32)).to(DEV))
    return _CASES[(name, E)]


@pytest.mark.parametrize("name", ["quadruped", "joint_zoo_free_root", "d6_zoo", "multi_art"])  # (the scenes of tests/test_ik_solver_emu.py)
def test_one_iteration_parity(name):
    import torch

    c = _case(name)
    c["solver"].reset()
    ref = reference_iteration(c["host"], c["start"])
    out = torch.full_like(c["q_in"], 7.0)
    c["solver"].step(c["q_in"], out, iterations=1)
    ratio = one_iteration_ratio(c["host"], c["start"], ref, _np(out))
    nd = c["model"].env.nd
    print(f"[ik gpu] {name}: max |d delta| / max(1, |delta|) / (2^-24 cond A) = {ratio.max():.3f} (nd^2 = {nd ** 2})")
    tolerances.record(f"ik_solver_{name}", {"delta_over_eps_cond": {"max": float(ratio.max())}}, {"delta_over_eps_cond": PARITY_GATE})
    assert ratio.max() <= nd ** 2  # beyond the textbook worst case of a Cholesky solve: a defect, not a number to adopt
    assert ratio.max() <= PARITY_GATE
    assert np.array_equal(_np(c["solver"].lambdas), np.where(ref["accept"], 0.05, 0.2).astype(np.float32))
    want, allowed = mirror_cost(c["host"], _np(out))
    assert np.all(np.abs(_np(c["solver"].costs) - want) <= allowed)


def test_one_iteration_parity_with_a_scaled_step():
    """step_size 0.6 on the scene whose every world violates a joint limit at the start."""
    import torch

    name, step = "joint_zoo_free_root", 0.6
    c = _case(name)
    c["solver"].reset()
    ref = reference_iteration(c["host"], c["start"], step)
    out = torch.full_like(c["q_in"], 7.0)
    c["solver"].step(c["q_in"], out, iterations=1, step_size=step)
    ratio = one_iteration_ratio(c["host"], c["start"], ref, _np(out))
    print(f"[ik gpu] {name} step {step}: max |d delta| / max(1, |delta|) / (2^-24 cond A) = {ratio.max():.3f}")
    tolerances.record(f"ik_solver_{name}_step06", {"delta_over_eps_cond": {"max": float(ratio.max())}}, {"delta_over_eps_cond": PARITY_GATE})
    assert ratio.max() <= PARITY_GATE
    assert np.array_equal(_np(c["solver"].lambdas), np.where(ref["accept"], 0.05, 0.2).astype(np.float32))
    want, allowed = mirror_cost(c["host"], _np(out))
    assert np.all(np.abs(_np(c["solver"].costs) - want) <= allowed)


def test_refusals_on_the_device():
    """A tile that does not fit the LDS (300 dofs: the packed J^T J of one world is 176 KB) is NotImplementedError at step, before any
    launch; an objective taken over from a solver of another world count is refused by its row count."""
    import torch

    from newton_amd import ik

    model = long_chain(300, device=DEV)
    solver = ik.IKSolver(model, [ik.IKObjectivePosition(299, OFFSET, np.zeros((1, 3), np.float32))])
    q = torch.zeros(300, dtype=torch.float32, device=DEV)
    with pytest.raises(NotImplementedError, match="NT_ERR_UNSUPPORTED"):
        solver.step(q, q, iterations=1)
    assert _np(solver.costs)[0] == 0.0 and _np(solver.lambdas)[0] == np.float32(0.1)
    c = _case("multi_art")
    taken = c["solver"].objectives[0]
    assert hasattr(taken.target_positions, "data_ptr")
    with pytest.raises(ValueError, match="rows"):
        ik.IKSolver(SCENES["multi_art"](3, device=DEV), [taken])


@pytest.mark.parametrize("name", sorted(SCENES))
def test_every_problem_converges_within_50_iterations(name):
    import torch

    c = _case(name)
    c["solver"].reset()
    out = torch.full_like(c["q_in"], 7.0)
    c["solver"].step(c["q_in"], out, iterations=0)
    cost_in = _np(c["solver"].costs).copy()
    c["solver"].step(c["q_in"], out, iterations=50)
    pos, rot = pose_errors(name, c["host_model"], _np(out).astype(np.float64), c["targets"])
    print(f"[ik gpu] {name}: position error max {pos.max():.3e} m, rotation error max {rot.max():.3e} rad after 50 iterations")
    tolerances.record(f"ik_solver_convergence_{name}", {"position_m": {"max": float(pos.max())}, "rotation_rad": {"max": float(rot.max())}},
                      {"position_m": POS_BOUND, "rotation_rad": ROT_BOUND})
    assert np.all(pos <= POS_BOUND) and np.all(rot <= ROT_BOUND)
    assert np.all(_np(c["solver"].costs) <= cost_in)
    want, allowed = mirror_cost(c["host"], _np(out))
    assert np.all(np.abs(_np(c["solver"].costs) - want) <= allowed)


def _tile(c, epb, iterations=12):
    import torch

    s = c["solver"]
    dm = c["model"].device_model()
    out = torch.full_like(c["q_in"], 7.0)
    lam = torch.full_like(s.lambdas, s.lambda_initial)
    cost = torch.full_like(s.costs, 7.0)
    st = dm.lib.nt_ik_solve_tile(C.byref(dm.desc), C.byref(s._problem), c["q_in"].data_ptr(), out.data_ptr(), lam.data_ptr(), cost.data_ptr(),
                                 iterations, 1.0, epb, dm.stream())
    assert st == 0, (epb, st)
    return [_np(x).copy() for x in (out, lam, cost)]


@pytest.mark.parametrize("name", ["quadruped", "d6_zoo", "multi_art"])
def test_all_tiles_give_the_same_bits(name):
    c = _case(name)
    base = _tile(c, 0)
    assert not np.any(base[0] == 7.0) and not np.any(base[2] == 7.0)
    for epb in (1, 4, 8, 16):
        got = _tile(c, epb)
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(base, got)), epb


def test_identical_worlds_give_identical_rows_and_one_world_model():
    import torch

    from newton_amd import ik

    name = "quadruped"
    model, q_star, targets, start = ik_case(name, N_WORLDS, 5, device=DEV)
    same_t = [None if t is None else np.tile(t[:1], (N_WORLDS, 1)) for t in targets]
    same_q = np.tile(start[:1], (N_WORLDS, 1)).astype(np.float32)
    solver = ik.IKSolver(model, make_objectives(name, model, same_t))
    q = torch.from_numpy(same_q).to(DEV)
    out = torch.empty_like(q)
    solver.step(q, out, iterations=12)
    got, lam, cost = _np(out), _np(solver.lambdas), _np(solver.costs)
    assert np.all(got.view(np.uint32) == got.view(np.uint32)[:1]) and np.all(lam == lam[0]) and np.all(cost == cost[0])
    assert not np.array_equal(got, same_q)
    # a 1-world model: the same problem, the same bits
    one, _, _, _ = ik_case(name, 1, 5, device=DEV)
    s1 = ik.IKSolver(one, make_objectives(name, one, [None if t is None else t[:1] for t in targets]))
    q1 = torch.from_numpy(same_q[:1].copy()).to(DEV)
    s1.step(q1, q1, iterations=12)
    assert np.array_equal(_np(q1).view(np.uint32), got[:1].view(np.uint32)) and _np(s1.costs)[0] == cost[0]


@pytest.mark.parametrize("backend", ["torch", "abi"])
def test_captured_step_replays_and_follows_in_place_targets(backend):
    import torch

    import newton_amd as nt
    from newton_amd import ik

    if not torch.cuda.is_available() or getattr(torch.cuda, "_newton_emulated", False):
        pytest.skip("needs the device (not emulated)")
    name = "quadruped"
    model, q_star, targets, start = ik_case(name, N_WORLDS, 5, device=DEV)
    solver = ik.IKSolver(model, make_objectives(name, model, targets))
    q_in = torch.from_numpy(start.astype(np.float32)).to(DEV)
    out = torch.full_like(q_in, 7.0)
    solver.step(q_in, out, iterations=20)
    torch.cuda.synchronize()
    direct = [_np(x).copy() for x in (out, solver.lambdas, solver.costs)]

    def frame():
        solver.lambdas.fill_(solver.lambda_initial)
        solver.step(q_in, out, iterations=20)

    out.fill_(7.0)
    g = nt.graph.capture(frame, warmup=1, backend=backend)
    out.fill_(float("nan"))  # poison: the replay overwrites every entry
    g.launch()
    torch.cuda.synchronize()
    assert all(np.array_equal(a.view(np.uint32), _np(b).view(np.uint32)) for a, b in zip(direct, (out, solver.lambdas, solver.costs)))
    # new targets written in place: the replay solves them
    q2 = ik_case(name, N_WORLDS, 6)[1]
    new_targets = targets_at(name, model, q2 * 0.5 + 0.5 * ik_case(name, N_WORLDS, 5)[1], np.float32)
    host_model = SCENES[name](N_WORLDS)
    for o, t in zip(solver.objectives, new_targets):
        if isinstance(o, ik.IKObjectivePosition):
            store = o.target_positions.data_ptr()
            o.set_target_positions(t)
            assert o.target_positions.data_ptr() == store
    new_targets = [t if kind == "position" else old for (kind, _), t, old in zip(objective_specs(name, model), new_targets, targets)]
    g.launch()
    torch.cuda.synchronize()
    replay = _np(out).copy()
    assert not np.array_equal(replay, direct[0])
    solver.reset()
    fresh = torch.empty_like(q_in)
    solver.step(q_in, fresh, iterations=20)
    assert np.array_equal(_np(fresh).view(np.uint32), replay.view(np.uint32))
    # in place: joint_q_in is joint_q_out
    solver.reset()
    buf = q_in.clone()
    solver.step(buf, buf, iterations=20)
    assert np.array_equal(_np(buf).view(np.uint32), replay.view(np.uint32))
    del host_model


def test_no_allocation_no_synchronisation():
    import torch

    if not torch.cuda.is_available() or getattr(torch.cuda, "_newton_emulated", False):
        pytest.skip("needs the device (not emulated)")
    c = _case("quadruped")
    out = torch.empty_like(c["q_in"])
    c["solver"].step(c["q_in"], out, iterations=2)
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        c["solver"].step(c["q_in"], out, iterations=2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.cuda.memory_stats(DEV)["allocation.all.allocated"] == before


def test_round_trip_with_the_stepper():
    """6 XPBD substeps, eval_ik, then an IKSolver whose targets are the current foot positions: joint_q stays, to the convergence bound."""
    import torch

    import newton_amd as nt
    from newton_amd import ik
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
    jq = _np(s0.joint_q).astype(np.float32).reshape(E, -1)
    specs = objective_specs("quadruped", model)
    targets = targets_at("quadruped", model, jq.astype(np.float64), np.float32)  # eval_fk's composition at the recovered joint_q
    iks = ik.IKSolver(model, make_objectives("quadruped", model, targets))
    q = torch.from_numpy(jq).to(DEV)
    out = torch.empty_like(q)
    iks.step(q, out, iterations=10)
    got = _np(out).astype(np.float64)
    pos, rot = pose_errors("quadruped", SCENES["quadruped"](E), got, targets)
    moved = np.abs(got - jq).max()
    print(f"[ik gpu] round trip: joint_q moved by max {moved:.3e}, foot error max {pos.max():.3e} m, base rotation error max {rot.max():.3e} rad")
    assert np.all(pos <= POS_BOUND) and np.all(rot <= ROT_BOUND) and moved <= POS_BOUND
    assert len(specs) == 6
