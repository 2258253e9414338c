"""GPU: SolverFeatherstone(update_mass_matrix_interval > 1) with three articulations per world, through the Python surface.

Same scenes, references, gates and guard-buffer pattern as tests/test_fs_factor_cache_emu.py, which runs every (scene, mode, width) used
here on the emulated kernels first.  The solver's factor cache is replaced by the first nd * max_art_dofs rows of a larger
sentinel-filled tensor (same base pointer), so a row bound that runs past the documented rows lands in memory the test owns."""
import numpy as np
import pytest

import tolerances
from test_fs_factor_cache_emu import (DT, FIELDS, GATES, INTERVAL, N_ENV, SENTINEL, assert_sensitive, check_guard, factor_rows,
                                       oracle_run)
from test_gpu_parity_xpbd import _rel

pytestmark = pytest.mark.gpu


def _model(name):
    from scenes import multi_articulation_scene

    return multi_articulation_scene(N_ENV, device="cuda:0", variant=name)


def _solver(model, mode, epb, interval=INTERVAL):
    """The solver with its factor cache inside a guard buffer: [max(nd W, nd (nd + 1) / 2) + 8][env_stride] sentinels."""
    import torch

    import newton_amd as nt

    solver = nt.solvers.SolverFeatherstone(model, update_mass_matrix_interval=interval, envs_per_block=epb, mass_matrix=mode)
    t = model.env
    doc = t.nd * t.max_art_dofs
    assert tuple(solver._factor_cache.shape) == (doc, t.env_stride)
    big = torch.full((max(doc, t.nd * (t.nd + 1) // 2) + 8, t.env_stride), float(SENTINEL), dtype=torch.float32,
                     device=solver._factor_cache.device)
    solver._factor_cache = big[:doc]
    assert solver._factor_cache.data_ptr() == big.data_ptr()
    return solver, big


def _guard_ok(big, model, mode):
    import torch

    torch.cuda.synchronize()
    check_guard(big.cpu().numpy(), model.env, mode == "dense")


def _loop(model, solver, steps, states=None, notify_before=()):
    import newton_amd as nt

    pipe = nt.CollisionPipeline(model)
    contacts = pipe.contacts()
    s0, s1 = states if states is not None else (model.state(), model.state())
    for k in range(steps):
        if k in notify_before:
            solver.notify_model_changed(0)  # no property flag: nothing is uploaded again, only the factor is marked stale
            assert solver._mass_matrix_dirty
        s0.clear_forces()
        pipe.collide(s0, contacts)
        solver.step(s0, s1, None, contacts, DT)
        assert not solver._mass_matrix_dirty
        s0, s1 = s1, s0
    return s0, s1, contacts


def _fields(state):
    return {f: getattr(state, f).cpu().numpy().copy() for f in FIELDS}


def _check_against_oracle(test, got, want):
    errs = {f: _rel(got[f], want[f]) for f in FIELDS}
    tolerances.record(test, errs, GATES)
    for f in FIELDS:
        assert errs[f] <= GATES[f], (test, f, errs[f], GATES[f])


@pytest.mark.parametrize("mode", ["tree", "dense"])
@pytest.mark.parametrize("name", ["mixed", "free3"])
def test_cache_writes_stay_inside_the_documented_rows(oracle_lib, name, mode):
    """Interval 2: 4 step calls (save at 0 and 2, reload at 1 and 3), then a rollout of 3 (steps 4 .. 6: save, reload, save)."""
    model = _model(name)
    solver, big = _solver(model, mode, 0, interval=2)
    s0, s1, contacts = _loop(model, solver, 4)
    _guard_ok(big, model, mode)
    solver.rollout(s0, s1, None, contacts, DT, 3)
    assert solver._step == 7 and not solver._mass_matrix_dirty
    _guard_ok(big, model, mode)


@pytest.mark.parametrize("kind,epb,mode", [("step", 0, "tree"), ("step", 1, "tree"), ("step", 8, "tree"), ("step", 0, "dense"),
                                           ("step", 1, "dense"), ("step", 8, "dense"), ("rollout", 0, "tree"),
                                           ("rollout", 16, "tree"), ("rollout", 0, "dense")])
@pytest.mark.parametrize("name", ["mixed", "free3"])
def test_stale_factor_steps_match_the_oracle(oracle_lib, name, kind, epb, mode):
    """7 open-loop steps at interval 3 (rebuilds at 0, 3, 6) vs the oracle at interval 3, launch by launch and as one fused rollout;
    the rollout at 16 is the uniform-parameter tile of 16 environments on 512 lanes.  Gates: test_free_bodies_single_step's 1e-5 on
    joint_q / body_q and 1e-4 on joint_qd / body_qd, after the scene has shown that the oracle's own interval-1 and interval-3
    results lie >= 50 gates apart (measured: "mixed" 139 gates on joint_q and 4 698 on joint_qd, "free3" 74 and 2 443).
    Measured maxima on the device, open loop, the same at every width and for step and rollout (joint_q / joint_qd; body_q and body_qd
    no larger): "mixed" tree 2.1e-7 / 7.3e-5, dense 1.5e-7 / 1.1e-5; "free3" tree 1.2e-7 / 1.3e-5, dense 0 / 0 -- inside the gates, so
    no step is restarted from the oracle's state."""
    import newton_amd as nt

    want = oracle_run(name, 7, INTERVAL)
    assert_sensitive(name, oracle_run(name, 7, 1), want, "interval 1 vs 3, 7 steps")
    model = _model(name)
    solver, big = _solver(model, mode, epb)
    if kind == "step":
        out, _, _ = _loop(model, solver, 7)
    else:
        if epb == 16:
            assert model.env.np_analytic == model.env.np  # (with uniform parameters: what the tile of 16 asks for)
        pipe = nt.CollisionPipeline(model)
        contacts = pipe.contacts()
        out = solver.rollout(model.state(), model.state(), None, contacts, DT, 7)
        assert not solver._mass_matrix_dirty
    assert solver._step == 7
    got = _fields(out)
    _guard_ok(big, model, mode)
    _check_against_oracle(f"fs factor cache {name} {kind} epb={epb} {mode}", got, want)


@pytest.mark.parametrize("epb,mode", [(0, "tree"), (16, "tree"), (0, "dense")])
@pytest.mark.parametrize("name", ["mixed", "free3"])
def test_fused_rollout_is_the_step_loop_across_two_calls(name, epb, mode):
    """rollout(7) + rollout(4) == 11 x {clear_forces; collide; step; swap}, bit for bit, the factor cache included."""
    import newton_amd as nt

    model = _model(name)
    loop_solver, loop_big = _solver(model, mode, epb)
    want, _, _ = _loop(model, loop_solver, 11)
    solver, big = _solver(model, mode, epb)
    pipe = nt.CollisionPipeline(model)
    contacts = pipe.contacts()
    s0, s1 = model.state(), model.state()
    out = solver.rollout(s0, s1, None, contacts, DT, 7)
    assert out is s1
    out = solver.rollout(s1, s0, None, contacts, DT, 4)
    assert out is s1 and solver._step == 11
    _guard_ok(big, model, mode)
    _guard_ok(loop_big, model, mode)
    a, b = _fields(out), _fields(want)
    for f in FIELDS:
        assert np.array_equal(a[f], b[f]), f
    rows = factor_rows(model.env, mode == "dense")  # (the rest of the region is LDS left-overs, never read back as the factor)
    assert np.array_equal(big.cpu().numpy()[rows], loop_big.cpu().numpy()[rows])


@pytest.mark.parametrize("mode", ["tree", "dense"])
def test_notify_model_changed_forces_a_refresh(oracle_lib, mode):
    """notify_model_changed(0) before steps 1 and 5 of 6 on "mixed" vs the oracle forced at the same steps (the forced and the
    unforced oracle lie >= 50 gates apart: measured 65 gates on joint_q, 3 054 on joint_qd); the flag is consumed by step and by
    rollout.  Measured maxima on the device (joint_q / joint_qd): tree 1.5e-7 / 6.1e-5 (body_q 2.4e-7), dense 7.3e-8 / 6.0e-6."""
    name, forced = "mixed", (1, 5)
    want = oracle_run(name, 6, INTERVAL, forced)
    assert_sensitive(name, want, oracle_run(name, 6, INTERVAL), "forced at steps 1 and 5 vs unforced, 6 steps")
    model = _model(name)
    solver, big = _solver(model, mode, 0)
    out, other, contacts = _loop(model, solver, 6, notify_before=forced)
    got = _fields(out)
    _guard_ok(big, model, mode)
    _check_against_oracle(f"fs forced refresh {name} {mode}", got, want)
    solver.notify_model_changed(0)
    assert solver._mass_matrix_dirty
    solver.rollout(out, other, None, contacts, DT, 2)
    assert not solver._mass_matrix_dirty and solver._step == 8
    _guard_ok(big, model, mode)
