"""SolverSemiImplicit.rollout on the device, public API only: one launch per frame == the loop
`clear_forces; pipeline.collide; solver.step; swap`, bit for bit on every body of every world, with the Contacts of the last
substep's collide; reproducible; graph-capturable; through the world groups of a heterogeneous model; and the launch-by-launch
path of models with an SDF leg."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FLAT = ("shape0", "shape1", "point0", "point1", "offset0", "offset1", "normal", "margin0", "margin1")


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _pendulum(n):
    from scenes import pendulum_scene

    return pendulum_scene(n, device="cuda:0", seed=11), None, 1e-3


def _quadruped(n):
    import newton_amd as nt
    from scenes import quadruped_scene

    model = quadruped_scene(n, device="cuda:0")
    model.joint_q.reshape(n, -1)[:, 2] -= 0.26  # lowered into contact
    model.body_q, model.body_qd = nt.articulation.eval_fk_numpy(model, model.joint_q, model.joint_qd)
    rng = np.random.default_rng(3)
    model.body_qd = (model.body_qd + rng.normal(0, 0.3, size=model.body_qd.shape)).astype(np.float32)
    return model, rng.normal(0, 1.0, size=model.joint_dof_count).astype(np.float32), 1e-4


def _box_stack(n):
    from scenes import box_stack_scene

    model = box_stack_scene(n, device="cuda:0")
    assert model.env.np_analytic < model.env.np  # the convex (MPR / GJK) variant of the kernel
    return model, None, 1e-4


def _d6_angular(n):
    from scenes import d6_angular_scene

    model = d6_angular_scene(n, device="cuda:0", seed=13, free_root=True)  # D6 joints with two and three angular axes
    return model, np.random.default_rng(4).normal(0, 0.5, size=model.joint_dof_count).astype(np.float32), 1e-4


SCENES = {"pendulum": _pendulum, "quadruped": _quadruped, "box_stack": _box_stack, "d6_angular": _d6_angular}


def _control(model, jf):
    ctrl = model.control()
    if jf is not None:
        ctrl.joint_f = jf
    return ctrl


def _loop(pipe, solver, s0, s1, ctrl, contacts, dt, substeps):
    for _ in range(substeps):
        s0.clear_forces()
        pipe.collide(s0, contacts)
        solver.step(s0, s1, ctrl, contacts, dt)
        s0, s1 = s1, s0
    return s0


def _check_rollout_equals_loop(model, jf, dt, substeps, min_contacts=0):
    import newton_amd as nt

    solver = nt.solvers.SolverSemiImplicit(model)
    pipe = nt.CollisionPipeline(model)
    ctrl = _control(model, jf)
    r0, r1, rct = model.state(), model.state(), pipe.contacts()
    out = solver.rollout(r0, r1, ctrl, rct, dt, substeps)
    assert out is (r1 if substeps % 2 else r0)
    l0, l1, lct = model.state(), model.state(), pipe.contacts()
    ref = _loop(pipe, solver, l0, l1, ctrl, lct, dt, substeps)
    assert ref is (l1 if substeps % 2 else l0)
    q = ref.body_q.cpu().numpy()
    assert np.isfinite(q).all() and not np.array_equal(q, np.asarray(model.body_q, np.float32))
    assert _same(out.body_q, ref.body_q) and _same(out.body_qd, ref.body_qd)
    assert not r0.body_f.cpu().numpy().any() and not r1.body_f.cpu().numpy().any()
    n = int(lct.rigid_contact_count.cpu().numpy()[0])
    assert int(rct.rigid_contact_count.cpu().numpy()[0]) == n and n >= min_contacts
    for k in FLAT:
        assert _same(getattr(rct, "rigid_contact_" + k), getattr(lct, "rigid_contact_" + k)), k
    assert _same(rct.rigid_contact_count_per_env, lct.rigid_contact_count_per_env)


@pytest.mark.parametrize("substeps", [6, 7])
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_rollout_equals_loop_bitwise(scene, substeps):
    model, jf, dt = SCENES[scene](37)
    _check_rollout_equals_loop(model, jf, dt, substeps, min_contacts=0 if scene in ("pendulum", "d6_angular") else 37)


def test_rollout_equals_loop_bitwise_at_full_size():
    """The quadruped at BASELINE.json's size: 4 096 worlds x 10 substeps, all feet in the ground."""
    import torch

    if getattr(torch.cuda, "_newton_emulated", False):
        pytest.skip("4 096 worlds take hours on the emulator (one OS thread per lane)")
    model, jf, dt = _quadruped(4096)
    _check_rollout_equals_loop(model, jf, dt, 10, min_contacts=4096 * 4)


def test_two_launches_give_identical_bits():
    import newton_amd as nt

    model, jf, dt = _quadruped(100)
    solver, pipe, ctrl = nt.solvers.SolverSemiImplicit(model), nt.CollisionPipeline(model), _control(model, jf)
    res = []
    for _ in range(2):
        s0, s1, ct = model.state(), model.state(), pipe.contacts()
        out = solver.rollout(s0, s1, ctrl, ct, dt, 9)
        res.append((out.body_q.cpu().numpy().copy(), out.body_qd.cpu().numpy().copy(),
                    *[getattr(ct, "rigid_contact_" + k).cpu().numpy().copy() for k in FLAT]))
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(*res))
    assert np.isfinite(res[0][0]).all()


def test_captured_rollout_replays_bit_identically():
    import torch

    import newton_amd as nt

    if not torch.cuda.is_available() or getattr(torch.cuda, "_newton_emulated", False):
        pytest.skip("hipGraph capture needs the device (not emulated)")
    model, jf, dt = _quadruped(64)
    solver, pipe, ctrl = nt.solvers.SolverSemiImplicit(model), nt.CollisionPipeline(model), _control(model, jf)
    d0, d1, dct = model.state(), model.state(), pipe.contacts()
    for _ in range(3):
        assert solver.rollout(d0, d1, ctrl, dct, dt, 4) is d0
    g0, g1, gct = model.state(), model.state(), pipe.contacts()
    # (the direct calls above were the warm-up: the capture pass records the frame without running it)
    graph = nt.graph.capture(lambda: solver.rollout(g0, g1, ctrl, gct, dt, 4), warmup=0, contacts=gct)
    for _ in range(3):
        graph.launch()
    torch.cuda.synchronize()
    assert np.isfinite(d0.body_q.cpu().numpy()).all()
    assert _same(g0.body_q, d0.body_q) and _same(g0.body_qd, d0.body_qd)
    assert int(gct.rigid_contact_count.cpu().numpy()[0]) == int(dct.rigid_contact_count.cpu().numpy()[0]) > 0
    for k in FLAT:
        assert _same(getattr(gct, "rigid_contact_" + k), getattr(dct, "rigid_contact_" + k)), k


@pytest.mark.parametrize("substeps", [4, 5])
def test_heterogeneous_worlds_rollout_equals_step_loop(substeps):
    """Quadrupeds + box stacks + pendulums in one model: GroupedSolver.rollout forwards to one fused launch per world group."""
    import newton_amd as nt
    from test_heterogeneous_worlds import LAYOUT, mixed_model

    model = mixed_model(LAYOUT, device="cuda:0")
    solver = nt.solvers.SolverSemiImplicit(model)
    pipe = nt.CollisionPipeline(model)
    ctrl = model.control()
    dt = 1e-4
    r0, r1, rct = model.state(), model.state(), pipe.contacts()
    out = solver.rollout(r0, r1, ctrl, rct, dt, substeps)
    assert out is (r1 if substeps % 2 else r0)
    l0, l1, lct = model.state(), model.state(), pipe.contacts()
    ref = _loop(pipe, solver, l0, l1, ctrl, lct, dt, substeps)
    assert np.isfinite(ref.body_q.cpu().numpy()).all()
    assert _same(out.body_q, ref.body_q) and _same(out.body_qd, ref.body_qd)
    n = int(lct.rigid_contact_count.cpu().numpy()[0])
    assert int(rct.rigid_contact_count.cpu().numpy()[0]) == n > 0
    for k in FLAT:
        assert _same(getattr(rct, "rigid_contact_" + k), getattr(lct, "rigid_contact_" + k)), k


def test_rollout_with_sdf_pairs_is_the_launch_by_launch_loop():
    """A model whose pairs go through the mesh-SDF leg: rollout runs the reference loop (clear_forces, collide incl. the SDF
    leg, step with the rows' penalty wrenches, swap), bit for bit what the caller's own loop produces."""
    import torch

    import newton_amd as nt
    from sdf_pipeline_checker import sdf_scene

    def run(fused, substeps):
        model = sdf_scene(3, 5, device="cuda:0", seed=12)
        q = np.asarray(model.body_q).copy()  # push the hulls of every world together: penetrating rows
        t = model.env
        c = q[:, :3].reshape(t.env_count, t.nb, 3)
        c[:, :, :2] *= 0.4
        q[:, :3] = c.reshape(-1, 3)
        model.body_q = q
        model.joint_q.reshape(-1, 7)[:, :3] = q[:, :3]
        pipe = nt.CollisionPipeline(model, broad_phase="sap")
        contacts = pipe.contacts()
        assert contacts._sdf_leg is not None
        s0, s1 = model.state(), model.state()
        solver = nt.solvers.SolverSemiImplicit(model)
        if fused:
            out = solver.rollout(s0, s1, None, contacts, 2.5e-4, substeps)
            assert out is (s1 if substeps % 2 else s0)
        else:
            out = _loop(pipe, solver, s0, s1, None, contacts, 2.5e-4, substeps)
        torch.cuda.synchronize()
        return out.body_q.cpu().numpy().copy(), out.body_qd.cpu().numpy().copy(), np.asarray(model.body_q, np.float32)

    for substeps in (4, 5):
        a, b = run(True, substeps), run(False, substeps)
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
        assert np.isfinite(a[0]).all() and not np.array_equal(a[0], a[2])
