"""newton_amd.sensors.SensorContact on the device (nt_contact_sensor, include/newton_hip_contacts.h): the synthetic exact and order sets
of tests/contact_sensor_cases.py with the assertions of the emulator file, and the product path -- quadrupeds on the ground (bitwise
against the float32 sequential sum over the public flat arrays; the float64 sum within the sequential-sum bound when the pipeline
orders its export by key), an SDF-leg scene whose rows carry force, one box at rest on the plane, a captured graph, world_mask."""
import numpy as np
import pytest

import contact_sensor_cases as cs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = 1.0 / 600.0


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _run_synthetic(case, mask=None):
    import torch

    model = cs.sensor_model(case.E, device=DEV)
    dm = model.device_model()
    call = cs.HostCall(case, dm.desc, upload=lambda a: torch.from_numpy(a).to(DEV), ptr=lambda x: x.data_ptr(), mask=mask)
    st = call.run(dm.lib, dm.stream())
    torch.cuda.synchronize()
    assert st == 0
    return _np(call.net_force)


@pytest.mark.parametrize("name", ["1_world_cells4", "5_worlds_cells289", "37_worlds_cells4", "37_worlds_cells64", "37_worlds_cells65_no_slots",
                                  "5_worlds_cells256"])
def test_exact_set_bit_for_bit(name):
    worlds, shape, nslot, rows = cs.EXACT_CASES[name]
    case = cs.exact_case(cs.sensor_model(worlds), nslot, *cs.SHAPES[shape], rows=rows, seed=len(name))
    cs.check_exact(case, _run_synthetic(case))


@pytest.mark.parametrize("name", ["5_worlds_cells20", "37_worlds_cells64", "5_worlds_cells65_no_rows", "1_world_cells289"])
def test_order_set_is_the_float32_sequential_sum(name):
    worlds, shape, nslot, rows, designed_all = cs.ORDER_CASES[name]
    case = cs.order_case(cs.sensor_model(worlds), nslot, *cs.SHAPES[shape], rows=rows, seed=len(name))
    cs.check_order(case, _run_synthetic(case), designed_all)


def test_masked_worlds_keep_the_poison():
    case = cs.exact_case(cs.sensor_model(37), 50, *cs.SHAPES["cells20"], rows="ragged", seed=4)
    mask = np.ones(37, bool)
    mask[[1, 4, 30]] = False
    cs.check_exact(case, _run_synthetic(case, mask=mask), mask=mask)


# ---------------------------------------------------------------------------------------------------------------------------------
# the product path
# ---------------------------------------------------------------------------------------------------------------------------------
def _quadrupeds(worlds):
    """scenes.quadruped_scene with the force attribute, every robot lowered by the same amount (the scene drops its robots from 0.2 m:
    a handful of steps would end in the air): by the height of the lowest far end of a shank's axis, taken over the legs of a robot and
    then the highest over the robots, plus 5 mm.  The legs then meet the ground while they settle into their target pose: every world
    carries foot force after each of the steps 7 to 11 (dt = 1/600 s), which is where the tests below read the sensor.
    -> (model, env-local bodies of the four lower legs, slot of the ground)."""
    import newton_amd as nt
    import scenes
    from newton_amd.articulation import _qrot

    model = scenes.quadruped_scene(worlds, device=DEV)
    t = model.env
    legs = [b for b in range(t.nb) if model.body_label[b].endswith("_SHANK")]
    assert len(legs) == 4 and t.ng == 1
    bq = np.asarray(model.body_q, np.float64).reshape(worlds, t.nb, 7)[:, legs]
    tip = bq[..., :3] + _qrot(bq[..., 3:], np.array([0.0, 0.0, -0.25]))
    drop = float(tip[..., 2].min(axis=1).max()) + 0.005
    model.joint_q.reshape(worlds, -1)[:, 2] -= np.float32(drop)
    model.body_q, model.body_qd = nt.articulation.eval_fk_numpy(model, model.joint_q, model.joint_qd)
    model.request_contact_attributes("force")
    return model, legs, t.ns


def _stepped(model, steps=8, **pipe_kw):
    import torch

    import newton_amd as nt

    pipe = nt.CollisionPipeline(model, **pipe_kw)
    contacts = pipe.contacts()
    solver = nt.solvers.SolverXPBD(model, iterations=2)
    s0, s1 = model.state(), model.state()
    for _ in range(steps):
        s0.clear_forces()
        pipe.collide(s0, contacts)
        solver.step(s0, s1, None, contacts, DT)
        s0, s1 = s1, s0
    torch.cuda.synchronize()
    return pipe, contacts, solver, s1, s0  # (the last step read s1 and wrote s0)


def _flat(contacts):
    n = int(_np(contacts.rigid_contact_count)[0])
    return np.array([n]), _np(contacts.rigid_contact_shape0)[:n], _np(contacts.rigid_contact_shape1)[:n], _np(contacts.force)[:n]


def test_quadruped_feet_equal_the_flat_sum_bit_for_bit():
    """Default pipeline: the flat order restricted to a world is the kernel's order, so the float32 sequential sum over the public
    Contacts.force / rigid_contact_shape0/1 (after update_contacts, which the sensor itself does not need) is met bit for bit."""
    import torch

    from newton_amd import sensors

    E = 37
    model, legs, ground = _quadrupeds(E)
    pipe, contacts, solver, _, _ = _stepped(model)
    sensor = sensors.SensorContact(model, sensing_bodies=legs, counterpart_shapes=[ground])
    assert sensor.shape == (4, 2) and tuple(sensor.net_force.shape) == (E, 4, 2, 3)
    sensor.net_force.fill_(cs.POISON)
    sensor.eval(contacts)
    torch.cuda.synchronize()
    got = _np(sensor.net_force).copy()
    solver.update_contacts(contacts)
    flat = _flat(contacts)
    want = sensors.contact_sensor_numpy(model, *flat, sensor.slot_sensing, sensor.slot_counterpart, 4, 1, True, dtype=np.float32)
    lists = cs.cell_lists(model.env, *flat, sensor.slot_sensing, sensor.slot_counterpart, True)
    assert max(len(v) for v in lists.values()) > 1  # some foot sums several contacts
    assert np.array_equal(cs.bits(got), cs.bits(want))
    assert np.all(np.any(got[:, :, 0, :] != 0.0, axis=(1, 2)))  # a foot force in every world
    assert np.array_equal(cs.bits(got[:, :, 0]), cs.bits(got[:, :, 1]))  # the feet touch nothing but the ground
    # world_mask on the product path: unselected rows keep what they hold
    mask = np.arange(E) % 3 != 1
    sensor.net_force.fill_(cs.POISON)
    sensor.eval(contacts, world_mask=mask)
    torch.cuda.synchronize()
    masked = _np(sensor.net_force)
    assert np.all(masked[~mask] == cs.POISON) and np.array_equal(cs.bits(masked[mask]), cs.bits(got[mask]))


def test_quadruped_feet_with_the_key_ordered_export():
    """CollisionPipeline(deterministic=True) orders the flat arrays by the contact key, not by slot: the kernel's sum is compared with
    the float64 sum of the flat arrays.  Bound per cell and component: the standard bound of a float32 sequential sum of n terms,
    (n - 1) * 2^-24 * sum |f_i| (n - 1 additions, each with a relative error of at most 2^-24 on a partial sum that never exceeds
    sum |f_i| in magnitude; the float64 reference's own error is 2^-29 of that)."""
    import torch

    from newton_amd import sensors

    E = 37
    model, legs, ground = _quadrupeds(E)
    pipe, contacts, solver, _, _ = _stepped(model, deterministic=True)
    sensor = sensors.SensorContact(model, sensing_bodies=legs, counterpart_shapes=[ground])
    sensor.eval(contacts)
    torch.cuda.synchronize()
    got = _np(sensor.net_force).astype(np.float64)
    solver.update_contacts(contacts)
    flat = _flat(contacts)
    want = sensors.contact_sensor_numpy(model, *flat, sensor.slot_sensing, sensor.slot_counterpart, 4, 1, True)
    bound = np.zeros_like(want)
    for key, items in cs.cell_lists(model.env, *flat, sensor.slot_sensing, sensor.slot_counterpart, True).items():
        bound[key] = (len(items) - 1) * 2.0 ** -24 * np.sum(np.abs(np.asarray(items, np.float64)), axis=0)
    err = np.abs(got - want)
    print("key-ordered export: max |kernel - float64| =", err.max(), "largest bound =", bound.max(), "largest force =", np.abs(want).max())
    assert np.any(want != 0.0) and np.all(err <= bound)


def test_sdf_leg_rows_are_part_of_the_sum():
    """sdf_pipeline_checker.sdf_scene, its hulls pushed together: the hull-hull contacts are rows of the SDF leg, summed after the slots.
    dt is a power of two: update_contacts scales the rows by float32(1.0 / dt) in torch and the slots by 1.0f / dt in its kernel; the
    sensor uses the kernel's expression for both (the contract), and the two agree when dt's reciprocal is exact."""
    import torch

    import newton_amd as nt
    from newton_amd import sensors
    from sdf_pipeline_checker import sdf_scene

    E, dt = 1, 2.0 ** -10
    assert np.float32(1.0) / np.float32(dt) == np.float32(1.0 / dt)
    model = sdf_scene(E, 5, device=DEV, seed=11)
    model.request_contact_attributes("force")
    q = np.asarray(model.body_q).copy()  # (push the hulls of every world together so that the rows carry penetrating contacts)
    q[:, :2] *= 0.4
    model.body_q = q
    model.joint_q.reshape(-1, 7)[:, :3] = q[:, :3]
    t = model.env
    pipe = nt.CollisionPipeline(model, broad_phase="sap")
    contacts = pipe.contacts()
    solver = nt.solvers.SolverXPBD(model, iterations=3)
    s0, s1 = model.state(), model.state()
    pipe.collide(s0, contacts)
    solver.step(s0, s1, model.control(), contacts, dt)
    bodies = list(range(t.nb))
    sensor = sensors.SensorContact(model, sensing_bodies=bodies, counterpart_bodies=bodies, counterpart_shapes=[t.ns])
    sensor.eval(contacts)
    torch.cuda.synchronize()
    got = _np(sensor.net_force).copy()
    n_rows = int((contacts._flat.shape0 != contacts._flat.shape1).sum().item())
    assert n_rows > 0
    solver.update_contacts(contacts)
    flat = _flat(contacts)
    args = (sensor.slot_sensing, sensor.slot_counterpart, t.nb, t.nb + 1, True)
    want = sensors.contact_sensor_numpy(model, *flat, *args, dtype=np.float32)
    assert np.array_equal(cs.bits(got), cs.bits(want))
    n_slot = flat[0][0] - n_rows
    slots_only = sensors.contact_sensor_numpy(model, np.array([n_slot]), *flat[1:], *args, dtype=np.float32)
    assert not np.array_equal(got, slots_only)  # the rows carry force


def test_box_at_rest_reads_its_weight():
    """The box of tests/test_contact_force.py::test_contact_forces_sum_to_weight (1 m cube of density 1000 on the plane, 32 iterations,
    8 substeps of 1/480 s per frame, 200 frames to settle, the force after each of 60 frames averaged) and that test's tolerances for
    it: 10 % of m g along up, 1.0 N sideways (test_contact_force.py:121-122)."""
    import torch

    import newton_amd as nt
    from newton_amd import sensors

    g, h = 9.81, 0.5
    mass = 1000.0 * (2.0 * h) ** 3
    b = nt.ModelBuilder()
    b.add_ground_plane()
    b.default_shape_cfg.density = 1000.0
    box = b.add_body(xform=[0.0, 0.0, h, 0.0, 0.0, 0.0, 1.0])
    b.add_shape_box(box, hx=h, hy=h, hz=h)
    b.request_contact_attributes("force")
    model = b.finalize(device=DEV)
    t = model.env
    assert t.env_count == 1 and t.ns == 1 and t.ng == 1
    plane = t.ns
    sensor = sensors.SensorContact(model, sensing_bodies=[0], sensing_shapes=[plane], counterpart_shapes=[plane], counterpart_bodies=[0])
    assert sensor.counterpart_labels == [("body", 0), ("shape", plane)]
    solver = nt.solvers.SolverXPBD(model, iterations=32, rigid_contact_con_weighting=True)
    pipe = nt.CollisionPipeline(model)
    contacts = pipe.contacts()
    s0, s1 = model.state(), model.state()
    sub_dt, substeps, settle, avg_steps = 1.0 / 60.0 / 8, 8, 200, 60
    mean = torch.zeros_like(sensor.net_force)
    for frame in range(settle + avg_steps):
        for _ in range(substeps):
            s0.clear_forces()
            pipe.collide(s0, contacts)
            solver.step(s0, s1, None, contacts, sub_dt)
            s0, s1 = s1, s0
        if frame >= settle:
            sensor.eval(contacts)
            mean += sensor.net_force
    torch.cuda.synchronize()
    f = _np(mean)[0] / avg_steps  # [sensing object: box, plane][column: total, box, plane][3]
    np.testing.assert_allclose(f[0, 0, 2], mass * g, rtol=0.10)
    np.testing.assert_allclose(f[0, 0, :2], 0.0, atol=1.0)
    assert np.array_equal(f[0, 2], f[0, 0]) and np.all(f[0, 1] == 0.0)  # all of it exchanged with the plane
    assert np.array_equal(f[1, 0], -f[0, 0]) and np.array_equal(f[1, 1], -f[0, 0]) and np.all(f[1, 2] == 0.0)  # the plane reads the negative


def test_captured_frame_replays_the_sensor():
    """collide; step; sensor.eval recorded once: a replay after the state was overwritten in place gives the eager result of that
    state bit for bit, and nothing is allocated."""
    import torch

    import newton_amd as nt
    from newton_amd import sensors

    if getattr(torch.cuda, "_newton_emulated", False):
        pytest.skip("hipGraph capture needs the device (not emulated)")
    E = 5
    model, legs, ground = _quadrupeds(E)
    pipe, contacts, solver, state_a, state_b = _stepped(model, steps=7)
    sensor = sensors.SensorContact(model, sensing_bodies=legs, counterpart_shapes=[ground])
    s0, s1 = model.state(), model.state()

    def frame():
        s0.clear_forces()
        pipe.collide(s0, contacts)
        solver.step(s0, s1, None, contacts, DT)
        sensor.eval(contacts)

    eager = {}
    for name, src in (("b", state_b), ("a", state_a)):
        s0.assign(src)
        frame()
        torch.cuda.synchronize()
        eager[name] = _np(sensor.net_force).copy()
    assert np.any(eager["a"] != 0.0) and not np.array_equal(eager["a"], eager["b"])
    graph = nt.graph.capture(frame, warmup=1, contacts=contacts)  # (s0 holds state a)
    sensor.net_force.fill_(cs.POISON)
    graph.launch()
    torch.cuda.synchronize()
    assert np.array_equal(cs.bits(_np(sensor.net_force)), cs.bits(eager["a"]))
    s0.assign(state_b)
    before = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]
    graph.launch()
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats(DEV)["allocation.all.allocated"] == before
    assert np.array_equal(cs.bits(_np(sensor.net_force)), cs.bits(eager["b"]))


def test_eval_needs_the_force_attribute_and_a_step():
    import newton_amd as nt
    import scenes
    from newton_amd import sensors

    model = scenes.quadruped_scene(2, device=DEV)
    sensor = sensors.SensorContact(model, sensing_bodies=[3], counterpart_shapes=[model.env.ns])
    pipe = nt.CollisionPipeline(model)
    with pytest.raises(ValueError, match="request_contact_attributes"):
        sensor.eval(pipe.contacts())
    model.request_contact_attributes("force")
    contacts = pipe.contacts()
    with pytest.raises(ValueError, match=r"SolverXPBD.step\(\)"):
        sensor.eval(contacts)
    with pytest.raises(ValueError, match="world_mask"):
        sensor.eval(contacts, world_mask=[True])
