"""newton_amd.sensors.SensorFrameTransform / SensorIMU on the device (nt_frame_sensor, include/newton_hip_kinematics.h): the shared
cases of tests/frame_sensor_cases.py through the entry point with the emulator file's tolerance, and the product path -- stepped
quadrupeds (shanks in the base frame, an IMU on the base) against frame_sensor_numpy on the AoS copies of the states, replicated
worlds bit for bit, a run-time gravity change, a captured graph, world_mask from torch and from numpy."""
import numpy as np
import pytest

import frame_sensor_cases as fc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = 1.0 / 600.0


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _run_shared(case, mask=None, only=tuple(fc.OUTPUTS)):
    import torch

    model = fc.sensor_model(case.E, device=DEV, varied_gravity=case.varied_gravity)
    dm = model.device_model()
    s, sp = model.state(), model.state()
    s.body_q, s.body_qd = case.body_q, case.body_qd
    sp.body_q, sp.body_qd = case.body_q, case.body_qd_prev
    call = fc.Call(case, upload=lambda a: torch.from_numpy(a).to(DEV), ptr=lambda x: x.data_ptr(), mask=mask, only=only)
    ds, dp = s._desc(), sp._desc()
    st = call.run(dm.lib, dm.desc, ds, dp if "accel" in only else None, stream=dm.stream())
    torch.cuda.synchronize()
    assert st == 0
    return {k: _np(v) for k, v in call.out.items()}


@pytest.mark.parametrize("rows", fc.ROWS)
@pytest.mark.parametrize("worlds", fc.WORLDS)
def test_shared_cases_within_the_tolerance(worlds, rows):
    case = fc.case(worlds, rows)
    fc.check(case.reference(), _run_shared(case), what=f"device {worlds} worlds {rows} rows")


@pytest.mark.parametrize("only", list(fc.OUTPUTS))
def test_every_output_alone(only):
    case = fc.case(5, 3)
    got = _run_shared(case, only=(only,))
    assert list(got) == [only]
    fc.check(case.reference(), got, what=f"device only {only}")


def test_masked_worlds_keep_the_poison():
    case = fc.case(37, 3)
    mask = np.ones(37, bool)
    mask[[1, 4, 30]] = False
    fc.check(case.reference(), _run_shared(case, mask=mask), mask=mask, what="device masked")


# ---------------------------------------------------------------------------------------------------------------------------------
# the product path
# ---------------------------------------------------------------------------------------------------------------------------------
E = 37
IMU_MOUNT = np.array([0.12, -0.03, 0.05, *(np.array([0.1, -0.2, 0.3, 0.9]) / np.linalg.norm([0.1, -0.2, 0.3, 0.9]))], np.float32)


def _quadrupeds(worlds):
    """scenes.quadruped_scene without its seeded per-world height jitter -- the worlds are replicas, which the bit-for-bit comparison
    between worlds needs -- lowered onto the ground so that contacts act within the few steps taken here.
    -> (model, base body, the four shank bodies)."""
    import newton_amd as nt
    import scenes

    model = scenes.quadruped_scene(worlds, device=DEV, seed=None, height_jitter=0.0)
    t = model.env
    model.joint_q.reshape(worlds, -1)[:, 2] -= np.float32(0.26)
    model.body_q, model.body_qd = nt.articulation.eval_fk_numpy(model, model.joint_q, model.joint_qd)
    shanks = [b for b in range(t.nb) if model.body_label[b].endswith("_SHANK")]
    base = [b for b in range(t.nb) if model.body_label[b].endswith("base")]
    assert len(shanks) == 4 and len(base) == 1
    return model, base[0], shanks


def _stepped(model, steps=8):
    """`steps` SolverXPBD steps with collide -> (solver, pipe, contacts, newest state, the one before it)."""
    import torch

    import newton_amd as nt

    pipe = nt.CollisionPipeline(model)
    contacts = pipe.contacts()
    solver = nt.solvers.SolverXPBD(model, iterations=2)
    s0, s1 = model.state(), model.state()
    for _ in range(steps):
        s0.clear_forces()
        pipe.collide(s0, contacts)
        solver.step(s0, s1, None, contacts, DT)
        s0, s1 = s1, s0
    torch.cuda.synchronize()
    return solver, pipe, contacts, s0, s1  # (the last step read s1 and wrote s0)


def _sensors(model, base, shanks):
    from newton_amd import sensors

    ft = sensors.SensorFrameTransform(model, [(b, [0.0, 0.0, -0.25, 0.0, 0.0, 0.0, 1.0]) for b in shanks], reference_frames=[(base, None)])
    imu = sensors.SensorIMU(model, [(base, IMU_MOUNT)], want_velocity=True, want_projected_gravity=True)
    return ft, imu


def _reference(model, ft, imu, new, old, dt):
    from newton_amd import sensors

    q, qd, qd_old = _np(new.body_q), _np(new.body_qd), _np(old.body_qd)
    ref_ft = sensors.frame_sensor_numpy(model, q, qd, ft.frame_body, ft.frame_xform, ft.out_frame, ft.out_ref, with_scale=True)
    ref_imu = sensors.frame_sensor_numpy(model, q, qd, imu.frame_body, imu.frame_xform, imu.out_frame, imu.out_ref, qd_old,
                                         float(np.float32(dt)), with_scale=True)
    return ref_ft, ref_imu


def _imu_outputs(imu):
    return {"velocity": _np(imu.velocity), "accel": _np(imu.accelerometer), "gravity_dir": _np(imu.projected_gravity)}


def test_quadrupeds_feet_in_the_base_frame_and_base_imu():
    import torch

    model, base, shanks = _quadrupeds(E)
    solver, pipe, contacts, new, old = _stepped(model)
    ft, imu = _sensors(model, base, shanks)
    assert tuple(ft.transforms.shape) == (E, 4, 7) and tuple(imu.accelerometer.shape) == (E, 1, 3)
    assert imu.gyroscope.data_ptr() == imu.velocity[..., 3:].data_ptr() and imu.linear_velocity.data_ptr() == imu.velocity.data_ptr()  # views
    ft.transforms.fill_(fc.POISON)
    ft.eval(new)
    imu.eval(new, old, DT)
    torch.cuda.synchronize()
    ref_ft, ref_imu = _reference(model, ft, imu, new, old, DT)
    got_ft, got_imu = {"transform": _np(ft.transforms)}, _imu_outputs(imu)
    fc.check(ref_ft, got_ft, what="quadruped feet")
    fc.check(ref_imu, got_imu, what="quadruped base imu")
    assert np.all(np.abs(ref_ft["transform"][:, :, 2]) > 0.1)  # the feet are below the base
    assert np.any(np.abs(ref_imu["accel"]) > 1.0) and np.any(ref_imu["velocity"] != 0.0)
    assert np.array_equal(_np(imu.gyroscope), got_imu["velocity"][..., 3:]) and np.array_equal(_np(imu.linear_velocity), got_imu["velocity"][..., :3])
    for got in (got_ft["transform"], *got_imu.values()):  # the worlds are replicas: every world equals world 0 bit for bit
        assert np.all(fc.bits(got) == fc.bits(got[:1]))


def test_runtime_gravity_change_is_followed_without_a_rebuild():
    import torch

    from newton_amd.enums import ModelFlags

    model, base, shanks = _quadrupeds(5)
    solver, pipe, contacts, new, old = _stepped(model, steps=3)
    ft, imu = _sensors(model, base, shanks)
    imu.eval(new, old, DT)
    torch.cuda.synchronize()
    before = _imu_outputs(imu)
    before = {k: v.copy() for k, v in before.items()}
    g = np.array([[0.0, 0.0, -2.0], [0.0, 0.0, -4.0], [1.0, 0.0, -6.0], [0.0, -3.0, 0.0], [0.0, 0.0, 0.0]], np.float32)
    model.set_gravity(g)
    solver.notify_model_changed(ModelFlags.MODEL_PROPERTIES)
    imu.eval(new, old, DT)
    torch.cuda.synchronize()
    _, ref_imu = _reference(model, ft, imu, new, old, DT)
    after = _imu_outputs(imu)
    fc.check(ref_imu, after, what="after set_gravity")
    assert np.array_equal(after["velocity"], before["velocity"])
    assert not np.array_equal(after["accel"][:4], before["accel"][:4]) and np.all(after["gravity_dir"][4] == 0.0)
    # accelerometer(new gravity) - accelerometer(old gravity) = rot_inv(q_f, g_old - g_new), to float32 rounding of readings of ~20 m/s^2
    from newton_amd.articulation import _qinv, _qmul, _qrot

    qf = _qmul(_np(new.body_q).astype(np.float64).reshape(5, -1, 7)[:, base, 3:], IMU_MOUNT[3:].astype(np.float64))
    want = _qrot(_qinv(qf), np.array([0.0, 0.0, -9.81]) - g.astype(np.float64))
    assert np.all(np.abs((after["accel"][:, 0].astype(np.float64) - before["accel"][:, 0]) - want) < 1e-3)


def test_captured_frame_replays_both_sensors():
    """collide; step; both evals recorded once: a replay after the states were advanced in place equals the eager call on those states
    bit for bit, and nothing is allocated."""
    import torch

    import newton_amd as nt

    if getattr(torch.cuda, "_newton_emulated", False):
        pytest.skip("hipGraph capture needs the device (not emulated)")
    model, base, shanks = _quadrupeds(5)
    solver, pipe, contacts, state_a, state_b = _stepped(model, steps=5)
    ft, imu = _sensors(model, base, shanks)
    s0, s1 = model.state(), model.state()

    def frame():
        s0.clear_forces()
        pipe.collide(s0, contacts)
        solver.step(s0, s1, None, contacts, DT)
        ft.eval(s1)
        imu.eval(s1, s0, DT)

    def outputs():
        torch.cuda.synchronize()
        return {"transform": _np(ft.transforms).copy(), **{k: v.copy() for k, v in _imu_outputs(imu).items()}}

    eager = {}
    for name, src in (("b", state_b), ("a", state_a)):
        s0.assign(src)
        frame()
        eager[name] = outputs()
    assert not np.array_equal(eager["a"]["accel"], eager["b"]["accel"]) and not np.array_equal(eager["a"]["transform"], eager["b"]["transform"])
    graph = nt.graph.capture(frame, warmup=1, contacts=contacts)  # (s0 holds state a)
    for x in (ft.transforms, imu.velocity, imu.accelerometer, imu.projected_gravity):
        x.fill_(fc.POISON)
    graph.launch()
    got = outputs()
    assert all(np.array_equal(fc.bits(got[k]), fc.bits(eager["a"][k])) for k in got)
    s0.assign(state_b)  # the states advance in place
    before = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]
    graph.launch()
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats(DEV)["allocation.all.allocated"] == before
    got = outputs()
    assert all(np.array_equal(fc.bits(got[k]), fc.bits(eager["b"][k])) for k in got)


def test_world_mask_from_torch_and_numpy():
    import torch

    model, base, shanks = _quadrupeds(5)
    solver, pipe, contacts, new, old = _stepped(model, steps=3)
    ft, imu = _sensors(model, base, shanks)
    ft.eval(new)
    imu.eval(new, old, DT)
    torch.cuda.synchronize()
    full = {"transform": _np(ft.transforms).copy(), **{k: v.copy() for k, v in _imu_outputs(imu).items()}}
    mask = np.array([True, False, True, True, False])
    for wm in (mask, torch.from_numpy(mask).to(DEV), torch.from_numpy(mask)):
        for x in (ft.transforms, imu.velocity, imu.accelerometer, imu.projected_gravity):
            x.fill_(fc.POISON)
        ft.eval(new, world_mask=wm)
        imu.eval(new, old, DT, world_mask=wm)
        torch.cuda.synchronize()
        got = {"transform": _np(ft.transforms), **_imu_outputs(imu)}
        for k in got:
            assert np.all(got[k][~mask] == fc.POISON) and np.array_equal(fc.bits(got[k][mask]), fc.bits(full[k][mask]))
    ft.eval(new)  # no mask again: every row is written
    torch.cuda.synchronize()
    assert np.array_equal(fc.bits(_np(ft.transforms)), fc.bits(full["transform"]))
    with pytest.raises(ValueError, match="world_mask must have 5 entries"):
        ft.eval(new, world_mask=[True])
    with pytest.raises(ValueError, match="dt must be positive"):
        imu.eval(new, old, 0.0)
    with pytest.raises(TypeError, match="needs State objects"):
        ft.eval(object())
