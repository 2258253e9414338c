"""newton_amd.sensors.SensorFrameTransform / SensorIMU on a host model: known answers of the float64 path (frame_sensor_numpy, the
reference of frame_sensor_kernel) that fix the physics -- a body at rest, free fall, constant spin, transform identities -- and the
classes' world_mask and errors.  Identities are met to 1e-12, the named quantities to 1e-9 relative."""
from types import SimpleNamespace

import numpy as np
import pytest

import frame_sensor_cases as fc
from newton_amd import sensors
from newton_amd.articulation import _qinv, _qmul, _qrot

E, NB = 5, 4
G = float(np.float32(9.81))  # |g| of the model: its gravity rows are float32
ID = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]


@pytest.fixture(scope="module")
def model():
    return fc.sensor_model(E, varied_gravity=False)  # (0, 0, -9.81) in every world


def _axis_angle(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return np.concatenate([axis * np.sin(0.5 * angle), [np.cos(0.5 * angle)]])


def _rand_quat(rng, n=None):
    q = rng.normal(size=(4,) if n is None else (n, 4))
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def _state(rng=None):
    """float64 body_q / body_qd [E * NB, ...]: at rest with identity attitude, or random."""
    q = np.zeros((E * NB, 7))
    q[:, 6] = 1.0
    qd = np.zeros((E * NB, 6))
    if rng is not None:
        q[:, :3], q[:, 3:] = rng.uniform(-3, 3, size=(E * NB, 3)), _rand_quat(rng, E * NB)
        qd[:] = rng.normal(size=(E * NB, 6))
    return q, qd


def _eval(model, q, qd, frames, refs=None, qd_prev=None, dt=None, **kw):
    """frames / refs: [(body, xform)]; rows measure frame k in refs[k] (None: the world)."""
    table = list(frames) + list(refs or [])
    n = len(frames)
    out_ref = np.full(n, -1) if not refs else n + np.arange(n)
    return sensors.frame_sensor_numpy(model, q, qd, [b for b, _ in table], np.array([ID if x is None else x for _, x in table], np.float64),
                                      np.arange(n), out_ref, qd_prev, dt, **kw)


def _close(got, want, scale):
    assert np.all(np.abs(np.asarray(got) - np.asarray(want)) <= 1e-9 * scale), (got, want)


def test_body_at_rest_reads_plus_g_along_up(model):
    q, qd = _state()
    pitch = _axis_angle([0, 1, 0], np.pi / 2)  # frame x axis = world -z, frame z axis = world +x
    roll = _axis_angle([1, 0, 0], np.pi / 2)   # frame y axis = world +z
    out = _eval(model, q, qd, [(1, None), (1, [0.1, 0.2, 0.3, *pitch]), (-1, [1.0, 2.0, 3.0, *roll])], qd_prev=qd, dt=1e-3)
    _close(out["accel"][:, 0], [0.0, 0.0, G], G)
    _close(out["accel"][:, 1], [-G, 0.0, 0.0], G)   # up is the frame's -x
    _close(out["accel"][:, 2], [0.0, G, 0.0], G)    # a frame fixed in the world: rot_inv(q_l, -g)
    _close(out["gravity_dir"][:, 0], [0.0, 0.0, -1.0], 1.0)
    _close(out["gravity_dir"][:, 1], [1.0, 0.0, 0.0], 1.0)
    assert np.all(out["velocity"] == 0.0)


def test_free_fall_reads_zero(model):
    rng = np.random.default_rng(0)
    q, qd_prev = _state(rng)
    dt = 2e-3
    qd_prev[:, 3:] = 0.0  # no spin: every point of the body falls freely
    qd = qd_prev.copy()
    qd[:, :3] += np.array([0.0, 0.0, -G]) * dt
    out = _eval(model, q, qd, [(0, None), (1, fc.random_xform(rng)), (3, fc.random_xform(rng))], qd_prev=qd_prev, dt=dt)
    assert np.all(np.abs(out["accel"]) <= 1e-9 * G)


def test_constant_spin_about_the_com(model):
    rng = np.random.default_rng(1)
    q, qd = _state()
    body, w = 3, np.array([0.0, 0.0, 2.5])
    com = np.asarray(model.body_com, np.float64).reshape(E, NB, 3)[0, body]
    assert np.any(com != 0.0)
    r = np.array([0.3, -0.4, 0.0])  # perpendicular to z
    ql = _rand_quat(rng)
    rows = np.arange(E) * NB + body
    q[rows, :3] = rng.uniform(-2, 2, size=(E, 3))
    qd[rows, 3:] = w  # the COM is at rest: the body spins about it
    out = _eval(model, q, qd, [(body, [*(com + r), *ql])], qd_prev=qd, dt=1e-3)
    qf = ql  # identity body attitude
    scale = w @ w * np.linalg.norm(r) + G
    _close(out["accel"][:, 0], _qrot(_qinv(qf), -(w @ w) * r - np.array([0.0, 0.0, -G])), scale)
    _close(out["velocity"][:, 0, 3:], _qrot(_qinv(qf), w), np.linalg.norm(w))
    _close(out["velocity"][:, 0, :3], _qrot(_qinv(qf), np.cross(w, r)), np.linalg.norm(w) * np.linalg.norm(r))
    # the same body rotated as a whole: readings in frame axes do not change, up to the direction of gravity
    qb = _rand_quat(rng)
    q[rows, 3:] = qb
    qd[rows, 3:] = _qrot(qb, w)
    out2 = _eval(model, q, qd, [(body, [*(com + r), *ql])], qd_prev=qd, dt=1e-3)
    qf2 = _qmul(qb, ql)
    _close(out2["velocity"][:, 0], out["velocity"][:, 0], np.linalg.norm(w))
    _close(out2["accel"][:, 0], _qrot(_qinv(qf2), -(w @ w) * _qrot(qb, r) - np.array([0.0, 0.0, -G])), scale)


def test_transform_identities(model):
    rng = np.random.default_rng(2)
    q, qd = _state(rng)
    a, b = (1, fc.random_xform(rng).astype(np.float64)), (2, fc.random_xform(rng).astype(np.float64))
    for x in (a, b):
        x[1][3:] /= np.linalg.norm(x[1][3:])  # unit to float64 accuracy
    self_ = _eval(model, q, qd, [a, b], [a, b])["transform"]
    assert np.all(np.abs(self_ - np.array(ID)) <= 1e-12)  # a frame relative to itself
    Ta_w, Tb_w = _eval(model, q, qd, [a, b])["transform"].transpose(1, 0, 2)
    Ta_b = _eval(model, q, qd, [a], [b])["transform"][:, 0]
    comp_p = Tb_w[:, :3] + _qrot(Tb_w[:, 3:], Ta_b[:, :3])
    comp_q = _qmul(Tb_w[:, 3:], Ta_b[:, 3:])
    assert np.all(np.abs(comp_p - Ta_w[:, :3]) <= 1e-12 * 10.0) and np.all(np.abs(comp_q - Ta_w[:, 3:]) <= 1e-12)  # T(a|w) = T(b|w) T(a|b)
    # one common rigid motion (P, Qm) applied to every body: T(a|b) stays
    P, Qm = rng.uniform(-5, 5, size=3), _rand_quat(rng)
    q2 = q.copy()
    q2[:, :3] = P + _qrot(Qm, q[:, :3])
    q2[:, 3:] = _qmul(Qm, q[:, 3:])
    moved = _eval(model, q2, qd, [a], [b])["transform"][:, 0]
    assert np.all(np.abs(moved - Ta_b) <= 1e-12 * 10.0)
    assert not np.allclose(_eval(model, q2, qd, [a])["transform"], Ta_w[:, None])  # (the world pose did move)


def test_zero_gravity_world_and_per_world_rows():
    model = fc.sensor_model(E)  # a gravity row of its own per world, world 3 without gravity
    g = np.asarray(model.gravity, np.float64)[:E]
    assert np.all(g[3] == 0.0) and np.all(np.any(g[[0, 1, 2, 4]] != 0.0, axis=1))
    q, qd = _state()
    out = _eval(model, q, qd, [(0, None), (-1, None)], qd_prev=qd, dt=1e-3)
    assert np.all(out["gravity_dir"][3] == 0.0) and np.all(out["accel"][3] == 0.0)
    for k in (0, 1):
        _close(out["gravity_dir"][[0, 1, 2, 4], k], g[[0, 1, 2, 4]] / np.linalg.norm(g[[0, 1, 2, 4]], axis=1, keepdims=True), 1.0)
        _close(out["accel"][:, k], -g, 20.0)


def test_classes_fill_their_outputs_and_world_mask_keeps_rows(model):
    rng = np.random.default_rng(3)
    s, sp = model.state(), model.state()
    q, qd = _state(rng)
    s.body_q, s.body_qd = q, qd
    sp.body_q, sp.body_qd = q, qd * 0.5
    xf = fc.random_xform(rng)
    ft = sensors.SensorFrameTransform(model, [(1, xf), (2, None), (-1, None)], reference_frames=[(0, None)])
    assert ft.transforms.shape == (E, 3, 7) and ft.transforms.dtype == np.float64
    assert list(ft.out_ref) == [3, 3, 3]  # one reference frame serves every frame
    ft.eval(s)
    want = sensors.frame_sensor_numpy(model, s.body_q, s.body_qd, [1, 2, -1, 0], [xf, ID, ID, ID], [0, 1, 2], [3, 3, 3])
    assert np.array_equal(ft.transforms, want["transform"]) and np.any(ft.transforms[:, :, :3] != 0.0)
    assert np.array_equal(sensors.SensorFrameTransform(model, [(1, xf)]).out_ref, [-1])  # no reference: the world
    mask = np.array([True, False, True, True, False])
    ft.transforms[...] = 7.0
    ft.eval(s, world_mask=mask)
    assert np.all(ft.transforms[~mask] == 7.0) and np.array_equal(ft.transforms[mask], want["transform"][mask])

    imu = sensors.SensorIMU(model, [(0, None), (1, xf)], want_velocity=True, want_projected_gravity=True)
    assert np.shares_memory(imu.gyroscope, imu.velocity) and np.shares_memory(imu.linear_velocity, imu.velocity)  # views, not copies
    dt = 4e-3
    imu.eval(s, sp, dt)
    want = sensors.frame_sensor_numpy(model, s.body_q, s.body_qd, [0, 1], [ID, xf], [0, 1], [-1, -1], sp.body_qd, dt)
    assert np.array_equal(imu.accelerometer, want["accel"]) and np.array_equal(imu.gyroscope, want["velocity"][..., 3:])
    assert np.array_equal(imu.linear_velocity, want["velocity"][..., :3]) and np.array_equal(imu.projected_gravity, want["gravity_dir"])
    assert np.any(imu.accelerometer != 0.0)
    imu.accelerometer[...] = 7.0
    imu.velocity[...] = 7.0
    imu.eval(s, sp, dt, world_mask=mask)
    assert np.all(imu.accelerometer[~mask] == 7.0) and np.all(imu.gyroscope[~mask] == 7.0)
    assert np.array_equal(imu.accelerometer[mask], want["accel"][mask])
    plain = sensors.SensorIMU(model, [(0, None)])
    assert plain.linear_velocity is None and plain.projected_gravity is None and plain.gyroscope.shape == (E, 1, 3)


def test_errors(model):
    s = model.state()
    for cls in (sensors.SensorFrameTransform, sensors.SensorIMU):
        name = cls.__name__
        with pytest.raises(NotImplementedError, match=f"{name}: heterogeneous models are unsupported"):
            cls(SimpleNamespace(is_heterogeneous=True), [(0, None)])
        with pytest.raises(ValueError, match=f"frame 1: body {NB} is out of range"):
            cls(model, [(0, None), (NB, None)])
        with pytest.raises(ValueError, match="frame 0: body -2 is out of range"):
            cls(model, [(-2, None)])
        with pytest.raises(ValueError, match="frame 2: the quaternion of xform is not a unit quaternion"):
            cls(model, [(0, None), (1, None), (1, [0, 0, 0, 0, 0, 0, 1.001])])
        with pytest.raises(ValueError, match="frame 0: xform must be 7 finite numbers"):
            cls(model, [(0, [0, 0, np.nan, 0, 0, 0, 1])])
        with pytest.raises(ValueError, match="frame 0: xform must be 7 finite numbers"):
            cls(model, [(0, [0, 0, 0, 1])])
        with pytest.raises(ValueError, match="no frame"):
            cls(model, [])
    with pytest.raises(ValueError, match="frame 1: body 9 is out of range"):
        sensors.SensorFrameTransform(model, [(0, None)], reference_frames=[(9, None)])  # (table index 1: the reference)
    with pytest.raises(ValueError, match="reference_frames must have 1 or 3 entries, got 2"):
        sensors.SensorFrameTransform(model, [(0, None)] * 3, reference_frames=[(1, None)] * 2)
    sensors.SensorFrameTransform(model, [(0, [0, 0, 0, 0, 0, 0, 1.00005])])  # inside the 1e-4 bound
    ft = sensors.SensorFrameTransform(model, [(0, None)])
    with pytest.raises(ValueError, match=f"world_mask must have {E} entries"):
        ft.eval(s, world_mask=[True])
    imu = sensors.SensorIMU(model, [(0, None)])
    with pytest.raises(ValueError, match=f"world_mask must have {E} entries"):
        imu.eval(s, s, 1e-3, world_mask=np.ones(E + 1, bool))
    for dt in (0.0, -1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="dt must be positive"):
            imu.eval(s, s, dt)


def test_shared_cases_are_not_vacuous():
    """The table of tests/frame_sensor_cases.py has what the kernel tests rely on, and the reference's scales are positive wherever
    something is added."""
    c = fc.case(5, 70)
    fb, fx = c.frame_body, c.frame_xform
    assert np.any(fb == -1) and np.sum(fb == 1) == 2 and np.any(np.all(fx == fc.IDENTITY, axis=1)) and np.any(fx[:, :3] != 0.0)
    assert np.any(c.out_ref > c.out_frame) and np.any(c.out_ref == c.out_frame) and np.any(c.out_ref == -1)
    assert set(range(c.M)) <= set(c.out_frame.tolist())  # every frame is measured
    one = fc.case(5, 1)
    assert one.out_ref[0] > one.out_frame[0] >= 0  # N = 1: a frame referenced to one later in the table
    ref = c.reference()
    assert all(ref[k].shape == (5, 70, n) for k, n in fc.OUTPUTS.items())
    assert np.all(ref["gravity_dir"][3] == 0.0) and np.any(ref["gravity_dir"][2] != 0.0)
    moving = fb[c.out_frame] >= 0
    assert np.all(ref["scale"]["accel"][:, moving] > 0.0) and np.all(ref["scale"]["velocity"][:, moving] > 0.0)
    assert np.all(ref["scale"]["accel"][[0, 1, 2, 4]] > 0.0) and np.all(ref["accel"][3][~moving] == 0.0)  # (fixed in a world without gravity)
    assert np.all(ref["velocity"][:, ~moving] == 0.0)
    # float32 evaluation of the same contract stays inside the derived tolerance: the bound is not met by construction only
    f32 = sensors.frame_sensor_numpy(c.model, c.body_q, c.body_qd, c.frame_body, c.frame_xform, c.out_frame, c.out_ref, c.body_qd_prev, c.dt,
                                     dtype=np.float32)
    got = {k: np.asarray(f32[k], np.float32) for k in fc.OUTPUTS}
    assert fc.check(ref, got, what="numpy float32")["transform"] > 0.0
