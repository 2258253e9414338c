"""newton_amd.sensors.SensorTiledCamera on a host model (float64 numpy, `camera_numpy`): closed forms of the pinhole table and of two
one-shape scenes, the tables the kernel reads, the argument checks.  No kernel runs here; test_camera_emu.py / test_gpu_camera.py do."""
import numpy as np
import pytest

import camera_cases as cc
import newton_amd as nt
import raycast_cases as rc
from newton_amd import sensors


def _ground(worlds=2, sphere=None, hull=False):
    env = nt.ModelBuilder()
    b = env.add_body(xform=[0.0, 0.0, 0.5, 0.0, 0.0, 0.0, 1.0])
    if hull:
        env.add_shape_convex_hull(b, mesh=nt.Mesh.create_box(0.1, 0.1, 0.1))
    else:
        env.add_shape_sphere(b, radius=0.05)
    scene = nt.ModelBuilder()
    scene.replicate(env, worlds)
    scene.add_ground_plane()
    if sphere is not None:
        scene.add_shape_sphere(-1, xform=[*sphere[0], 0.0, 0.0, 0.0, 1.0], radius=sphere[1])
    return scene.finalize()


def test_pinhole_rays_closed_forms():
    W, H, fov = 7, 5, np.deg2rad(50.0)
    d = sensors.pinhole_rays(W, H, fov)
    assert d.shape == (H * W, 3) and d.dtype == np.float32
    img = d.reshape(H, W, 3)
    assert np.array_equal(img[H // 2, W // 2], np.array([0.0, 0.0, -1.0], np.float32))  # the centre pixel of an odd image, exactly
    th = np.tan(0.5 * fov)
    for (i, j) in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (1, 4)):
        want = np.array([((j + 0.5) / W * 2 - 1) * th * W / H, (1 - (i + 0.5) / H * 2) * th, -1.0])
        assert np.array_equal(img[i, j], want.astype(np.float32))
    assert np.all(img[0, :, 1] > 0.0) and np.all(img[-1, :, 1] < 0.0)  # row 0 is the top: +y is up
    assert np.all(img[:, 0, 0] < 0.0) and np.all(img[:, -1, 0] > 0.0)  # column 0 is the left: +x is right
    with pytest.raises(ValueError):
        sensors.pinhole_rays(0, 4, fov)


def test_tables_of_a_rotated_camera():
    """ray_directions = R(q) pinhole in float64, rounded once; ray_origins = p; forward = R(q) (0, 0, -1); a [C, H * W, 3] table per camera."""
    model = _ground()
    q = nt._np_math.quat_rpy(0.7, -0.4, 1.9)
    xf = np.array([0.3, -0.2, 1.1, *q])
    W, H = 6, 4
    s = sensors.SensorTiledCamera(model, [(0, xf), (-1, None)], W, H, fov_y=0.9)
    R = np.asarray(nt._np_math.quat_to_matrix(np.asarray(q, np.float64)), np.float64).reshape(3, 3)
    lens = sensors.pinhole_rays(W, H, 0.9).astype(np.float64)
    assert s.ray_directions.dtype == np.float32 and s.ray_directions.shape == (2, H * W, 3)
    assert np.max(np.abs(s.ray_directions[0] - lens @ R.T)) <= 1.0e-7 * np.max(np.abs(lens))
    assert np.array_equal(s.ray_directions[1], lens.astype(np.float32))
    assert np.array_equal(s.ray_origins, np.array([xf[:3], [0, 0, 0]], np.float32)) and np.array_equal(s.ray_bodies, [0, -1])
    assert np.max(np.abs(s.forward[0] - R @ [0.0, 0.0, -1.0])) <= 1.0e-7 and np.array_equal(s.forward[1], [0.0, 0.0, -1.0])
    table = np.stack([lens, lens * [1.0, 0.5, 2.0]]).astype(np.float32)
    s2 = sensors.SensorTiledCamera(model, [(-1, None), (-1, None)], W, H, rays=table)
    assert np.array_equal(s2.ray_directions, table)
    # every unit ray of a block lies inside the block's cone
    cones = s.block_cones.astype(np.float64)
    assert cones.shape == (2, 1, 5)
    u = s.ray_directions[0].astype(np.float64)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    assert np.all(u @ cones[0, 0, :3] >= cones[0, 0, 3]) and abs(np.hypot(cones[0, 0, 3], cones[0, 0, 4]) - 1.0) < 1e-6


def test_looking_straight_down_at_the_ground():
    model = _ground()
    W, H = 9, 7
    s = sensors.SensorTiledCamera(model, [(-1, [0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 1.0])], W, H, fov_y=np.deg2rad(35.0), exclude_bodies=(0,))
    s.eval(model.state())
    d = s.ray_directions[0].astype(np.float64)
    cos = -d[:, 2] / np.linalg.norm(d, axis=1)
    assert s.distance.shape == (2, 1, H, W) and s.distance.dtype == np.float64 and s.shape.dtype == np.int32
    assert np.max(np.abs(s.depth - 2.0)) <= 1e-12
    assert np.max(np.abs(s.distance - (2.0 / cos).reshape(H, W))) <= 1e-12
    assert np.all(s.shape == model.env.gshape_id[0]) and np.max(np.abs(s.normal - [0.0, 0.0, 1.0])) <= 1e-12


def test_sphere_on_the_axis():
    h, r = 1.75, 0.25  # (exact in float32, the format of ray_origins and of the model's tables)
    model = _ground(sphere=((0.0, 0.0, 0.0), r))
    s = sensors.SensorTiledCamera(model, [(-1, [0.0, 0.0, h, 0.0, 0.0, 0.0, 1.0])], 5, 5, fov_y=0.5, exclude_bodies=(0,))
    s.eval(model.state())
    assert abs(s.distance[0, 0, 2, 2] - (h - r)) <= 1e-12 and abs(s.depth[0, 0, 2, 2] - (h - r)) <= 1e-12
    assert s.shape[0, 0, 2, 2] == model.env.gshape_id[1]
    # the same camera carried by body 0 (at z = 0.5, upright): the pose composes
    s2 = sensors.SensorTiledCamera(model, [(0, [0.0, 0.0, h - 0.5, 0.0, 0.0, 0.0, 1.0])], 5, 5, fov_y=0.5, exclude_bodies=(0,))
    s2.eval(model.state())
    assert np.max(np.abs(s2.distance - s.distance)) <= 1e-12
    # a world mask: the other rows keep what they hold
    s.distance[:], s.depth[:] = 7.0, 7.0
    s.eval(model.state(), world_mask=[False, True])
    assert np.all(s.distance[0] == 7.0) and np.all(s.depth[0] == 7.0) and np.max(np.abs(s.distance[1] - s2.distance[1])) <= 1e-12


def test_set_cameras_and_optional_outputs():
    model = _ground()
    s = sensors.SensorTiledCamera(model, [(-1, [0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 1.0])], 4, 4, fov_y=0.6, want_depth=False, want_normal=False,
                                  want_shape=False, exclude_bodies=(0,))
    assert s.depth is None and s.normal is None and s.shape is None
    s.eval(model.state())
    first = s.distance.copy()
    s.set_cameras([(-1, [0.0, 0.0, 3.0, 0.0, 0.0, 0.0, 1.0])])
    s.eval(model.state())
    assert np.max(np.abs(s.distance - 1.5 * first)) <= 1e-12 and s.ray_origins[0, 2] == 3.0
    with pytest.raises(ValueError, match="1 cameras expected"):
        s.set_cameras([(-1, None), (-1, None)])


def test_argument_checks():
    model = _ground()
    cam = [(-1, None)]
    with pytest.raises(ValueError, match="no camera"):
        sensors.SensorTiledCamera(model, [], 4, 4, fov_y=0.5)
    with pytest.raises(ValueError, match="exactly one of rays and fov_y"):
        sensors.SensorTiledCamera(model, cam, 4, 4)
    with pytest.raises(ValueError, match="exactly one of rays and fov_y"):
        sensors.SensorTiledCamera(model, cam, 4, 4, rays=sensors.pinhole_rays(4, 4, 0.5), fov_y=0.5)
    with pytest.raises(ValueError, match="rays must be finite with shape"):
        sensors.SensorTiledCamera(model, cam, 4, 4, rays=np.zeros((15, 3)))
    with pytest.raises(ValueError, match="rays must be finite with shape"):
        sensors.SensorTiledCamera(model, cam, 4, 4, rays=np.zeros((2, 16, 3)))
    with pytest.raises(ValueError, match="not a unit quaternion"):
        sensors.SensorTiledCamera(model, [(-1, [0, 0, 0, 0, 0, 0.5, 1.0])], 4, 4, fov_y=0.5)
    with pytest.raises(ValueError, match="body 1 is out of range"):
        sensors.SensorTiledCamera(model, [(1, None)], 4, 4, fov_y=0.5)
    with pytest.raises(ValueError, match="7 finite numbers"):
        sensors.SensorTiledCamera(model, [(0, [0.0, 0.0, 1.0])], 4, 4, fov_y=0.5)
    with pytest.raises(ValueError, match="shape_mask must have"):
        sensors.SensorTiledCamera(model, cam, 4, 4, fov_y=0.5, shape_mask=[True])
    with pytest.raises(ValueError, match="max_distance"):
        sensors.SensorTiledCamera(model, cam, 4, 4, fov_y=0.5, max_distance=-1.0)
    with pytest.raises(NotImplementedError, match="CONVEX_MESH"):
        sensors.SensorTiledCamera(_ground(hull=True), cam, 4, 4, fov_y=0.5)
    sensors.SensorTiledCamera(_ground(hull=True), cam, 4, 4, fov_y=0.5, exclude_bodies=(0,))  # (masked out: accepted)

    class Heterogeneous:
        is_heterogeneous = True

    with pytest.raises(NotImplementedError, match="heterogeneous"):
        sensors.SensorTiledCamera(Heterogeneous(), cam, 4, 4, fov_y=0.5)


def test_camera_numpy_is_raycast_numpy_on_the_expanded_rays():
    s, ref, depth = cc.reference("primitives", "19x11")
    model = s.model
    E, Cn, H, W = model.env.env_count, 2, 11, 19
    dist, dep, normal, shape = sensors.camera_numpy(model, model.body_q, s.ray_origins, s.ray_bodies, s.ray_directions, s.forward, W, H,
                                                    s.max_distance, s.slots)
    o, d, body = cc.expanded_rays(s)
    rd, rn, rs = sensors.raycast_numpy(model, model.body_q, o, d, body, s.max_distance, s.slots)
    assert np.array_equal(dist.reshape(E, -1), rd) and np.array_equal(normal.reshape(E, -1, 3), rn) and np.array_equal(shape.reshape(E, -1), rs)
    assert np.array_equal(dist.reshape(E, -1), ref["distance"]) and dist.shape == (E, Cn, H, W)
    # depth never exceeds the distance, equals it on the optical axis only, and is -1 exactly where the distance is
    hit = dist >= 0.0
    assert np.array_equal(dep < 0.0, ~hit) and np.all(dep[~hit] == -1.0)
    # (1e-6: forward and the body quaternions are float32 inputs, unit to 1e-7 only; the corner pixels: cos 34 degrees)
    assert np.all(dep[hit] <= dist[hit] * (1.0 + 1e-6)) and np.all(dep[hit] > 0.8 * dist[hit])
    # the conditions the parity tests rest on: most pixels are clear, most hit something, one world shows nine shapes
    assert ref["clear"].mean() >= 0.99 and hit.mean() > 0.5 and len(np.unique(shape[0][hit[0]])) >= 9


@pytest.mark.parametrize("name,image", cc.PARITY_CASES)
def test_parity_cases_are_clear(name, image):
    s, ref, depth = cc.reference(name, image)
    assert ref["clear"].mean() >= 0.99 and (ref["distance"] >= 0.0).mean() > 0.5


def test_the_cull_mirror_drops_targets_on_the_sphere_grid():
    """The float64 mirror of the kernel's cone test on the sphere-grid scene at 24 x 16 (K = 309): the expectation the device test
    checks the kernel's own counts against.  The mirror keeps 29 .. 35 of 309 targets per block; every block holds rays."""
    s = cc.host_sensor("sphere_grid", "24x16")
    K = len(s.slots)
    counts = cc.mirror_survivors(s)
    assert K == 309 and counts.shape == (6,) and np.all(counts >= 1)
    assert np.all(counts < K // 2)
    # nothing that is hit was dropped: the host image names at most `count` shapes per block
    s.eval(s.model.state())
    assert np.all(cc.shapes_per_block(s.shape, 24, 16)[0] <= counts) and np.any(np.isin(s.shape, rc.small_sphere_ids(s.model)))
