"""newton_amd.sensors.SensorTiledCamera on the device (nt_camera_render, include/newton_hip_mesh.h).  The oracle is exact: distance,
normal and shape of every pixel equal, bit for bit, what SensorRaycast returns on the same State for the same rays.  On top: parity
with the float64 host path under the raycast gates and the depth gate, the launch shapes (blocks per group, 4 / 2 / 1 worlds per
workgroup, masked worlds), the cull and its survivor counts, and a captured graph that follows set_cameras and a changed State.
Scenes, cameras and images: tests/camera_cases.py."""
import numpy as np
import pytest

import camera_cases as cc
import raycast_cases as rc
import tolerances
from raycast_cases import DISTANCE_GATE, MAX_DISTANCE, NORMAL_GATE, compare

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_GPU, _ORACLE, _RENDER = {}, {}, {}


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _bits(x):
    return np.ascontiguousarray(_np(x)).view(np.uint32)


def _model(name):
    """(GPU model, its state), built once per scene."""
    if name not in _GPU:
        model = rc.primitive_scene(7, device=DEV) if name == "seven" else cc.SCENES[name][0](device=DEV)
        _GPU[name] = (model, model.state())
    return _GPU[name]


def _sensor(name, image, cameras=None, **extra):
    from newton_amd import sensors

    make, cams, fov, kw = cc.SCENES["primitives" if name == "seven" else name]
    W, H = cc.IMAGES[image]
    return sensors.SensorTiledCamera(_model(name)[0], cams if cameras is None else cameras, W, H, fov_y=fov, max_distance=MAX_DISTANCE, **{**kw, **extra})


def _render(s, state, mask=None, blocks_per_group=0, survivors=False):
    """Poison the outputs, render, copy back: (distance, depth, normal, shape[, survivors]) as numpy."""
    import torch

    for x, v in ((s.distance, 7.0), (s.depth, 7.0), (s.normal, 7.0), (s.shape, -7)):
        if x is not None:
            x.fill_(v)
    s._args.blocks_per_group = blocks_per_group
    surv = torch.full((s.model.env.env_count, s.blocks), -7, dtype=torch.int32, device=DEV) if survivors else None
    s._args.survivors = None if surv is None else surv.data_ptr()
    before = _np(state.body_q).copy()
    s.eval(state, world_mask=mask)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(state.body_q), before.view(np.uint32))  # body_q is only read
    out = [None if x is None else _np(x).copy() for x in (s.distance, s.depth, s.normal, s.shape)]
    return (*out, _np(surv).copy()) if survivors else tuple(out)


def _raycast(s, state):
    """SensorRaycast on the same State over the sensor's own tables, reshaped to images."""
    import torch

    from newton_amd import sensors

    o, d, body = (_np(s._resident[k]) for k in ("ray_origins", "ray_directions", "ray_bodies"))
    n = s.width * s.height
    r = sensors.SensorRaycast(s.model, np.repeat(o, n, axis=0), d.reshape(-1, 3), ray_body=np.repeat(body, n), max_distance=s.max_distance,
                              shape_mask=s.shape_mask)
    assert np.array_equal(r.slots, s.slots)
    r.eval(state)
    torch.cuda.synchronize()
    E, shp = s.model.env.env_count, (s.camera_count, s.height, s.width)
    return _np(r.distance).reshape(E, *shp).copy(), _np(r.normal).reshape(E, *shp, 3).copy(), _np(r.shape).reshape(E, *shp).copy()


def _oracle(name, image):
    if (name, image) not in _ORACLE:
        s = _sensor(name, image)
        _ORACLE[(name, image)] = (s, *_raycast(s, _model(name)[1]))
    return _ORACLE[(name, image)]


def _default_render(name, image):
    if (name, image) not in _RENDER:
        _RENDER[(name, image)] = _render(_oracle(name, image)[0], _model(name)[1])
    return _RENDER[(name, image)]


def _same(got, dist, normal, shape, sel=slice(None)):
    return (np.array_equal(_bits(got[0][sel]), _bits(dist[sel])) and np.array_equal(_bits(got[2][sel]), _bits(normal[sel]))
            and np.array_equal(got[3][sel], shape[sel]))


def test_launch_constants_are_the_kernels():
    assert cc.kernel_constants() == (cc.CAM_SLOTS, cc.CAM_TARGET_ITEMS, cc.TILE)


@pytest.mark.parametrize("name,image", cc.ORACLE_CASES)
def test_every_pixel_equals_the_ray_cast_bit_for_bit(name, image):
    """distance / normal / shape as uint32 views against SensorRaycast on the same State (cull on, the entry point's launch shape);
    the sensor's resident tables are the host sensor's."""
    s, dist, normal, shape = _oracle(name, image)
    host = cc.host_sensor(name, image)
    for k in ("ray_origins", "ray_bodies", "ray_directions", "forward", "block_cones"):
        assert np.array_equal(_np(s._resident[k]), getattr(host, k))
    got = _default_render(name, image)
    assert not np.any(got[0] == 7.0) and not np.any(got[1] == 7.0) and not np.any(got[2] == 7.0) and not np.any(got[3] == -7)
    assert _same(got, dist, normal, shape)
    assert np.any(dist >= 0.0) and np.any(dist < 0.0)
    assert np.array_equal(got[1] < 0.0, dist < 0.0) and np.all(got[1][dist < 0.0] == -1.0)
    K, B = len(s.slots), s.blocks
    wpb, spw, bpg, items, lds = cc.launch_shape(s.model.env.env_count, B, K)
    if name == "sphere_grid":  # one camera, 309 targets: five mask words per slot, hipFuncSetAttribute with four worlds staged
        assert K == 309 and (B, wpb) == {"8x8": (1, 4), "16x8": (2, 2), "19x11": (6, 1), "24x16": (6, 1)}[image]
        assert (lds > rc.RC_DEFAULT_LDS) == (wpb == 4) and lds == wpb * K * 48 + 4 * 5 * 8
    else:  # two cameras
        assert (B, wpb) == {"8x8": (2, 2), "16x8": (4, 1), "19x11": (12, 1), "24x16": (12, 1)}[image]


@pytest.mark.parametrize("name,image", cc.PARITY_CASES)
def test_parity_with_the_host_reference(name, image):
    """The raycast rule on the clear pixels (>= 0.99 of them) under the raycast gates; the depth under its own gate."""
    host, ref, depth_ref = cc.reference(name, image)
    model = _model(name)[0]
    assert np.array_equal(np.asarray(model.body_q), np.asarray(host.model.body_q))
    got = _default_render(name, image)
    E = model.env.env_count
    assert ref["clear"].mean() >= 0.99
    err_d, err_n = compare(ref, got[0].reshape(E, -1), got[2].reshape(E, -1, 3), got[3].reshape(E, -1), f"gpu camera {name} {image}")
    err_z = cc.depth_error(ref, depth_ref, got[1])
    print(f"[camera] gpu {name} {image}: max |dz| / max(1, z) = {err_z:.3e}")
    tolerances.record(f"camera_{name}_{image}", {"distance_rel": {"max": err_d}, "normal_angle": {"max": err_n}, "depth_rel": {"max": err_z}},
                      {"distance_rel": DISTANCE_GATE, "normal_angle": NORMAL_GATE, "depth_rel": cc.DEPTH_GATE})
    assert err_d <= DISTANCE_GATE and err_n <= NORMAL_GATE and err_z <= cc.DEPTH_GATE


@pytest.mark.parametrize("bpg", [1, 2, 3, 12, 0])
def test_blocks_per_group_keeps_every_bit(bpg):
    """19 x 11, two cameras: B = 12 blocks per world on four slots; 1, 2, 3 blocks per slot and item, all of them, and the entry
    point's choice."""
    s, dist, normal, shape = _oracle("primitives", "19x11")
    assert s.blocks == 12 and cc.launch_shape(5, 12, len(s.slots), bpg)[:3] == (1, 4, {1: 1, 2: 2, 3: 3, 12: 3, 0: 1}[bpg])
    full = _default_render("primitives", "19x11")
    got = _render(s, _model("primitives")[1], blocks_per_group=bpg)
    assert _same(got, dist, normal, shape) and np.array_equal(_bits(got[1]), _bits(full[1]))


@pytest.mark.parametrize("image,wpb", [("8x8", 4), ("16x8", 2)])
def test_worlds_sharing_a_workgroup_at_seven_worlds(image, wpb):
    """One camera, B = 1 / 2: four / two worlds per workgroup, the last workgroup partial; each slot reads its own world's records."""
    s = _sensor("seven", image, cameras=[cc.BODY_CAMERA])
    state = _model("seven")[1]
    assert cc.launch_shape(7, s.blocks, len(s.slots))[0] == wpb
    got = _render(s, state)
    assert _same(got, *_raycast(s, state))
    assert len({got[0][e].tobytes() for e in range(7)}) == 7  # (jittered worlds: every image differs)


@pytest.mark.parametrize("image", ["8x8", "19x11"])
def test_masked_worlds_inside_a_live_workgroup(image):
    """Worlds 1 and 4 off: at 8 x 8 with one camera world 1 shares its workgroup with three live worlds.  Masked images keep their
    poison, live images the bits of the unmasked run."""
    mask = np.array([1, 0, 1, 1, 0], bool)
    s = _sensor("primitives", image, cameras=[cc.WORLD_CAMERA]) if image == "8x8" else _oracle("primitives", image)[0]
    if image == "8x8":
        assert cc.launch_shape(5, s.blocks, len(s.slots))[0] == 4
    state = _model("primitives")[1]
    full, got = _render(s, state), _render(s, state, mask=mask, survivors=True)
    for a, b in zip(got[:4], full):
        assert np.all(np.abs(a[~mask]) == 7) and np.array_equal(_bits(a[mask]), _bits(b[mask]))
    assert np.all(got[4][~mask] == -7) and np.all(got[4][mask] >= 0)


@pytest.mark.parametrize("name", list(cc.SCENES))
def test_cull_on_and_off_give_equal_bits(name):
    on = _default_render(name, "24x16")
    s = _sensor(name, "24x16", cull=False)
    off = _render(s, _model(name)[1], survivors=True)
    for a, b in zip(on, off[:4]):
        assert np.array_equal(_bits(a), _bits(b))
    assert np.all(off[4] == len(s.slots))  # cull off: every staged target is walked


def test_survivor_counts_on_the_sphere_grid():
    """K = 309 (five mask words).  Every count <= K, >= the distinct shapes hit in the block, and < K on at least half of the blocks
    holding rays -- the float64 mirror of the cone test (camera_cases.mirror_survivors) keeps 29 .. 35 of 309 on all six blocks, and
    the kernel may keep a target the mirror drops only inside the margin."""
    s, dist, normal, shape = _oracle("sphere_grid", "24x16")
    got = _render(s, _model("sphere_grid")[1], survivors=True)
    K = len(s.slots)
    assert _same(got, dist, normal, shape) and np.any(np.isin(shape, rc.small_sphere_ids(cc.host_model("sphere_grid"))))
    assert K == 309 and np.all(got[4] <= K) and np.all(got[4] >= cc.shapes_per_block(shape, 24, 16))
    assert np.mean(got[4] < K) >= 0.5
    assert np.all(np.abs(got[4] - cc.mirror_survivors(cc.host_sensor("sphere_grid", "24x16"))[None, :]) <= 2)


def test_a_sphere_grazed_by_one_corner_pixel_survives():
    """camera_cases.graze_model: a 1 cm sphere on the ray of pixel (7, 7), the corner of block 0 where four blocks meet, two metres
    out.  Block 0 keeps it and the pixel hits it with the cull on; the blocks its disc does not reach drop it; a second sphere just
    outside block 1's cone, inside the margin's band, is kept there."""
    from newton_amd import sensors

    model, sid, band = cc.graze_model(device=DEV)
    state = model.state()
    on, off = (sensors.SensorTiledCamera(model, [cc.GRAZE_CAMERA], *cc.GRAZE_IMAGE, fov_y=cc.FOV_Y, max_distance=MAX_DISTANCE, cull=c) for c in (True, False))
    got, ref = _render(on, state, survivors=True), _render(off, state)
    cc.check_graze(sid, band, len(on.slots), got[0], got[3], got[4], ref[0], ref[3])


def test_graph_replay_follows_set_cameras_and_the_state():
    """A graph captured around eval replays to the same bits, then follows a set_cameras and a changed State (both written in
    place) on its next replay, without allocating."""
    import torch

    import newton_amd as nt

    name, image = "terrain_hfield", "19x11"
    model = _model(name)[0]
    state = model.state()  # (its own: the test writes into it)
    s = _sensor(name, image)
    direct = _render(s, state)
    g = nt.graph.capture(lambda: s.eval(state), warmup=1)
    s.distance.fill_(float("nan"))
    g.launch()
    torch.cuda.synchronize()
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(direct, (s.distance, s.depth, s.normal, s.shape)))
    # the cameras moved in place: the replay renders the new poses (the reference is a fresh sensor with those cameras)
    cams = [(-1, cc.look_at((-0.9, 1.2, 1.6), (0.1, -0.1, 0.0))), (0, np.array([0.0, 0.03, 0.25, *nt._np_math.quat_rpy(0.5, -0.2, 1.1)]))]
    store = s._resident["ray_directions"].data_ptr()
    s.set_cameras(cams)
    assert s._resident["ray_directions"].data_ptr() == store
    before = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]
    g.launch()
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats(DEV)["allocation.all.allocated"] == before
    moved = [_np(x).copy() for x in (s.distance, s.depth, s.normal, s.shape)]
    fresh = _sensor(name, image, cameras=cams)
    want = _render(fresh, state)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(moved, want)) and not np.array_equal(moved[0], direct[0])
    # the state changed in place: body 0 of every world (it carries camera 1) lifted by 0.2 m
    bq = _np(state.body_q).copy()
    bq2 = bq.copy()
    bq2.reshape(model.env.env_count, -1, 7)[:, 0, 2] += 0.2
    state.body_q = bq2
    g.launch()
    torch.cuda.synchronize()
    lifted = [_np(x).copy() for x in (s.distance, s.depth, s.normal, s.shape)]
    want = _render(fresh, state)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(lifted, want))
    assert np.array_equal(lifted[0][:, 0], moved[0][:, 0]) and not np.array_equal(lifted[0][:, 1], moved[0][:, 1])


def test_unsupported_target_is_refused_before_any_launch():
    import newton_amd as nt
    from newton_amd import sensors

    env = nt.ModelBuilder()
    b = env.add_body(xform=[0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0])
    env.add_shape_convex_hull(b, mesh=nt.Mesh.create_box(0.1, 0.1, 0.1))
    scene = nt.ModelBuilder()
    scene.replicate(env, 3)
    scene.add_ground_plane()
    model = scene.finalize(device=DEV)
    cam = [(-1, [0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 1.0])]
    with pytest.raises(NotImplementedError, match="CONVEX_MESH"):
        sensors.SensorTiledCamera(model, cam, 8, 8, fov_y=0.5)
    s = sensors.SensorTiledCamera(model, cam, 8, 8, fov_y=0.5, exclude_bodies=(0,))
    s._targets_host[0, 1] = int(nt.GeoType.CONVEX_MESH)  # the C entry point refuses the type too (the host table names it)
    s.distance.fill_(7.0)
    with pytest.raises(NotImplementedError, match="NT_ERR_UNSUPPORTED"):
        s.eval(model.state())
    assert np.all(_np(s.distance) == 7.0)
