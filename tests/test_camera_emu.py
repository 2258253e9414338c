"""camera_kernel (nt_camera_render, include/newton_hip_mesh.h) on the emulator: the kernel SOURCES executed on the CPU (tests/emu).
The oracle is exact: distance, normal and shape of every pixel equal, bit for bit, what nt_raycast -- raycast_kernel, pinned by
tests/test_raycast_emu.py -- returns for the same rays.  On top: parity with the float64 host path under the raycast gates, the depth
gate, the launch shapes, the world mask and the cull.  Scenes, cameras and images: tests/camera_cases.py (5 worlds, 7 where four
worlds share a workgroup)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import camera_cases as cc  # noqa: E402
import raycast_cases as rc  # noqa: E402
import tolerances  # noqa: E402
from camera_cases import HostCameraArgs, emu_render  # noqa: E402
from raycast_cases import DISTANCE_GATE, NORMAL_GATE, HostArgs, compare, emu_cast  # noqa: E402


@pytest.fixture(scope="module")
def H(oracle_lib):
    import harness

    harness.lib()  # builds tests/emu/_build/libnewton_emu.so on first use
    return harness


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


_EMU, _ORACLE, _RENDER = {}, {}, {}


def _emu_model(H, model):
    if id(model) not in _EMU:
        em = H.EmuModel(model)
        _EMU[id(model)] = (em, H.EmuState(em))
    return _EMU[id(model)]


def _render(H, s, mask=None, **kw):
    em, state = _emu_model(H, s.model)
    before = state.body_q.copy()
    args = HostCameraArgs(s, **kw)
    if mask is not None:
        args.set_world_mask(mask)
    H.check(emu_render(H, em, state, args), "nt_camera_render")
    assert np.array_equal(_bits(state.body_q), _bits(before))  # body_q is only read
    return args


def _oracle(H, name, image):
    """nt_raycast over the sensor's expanded rays: (distance, normal, shape) as [E, C, H, W(, 3)], computed once per case."""
    if (name, image) not in _ORACLE:
        s = cc.host_sensor(name, image)
        em, state = _emu_model(H, s.model)
        args = HostArgs(s.model, cc.expanded_rays(s), s.slots, max_distance=s.max_distance)
        H.check(emu_cast(H, em, state, args), "nt_raycast")
        E, shp = s.model.env.env_count, (s.camera_count, s.height, s.width)
        _ORACLE[(name, image)] = (s, args.distance.reshape(E, *shp), args.normal.reshape(E, *shp, 3), args.shape.reshape(E, *shp))
    return _ORACLE[(name, image)]


def _default_render(H, name, image):
    if (name, image) not in _RENDER:
        _RENDER[(name, image)] = _render(H, _oracle(H, name, image)[0])
    return _RENDER[(name, image)]


def _same(args, dist, normal, shape, sel=slice(None)):
    return (np.array_equal(_bits(args.distance[sel]), _bits(dist[sel])) and np.array_equal(_bits(args.normal[sel]), _bits(normal[sel]))
            and np.array_equal(args.shape[sel], shape[sel]))


def test_launch_constants_are_the_kernels():
    assert cc.kernel_constants() == (cc.CAM_SLOTS, cc.CAM_TARGET_ITEMS, cc.TILE)


@pytest.mark.parametrize("name,image", cc.ORACLE_CASES)
def test_every_pixel_equals_the_ray_cast_bit_for_bit(H, name, image):
    """distance / normal / shape as uint32 views against nt_raycast on the expanded rays (cull on, the entry point's launch shape)."""
    s, dist, normal, shape = _oracle(H, name, image)
    args = _default_render(H, name, image)
    assert not np.any(args.distance == 7.0) and not np.any(args.depth == 7.0) and not np.any(args.normal == 7.0) and not np.any(args.shape == -7)
    assert _same(args, dist, normal, shape)
    assert np.any(dist >= 0.0) and np.any(dist < 0.0)
    assert np.array_equal(args.depth < 0.0, dist < 0.0) and np.all(args.depth[dist < 0.0] == -1.0)
    K, B = len(s.slots), s.blocks
    wpb, spw, bpg, items, lds = cc.launch_shape(s.model.env.env_count, B, K)
    if name == "sphere_grid":  # one camera, 309 targets: five mask words per slot, the LDS request above 48 KB with four worlds staged
        assert K == 309 and (B, wpb) == {"8x8": (1, 4), "16x8": (2, 2), "19x11": (6, 1), "24x16": (6, 1)}[image]
        assert (lds > rc.RC_DEFAULT_LDS) == (wpb == 4) and lds == wpb * K * 48 + 4 * 5 * 8
    else:  # two cameras
        assert (B, wpb) == {"8x8": (2, 2), "16x8": (4, 1), "19x11": (12, 1), "24x16": (12, 1)}[image]


@pytest.mark.parametrize("name,image", cc.PARITY_CASES)
def test_parity_with_the_host_reference(H, name, image):
    """The raycast rule on the clear pixels (>= 0.99 of them), the raycast gates; the depth under its own gate."""
    s, ref, depth_ref = cc.reference(name, image)
    args = _default_render(H, name, image)
    E = s.model.env.env_count
    assert ref["clear"].mean() >= 0.99
    err_d, err_n = compare(ref, args.distance.reshape(E, -1), args.normal.reshape(E, -1, 3), args.shape.reshape(E, -1), f"emu camera {name} {image}")
    err_z = cc.depth_error(ref, depth_ref, args.depth)
    print(f"[camera] emu {name} {image}: max |dz| / max(1, z) = {err_z:.3e}")
    tolerances.record(f"camera_emu_{name}_{image}", {"distance_rel": {"max": err_d}, "normal_angle": {"max": err_n}, "depth_rel": {"max": err_z}},
                      {"distance_rel": DISTANCE_GATE, "normal_angle": NORMAL_GATE, "depth_rel": cc.DEPTH_GATE})
    assert err_d <= DISTANCE_GATE and err_n <= NORMAL_GATE and err_z <= cc.DEPTH_GATE


@pytest.mark.parametrize("bpg", [1, 2, 3, 12, 0])
def test_blocks_per_group_keeps_every_bit(H, bpg):
    """19 x 11, two cameras: B = 12 blocks per world on four slots; 1, 2, 3 blocks per slot and item, all of them, and the entry
    point's choice."""
    s, dist, normal, shape = _oracle(H, "primitives", "19x11")
    assert s.blocks == 12 and cc.launch_shape(5, 12, len(s.slots), bpg)[:3] == (1, 4, {1: 1, 2: 2, 3: 3, 12: 3, 0: 1}[bpg])
    full = _default_render(H, "primitives", "19x11")
    args = _render(H, s, blocks_per_group=bpg)
    assert _same(args, dist, normal, shape) and np.array_equal(_bits(args.depth), _bits(full.depth))


@pytest.mark.parametrize("image,wpb", [("8x8", 4), ("16x8", 2)])
def test_worlds_sharing_a_workgroup_at_seven_worlds(H, image, wpb):
    """One camera, B = 1 / 2: four / two worlds per workgroup, the last workgroup partial; each slot reads its own world's records."""
    model = _seven()
    cams = [cc.BODY_CAMERA]
    W, Hh = cc.IMAGES[image]
    from newton_amd import sensors

    s = sensors.SensorTiledCamera(model, cams, W, Hh, fov_y=cc.FOV_Y, max_distance=rc.MAX_DISTANCE, exclude_bodies=(0,))
    assert cc.launch_shape(7, s.blocks, len(s.slots))[0] == wpb
    em, state = _emu_model(H, model)
    ray = HostArgs(model, cc.expanded_rays(s), s.slots, max_distance=s.max_distance)
    H.check(emu_cast(H, em, state, ray), "nt_raycast")
    args = _render(H, s)
    shp = (7, 1, Hh, W)
    assert _same(args, ray.distance.reshape(shp), ray.normal.reshape(*shp, 3), ray.shape.reshape(shp))
    assert len({args.distance[e].tobytes() for e in range(7)}) == 7  # (jittered worlds: every image differs)


_SEVEN = {}


def _seven():
    if "m" not in _SEVEN:
        _SEVEN["m"] = rc.primitive_scene(7)
    return _SEVEN["m"]


@pytest.mark.parametrize("image", ["8x8", "19x11"])
def test_masked_worlds_inside_a_live_workgroup(H, image):
    """Worlds 1 and 4 off: at 8 x 8 with one camera world 1 shares its workgroup with three live worlds.  Masked images keep their
    poison, live images the bits of the unmasked run."""
    from newton_amd import sensors

    mask = np.array([1, 0, 1, 1, 0], bool)
    if image == "8x8":
        s = sensors.SensorTiledCamera(cc.host_model("primitives"), [cc.WORLD_CAMERA], 8, 8, fov_y=cc.FOV_Y, max_distance=rc.MAX_DISTANCE)
        assert cc.launch_shape(5, s.blocks, len(s.slots))[0] == 4
    else:
        s = cc.host_sensor("primitives", image)
    full, args = _render(H, s), _render(H, s, mask=mask, survivors=True)
    for got, want in ((args.distance, full.distance), (args.depth, full.depth), (args.normal, full.normal), (args.shape, full.shape)):
        assert np.all(np.abs(got[~mask]) == 7) and np.array_equal(_bits(got[mask]), _bits(want[mask]))
    assert np.all(args.survivors[~mask] == -7) and np.all(args.survivors[mask] >= 0)


@pytest.mark.parametrize("name", list(cc.SCENES))
def test_cull_on_and_off_give_equal_bits(H, name):
    s = _oracle(H, name, "24x16")[0]
    on = _default_render(H, name, "24x16")
    off = _render(H, s, cull=False, survivors=True)
    for a, b in ((on.distance, off.distance), (on.depth, off.depth), (on.normal, off.normal), (on.shape, off.shape)):
        assert np.array_equal(_bits(a), _bits(b))
    assert np.all(off.survivors == len(s.slots))  # cull off: every staged target is walked


def test_survivor_counts_on_the_sphere_grid(H):
    """K = 309 (five mask words).  Every count <= K, >= the distinct shapes hit in the block, and < K on at least half of the blocks
    holding rays -- the float64 mirror of the cone test (camera_cases.mirror_survivors) keeps 29 .. 35 of 309 on all six blocks, and
    the kernel may keep a target the mirror drops only inside the margin."""
    s, dist, normal, shape = _oracle(H, "sphere_grid", "24x16")
    args = _render(H, s, survivors=True)
    K = len(s.slots)
    assert _same(args, dist, normal, shape) and np.any(np.isin(shape, rc.small_sphere_ids(s.model)))
    assert K == 309 and np.all(args.survivors <= K) and np.all(args.survivors >= cc.shapes_per_block(shape, 24, 16))
    assert np.mean(args.survivors < K) >= 0.5
    mirror = cc.mirror_survivors(s)
    assert np.all(np.abs(args.survivors - mirror[None, :]) <= 2)  # (a sphere on the margin's edge may fall either way)


def test_a_sphere_grazed_by_one_corner_pixel_survives(H):
    """camera_cases.graze_model: a 1 cm sphere on the ray of pixel (7, 7), the corner of block 0 where four blocks meet, two metres
    out.  Block 0 keeps it and the pixel hits it with the cull on; the blocks its disc does not reach drop it; a second sphere just
    outside block 1's cone, inside the margin's band, is kept there."""
    from newton_amd import sensors

    model, sid, band = cc.graze_model()
    s = sensors.SensorTiledCamera(model, [cc.GRAZE_CAMERA], *cc.GRAZE_IMAGE, fov_y=cc.FOV_Y, max_distance=rc.MAX_DISTANCE)
    args = _render(H, s, survivors=True)
    off = _render(H, s, cull=False)
    cc.check_graze(sid, band, len(s.slots), args.distance, args.shape, args.survivors, off.distance, off.shape)


def test_outputs_one_at_a_time(H):
    s = _oracle(H, "primitives", "19x11")[0]
    full = _default_render(H, "primitives", "19x11")
    only_d = _render(H, s, want=())
    only_z = _render(H, s, want=("depth",))
    only_n = _render(H, s, want=("normal",))
    assert only_d.depth is None and only_d.normal is None and only_d.shape is None
    assert all(np.array_equal(_bits(x.distance), _bits(full.distance)) for x in (only_d, only_z, only_n))
    assert np.array_equal(_bits(only_z.depth), _bits(full.depth)) and np.array_equal(_bits(only_n.normal), _bits(full.normal))


def test_errors(H):
    s = cc.host_sensor("primitives", "19x11")
    em, state = _emu_model(H, s.model)
    lib = H.lib()
    d = state.desc()
    args = HostCameraArgs(s)
    assert lib.nt_camera_render(None, C.byref(d), C.byref(args.desc), None) == -1
    assert lib.nt_camera_render(C.byref(em.desc), C.byref(d), None, None) == -1
    for field, bad in (("distance", None), ("ray_directions", None), ("forward", None), ("width", 0), ("camera_count", 0), ("blocks_per_group", -1),
                       ("block_cones", None)):
        saved = getattr(args.desc, field)
        setattr(args.desc, field, bad)
        assert emu_render(H, em, state, args) == -1, field
        setattr(args.desc, field, saved)
    args.desc.flags, saved = 0, args.desc.block_cones
    args.desc.block_cones = None  # (not needed without the cull)
    assert emu_render(H, em, state, args) == 0
    args.desc.flags, args.desc.block_cones = 1, saved
    args.distance[:] = 7.0
    table = args.tables.keep["targets"]
    kept = table[0, 1]
    table[0, 1] = 10  # CONVEX_MESH-like: no ray target
    assert emu_render(H, em, state, args) == -3
    table[0, 1] = kept
    table[[0, 1]] = table[[1, 0]]  # not ascending
    assert emu_render(H, em, state, args) == -1
    table[[0, 1]] = table[[1, 0]]
    assert np.all(args.distance == 7.0)
    n = 160 * 1024 // 48 + 1  # more staged targets than the LDS of a CU holds
    big = np.zeros((n, 2), np.int32)
    args.desc.target_count, args.desc.targets, args.desc.targets_host = n, big.ctypes.data, big.ctypes.data
    assert emu_render(H, em, state, args) in (-1, -3)
