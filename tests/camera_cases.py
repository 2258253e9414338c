"""Scenes, cameras and helpers shared by tests/test_camera_host.py, test_camera_emu.py and test_gpu_camera.py (test infrastructure).
The scenes, the float64 reference and the comparison rule are those of tests/raycast_cases.py: a pixel is a ray, and the oracle of
camera_kernel is raycast_kernel on the same rays, bit for bit."""
import ctypes as C
import os
import re

import numpy as np

import newton_amd as nt
import raycast_cases as rc
from newton_amd import sensors
from raycast_cases import MAX_DISTANCE

WORLDS = 5
FOV_Y = np.deg2rad(40.0)
# width x height: partial blocks on both axes (B = 6 per camera); B = 1 (four worlds per workgroup); B = 2 (two); whole blocks
IMAGES = {"19x11": (19, 11), "8x8": (8, 8), "16x8": (16, 8), "24x16": (24, 16)}


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """The camera pose (p, q xyzw) at `eye` looking at `target`: the camera looks along its -z, +y is up, +x right."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (eye - target) / np.linalg.norm(eye - target)
    x = np.cross(np.asarray(up, np.float64), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    m = np.stack([x, y, z], axis=1)  # columns: the camera's axes in the parent frame
    w = 0.5 * np.sqrt(max(0.0, 1.0 + m[0, 0] + m[1, 1] + m[2, 2]))
    if w > 1e-6:
        q = np.array([(m[2, 1] - m[1, 2]) / (4 * w), (m[0, 2] - m[2, 0]) / (4 * w), (m[1, 0] - m[0, 1]) / (4 * w), w])
    else:  # a half turn: the axis from the diagonal
        i = int(np.argmax(np.diag(m)))
        v = (m[:, i] + np.eye(3)[i]) / 2.0
        q = np.array([*(v / np.sqrt(v[i])), 0.0])
    q /= np.linalg.norm(q)
    return np.array([*eye, *q])


# the two cameras of the issue: one fixed in the world, one carried by body 0 with a tilted xform (body 0's shapes excluded)
WORLD_CAMERA = (-1, look_at((2.0, -1.6, 1.4), (0.2, 0.2, 0.1)))
CARRIER_CAMERA = (0, np.array([0.05, -0.02, 0.3, *nt._np_math.quat_rpy(0.6, 0.3, 1.0)]))  # under the terrain scenes' carrier, tilted


def _on_body_0(pose):
    """`pose` (a world pose at the primitive scene's rest state) in the frame of body 0, the sphere with its seeded random rotation."""
    m = nt._np_math
    x0 = np.asarray(rc.primitive_scene(1, jitter=False).body_q, np.float64)[0]
    return np.asarray(m.transform_mul(m.transform_inverse(x0), pose), np.float64)


BODY_CAMERA = (0, _on_body_0(look_at((-1.1, -1.2, 0.8), (0.3, 0.2, 0.15))))  # rides on the sphere, looks across the other bodies
TERRAIN_CAMERA = (-1, look_at((1.1, -0.9, 1.8), (0.0, 0.0, 0.0)))
# under the grid of 1 cm spheres (z = 2.5, x = -1 .. 1.2, y = -1 .. -0.7 for 300 of them), looking up at its middle
GRID_CAMERA = (-1, look_at((0.11, -0.86, 1.3), (0.11, -0.86, 2.5), up=(0.0, 1.0, 0.0)))
GRID_FOV_Y = np.deg2rad(30.0)

# name -> (model factory(device), cameras, fov_y, sensor keyword arguments)
SCENES = {
    "primitives": (lambda device=None: rc.primitive_scene(WORLDS, device=device), [WORLD_CAMERA, BODY_CAMERA], FOV_Y, {"exclude_bodies": (0,)}),
    "terrain_mesh": (lambda device=None: rc.terrain_model(False, world_count=WORLDS, device=device), [TERRAIN_CAMERA, CARRIER_CAMERA], FOV_Y,
                     {"exclude_bodies": (0,)}),
    "terrain_hfield": (lambda device=None: rc.terrain_model(True, world_count=WORLDS, device=device), [TERRAIN_CAMERA, CARRIER_CAMERA], FOV_Y,
                       {"exclude_bodies": (0,)}),
    "sphere_grid": (lambda device=None: rc.launch_model(extra_spheres=300, device=device), [GRID_CAMERA], GRID_FOV_Y, {}),
}
_MODELS, _REF = {}, {}


def host_model(name):
    if name not in _MODELS:
        _MODELS[name] = SCENES[name][0]()
    return _MODELS[name]


def host_sensor(name, image, cameras=None, **extra):
    """A SensorTiledCamera on the host model of the scene (for the tables the kernel reads, and as the float64 path)."""
    make, cams, fov, kw = SCENES[name]
    W, H = IMAGES[image]
    return sensors.SensorTiledCamera(host_model(name), cams if cameras is None else cameras, W, H, fov_y=fov, max_distance=MAX_DISTANCE,
                                     **{**kw, **extra})


def expanded_rays(s):
    """(origins, directions, ray_body) of SensorRaycast / nt_raycast for the sensor's pixels."""
    n = s.width * s.height
    return (np.repeat(s.ray_origins, n, axis=0), s.ray_directions.reshape(-1, 3).copy(), np.repeat(s.ray_bodies, n).astype(np.int32))


def reference(name, image):
    """(host sensor, raycast_cases.reference over the expanded rays, float64 depth [E, C, H, W]); built once, nothing writes into it."""
    if (name, image) not in _REF:
        s = host_sensor(name, image)
        model = host_model(name)
        ref = rc.reference(model, model.body_q, expanded_rays(s), **SCENES[name][3])
        depth = sensors.camera_numpy(model, model.body_q, s.ray_origins, s.ray_bodies, s.ray_directions, s.forward, s.width, s.height,
                                     s.max_distance, s.slots)[1]
        _REF[(name, image)] = (s, ref, depth)
    return _REF[(name, image)]


def depth_error(ref, depth_ref, depth):
    """max |depth - depth_ref| / max(1, depth_ref) over the clear pixels that hit."""
    ok = (ref["clear"] & (ref["distance"] >= 0.0)).reshape(depth_ref.shape)
    d = np.asarray(depth, np.float64).reshape(depth_ref.shape)
    return float(np.max(np.abs(d - depth_ref)[ok] / np.maximum(1.0, depth_ref[ok])))


# The depth gate: 4 x the largest |depth_dev - depth_ref| / max(1, depth_ref) the emulator measures on the parity cases below
# (primitives 24x16: 7.73e-07, 19x11: 6.70e-07; terrain_mesh / terrain_hfield 24x16: 4.22e-07, 19x11: 4.93e-07; the distance errors of
# the same runs: 6.26e-07, 5.81e-07, 3.67e-07, 5.02e-07).  3.09e-06 lies below raycast_cases.DISTANCE_GATE (5.64e-06), as expected of
# the distance times one more fp32 dot product with a factor <= 1.
DEPTH_GATE = 4 * 7.73e-7
PARITY_CASES = [("primitives", "24x16"), ("primitives", "19x11"), ("terrain_mesh", "24x16"), ("terrain_hfield", "24x16"),
                ("terrain_mesh", "19x11"), ("terrain_hfield", "19x11")]
ORACLE_CASES = [(n, i) for n in SCENES for i in IMAGES]


# ---------------------------------------------------------------------------------------------------------------------------------
# nt_camera_render on host arrays (the emulated library takes numpy arrays where the product passes device pointers)
# ---------------------------------------------------------------------------------------------------------------------------------
class HostCameraArgs:
    """nt_camera_args over numpy arrays for the host sensor `s`; the mesh / heightfield tables are raycast_cases.HostArgs' own."""

    def __init__(self, s, cull=True, blocks_per_group=0, survivors=False, want=("depth", "normal", "shape")):
        from newton_amd import _lib as L

        model = s.model
        E, Cn, H, W = model.env.env_count, s.camera_count, s.height, s.width
        self.tables = rc.HostArgs(model, expanded_rays(s), s.slots, max_distance=s.max_distance)
        ptr = lambda x: x.ctypes.data_as(C.c_void_p).value  # noqa: E731
        self.keep = k = dict(o=np.ascontiguousarray(s.ray_origins, np.float32), b=np.ascontiguousarray(s.ray_bodies, np.int32),
                             d=np.ascontiguousarray(s.ray_directions, np.float32), f=np.ascontiguousarray(s.forward, np.float32),
                             cones=np.ascontiguousarray(s.block_cones, np.float32))
        self.distance = np.full((E, Cn, H, W), 7.0, np.float32)  # poisoned: the call overwrites every selected image
        self.depth = np.full((E, Cn, H, W), 7.0, np.float32) if "depth" in want else None
        self.normal = np.full((E, Cn, H, W, 3), 7.0, np.float32) if "normal" in want else None
        self.shape = np.full((E, Cn, H, W), -7, np.int32) if "shape" in want else None
        self.survivors = np.full((E, s.blocks), -7, np.int32) if survivors else None
        a = L.nt_camera_args()
        a.camera_count, a.width, a.height = Cn, W, H
        a.ray_origins, a.ray_bodies, a.ray_directions, a.forward, a.block_cones = ptr(k["o"]), ptr(k["b"]), ptr(k["d"]), ptr(k["f"]), ptr(k["cones"])
        t = self.tables.desc
        a.max_distance, a.target_count, a.targets, a.targets_host = t.max_distance, t.target_count, t.targets, t.targets_host
        for f in ("shape_vertex_range", "shape_triangle_range", "vertices", "indices", "block_bounds", "shape_block_start",
                  "shape_heightfield_index", "heightfields", "elevations"):
            setattr(a, f, getattr(t, f))
        for f in ("distance", "depth", "normal", "shape", "survivors"):
            setattr(a, f, None if getattr(self, f) is None else ptr(getattr(self, f)))
        a.flags, a.blocks_per_group = int(cull), blocks_per_group
        self.desc = a

    def set_world_mask(self, mask):
        self.keep["wm"] = np.ascontiguousarray(mask, np.uint8)
        self.desc.world_mask = self.keep["wm"].ctypes.data


def emu_render(H, em, state, args):
    d = state.desc()
    return H.lib().nt_camera_render(C.byref(em.desc), C.byref(d), C.byref(args.desc), None)


# ---------------------------------------------------------------------------------------------------------------------------------
# camera_kernel's launch rule, restated from newton_amd/csrc/nt_mesh_plane.hip (nt_camera_render).  The launch-shape tests assert
# from it that every case lands on the path it is there for, and from the source text that the constants are still these.
# ---------------------------------------------------------------------------------------------------------------------------------
CAM_SLOTS, CAM_TARGET_ITEMS, TILE = 4, 1024, 8


def block_count(cameras, width, height):
    return cameras * ((height + TILE - 1) // TILE) * ((width + TILE - 1) // TILE)


def launch_shape(worlds, blocks, target_count, blocks_per_group=0):
    """(worlds per workgroup, wave slots per world, blocks per slot and item, workgroup items, dynamic LDS bytes)."""
    wpb = 4 if blocks == 1 else (2 if blocks == 2 else 1)
    per_world = target_count * rc.RC_REC * 4
    mask_bytes = CAM_SLOTS * ((target_count + 63) // 64) * 8 if target_count > 64 else 0
    while wpb > 1 and wpb * per_world + mask_bytes > rc.RC_LDS_BYTES_PER_CU:
        wpb //= 2
    spw = CAM_SLOTS // wpb
    world_groups, per_slot = (worlds + wpb - 1) // wpb, (blocks + spw - 1) // spw
    bpg = blocks_per_group
    if bpg == 0:
        cuts = min(max((CAM_TARGET_ITEMS + world_groups - 1) // world_groups, 1), per_slot)
        bpg = (per_slot + cuts - 1) // cuts
    bpg = min(bpg, per_slot)
    return wpb, spw, bpg, world_groups * ((blocks + bpg * spw - 1) // (bpg * spw)), wpb * per_world + mask_bytes


def kernel_constants():
    """(wave slots, target items, tile) as the kernel source and the header state them."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "newton_amd", "csrc", "nt_mesh_plane.hip")).read()
    hdr = open(os.path.join(root, "include", "newton_hip_mesh.h")).read()
    assert "constexpr int CAM_SLOTS = RC_THREADS / 64;" in src and "int wpb = B == 1 ? 4 : (B == 2 ? 2 : 1);" in src
    assert "(size_t)CAM_SLOTS * ((K + 63) / 64) * 8" in src and sensors.CAMERA_TILE == TILE
    items = int(re.search(r"constexpr long long CAM_TARGET_ITEMS = (\d+);", src).group(1))
    tile = int(re.search(r"#define NT_CAMERA_TILE (\d+)", hdr).group(1))
    return rc.RC_THREADS // 64, items, tile


# ---------------------------------------------------------------------------------------------------------------------------------
# the cone test of camera_kernel in float64 (the same formula and margin), for the survivor-count expectations
# ---------------------------------------------------------------------------------------------------------------------------------
CULL_REL, CULL_ABS = 1.0e-3, 1.0e-5


def bounding_radius(gtype, s):
    from newton_amd.enums import GeoType

    a = np.abs(np.asarray(s, np.float64))
    if gtype == GeoType.PLANE:
        return None if (s[0] == 0.0 and s[1] == 0.0) else float(np.hypot(a[0], a[1]))
    if gtype == GeoType.SPHERE:
        return float(a[0])
    if gtype == GeoType.ELLIPSOID:
        return float(a.max())
    if gtype == GeoType.BOX:
        return float(np.linalg.norm(a))
    if gtype == GeoType.CAPSULE:
        return float(a[0] + a[1])
    if gtype in (GeoType.CYLINDER, GeoType.CONE):
        return float(np.hypot(a[0], a[1]))
    return None


def mirror_survivors(s, world=0):
    """[blocks] the survivor count of every pixel block of world `world`, by the kernel's cone test in float64 (world-fixed cameras and
    global or resting shapes: the poses are the model's)."""
    model, t = s.model, s.model.env
    assert np.all(s.ray_bodies == -1)
    bq = np.asarray(model.body_q, np.float64).reshape(t.env_count, t.nb, 7)[world]
    xf, sc = np.asarray(model.shape_transform, np.float64).reshape(-1, 7), np.asarray(model.shape_scale, np.float64).reshape(-1, 3)
    centres, radii = [], []
    for slot in s.slots:
        sid = t.shape_local0 + world * t.ns + slot if slot < t.ns else int(t.gshape_id[slot - t.ns])
        body = int(t.shape_body[slot])
        p = xf[sid, :3] if body < 0 else bq[body, :3] + sensors._qrot(bq[body, 3:], xf[sid, :3])
        centres.append(p)
        radii.append(bounding_radius(int(t.shape_type[slot]), sc[sid]))
    centres = np.array(centres)
    counts = []
    cones = np.asarray(s.block_cones, np.float64).reshape(-1, 5)
    per_cam = len(cones) // s.camera_count
    for b, (ax, ay, az, ch, sh) in enumerate(cones):
        O, A = np.asarray(s.ray_origins[b // per_cam], np.float64), np.array([ax, ay, az])
        n = 0
        for c, r in zip(centres, radii):
            v = c - O
            drop = ch > 0.0 and r is not None and (np.linalg.norm(np.cross(v, A)) * ch - v @ A * sh
                                                  > r + CULL_REL * (np.linalg.norm(v) + r) + CULL_ABS)
            n += not drop
        counts.append(n)
    return np.array(counts)


GRAZE_IMAGE, GRAZE_PIXEL, GRAZE_RANGE, GRAZE_RADIUS = (16, 16), (7, 7), 2.0, 0.01
GRAZE_CAMERA = (-1, look_at((0.0, -3.0, 1.0), (0.0, 0.0, 1.0)))


def graze_model(device=None):
    """Two worlds of one box on the ground, and two global spheres of 1 cm radius, two metres from GRAZE_CAMERA (16 x 16 pixels):
    one centred on the ray of pixel (7, 7) -- the corner of block 0 where four blocks meet; from the eye it is a disc of 0.3 degrees,
    a quarter of a pixel -- and one OUTSIDE every ray, beyond the outer edge of block 1's cone by the radius plus HALF the kernel's
    cull margin (1 mm of 2 mm): a test without margin drops it, the kernel's keeps it, a margin of the wrong sign drops it.
    Returns (model, Newton shape id of the first sphere, of the second)."""
    W, H = GRAZE_IMAGE
    lens = sensors.pinhole_rays(W, H, FOV_Y).astype(np.float64)
    p, q = GRAZE_CAMERA[1][:3], GRAZE_CAMERA[1][3:]
    d = lens[GRAZE_PIXEL[0] * W + GRAZE_PIXEL[1]]
    centre = p + GRAZE_RANGE * sensors._qrot(q, d / np.linalg.norm(d))
    ax, ay, az, ch, sh = sensors.camera_block_cones(sensors._qrot(q, lens).astype(np.float32)[None], W, H)[0, 1].astype(np.float64)
    A, F = np.array([ax, ay, az]) / np.linalg.norm([ax, ay, az]), sensors._qrot(q, np.array([0.0, 0.0, -1.0]))
    out = A * (A @ F) - F  # perpendicular to the cone's axis, away from the optical axis: towards the image's corner
    out /= np.linalg.norm(out)
    gap = GRAZE_RADIUS + 0.5 * (CULL_REL * (GRAZE_RANGE + GRAZE_RADIUS) + CULL_ABS)  # distance from the centre to the cone's mantle
    ang = np.arctan2(sh, ch) + np.arcsin(gap / GRAZE_RANGE)
    band = p + GRAZE_RANGE * (np.cos(ang) * A + np.sin(ang) * out)
    env = nt.ModelBuilder()
    b = env.add_body(xform=[0.0, 0.5, 0.3, 0.0, 0.0, 0.0, 1.0])
    env.add_shape_box(b, hx=0.1, hy=0.1, hz=0.1)
    scene = nt.ModelBuilder()
    scene.replicate(env, 2)
    scene.add_ground_plane()
    for c in (centre, band):
        scene.add_shape_sphere(-1, xform=[*c, 0.0, 0.0, 0.0, 1.0], radius=GRAZE_RADIUS)
    model = scene.finalize(device=device)
    return model, int(model.env.gshape_id[1]), int(model.env.gshape_id[2])


def check_graze(sid, band_id, K, distance, shape, survivors, off_distance, off_shape):
    """Block 0 keeps the grazed sphere and pixel (7, 7) hits it with the cull on; the images with the cull on and off are the same;
    the blocks a sphere's disc does not reach drop it, and the sphere inside the margin's band stays in block 1 unseen."""
    i, j = GRAZE_PIXEL
    assert np.all(shape[:, 0, i, j] == sid) and np.all(np.abs(distance[:, 0, i, j] - (GRAZE_RANGE - GRAZE_RADIUS)) < 1e-3)
    assert np.array_equal(distance.view(np.uint32), off_distance.view(np.uint32)) and np.array_equal(shape, off_shape)
    assert 1 <= np.sum(shape[0] == sid) <= 4 and not np.any(shape == band_id)
    # block 0 (top left): the ground and the grazed sphere; block 1: the ground and the sphere in the band -- the grazed one, 14 degrees
    # off its axis, is dropped by its 12-degree cone; blocks 2 and 3 (the lower half): the ground and the box, which straddles the
    # middle column
    assert K == 4 and np.array_equal(survivors, [[2, 2, 2, 2]] * len(survivors))


def shapes_per_block(shape, width, height):
    """[..., blocks per camera * C] the number of distinct shape ids hit in every 8 x 8 block of `shape` [E, C, H, W]."""
    E, Cn = shape.shape[:2]
    by, bx = (height + TILE - 1) // TILE, (width + TILE - 1) // TILE
    out = np.zeros((E, Cn, by * bx), np.int64)
    for e in range(E):
        for c in range(Cn):
            for r in range(by):
                for q in range(bx):
                    ids = shape[e, c, r * TILE:(r + 1) * TILE, q * TILE:(q + 1) * TILE]
                    out[e, c, r * bx + q] = len(np.unique(ids[ids >= 0]))
    return out.reshape(E, -1)
