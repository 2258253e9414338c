"""Scenes, ray sets and the comparison rule shared by tests/test_raycast_host.py, test_raycast_emu.py and test_gpu_raycast.py
(test infrastructure).  The reference is the float64 host path of newton_amd.sensors on the same fp32 inputs.

Which rays are compared is decided from the reference alone: a ray is CLEAR when the reference gives the same hit / miss and the same
shape id for the ray and for its four copies whose origins are shifted by +-SHIFT along two directions perpendicular to the ray
(1e-4 m: two decades above fp32 rounding at the scenes' 3 m scale); its normal is compared when the five reference normals lie within
NORMAL_SPREAD of one another.  fp32 and float64 may disagree at silhouettes and facet edges; nowhere else."""
import numpy as np

import newton_amd as nt
from newton_amd import sensors
from newton_amd.enums import GeoType
from scenes import terrain_scene

N_WORLDS, N_RAYS = 37, 70
SHIFT, NORMAL_SPREAD = 1e-4, 0.05
MAX_DISTANCE = 6.0
# Gates on clear rays, |t_dev - t_ref| / max(1, t_ref) and the angle between the normals: 4 x the largest value measured over the five
# cases (`raycast_kernel`, lists them per case, emulator and MI355X): 1.41e-06 and 3.08e-05 rad, both on the
# primitive scene.  The distance gate stays below the project's single-call kinematics gate of 1e-5 (test_eval_ik_host.Q_GATE).
DISTANCE_GATE = 4 * 1.41e-6
NORMAL_GATE = 4 * 3.08e-5
SPECS = ["sphere", "capsule", "box", "cylinder", "ellipsoid", "sphere", "capsule", "cone"]


def primitive_scene(world_count, device=None, seed=3, jitter=True, finite_plane=True, extra_spheres=0):
    """tests/scenes.py::mixed_primitive_scene (the same seven bodies, poses and ground plane) plus a cone body, and a finite plane
    (0.5 m x 0.3 m half extents, tilted, 0.45 m up) as a second global shape.  extra_spheres: that many global spheres of 1 cm radius
    on a 5 cm grid 2.5 m up, away from everything else (the launch-shape scenes choose their target count with them)."""
    rng = np.random.default_rng(seed)
    env = nt.ModelBuilder()
    for k, kind in enumerate(SPECS):
        q = nt._np_math.quat_rpy(*rng.uniform(-1.0, 1.0, size=3))
        b = env.add_body(xform=[0.35 * (k % 3) - 0.3, 0.4 * (k // 3) - 0.3, 0.12 + 0.02 * k, *q])
        if kind == "sphere":
            env.add_shape_sphere(b, radius=0.1)
        elif kind == "capsule":
            env.add_shape_capsule(b, radius=0.07, half_height=0.15)
        elif kind == "box":
            env.add_shape_box(b, hx=0.1, hy=0.08, hz=0.06)
        elif kind == "cylinder":
            env.add_shape_cylinder(b, radius=0.08, half_height=0.1)
        elif kind == "cone":
            env.add_shape_cone(b, radius=0.09, half_height=0.12)
        else:
            env.add_shape_ellipsoid(b, rx=0.12, ry=0.08, rz=0.06)
    scene = nt.ModelBuilder()
    scene.replicate(env, world_count)
    scene.add_ground_plane()
    if finite_plane:
        scene.add_shape_plane(xform=[0.9, 0.1, 0.45, *nt._np_math.quat_rpy(0.3, -0.4, 0.2)], width=0.5, length=0.3)
    for i in range(extra_spheres):
        scene.add_shape_sphere(-1, xform=[*small_sphere_centre(i), 0.0, 0.0, 0.0, 1.0], radius=SMALL_RADIUS)
    model = scene.finalize(device=device)
    if jitter:
        off = rng.uniform(-0.02, 0.02, size=(model.body_count, 3)).astype(np.float32)
        model.body_q[:, :3] += off
        model.joint_q.reshape(-1, 7)[:, :3] += off
    return model


SMALL_RADIUS, SMALL_PER_ROW = 0.01, 45


def small_sphere_centre(i):
    return [-1.0 + 0.05 * (i % SMALL_PER_ROW), -1.0 + 0.05 * (i // SMALL_PER_ROW), 2.5]


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def primitive_rays(seed=11, count=N_RAYS):
    """(origins [70, 3], directions [70, 3], ray_body [70]) float32 / int32: world-frame rays from a shell around the scene aimed at
    and around the shapes, rays from below the ground (its back face), rays that look away (misses), and body-attached rays, some of
    which start at the body's origin -- inside its shape."""
    rng = np.random.default_rng(seed)
    nb = len(SPECS)
    centres = np.array([[0.35 * (k % 3) - 0.3, 0.4 * (k // 3) - 0.3, 0.12 + 0.02 * k] for k in range(nb)] + [[0.9, 0.1, 0.45]] * 2)
    o, d, body = [], [], []
    for i in range(count):
        kind = i % 7
        if kind in (0, 1, 2):  # from the upper shell at a shape, +- 0.12 m
            az, el, r = rng.uniform(0, 2 * np.pi), rng.uniform(0.15, 1.3), rng.uniform(1.5, 3.0)
            org = np.array([0.2, 0.2, 0.1]) + r * np.array([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)])
            tgt = centres[rng.integers(len(centres))] + rng.uniform(-0.12, 0.12, size=3)
            o.append(org); d.append(tgt - org); body.append(-1)
        elif kind == 3:  # from below the ground, upwards: the plane's back face is culled
            org = np.array([rng.uniform(-0.6, 1.0), rng.uniform(-0.6, 0.8), rng.uniform(-1.0, -0.3)])
            tgt = centres[rng.integers(nb)] + rng.uniform(-0.15, 0.15, size=3)
            o.append(org); d.append((tgt - org) * rng.uniform(0.2, 3.0)); body.append(-1)  # (directions need not be unit)
        elif kind == 4:  # looking away: up and outwards
            org = np.array([rng.uniform(-0.5, 0.9), rng.uniform(-0.5, 0.7), rng.uniform(0.5, 1.2)])
            o.append(org); d.append(np.array([rng.normal(), rng.normal(), rng.uniform(0.05, 1.0)])); body.append(-1)
        elif kind == 5:  # attached to a body, from its origin: inside its own shape
            o.append(np.zeros(3)); d.append(rng.normal(size=3)); body.append(int(rng.integers(nb)))
        else:  # attached to a body, from outside its shape
            v = _unit(rng.normal(size=3))
            o.append(0.35 * v); d.append(_unit(rng.normal(size=3)) - 0.5 * v); body.append(int(rng.integers(nb)))
    return np.array(o, np.float32), np.array(d, np.float32), np.array(body, np.int32)


def terrain_model(heightfield, world_count=N_WORLDS, device=None, seed=21, jitter=True):
    """terrain_scene(world_count, cells=9) with body 0 of every world lifted 0.6 .. 0.9 m above the field and tilted by a seeded random
    pose (the scanner's carrier)."""
    model = terrain_scene(world_count, cells=9, heightfield=heightfield, device=device)
    rng = np.random.default_rng(seed)
    nb = model.body_count // world_count
    for w in range(world_count):
        if not jitter and w > 0:
            model.body_q[w * nb:(w + 1) * nb] = model.body_q[:nb]
            continue
        q = nt._np_math.quat_rpy(rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(-3.0, 3.0))
        model.body_q[w * nb] = [rng.uniform(-0.7, 0.7), rng.uniform(-0.7, 0.7), rng.uniform(0.6, 0.9), *q]
    model.joint_q.reshape(-1, 7)[:] = model.body_q
    return model


def scan_rays():
    """A 7 x 10 grid pointing down from body 0; the body's tilt swings some of the rays out of the 3.2 m field."""
    xs, ys = np.linspace(-0.9, 0.9, 7), np.linspace(-1.2, 1.2, 10)
    o = np.array([[x, y, 0.0] for x in xs for y in ys], np.float32)
    return o, np.tile(np.array([0.0, 0.0, -1.0], np.float32), (N_RAYS, 1)), np.zeros(N_RAYS, np.int32)


def skim_rays(seed=13):
    """70 world-frame rays 6 .. 20 degrees below the horizon from 0.1 .. 0.45 m above the field (they walk many cells), every fifth one
    from below the terrain upwards (its back faces), every seventh one above the horizon (a miss)."""
    rng = np.random.default_rng(seed)
    o, d = [], []
    for i in range(N_RAYS):
        az = rng.uniform(0, 2 * np.pi)
        el = -np.deg2rad(rng.uniform(6.0, 20.0))
        org = np.array([rng.uniform(-1.4, 1.4), rng.uniform(-1.4, 1.4), rng.uniform(0.1, 0.45)])
        if i % 5 == 4:
            org[2], el = rng.uniform(-0.5, -0.1), np.deg2rad(rng.uniform(8.0, 40.0))
        elif i % 7 == 6:
            el = np.deg2rad(rng.uniform(1.0, 20.0))
        o.append(org); d.append([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)])
    return np.array(o, np.float32), np.array(d, np.float32), np.full(N_RAYS, -1, np.int32)


# ---------------------------------------------------------------------------------------------------------------------------------
# table layouts: a field that is not square, two heightfields, two meshes (5 worlds; the carrier is body 0 of every world)
# ---------------------------------------------------------------------------------------------------------------------------------
LAYOUT_WORLDS = 5


def _carrier_env():
    """Body 0, the scanner's carrier, with a 5 cm sphere the scan excludes, and a box resting beside the field's centre."""
    env = nt.ModelBuilder()
    b = env.add_body(xform=[0.0, 0.0, 0.8, 0.0, 0.0, 0.0, 1.0])
    env.add_shape_sphere(b, radius=0.05)
    b = env.add_body(xform=[-0.45, 0.3, 0.3, *nt._np_math.quat_rpy(0.3, 0.2, 0.5)])
    env.add_shape_box(b, hx=0.1, hy=0.08, hz=0.06)
    return env


def _place_carriers(model, seed, x_range, y_range, z_range=(0.6, 0.9), tilt=0.5):
    rng = np.random.default_rng(seed)
    E = model.env.env_count
    nb = model.body_count // E
    for w in range(E):
        q = nt._np_math.quat_rpy(rng.uniform(-tilt, tilt), rng.uniform(-tilt, tilt), rng.uniform(-3.0, 3.0))
        model.body_q[w * nb] = [rng.uniform(*x_range), rng.uniform(*y_range), rng.uniform(*z_range), *q]
    model.joint_q.reshape(-1, 7)[:] = model.body_q
    return model


def layout_height(x, y):
    """Not symmetric in x, in y, or under their exchange."""
    return 0.03 * np.sin(2.3 * x + 0.4) * np.cos(3.1 * y - 0.2) + 0.02 * x - 0.015 * y


def _heightfield(nrow, ncol, hx, hy):
    raw = np.array([[layout_height(x, y) for x in np.linspace(-hx, hx, ncol)] for y in np.linspace(-hy, hy, nrow)], np.float32)
    return nt.Heightfield(raw, nrow, ncol, hx=hx, hy=hy)


def grid_mesh(ncx, ncy, hx, hy):
    """ncx x ncy cells, two triangles each, wound to face +z."""
    xs, ys = np.linspace(-hx, hx, ncx + 1), np.linspace(-hy, hy, ncy + 1)
    pts = np.array([(x, y, layout_height(2.0 * x, 2.0 * y)) for y in ys for x in xs], np.float32)
    idx = []
    for j in range(ncy):
        for i in range(ncx):
            a, b, c, d = j * (ncx + 1) + i, j * (ncx + 1) + i + 1, (j + 1) * (ncx + 1) + i, (j + 1) * (ncx + 1) + i + 1
            idx += [a, b, d, a, d, c]
    return nt.Mesh(pts, np.array(idx, np.int32))


RECT = dict(nrow=7, ncol=12, hx=1.8, hy=0.9, yaw=0.5)


def hfield_rect_model(device=None, jitter=True):
    """One heightfield of 7 rows x 12 columns over 3.6 m x 1.8 m (dx = 0.327 m, dy = 0.3 m), turned 0.5 rad about z."""
    scene = nt.ModelBuilder()
    scene.replicate(_carrier_env(), LAYOUT_WORLDS)
    scene.add_shape_heightfield(xform=[0.0, 0.0, 0.0, *nt._np_math.quat_rpy(0.0, 0.0, RECT["yaw"])],
                                heightfield=_heightfield(RECT["nrow"], RECT["ncol"], RECT["hx"], RECT["hy"]))
    return _place_carriers(scene.finalize(device=device), 31, (-0.8, 0.8), (-0.3, 0.3), tilt=0.3)


def _mixed_rays(scan_scale, skim_scale, skim_yaw=0.0):
    """35 rays of the scan grid (attached to body 0) and 35 of the skim set (world frame), rescaled to a field."""
    so, sd, sb = scan_rays()
    ko, kd, kb = skim_rays()
    so, sd, sb = so[::2] * np.array([*scan_scale, 1.0], np.float32), sd[::2], sb[::2]
    c, s_ = np.cos(skim_yaw), np.sin(skim_yaw)
    turn = np.array([[c, -s_, 0.0], [s_, c, 0.0], [0.0, 0.0, 1.0]])
    ko = (ko[:35] * np.array([*skim_scale, 1.0])) @ turn.T
    kd = kd[:35] @ turn.T
    return (np.concatenate([so, ko]).astype(np.float32), np.concatenate([sd, kd]).astype(np.float32), np.concatenate([sb, kb[:35]]).astype(np.int32))


def hfield_rect_rays():
    return _mixed_rays((1.0, 0.4), (1.8 / 1.6, 0.9 / 1.6), RECT["yaw"])


def hfield_two_model(device=None, jitter=True):
    """The 10 x 10 field of the other scenes' size, and a second field of 6 rows x 9 columns (1.2 m x 0.8 m) floating 0.35 m above
    it, tilted: its record has data_offset = 100."""
    scene = nt.ModelBuilder()
    scene.replicate(_carrier_env(), LAYOUT_WORLDS)
    scene.add_shape_heightfield(heightfield=_heightfield(10, 10, 1.6, 1.6))
    scene.add_shape_heightfield(xform=[0.4, -0.25, 0.35, *nt._np_math.quat_rpy(0.15, -0.1, 0.8)], heightfield=_heightfield(6, 9, 0.6, 0.4))
    return _place_carriers(scene.finalize(device=device), 32, (0.1, 0.7), (-0.55, 0.05))


def hfield_two_rays():
    return _mixed_rays((1.0, 0.6), (1.0, 1.0))


MESH_TWO_SCALE = (1.5, 0.5, 2.0)


def mesh_two_model(device=None, jitter=True):
    """The terrain mesh (9 x 9 cells, 162 triangles, a global shape) and a second mesh of 7 x 10 cells (140 triangles: three blocks,
    the last one partial) carried by body 0, 0.25 m under it, tilted and scaled by (1.5, 0.5, 2.0).  The terrain is added first, so
    the carried mesh has non-zero vertex, triangle and block starts."""
    xs = np.linspace(-1.6, 1.6, 10)
    from scenes import terrain_height

    pts = np.array([(x, y, terrain_height(x, y)) for y in xs for x in xs], np.float32)
    idx = []
    for j in range(9):
        for i in range(9):
            a, b, c, d = j * 10 + i, j * 10 + i + 1, (j + 1) * 10 + i, (j + 1) * 10 + i + 1
            idx += [a, b, d, a, d, c]
    scene = nt.ModelBuilder()
    scene.add_shape_mesh(-1, mesh=nt.Mesh(pts, np.array(idx, np.int32)))
    env = _carrier_env()
    cfg = nt.ModelBuilder.ShapeConfig(has_shape_collision=False)  # (a ray target only: the build has no mesh-mesh contact leg)
    env.add_shape_mesh(0, xform=[0.0, 0.0, -0.25, *nt._np_math.quat_rpy(0.2, -0.15, 0.4)], mesh=grid_mesh(7, 10, 0.44, 0.66), scale=MESH_TWO_SCALE,
                       cfg=cfg)
    scene.replicate(env, LAYOUT_WORLDS)
    return _place_carriers(scene.finalize(device=device), 33, (-0.7, 0.7), (-0.7, 0.7))


def mesh_two_rays():
    """The scan grid from body 0 (the middle of it meets the carried mesh, the rest the terrain); its four corner rays look up."""
    o, d, body = scan_rays()
    d = d.copy()
    d[[0, 9, 60, 69]] = [0.1, 0.2, 1.0]
    return o, d, body


# ---------------------------------------------------------------------------------------------------------------------------------
# launch shapes: the primitive scene's eight bodies and ground in 5 worlds, and a chosen number of small global spheres
# ---------------------------------------------------------------------------------------------------------------------------------
LAUNCH_RAYS = 257
LAUNCH_SMALL = (0, 44, 150, 299, 600, 899, 298, 898)  # the small spheres the rays 7, 15, 23, ... are aimed at, in turn


def launch_model(extra_spheres=0, device=None):
    return primitive_scene(LAYOUT_WORLDS, device=device, finite_plane=False, extra_spheres=extra_spheres)


def launch_rays():
    """P: 257 rays built like primitive_rays; every eighth one goes up at one of the LAUNCH_SMALL spheres from 1 m below it, a
    third of its radius off its axis (a miss while the scene does not hold that sphere)."""
    o, d, body = primitive_rays(seed=17, count=LAUNCH_RAYS)
    for n, i in enumerate(range(7, LAUNCH_RAYS, 8)):
        c = np.array(small_sphere_centre(LAUNCH_SMALL[n % len(LAUNCH_SMALL)]))
        o[i], d[i], body[i] = c + [0.003, -0.002, -1.0], [0.0, 0.0, 2.0], -1
    return o, d, body


# name -> (model factory(device, jitter), rays, sensor keyword arguments)
CASES = {
    "primitives": (lambda device=None, jitter=True: primitive_scene(N_WORLDS, device=device, jitter=jitter), primitive_rays, {}),
    "terrain_scan": (lambda device=None, jitter=True: terrain_model(False, device=device, jitter=jitter), scan_rays, {"exclude_bodies": (0,)}),
    "terrain_skim": (lambda device=None, jitter=True: terrain_model(False, device=device, jitter=jitter), skim_rays, {}),
    "hfield_scan": (lambda device=None, jitter=True: terrain_model(True, device=device, jitter=jitter), scan_rays, {"exclude_bodies": (0,)}),
    "hfield_skim": (lambda device=None, jitter=True: terrain_model(True, device=device, jitter=jitter), skim_rays, {}),
    "hfield_rect": (hfield_rect_model, hfield_rect_rays, {"exclude_bodies": (0,)}),
    "hfield_two": (hfield_two_model, hfield_two_rays, {"exclude_bodies": (0,)}),
    "mesh_two": (mesh_two_model, mesh_two_rays, {}),
}
LAYOUT_CASES = ("hfield_rect", "hfield_two", "mesh_two")


def perpendicular_shifts(directions):
    """Two unit vectors perpendicular to every direction (in the ray's own frame; a rotation keeps them perpendicular)."""
    d = _unit(np.asarray(directions, np.float64))
    helper = np.where(np.abs(d[..., :1]) < 0.9, np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]))
    u = _unit(np.cross(d, helper))
    return u, np.cross(d, u)


def reference(model, body_q, rays, **kw):
    """The float64 host contract for the ray set, plus the clear / normal-comparable masks from the four shifted copies.  Computed once
    per case and shared (see `case`); nothing writes into it."""
    o, d, body = rays
    s = sensors.SensorRaycast(model, o, d, ray_body=body, max_distance=MAX_DISTANCE, **kw)
    u, v = perpendicular_shifts(d)
    runs = [sensors.raycast_numpy(model, body_q, o.astype(np.float64) + sh, d, body, MAX_DISTANCE, s.slots)
            for sh in (0.0, SHIFT * u, -SHIFT * u, SHIFT * v, -SHIFT * v)]
    dist, normal, shape = runs[0]
    clear = np.all([(r[0] >= 0.0) == (dist >= 0.0) for r in runs], axis=0) & np.all([r[2] == shape for r in runs], axis=0)
    cos = np.min([np.sum(a[1] * b[1], axis=-1) for a in runs for b in runs], axis=0)
    normal_ok = clear & (dist >= 0.0) & (np.arccos(np.clip(cos, -1.0, 1.0)) <= NORMAL_SPREAD)
    return dict(distance=dist, normal=normal, shape=shape, clear=clear, normal_ok=normal_ok, slots=s.slots)


_HOST = {}


def case(name):
    """(host model, rays, sensor kwargs, reference dict at the model's own body_q), built once."""
    if name not in _HOST:
        make, rays, kw = CASES[name]
        model = make()
        r = rays()
        _HOST[name] = (model, r, kw, reference(model, model.body_q, r, **kw))
    return _HOST[name]


def compare(ref, distance, normal, shape, label):
    """Hit / miss and shape id equal on the clear rays; returns (max distance error, max normal angle) over them, printed."""
    distance, normal, shape = np.asarray(distance, np.float64), np.asarray(normal, np.float64), np.asarray(shape)
    c = ref["clear"]
    assert np.array_equal((distance >= 0.0)[c], (ref["distance"] >= 0.0)[c]), f"{label}: hit / miss differs on clear rays"
    assert np.array_equal(shape[c], ref["shape"][c]), f"{label}: shape id differs on clear rays"
    assert np.all(distance[distance < 0.0] == -1.0) and np.all(shape[distance < 0.0] == -1) and np.all(normal[distance < 0.0] == 0.0)
    hit = c & (ref["distance"] >= 0.0)
    err_d = np.abs(distance - ref["distance"])[hit] / np.maximum(1.0, ref["distance"][hit])
    k = ref["normal_ok"]
    # (atan2 of |a x b| and a . b: arccos loses half the digits at small angles, 1 - 1e-7 reads as 4e-4 rad)
    ang = np.arctan2(np.linalg.norm(np.cross(normal[k], ref["normal"][k]), axis=-1), np.sum(normal[k] * ref["normal"][k], axis=-1))
    assert np.all(np.abs(np.linalg.norm(normal[distance >= 0.0], axis=-1) - 1.0) < 1e-5)
    out = float(err_d.max()), float(ang.max())
    print(f"[raycast] {label}: clear {c.mean():.3f}, hits {hit.sum()}, max |dt| / max(1, t) = {out[0]:.3e}, max normal angle = {out[1]:.3e} rad "
          f"({k.sum()} normals)")
    return out


def hit_types(model, ref):
    """GeoTypes hit by clear rays."""
    ids = np.unique(ref["shape"][ref["clear"] & (ref["shape"] >= 0)])
    return {int(np.asarray(model.shape_type)[i]) for i in ids}


ALL_TARGET_TYPES = {int(g) for g in (GeoType.PLANE, GeoType.HFIELD, GeoType.SPHERE, GeoType.CAPSULE, GeoType.ELLIPSOID, GeoType.CYLINDER,
                                     GeoType.BOX, GeoType.MESH, GeoType.CONE)}


# ---------------------------------------------------------------------------------------------------------------------------------
# nt_raycast on host arrays: the emulated library (tests/emu) takes numpy arrays where the product passes device pointers
# ---------------------------------------------------------------------------------------------------------------------------------
class HostArgs:
    """nt_raycast_args over numpy arrays for `model`, the tables built the way SensorRaycast builds its device copies."""

    def __init__(self, model, rays, slots, max_distance=MAX_DISTANCE, per_world=False, block_bounds=True, want_normal=True, want_shape=True):
        import ctypes as C

        from newton_amd import _lib as L
        from newton_amd.mesh import triangle_block_bounds

        t = model.env
        E = t.env_count
        o, d, body = rays
        if per_world and o.ndim == 2:
            o, d = np.tile(o, (E, 1, 1)), np.tile(d, (E, 1, 1))
        R = o.shape[-2]
        ptr = lambda a: a.ctypes.data_as(C.c_void_p).value  # noqa: E731
        self.keep = k = dict(o=np.ascontiguousarray(o, np.float32), d=np.ascontiguousarray(d, np.float32), body=np.ascontiguousarray(body, np.int32))
        k["targets"] = np.ascontiguousarray(np.stack([slots, np.asarray(t.shape_type)[slots]], axis=1), np.int32).reshape(-1, 2)
        self.distance = np.full((E, R), 7.0, np.float32)  # poisoned: the call overwrites every selected row
        self.normal = np.full((E, R, 3), 7.0, np.float32) if want_normal else None
        self.shape = np.full((E, R), -7, np.int32) if want_shape else None  # (7 is a shape id)
        a = L.nt_raycast_args()
        a.ray_count, a.rays_per_world = R, int(o.ndim == 3)
        a.origins, a.directions, a.ray_body = ptr(k["o"]), ptr(k["d"]), ptr(k["body"])
        a.max_distance, a.target_count = max_distance, len(slots)
        a.targets = a.targets_host = ptr(k["targets"])
        a.distance = ptr(self.distance)
        a.normal = None if self.normal is None else ptr(self.normal)
        a.shape = None if self.shape is None else ptr(self.shape)
        types = k["targets"][:, 1]
        if np.any(types == int(GeoType.MESH)):
            vr, tr = np.asarray(model.mesh_vertex_range, np.int32).reshape(-1, 2), np.asarray(model.mesh_triangle_range, np.int32).reshape(-1, 2)
            k["vr"], k["tr"] = np.ascontiguousarray(vr), np.ascontiguousarray(tr)
            k["v"], k["i"] = np.ascontiguousarray(model.mesh_vertices, np.float32), np.ascontiguousarray(model.mesh_indices, np.int32)
            a.shape_vertex_range, a.shape_triangle_range, a.vertices, a.indices = ptr(k["vr"]), ptr(k["tr"]), ptr(k["v"]), ptr(k["i"])
            if block_bounds:  # one table per distinct mesh, each shape pointing at its mesh's first block
                blk_start, blk_of, tables, n_blk = np.zeros(len(vr), np.int32), {}, [], 0
                for i in range(len(vr)):
                    if tr[i, 1] <= 0:
                        continue
                    key = (int(vr[i, 0]), int(tr[i, 0]), int(tr[i, 1]))
                    if key not in blk_of:
                        blk_of[key] = n_blk
                        tables.append(triangle_block_bounds(k["v"][vr[i, 0]:vr[i, 0] + vr[i, 1]], k["i"][tr[i, 0]:tr[i, 0] + tr[i, 1]]))
                        n_blk += len(tables[-1])
                    blk_start[i] = blk_of[key]
                k["bb"], k["bs"] = np.ascontiguousarray(np.concatenate(tables), np.float32), blk_start
                a.block_bounds, a.shape_block_start = ptr(k["bb"]), ptr(k["bs"])
        if np.any(types == int(GeoType.HFIELD)):
            hf = (L.nt_heightfield * model.heightfield_count)()
            for n, (off, nrow, ncol, hx, hy, zlo, zhi) in enumerate(model.heightfield_data):
                hf[n] = L.nt_heightfield(int(off), int(nrow), int(ncol), float(hx), float(hy), float(zlo), float(zhi))
            k["hf"], k["hi"] = hf, np.ascontiguousarray(model.shape_heightfield_index, np.int32)
            k["he"] = np.ascontiguousarray(model.heightfield_elevations, np.float32)
            a.shape_heightfield_index, a.heightfields, a.elevations = ptr(k["hi"]), C.addressof(hf), ptr(k["he"])
        self.desc = a

    def set_world_mask(self, mask):
        self.keep["wm"] = np.ascontiguousarray(mask, np.uint8)
        self.desc.world_mask = self.keep["wm"].ctypes.data


# raycast_kernel's launch rule, restated from newton_amd/csrc/nt_mesh_plane.hip (RC_REC, RC_THREADS, RC_LDS_BYTES_PER_CU and nt_raycast's
# choice of the worlds per workgroup).  The launch-shape tests assert from it that every case lands on the path it is there for, and
# from the source text that the constants are still these: a later change fails the tests, it does not silently stop covering a path.
RC_REC, RC_THREADS, RC_LDS_BYTES_PER_CU, RC_DEFAULT_LDS = 12, 256, 160 * 1024, 48 * 1024


def launch_shape(ray_count, target_count):
    """(worlds per workgroup, lanes per world, dynamic LDS bytes) nt_raycast chooses."""
    wpb = 4 if ray_count <= 64 else (2 if ray_count <= 128 else 1)
    per_world = target_count * RC_REC * 4
    while wpb > 1 and wpb * per_world > RC_LDS_BYTES_PER_CU:
        wpb //= 2
    return wpb, RC_THREADS // wpb, wpb * per_world


def kernel_constants():
    """The three constants as the kernel source states them."""
    import os
    import re

    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "newton_amd", "csrc", "nt_mesh_plane.hip")).read()
    rec = int(re.search(r"constexpr int RC_REC = (\d+);", src).group(1))
    threads = int(re.search(r"constexpr int RC_THREADS = (\d+);", src).group(1))
    a, b = re.search(r"constexpr size_t RC_LDS_BYTES_PER_CU = (\d+) \* (\d+);", src).groups()
    assert "a->ray_count <= 64 ? 4 : (a->ray_count <= 128 ? 2 : 1)" in src and "lds_bytes > 48 * 1024" in src
    return rec, threads, int(a) * int(b)


# name -> (rays of P, small spheres, worlds per workgroup, the dynamic LDS request goes through hipFuncSetAttribute)
LAUNCH_PREFIXES = (1, 63, 64, 65, 128, 129, 256, 257)
# (wpb halved twice needs 1 707 targets and more: its float64 reference with the four shifted copies takes over ten seconds on a CPU, so
# that case is left out; one world per workgroup is reached through R > 128)
LAUNCH_TARGETS = {"lds_above_48k": (64, 300, 4, True), "wpb_halved_once": (64, 900, 2, True)}
_LAUNCH = {}


def launch_case(extra_spheres, ray_count):
    """(host model, rays P[:ray_count], reference), built once."""
    key = (extra_spheres, ray_count)
    if key not in _LAUNCH:
        model = _LAUNCH[("model", extra_spheres)] = _LAUNCH.get(("model", extra_spheres)) or launch_model(extra_spheres)
        rays = tuple(a[:ray_count] for a in launch_rays())
        _LAUNCH[key] = (model, rays, reference(model, model.body_q, rays))
    return _LAUNCH[key]


def small_sphere_ids(model):
    t = model.env
    return np.asarray(t.gshape_id)[1:].astype(np.int64)  # (global shape 0 is the ground)


def emu_cast(H, em, state, args):
    import ctypes as C

    d = state.desc()
    return H.lib().nt_raycast(C.byref(em.desc), C.byref(d), C.byref(args.desc), None)
