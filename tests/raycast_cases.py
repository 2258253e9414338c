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


def primitive_scene(world_count, device=None, seed=3, jitter=True):
    """tests/scenes.py::mixed_primitive_scene (the same seven bodies, poses and ground plane) plus a cone body, and a finite plane
    (0.5 m x 0.3 m half extents, tilted, 0.45 m up) as a second global shape."""
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
    scene.add_shape_plane(xform=[0.9, 0.1, 0.45, *nt._np_math.quat_rpy(0.3, -0.4, 0.2)], width=0.5, length=0.3)
    model = scene.finalize(device=device)
    if jitter:
        off = rng.uniform(-0.02, 0.02, size=(model.body_count, 3)).astype(np.float32)
        model.body_q[:, :3] += off
        model.joint_q.reshape(-1, 7)[:, :3] += off
    return model


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def primitive_rays(seed=11):
    """(origins [70, 3], directions [70, 3], ray_body [70]) float32 / int32: world-frame rays from a shell around the scene aimed at
    and around the shapes, rays from below the ground (its back face), rays that look away (misses), and body-attached rays, some of
    which start at the body's origin -- inside its shape."""
    rng = np.random.default_rng(seed)
    nb = len(SPECS)
    centres = np.array([[0.35 * (k % 3) - 0.3, 0.4 * (k // 3) - 0.3, 0.12 + 0.02 * k] for k in range(nb)] + [[0.9, 0.1, 0.45]] * 2)
    o, d, body = [], [], []
    for i in range(N_RAYS):
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


# name -> (model factory(device, jitter), rays, sensor keyword arguments)
CASES = {
    "primitives": (lambda device=None, jitter=True: primitive_scene(N_WORLDS, device=device, jitter=jitter), primitive_rays, {}),
    "terrain_scan": (lambda device=None, jitter=True: terrain_model(False, device=device, jitter=jitter), scan_rays, {"exclude_bodies": (0,)}),
    "terrain_skim": (lambda device=None, jitter=True: terrain_model(False, device=device, jitter=jitter), skim_rays, {}),
    "hfield_scan": (lambda device=None, jitter=True: terrain_model(True, device=device, jitter=jitter), scan_rays, {"exclude_bodies": (0,)}),
    "hfield_skim": (lambda device=None, jitter=True: terrain_model(True, device=device, jitter=jitter), skim_rays, {}),
}


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
            if block_bounds:  # (the scenes carry one mesh: its blocks start at 0)
                assert len({(int(x), int(y)) for x, y in tr if y > 0}) == 1
                i0 = int(np.flatnonzero(tr[:, 1] > 0)[0])
                k["bb"] = triangle_block_bounds(k["v"][vr[i0, 0]:vr[i0, 0] + vr[i0, 1]], k["i"][tr[i0, 0]:tr[i0, 0] + tr[i0, 1]])
                k["bs"] = np.zeros(len(vr), np.int32)
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


def emu_cast(H, em, state, args):
    import ctypes as C

    d = state.desc()
    return H.lib().nt_raycast(C.byref(em.desc), C.byref(d), C.byref(args.desc), None)
