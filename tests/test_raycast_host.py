"""The float64 host path of newton_amd.sensors.SensorRaycast -- the reference of the kernel tests -- against closed-form answers, and
the conditions the comparison scenes of tests/raycast_cases.py have to meet (they are asserted, not measured)."""
import numpy as np
import pytest

import newton_amd as nt
from newton_amd import sensors
from newton_amd.enums import GeoType
from raycast_cases import ALL_TARGET_TYPES, CASES, N_RAYS, N_WORLDS, case, hit_types
from scenes import terrain_height, terrain_scene

E = 3
# body k at (k, 0, 1), identity rotation; (kind, top of the shape above the body origin along +z, extent along +x)
ROW = [("sphere", 0.1, 0.1), ("box", 0.06, 0.1), ("capsule", 0.22, 0.07), ("cylinder", 0.1, 0.08), ("ellipsoid", 0.06, 0.12), ("cone", 0.12, None)]


def row_scene(extra=None):
    env = nt.ModelBuilder()
    for k, (kind, _, _) in enumerate(ROW):
        b = env.add_body(xform=[float(k), 0.0, 1.0, 0.0, 0.0, 0.0, 1.0])
        if kind == "sphere":
            env.add_shape_sphere(b, radius=0.1)
        elif kind == "box":
            env.add_shape_box(b, hx=0.1, hy=0.08, hz=0.06)
        elif kind == "capsule":
            env.add_shape_capsule(b, radius=0.07, half_height=0.15)
        elif kind == "cylinder":
            env.add_shape_cylinder(b, radius=0.08, half_height=0.1)
        elif kind == "ellipsoid":
            env.add_shape_ellipsoid(b, rx=0.12, ry=0.08, rz=0.06)
        else:
            env.add_shape_cone(b, radius=0.09, half_height=0.12)
    if extra is not None:
        extra(env)
    scene = nt.ModelBuilder()
    scene.replicate(env, E)
    scene.add_ground_plane()
    return scene.finalize()


def cast(model, o, d, body=-1, state=None, **kw):
    s = sensors.SensorRaycast(model, np.asarray(o, np.float32), np.asarray(d, np.float32), ray_body=body, **kw)
    st = model.state() if state is None else state
    s.eval(st)
    return s


def test_rays_down_the_axis_of_every_primitive():
    model = row_scene()
    n = len(ROW)
    o = [[k, 0.0, 3.0] for k in range(n)]
    s = cast(model, o, [[0.0, 0.0, -1.0]] * n)
    for k, (kind, top, _) in enumerate(ROW):
        if kind == "cone":  # (the apex itself is a degenerate point: see the offset ray below)
            continue
        assert np.allclose(s.distance[:, k], 3.0 - (1.0 + top), rtol=0, atol=2e-8), kind  # (the sizes are float32 inputs: 0.1 is 0.1 + 1.5e-9)
        assert np.allclose(s.normal[:, k], [0.0, 0.0, 1.0], atol=1e-12), kind
        assert np.array_equal(s.shape[:, k], model.env.shape_local0 + np.arange(E) * model.env.ns + k), kind
    assert s.distance.dtype == np.float64 and s.shape.dtype == np.int32


def test_rays_from_the_side_and_the_cone():
    model = row_scene()
    o, d, want, normal = [], [], [], []
    for k, (kind, _, side) in enumerate(ROW):
        if side is not None:  # along -x at the body's height: the +x extreme
            o.append([k + 0.45, 0.0, 1.0]); d.append([-1.0, 0.0, 0.0]); want.append(0.45 - side); normal.append([1.0, 0.0, 0.0])
    # cone (body 5, apex up, k = r / (2 h) = 0.375): down at 0.03 m from the axis, the lateral surface at w = 0.03 / k below the apex
    kk, rho = 0.09 / 0.24, 0.03
    o.append([5.0 + rho, 0.0, 3.0]); d.append([0.0, 0.0, -1.0]); want.append(3.0 - (1.0 + 0.12 - rho / kk))
    normal.append(np.array([1.0, 0.0, kk]) / np.hypot(1.0, kk))
    # cone from below: the base disc
    o.append([5.02, 0.01, 0.5]); d.append([0.0, 0.0, 2.0]); want.append(1.0 - 0.12 - 0.5); normal.append([0.0, 0.0, -1.0])
    # cylinder (body 3) from above off the axis: the cap; capsule (body 2) along -y at z = 1.15 + 0.05: the upper hemisphere
    o.append([3.05, 0.02, 2.0]); d.append([0.0, 0.0, -1.0]); want.append(2.0 - 1.1); normal.append([0.0, 0.0, 1.0])
    hz = 0.05
    o.append([2.0, 0.5, 1.15 + hz]); d.append([0.0, -1.0, 0.0]); want.append(0.5 - np.sqrt(0.07 ** 2 - hz ** 2))
    normal.append([0.0, np.sqrt(0.07 ** 2 - hz ** 2) / 0.07, hz / 0.07])
    s = cast(model, o, d)
    assert np.allclose(s.distance, np.array(want)[None, :], rtol=0, atol=1e-6)  # (float32 inputs: 4.45 is off by 2e-7, and 0.03 m beside the cone's axis is 5.03 - 5)
    assert np.allclose(s.normal, np.array(normal)[None], atol=1e-6)


def test_rotated_pose_and_body_attached_rays():
    """The box turned a quarter about x shows its hy = 0.08 upwards; a ray attached to the body sees the shape as at identity."""
    model = row_scene()
    q = nt._np_math.quat_rpy(np.pi / 2, 0.0, 0.0)
    nb = model.env.nb
    state = model.state()
    bq = np.array(state.body_q, np.float32)
    bq[1::nb, 3:] = q
    state.body_q = bq
    s = cast(model, [[1.0, 0.0, 3.0], [0.0, 0.0, 0.5], [0.0, 0.0, 0.0]], [[0.0, 0.0, -1.0], [0.0, 0.0, -1.0], [0.0, 0.0, 0.0]], body=[-1, 1, 1], state=state,
             exclude_bodies=())
    assert np.allclose(s.distance[:, 0], 3.0 - 1.08, atol=1e-6)
    assert np.allclose(s.distance[:, 1], 0.5 - 0.06, atol=1e-6)  # in the body frame the box still has hz = 0.06
    assert np.allclose(s.normal[:, 1], [0.0, -1.0, 0.0], atol=1e-6)  # body +z is world -y after the turn
    assert np.all(s.distance[:, 2] == -1.0) and np.all(s.shape[:, 2] == -1) and np.all(s.normal[:, 2] == 0.0)  # zero direction: a miss


@pytest.mark.parametrize("heightfield", [False, True])
def test_vertical_ray_over_a_terrain_node(heightfield):
    model = terrain_scene(E, cells=9, heightfield=heightfield)
    xs = np.linspace(-1.6, 1.6, 10)
    nodes = [(2, 3), (5, 5), (7, 1)]
    o = np.array([[np.float32(xs[i]), np.float32(xs[j]), 0.5] for i, j in nodes], np.float32)
    terrain_slot = model.env.ns  # the one global shape
    mask = np.zeros(model.env.ns + model.env.ng, bool)
    mask[terrain_slot] = True
    s = cast(model, o, [[0.0, 0.0, -1.0]] * 3, shape_mask=mask)
    if heightfield:  # the node height as the HeightfieldData record stores it: min_z + h (max_z - min_z), float32 h
        off, nrow, ncol, hx, hy, zlo, zhi = model.heightfield_data[0]
        e = np.asarray(model.heightfield_elevations, np.float64).reshape(nrow, ncol)
        z = [float(np.float32(zlo)) + e[j, i] * (float(np.float32(zhi)) - float(np.float32(zlo))) for i, j in nodes]
        assert np.allclose(z, [terrain_height(xs[i], xs[j]) for i, j in nodes], atol=1e-7)
    else:
        z = [float(np.float32(terrain_height(xs[i], xs[j]))) for i, j in nodes]
    assert np.allclose(s.distance, 0.5 - np.array(z)[None, :], rtol=0, atol=1e-12 if not heightfield else 1e-7)
    assert np.all(s.shape == model.env.gshape_id[0])
    assert np.all(s.normal[..., 2] > 0.99)
    # from below: the back faces are culled, a heightfield is hit on its top only
    s = cast(model, o - np.array([0, 0, 1.0], np.float32), [[0.0, 0.0, 1.0]] * 3, shape_mask=mask)
    assert np.all(s.distance == -1.0)


def stacked(env):
    """Two boxes of one size in one place (a tie), and a third 0.5 m above them."""
    for z in (2.0, 2.0, 2.5):
        b = env.add_body(xform=[10.0, 0.0, z, 0.0, 0.0, 0.0, 1.0])
        env.add_shape_box(b, hx=0.2, hy=0.2, hz=0.1)


def test_nearest_shape_tie_rule_max_distance_and_facing():
    model = row_scene(stacked)
    t, n = model.env, len(ROW)
    ids = lambda slot: t.shape_local0 + np.arange(E) * t.ns + slot  # noqa: E731
    s = cast(model, [[10.0, 0.0, 4.0], [10.0, 0.0, 0.5], [10.05, 0.0, 2.0], [0.0, 0.0, 1.0], [20.0, 0.0, -1.0]],
             [[0.0, 0.0, -1.0], [0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [0.3, 0.2, 0.5], [0.0, 0.0, 1.0]])
    assert np.allclose(s.distance[:, 0], 4.0 - 2.6) and np.array_equal(s.shape[:, 0], ids(n + 2))  # the upper box is nearer from above
    assert np.allclose(s.distance[:, 1], 1.9 - 0.5) and np.array_equal(s.shape[:, 1], ids(n))  # a tie from below: the lower shape id
    # from inside the two lower boxes: neither is hit (their far faces look away), the ground is
    assert np.allclose(s.distance[:, 2], 2.0) and np.all(s.shape[:, 2] == t.gshape_id[0])
    assert np.all(s.distance[:, 3] == -1.0)  # from the centre of the sphere upwards: its own surface does not face the ray
    assert np.all(s.distance[:, 4] == -1.0)  # the ground plane from below
    near = cast(model, [[10.0, 0.0, 4.0]] * 2, [[0.0, 0.0, -1.0]] * 2, max_distance=1.4 - 1e-6)
    assert np.all(near.distance == -1.0)
    at = cast(model, [[10.0, 0.0, 4.0]], [[0.0, 0.0, -2.0]], max_distance=1.4 + 1e-6)  # t counts metres along the unit direction
    assert np.allclose(at.distance, 1.4)


def test_world_mask_exclude_bodies_and_shape_mask():
    model = row_scene()
    o, d = [[0.0, 0.0, 3.0], [1.0, 0.0, 3.0]], [[0.0, 0.0, -1.0]] * 2
    s = cast(model, o, d)
    s.distance[...], s.normal[...], s.shape[...] = 7.0, 7.0, 7
    s.eval(model.state(), world_mask=[True, False, True])
    assert np.all(s.distance[1] == 7.0) and np.all(s.normal[1] == 7.0) and np.all(s.shape[1] == 7)
    assert np.allclose(s.distance[[0, 2]], [[1.9, 1.94]] * 2)
    ex = cast(model, o, d, exclude_bodies=(0,))
    assert np.allclose(ex.distance, [[3.0, 1.94]] * E) and np.all(ex.shape[:, 0] == model.env.gshape_id[0])  # through to the ground
    mask = np.ones(model.env.ns + model.env.ng, bool)
    mask[[1, model.env.ns]] = False
    sm = cast(model, o, d, shape_mask=mask)
    assert np.allclose(sm.distance[:, 0], 1.9) and np.all(sm.distance[:, 1] == -1.0)
    # per-world rays and set_rays in place
    pw = sensors.SensorRaycast(model, np.tile(np.array(o, np.float32), (E, 1, 1)), np.tile(np.array(d, np.float32), (E, 1, 1)))
    store = pw.origins
    moved = np.tile(np.array(o, np.float32), (E, 1, 1))
    moved[1, :, 2] = 4.0
    pw.set_rays(moved, pw.directions.copy())
    pw.eval(model.state())
    assert pw.origins is store and np.allclose(pw.distance, [[1.9, 1.94], [2.9, 2.94], [1.9, 1.94]])
    with pytest.raises(ValueError):
        pw.set_rays(np.zeros((2, 3)), np.zeros((2, 3)))


def test_unsupported_targets_are_refused_and_named():
    hull = nt.Mesh.create_box(0.1, 0.1, 0.1)

    def extra(env):
        b = env.add_body(xform=[0.0, 3.0, 1.0, 0.0, 0.0, 0.0, 1.0])
        env.add_shape_convex_hull(b, mesh=hull)
        b = env.add_body(xform=[0.0, 4.0, 1.0, 0.0, 0.0, 0.0, 1.0])
        env.add_shape_cylinder(b, radius=0.1, half_height=0.1, barrel_radius=0.3)

    model = row_scene(extra)
    n = len(ROW)
    with pytest.raises(NotImplementedError, match=rf"slot {n} .*CONVEX_MESH.*slot {n + 1} .*barrel CYLINDER"):
        sensors.SensorRaycast(model, np.zeros((1, 3)), np.ones((1, 3)))
    mask = np.ones(model.env.ns + model.env.ng, bool)
    mask[[n, n + 1]] = False
    s = sensors.SensorRaycast(model, [[0.0, 0.0, 3.0]], [[0.0, 0.0, -1.0]], shape_mask=mask)  # taken out of the mask: fine
    s.eval(model.state())
    assert np.allclose(s.distance, 1.9)
    no_extras = sensors.SensorRaycast(model, [[0.0, 0.0, 3.0]], [[0.0, 0.0, -1.0]], exclude_bodies=(n, n + 1), want_normal=False, want_shape=False)
    no_extras.eval(model.state())
    assert no_extras.normal is None and no_extras.shape is None and np.allclose(no_extras.distance, 1.9)


def test_the_binding_declares_nt_raycast():
    import ctypes as C

    from newton_amd import _lib

    restype, argtypes = _lib.SYMBOLS["nt_raycast"]
    assert restype is C.c_int32 and argtypes[2] == C.POINTER(_lib.nt_raycast_args) and len(argtypes) == 4
    assert nt.sensors is sensors and "sensors" in nt.__all__


# ---------------------------------------------------------------------------------------------------------------------------------
# the comparison scenes: what the kernel tests rely on (raycast_cases.py), asserted on the reference
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_comparison_scene_conditions(name):
    model, rays, kw, ref = case(name)
    assert ref["distance"].shape == (N_WORLDS, N_RAYS)
    c, hit = ref["clear"], ref["distance"] >= 0.0
    print(f"[raycast] {name}: clear {c.mean():.3f}, of them hit {hit[c].mean():.3f}, miss {(~hit)[c].mean():.3f}")
    assert c.mean() >= 0.90
    assert hit[c].mean() >= 0.25 and (~hit)[c].mean() >= 0.10


def test_comparison_scenes_cover_every_type_inside_starts_and_back_faces():
    seen = set()
    for name in CASES:
        model, rays, kw, ref = case(name)
        seen |= hit_types(model, ref)
    assert seen == ALL_TARGET_TYPES
    model, (o, d, body), kw, ref = case("primitives")
    t = model.env
    finite_plane = int(t.gshape_id[1])
    assert np.asarray(model.shape_scale)[finite_plane, 0] > 0.0 and np.any(ref["shape"][ref["clear"]] == finite_plane)
    # rays that start at a body's origin are inside its shape (every shape of the scene contains its origin): clear ones exist, none
    # reports the own shape
    inside = (body >= 0) & np.all(o == 0.0, axis=1)
    own = t.shape_local0 + np.arange(N_WORLDS)[:, None] * t.ns + np.where(body >= 0, body, 0)[None, :]  # (shape k sits on body k)
    assert np.any(ref["clear"][:, inside]) and not np.any((ref["shape"] == own)[:, inside])
    # rays from below the ground plane upwards cross its back face at t = -z / dz: clear ones exist, none stops there
    below = (body < 0) & (o[:, 2] < 0.0) & (d[:, 2] > 0.0)
    assert np.any(ref["clear"][:, below]) and not np.any(ref["shape"][:, below] == t.gshape_id[0])
    for name in ("terrain_skim", "hfield_skim"):  # ... and below the terrain: a culled mesh / heightfield back face
        model, (o, d, body), kw, ref = case(name)
        below = o[:, 2] < -0.05
        crossing = below & (np.abs(o[:, 0] + d[:, 0] * (-o[:, 2] / d[:, 2])) < 1.5) & (np.abs(o[:, 1] + d[:, 1] * (-o[:, 2] / d[:, 2])) < 1.5)
        assert np.any(ref["clear"][:, crossing]) and not np.any(ref["shape"][:, below] == model.env.gshape_id[0])


def test_heterogeneous_models_are_refused():
    class Hetero:
        is_heterogeneous = True

    with pytest.raises(NotImplementedError, match="heterogeneous"):
        sensors.SensorRaycast(Hetero(), np.zeros((1, 3)), np.ones((1, 3)))
