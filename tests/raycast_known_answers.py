"""Rays whose answer can be written down, shared by tests/test_raycast_host.py, test_raycast_emu.py and test_gpu_raycast.py (test
infrastructure; case tables only).  Every backend -- the float64 host path, the emulated kernel, the kernel on the device -- casts
the same table and is compared with the closed form, not with another backend.

The expected values are float64, computed from the FLOAT32-ROUNDED inputs (`f`): 0.1 is 0.1 + 1.5e-9 once it is a shape size, 5.03
is off by 2e-7 once it is a ray origin.  The `dyadic` scene has sizes and positions that are sums of a few powers of two, so that
the shape-frame ray is exact in fp32 and in float64 and the branches that ask for an exact zero or an exact equality (a direction
component of 0, |z| == half height, a ray in a face plane) are taken on every backend.

A case: name, scene, rays (o, d, body), kw(model) -> SensorRaycast keyword arguments, pose(model) -> body_q or None, and per ray
`t` (NaN: the ray misses), `n` (NaN row: the normal is not compared), `nz_min` (NaN or a lower bound of n.z), `shape` (None, ("local",
slot) or ("global", index)); `host_t` / `host_n`: the absolute bounds of the host path (those of the tests these cases came from)."""
import numpy as np

import newton_amd as nt
from scenes import terrain_height, terrain_scene

E = 3
NAN = float("nan")
# body k at (k, 0, 1), identity rotation; (kind, top of the shape above the body origin along +z, extent along +x)
ROW = [("sphere", 0.1, 0.1), ("box", 0.06, 0.1), ("capsule", 0.22, 0.07), ("cylinder", 0.1, 0.08), ("ellipsoid", 0.06, 0.12), ("cone", 0.12, None)]


def f(x):
    return float(np.float32(x))


def row_scene(extra=None, device=None):
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
    return scene.finalize(device=device)


def stacked(env):
    """Two boxes of one size in one place (a tie), and a third 0.5 m above them."""
    for z in (2.0, 2.0, 2.5):
        b = env.add_body(xform=[10.0, 0.0, z, 0.0, 0.0, 0.0, 1.0])
        env.add_shape_box(b, hx=0.2, hy=0.2, hz=0.1)


# the dyadic scene: body k at (k, 0, 1), identity rotation
BOX_H = (0.125, 0.09375, 0.0625)
CYL_R, CYL_HH = 0.125, 0.25
CAP_R, CAP_HH = 0.0625, 0.1875
CONE_R, CONE_HH = 0.375, 0.25  # k = r / (2 h) = 0.75: the generators are 3-4-5 triangles
PLANE_AT, PLANE_HALF = (5.0, 0.0, 0.5), (0.5, 0.25)


def dyadic_scene(device=None):
    env = nt.ModelBuilder()
    b = env.add_body(xform=[0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0])
    env.add_shape_box(b, hx=BOX_H[0], hy=BOX_H[1], hz=BOX_H[2])
    b = env.add_body(xform=[1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0])
    env.add_shape_cylinder(b, radius=CYL_R, half_height=CYL_HH)
    b = env.add_body(xform=[2.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0])
    env.add_shape_capsule(b, radius=CAP_R, half_height=CAP_HH)
    b = env.add_body(xform=[3.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0])
    env.add_shape_cone(b, radius=CONE_R, half_height=CONE_HH)
    scene = nt.ModelBuilder()
    scene.replicate(env, E)
    scene.add_ground_plane()
    scene.add_shape_plane(xform=[*PLANE_AT, 0.0, 0.0, 0.0, 1.0], width=PLANE_HALF[0], length=PLANE_HALF[1])
    return scene.finalize(device=device)


TERRAIN_CELLS, TERRAIN_HALF = 8, 1.0  # nodes at -1 + 0.25 i: exact in fp32, so a ray can stand exactly on an edge or a diagonal

SCENES = {
    "row": row_scene,
    "row_stacked": lambda device=None: row_scene(stacked, device=device),
    "dyadic": dyadic_scene,
    "terrain9_mesh": lambda device=None: terrain_scene(E, cells=9, heightfield=False, device=device),
    "terrain9_hfield": lambda device=None: terrain_scene(E, cells=9, heightfield=True, device=device),
    "terrain8_mesh": lambda device=None: terrain_scene(E, cells=TERRAIN_CELLS, half=TERRAIN_HALF, heightfield=False, device=device),
    "terrain8_hfield": lambda device=None: terrain_scene(E, cells=TERRAIN_CELLS, half=TERRAIN_HALF, heightfield=True, device=device),
}


def no_kw(model):
    return {}


def only_global(index):
    def kw(model):
        mask = np.zeros(model.env.ns + model.env.ng, bool)
        mask[model.env.ns + index] = True
        return {"shape_mask": mask}

    return kw


def without_ground(model):
    mask = np.ones(model.env.ns + model.env.ng, bool)
    mask[model.env.ns] = False
    return {"shape_mask": mask}


def _case(name, scene, rays, kw=no_kw, pose=None, host_t=1e-9, host_n=1e-9):
    """rays: a list of (origin, direction, body, t, normal or None, shape or None[, nz_min])."""
    o = np.array([r[0] for r in rays], np.float32).reshape(-1, 3)
    d = np.array([r[1] for r in rays], np.float32).reshape(-1, 3)
    body = np.array([r[2] for r in rays], np.int32)
    t = np.array([NAN if r[3] is None else r[3] for r in rays], np.float64)
    n = np.array([[NAN] * 3 if r[4] is None else r[4] for r in rays], np.float64).reshape(-1, 3)
    nz_min = np.array([r[6] if len(r) > 6 else NAN for r in rays], np.float64)
    shape = [r[5] for r in rays]
    assert all((s is None) == bool(np.isnan(x)) for s, x in zip(shape, t)), name
    return dict(name=name, scene=scene, rays=(o, d, body), kw=kw, pose=pose, t=t, n=n, nz_min=nz_min, shape=shape, host_t=host_t, host_n=host_n)


def expected_ids(model, case):
    """[world, R] Newton shape ids of a case, -1 for a miss."""
    t = model.env
    out = np.full((t.env_count, len(case["shape"])), -1, np.int64)
    for r, s in enumerate(case["shape"]):
        if s is not None:
            out[:, r] = t.shape_local0 + np.arange(t.env_count) * t.ns + s[1] if s[0] == "local" else int(t.gshape_id[s[1]])
    return out


UP, DOWN = [0.0, 0.0, 1.0], [0.0, 0.0, -1.0]
MISS = (None, None, None)


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases that were the host tests of tests/test_raycast_host.py (the row scene, the 9-cell terrain)
# ---------------------------------------------------------------------------------------------------------------------------------
def _row_cases():
    out = []
    # down the axis of every primitive but the cone (the apex itself is a degenerate point: see the offset ray below)
    rays = [([k, 0.0, 3.0], DOWN, -1, 3.0 - (1.0 + f(top)), UP, ("local", k)) for k, (kind, top, _) in enumerate(ROW) if kind != "cone"]
    rays[2] = ([2.0, 0.0, 3.0], DOWN, -1, 3.0 - (1.0 + f(0.15) + f(0.07)), UP, ("local", 2))  # (the capsule's top: two float32 sizes)
    out.append(_case("row_down_the_axis", "row", rays, host_t=2e-8, host_n=1e-12))
    # from the side, along -x at the body's height: the +x extreme
    rays = [([k + 0.45, 0.0, 1.0], [-1.0, 0.0, 0.0], -1, f(k + 0.45) - k - f(side), [1.0, 0.0, 0.0], ("local", k))
            for k, (kind, _, side) in enumerate(ROW) if side is not None]
    # cone (body 5, apex up, k = r / (2 h) = 0.375): down at 0.03 m from the axis, the lateral surface at w = rho / k below the apex
    r, hh = f(0.09), f(0.12)
    kk, rho = r / (2.0 * hh), f(5.03) - 5.0
    rays.append(([5.03, 0.0, 3.0], DOWN, -1, 3.0 - (1.0 + hh - rho / kk), np.array([1.0, 0.0, kk]) / np.hypot(1.0, kk), ("local", 5)))
    rays.append(([5.02, 0.01, 0.5], [0.0, 0.0, 2.0], -1, 1.0 - hh - 0.5, DOWN, ("local", 5)))  # the cone from below: the base disc
    # cylinder (body 3) from above off the axis: the cap; capsule (body 2) along -y at z = 1.15 + 0.05: the upper hemisphere
    rays.append(([3.05, 0.02, 2.0], DOWN, -1, 2.0 - (1.0 + f(0.1)), UP, ("local", 3)))
    hz, rc = f(1.2) - 1.0 - f(0.15), f(0.07)
    rays.append(([2.0, 0.5, 1.2], [0.0, -1.0, 0.0], -1, 0.5 - np.sqrt(rc ** 2 - hz ** 2), [0.0, np.sqrt(rc ** 2 - hz ** 2) / rc, hz / rc], ("local", 2)))
    out.append(_case("row_from_the_side_and_the_cone", "row", rays, host_t=1e-6, host_n=1e-6))

    # the box turned a quarter about x shows its hy = 0.08 upwards; a ray attached to the body sees the shape as at identity
    def quarter_turn(model):
        bq = np.array(model.body_q, np.float32)
        bq[1::model.env.nb, 3:] = nt._np_math.quat_rpy(np.pi / 2, 0.0, 0.0)
        return bq

    rays = [([1.0, 0.0, 3.0], DOWN, -1, 3.0 - (1.0 + f(0.08)), None, ("local", 1)),
            ([0.0, 0.0, 0.5], DOWN, 1, 0.5 - f(0.06), [0.0, -1.0, 0.0], ("local", 1)),  # body +z is world -y after the turn
            ([0.0, 0.0, 0.0], [0.0, 0.0, 0.0], 1, *MISS)]  # zero direction: a miss
    out.append(_case("row_rotated_pose_and_body_attached_rays", "row", rays, pose=quarter_turn, host_t=1e-6, host_n=1e-6))
    return out


def _node_heights(model, heightfield, nodes, xs):
    if heightfield:  # the node height as the HeightfieldData record stores it: min_z + h (max_z - min_z), float32 h
        off, nrow, ncol, hx, hy, zlo, zhi = model.heightfield_data[0]
        e = np.asarray(model.heightfield_elevations, np.float64).reshape(nrow, ncol)
        return [f(zlo) + e[j, i] * (f(zhi) - f(zlo)) for i, j in nodes]
    return [f(terrain_height(xs[i], xs[j])) for i, j in nodes]


def _terrain9_cases(heightfield):
    """A vertical ray over a node, where four cells and eight triangles meet (the normal is one of theirs: only n.z is bounded)."""
    scene = "terrain9_hfield" if heightfield else "terrain9_mesh"
    model = SCENES[scene]()
    xs = np.linspace(-1.6, 1.6, 10)
    nodes = [(2, 3), (5, 5), (7, 1)]
    z = _node_heights(model, heightfield, nodes, xs)
    o = [[f(xs[i]), f(xs[j]), 0.5] for i, j in nodes]
    down = [(p, DOWN, -1, 0.5 - zz, None, ("global", 0), 0.99) for p, zz in zip(o, z)]
    # from below: the back faces are culled, a heightfield is hit on its top only
    up = [([p[0], p[1], -0.5], UP, -1, *MISS) for p in o]
    tol = 1e-7 if heightfield else 1e-12
    return [_case(f"{scene}_vertical_over_a_node", scene, down, kw=only_global(0), host_t=tol),
            _case(f"{scene}_from_below", scene, up, kw=only_global(0))]


def _stacked_cases():
    n = len(ROW)
    g = ("global", 0)
    rays = [([10.0, 0.0, 4.0], DOWN, -1, 4.0 - (2.5 + f(0.1)), UP, ("local", n + 2)),  # the upper box is nearer from above
            ([10.0, 0.0, 0.5], UP, -1, 2.0 - f(0.1) - 0.5, DOWN, ("local", n)),  # a tie from below: the lower shape id
            # from inside the two lower boxes: neither is hit (their far faces look away), the ground is
            ([10.05, 0.0, 2.0], DOWN, -1, 2.0, UP, g),
            ([0.0, 0.0, 1.0], [0.3, 0.2, 0.5], -1, *MISS),  # from the centre of the sphere upwards: its own surface does not face the ray
            ([20.0, 0.0, -1.0], UP, -1, *MISS)]  # the ground plane from below
    t = 4.0 - (2.5 + f(0.1))
    return [_case("stacked_tie_and_facing", "row_stacked", rays, host_t=1e-8),
            _case("stacked_max_distance_below", "row_stacked", [([10.0, 0.0, 4.0], DOWN, -1, *MISS)] * 2, kw=lambda m: {"max_distance": 1.4 - 1e-6}),
            # (t counts metres along the unit direction)
            _case("stacked_max_distance_above", "row_stacked", [([10.0, 0.0, 4.0], [0.0, 0.0, -2.0], -1, t, UP, ("local", n + 2))],
                  kw=lambda m: {"max_distance": 1.4 + 1e-6}, host_t=1e-8)]


# ---------------------------------------------------------------------------------------------------------------------------------
# the branches no random ray reaches (the dyadic scene, the ground plane taken out of the mask: a miss is a miss)
# ---------------------------------------------------------------------------------------------------------------------------------
def _dyadic_cases():
    hx, hy, hz = BOX_H
    box, cyl, cap, cone, plane = ("local", 0), ("local", 1), ("local", 2), ("local", 3), ("global", 1)
    X = [1.0, 0.0, 0.0]
    out = []
    rays = [([0.03125, 0.015625, 3.0], DOWN, -1, 2.0 - hz, UP, box),  # two zero direction components, straight at a face
            ([0.25, 0.0, 3.0], DOWN, -1, *MISS),  # the same ray beside the face: refused by the arm of a zero component
            ([0.5, 0.03125, 1.0 + hz], [-1.0, 0.0, 0.0], -1, *MISS),  # in the plane of the top face: it touches, it does not enter
            ([0.5, 0.03125, 1.0 + hz - 0.015625], [-1.0, 0.0, 0.0], -1, 0.5 - hx, X, box)]  # ... and just under that plane
    out.append(_case("dyadic_box", "dyadic", rays, kw=without_ground))
    rays = [([1.0625, 0.03125, 3.0], DOWN, -1, 2.0 - CYL_HH, UP, cyl),  # parallel to the axis, inside the radius: the caps
            ([1.0625, 0.03125, 0.25], UP, -1, 0.75 - CYL_HH, DOWN, cyl),
            ([1.25, 0.0, 3.0], DOWN, -1, *MISS),  # parallel and outside
            ([1.5, 0.0, 1.0 + CYL_HH], [-1.0, 0.0, 0.0], -1, 0.5 - CYL_R, X, cyl),  # perpendicular at z = +-hh exactly: the side
            ([1.5, 0.0, 1.0 - CYL_HH], [-1.0, 0.0, 0.0], -1, 0.5 - CYL_R, X, cyl)]
    out.append(_case("dyadic_cylinder", "dyadic", rays, kw=without_ground))
    s = np.sqrt(CAP_R ** 2 - 0.03125 ** 2)
    rays = [([2.0, 0.0, 3.0], DOWN, -1, 2.0 - CAP_HH - CAP_R, UP, cap),  # on the axis: the pole of the hemisphere that faces the ray
            ([2.0, 0.0, 0.25], UP, -1, 0.75 - CAP_HH - CAP_R, DOWN, cap),
            ([2.03125, 0.0, 3.0], DOWN, -1, 2.0 - CAP_HH - s, [0.03125 / CAP_R, 0.0, s / CAP_R], cap),  # parallel, off the axis
            ([2.03125, 0.0, 0.25], UP, -1, 0.75 - CAP_HH - s, [0.03125 / CAP_R, 0.0, -s / CAP_R], cap),
            ([2.5, 0.0, 1.0 + CAP_HH], [-1.0, 0.0, 0.0], -1, 0.5 - CAP_R, X, cap),  # perpendicular at z = +-hh: still the barrel
            ([2.5, 0.0, 1.0 - CAP_HH], [-1.0, 0.0, 0.0], -1, 0.5 - CAP_R, X, cap)]
    out.append(_case("dyadic_capsule", "dyadic", rays, kw=without_ground))
    # cone: a ray parallel to the generator on the +x side (A = 0: one root) from the apex's height enters through the -x side at
    # w = 0.4 below the apex, x = -k w = -0.3, after t = 0.5; n = (x, 0, k^2 w) = (-0.3, 0, 0.225) -> (-0.8, 0, 0.6)
    # (f(2.4) is 2.4 + 9.5e-8: the entry slides along the generator, t changes by that / 1.2, the normal does not)
    rays = [([2.4, 0.0, 1.0 + CONE_HH], [3.0, 0.0, -4.0], -1, 0.5 - (f(2.4) - 2.4) / 1.2, [-0.8, 0.0, 0.6], cone),
            ([3.125, 0.0625, 0.25], UP, -1, 0.75 - CONE_HH, DOWN, cone),  # through the base from below, off the axis
            ([3.03125, 0.0, 0.875], UP, -1, *MISS)]  # from inside upwards
    out.append(_case("dyadic_cone", "dyadic", rays, kw=without_ground))
    px, py, pz = PLANE_AT
    rays = [([px + 0.25, py + 0.125, pz + 1.0], DOWN, -1, 1.0, UP, plane),  # inside the extent
            ([px + 0.501, py, pz + 1.0], DOWN, -1, *MISS),  # 1 mm outside
            ([px + 0.25, py + 0.125, pz - 0.25], UP, -1, *MISS)]  # from behind
    out.append(_case("dyadic_finite_plane", "dyadic", rays, kw=without_ground))
    # max_distance one float32 step below and above the hit (t = 1.9375 is exact on every backend): a miss, then a hit
    t = 2.0 - hz
    face = ([0.03125, 0.015625, 3.0], DOWN, -1)
    out.append(_case("dyadic_max_distance_one_step_below", "dyadic", [(*face, *MISS)],
                     kw=lambda m: {**without_ground(m), "max_distance": float(np.nextafter(np.float32(t), np.float32(0.0)))}))
    out.append(_case("dyadic_max_distance_one_step_above", "dyadic", [(*face, t, UP, box)],
                     kw=lambda m: {**without_ground(m), "max_distance": float(np.nextafter(np.float32(t), np.float32(4.0)))}))
    out.append(_case("dyadic_max_distance_at_the_hit", "dyadic", [(*face, t, UP, box)], kw=lambda m: {**without_ground(m), "max_distance": t}))
    # directions: zero, tiny and huge (normalised, then cast); a ray attached to the last body (the cone's, at (3, 0, 1))
    rays = [([0.03125, 0.015625, 3.0], [0.0, 0.0, 0.0], -1, *MISS),
            ([0.03125, 0.015625, 3.0], [0.0, 0.0, -1e-20], -1, t, UP, box),
            ([0.03125, 0.015625, 3.0], [0.0, 0.0, -1e18], -1, t, UP, box),
            ([-1.0, 0.0, 2.0], DOWN, 3, 2.0 - CAP_HH - CAP_R, UP, cap)]
    out.append(_case("dyadic_direction_and_frame", "dyadic", rays, kw=without_ground))
    return out


def _terrain8_cases(heightfield):
    """Vertical rays over the midpoint of a cell edge and of a cell diagonal: the height is the mean of the two float32 node heights,
    the triangle the lower index of the two that share the line.  Horizontal rays: one below the field, one at a node's height."""
    scene = "terrain8_hfield" if heightfield else "terrain8_mesh"
    model = SCENES[scene]()
    xs = -1.0 + 0.25 * np.arange(TERRAIN_CELLS + 1)
    nodes = [(i, j) for j in range(TERRAIN_CELLS + 1) for i in range(TERRAIN_CELLS + 1)]
    z = np.array(_node_heights(model, heightfield, nodes, xs)).reshape(TERRAIN_CELLS + 1, TERRAIN_CELLS + 1)  # [row j, col i]
    P = lambda i, j: np.array([xs[i], xs[j], z[j, i]])  # noqa: E731
    unit = lambda v: v / np.linalg.norm(v)  # noqa: E731
    g = ("global", 0)
    # the edge between nodes (4, 3) and (5, 3): shared by triangle 1 of cell (row 2, col 4), index 41, and triangle 0 of cell (row 3,
    # col 4), index 56.  Triangle 1 of a cell is (p00, p11, p01)
    n_edge = unit(np.cross(P(5, 3) - P(4, 2), P(4, 3) - P(4, 2)))
    # the diagonal of cell (row 5, col 2): triangle 0 = (p00, p10, p11), index 84, before triangle 1, index 85
    n_diag = unit(np.cross(P(3, 5) - P(2, 5), P(3, 6) - P(2, 5)))
    rays = [([0.125, -0.25, 0.5], DOWN, -1, 0.5 - 0.5 * (z[3, 4] + z[3, 5]), n_edge, g),
            ([-0.375, 0.375, 0.5], DOWN, -1, 0.5 - 0.5 * (z[5, 2] + z[6, 3]), n_diag, g),
            ([-2.0, -0.25, -0.0625], [1.0, 0.0, 0.0], -1, *MISS)]  # along a grid row, below the lowest node
    # at the height of node (6, 3), the highest of its row, from x = 1 along -x in the row's own line (d.y = 0, on the edges between
    # two rows of cells): the surface rises from node (7, 3) to the node and is met there.  Mesh: the float32 height of the vertex
    # itself.  Heightfield: every backend rounds min_z + h (max_z - min_z) its own way, so the ray runs 2^-20 m lower and meets the
    # edge that far below the node (the normal is that of either row: not compared)
    assert z[3, 6] == z[3].max() and z[3, 7] < z[3, 6] and z[3, 8] < z[3, 7]
    z_ray = f(z[3, 6] - 2.0 ** -20) if heightfield else z[3, 6]
    x_hit = 0.75 - 0.25 * (z_ray - z[3, 7]) / (z[3, 6] - z[3, 7])
    rays.append(([1.0, -0.25, z_ray], [-1.0, 0.0, 0.0], -1, 1.0 - x_hit, None, g))
    return [_case(f"{scene}_edges_and_rows", scene, rays, kw=only_global(0), host_t=1e-7 if heightfield else 1e-9)]


def _build():
    cases = _row_cases() + _stacked_cases() + _dyadic_cases()
    for hf in (False, True):
        cases += _terrain9_cases(hf) + _terrain8_cases(hf)
    return {c["name"]: c for c in cases}


CASES = _build()


def compare_known(case, model, distance, normal, shape, t_abs=None, t_rel=None, n_abs=None, n_angle=None, label=""):
    """Hit / miss and shape id exact; the distance within t_abs (absolute) or t_rel (relative to max(1, t)) of the closed form; the
    normal within n_abs (per component) or n_angle (rad) where the case names one.  Returns (max |dt| / max(1, t), max angle)."""
    distance, normal, shape = np.asarray(distance, np.float64), np.asarray(normal, np.float64), np.asarray(shape)
    t, n, ids = case["t"], case["n"], expected_ids(model, case)
    miss = np.isnan(t)
    assert distance.shape == ids.shape, label
    assert np.array_equal(distance < 0.0, np.broadcast_to(miss, distance.shape)), f"{label}: hit / miss {distance} against {t}"
    assert np.array_equal(shape, ids), f"{label}: shape ids {shape} against {ids}"
    assert np.all(distance[:, miss] == -1.0) and np.all(normal[:, miss] == 0.0), label
    hit = ~miss
    err = np.abs(distance[:, hit] - t[hit])
    print(f"[raycast known] {label}: |dt| = {err.max(axis=0) if hit.any() else []}")
    if t_abs is not None:
        assert np.all(err <= t_abs), f"{label}: distance {distance[:, hit]} against {t[hit]} (bound {t_abs:g})"
    err_rel = float((err / np.maximum(1.0, t[hit])).max()) if hit.any() else 0.0
    if t_rel is not None:
        assert err_rel <= t_rel, f"{label}: |dt| / max(1, t) = {err_rel:.3e} (gate {t_rel:.3e})"
    k = hit & ~np.isnan(n[:, 0])
    ang = 0.0
    if k.any():
        got, want = normal[:, k], np.broadcast_to(n[k], normal[:, k].shape)
        if n_abs is not None:
            assert np.all(np.abs(got - want) <= n_abs), f"{label}: normals {got} against {n[k]} (bound {n_abs:g})"
        ang = float(np.arctan2(np.linalg.norm(np.cross(got, want), axis=-1), np.sum(got * want, axis=-1)).max())
        print(f"[raycast known] {label}: max normal angle = {ang:.3e} rad")
        if n_angle is not None:
            assert ang <= n_angle, f"{label}: normal angle {ang:.3e} rad (gate {n_angle:.3e})"
    z = hit & ~np.isnan(case["nz_min"])
    assert np.all(normal[:, z, 2] > case["nz_min"][z]), label
    assert np.all(np.abs(np.linalg.norm(normal[:, hit], axis=-1) - 1.0) < 1e-5), label
    return err_rel, ang
