"""The float64 host path of newton_amd.sensors.SensorRaycast -- the reference of the kernel tests -- against closed-form answers (the
table of tests/raycast_known_answers.py, which the kernel tests cast too), against an independent reference sampled from the signed
distance functions, and the conditions the comparison scenes of tests/raycast_cases.py have to meet (asserted, not measured)."""
import numpy as np
import pytest

import newton_amd as nt
import raycast_known_answers as known
import tolerances
from scenes import terrain_height
from newton_amd import sensors
from newton_amd.enums import GeoType
from raycast_cases import ALL_TARGET_TYPES, CASES, LAYOUT_CASES, LAYOUT_WORLDS, N_RAYS, N_WORLDS, case, hit_types

E = known.E
ROW, row_scene = known.ROW, known.row_scene


def cast(model, o, d, body=-1, state=None, **kw):
    s = sensors.SensorRaycast(model, np.asarray(o, np.float32), np.asarray(d, np.float32), ray_body=body, **kw)
    st = model.state() if state is None else state
    s.eval(st)
    return s


_MODELS = {}


def known_model(scene):
    if scene not in _MODELS:
        _MODELS[scene] = known.SCENES[scene]()
    return _MODELS[scene]


def _known_on_the_host(name):
    c = known.CASES[name]
    model = known_model(c["scene"])
    o, d, body = c["rays"]
    state = model.state()
    if c["pose"] is not None:
        state.body_q = c["pose"](model)
    s = cast(model, o, d, body=body, state=state, **c["kw"](model))
    assert s.distance.dtype == np.float64 and s.shape.dtype == np.int32
    err_t, err_n = known.compare_known(c, model, s.distance, s.normal, s.shape, t_abs=c["host_t"], n_abs=c["host_n"], label=f"host {name}")
    tolerances.record(f"raycast_known_host_{name}", {"distance_rel": {"max": err_t}, "normal_angle": {"max": err_n}},
                      {"distance_abs": c["host_t"], "normal_abs": c["host_n"]})


@pytest.mark.parametrize("name", list(known.CASES))
def test_known_answers(name):
    """The closed forms of tests/raycast_known_answers.py on the float64 host path, within the absolute bounds the table carries (those
    of the host tests the first cases came from; 1e-9 for the others: float64 on the same float32-rounded inputs)."""
    _known_on_the_host(name)


# the closed-form tests this file had before the table: their rays, answers and bounds are the table's first cases now
def test_rays_down_the_axis_of_every_primitive():
    _known_on_the_host("row_down_the_axis")


def test_rays_from_the_side_and_the_cone():
    _known_on_the_host("row_from_the_side_and_the_cone")


def test_rotated_pose_and_body_attached_rays():
    _known_on_the_host("row_rotated_pose_and_body_attached_rays")


@pytest.mark.parametrize("heightfield", [False, True])
def test_vertical_ray_over_a_terrain_node(heightfield):
    scene = "terrain9_hfield" if heightfield else "terrain9_mesh"
    if heightfield:  # the record's node heights are the terrain's, to float32
        model = known_model(scene)
        xs = np.linspace(-1.6, 1.6, 10)
        nodes = [(2, 3), (5, 5), (7, 1)]
        assert np.allclose(known._node_heights(model, True, nodes, xs), [terrain_height(xs[i], xs[j]) for i, j in nodes], atol=1e-7)
    _known_on_the_host(f"{scene}_vertical_over_a_node")
    _known_on_the_host(f"{scene}_from_below")


def test_nearest_shape_tie_rule_max_distance_and_facing():
    for name in ("stacked_tie_and_facing", "stacked_max_distance_below", "stacked_max_distance_above"):
        _known_on_the_host(name)


# ---------------------------------------------------------------------------------------------------------------------------------
# an independent float64 reference for the primitives: the sign of newton_amd.sdf.primitive_sdf sampled along the ray, the first
# outside-to-inside change bisected, the normal from central differences.  It shares no formula with sensors._primitive
# ---------------------------------------------------------------------------------------------------------------------------------
SDF_STEP, SDF_BRACKET, SDF_H = 1.5e-3, 1e-12, 1e-6


def sdf_reference(model, body_q, rays, slots, max_distance):
    """(distance [E, R], normal [E, R, 3], shape [E, R], hit point in the shape frame [E, R, 3], slot [E, R]) in float64.  A shape is
    sampled only where the ray is within its bounding radius of its centre (|t - t_c| <= radius: the projection of the bounding
    ball on the ray; outside it the distance is positive), every SDF_STEP or finer; an origin inside a shape does not hit it."""
    from newton_amd.articulation import _qinv, _qmul, _qrot
    from newton_amd.sdf import primitive_extents, primitive_sdf

    t = model.env
    E, nb, ns = t.env_count, t.nb, t.ns
    o, d, rb = (np.asarray(a) for a in rays)
    R = len(rb)
    bq = np.asarray(body_q, np.float64).reshape(E, nb, 7)
    X = bq[:, np.where(rb >= 0, rb, 0), :]
    att = (rb >= 0)[None, :, None]
    O = np.where(att, X[..., :3] + _qrot(X[..., 3:], np.broadcast_to(o.astype(np.float64), (E, R, 3))), o.astype(np.float64)).reshape(-1, 3)
    D = np.where(att, _qrot(X[..., 3:], np.broadcast_to(d.astype(np.float64), (E, R, 3))), d.astype(np.float64)).reshape(-1, 3)
    D = D / np.linalg.norm(D, axis=1, keepdims=True)
    N = E * R
    best_t, best_id, best_n = np.full(N, np.inf), np.full(N, -1, np.int64), np.zeros((N, 3))
    best_p, best_slot = np.zeros((N, 3)), np.full(N, -1, np.int64)
    xf = np.asarray(model.shape_transform, np.float64).reshape(-1, 7)
    sc = np.asarray(model.shape_scale, np.float64).reshape(-1, 3)
    for slot in (int(s) for s in slots):
        ids = t.shape_local0 + np.arange(E) * ns + slot if slot < ns else np.full(E, int(t.gshape_id[slot - ns]))
        gtype, body = int(t.shape_type[slot]), int(t.shape_body[slot])
        Xs = xf[ids]
        if body >= 0:
            Xb = bq[:, body]
            Xs = np.concatenate([Xb[:, :3] + _qrot(Xb[:, 3:], Xs[:, :3]), _qmul(Xb[:, 3:], Xs[:, 3:])], axis=1)
        Xs, rid = np.repeat(Xs, R, axis=0), np.repeat(ids, R)
        qi = _qinv(Xs[:, 3:])
        ol, dl = _qrot(qi, O - Xs[:, :3]), _qrot(qi, D)
        scale = sc[ids[0]]
        assert np.all(sc[ids] == scale)
        hit, tt, n, p = np.zeros(N, bool), np.full(N, np.inf), np.zeros((N, 3)), np.zeros((N, 3))
        if gtype == GeoType.PLANE:  # the direct formula
            with np.errstate(divide="ignore", invalid="ignore"):
                tp = -ol[:, 2] / dl[:, 2]
                p = ol + dl * tp[:, None]
            inside = np.ones(N, bool) if scale[0] == 0.0 and scale[1] == 0.0 else (np.abs(p[:, 0]) <= scale[0]) & (np.abs(p[:, 1]) <= scale[1])
            hit = (dl[:, 2] < 0.0) & (tp >= 0.0) & inside
            tt, n = np.where(hit, tp, np.inf), np.tile([0.0, 0.0, 1.0], (N, 1))
        else:
            sdf = lambda x: primitive_sdf(gtype, scale, x)  # noqa: E731
            radius = float(np.linalg.norm(primitive_extents(gtype, scale)[1])) + 0.01
            tc = -np.sum(ol * dl, axis=1)
            lo, hi = np.maximum(tc - radius, 0.0), np.minimum(tc + radius, max_distance)
            cand = np.flatnonzero((hi > lo) & (sdf(ol) >= 0.0))
            if len(cand):
                steps = int(np.ceil(2.0 * radius / SDF_STEP)) + 1
                ts = lo[cand, None] + (hi[cand] - lo[cand])[:, None] * np.linspace(0.0, 1.0, steps)[None, :]
                assert np.all(np.diff(ts, axis=1) <= SDF_STEP)
                neg = sdf((ol[cand, None, :] + dl[cand, None, :] * ts[..., None]).reshape(-1, 3)).reshape(len(cand), steps) < 0.0
                first = np.argmax(neg, axis=1)
                ok = neg.any(axis=1) & (first > 0)  # (first == 0: the interval starts inside, which only an inside origin does)
                assert not np.any(neg[:, 0])
                rows = np.flatnonzero(ok)
                a, b = ts[rows, first[rows] - 1], ts[rows, first[rows]]
                c = cand[rows]
                while len(c) and np.max(b - a) > SDF_BRACKET:
                    m = 0.5 * (a + b)
                    inside = sdf(ol[c] + dl[c] * m[:, None]) < 0.0
                    a, b = np.where(inside, a, m), np.where(inside, m, b)
                th = 0.5 * (a + b)
                hit[c], tt[c], p[c] = True, th, ol[c] + dl[c] * th[:, None]
                g = np.stack([(sdf(p[c] + SDF_H * e) - sdf(p[c] - SDF_H * e)) / (2.0 * SDF_H) for e in np.eye(3)], axis=1)
                n[c] = g / np.linalg.norm(g, axis=1, keepdims=True)
        take = hit & (tt <= max_distance) & ((tt < best_t) | ((tt == best_t) & (rid < best_id)))
        best_t, best_id = np.where(take, tt, best_t), np.where(take, rid, best_id)
        best_n, best_p = np.where(take[:, None], _qrot(Xs[:, 3:], n), best_n), np.where(take[:, None], p, best_p)
        best_slot = np.where(take, slot, best_slot)
    h = best_t < np.inf
    return (np.where(h, best_t, -1.0).reshape(E, R), best_n.reshape(E, R, 3), best_id.reshape(E, R), best_p.reshape(E, R, 3), best_slot.reshape(E, R))


def test_host_primitives_against_the_sampled_sdf_reference():
    """sensors.raycast_numpy on the primitives scene, its ray set and a second seeded one, against sdf_reference on the rays the
    comparison rule calls clear: hit / miss and shape id equal, the distance within 1e-9 m (the bisection stops at 1e-12 m; a clear ray
    is 1e-4 m from a silhouette, which bounds the conditioning of the root by sqrt(r / 2e-4), about 22), the normal within 1e-6 rad
    (central differences with h = 1e-6 m: truncation h^2 / r^2 and rounding eps / h, both about 1e-10).  A 1.5 mm step misses only
    chords shorter than itself, which graze at most 3e-6 m deep: not clear rays.  Coverage is asserted from the references alone."""
    from raycast_cases import MAX_DISTANCE, primitive_rays, reference

    model, rays0, kw, ref0 = case("primitives")
    rays1 = primitive_rays(seed=12)
    t = model.env
    counts, parts = {}, set()
    worst_t = worst_n = 0.0
    for label, rays, ref in (("set 0", rays0, ref0), ("set 1", rays1, reference(model, model.body_q, rays1, **kw))):
        dist, normal, shape, p, slot = sdf_reference(model, model.body_q, rays, ref["slots"], MAX_DISTANCE)
        c, k = ref["clear"], ref["normal_ok"]
        assert c.mean() >= 0.9
        assert np.array_equal((dist >= 0.0)[c], (ref["distance"] >= 0.0)[c]), f"{label}: hit / miss (the sampled reference must miss no hit of a clear ray)"
        assert np.array_equal(shape[c], ref["shape"][c]), f"{label}: shape ids"
        hit = c & (ref["distance"] >= 0.0)
        err_t = np.abs(dist - ref["distance"])[hit].max()
        ang = np.arctan2(np.linalg.norm(np.cross(normal[k], ref["normal"][k]), axis=-1), np.sum(normal[k] * ref["normal"][k], axis=-1)).max()
        print(f"[raycast] sdf reference, {label}: clear {c.mean():.3f}, hits {hit.sum()}, max |dt| = {err_t:.3e} m, max normal angle = {ang:.3e} rad ({k.sum()})")
        worst_t, worst_n = max(worst_t, err_t), max(worst_n, ang)
        assert err_t <= 1e-9 and ang <= 1e-6
        # coverage, from the sampled reference's own hit points
        for s in np.unique(slot[hit]):
            gtype = GeoType(int(t.shape_type[s]))
            sel = hit & (slot == s)
            counts[gtype] = counts.get(gtype, 0) + int(sel.sum())
            z, sc = p[sel][:, 2], np.asarray(model.shape_scale, np.float64)[t.shape_local0 + s if s < t.ns else int(t.gshape_id[s - t.ns])]
            if gtype == GeoType.CONE:
                parts |= {("cone", "base")} if np.any(np.abs(z + sc[1]) < 1e-9) else set()
                parts |= {("cone", "lateral")} if np.any(z > -sc[1] + 1e-6) else set()
            elif gtype == GeoType.CAPSULE:
                parts |= {("capsule", "barrel")} if np.any(np.abs(z) < sc[1] - 1e-6) else set()
                parts |= {("capsule", "hemisphere")} if np.any(np.abs(z) > sc[1] + 1e-6) else set()
            elif gtype == GeoType.CYLINDER:
                parts |= {("cylinder", "cap")} if np.any(np.abs(np.abs(z) - sc[1]) < 1e-9) else set()
                parts |= {("cylinder", "side")} if np.any(np.abs(z) < sc[1] - 1e-6) else set()
    tolerances.record("raycast_host_vs_sdf_reference", {"distance_abs": {"max": float(worst_t)}, "normal_angle": {"max": float(worst_n)}},
                      {"distance_abs": 1e-9, "normal_angle": 1e-6})
    print(f"[raycast] sdf reference: clear hits per type {({g.name: n for g, n in counts.items()})}, parts {sorted(parts)}")
    for g in (GeoType.PLANE, GeoType.SPHERE, GeoType.CAPSULE, GeoType.ELLIPSOID, GeoType.CYLINDER, GeoType.BOX, GeoType.CONE):
        assert counts.get(g, 0) >= 5, g.name
    assert parts == {("cone", "base"), ("cone", "lateral"), ("capsule", "barrel"), ("capsule", "hemisphere"), ("cylinder", "cap"), ("cylinder", "side")}


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
@pytest.mark.parametrize("name", [n for n in CASES if n not in LAYOUT_CASES])
def test_comparison_scene_conditions(name):
    model, rays, kw, ref = case(name)
    assert ref["distance"].shape == (N_WORLDS, N_RAYS)
    c, hit = ref["clear"], ref["distance"] >= 0.0
    print(f"[raycast] {name}: clear {c.mean():.3f}, of them hit {hit[c].mean():.3f}, miss {(~hit)[c].mean():.3f}")
    assert c.mean() >= 0.90
    assert hit[c].mean() >= 0.25 and (~hit)[c].mean() >= 0.10


@pytest.mark.parametrize("name", LAYOUT_CASES)
def test_layout_scene_conditions(name):
    """The scenes whose tables differ from the others' (a field that is not square, a second heightfield, a second mesh): 5 worlds, at
    most 70 rays, a clear share of 0.8, ten clear hits on every mesh / heightfield of the scene, a clear miss."""
    model, rays, kw, ref = case(name)
    t = model.env
    assert t.env_count == LAYOUT_WORLDS and ref["distance"].shape[0] == LAYOUT_WORLDS and ref["distance"].shape[1] <= N_RAYS
    c, hit = ref["clear"], ref["distance"] >= 0.0
    print(f"[raycast] {name}: clear {c.mean():.3f}, of them hit {hit[c].mean():.3f}, miss {(~hit)[c].mean():.3f}")
    assert c.mean() >= 0.8 and np.any(c & ~hit)
    types = np.asarray(model.shape_type)
    slots = [s for s in ref["slots"] if int(t.shape_type[s]) in (int(GeoType.MESH), int(GeoType.HFIELD))]
    assert len(slots) == (1 if name == "hfield_rect" else 2)
    for s in slots:  # (a slot is one shape per world, or one global shape)
        ids = t.shape_local0 + np.arange(t.env_count) * t.ns + s if s < t.ns else np.array([int(t.gshape_id[s - t.ns])])
        n = int(np.sum(c & hit & np.isin(ref["shape"], ids)))
        print(f"[raycast] {name}: slot {int(s)} ({GeoType(int(types[ids[0]])).name}): {n} clear hits")
        assert n >= 10
    if name == "hfield_rect":
        (off, nrow, ncol, hx, hy, zlo, zhi), = model.heightfield_data
        assert (nrow, ncol) == (7, 12) and 2 * hx / (ncol - 1) != 2 * hy / (nrow - 1) and off == 0
    elif name == "hfield_two":
        a, b = model.heightfield_data
        assert (a[1], a[2]) != (b[1], b[2]) and b[0] == a[1] * a[2] > 0  # the second record starts behind the first one's nodes
    else:  # the carried mesh: non-zero vertex and triangle starts, three blocks, a scale that differs by axis
        s = int(slots[0])
        assert s < t.ns
        i = t.shape_local0 + s
        vr, tr = np.asarray(model.mesh_vertex_range)[i], np.asarray(model.mesh_triangle_range)[i]
        assert vr[0] > 0 and tr[0] > 0 and 128 < tr[1] <= 192 and len(set(np.asarray(model.shape_scale)[i].tolist())) == 3


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
