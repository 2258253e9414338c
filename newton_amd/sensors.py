"""Sensors.  ``SensorContact`` (further down): the net contact force per world on chosen bodies / shapes, split by counterpart.
``SensorFrameTransform`` / ``SensorIMU`` (at the end): pose, velocity, projected gravity and specific force of sensor-owned frames.
Ray-cast sensors: ``SensorRaycast`` casts R rays per world against the shapes of that world -- a height scan under a robot's base,
a lidar sweep over the other bodies.  The capability of the reference's ``newton.sensors.SensorRaycast``; that one is a single
camera, this one is ONE SENSOR PER WORLD of the replicated model, because that is what the batched layout serves: the same R rays
(or R rays of its own) in every world, attached to a body of that world or fixed in the world frame.  ``SensorTiledCamera`` (after
it) is the image-shaped launch over the same per-ray code: C cameras of W x H pixels per world, one wave per 8 x 8 pixels
(nt_camera_render), every pixel bit for bit the ray cast of its ray.

On a GPU model ``SensorRaycast.eval`` is one launch of raycast_kernel (nt_raycast, include/newton_hip_mesh.h -- the contract is written
there): no allocation, no synchronisation, recordable by ``newton_amd.graph.capture``; the rays are read through resident pointers,
so ``set_rays`` followed by a replay takes effect.  On a host model the same contract runs in numpy, float64 inside, vectorised over
worlds and rays, every triangle of a mesh / heightfield tested (no block skip, no grid walk); that path is the reference the kernel is
tested against."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .articulation import _host_array, _qinv, _qmul, _qrot
from .enums import GeoType

RAY_TARGET_TYPES = (GeoType.PLANE, GeoType.HFIELD, GeoType.SPHERE, GeoType.CAPSULE, GeoType.ELLIPSOID, GeoType.CYLINDER, GeoType.BOX, GeoType.MESH,
                    GeoType.CONE)
_PAIR_CHUNK = 1 << 19  # (ray, triangle) pairs per batch of the host path's triangle tests (bounds its memory)


def _dot(a, b):
    return np.sum(a * b, axis=-1)


# ---------------------------------------------------------------------------------------------------------------------------------
# the float64 host mathematics (the reference of the kernel).  Every routine takes the ray in the shape frame, o / d [N, 3], and returns
# (hit [N] bool, t [N], n [N, 3]): the entering point of the surface that faces the ray, its normal unnormalised in the shape frame
# ---------------------------------------------------------------------------------------------------------------------------------
def _sphere(o, d, r):
    a = _dot(d, d)
    t0 = -_dot(o, d) / a
    c = o + d * t0[:, None]
    disc = r * r - _dot(c, c)
    ok = disc > 0.0
    h = np.sqrt(np.where(ok, disc, 0.0) / a)
    return ok, t0 - h, c - d * h[:, None]


def _lateral(o, d, r):
    """Entering root on the infinite cylinder about z: (root exists, parallel and inside, t)."""
    a = d[:, 0] ** 2 + d[:, 1] ** 2
    par = ~(a > 0.0)
    a_ = np.where(par, 1.0, a)
    t0 = -(o[:, 0] * d[:, 0] + o[:, 1] * d[:, 1]) / a_
    cx, cy = o[:, 0] + d[:, 0] * t0, o[:, 1] + d[:, 1] * t0
    disc = r * r - (cx * cx + cy * cy)
    root = ~par & (disc > 0.0)
    t = t0 - np.sqrt(np.where(root, disc, 0.0) / a_)
    return root, par & (o[:, 0] ** 2 + o[:, 1] ** 2 < r * r), t


def _capped(o, d, r, hh, round_ends):
    root, inside, tl = _lateral(o, d, r)
    z = o[:, 2] + d[:, 2] * tl
    lat = root & (np.abs(z) <= hh)
    end = np.where(root, np.where(z > 0.0, hh, -hh), np.where(d[:, 2] < 0.0, hh, -hh))
    need = (root & ~lat) | inside
    n_lat = np.stack([o[:, 0] + d[:, 0] * tl, o[:, 1] + d[:, 1] * tl, np.zeros_like(tl)], axis=1)
    if round_ends:  # capsule: the hemisphere of that end
        oc = o.copy()
        oc[:, 2] -= end
        ok, ts, p = _sphere(oc, d, r)
        cap = need & ok & ~(p[:, 2] * end < 0.0)
        n_cap = p
    else:  # cylinder: the cap disc
        facing = d[:, 2] * end < 0.0
        ts = (end - o[:, 2]) / np.where(facing, d[:, 2], 1.0)
        x, y = o[:, 0] + d[:, 0] * ts, o[:, 1] + d[:, 1] * ts
        cap = need & facing & (x * x + y * y <= r * r)
        n_cap = np.stack([np.zeros_like(ts), np.zeros_like(ts), end], axis=1)
    return lat | cap, np.where(lat, tl, ts), np.where(lat[:, None], n_lat, n_cap)


def _box(o, d, half):
    t0 = -_dot(o, d) / _dot(d, d)
    c = o + d * t0[:, None]
    nz = d != 0.0
    d_ = np.where(nz, d, 1.0)
    ta, tb = (-half - c) / d_, (half - c) / d_
    tn = np.where(nz, np.minimum(ta, tb), -np.inf)
    tf = np.where(nz, np.maximum(ta, tb), np.inf)
    miss = np.any(~nz & (np.abs(c) >= half), axis=1)  # (a ray in a face plane touches the box, it does not enter it: a miss)
    axis = np.argmax(tn, axis=1)  # (the first axis on a tie)
    t_in, t_out = tn.max(axis=1), tf.min(axis=1)
    n = np.zeros_like(o)
    rows = np.arange(len(o))
    n[rows, axis] = np.where(d[rows, axis] > 0.0, -1.0, 1.0)
    return ~miss & (t_in < t_out), t0 + t_in, n


def _cone(o, d, r, hh):
    t0 = -_dot(o, d) / _dot(d, d)
    c = o + d * t0[:, None]
    k = np.where(hh > 0.0, r / np.where(hh > 0.0, 2.0 * hh, 1.0), 0.0)
    k2 = k * k
    w0 = hh - c[:, 2]
    A = d[:, 0] ** 2 + d[:, 1] ** 2 - k2 * d[:, 2] ** 2
    B = c[:, 0] * d[:, 0] + c[:, 1] * d[:, 1] + k2 * w0 * d[:, 2]
    Cc = c[:, 0] ** 2 + c[:, 1] ** 2 - k2 * w0 * w0
    disc = B * B - A * Cc
    q = -(B + np.where(B < 0.0, -1.0, 1.0) * np.sqrt(np.where(disc >= 0.0, disc, 0.0)))
    best = np.full(len(o), np.inf)
    bn = np.zeros_like(o)
    for num, den in ((q, A), (Cc, q)):
        ok = (disc >= 0.0) & (den != 0.0)
        tr = num / np.where(den != 0.0, den, 1.0)
        w = w0 - tr * d[:, 2]
        nn = np.stack([c[:, 0] + d[:, 0] * tr, c[:, 1] + d[:, 1] * tr, k2 * w], axis=1)
        ok = ok & (w > 0.0) & (w <= 2.0 * hh) & (_dot(nn, d) < 0.0) & (tr < best)
        best = np.where(ok, tr, best)
        bn = np.where(ok[:, None], nn, bn)
    up = d[:, 2] > 0.0  # the base disc, facing -z
    tr = (-hh - c[:, 2]) / np.where(up, d[:, 2], 1.0)
    x, y = c[:, 0] + d[:, 0] * tr, c[:, 1] + d[:, 1] * tr
    ok = up & (x * x + y * y <= r * r) & (tr < best)
    best = np.where(ok, tr, best)
    bn = np.where(ok[:, None], np.array([0.0, 0.0, -1.0]), bn)
    return best < np.inf, t0 + best, bn


def _plane(o, d, s):
    facing = d[:, 2] < 0.0
    t = -o[:, 2] / np.where(facing, d[:, 2], 1.0)
    finite = (s[:, 0] != 0.0) | (s[:, 1] != 0.0)
    x, y = o[:, 0] + d[:, 0] * t, o[:, 1] + d[:, 1] * t
    inside = ~finite | ((np.abs(x) <= s[:, 0]) & (np.abs(y) <= s[:, 1]))
    return facing & inside, t, np.broadcast_to(np.array([0.0, 0.0, 1.0]), o.shape).copy()


def _primitive(gtype, s, o, d):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if gtype == GeoType.PLANE:
            return _plane(o, d, s)
        if gtype in (GeoType.SPHERE, GeoType.ELLIPSOID):
            rad = np.repeat(s[:, :1], 3, axis=1) if gtype == GeoType.SPHERE else s
            ok, t, p = _sphere(o / rad, d / rad, 1.0)
            return ok, t, p / rad
        if gtype == GeoType.BOX:
            return _box(o, d, s)
        if gtype == GeoType.CAPSULE:
            return _capped(o, d, s[:, 0], s[:, 1], True)
        if gtype == GeoType.CYLINDER:
            return _capped(o, d, s[:, 0], s[:, 1], False)
        if gtype == GeoType.CONE:
            return _cone(o, d, s[:, 0], s[:, 1])
    raise NotImplementedError(f"no ray test for {GeoType(gtype).name}")


def _triangles(o, d, v0, v1, v2, s, max_distance):
    """Moeller-Trumbore of every ray against every triangle (vertices [T, 3] times the ray's scale s [N, 3]), front faces only:
    (hit, t, n) of the nearest, the lower triangle index on a tie."""
    N = len(o)
    hit, t_out, n_out = np.zeros(N, bool), np.full(N, np.inf), np.zeros((N, 3))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        chunk = max(1, _PAIR_CHUNK // max(len(v0), 1))
        for c0 in range(0, N, chunk):
            sl = slice(c0, min(c0 + chunk, N))
            oo, dd, ss = o[sl, None, :], d[sl, None, :], s[sl, None, :]
            a0, a1, a2 = v0[None] * ss, v1[None] * ss, v2[None] * ss
            e1, e2 = a1 - a0, a2 - a0
            pvec = np.cross(dd, e2)
            det = _dot(e1, pvec)
            tvec = oo - a0
            u = _dot(tvec, pvec)
            qvec = np.cross(tvec, e1)
            v = _dot(dd, qvec)
            t = _dot(e2, qvec) / np.where(det > 0.0, det, 1.0)
            ok = (det > 0.0) & (u >= 0.0) & (u <= det) & (v >= 0.0) & (u + v <= det) & (t >= 0.0) & (t <= max_distance)
            t = np.where(ok, t, np.inf)
            k = np.argmin(t, axis=1)  # (the first of equal minima: the lower index)
            rows = np.arange(t.shape[0])
            hit[sl], t_out[sl] = ok[rows, k], t[rows, k]
            n_out[sl] = np.cross(e1[rows, k], e2[rows, k])
    return hit, t_out, n_out


def _heightfield_triangles(model, h):
    """The two triangles per cell of heightfield h, vertices in float64 from the float32 record, in the triangle leg's index order."""
    off, nrow, ncol, hx, hy, zlo, zhi = model.heightfield_data[h]
    hx, hy, zlo, zhi = (float(np.float32(x)) for x in (hx, hy, zlo, zhi))
    e = np.asarray(model.heightfield_elevations, dtype=np.float64)[off:off + nrow * ncol].reshape(nrow, ncol)
    dx, dy = 2.0 * hx / (ncol - 1), 2.0 * hy / (nrow - 1)
    x0 = -hx + np.arange(ncol - 1) * dx
    y0 = -hy + np.arange(nrow - 1) * dy
    X0, Y0 = np.meshgrid(x0, y0)  # [row, col]
    z = zlo + e * (zhi - zlo)
    p00 = np.stack([X0, Y0, z[:-1, :-1]], axis=-1)
    p10 = np.stack([X0 + dx, Y0, z[:-1, 1:]], axis=-1)
    p01 = np.stack([X0, Y0 + dy, z[1:, :-1]], axis=-1)
    p11 = np.stack([X0 + dx, Y0 + dy, z[1:, 1:]], axis=-1)
    v0 = np.stack([p00, p00], axis=2).reshape(-1, 3)
    v1 = np.stack([p10, p11], axis=2).reshape(-1, 3)
    v2 = np.stack([p11, p01], axis=2).reshape(-1, 3)
    return v0, v1, v2


def raycast_numpy(model, body_q, origins, directions, ray_body, max_distance, slots, world_mask=None):
    """The contract of nt_raycast in float64: (distance [E, R], normal [E, R, 3], shape [E, R] int32).  body_q [E * nb, 7]; origins /
    directions [R, 3] or [E, R, 3]; ray_body [R]; slots: the selected shape slots (env-local shapes, then global shapes).  Rows of
    worlds outside world_mask are returned as misses."""
    t = model.env
    E, nb, ns = t.env_count, t.nb, t.ns
    bq = np.asarray(_host_array(body_q), dtype=np.float64).reshape(E, nb, 7)
    rb = np.asarray(ray_body, dtype=np.int64).reshape(-1)
    R = len(rb)
    o = np.broadcast_to(np.asarray(_host_array(origins), dtype=np.float64).reshape(-1, R, 3), (E, R, 3))
    d = np.broadcast_to(np.asarray(_host_array(directions), dtype=np.float64).reshape(-1, R, 3), (E, R, 3))
    live = (rb >= -1) & (rb < nb)
    attached = live & (rb >= 0)
    X = bq[:, np.where(attached, rb, 0), :]  # [E, R, 7]
    O = np.where(attached[None, :, None], X[..., :3] + _qrot(X[..., 3:], o), o).reshape(-1, 3)
    D = np.where(attached[None, :, None], _qrot(X[..., 3:], d), d).reshape(-1, 3)
    length = np.linalg.norm(D, axis=1)
    live = np.repeat(live[None, :], E, axis=0).reshape(-1) & (length > 0.0)
    if world_mask is not None:
        live = live & np.repeat(np.asarray(_host_array(world_mask)).astype(bool).reshape(E), R)
    D = D / np.where(length > 0.0, length, 1.0)[:, None]
    N = E * R
    best_t, best_id, best_n = np.full(N, np.inf), np.full(N, np.iinfo(np.int64).max), np.zeros((N, 3))
    xf = np.asarray(model.shape_transform, dtype=np.float64).reshape(-1, 7)
    sc = np.asarray(model.shape_scale, dtype=np.float64).reshape(-1, 3)
    for slot in slots:
        slot = int(slot)
        ids = t.shape_local0 + np.arange(E) * ns + slot if slot < ns else np.full(E, int(t.gshape_id[slot - ns]))
        gtype, body = int(t.shape_type[slot]), int(t.shape_body[slot])
        Xs = xf[ids]
        if body >= 0:
            Xb = bq[:, body]
            Xs = np.concatenate([Xb[:, :3] + _qrot(Xb[:, 3:], Xs[:, :3]), _qmul(Xb[:, 3:], Xs[:, 3:])], axis=1)
        Xs, s, rid = np.repeat(Xs, R, axis=0), np.repeat(sc[ids], R, axis=0), np.repeat(ids, R)
        qi = _qinv(Xs[:, 3:])
        ol, dl = _qrot(qi, O - Xs[:, :3]), _qrot(qi, D)
        if gtype == GeoType.MESH:
            i0 = int(ids[0])
            (vs, nv), (ts, nt) = model.mesh_vertex_range[i0], model.mesh_triangle_range[i0]
            V = np.asarray(model.mesh_vertices, dtype=np.float64)[vs:vs + nv]
            tri = np.asarray(model.mesh_indices)[ts:ts + nt]
            hit, tt, n = _triangles(ol, dl, V[tri[:, 0]], V[tri[:, 1]], V[tri[:, 2]], s, max_distance)
        elif gtype == GeoType.HFIELD:
            v0, v1, v2 = _heightfield_triangles(model, int(model.shape_heightfield_index[int(ids[0])]))
            hit, tt, n = _triangles(ol, dl, v0, v1, v2, np.ones_like(s), max_distance)
        else:
            hit, tt, n = _primitive(gtype, s, ol, dl)
        with np.errstate(invalid="ignore"):
            take = live & hit & (tt >= 0.0) & (tt <= max_distance) & ((tt < best_t) | ((tt == best_t) & (rid < best_id)))
        nw = _qrot(Xs[:, 3:], n / np.where(take, np.linalg.norm(n, axis=1), 1.0)[:, None])
        best_t, best_id = np.where(take, tt, best_t), np.where(take, rid, best_id)
        best_n = np.where(take[:, None], nw, best_n)
    hit = best_t < np.inf
    return (np.where(hit, best_t, -1.0).reshape(E, R), np.where(hit[:, None], best_n, 0.0).reshape(E, R, 3),
            np.where(hit, best_id, -1).astype(np.int32).reshape(E, R))


class SensorRaycast:
    """R rays per world, cast at the shapes of that world (see the module text: one sensor per world, not one camera).

    ``origins`` / ``directions``: [R, 3] (one pattern shared by every world) or [world, R, 3]; ``ray_body``: an int or [R], the
    env-local body a ray is attached to, -1 for the world frame.  ``shape_mask``: bool per shape slot of a world (its env-local shapes,
    then the global shapes), default every slot; ``exclude_bodies`` removes the shapes carried by those env-local bodies (a lidar on
    the robot ignores the robot).  Only surfaces facing the ray are hit, the nearest within ``max_distance`` wins.

    ``eval(state)`` fills ``distance`` [world, R] (-1: miss), ``normal`` [world, R, 3] (unit, world frame; zeros on a miss) and
    ``shape`` [world, R] (Newton shape id, -1 on a miss): resident float32 / int32 tensors on a GPU model, float64 / int32 numpy
    arrays on a host model.  Refused with NotImplementedError: heterogeneous models, and a mask that selects a CONVEX_MESH, a
    GAUSSIAN or a barrel cylinder (they are named)."""

    def __init__(self, model, origins, directions, ray_body=-1, max_distance=1e3, shape_mask=None, exclude_bodies=(), want_normal=True,
                 want_shape=True):
        if getattr(model, "is_heterogeneous", False):
            raise NotImplementedError("SensorRaycast: heterogeneous models are unsupported (one sensor is R rays in every world of a replicated model)")
        t = model.env
        E, nslot = t.env_count, t.ns + t.ng
        self.model, self.max_distance = model, float(max_distance)
        if not self.max_distance >= 0.0:
            raise ValueError("max_distance must be >= 0")
        o = np.asarray(_host_array(origins), dtype=np.float32)
        d = np.asarray(_host_array(directions), dtype=np.float32)
        if o.shape != d.shape or o.ndim not in (2, 3) or o.shape[-1] != 3 or o.shape[-2] == 0 or (o.ndim == 3 and o.shape[0] != E):
            raise ValueError(f"origins / directions must both have shape [R, 3] or [{E}, R, 3]")
        self.ray_count, self.rays_per_world = int(o.shape[-2]), o.ndim == 3
        rb = np.asarray(ray_body, dtype=np.int32).reshape(-1)
        rb = np.full(self.ray_count, rb[0], np.int32) if rb.size == 1 else rb
        if rb.shape != (self.ray_count,) or np.any(rb < -1) or np.any(rb >= t.nb):
            raise ValueError(f"ray_body must be an int or [R] of env-local body indices (-1 .. {t.nb - 1})")
        self.ray_body = rb
        mask = np.ones(nslot, bool) if shape_mask is None else np.asarray(_host_array(shape_mask)).astype(bool).reshape(-1)
        if mask.shape != (nslot,):
            raise ValueError(f"shape_mask must have {nslot} entries (env-local shapes, then global shapes)")
        excluded = [int(b) for b in exclude_bodies]
        if any(not 0 <= b < t.nb for b in excluded):
            raise ValueError(f"exclude_bodies: env-local body indices 0 .. {t.nb - 1}")
        self.shape_mask = mask & ~np.isin(np.asarray(t.shape_body), excluded)
        self.slots = np.flatnonzero(self.shape_mask).astype(np.int32)
        self._check_targets()
        R = self.ray_count
        self._gpu = bool(getattr(model, "is_gpu", False))
        if self._gpu:
            self._init_device(o, d, want_normal, want_shape)
        else:
            self.origins, self.directions = o.copy(), d.copy()
            self.distance = np.full((E, R), -1.0)
            self.normal = np.zeros((E, R, 3)) if want_normal else None
            self.shape = np.full((E, R), -1, np.int32) if want_shape else None

    def _check_targets(self):
        model, t = self.model, self.model.env
        scale = np.asarray(model.shape_scale).reshape(-1, 3)
        bad = []
        for slot in self.slots:
            gtype = int(t.shape_type[slot])
            ids = t.shape_local0 + np.arange(t.env_count) * t.ns + slot if slot < t.ns else np.array([int(t.gshape_id[slot - t.ns])])
            if gtype not in [int(g) for g in RAY_TARGET_TYPES]:
                bad.append(f"slot {int(slot)} (shape {int(ids[0])}): {GeoType(gtype).name}")
            elif gtype == GeoType.CYLINDER and np.any(scale[ids, 2] != 0.0):
                bad.append(f"slot {int(slot)} (shape {int(ids[0])}): barrel CYLINDER")
        if bad:
            raise NotImplementedError("SensorRaycast: these shapes are no ray targets, take them out of shape_mask -- " + "; ".join(bad))

    # -----------------------------------------------------------------------------------------------------------------------------
    def _init_device(self, o, d, want_normal, want_shape):
        import torch  # noqa: PLC0415

        from . import _lib  # noqa: PLC0415

        model, t = self.model, self.model.env
        dm = model.device_model()
        dev = dm.device
        E, R = t.env_count, self.ray_count
        self._keep = []

        def up(a, dtype):
            x = torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)
            if x.numel() == 0:
                x = torch.zeros(1, dtype=x.dtype, device=dev)
            self._keep.append(x)
            return x

        self.origins, self.directions = up(o, np.float32), up(d, np.float32)
        self._ray_body = up(self.ray_body, np.int32)
        self.distance = torch.full((E, R), -1.0, dtype=torch.float32, device=dev)
        self.normal = torch.zeros((E, R, 3), dtype=torch.float32, device=dev) if want_normal else None
        self.shape = torch.full((E, R), -1, dtype=torch.int32, device=dev) if want_shape else None
        self._world_mask = torch.ones(E, dtype=torch.uint8, device=dev)
        types = np.asarray(t.shape_type)[self.slots]
        self._targets_host = np.ascontiguousarray(np.stack([self.slots, types], axis=1), dtype=np.int32).reshape(-1, 2)
        a = _lib.nt_raycast_args()
        a.ray_count, a.rays_per_world = R, int(self.rays_per_world)
        a.origins, a.directions, a.ray_body = self.origins.data_ptr(), self.directions.data_ptr(), self._ray_body.data_ptr()
        a.max_distance, a.target_count = self.max_distance, len(self.slots)
        a.targets, a.targets_host = up(self._targets_host, np.int32).data_ptr(), self._targets_host.ctypes.data
        a.distance = self.distance.data_ptr()
        a.normal = None if self.normal is None else self.normal.data_ptr()
        a.shape = None if self.shape is None else self.shape.data_ptr()
        # The sensor uploads its own mesh / heightfield tables: the copies of sdf_pipeline.SdfLeg exist only for models whose pairs take
        # those legs, and belong to a CollisionPipeline the sensor may never see.
        if np.any(types == int(GeoType.MESH)):
            from .mesh import triangle_block_bounds  # noqa: PLC0415

            vr, tr = np.asarray(model.mesh_vertex_range).reshape(-1, 2), np.asarray(model.mesh_triangle_range).reshape(-1, 2)
            blk_start, blk_of, tables, n_blk = np.zeros(len(vr), np.int32), {}, [], 0
            for i in range(len(vr)):  # one table per distinct mesh, as in sdf_pipeline.SdfLeg
                if tr[i, 1] <= 0:
                    continue
                key = (int(vr[i, 0]), int(tr[i, 0]), int(tr[i, 1]))
                if key not in blk_of:
                    blk_of[key] = n_blk
                    tables.append(triangle_block_bounds(np.asarray(model.mesh_vertices)[vr[i, 0]:vr[i, 0] + vr[i, 1]],
                                                        np.asarray(model.mesh_indices)[tr[i, 0]:tr[i, 0] + tr[i, 1]]))
                    n_blk += len(tables[-1])
                blk_start[i] = blk_of[key]
            a.shape_vertex_range, a.shape_triangle_range = up(vr, np.int32).data_ptr(), up(tr, np.int32).data_ptr()
            a.vertices, a.indices = up(model.mesh_vertices, np.float32).data_ptr(), up(model.mesh_indices, np.int32).data_ptr()
            a.block_bounds, a.shape_block_start = up(np.concatenate(tables), np.float32).data_ptr(), up(blk_start, np.int32).data_ptr()
        if np.any(types == int(GeoType.HFIELD)):
            hf = (_lib.nt_heightfield * model.heightfield_count)()
            for k, (off, nrow, ncol, hx, hy, zlo, zhi) in enumerate(model.heightfield_data):
                hf[k] = _lib.nt_heightfield(int(off), int(nrow), int(ncol), float(hx), float(hy), float(zlo), float(zhi))
            a.shape_heightfield_index = up(model.shape_heightfield_index, np.int32).data_ptr()
            a.heightfields = up(np.frombuffer(bytes(hf), dtype=np.uint8).copy(), np.uint8).data_ptr()
            a.elevations = up(model.heightfield_elevations, np.float32).data_ptr()
        self._args = a

    # -----------------------------------------------------------------------------------------------------------------------------
    def set_rays(self, origins, directions):
        """New origins / directions of the same shape, copied into the resident arrays (a captured graph sees them on its next replay)."""
        for dst, src, what in ((self.origins, origins, "origins"), (self.directions, directions, "directions")):
            if hasattr(dst, "copy_"):
                import torch  # noqa: PLC0415

                x = src if hasattr(src, "data_ptr") else torch.from_numpy(np.ascontiguousarray(_host_array(src), dtype=np.float32))
                if tuple(x.shape) != tuple(dst.shape):
                    raise ValueError(f"{what} must have shape {tuple(dst.shape)}")
                dst.copy_(x)
            else:
                x = np.asarray(_host_array(src), dtype=np.float32)
                if x.shape != dst.shape:
                    raise ValueError(f"{what} must have shape {dst.shape}")
                dst[...] = x

    def eval(self, state, world_mask=None):
        """Cast from ``state.body_q``.  ``world_mask`` ([world] bool): the rows of unselected worlds are neither computed nor written.
        GPU model: one kernel launch on the model's stream (the mask is copied into a resident buffer first)."""
        t = self.model.env
        if world_mask is not None and int(np.prod(np.shape(world_mask))) != t.env_count:
            raise ValueError(f"world_mask must have {t.env_count} entries")
        if self._gpu:
            from . import _lib  # noqa: PLC0415
            from .state import State  # noqa: PLC0415

            if not isinstance(state, State):
                raise TypeError("SensorRaycast.eval: a GPU model needs a State (body_q is read on the device)")
            dm = self.model.device_model()
            if world_mask is not None:
                import torch  # noqa: PLC0415

                wm = world_mask if hasattr(world_mask, "data_ptr") else torch.from_numpy(np.asarray(world_mask).astype(np.uint8))
                self._world_mask.copy_(wm.reshape(-1).to(torch.uint8))
            self._args.world_mask = None if world_mask is None else self._world_mask.data_ptr()
            d = state._desc()
            st = dm.lib.nt_raycast(C.byref(dm.desc), C.byref(d), C.byref(self._args), dm.stream())
            if st == -3:  # NT_ERR_UNSUPPORTED
                raise NotImplementedError("SensorRaycast.eval: nt_raycast answered NT_ERR_UNSUPPORTED (the selected shapes of one world do "
                                          "not fit the LDS, or a shape type is no ray target)")
            _lib.check(st, "nt_raycast")
            return
        dist, normal, shape = raycast_numpy(self.model, state.body_q, self.origins, self.directions, self.ray_body, self.max_distance, self.slots,
                                            world_mask)
        sel = slice(None) if world_mask is None else np.asarray(_host_array(world_mask)).astype(bool).reshape(-1)
        self.distance[sel] = dist[sel]
        if self.normal is not None:
            self.normal[sel] = normal[sel]
        if self.shape is not None:
            self.shape[sel] = shape[sel]


# ---------------------------------------------------------------------------------------------------------------------------------
# SensorTiledCamera: C cameras of width x height pixels in every world (nt_camera_render, contract in include/newton_hip_mesh.h)
# ---------------------------------------------------------------------------------------------------------------------------------
CAMERA_TILE = 8            # NT_CAMERA_TILE: the pixel block of one wave
_CONE_INFLATE = 1.0e-6     # rad added to a block cone's half-angle: above the rounding of its axis to float32 (6e-8)
_CONE_MAX_HALF_ANGLE = np.deg2rad(80.0)  # a wider block is not culled (the test needs cos h comfortably above 0)
_FORWARD = np.array([0.0, 0.0, -1.0])    # the camera looks along -z; +x is right, +y is up


def pinhole_rays(width, height, fov_y):
    """[height * width, 3] float32 camera-frame directions of a pinhole camera with vertical field of view ``fov_y`` (radians): pixel
    (row i, column j), row 0 at the top, looks along (((j + 0.5) / W * 2 - 1) tan(fov_y / 2) W / H, (1 - (i + 0.5) / H * 2) tan(fov_y / 2),
    -1).  Computed in float64 and rounded once; not unit."""
    W, H = int(width), int(height)
    if W <= 0 or H <= 0 or not 0.0 < float(fov_y) < np.pi:
        raise ValueError("pinhole_rays: width and height must be positive and fov_y inside (0, pi)")
    th = np.tan(0.5 * float(fov_y))
    x = ((np.arange(W) + 0.5) / W * 2.0 - 1.0) * th * W / H
    y = (1.0 - (np.arange(H) + 0.5) / H * 2.0) * th
    d = np.empty((H, W, 3))
    d[..., 0], d[..., 1], d[..., 2] = x[None, :], y[:, None], -1.0
    return d.reshape(H * W, 3).astype(np.float32)


def camera_block_cones(directions, width, height):
    """[C, blocks, 5] float32 for ``directions`` [C, H * W, 3] (the float32 table the kernel reads): per 8 x 8 pixel block, numbered
    over block row then block column, the unit axis of a cone about every unit ray of the block, and cos / sin of its half-angle.
    float64 inside; the half-angle is rounded outward by _CONE_INFLATE.  (0, 0, 0, -1, 0) -- no cull -- for a block wider than
    _CONE_MAX_HALF_ANGLE or without a ray of positive length."""
    W, H, T = int(width), int(height), CAMERA_TILE
    d = np.asarray(directions, dtype=np.float64).reshape(-1, H, W, 3)
    by, bx = (H + T - 1) // T, (W + T - 1) // T
    out = np.zeros((len(d), by * bx, 5), np.float32)
    out[..., 3] = -1.0
    for c in range(len(d)):
        for r in range(by):
            for q in range(bx):
                u = d[c, r * T:(r + 1) * T, q * T:(q + 1) * T].reshape(-1, 3)
                n = np.linalg.norm(u, axis=1)
                u = u[n > 0.0] / n[n > 0.0, None]
                if len(u) == 0 or np.linalg.norm(u.sum(axis=0)) == 0.0:
                    continue
                axis = (u.sum(axis=0) / np.linalg.norm(u.sum(axis=0))).astype(np.float32).astype(np.float64)  # as the kernel reads it
                axis_n = axis / np.linalg.norm(axis)
                half = float(np.max(np.arctan2(np.linalg.norm(np.cross(u, axis_n), axis=1), u @ axis_n))) + _CONE_INFLATE
                if half < _CONE_MAX_HALF_ANGLE:
                    out[c, r * bx + q] = [*axis, np.cos(half), np.sin(half)]
    return out


def camera_numpy(model, body_q, ray_origins, ray_bodies, ray_directions, forward, width, height, max_distance, slots, world_mask=None):
    """The contract of nt_camera_render in float64: ``raycast_numpy`` over the expanded rays (origin and body of camera c repeated for
    its H * W directions), reshaped to images: (distance [E, C, H, W], depth, normal [E, C, H, W, 3], shape int32).  depth =
    t (D . F) with D the unit world direction and F the camera's world forward axis; -1 on a miss."""
    t = model.env
    E, nb = t.env_count, t.nb
    W, H = int(width), int(height)
    rb = np.asarray(ray_bodies, dtype=np.int64).reshape(-1)
    Cn = len(rb)
    d = np.asarray(_host_array(ray_directions), dtype=np.float64).reshape(Cn * H * W, 3)
    o = np.repeat(np.asarray(_host_array(ray_origins), dtype=np.float64).reshape(Cn, 3), H * W, axis=0)
    dist, normal, shape = raycast_numpy(model, body_q, o, d, np.repeat(rb, H * W), max_distance, slots, world_mask)
    bq = np.asarray(_host_array(body_q), dtype=np.float64).reshape(E, nb, 7)
    att = (rb >= 0) & (rb < nb)
    q = np.where(att[None, :, None], bq[:, np.where(att, rb, 0), 3:], np.array([0.0, 0.0, 0.0, 1.0]))  # [E, C, 4]
    F = _qrot(q, np.broadcast_to(np.asarray(forward, dtype=np.float64).reshape(1, Cn, 3), (E, Cn, 3)))
    D = _qrot(q[:, :, None, :], np.broadcast_to(d.reshape(1, Cn, H * W, 3), (E, Cn, H * W, 3)))
    n = np.linalg.norm(D, axis=-1, keepdims=True)
    D = D / np.where(n > 0.0, n, 1.0)
    dist = dist.reshape(E, Cn, H * W)
    depth = np.where(dist >= 0.0, dist * np.sum(D * F[:, :, None, :], axis=-1), -1.0)
    return (dist.reshape(E, Cn, H, W), depth.reshape(E, Cn, H, W), normal.reshape(E, Cn, H, W, 3), shape.reshape(E, Cn, H, W))


def _check_ray_targets(name, model, slots):
    """SensorRaycast._check_targets for another sensor: the selected slots must be ray targets."""
    t = model.env
    scale = np.asarray(model.shape_scale).reshape(-1, 3)
    bad = []
    for slot in slots:
        gtype = int(t.shape_type[slot])
        ids = t.shape_local0 + np.arange(t.env_count) * t.ns + slot if slot < t.ns else np.array([int(t.gshape_id[slot - t.ns])])
        if gtype not in [int(g) for g in RAY_TARGET_TYPES]:
            bad.append(f"slot {int(slot)} (shape {int(ids[0])}): {GeoType(gtype).name}")
        elif gtype == GeoType.CYLINDER and np.any(scale[ids, 2] != 0.0):
            bad.append(f"slot {int(slot)} (shape {int(ids[0])}): barrel CYLINDER")
    if bad:
        raise NotImplementedError(f"{name}: these shapes are no ray targets, take them out of shape_mask -- " + "; ".join(bad))


def _upload_ray_target_tables(model, types, a, up):
    """The mesh / heightfield tables the selected target ``types`` need, uploaded with ``up`` and entered into the argument struct
    ``a`` (the field names of nt_raycast_args), as SensorRaycast builds them: block bounds per distinct mesh."""
    from . import _lib  # noqa: PLC0415

    if np.any(types == int(GeoType.MESH)):
        from .mesh import triangle_block_bounds  # noqa: PLC0415

        vr, tr = np.asarray(model.mesh_vertex_range).reshape(-1, 2), np.asarray(model.mesh_triangle_range).reshape(-1, 2)
        blk_start, blk_of, tables, n_blk = np.zeros(len(vr), np.int32), {}, [], 0
        for i in range(len(vr)):
            if tr[i, 1] <= 0:
                continue
            key = (int(vr[i, 0]), int(tr[i, 0]), int(tr[i, 1]))
            if key not in blk_of:
                blk_of[key] = n_blk
                tables.append(triangle_block_bounds(np.asarray(model.mesh_vertices)[vr[i, 0]:vr[i, 0] + vr[i, 1]],
                                                    np.asarray(model.mesh_indices)[tr[i, 0]:tr[i, 0] + tr[i, 1]]))
                n_blk += len(tables[-1])
            blk_start[i] = blk_of[key]
        a.shape_vertex_range, a.shape_triangle_range = up(vr, np.int32).data_ptr(), up(tr, np.int32).data_ptr()
        a.vertices, a.indices = up(model.mesh_vertices, np.float32).data_ptr(), up(model.mesh_indices, np.int32).data_ptr()
        a.block_bounds, a.shape_block_start = up(np.concatenate(tables), np.float32).data_ptr(), up(blk_start, np.int32).data_ptr()
    if np.any(types == int(GeoType.HFIELD)):
        hf = (_lib.nt_heightfield * model.heightfield_count)()
        for k, (off, nrow, ncol, hx, hy, zlo, zhi) in enumerate(model.heightfield_data):
            hf[k] = _lib.nt_heightfield(int(off), int(nrow), int(ncol), float(hx), float(hy), float(zlo), float(zhi))
        a.shape_heightfield_index = up(model.shape_heightfield_index, np.int32).data_ptr()
        a.heightfields = up(np.frombuffer(bytes(hf), dtype=np.uint8).copy(), np.uint8).data_ptr()
        a.elevations = up(model.heightfield_elevations, np.float32).data_ptr()


class SensorTiledCamera:
    """C depth cameras of ``width`` x ``height`` pixels in every world (the capability of the reference's
    ``newton.sensors.SensorTiledCamera``): the observation of a vision policy, one image per world and camera.

    ``cameras``: a sequence of ``(body, xform)`` exactly as SensorFrameTransform's ``frames`` -- an env-local body (or -1: fixed in the
    world) and the camera's pose in it, 7 numbers (p, q xyzw) or None.  The same C cameras exist in every world; per-world camera
    poses are out of scope.  Camera frame: +x right, +y up, looking along -z; pixel (row i, column j) has row 0 at the top.  The lens
    is a table of camera-frame directions (not necessarily unit): ``rays`` [H * W, 3] or [C, H * W, 3] -- any distortion -- or
    ``fov_y`` for ``pinhole_rays``; exactly one of the two.  ``shape_mask``, ``exclude_bodies``, ``max_distance``: as SensorRaycast.

    ``eval(state)`` fills, per pixel, ``distance`` [world, C, H, W] (t along the unit ray, -1: miss -- SensorRaycast's values for the
    same rays, bit for bit on the device), ``depth`` (t times the cosine to the optical axis: the distance along the camera's forward
    axis, -1: miss), ``normal`` [world, C, H, W, 3] (unit, world frame, zeros on a miss) and ``shape`` (Newton shape id, -1).  There
    is no colour image: the model carries no shape colours.  ``ray_origins`` [C, 3], ``ray_bodies`` [C] and ``ray_directions``
    [C, H * W, 3] are exactly what the kernel reads: the body frame, float32, the directions turned by the camera's rotation in float64
    and rounded once.

    GPU model: resident float32 / int32 tensors, one launch of camera_kernel on the model's stream per ``eval`` (one wave per 8 x 8
    pixels), no allocation, recordable by ``newton_amd.graph.capture``.  ``cull``: the wave of a block skips the bounded primitives
    no ray of the block can reach; it changes no output bit.  Host model: float64 / int32 numpy (``camera_numpy``).  Refused with
    NotImplementedError: heterogeneous models, and a mask that selects a CONVEX_MESH, a GAUSSIAN or a barrel cylinder."""

    def __init__(self, model, cameras, width, height, rays=None, fov_y=None, max_distance=1e3, shape_mask=None, exclude_bodies=(),
                 want_depth=True, want_normal=True, want_shape=True, cull=True):
        if getattr(model, "is_heterogeneous", False):
            raise NotImplementedError("SensorTiledCamera: heterogeneous models are unsupported (one sensor is C cameras in every world of a "
                                      "replicated model)")
        t = model.env
        E, nslot = t.env_count, t.ns + t.ng
        self.model, self.max_distance = model, float(max_distance)
        self.width, self.height, self.cull = int(width), int(height), bool(cull)
        W, H = self.width, self.height
        if W <= 0 or H <= 0:
            raise ValueError("SensorTiledCamera: width and height must be positive")
        if not self.max_distance >= 0.0:
            raise ValueError("max_distance must be >= 0")
        cameras = list(cameras)
        Cn = self.camera_count = len(cameras)
        if Cn == 0:
            raise ValueError("SensorTiledCamera: no camera")
        if (rays is None) == (fov_y is None):
            raise ValueError("SensorTiledCamera: give exactly one of rays and fov_y")
        lens = pinhole_rays(W, H, fov_y) if rays is None else np.asarray(_host_array(rays), dtype=np.float32)
        if lens.shape not in ((H * W, 3), (Cn, H * W, 3)) or not np.all(np.isfinite(lens)):
            raise ValueError(f"SensorTiledCamera: rays must be finite with shape [{H * W}, 3] or [{Cn}, {H * W}, 3]")
        self._lens = np.broadcast_to(lens.astype(np.float64), (Cn, H * W, 3))
        mask = np.ones(nslot, bool) if shape_mask is None else np.asarray(_host_array(shape_mask)).astype(bool).reshape(-1)
        if mask.shape != (nslot,):
            raise ValueError(f"shape_mask must have {nslot} entries (env-local shapes, then global shapes)")
        excluded = [int(b) for b in exclude_bodies]
        if any(not 0 <= b < t.nb for b in excluded):
            raise ValueError(f"exclude_bodies: env-local body indices 0 .. {t.nb - 1}")
        self.shape_mask = mask & ~np.isin(np.asarray(t.shape_body), excluded)
        self.slots = np.flatnonzero(self.shape_mask).astype(np.int32)
        _check_ray_targets("SensorTiledCamera", model, self.slots)
        self.blocks = Cn * ((H + CAMERA_TILE - 1) // CAMERA_TILE) * ((W + CAMERA_TILE - 1) // CAMERA_TILE)
        self._tables(cameras)
        self._gpu = bool(getattr(model, "is_gpu", False))
        if self._gpu:
            self._init_device(want_depth, want_normal, want_shape)
        else:
            self.distance = np.full((E, Cn, H, W), -1.0)
            self.depth = np.full((E, Cn, H, W), -1.0) if want_depth else None
            self.normal = np.zeros((E, Cn, H, W, 3)) if want_normal else None
            self.shape = np.full((E, Cn, H, W), -1, np.int32) if want_shape else None

    def _tables(self, cameras):
        """The host tables of ``cameras``: what the kernel reads, float32, computed in float64 and rounded once."""
        if len(cameras) != self.camera_count:
            raise ValueError(f"SensorTiledCamera: {self.camera_count} cameras expected, got {len(cameras)}")
        body, xf = _frame_table("SensorTiledCamera", self.model, cameras)
        q = xf[:, None, 3:] / np.linalg.norm(xf[:, None, 3:], axis=-1, keepdims=True)
        self.ray_bodies = body
        self.ray_origins = xf[:, :3].astype(np.float32)
        self.ray_directions = _qrot(q, self._lens).astype(np.float32)
        self.forward = _qrot(q[:, 0], np.broadcast_to(_FORWARD, (len(body), 3))).astype(np.float32)
        self.block_cones = camera_block_cones(self.ray_directions, self.width, self.height)

    # -----------------------------------------------------------------------------------------------------------------------------
    def _init_device(self, want_depth, want_normal, want_shape):
        import torch  # noqa: PLC0415

        from . import _lib  # noqa: PLC0415

        model, t = self.model, self.model.env
        dev = model.device_model().device
        E, Cn, H, W = t.env_count, self.camera_count, self.height, self.width
        self._keep = []

        def up(a, dtype):
            x = torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)
            if x.numel() == 0:
                x = torch.zeros(1, dtype=x.dtype, device=dev)
            self._keep.append(x)
            return x

        self._resident = {k: up(getattr(self, k), np.int32 if k == "ray_bodies" else np.float32)
                          for k in ("ray_origins", "ray_bodies", "ray_directions", "forward", "block_cones")}
        self.distance = torch.full((E, Cn, H, W), -1.0, dtype=torch.float32, device=dev)
        self.depth = torch.full((E, Cn, H, W), -1.0, dtype=torch.float32, device=dev) if want_depth else None
        self.normal = torch.zeros((E, Cn, H, W, 3), dtype=torch.float32, device=dev) if want_normal else None
        self.shape = torch.full((E, Cn, H, W), -1, dtype=torch.int32, device=dev) if want_shape else None
        self._world_mask = torch.ones(E, dtype=torch.uint8, device=dev)
        types = np.asarray(t.shape_type)[self.slots]
        self._targets_host = np.ascontiguousarray(np.stack([self.slots, types], axis=1), dtype=np.int32).reshape(-1, 2)
        a = _lib.nt_camera_args()
        a.camera_count, a.width, a.height = Cn, W, H
        for k in ("ray_origins", "ray_bodies", "ray_directions", "forward", "block_cones"):
            setattr(a, k, self._resident[k].data_ptr())
        a.max_distance, a.target_count = self.max_distance, len(self.slots)
        a.targets, a.targets_host = up(self._targets_host, np.int32).data_ptr(), self._targets_host.ctypes.data
        for k in ("distance", "depth", "normal", "shape"):
            setattr(a, k, None if getattr(self, k) is None else getattr(self, k).data_ptr())
        a.flags = 1 if self.cull else 0  # NT_CAMERA_CULL
        _upload_ray_target_tables(model, types, a, up)
        self._args = a

    def set_cameras(self, cameras):
        """New ``(body, xform)`` of the same C cameras: the tables and the cull cones are recomputed and copied into the resident
        arrays (a captured graph sees the new poses on its next replay)."""
        self._tables(list(cameras))
        if self._gpu:
            import torch  # noqa: PLC0415

            for k, dst in self._resident.items():
                dst.copy_(torch.from_numpy(np.ascontiguousarray(getattr(self, k))).reshape(dst.shape))

    def eval(self, state, world_mask=None):
        """Render from ``state.body_q``.  ``world_mask`` ([world] bool): the images of unselected worlds are neither computed nor
        written.  GPU model: one kernel launch on the model's stream (the mask is copied into a resident buffer first)."""
        t = self.model.env
        if world_mask is not None and int(np.prod(np.shape(world_mask))) != t.env_count:
            raise ValueError(f"world_mask must have {t.env_count} entries")
        if self._gpu:
            from . import _lib  # noqa: PLC0415
            from .state import State  # noqa: PLC0415

            if not isinstance(state, State):
                raise TypeError("SensorTiledCamera.eval: a GPU model needs a State (body_q is read on the device)")
            dm = self.model.device_model()
            if world_mask is not None:
                import torch  # noqa: PLC0415

                wm = world_mask if hasattr(world_mask, "data_ptr") else torch.from_numpy(np.asarray(world_mask).astype(np.uint8))
                self._world_mask.copy_(wm.reshape(-1).to(torch.uint8))
            self._args.world_mask = None if world_mask is None else self._world_mask.data_ptr()
            d = state._desc()
            st = dm.lib.nt_camera_render(C.byref(dm.desc), C.byref(d), C.byref(self._args), dm.stream())
            if st == -3:  # NT_ERR_UNSUPPORTED
                raise NotImplementedError("SensorTiledCamera.eval: nt_camera_render answered NT_ERR_UNSUPPORTED (the selected shapes of one "
                                          "world do not fit the LDS, or a shape type is no ray target)")
            _lib.check(st, "nt_camera_render")
            return
        got = camera_numpy(self.model, state.body_q, self.ray_origins, self.ray_bodies, self.ray_directions, self.forward, self.width,
                           self.height, self.max_distance, self.slots, world_mask)
        sel = slice(None) if world_mask is None else np.asarray(_host_array(world_mask)).astype(bool).reshape(-1)
        for dst, src in zip((self.distance, self.depth, self.normal, self.shape), got):
            if dst is not None:
                dst[sel] = src[sel]


# ---------------------------------------------------------------------------------------------------------------------------------
# SensorContact: net contact force per world on chosen bodies / shapes, split by counterpart (nt_contact_sensor, contract in
# include/newton_hip_contacts.h)
# ---------------------------------------------------------------------------------------------------------------------------------
def contact_sensor_numpy(model, count, shape0, shape1, force, slot_sensing, slot_counterpart, sensing_count, counterpart_count,
                         include_total=True, world_mask=None, dtype=np.float64):
    """The contract of nt_contact_sensor over Newton's flat arrays: net_force [E, S, include_total + C, 3] in ``dtype`` (float64: the
    reference the kernel is tested against; float32: the kernel's own sequential sum when the flat order is the raw export order).
    ``count`` / ``shape0`` / ``shape1`` / ``force``: rigid_contact_count, rigid_contact_shape0 / _shape1 and Contacts.force (its linear
    part is read); every world's entries are added in their flat order, +f on the sensing object of shape0, then -f on that of shape1.
    The world of an entry is that of its env-local shape; entries with shape0 < 0, with shape0 == shape1 or between shapes of no one
    world are skipped.  Rows of worlds outside ``world_mask`` stay zero."""
    t = model.env
    E, ns, lo = t.env_count, t.ns, t.shape_local0
    S, Cn, tot = int(sensing_count), int(counterpart_count), int(bool(include_total))
    sens = np.asarray(slot_sensing, dtype=np.int64).reshape(-1)
    cpart = np.full(ns + t.ng, -1, np.int64) if Cn == 0 else np.asarray(slot_counterpart, dtype=np.int64).reshape(-1)
    gslot = {int(g): ns + k for k, g in enumerate(np.asarray(t.gshape_id).reshape(-1)[:t.ng])}
    n = int(np.asarray(_host_array(count)).reshape(-1)[0])
    s0 = np.asarray(_host_array(shape0)).reshape(-1)
    s1 = np.asarray(_host_array(shape1)).reshape(-1)
    f = np.asarray(_host_array(force)).reshape(len(s0), -1)[:, :3].astype(dtype)
    n = min(n, len(s0))
    mask = None if world_mask is None else np.asarray(_host_array(world_mask)).astype(bool).reshape(E)
    out = np.zeros((E, S, tot + Cn, 3), dtype=dtype)

    def locate(i):  # (world or -1 for a global shape, slot or -1)
        if lo <= i < lo + E * ns:
            return (i - lo) // ns, (i - lo) % ns
        return -1, gslot.get(i, -1)

    for i in range(n):
        a, b = int(s0[i]), int(s1[i])
        if a < 0 or a == b:
            continue
        (wa, sa), (wb, sb) = locate(a), locate(b)
        w = wa if wa >= 0 else wb
        if w < 0 or (wa >= 0 and wb >= 0 and wa != wb) or (mask is not None and not mask[w]):
            continue
        for mine, other, sign in ((sa, sb, 1), (sb, sa, -1)):
            k = sens[mine] if mine >= 0 else -1
            if k < 0:
                continue
            c = cpart[other] if other >= 0 else -1
            if tot:
                out[w, k, 0] = out[w, k, 0] + f[i] if sign > 0 else out[w, k, 0] - f[i]
            if c >= 0:
                out[w, k, tot + c] = out[w, k, tot + c] + f[i] if sign > 0 else out[w, k, tot + c] - f[i]
    return out


class SensorContact:
    """Net contact force on chosen bodies / shapes of every world, split by counterpart (the capability of the reference's
    ``newton.sensors.SensorContact``): feet against the ground give contact flags, air time and reward terms.

    Indices are env-local.  ``sensing_bodies`` / ``counterpart_bodies``: bodies 0 .. nb-1, a body meaning every shape it carries;
    ``sensing_shapes`` / ``counterpart_shapes``: shape slots 0 .. ns+ng-1, the global shapes addressed as ns + k (the ground plane).
    The sensing objects are the bodies in the given order, then the shapes (``sensing_labels``, a list of ("body", i) / ("shape", slot));
    the counterparts likewise (``counterpart_labels``).  A shape slot belongs to at most one sensing object and at most one counterpart.

    ``eval(contacts)`` fills ``net_force`` [world, S, include_total + C, 3], the force ON the sensing object: column 0 the total over
    all its contacts (with ``include_total``), column include_total + c the part exchanged with counterpart c; ``shape`` is
    (S, include_total + C).  GPU model: one launch of contact_sensor_kernel on the model's stream straight from the contacts a
    ``SolverXPBD.step`` reported its impulses into (``model.request_contact_attributes("force")`` before the Contacts are created;
    ``update_contacts`` is neither needed nor called), float32, every cell a sequential sum over the world's slots, then its SDF-leg
    rows; recordable by ``newton_amd.graph.capture``.  Host model, or any object with numpy ``rigid_contact_count`` /
    ``rigid_contact_shape0`` / ``rigid_contact_shape1`` / ``force``: the same contract in float64 (``contact_sensor_numpy``)."""

    def __init__(self, model, sensing_bodies=(), sensing_shapes=(), counterpart_bodies=(), counterpart_shapes=(), include_total=True):
        if getattr(model, "is_heterogeneous", False):
            raise NotImplementedError("SensorContact: heterogeneous models are unsupported (one sensor is S sensing objects in every world of a replicated model)")
        t = model.env
        nslot = t.ns + t.ng
        self.model, self.include_total = model, bool(include_total)
        shape_body = np.asarray(t.shape_body).reshape(-1)[:nslot]

        def table(bodies, shapes, what):
            tab, labels = np.full(nslot, -1, np.int32), []
            for kind, idx in [("body", b) for b in bodies] + [("shape", s) for s in shapes]:
                idx, hi = int(idx), (t.nb if kind == "body" else nslot)
                if not 0 <= idx < hi:
                    raise ValueError(f"SensorContact: {what} {kind} {idx} is out of range (env-local 0 .. {hi - 1})")
                slots = np.flatnonzero(shape_body == idx) if kind == "body" else np.array([idx])
                for slot in slots:
                    if tab[slot] >= 0:
                        raise ValueError(f"SensorContact: shape slot {int(slot)} is claimed by two {what} objects, "
                                         f"{labels[tab[slot]]} and {(kind, idx)}")
                    tab[slot] = len(labels)
                labels.append((kind, idx))
            return tab, labels

        self.slot_sensing, self.sensing_labels = table(sensing_bodies, sensing_shapes, "sensing")
        self.slot_counterpart, self.counterpart_labels = table(counterpart_bodies, counterpart_shapes, "counterpart")
        if not self.sensing_labels:
            raise ValueError("SensorContact: no sensing object (give sensing_bodies and / or sensing_shapes)")
        S, cols = len(self.sensing_labels), int(self.include_total) + len(self.counterpart_labels)
        if cols == 0:
            raise ValueError("SensorContact: no output column (include_total is off and there is no counterpart)")
        self.shape = (S, cols)
        self._gpu = bool(getattr(model, "is_gpu", False))
        if self._gpu:
            import torch  # noqa: PLC0415

            from . import _lib  # noqa: PLC0415

            dev = model.device_model().device
            self.net_force = torch.zeros((t.env_count, S, cols, 3), dtype=torch.float32, device=dev)
            self._world_mask = torch.ones(t.env_count, dtype=torch.uint8, device=dev)
            self._tables = (torch.from_numpy(self.slot_sensing).to(dev), torch.from_numpy(self.slot_counterpart).to(dev))
            a = _lib.nt_contact_sensor_args()
            a.sensing_count, a.counterpart_count, a.include_total = S, len(self.counterpart_labels), int(self.include_total)
            a.slot_sensing, a.slot_counterpart = self._tables[0].data_ptr(), self._tables[1].data_ptr()
            a.slot_sensing_host, a.slot_counterpart_host = self.slot_sensing.ctypes.data, self.slot_counterpart.ctypes.data
            a.net_force = self.net_force.data_ptr()
            self._args = a
        else:
            self.net_force = np.zeros((t.env_count, S, cols, 3))

    def eval(self, contacts, world_mask=None):
        """Sum the contact forces of ``contacts``.  ``world_mask`` ([world] bool): the rows of unselected worlds are neither computed
        nor written.  GPU model: one kernel launch on the model's stream (the mask is copied into a resident buffer first)."""
        t = self.model.env
        if world_mask is not None and int(np.prod(np.shape(world_mask))) != t.env_count:
            raise ValueError(f"world_mask must have {t.env_count} entries")
        S, Cn = len(self.sensing_labels), len(self.counterpart_labels)
        if self._gpu:
            from . import _lib  # noqa: PLC0415

            if getattr(contacts, "force", None) is None or getattr(contacts, "_impulse", None) is None:
                raise ValueError("SensorContact.eval: contacts.force is not allocated. Call model.request_contact_attributes('force') "
                                 "before creating the Contacts object.")
            dt = getattr(contacts, "_impulse_dt", None)
            if dt is None:
                raise ValueError("SensorContact.eval: no contact impulses on these contacts. Call SolverXPBD.step() with them first.")
            dm = self.model.device_model()
            if world_mask is not None:
                import torch  # noqa: PLC0415

                wm = world_mask if hasattr(world_mask, "data_ptr") else torch.from_numpy(np.asarray(world_mask).astype(np.uint8))
                self._world_mask.copy_(wm.reshape(-1).to(torch.uint8))
            a = self._args
            a.world_mask = None if world_mask is None else self._world_mask.data_ptr()
            flat = getattr(contacts, "_flat", None)
            a.row_capacity = int(flat.capacity) if flat is not None and flat.impulse is not None else 0
            d = contacts._desc()
            _lib.check(dm.lib.nt_contact_sensor(C.byref(dm.desc), C.byref(d), contacts._impulse.data_ptr(), float(dt), C.byref(a),
                                                dm.stream()), "nt_contact_sensor")
            return
        out = contact_sensor_numpy(self.model, contacts.rigid_contact_count, contacts.rigid_contact_shape0, contacts.rigid_contact_shape1,
                                   contacts.force, self.slot_sensing, self.slot_counterpart, S, Cn, self.include_total, world_mask)
        sel = slice(None) if world_mask is None else np.asarray(_host_array(world_mask)).astype(bool).reshape(-1)
        self.net_force[sel] = out[sel]


# ---------------------------------------------------------------------------------------------------------------------------------
# SensorFrameTransform / SensorIMU: pose, velocity, gravity direction and specific force of sensor-owned frames (nt_frame_sensor,
# contract in include/newton_hip_kinematics.h)
# ---------------------------------------------------------------------------------------------------------------------------------
_QUAT_NORM_TOL = 1.0e-4  # nt_frame_sensor's own bound on | |q| - 1 | of a frame's local rotation


def _world_gravity(model, dtype=np.float64):
    """[E, 3]: the gravity row of every world, chosen as newton_amd.model.pack_param_arrays chooses nt_model.gravity."""
    t = model.env
    g = np.asarray(model.gravity, dtype=dtype).reshape(-1, 3)
    world = np.asarray(model.body_world).reshape(t.env_count, t.nb)[:, 0] if t.nb else np.zeros(t.env_count, np.int64)
    return g[world]


def frame_sensor_numpy(model, body_q, body_qd, frame_body, frame_xform, out_frame, out_ref, body_qd_prev=None, dt=None, world_mask=None,
                       dtype=np.float64, with_scale=False):
    """The contract of nt_frame_sensor over Newton's flat AoS arrays (body_q [E * nb, 7], body_qd / body_qd_prev [E * nb, 6]): a dict
    with ``transform`` [E, N, 7], ``velocity`` [E, N, 6], ``gravity_dir`` [E, N, 3] and ``accel`` [E, N, 3] in ``dtype`` (float64: the
    reference the kernel is tested against, and the host-model path).  ``velocity`` is None without body_qd, ``accel`` without
    body_qd_prev / dt.  Rows of worlds outside ``world_mask`` stay zero.  ``with_scale``: a fifth entry ``scale``, a dict of arrays that
    broadcast against the four outputs -- per element the sum of the magnitudes of the terms the contract adds to form it (what a
    rounding-error bound of the float32 kernel is proportional to)."""
    t = model.env
    E, nb = t.env_count, t.nb
    fb = np.asarray(frame_body, dtype=np.int64).reshape(-1)
    fx = np.asarray(_host_array(frame_xform), dtype=dtype).reshape(len(fb), 7)
    of = np.asarray(out_frame, dtype=np.int64).reshape(-1)
    orf = np.asarray(out_ref, dtype=np.int64).reshape(-1)
    bq = np.asarray(_host_array(body_q), dtype=dtype).reshape(E, nb, 7)
    att = fb >= 0
    bi = np.where(att, fb, 0)
    sel3 = att[None, :, None]
    pl, ql = fx[None, :, :3], fx[None, :, 3:]
    P, Q = bq[:, bi, :3], bq[:, bi, 3:]  # [E, M, ...]
    x = np.where(sel3, P + _qrot(Q, pl), pl)
    qf = np.where(sel3, _qmul(Q, ql), ql)
    g = _world_gravity(model, dtype)  # [E, 3]
    gn = np.linalg.norm(g, axis=-1, keepdims=True)
    gdir = np.where(gn > 0.0, g / np.where(gn > 0.0, gn, 1.0), 0.0)
    live = np.ones(E, bool) if world_mask is None else np.asarray(_host_array(world_mask)).astype(bool).reshape(E)
    norm = lambda a: np.linalg.norm(a, axis=-1, keepdims=True)  # noqa: E731

    # transform: X_ref^-1 X_frame
    has_ref = (orf >= 0)[None, :, None]
    ri = np.where(orf >= 0, orf, 0)
    xr, qr = x[:, ri], qf[:, ri]
    xm, qm = x[:, of], qf[:, of]
    out = {"transform": np.concatenate([np.where(has_ref, _qrot(_qinv(qr), xm - xr), xm), np.where(has_ref, _qmul(_qinv(qr), qm), qm)],
                                       axis=-1),
           "velocity": None, "accel": None,
           "gravity_dir": _qrot(_qinv(qm), np.broadcast_to(gdir[:, None, :], xm.shape))}
    scale = {"transform": np.concatenate([np.broadcast_to(norm(xm) + np.where(has_ref, norm(xr), 0.0), xm.shape), np.ones_like(qm)], axis=-1),
             "gravity_dir": np.ones(()), "velocity": None, "accel": None}
    if body_qd is not None:
        bqd = np.asarray(_host_array(body_qd), dtype=dtype).reshape(E, nb, 6)
        com = np.asarray(model.body_com, dtype=dtype).reshape(E, nb, 3)
        r = np.where(sel3, _qrot(Q, pl - com[:, bi]), 0.0)
        vc, w = np.where(sel3, bqd[:, bi, :3], 0.0), np.where(sel3, bqd[:, bi, 3:], 0.0)
        v = vc + np.cross(w, r)
        out["velocity"] = np.concatenate([_qrot(_qinv(qm), v[:, of]), _qrot(_qinv(qm), w[:, of])], axis=-1)
        s_lin = norm(vc) + norm(w) * norm(r)
        # (the angular half adds nothing to w: its own magnitude bounds it, and never more than the linear half's scale is allowed)
        scale["velocity"] = np.concatenate([np.broadcast_to(s_lin[:, of], xm.shape),
                                            np.broadcast_to(np.minimum(s_lin, norm(w))[:, of], xm.shape)], axis=-1)
        if body_qd_prev is not None:
            if dt is None or not float(dt) > 0.0:
                raise ValueError("frame_sensor_numpy: accel needs dt > 0, the time between the two states")
            dt = float(dt)
            pqd = np.asarray(_host_array(body_qd_prev), dtype=dtype).reshape(E, nb, 6)
            vp, wp = np.where(sel3, pqd[:, bi, :3], 0.0), np.where(sel3, pqd[:, bi, 3:], 0.0)
            acc = (vc - vp) / dt + np.cross((w - wp) / dt, r) + np.cross(w, np.cross(w, r)) - g[:, None, :]
            out["accel"] = _qrot(_qinv(qm), acc[:, of])
            s_acc = (norm(vc) + norm(vp) + (norm(w) + norm(wp)) * norm(r)) / dt + norm(w) ** 2 * norm(r) + gn[:, None, :]
            scale["accel"] = np.broadcast_to(s_acc[:, of], xm.shape)
    for k, v_ in out.items():
        if v_ is not None:
            out[k] = np.where(live[:, None, None], v_, 0.0).astype(dtype)
    if with_scale:
        out["scale"] = scale
    return out


def _frame_table(name, model, table):
    """[(body, xform or None)] checked for sensor ``name``: (body [M] int32, xform [M, 7] float64)."""
    nb = model.env.nb
    bodies, xforms = np.zeros(len(table), np.int32), np.zeros((len(table), 7))
    for k, (body, xf) in enumerate(table):
        body = int(body)
        if not -1 <= body < nb:
            raise ValueError(f"{name}: frame {k}: body {body} is out of range (env-local 0 .. {nb - 1}, or -1 for the world)")
        xf = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]) if xf is None else np.asarray(_host_array(xf), dtype=np.float64).reshape(-1)
        if xf.shape != (7,) or not np.all(np.isfinite(xf)):
            raise ValueError(f"{name}: frame {k}: xform must be 7 finite numbers (p, q xyzw) or None")
        if abs(np.linalg.norm(xf[3:]) - 1.0) > _QUAT_NORM_TOL:
            raise ValueError(f"{name}: frame {k}: the quaternion of xform is not a unit quaternion (norm {np.linalg.norm(xf[3:]):.6g})")
        bodies[k], xforms[k] = body, xf
    return bodies, xforms


class _FrameSensor:
    """What SensorFrameTransform and SensorIMU share: the frame table, its checks, the resident outputs and the one launch."""

    def _setup(self, model, table, out_frame, out_ref, outputs):
        """table: [(body, xform or None)]; outputs: {name of the entry point's output: (attribute, components)} to allocate."""
        name = type(self).__name__
        if getattr(model, "is_heterogeneous", False):
            raise NotImplementedError(f"{name}: heterogeneous models are unsupported (one sensor is N frames in every world of a replicated model)")
        t = model.env
        self.model = model
        M = len(table)
        self.frame_body, xf = _frame_table(name, model, table)
        self.frame_xform = xf.astype(np.float32)
        self.out_frame = np.ascontiguousarray(out_frame, dtype=np.int32)
        self.out_ref = np.ascontiguousarray(out_ref, dtype=np.int32)
        E, N = t.env_count, len(self.out_frame)
        self._gpu = bool(getattr(model, "is_gpu", False))
        self._out = {}
        if self._gpu:
            import torch  # noqa: PLC0415

            from . import _lib  # noqa: PLC0415

            dev = model.device_model().device
            self._world_mask = torch.ones(E, dtype=torch.uint8, device=dev)
            self._tables = [torch.from_numpy(x).to(dev) for x in (self.frame_body, self.frame_xform, self.out_frame, self.out_ref)]
            a = _lib.nt_frame_sensor_args()
            a.frame_count, a.out_count = M, N
            a.frame_body, a.frame_xform, a.out_frame, a.out_ref = (x.data_ptr() for x in self._tables)
            a.frame_body_host, a.frame_xform_host = self.frame_body.ctypes.data, self.frame_xform.ctypes.data
            a.out_frame_host, a.out_ref_host = self.out_frame.ctypes.data, self.out_ref.ctypes.data
            for key, ncomp in outputs.items():
                self._out[key] = torch.zeros((E, N, ncomp), dtype=torch.float32, device=dev)
                setattr(a, key, self._out[key].data_ptr())
            self._args = a
        else:
            for key, ncomp in outputs.items():
                self._out[key] = np.zeros((E, N, ncomp))

    def _launch(self, state, state_prev, dt, world_mask):
        name, t = type(self).__name__, self.model.env
        if world_mask is not None and int(np.prod(np.shape(world_mask))) != t.env_count:
            raise ValueError(f"world_mask must have {t.env_count} entries")
        if self._gpu:
            from . import _lib  # noqa: PLC0415
            from .state import State  # noqa: PLC0415

            if not isinstance(state, State) or not (state_prev is None or isinstance(state_prev, State)):
                raise TypeError(f"{name}.eval: a GPU model needs State objects (body_q / body_qd are read on the device)")
            dm = self.model.device_model()
            if world_mask is not None:
                import torch  # noqa: PLC0415

                wm = world_mask if hasattr(world_mask, "data_ptr") else torch.from_numpy(np.asarray(world_mask).astype(np.uint8))
                self._world_mask.copy_(wm.reshape(-1).to(torch.uint8))
            self._args.world_mask = None if world_mask is None else self._world_mask.data_ptr()
            d = state._desc()
            dp = None if state_prev is None else state_prev._desc()
            _lib.check(dm.lib.nt_frame_sensor(C.byref(dm.desc), C.byref(d), None if dp is None else C.byref(dp), float(dt), C.byref(self._args),
                                              dm.stream()), "nt_frame_sensor")
            return
        got = frame_sensor_numpy(self.model, state.body_q, state.body_qd, self.frame_body, self.frame_xform, self.out_frame, self.out_ref,
                                 None if state_prev is None else state_prev.body_qd, dt if state_prev is not None else None, world_mask)
        sel = slice(None) if world_mask is None else np.asarray(_host_array(world_mask)).astype(bool).reshape(-1)
        for key, dst in self._out.items():
            dst[sel] = got[key][sel]


class SensorFrameTransform(_FrameSensor):
    """The pose of frames rigidly attached to bodies, relative to other such frames (the capability of the reference's
    ``newton.sensors.SensorFrameTransform``): the four feet in the base frame.  The model has no sites, so the sensor owns its frames.

    ``frames`` / ``reference_frames``: sequences of ``(body, xform)`` -- an env-local body 0 .. nb-1 (or -1: fixed in the world) and
    the frame's transform in that body, 7 numbers (p, q xyzw) or None for the identity.  ``reference_frames`` has one entry per frame,
    or one entry that serves every frame; None expresses the frames in the world.

    ``eval(state)`` fills ``transforms`` [world, N, 7] = X_reference^-1 X_frame: a resident float32 tensor on a GPU model (one launch
    of frame_sensor_kernel on the model's stream, no allocation, recordable by ``newton_amd.graph.capture``), a float64 numpy array on
    a host model (``frame_sensor_numpy``).  Heterogeneous models: NotImplementedError."""

    def __init__(self, model, frames, reference_frames=None):
        frames = list(frames)
        refs = [] if reference_frames is None else list(reference_frames)
        N = len(frames)
        if N == 0:
            raise ValueError("SensorFrameTransform: no frame")
        if reference_frames is not None and len(refs) not in (1, N):
            raise ValueError(f"SensorFrameTransform: reference_frames must have 1 or {N} entries, got {len(refs)}")
        out_ref = np.full(N, -1) if not refs else N + (np.arange(N) if len(refs) == N else np.zeros(N, np.int64))
        self._setup(model, frames + refs, np.arange(N), out_ref, {"transform": 7})
        self.transforms = self._out["transform"]

    def eval(self, state, world_mask=None):
        """Measure ``state.body_q``.  ``world_mask`` ([world] bool, numpy or torch): the rows of unselected worlds are neither computed
        nor written.  GPU model: one kernel launch on the model's stream (the mask is copied into a resident buffer first)."""
        self._launch(state, None, 0.0, world_mask)


class SensorIMU(_FrameSensor):
    """Accelerometer and gyroscope in body-attached frames (the capability of the reference's ``newton.sensors.SensorIMU``), and on
    request the two proprioceptive terms locomotion policies take in the same frame.  ``frames``: as for SensorFrameTransform.

    ``eval(state, state_prev, dt)`` fills, all in the frame's own axes and all [world, N, 3]:
      ``accelerometer``      the specific force at the frame origin (a frame at rest reads -g: +|g| along the axis that points up);
      ``gyroscope``          the angular velocity of the body;
      ``linear_velocity``    (``want_velocity``) the velocity of the frame origin;
      ``projected_gravity``  (``want_projected_gravity``) the unit gravity direction, zeros in a world without gravity.
    ``gyroscope`` and ``linear_velocity`` are views of ``velocity`` [world, N, 6], not copies.

    The model carries no ``body_qdd``, so the acceleration is the finite difference of the body velocities of two states the caller
    already holds -- the ``state_in`` / ``state_out`` of a ``step`` or ``rollout``: ``state`` is the newer one, ``dt`` the time
    between the two (after ``rollout(s0, s1, n)`` that is n times the substep).  The reading is therefore the MEAN acceleration over
    that interval, not the reference's instantaneous ``body_qdd``; attitude, lever arm and the centripetal term are those of ``state``.
    ``state_prev`` may be ``state`` itself: the centripetal term minus gravity.  Gravity is read from the model at every call: a
    run-time ``set_gravity`` (after the solver's ``notify_model_changed``) takes effect without rebuilding the sensor.

    GPU model: resident float32 tensors, one launch of frame_sensor_kernel on the model's stream per ``eval``, no allocation,
    recordable by ``newton_amd.graph.capture``.  Host model: float64 numpy (``frame_sensor_numpy``).  Heterogeneous models:
    NotImplementedError."""

    def __init__(self, model, frames, want_velocity=False, want_projected_gravity=False):
        frames = list(frames)
        N = len(frames)
        if N == 0:
            raise ValueError("SensorIMU: no frame")
        outputs = {"velocity": 6, "accel": 3}
        if want_projected_gravity:
            outputs["gravity_dir"] = 3
        self._setup(model, frames, np.arange(N), np.full(N, -1), outputs)
        self.velocity, self.accelerometer = self._out["velocity"], self._out["accel"]
        self.gyroscope = self.velocity[..., 3:]
        self.linear_velocity = self.velocity[..., :3] if want_velocity else None
        self.projected_gravity = self._out.get("gravity_dir")

    def eval(self, state, state_prev, dt, world_mask=None):
        """``state``: the newer state, ``state_prev``: the older one, ``dt`` > 0: the time between them.  ``world_mask`` as for
        SensorFrameTransform.eval."""
        if not float(dt) > 0.0 or not np.isfinite(float(dt)):
            raise ValueError(f"SensorIMU.eval: dt must be positive and finite (the time between the two states), got {dt}")
        self._launch(state, state_prev, float(dt), world_mask)
