"""Heterogeneous worlds (newton/_src/sim/model.py:881-900: every per-world entity carries its world index and worlds may differ
in topology; newton/_src/sim/builder.py add_world / add_builder with different sub-builders).

The fused kernels keep one topology per launch (one workgroup = several environments of the SAME template, tables in LDS,
DESIGN.md section 1).  A model whose worlds differ is therefore cut into *world groups*: maximal contiguous runs of worlds with
one topology (``world_runs``), each a valid homogeneous sub-model (``worlds.slice_worlds``) with its own device tables, and
the Newton-shaped objects a caller holds (State / Control / Contacts / CollisionPipeline / the solver classes) become thin
composites over the groups' objects:

* the reference lays every flat array out world-major, so concatenating the groups' arrays in group order IS the global array
  (the same property the per-rank shards use) - getters concatenate, setters split;
* ``collide`` / ``step`` / ``rollout`` issue one launch per group, each group on its own HIP stream forked from and joined
  back into the caller's stream (the groups are independent, and a small group does not fill 256 CUs on its own);
* contact shape ids are translated back to the global model's shape ids, rows are the groups' rows in group order, which is
  the reference's append order over the world-major candidate pairs;
* ``CollisionPipeline(deterministic=True)`` and contact matching work over the whole model: the flat arrays are that raw order
  under one stable sort on (shape0 << 32 | shape1) in global ids, written on the device into persistent arrays after the groups'
  launches join (``nt_contacts_export_sorted_groups``, include/newton_hip_contacts.h), and match indices / the new / broken
  lists are global positions, each group keeping its own matcher -- such a ``collide()`` reads nothing back.

Nothing here touches the arithmetic: a group of k identical worlds steps exactly like a k-world replicated model.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from .worlds import _BODY, _DOF, _JOINT, _SHAPE, slice_worlds


def _torch():
    import torch  # noqa: PLC0415

    return torch


def _world_signature(model, w, spans) -> bytes:
    """Everything the EnvTemplate must find identical between two worlds, relative to the world's own first body / joint /
    coordinate / shape (model.py:881-900 start offsets removed)."""
    (b0, b1), (j0, j1), sh = spans
    jt = np.asarray(model.joint_type[j0:j1], dtype=np.int64)

    def rel(a, off):
        a = np.asarray(a, dtype=np.int64)
        return np.where(a >= 0, a - off, a)

    parts = [np.asarray([b1 - b0, j1 - j0, len(sh)], dtype=np.int64), jt, rel(model.joint_parent[j0:j1], b0),
             rel(model.joint_child[j0:j1], b0), np.asarray(model.joint_dof_dim[j0:j1], dtype=np.int64).ravel(),
             np.asarray(model.joint_q_start[j0:j1], dtype=np.int64) - (int(model.joint_q_start[j0]) if j1 > j0 else 0),
             np.asarray(model.joint_qd_start[j0:j1], dtype=np.int64) - (int(model.joint_qd_start[j0]) if j1 > j0 else 0),
             np.asarray(model.shape_type, dtype=np.int64)[sh], rel(np.asarray(model.shape_body)[sh], b0),
             np.asarray(model.shape_flags, dtype=np.int64)[sh], np.asarray(model.shape_collision_group, dtype=np.int64)[sh],
             np.asarray(model.shape_mesh_count, dtype=np.int64)[sh]]
    return b"|".join(np.ascontiguousarray(p).tobytes() for p in parts)


def world_runs(model) -> list[tuple[int, int]]:
    """Maximal contiguous runs [begin, end) of worlds that share one topology signature."""
    W = model.world_count
    if W <= 1:
        return [(0, max(W, 1))]

    def spans_of(world_arr):
        w = np.asarray(world_arr)
        loc = w[w >= 0]
        first = int(np.flatnonzero(w >= 0)[0]) if len(loc) else 0
        if len(loc) and np.any(np.diff(loc) < 0):
            raise NotImplementedError("worlds must be laid out contiguously (world-major)")
        bounds = first + np.searchsorted(loc, np.arange(W + 1))
        return [(int(bounds[i]), int(bounds[i + 1])) for i in range(W)]

    bs, js = spans_of(model.body_world), spans_of(model.joint_world)
    sw = np.asarray(model.shape_world)
    pairs = np.asarray(model.shape_contact_pairs, dtype=np.int64).reshape(-1, 2)
    n_glob_front = int(np.flatnonzero(sw >= 0)[0]) if np.any(sw >= 0) else 0
    sigs = []
    for w in range(W):
        sh = np.flatnonzero(sw == w)
        sig = _world_signature(model, w, (bs[w], js[w], sh))
        if len(pairs) and len(sh):  # candidate pairs of this world, local ids relative to the world's first shape
            s0 = int(sh[0])
            mine = pairs[(sw[pairs[:, 0]] == w) | (sw[pairs[:, 1]] == w)]
            loc = np.where(sw[mine] >= 0, mine - s0, np.where(mine < n_glob_front, -1 - mine, -1_000_000 - (mine - len(sw))))
            sig += b"|" + np.ascontiguousarray(loc).tobytes()
        sigs.append(sig)
    runs, b = [], 0
    for w in range(1, W + 1):
        if w == W or sigs[w] != sigs[b]:
            runs.append((b, w))
            b = w
    return runs


class WorldGroups:
    """The homogeneous sub-models of a heterogeneous Model, in world order."""

    def __init__(self, model):
        self.model = model
        self.ranges: list[tuple[int, int]] = []
        self.parts = []
        for b, e in world_runs(model):
            part = slice_worlds(model, b, e)
            if part.env is None:  # the signature missed a difference the EnvTemplate insists on: one world per group
                for w in range(b, e):
                    self.ranges.append((w, w + 1))
                    self.parts.append(slice_worlds(model, w, w + 1))
            else:
                self.ranges.append((b, e))
                self.parts.append(part)
        for p in self.parts:
            p._requested_state_attributes = model._requested_state_attributes  # shared sets: later requests reach the groups
            p._requested_contact_attributes = model._requested_contact_attributes
        self._streams = None
        self.concurrent = True  # False: the groups' launches stay on the caller's stream, one after the other

    def __len__(self):
        return len(self.parts)

    _HOST_KEYS = _BODY + _JOINT + _DOF + _SHAPE + ("gravity", "joint_q", "joint_target_q")

    def sync_host(self):
        """The groups hold copies of the global model's host arrays taken when they were cut.  Callers edit the global arrays
        between finalize() and the first State / solver (initial poses, masses, gains): re-slice every group that has not been
        uploaded yet.  Called whenever a composite object is created."""
        for (b, e), part in zip(self.ranges, self.parts):
            if part._dev is not None:
                continue
            fresh = slice_worlds(self.model, b, e)
            if fresh.env is None:
                raise NotImplementedError("heterogeneous worlds: the topology of a world group changed after it was cut")
            for k in self._HOST_KEYS:
                setattr(part, k, getattr(fresh, k))

    def refresh_parameters(self):
        """Host arrays of the global model were edited (masses, gains, materials, gravity ...): copy them into the groups and
        re-upload (solver.py:394-440 notify_model_changed)."""
        for (b, e), part in zip(self.ranges, self.parts):
            fresh = slice_worlds(self.model, b, e)
            if fresh.env is None:
                raise NotImplementedError("heterogeneous worlds: the topology of a world group changed after a runtime edit")
            for k in self._HOST_KEYS:
                setattr(part, k, getattr(fresh, k))
            part.notify_model_changed()

    # -- one launch per group, groups on sibling streams ---------------------------------------------------------------
    def run(self, fn):
        """fn(i, part) for every group.  With more than one group on a real device each group runs on its own stream between
        a fork from and a join into the caller's current stream."""
        torch = _torch()
        dev = self.parts[0].device
        if len(self.parts) == 1 or not self.concurrent or not _real_device(torch):
            for i, p in enumerate(self.parts):
                fn(i, p)
            return
        if self._streams is None:
            self._streams = [torch.cuda.Stream(device=dev) for _ in self.parts]
        cur = torch.cuda.current_stream(dev)
        fork = torch.cuda.Event()
        fork.record(cur)
        for i, (p, s) in enumerate(zip(self.parts, self._streams)):
            s.wait_event(fork)
            with torch.cuda.stream(s):
                fn(i, p)
            done = torch.cuda.Event()
            done.record(s)
            cur.wait_event(done)


def _real_device(torch) -> bool:
    try:
        return bool(torch.cuda.is_available()) and torch.version.hip is not None and torch.cuda.device_count() > 0 and \
            not getattr(torch.cuda, "_newton_emulated", False)
    except Exception:  # noqa: BLE001
        return False


def _cat(values):
    torch = _torch()
    if isinstance(values[0], torch.Tensor):
        return torch.cat(values)
    return np.concatenate(values)


def _split(value, sizes):
    torch = _torch()
    if isinstance(value, torch.Tensor):
        flat = value.reshape(sum(sizes), -1) if value.ndim > 1 else value
        return list(torch.split(flat, sizes))
    a = np.asarray(value)
    a = a.reshape(sum(sizes), -1) if a.ndim > 1 else a
    return np.split(a, np.cumsum(sizes)[:-1])


class _Composite:
    """Concatenating getter / splitting setter over the groups' containers."""

    _PART_CLASS = None

    def __init__(self, model):
        self.model = model
        self.groups: WorldGroups = model.world_groups
        self.groups.sync_host()
        self.parts = [self._PART_CLASS(p) for p in self.groups.parts]
        self.requires_grad = False
        for name, (_ncomp, _slots, default) in self._PART_CLASS._FIELDS.items():
            if default is not None:  # initial values come from the GLOBAL model's arrays as they are now (model.py:1779-1863)
                self._set(name, getattr(model, default))

    def _rows(self, name):
        out = []
        for c in self.parts:
            ncomp, slots, _ = c._FIELDS[name]
            out.append(c.model.env.env_count * getattr(c.model.env, slots))
        return out

    def _get(self, name):
        return _cat([getattr(c, name) for c in self.parts])

    def _set(self, name, value):
        rows = self._rows(name)
        torch = _torch()
        n = value.numel() if isinstance(value, torch.Tensor) else np.asarray(value).size
        ncomp = self.parts[0]._FIELDS[name][0]
        if n != sum(rows) * ncomp:
            raise ValueError(f"{name}: expected {sum(rows) * ncomp} values, got {n}")
        if ncomp > 1 and not isinstance(value, torch.Tensor):
            value = np.asarray(value).reshape(-1, ncomp)
        elif ncomp > 1:
            value = value.reshape(-1, ncomp)
        for c, v in zip(self.parts, _split(value, rows)):
            setattr(c, name, v)


def _split_world_mask(world_mask, groups):
    """Per-group pieces of a world mask of length world_count or the reference's world_count + 1 (trailing global-entity
    slot, core/reset.py:13-60); None stays None."""
    if world_mask is None:
        return None
    sizes = [e - b for b, e in groups.ranges]
    n = int(world_mask.shape[0]) if hasattr(world_mask, "shape") else len(world_mask)
    if n not in (sum(sizes), sum(sizes) + 1):
        raise ValueError(f"'world_mask' length {n} must equal model.world_count + 1 ({sum(sizes) + 1})")
    return _split(world_mask[: sum(sizes)], sizes)


def _composite_property(name):
    return property(lambda self: self._get(name), lambda self, v: self._set(name, v))


@functools.lru_cache(maxsize=1)
def _make_state_classes():
    from .state import Control, State  # noqa: PLC0415

    class GroupedState(_Composite):
        """State of a heterogeneous model (state.py:113-171): same attributes, world-major concatenation of the groups."""

        _PART_CLASS = State
        body_q = _composite_property("body_q")
        body_qd = _composite_property("body_qd")
        body_f = _composite_property("body_f")
        joint_q = _composite_property("joint_q")
        joint_qd = _composite_property("joint_qd")

        def __init__(self, model):
            super().__init__(model)
            self.particle_count = 0

        @property
        def body_parent_f(self):
            vals = [c.body_parent_f for c in self.parts]
            return None if any(v is None for v in vals) else _cat(vals)

        @property
        def body_count(self):
            return self.model.body_count

        @property
        def joint_coord_count(self):
            return self.model.joint_coord_count

        @property
        def joint_dof_count(self):
            return self.model.joint_dof_count

        def clear_forces(self):
            for c in self.parts:
                c.clear_forces()

        def assign(self, other):
            for c, o in zip(self.parts, other.parts):
                c.assign(o)

        def reset(self, source, world_mask=None):
            """State.reset over the groups (solver.py:344-375): the mask is cut at the group boundaries."""
            masks = _split_world_mask(world_mask, self.groups)
            for i, (c, o) in enumerate(zip(self.parts, source.parts)):
                c.reset(o, None if masks is None else masks[i])

    class GroupedControl(_Composite):
        """Control of a heterogeneous model (control.py:31-68)."""

        _PART_CLASS = Control
        joint_f = _composite_property("joint_f")
        joint_target_q = _composite_property("joint_target_q")
        joint_target_qd = _composite_property("joint_target_qd")

        def clear(self, model=None):
            for c in self.parts:
                c.clear(c.model if model is not None else None)

    return GroupedState, GroupedControl


def grouped_contact_order_tables(model, with_rows):
    """Global ranks of the key-ordered export over the world groups (nt_contact_group, include/newton_hip_contacts.h), built once
    per heterogeneous model and row layout: every group's buckets (collide.contact_order_tables of its sub-model) keyed in GLOBAL
    shape ids and enumerated in the raw heterogeneous order -- the analytic tile buckets of every group in group order, then per
    group its convex tile buckets and its row buckets -- ranked by one stable argsort of the keys.  A group's local -> global id map
    is increasing, so its own key order is kept.  `with_rows[g]`: group g's contacts carry the rows of an SDF / vertex leg.
    -> {"bucket_count": B, "bucket_key": [B] key by global bucket id, "groups": [(tile_rank [P*E*2], row_rank [E, K], K)]}"""
    from .collide import _tile_shape_ids, contact_order_tables  # noqa: PLC0415

    key = tuple(bool(r) for r in with_rows)
    cache = model.__dict__.setdefault("_grouped_contact_order", {})
    if key in cache:
        return cache[key]
    first, second, layout, off = [], [], [], 0  # (keys, global bucket ids) per segment of the raw order
    for part, rows in zip(model.world_groups.parts, key):
        t, tab = part.env, contact_order_tables(part)
        gid = np.asarray(part._global_shape_ids, np.int64)
        E, P, npa = t.env_count, t.np, t.np_analytic
        a, b = (gid[x] for x in _tile_shape_ids(t))
        tile_key = np.stack([(a << 32) + b, (b << 32) + a], axis=-1)  # [P, E, 2]
        ids = off + np.arange(P * E * 2).reshape(P, E, 2)
        for (lo, hi), dst in (((0, npa), first), ((npa, P), second)):  # env-major, then pair, then orientation
            dst.append((tile_key[lo:hi].transpose(1, 0, 2).reshape(-1), ids[lo:hi].transpose(1, 0, 2).reshape(-1)))
        K = int(tab["row_keys"]) if rows else 0
        if K:  # (the row keys stay group-local on the device: only their ranks are global)
            rk = np.asarray(tab["row_key"], np.int64)
            second.append((((gid[rk >> 32] << 32) + gid[rk & 0xFFFFFFFF]).reshape(-1), off + P * E * 2 + np.arange(E * K)))
        layout.append((off, P * E * 2, E, K))
        off += P * E * 2 + E * K
    keys = np.concatenate([k for k, _ in first + second] + [np.zeros(0, np.int64)])
    ids = np.concatenate([i for _, i in first + second] + [np.zeros(0, np.int64)])
    rank = np.empty(off, np.int64)
    rank[ids[np.argsort(keys, kind="stable")]] = np.arange(off)
    bucket_key = np.empty(off, np.int64)
    bucket_key[ids] = keys
    out = {"bucket_count": off, "bucket_key": bucket_key,
           "groups": [(rank[o:o + n].astype(np.int32), rank[o + n:o + n + E * K].reshape(E, K).astype(np.int32), K)
                      for o, n, E, K in layout]}
    cache[key] = out
    return out


class GroupedContacts:
    """Contacts of a heterogeneous model (contacts.py:227-277), shape ids of the global model.  Row order = the reference's
    append order: its primitive narrow-phase launch writes first and its MPR / GJK launch second (narrow_phase.py:458-1014,
    1221-1452), each over the world-major candidate pairs - so the analytic rows of every group in group order, then the
    convex rows of every group (a group's own export already has this two-segment shape, nt_contacts_export).

    With sort_by_key (CollisionPipeline(deterministic=True) or contact matching) the flat views are persistent arrays over the whole
    model, written on the device by nt_contacts_export_sorted_groups: that raw order under a stable sort on (shape0 << 32 | shape1)
    in global ids.  The groups' own Contacts stay raw."""

    def __init__(self, model, parts, sort_by_key=False):
        self.model = model
        self.parts = parts
        self.rigid_contact_max = sum(c.rigid_contact_max for c in parts)
        self.soft_contact_max = 0
        from .model import pair_types_analytic  # noqa: PLC0415

        torch = _torch()
        nt_ = int(np.max(model.shape_type)) + 1 if model.shape_count else 1
        tab = np.array([[pair_types_analytic(a, b) for b in range(nt_)] for a in range(nt_)], dtype=bool)
        dev = parts[0]._shape0.device
        self._analytic = torch.from_numpy(tab).to(dev)
        self._types = [torch.as_tensor(np.asarray(c.model.shape_type), dtype=torch.int64, device=dev) for c in parts]
        self._gids = [torch.as_tensor(np.asarray(c.model._global_shape_ids), dtype=torch.int64, device=dev) for c in parts]
        self._seg_cache = (None, None)  # (generations, segments): one host sync per group and per collide, not per field read
        self._row_cache = {}
        self.sort_by_key = bool(sort_by_key)
        if self.sort_by_key:
            self._init_sorted_export()

    # -- key-ordered views over all groups (sort_by_key) ----------------------------------------------------------------------------
    def _init_sorted_export(self):
        """Allocate the global arrays, every group's positions and global-rank tables and the global scan once."""
        from . import _lib  # noqa: PLC0415
        from .collide import contact_order_tables  # noqa: PLC0415

        torch = _torch()
        parts = self.parts
        dev, cap = parts[0]._shape0.device, max(self.rigid_contact_max, 1)
        i32, f32 = torch.int32, torch.float32
        e = {"count": torch.zeros(1, dtype=i32, device=dev),
             "shape0": torch.full((cap,), -1, dtype=i32, device=dev), "shape1": torch.full((cap,), -1, dtype=i32, device=dev)}
        for name in ("point0", "point1", "offset0", "offset1", "normal"):
            e[name] = torch.zeros((cap, 3), dtype=f32, device=dev)
        e["margin0"], e["margin1"] = torch.zeros(cap, dtype=f32, device=dev), torch.zeros(cap, dtype=f32, device=dev)
        if any(c._prop is not None or (c._flat is not None and c._flat.stiffness is not None) for c in parts):
            for name in ("stiffness", "damping", "friction"):
                e[name] = torch.zeros(cap, dtype=f32, device=dev)
        self._export, self._export_gen, self._order_cache, self._force = e, None, None, None
        tab = grouped_contact_order_tables(self.model, [c._flat is not None for c in parts])
        B = tab["bucket_count"]

        def up(a, dtype):
            a = np.ascontiguousarray(a)
            return torch.from_numpy(a if a.size else np.zeros(1, a.dtype)).to(device=dev, dtype=dtype)

        self._order_scratch = (torch.zeros(max(B, 1), dtype=i32, device=dev), torch.zeros(max(B, 1), dtype=i32, device=dev),
                               torch.zeros(B // 1024 + 2, dtype=i32, device=dev))
        self.order_unmatched_rows = torch.zeros(1, dtype=i32, device=dev)  # rows outside every bucket (stays 0)
        o = _lib.nt_contact_order()
        o.bucket_count = B
        o.bucket_fill, o.bucket_start, o.block_sum = (x.data_ptr() for x in self._order_scratch)
        self._order = o
        so = _lib.nt_sorted_contacts()
        so.cap = cap
        for name, v in e.items():
            setattr(so, name, v.data_ptr())
        self._sorted = so
        self._group_tabs = []  # per group: (nt_contact_order, slot_flat, row_flat, row capacity, tensors kept alive)
        for c, (tile_rank, row_rank, K) in zip(parts, tab["groups"]):
            t, ptab = c.model.env, contact_order_tables(c.model)
            row_cap = c._flat.capacity if c._flat is not None else 0
            slot_flat = torch.full((max(c._slots, 1), t.env_stride), -1, dtype=i32, device=dev)
            row_flat = torch.full((max(row_cap, 1),), -1, dtype=i32, device=dev)
            keep = (up(ptab["tile_shape0"], i32), up(tile_rank, i32), up(ptab["row_key"], torch.int64), up(row_rank, i32),
                    up(c.model._global_shape_ids, i32), torch.zeros(max(row_cap, 1), dtype=i32, device=dev),
                    torch.zeros(max(row_cap, 1), dtype=i32, device=dev))
            go = _lib.nt_contact_order()
            go.bucket_count, go.row_keys = 2 * t.env_count * t.np + t.env_count * K, K
            go.tile_shape0, go.tile_rank, go.row_key, go.row_rank = (x.data_ptr() for x in keep[:4])
            go.row_bucket, go.row_sub = keep[5].data_ptr(), keep[6].data_ptr()
            go.row_unmatched = self.order_unmatched_rows.data_ptr()
            self._group_tabs.append((go, slot_flat, row_flat, row_cap, keep))

    def _group_descs(self, matchers=None):
        """-> (nt_contact_group array, what it points to); `matchers`: the groups' ContactMatcher (report / save)."""
        from . import _lib  # noqa: PLC0415

        n = len(self.parts)
        arr, keep = (_lib.nt_contact_group * n)(), []
        for i, (c, (go, slot_flat, row_flat, row_cap, tabs)) in enumerate(zip(self.parts, self._group_tabs)):
            d = c._desc()
            keep.append(d)
            g = arr[i]
            g.m, g.c, g.o = C.pointer(c.model.device_model().desc), C.pointer(d), C.pointer(go)
            g.shape_id, g.row_capacity = tabs[4].data_ptr(), row_cap
            g.slot_flat, g.row_flat = slot_flat.data_ptr(), row_flat.data_ptr()
            if matchers is not None:
                r = matchers[i]._report_desc()
                keep.append(r)
                g.r = C.pointer(r)
        return arr, keep

    def _export_sorted(self):
        """(Re)write the global key-ordered views from every group's slots and rows: device work only, no host read."""
        from . import _lib  # noqa: PLC0415

        dm = self.parts[0].model.device_model()
        groups, _keep = self._group_descs()
        _lib.check(dm.lib.nt_contacts_export_sorted_groups(len(self.parts), groups, C.byref(self._order), C.byref(self._sorted),
                                                           dm.stream()), "nt_contacts_export_sorted_groups")
        self._export_gen = tuple(c._generation for c in self.parts)
        return self._export

    def _exported(self):
        """The global views, re-exported when a group's contacts changed since (a rollout, a graph replay, clear())."""
        if self._export_gen == tuple(c._generation for c in self.parts):
            return self._export
        return self._export_sorted()

    def export_order(self):
        """Permutation from the raw heterogeneous order to the order of the rigid_contact_* arrays (None = identity).  Non-trivial
        only with CollisionPipeline(deterministic=True).  (A query: it reads the count back.)"""
        if not self.sort_by_key:
            return None
        e = self._exported()
        if self._order_cache is not None and self._order_cache[1] == self._export_gen:
            return self._order_cache[0]
        torch = _torch()
        n = min(int(e["count"].item()), max(self.rigid_contact_max, 1))
        order = None
        if n > 1:  # (the raw index of every slot / row, scattered to its sorted position)
            order = torch.empty(n, dtype=torch.int64, device=e["count"].device)
            first, second = [], []
            for c, (_go, slot_flat, row_flat, row_cap, _k) in zip(self.parts, self._group_tabs):
                t = c.model.env
                E, nas = t.env_count, t.np_analytic * t.cpp
                first.append(slot_flat[:nas, :E].T.reshape(-1))
                second.append(slot_flat[nas:c._slots, :E].T.reshape(-1))
                if row_cap:
                    second.append(row_flat[:row_cap])
            base = 0
            for pos in first + second:
                pos = pos[pos >= 0].to(torch.int64)
                order[pos] = base + torch.arange(pos.numel(), device=pos.device)
                base += int(pos.numel())
        self._order_cache = (order, self._export_gen)
        return order

    def _sorted_view(self, name):
        return self._exported()[name[len("rigid_contact_"):]]

    def _segments(self):
        """Per group (row count, analytic row count) of its current export."""
        torch = _torch()
        gen = tuple(c._generation for c in self.parts)
        if self._seg_cache[0] == gen:
            return self._seg_cache[1]
        seg = []
        for c, ty in zip(self.parts, self._types):
            n = min(int(c.rigid_contact_count.cpu().numpy()[0]), c.rigid_contact_max)
            a, b = c.rigid_contact_shape0[:n].to(torch.int64), c.rigid_contact_shape1[:n].to(torch.int64)
            na = int(self._analytic[ty[a], ty[b]].sum().item()) if n and not c.sort_by_key else n
            seg.append((n, na))
        self._seg_cache = (gen, seg)
        self._row_cache = {}
        return seg

    @property
    def rigid_contact_count(self):
        if self.sort_by_key:
            return self._exported()["count"]
        torch = _torch()
        return torch.stack([c.rigid_contact_count.reshape(-1)[0] for c in self.parts]).sum().reshape(1).to(torch.int32)

    def _rows(self, get, translate=False, key=None):
        torch = _torch()
        seg = self._segments()
        if key is not None and key in self._row_cache:
            return self._row_cache[key]
        first, second = [], []
        for c, ids, (n, na) in zip(self.parts, self._gids, seg):
            v = get(c)[:n]
            if translate:
                v = ids[v.to(torch.int64)].to(torch.int32)
            first.append(v[:na])
            second.append(v[na:])
        out = torch.cat(first + second)
        if key is not None:
            self._row_cache[key] = out
        return out

    @staticmethod
    def _field(name, translate=False):
        return property(lambda self: self._sorted_view(name) if self.sort_by_key else
                        self._rows(lambda c: getattr(c, name), translate, key=name))

    @staticmethod
    def _sorted_field(name):
        """per-contact overrides of the key-ordered views (None unless a group's contacts carry them)"""
        def get(self):
            if not self.sort_by_key:
                raise AttributeError(name)
            return self._exported().get(name[len("rigid_contact_"):])

        return property(get)

    @property
    def rigid_contact_count_per_env(self):
        return _cat([c.rigid_contact_count_per_env for c in self.parts])

    @property
    def force(self):
        if any(c.force is None for c in self.parts):
            return None
        if not self.sort_by_key:
            return self._rows(lambda c: c.force)
        # the groups' forces in the raw order, permuted like the key-ordered views: force[i] is the force of contact i
        raw, order = self._rows(lambda c: c.force), self.export_order()
        if self._force is None:
            torch = _torch()
            self._force = torch.zeros((max(self.rigid_contact_max, 1), 6), dtype=raw.dtype, device=raw.device)
        n = int(raw.shape[0])
        self._force.zero_()
        self._force[:n] = raw if order is None else raw[order]
        return self._force

    def clear(self):
        for c in self.parts:
            c.clear()

    def invalidate_views(self):
        for c in self.parts:
            c.invalidate_views()


GroupedContacts.rigid_contact_shape0 = GroupedContacts._field("rigid_contact_shape0", True)
GroupedContacts.rigid_contact_shape1 = GroupedContacts._field("rigid_contact_shape1", True)
for _n in ("point0", "point1", "offset0", "offset1", "normal", "margin0", "margin1"):
    setattr(GroupedContacts, "rigid_contact_" + _n, GroupedContacts._field("rigid_contact_" + _n))
for _n in ("stiffness", "damping", "friction"):
    setattr(GroupedContacts, "rigid_contact_" + _n, GroupedContacts._sorted_field("rigid_contact_" + _n))


class GroupedCollisionPipeline:
    """CollisionPipeline over the world groups (collide.py:1765-2207: one collide() per frame on the whole model).

    Every group runs a default pipeline of its own (raw contacts).  deterministic=True and contact matching are served over the
    whole model: each group keeps its own ContactMatcher (histories, sticky replay; a pair never spans two groups), and after the
    groups' launches have joined the caller's stream the key-ordered export, the report and the save run once over all groups
    (nt_contacts_export_sorted_groups / _match_report_groups / _order_save_groups): match indices are global positions."""

    def __init__(self, cls, model, **kwargs):
        from .collide import ContactMatcher, check_matching_options  # noqa: PLC0415

        self.model = model
        self.groups: WorldGroups = model.world_groups
        if kwargs.get("rigid_contact_max") is not None:
            raise NotImplementedError("heterogeneous worlds: rigid_contact_max is derived per world group")
        deterministic = bool(kwargs.pop("deterministic", False))
        mode, report = kwargs.pop("contact_matching", "disabled"), bool(kwargs.pop("contact_report", False))
        pos = kwargs.pop("contact_matching_pos_threshold", 0.0005)
        dot = kwargs.pop("contact_matching_normal_dot_threshold", 0.995)
        check_matching_options(mode, pos, dot, report)
        self.groups.sync_host()
        self.parts = [cls(p, **kwargs) for p in self.groups.parts]
        if mode != "disabled" and any(p._sdf_leg is not None and p._sdf_leg.has_hydro_pairs for p in self.parts):
            # the reference matcher does not cover hydroelastic contacts either (contact_match.py:497-501)
            raise NotImplementedError("contact_matching is not supported for hydroelastic contact pairs")
        self.contact_matching, self.contact_report = mode, report
        self.deterministic = deterministic or mode != "disabled"
        self._matchers, self._prev_count = None, None
        if mode != "disabled":
            torch = _torch()
            self._matchers = [ContactMatcher(p.model, pos, dot, sticky=mode == "sticky", sdf_leg=p._sdf_leg) for p in self.parts]
            self._prev_count = torch.zeros(1, dtype=torch.int32, device=self.parts[0].dm.device)  # the previous frame's global count

    @property
    def rigid_contact_max(self):
        return sum(p.rigid_contact_max for p in self.parts)

    def contacts(self, **kwargs):
        c = GroupedContacts(self.model, [p.contacts(**kwargs) for p in self.parts], sort_by_key=self.deterministic)
        c._contact_matching_mode = self.contact_matching
        if self._matchers is not None:
            from .collide import add_matching_buffers  # noqa: PLC0415

            add_matching_buffers(c, c.rigid_contact_max, self.contact_report, self.parts[0].dm.device)
        return c

    def reset_contact_matching(self, world_mask=None):
        if self._matchers is None:
            if world_mask is not None:
                _split_world_mask(world_mask, self.groups)
            raise ValueError('reset_contact_matching requires contact_matching != "disabled"')
        masks = _split_world_mask(world_mask, self.groups)
        for i, mt in enumerate(self._matchers):
            mt.reset(None if masks is None else masks[i])
        if world_mask is None:
            self._prev_count.zero_()

    def collide(self, state, contacts, **kwargs):
        if not self.deterministic:
            self.groups.run(lambda i, _p: self.parts[i].collide(state.parts[i], contacts.parts[i], **kwargs))
            return
        if not getattr(contacts, "sort_by_key", False):
            raise ValueError("CollisionPipeline(deterministic=True) needs its own Contacts: use pipeline.contacts()")
        mts = self._matchers
        if mts is not None and getattr(contacts, "rigid_contact_match_index", None) is None:
            raise ValueError("CollisionPipeline has contact_matching enabled but the Contacts buffer was created without it. "
                             "Use pipeline.contacts() to create a compatible buffer.")

        def go(i, _p):  # per group, on its stream: collide, then its matcher (previous SLOT / ROW per contact) [+ sticky replay]
            s, c = state.parts[i], contacts.parts[i]
            self.parts[i].collide(s, c, **kwargs)
            if mts is not None:
                mts[i]._match_kernels(s, c)
                if mts[i].sticky:
                    mts[i].replay_matched(s, c)

        self.groups.run(go)
        # joined: the global views (after the replay: the geometry the solver sees), then the report and the save over all groups
        contacts._export_sorted()
        if mts is not None:
            self._report_and_save(state, contacts)

    def _report_and_save(self, state, contacts):
        from . import _lib  # noqa: PLC0415

        mts = self._matchers
        dm = self.parts[0].dm
        r = _lib.nt_contact_report()
        r.prev_count, r.match_index = self._prev_count.data_ptr(), contacts.rigid_contact_match_index.data_ptr()
        if contacts._report_buffers is not None:  # (new_indices, new_count, broken_indices, broken_count, flag, offset, block_sum)
            (r.new_indices, r.new_count, r.broken_indices, r.broken_count, r.flag, r.offset,
             r.block_sum) = (x.data_ptr() for x in contacts._report_buffers)
        groups, _keep = contacts._group_descs(mts)
        n = len(self.parts)
        _lib.check(dm.lib.nt_contacts_match_report_groups(n, groups, C.byref(contacts._sorted), C.byref(r), dm.stream()),
                   "nt_contacts_match_report_groups")
        for i, mt in enumerate(mts):  # (the report read the histories of the previous frame: save them only now)
            mt._save_history(state.parts[i], contacts.parts[i])
        _lib.check(dm.lib.nt_contacts_order_save_groups(n, groups, C.byref(contacts._sorted), C.byref(r), dm.stream()),
                   "nt_contacts_order_save_groups")


class GroupedSolver:
    """One solver instance per world group behind the reference's solver surface (solvers/solver.py:190-450)."""

    def __init__(self, cls, model, *args, **kwargs):
        self.model = model
        self.groups: WorldGroups = model.world_groups
        self.groups.sync_host()
        self.parts = [cls(p, *args, **kwargs) for p in self.groups.parts]

    @property
    def device(self):
        return self.model.device

    @staticmethod
    def _part(obj, i):
        return None if obj is None else obj.parts[i]

    def step(self, state_in, state_out, control, contacts, dt):
        self.groups.run(lambda i, _p: self.parts[i].step(state_in.parts[i], state_out.parts[i], self._part(control, i),
                                                         self._part(contacts, i), dt))

    def rollout(self, state_0, state_1, control, contacts, dt, substeps, **kwargs):
        """substeps x {clear_forces, collide, step} per group in one launch each; returns the state holding the result."""
        res = [None] * len(self.parts)

        def go(i, _p):
            res[i] = self.parts[i].rollout(state_0.parts[i], state_1.parts[i], self._part(control, i),
                                           self._part(contacts, i), dt, substeps, **kwargs)

        self.groups.run(go)
        return state_1 if res[0] is state_1.parts[0] else state_0

    def update_contacts(self, contacts, state=None):
        for i, s in enumerate(self.parts):
            s.update_contacts(contacts.parts[i], self._part(state, i))

    def notify_model_changed(self, flags):
        self.groups.refresh_parameters()
        for s in self.parts:
            s.notify_model_changed(flags)

    def reset(self, state, world_mask=None, flags=None):
        masks = _split_world_mask(world_mask, self.groups)
        for i, s in enumerate(self.parts):
            s.reset(state.parts[i], None if masks is None else masks[i], flags)
