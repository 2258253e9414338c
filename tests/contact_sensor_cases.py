"""Synthetic inputs and references shared by tests/test_contact_sensor_host.py, test_contact_sensor_emu.py and
test_gpu_contact_sensor.py (test infrastructure).  nt_contact_sensor (include/newton_hip_contacts.h) is fed directly: shape0 / shape1
[slots][ES], impulse [6][slots][ES], optional rows with row_start, on a tiny model whose only role is ns, ng, nb and the shape ids --
the slot count of the synthetic arrays is written over np * cpp in a copy of the model descriptor, so many slots need no real pairs.

EXACT set: impulse components are small integers times 2^-10 and dt = 2^-7, so every product and every partial sum is exact in float32:
the float64 reference (sensors.contact_sensor_numpy over the flat arrays) has to be met bit for bit whatever the order.
ORDER set: every (sensing object, counterpart) cell gets the contributions 1, 2^24, 1, -2^24 (times a power of two) spread over the
slots and rows of the world.  Their float32 sequential sum in the contracted order is 0, the float64 sum 2, the reversed order 2, a
pairwise order 1 (times the power of two): the expected value is the sequential one, and `order_alternatives` shows that it differs from
the others."""
import ctypes as C
import os
import re

import numpy as np

import newton_amd as nt
from newton_amd import _lib as L
from newton_amd import sensors

DT = 2.0 ** -7
N_WORLDS = 37
POISON = 7.0
CS_THREADS, CS_MAX_WPB, CS_ITEMS = 256, 16, 512
# (S, C, include_total): 4, 20, 64, 65, 256 and 289 output cells per world -- 16 / 8 / 4 / 2 / 1 worlds per workgroup, the last with
# more cells than a world has lanes; from (8, 15) on the sensing and counterpart sets overlap
SHAPES = {"cells4": (2, 1, True), "cells20": (4, 4, True), "cells64": (8, 7, True), "cells65": (5, 12, True), "cells256": (16, 16, False),
          "cells289": (17, 16, True)}
_MODELS = {}

# worlds, shape of the output, slots of the synthetic arrays, rows
EXACT_CASES = {
    "1_world_cells4": (1, "cells4", 40, "ragged"),
    "5_worlds_cells20_no_rows": (5, "cells20", 70, None),          # 70 slots > 64 entries per round at 8 worlds per workgroup
    "5_worlds_cells289": (5, "cells289", 600, 30),                  # two passes over 630 entries, two rounds each
    "37_worlds_cells4": (37, "cells4", 100, "ragged"),              # 100 slots > 16 lanes per world, 32 entries per round
    "37_worlds_cells64": (37, "cells64", 9, "ragged"),              # fewer slots than a round, rows in some worlds only
    "37_worlds_cells65_no_slots": (37, "cells65", 0, "ragged"),     # rows only
    "5_worlds_cells256": (5, "cells256", 530, None),                # one world per workgroup, 530 slots > 512 entries per round
}
# worlds, shape of the output, slots, rows, every designed cell shows the order (sets that do not overlap)
ORDER_CASES = {
    "5_worlds_cells20": (5, "cells20", 70, "ragged", True),
    "37_worlds_cells64": (37, "cells64", 230, "ragged", True),
    "5_worlds_cells65_no_rows": (5, "cells65", 250, None, True),
    "1_world_cells289": (1, "cells289", 1000, 200, False),
}


def kernel_constants():
    """The launch constants as the kernel source states them."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "newton_amd", "csrc", "nt_match.hip")).read()
    vals = tuple(int(re.search(rf"constexpr int {k} = (\d+);", src).group(1)) for k in ("CS_THREADS", "CS_MAX_WPB", "CS_ITEMS"))
    assert "while (wpb > 1 && wpb * cells > CS_THREADS) wpb /= 2;" in src
    return vals


def launch_shape(cells):
    """(worlds per workgroup, lanes per world, entries of a world per round) nt_contact_sensor chooses."""
    wpb = CS_MAX_WPB
    while wpb > 1 and wpb * cells > CS_THREADS:
        wpb //= 2
    return wpb, CS_THREADS // wpb, CS_ITEMS // wpb


def sensor_model(world_count, device=None):
    """20 bodies per world far from one another, body 0 carrying two shapes (ns = 21), a ground plane and one static sphere (ng = 2)."""
    key = (world_count, device)
    if key not in _MODELS:
        env = nt.ModelBuilder()
        for k in range(20):
            b = env.add_body(xform=[1.0 * (k % 5), 1.0 * (k // 5), 0.5, 0.0, 0.0, 0.0, 1.0])
            env.add_shape_sphere(b, radius=0.1)
            if k == 0:
                env.add_shape_box(b, xform=[0.0, 0.0, 0.15, 0.0, 0.0, 0.0, 1.0], hx=0.05, hy=0.05, hz=0.05)
        scene = nt.ModelBuilder()
        scene.replicate(env, world_count)
        scene.add_ground_plane()
        scene.add_shape_sphere(-1, xform=[-3.0, -3.0, 1.0, 0.0, 0.0, 0.0, 1.0], radius=0.1)
        _MODELS[key] = scene.finalize(device=device)
    return _MODELS[key]


def shape_id(t, world, slot):
    return int(t.shape_local0 + world * t.ns + slot) if slot < t.ns else int(np.asarray(t.gshape_id)[slot - t.ns])


class Case:
    """One synthetic input.  Slot arrays in the device layout, rows in Newton's flat layout; `flat()` is what the public export would
    show (every world's live slots in ascending index, then the live rows; force = impulse * (1.0f / dt))."""

    def __init__(self, model, nslot, S, C, include_total, rows):
        t = self.t = model.env
        self.model, self.E, self.ES, self.nslot = model, t.env_count, t.env_stride, int(nslot)
        self.S, self.C, self.tot = S, C, int(bool(include_total))
        self.cols = self.tot + C
        n = t.ns + t.ng
        assert S <= n and C <= n
        self.slot_sensing = np.full(n, -1, np.int32)
        self.slot_sensing[:S] = np.arange(S)  # (slots 0 and 1 are the two shapes of body 0: separate sensing objects here)
        self.slot_counterpart = np.full(n, -1, np.int32)
        if C:
            self.slot_counterpart[n - C:] = np.arange(C)
        if S + 3 <= n - C:  # room between the two sets: sensing object 0 and counterpart 0 become sets of several slots
            self.slot_sensing[S:S + 2] = 0
            if C:
                self.slot_counterpart[n - C - 1] = 0
        self.shape0 = np.full((max(self.nslot, 1), self.ES), -1, np.int32)
        self.shape1 = np.full((max(self.nslot, 1), self.ES), -1, np.int32)
        self.impulse = np.zeros((6, max(self.nslot, 1), self.ES), np.float32)
        self.rows = rows is not None
        if self.rows:
            counts = np.asarray(rows, np.int64).reshape(self.E)
            self.row_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
            self.row_capacity = int(self.row_start[-1]) + 3
            self.rshape0 = np.full(self.row_capacity, -1, np.int32)
            self.rshape1 = np.full(self.row_capacity, -1, np.int32)
            self.rimpulse = np.zeros((self.row_capacity, 6), np.float32)
        self.dt = DT

    def entries(self, w):
        """Number of entry positions of world w: its slots, then its rows."""
        return self.nslot + (int(self.row_start[w + 1] - self.row_start[w]) if self.rows else 0)

    def put(self, w, pos, s0, s1, imp):
        if pos < self.nslot:
            self.shape0[pos, w], self.shape1[pos, w], self.impulse[:, pos, w] = s0, s1, imp
        else:
            r = int(self.row_start[w]) + pos - self.nslot
            assert r < self.row_start[w + 1]
            self.rshape0[r], self.rshape1[r], self.rimpulse[r] = s0, s1, imp

    def flat(self):
        inv_dt = np.float32(1.0) / np.float32(self.dt)
        s0, s1, f = [], [], []
        for w in range(self.E):
            live = np.flatnonzero(self.shape0[:self.nslot, w] >= 0)
            s0.append(self.shape0[live, w]); s1.append(self.shape1[live, w]); f.append(self.impulse[:, live, w].T * inv_dt)
        if self.rows:
            n = int(self.row_start[-1])
            live = np.flatnonzero(self.rshape0[:n] != self.rshape1[:n])
            s0.append(self.rshape0[live]); s1.append(self.rshape1[live]); f.append(self.rimpulse[live] * inv_dt)
        s0, s1, f = np.concatenate(s0), np.concatenate(s1), np.concatenate(f).astype(np.float32)
        return np.array([len(s0)], np.int32), s0.astype(np.int32), s1.astype(np.int32), f

    def reference(self, dtype=np.float64, world_mask=None):
        count, s0, s1, f = self.flat()
        return sensors.contact_sensor_numpy(self.model, count, s0, s1, f, self.slot_sensing, self.slot_counterpart, self.S, self.C, self.tot,
                                            world_mask=world_mask, dtype=dtype)


def _row_counts(E, rows, rng):
    if rows is None:
        return None
    if rows == "ragged":  # (zero rows in some worlds: empty row_start ranges)
        c = rng.integers(0, 40, size=E)
        c[::4] = 0
        return c
    return np.full(E, int(rows))


def exact_case(model, nslot, S, C, include_total, rows=None, seed=0, replicated=False):
    """Random contacts among the shapes of every world: live slots / rows, unused slots and inert rows (with garbage impulses), shapes on
    either side, the same sensing object on both sides now and then."""
    rng = np.random.default_rng(seed)
    t = model.env
    c = Case(model, nslot, S, C, include_total, _row_counts(t.env_count, rows, rng))
    n = t.ns + t.ng
    for w in range(c.E):
        wr = np.random.default_rng(seed) if replicated else rng  # (replicated: the same draws in every world)
        for pos in range(c.entries(w)):
            imp = wr.integers(-40, 41, size=6).astype(np.float32) * np.float32(2.0 ** -10)
            if wr.random() < 0.35:
                c.put(w, pos, -1, -1, imp)  # unused slot / inert row
                continue
            a, b = wr.choice(n, size=2, replace=False)
            c.put(w, pos, shape_id(t, w, a), shape_id(t, w, b), imp)
    return c


ORDER_VALUES = (1.0, 2.0 ** 24, 1.0, -(2.0 ** 24))


def order_case(model, nslot, S, C, include_total, rows=None, seed=0):
    """Cell (s, c) of every world: four contacts between the shape of sensing object s and the first shape of counterpart c, contact i
    in the i-th quarter of the world's used entry positions, contributing ORDER_VALUES[i] * 2^(q % 5 - 2) in component q % 3 (q = s * C
    + c); the sensing shape is shape0 or shape1 in turn (the impulse then carries the opposite sign)."""
    assert C > 0
    rng = np.random.default_rng(seed)
    t = model.env
    c = Case(model, nslot, S, C, include_total, _row_counts(t.env_count, rows, rng))
    ncell = S * C
    cp_slot = [int(np.flatnonzero(c.slot_counterpart == k)[0]) for k in range(C)]
    for w in range(c.E):
        assert c.entries(w) >= 4 * ncell
        positions = np.sort(rng.choice(c.entries(w), size=4 * ncell, replace=False))
        for i in range(4):
            order = rng.permutation(ncell)
            for q in range(ncell):
                s, k = divmod(q, C)
                if cp_slot[k] == s:  # (overlapping sets: a shape has no contact with itself)
                    continue
                v = np.zeros(6, np.float32)
                v[q % 3] = np.float32(ORDER_VALUES[i] * 2.0 ** (q % 5 - 2) * DT)
                v[3:] = 0.25  # (the torque part is not read)
                ids = shape_id(t, w, s), shape_id(t, w, cp_slot[k])
                if (q + w) % 2:
                    c.put(w, int(positions[i * ncell + order[q]]), ids[1], ids[0], -v)
                else:
                    c.put(w, int(positions[i * ncell + order[q]]), ids[0], ids[1], v)
    return c


def cell_lists(t, count, s0, s1, f, slot_sensing, slot_counterpart, include_total):
    """{(world, sensing object, column): the float32 contributions in flat order} over Newton's flat arrays -- the contract restated
    independently of sensors.contact_sensor_numpy."""
    lists = {}
    lo, ns, E = t.shape_local0, t.ns, t.env_count
    g = {int(x): ns + k for k, x in enumerate(np.asarray(t.gshape_id)[:t.ng])}
    tot = int(bool(include_total))

    def loc(i):
        return ((i - lo) // ns, (i - lo) % ns) if lo <= i < lo + E * ns else (-1, g.get(i, -1))

    for i in range(int(np.asarray(count).reshape(-1)[0])):
        if s0[i] < 0 or s0[i] == s1[i]:
            continue
        (wa, sa), (wb, sb) = loc(int(s0[i])), loc(int(s1[i]))
        w = wa if wa >= 0 else wb
        for mine, other, sign in ((sa, sb, 1.0), (sb, sa, -1.0)):
            k = slot_sensing[mine] if mine >= 0 else -1
            if k < 0:
                continue
            cp = slot_counterpart[other] if other >= 0 else -1
            if tot:
                lists.setdefault((w, k, 0), []).append(np.float32(sign) * np.asarray(f[i, :3], np.float32))
            if cp >= 0:
                lists.setdefault((w, k, tot + cp), []).append(np.float32(sign) * np.asarray(f[i, :3], np.float32))
    return lists


def order_alternatives(case):
    """Per world and cell the contributions in the contracted order -> their sums: float32 sequential, float64, float32 reversed,
    float32 pairwise ((a0 + a1) + (a2 + a3) ...).  [E, S, cols, 3] each."""
    lists = cell_lists(case.t, *case.flat(), case.slot_sensing, case.slot_counterpart, case.tot)
    shape = (case.E, case.S, case.cols, 3)
    seq, f64, rev, pair = np.zeros(shape, np.float32), np.zeros(shape), np.zeros(shape, np.float32), np.zeros(shape, np.float32)

    def seq32(items):
        acc = np.zeros(3, np.float32)
        for x in items:
            acc = acc + x
        return acc

    def pairwise(items):
        items = list(items)
        while len(items) > 1:
            items = [items[j] + items[j + 1] if j + 1 < len(items) else items[j] for j in range(0, len(items), 2)]
        return items[0]

    for key, items in lists.items():
        seq[key], rev[key], pair[key] = seq32(items), seq32(items[::-1]), pairwise(items)
        f64[key] = np.sum(np.asarray(items, np.float64), axis=0)
    return seq, f64, rev, pair


# ---------------------------------------------------------------------------------------------------------------------------------
# the entry point over host arrays (the emulator) or device tensors (the GPU test uploads the same arrays)
# ---------------------------------------------------------------------------------------------------------------------------------
def _ptr(a):
    return a.ctypes.data_as(C.c_void_p).value


class HostCall:
    """nt_contacts + nt_contact_sensor_args over `case`; `upload` maps a host array to what the callee reads (identity on the emulator, a
    device tensor on the GPU, which must then provide `ptr`)."""

    def __init__(self, case, model_desc, upload=None, ptr=_ptr, mask=None):
        self.case, self.keep = case, []
        up = (lambda a: a) if upload is None else upload

        def dev(a):
            x = up(np.ascontiguousarray(a))
            self.keep.append(x)
            return x

        self.ptr = ptr
        self.desc = type(model_desc).from_buffer_copy(model_desc)
        self.desc.np, self.desc.cpp = case.nslot, 1  # (the kernel reads only their product)
        c = self.contacts = L.nt_contacts()
        c.shape0, c.shape1 = ptr(dev(case.shape0)), ptr(dev(case.shape1))
        self.impulse = dev(case.impulse)
        a = self.args = L.nt_contact_sensor_args()
        a.sensing_count, a.counterpart_count, a.include_total = case.S, case.C, case.tot
        if case.rows:
            c.flat.row_start, c.flat.shape0, c.flat.shape1 = ptr(dev(case.row_start)), ptr(dev(case.rshape0)), ptr(dev(case.rshape1))
            c.flat.impulse = ptr(dev(case.rimpulse))
            a.row_capacity = case.row_capacity
        a.slot_sensing, a.slot_counterpart = ptr(dev(case.slot_sensing)), ptr(dev(case.slot_counterpart))
        self.host_tables = (case.slot_sensing.copy(), case.slot_counterpart.copy())
        a.slot_sensing_host, a.slot_counterpart_host = _ptr(self.host_tables[0]), _ptr(self.host_tables[1])
        self.net_force = dev(np.full((case.E, case.S, case.cols, 3), POISON, np.float32))
        a.net_force = ptr(self.net_force)
        if mask is not None:
            self.mask = dev(np.asarray(mask).astype(np.uint8))
            a.world_mask = ptr(self.mask)

    def run(self, lib, stream=None, dt=None):
        return lib.nt_contact_sensor(C.byref(self.desc), C.byref(self.contacts), self.ptr(self.impulse), float(self.case.dt if dt is None else dt),
                                     C.byref(self.args), stream)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_exact(case, got, mask=None):
    """`got` against the float64 reference, bit for bit; masked rows keep the poison."""
    ref = case.reference(world_mask=mask)
    sel = np.ones(case.E, bool) if mask is None else np.asarray(mask, bool)
    assert np.any(ref[sel] != 0.0)
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)  # (the exact set: the float64 sums are float32 numbers)
    assert np.array_equal(bits(got[sel]), bits(ref[sel].astype(np.float32)))
    assert np.all(got[~sel] == POISON)


def check_order(case, got, designed_all=True):
    """`got` against the float32 sequential sum in the contracted order; that sum differs from the float64, reversed and pairwise ones in
    every designed cell (sets that do not overlap) or in some (overlapping sets: a contact then feeds several cells)."""
    seq, f64, rev, pair = order_alternatives(case)
    assert np.array_equal(bits(seq), bits(case.reference(dtype=np.float32)))  # (the product's own host path, asked for float32)
    differs = np.zeros((case.E, case.S, case.C), bool)
    for q in range(case.S * case.C):
        s, k = divmod(q, case.C)
        col, comp = case.tot + k, q % 3
        differs[:, s, k] = ((seq[:, s, col, comp] != f64[:, s, col, comp]) & (seq[:, s, col, comp] != rev[:, s, col, comp]) &
                            (seq[:, s, col, comp] != pair[:, s, col, comp]))
    assert np.all(differs) if designed_all else np.mean(differs) > 0.5
    assert np.array_equal(bits(got), bits(seq))
