"""Inputs, frame tables, the reference and the tolerance shared by tests/test_frame_sensor_host.py, test_frame_sensor_emu.py and
test_gpu_frame_sensor.py (test infrastructure).  nt_frame_sensor (include/newton_hip_kinematics.h) is fed directly: a small replicated
model of four free bodies (two of them with a COM away from the body origin), seeded random float32 body_q / body_qd / previous
body_qd, and a frame table that mixes identity and random local transforms, a frame fixed in the world, two frames on one body, a frame
referenced to a frame later in the table and a frame referenced to itself.  Every world but the first has a gravity row of its own;
world 3 has none (projected gravity 0).

Tolerance (derived, not measured): the kernel evaluates the contract in float32, the reference (sensors.frame_sensor_numpy) in float64
on the same float32 inputs.  An output element may differ by 64 * 2^-24 * scale, scale being the sum of the magnitudes of the terms the
contract adds to form that element, as the reference reports it (``with_scale``):
    translation   |x| + |x_ref|                         quaternion components, unit directions   1
    velocity      |v_com| + |w| |r|   (the angular half: its own |w| where that is smaller -- nothing is added to it)
    accel         (|v_com| + |v_com_prev| + (|w| + |w_prev|) |r|) / dt + |w|^2 |r| + |g|
The longest chain (accel: two differences, two divisions, three cross products, three additions, the rotation into the frame) is
about 20 roundings of at most 2^-24 each relative to a partial result no larger than scale; 64 leaves a margin of three.  The
float64 reference's own error is 2^-29 of that.  `check` prints the largest error / (2^-24 scale) per output: above 8 something other
than rounding is going on.  One figure is above 8 by construction of the scale, not of the kernel: the angular half of `velocity` is
held to the linear half's scale where that is the smaller one, and that scale has no term for w itself -- a frame on the COM of a body
that spins fast and moves slowly (|w| = 5.8, |v_com| = 0.71 in the 37-world, 70-row case) reads 11.4 against it and 1.4 against |w|."""
import ctypes as C

import numpy as np

import newton_amd as nt
from newton_amd import _lib as L
from newton_amd import sensors

DT = float(np.float32(0.002))  # (a float32 number: the kernel and the reference divide by the same dt)
POISON = 7.0
EPS = 2.0 ** -24
TOL = 64.0 * EPS
FR_THREADS = 64  # lanes of a workgroup of frame_sensor_kernel: one wave, 64 worlds of one row
WORLDS = (1, 5, 37)
ROWS = (1, 3, 70)
OUTPUTS = {"transform": 7, "velocity": 6, "gravity_dir": 3, "accel": 3}
_MODELS, _CASES = {}, {}


def sensor_model(world_count, device=None, varied_gravity=True):
    """Four free bodies per world; bodies 1 and 3 carry their COM away from the body origin."""
    key = (world_count, device, varied_gravity)
    if key not in _MODELS:
        env = nt.ModelBuilder()
        coms = [None, (0.05, -0.02, 0.1), None, (-0.2, 0.0, 0.03)]
        for k, com in enumerate(coms):
            b = env.add_body(xform=[0.5 * k, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], com=com, mass=1.0 + k, inertia=np.eye(3) * 0.01 * (k + 1),
                             lock_inertia=True)
            env.add_shape_sphere(b, radius=0.05)
        scene = nt.ModelBuilder()
        scene.replicate(env, world_count)
        model = scene.finalize(device=device)
        com = np.asarray(model.body_com).reshape(world_count, 4, 3)
        assert np.all(com[:, 0] == 0.0) and np.all(np.any(com[:, 1] != 0.0, axis=-1)) and np.all(np.any(com[:, 3] != 0.0, axis=-1))
        if varied_gravity:
            rng = np.random.default_rng(99)
            g = np.tile(np.array([0.0, 0.0, -9.81], np.float32), (world_count, 1))
            g[1:] = rng.normal(size=(world_count - 1, 3)).astype(np.float32) * np.float32(6.0)
            if world_count > 3:
                g[3] = 0.0
            model.set_gravity(g)
            model.notify_model_changed()
        _MODELS[key] = model
    return _MODELS[key]


def random_xform(rng, reach=0.4):
    q = rng.normal(size=4)
    return np.concatenate([rng.uniform(-reach, reach, size=3), q / np.linalg.norm(q)]).astype(np.float32)


IDENTITY = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0], np.float32)


def frame_table(rng):
    """(frame_body [M], frame_xform [M, 7]): 0 identity on body 0 (COM at the origin); 1, 2 two frames on body 1 (COM off the origin);
    3 fixed in the world; 4 on body 2; 5 identity on body 3 (COM off the origin); 6 identity in the world; 7 on body 0."""
    body = np.array([0, 1, 1, -1, 2, 3, -1, 0], np.int32)
    xform = np.stack([IDENTITY, random_xform(rng), random_xform(rng), random_xform(rng, 2.0), random_xform(rng), IDENTITY, IDENTITY,
                      random_xform(rng)])
    return body, xform


# (frame, reference) of the first rows: a frame referenced to one LATER in the table first (so that N = 1 has it), to itself, the
# world-fixed frame in the world, a frame in the world-fixed frame, the two frames of body 1 in one another, ...
ROW_PATTERN = ((1, 4), (2, 2), (3, -1), (4, 3), (1, 2), (0, -1), (5, 7), (6, 5), (7, 0), (5, -1), (3, 6), (2, 1))


def rows(N, M, rng):
    frame = np.array([ROW_PATTERN[n][0] if n < len(ROW_PATTERN) else rng.integers(0, M) for n in range(N)], np.int32)
    ref = np.array([ROW_PATTERN[n][1] if n < len(ROW_PATTERN) else rng.integers(-1, M) for n in range(N)], np.int32)
    return frame, ref


class Case:
    def __init__(self, worlds, N, seed=0, varied_gravity=True):
        self.model = sensor_model(worlds, varied_gravity=varied_gravity)  # (the host model: tables and the reference; device models are the callers')
        self.varied_gravity = varied_gravity
        t = self.model.env
        self.E, self.N, self.nb = worlds, N, t.nb
        rng = np.random.default_rng(1000 * worlds + N + seed)
        B = worlds * t.nb
        q = rng.normal(size=(B, 4))
        self.body_q = np.concatenate([rng.uniform(-3.0, 3.0, size=(B, 3)), q / np.linalg.norm(q, axis=1, keepdims=True)], axis=1).astype(np.float32)
        self.body_qd = (rng.normal(size=(B, 6)) * np.array([1.5, 1.5, 1.5, 3.0, 3.0, 3.0])).astype(np.float32)
        self.body_qd_prev = (self.body_qd + rng.normal(size=(B, 6)) * 0.05).astype(np.float32)
        self.frame_body, self.frame_xform = frame_table(rng)
        self.M = len(self.frame_body)
        self.out_frame, self.out_ref = rows(N, self.M, rng)
        self.dt = DT
        self._ref = None

    def reference(self):
        """float64, every world, with the scales; computed once."""
        if self._ref is None:
            self._ref = sensors.frame_sensor_numpy(self.model, self.body_q, self.body_qd, self.frame_body, self.frame_xform, self.out_frame,
                                                   self.out_ref, self.body_qd_prev, self.dt, with_scale=True)
            for v in self._ref.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        return self._ref


def case(worlds, N, seed=0, varied_gravity=True):
    key = (worlds, N, seed, varied_gravity)
    if key not in _CASES:
        _CASES[key] = Case(worlds, N, seed, varied_gravity)
    return _CASES[key]


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p).value


class Call:
    """nt_frame_sensor_args over `case`; `upload` maps a host array to what the callee reads (identity on the emulator, a device tensor
    on the GPU, which must then provide `ptr`).  `only`: the outputs that get a buffer (poisoned), the others stay NULL."""

    def __init__(self, case, upload=None, ptr=_ptr, mask=None, only=tuple(OUTPUTS)):
        self.case, self.keep, self.ptr = case, [], ptr
        up = (lambda a: a) if upload is None else upload

        def dev(a):
            x = up(np.ascontiguousarray(a))
            self.keep.append(x)
            return x

        a = self.args = L.nt_frame_sensor_args()
        a.frame_count, a.out_count = case.M, case.N
        a.frame_body, a.frame_xform = ptr(dev(case.frame_body)), ptr(dev(case.frame_xform))
        a.out_frame, a.out_ref = ptr(dev(case.out_frame)), ptr(dev(case.out_ref))
        self.host = [x.copy() for x in (case.frame_body, case.frame_xform, case.out_frame, case.out_ref)]
        a.frame_body_host, a.frame_xform_host, a.out_frame_host, a.out_ref_host = (_ptr(x) for x in self.host)
        self.out = {}
        for k in only:
            self.out[k] = dev(np.full((case.E, case.N, OUTPUTS[k]), POISON, np.float32))
            setattr(a, k, ptr(self.out[k]))
        if mask is not None:
            self.mask = dev(np.asarray(mask).astype(np.uint8))
            a.world_mask = ptr(self.mask)

    def run(self, lib, model_desc, state_desc, prev_desc, stream=None, dt=None):
        return lib.nt_frame_sensor(C.byref(model_desc), C.byref(state_desc), None if prev_desc is None else C.byref(prev_desc),
                                   float(self.case.dt if dt is None else dt), C.byref(self.args), stream)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check(ref, got, mask=None, what=""):
    """Every non-None array of `got` (name -> [E, N, comp], host) against the reference dict `ref` (frame_sensor_numpy(...,
    with_scale=True)) within TOL * scale; rows of worlds outside `mask` keep the poison.  -> {name: largest error / (2^-24 scale)}."""
    ratios = {}
    for k, g in got.items():
        if g is None:
            continue
        g = np.asarray(g)
        E = g.shape[0]
        sel = np.ones(E, bool) if mask is None else np.asarray(mask, bool)
        want = ref[k]
        scale = np.broadcast_to(ref["scale"][k], want.shape)
        assert g.shape == want.shape and np.all(np.isfinite(g[sel]))
        err = np.abs(g.astype(np.float64) - want)[sel]
        sc = scale[sel]
        ratio = float(np.max(np.where(sc > 0.0, err / np.where(sc > 0.0, sc * EPS, 1.0), np.where(err == 0.0, 0.0, np.inf)), initial=0.0))
        ratios[k] = ratio
        print(f"frame sensor {what} {k}: largest error / (2^-24 scale) = {ratio:.3f}, largest |value| = {np.abs(want[sel]).max(initial=0.0):.4g}")
        assert np.all(err <= TOL * sc), (k, ratio)
        assert np.all(g[~sel] == POISON), k
    return ratios
