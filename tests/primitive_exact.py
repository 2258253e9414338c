"""Exact float64 geometry for the analytic contact pairs (newton_amd/csrc/nt_primitives.hpp), and the case tables shared by
tests/test_primitive_exact_host.py (no kernel), tests/test_primitive_exact_emu.py (kernel sources on the CPU) and
tests/test_gpu_primitive_exact.py (the device).  No tests in this module.

Everything here is written from the geometry of the shapes (distance to a plane, a segment, a box, a capped cylinder, the support
function of an ellipsoid, the closest points of two segments), not from the kernels or the CPU oracle, which are float32
restatements of one another.  Every routine takes the number type `dt`: float64 is the reference, float32 is used by the host test
alone, to measure how far a float32 evaluation of these same closed forms strays from float64 on the tables (the constant C below).

A table is a two-body scene (a global plane and one body for the plane pairs) replicated over worlds, one pose per world; one collide
launch covers a table.  Conventions of a decoded contact (pair_scenes.decode_world and nt_collide.hpp write_contact_slot): shape A is
the one of the lower type, the normal points from A into B, point0 / point1 sit on the CORE of A / B (sphere centre, capsule axis, the
surface itself for every other shape), margin0 / margin1 are radius + margin, d = n . (p1 - p0) - margin0 - margin1.

Allowance of a case: C * eps32 * L, L the largest of |position| and size; C per pair function from derive_constants().  Terms that
the contract formula itself adds are derived from that formula and added explicitly (Answer.bias_d / bias_n):
  sphere-capsule   closest_segment_point divides by |ab|^2 + 1e-6: the parameter is scaled by 1 / (1 + 1e-6 / |ab|^2)
  sphere-box       a centre outside by delta <= 1e-6 takes the interior formula: d = -delta - r instead of delta - r
  capsule-capsule  the two contacts of parallel capsules share the first one's normal (Contacts4 holds one normal)
A pose closer to a branch switch than its allowance (Answer.switch) is LEFT OUT of the branch-specific checks and held to the generic
invariants only; host test: at most 2 % of a table."""
import numpy as np

import newton_amd as nt
from newton_amd import _np_math as nm

EPS32 = float(np.finfo(np.float32).eps)
F64, F32 = np.float64, np.float32
COS_FLAT = 0.9238795325112867  # cos(22.5 deg): plane-cylinder flat / rolling switch
SURFACE_SWITCH = 1e-6  # sphere-box: |clamped - centre| <= 1e-6 takes the interior formula
SEGMENT_REG = 1e-6  # closest_segment_point: t = dot / (|ab|^2 + 1e-6)
CAPSULE_PARALLEL = 1e-11  # capsule-capsule: sin^2(angle) at or below this counts as parallel (NT_CAPSULE_PARALLEL)
LEFT_OUT_CAP = 0.02
ROUND = {"sphere": 1, "capsule": 1}  # kinds whose core is offset by the radius size[0]


# ---------------------------------------------------------------------------------------------------------------------------------
# number-type generic helpers
# ---------------------------------------------------------------------------------------------------------------------------------
def vec(x, dt):
    return np.asarray(x, dtype=dt)


def norm(v):
    return np.sqrt(np.dot(v, v))


def rot_matrix(q, dt):
    """Rotation matrix of the (normalised) quaternion xyzw."""
    q = vec(q, dt)
    x, y, z, w = q / norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=dt)


class Shape:
    """A shape in the world: kind, size (the builder's scale triple), position, rotation matrix."""

    def __init__(self, kind, size, xf, dt=F64):
        self.kind, self.size, self.p, self.R, self.dt = kind, vec(size, dt), vec(xf[:3], dt), rot_matrix(xf[3:7], dt), dt

    @property
    def axis(self):  # plane normal / capsule and cylinder axis
        return self.R[:, 2]

    def local(self, x):
        return self.R.T @ (vec(x, self.dt) - self.p)

    def radius(self):
        return self.size[0] if self.kind in ROUND else self.dt(0)


def closest_on_segment(a, b, x):
    """Closest point of segment ab to x, and the unclamped parameter; valid for a == b."""
    ab = b - a
    den = np.dot(ab, ab)
    t = np.dot(x - a, ab) / den if den > 0 else den * 0
    return a + np.clip(t, 0, 1) * ab, t


# ---------------------------------------------------------------------------------------------------------------------------------
# surface functions: signed distance of a world point to the surface (ellipsoid: first-order distance from the implicit residual)
# ---------------------------------------------------------------------------------------------------------------------------------
def sdf_plane(s, x):
    return np.dot(s.axis, x - s.p)


def sdf_sphere(s, x):
    return norm(x - s.p) - s.size[0]


def sdf_capsule(s, x):
    h = s.axis * s.size[1]
    c, _ = closest_on_segment(s.p - h, s.p + h, x)
    return norm(x - c) - s.size[0]


def sdf_box(s, x):
    q = np.abs(s.local(x)) - s.size
    return norm(np.maximum(q, 0)) + min(np.max(q), 0)


def sdf_cylinder(s, x):
    l = s.local(x)
    q = np.array([np.sqrt(l[0] * l[0] + l[1] * l[1]) - s.size[0], abs(l[2]) - s.size[1]])
    return norm(np.maximum(q, 0)) + min(np.max(q), 0)


def ellipsoid_residual(s, x):
    l = s.local(x) / s.size
    return np.dot(l, l) - 1


def ellipsoid_support(s, n):
    """h(n) = sqrt(sum (s_i n_i)^2), n in the world; and the support point in direction n."""
    nl = s.R.T @ n
    h = norm(s.size * nl)
    return h, s.p + s.R @ (s.size * s.size * nl / h)


def sdf_ellipsoid(s, x):
    l = s.local(x)
    g = l / (s.size * s.size)
    return ellipsoid_residual(s, x) / (2 * norm(g))


SDF = {"plane": sdf_plane, "sphere": sdf_sphere, "capsule": sdf_capsule, "box": sdf_box, "cylinder": sdf_cylinder,
       "ellipsoid": sdf_ellipsoid}


# ---------------------------------------------------------------------------------------------------------------------------------
# exact answers per pair
# ---------------------------------------------------------------------------------------------------------------------------------
class Answer:
    """d: exact smallest signed surface distance (margins not subtracted); n: exact direction A -> B, None where it is not unique;
    lever: the length that turns an error of n into a length (the distance between the features that define n, or L for a normal fixed
    by a face); branch: label; switch: distance to the nearest branch switch in length units (switch_rel: of a dimensionless quantity
    such as a cosine, turned into a length by the case's scale L); count: expected number of exported
    contacts (None: not asserted); all_d: every expected distance, sorted (None: only the minimum is known); bias_*: see the module
    docstring; extra_n: allowance added to the surface invariants of the contacts after the first (shared normal)."""

    def __init__(self, d, n, lever, branch, switch=np.inf, count=1, all_d=None, bias_d=0.0, bias_n=0.0, extra_n=0.0, corners=None,
                 switch_rel=np.inf):
        self.switch_rel = switch_rel
        self.d, self.n, self.lever, self.branch, self.switch, self.count = d, n, lever, branch, switch, count
        self.all_d, self.bias_d, self.bias_n, self.extra_n, self.corners = all_d, bias_d, bias_n, extra_n, corners


def plane_sphere(A, B):
    return Answer(sdf_plane(A, B.p) - B.size[0], A.axis, None, "plane_sphere")


def sphere_sphere(A, B):
    dirv = B.p - A.p
    L = norm(dirv)
    rr = A.size[0] + B.size[0]
    if L == 0:
        return Answer(-rr, None, None, "coincident")  # (the reference's fallback normal (1, 0, 0): any unit vector is exact)
    d = L - rr
    return Answer(d, dirv / L, L, "touching" if abs(d) < 1e-6 * rr else ("apart" if d > 0 else "overlapping"))


def plane_capsule(A, B):
    n, h = A.axis, B.axis * B.size[1]
    ds = sorted([sdf_plane(A, B.p + h) - B.size[0], sdf_plane(A, B.p - h) - B.size[0]])
    c = abs(np.dot(n, B.axis))
    branch = "parallel" if c < 1e-6 else ("perpendicular" if c > 1 - 1e-9 else "oblique")
    return Answer(ds[0], n, None, branch, count=2, all_d=ds)


def sphere_capsule(A, B):
    h = B.axis * B.size[1]
    a, b = B.p - h, B.p + h
    pt, t = closest_on_segment(a, b, A.p)
    rho = norm(A.p - pt)
    rr = A.size[0] + B.size[0]
    ab2 = np.dot(b - a, b - a)
    # the contract formula's point: parameter t * |ab|^2 / (|ab|^2 + 1e-6)
    ptb = a + np.clip(t * ab2 / (ab2 + SEGMENT_REG), 0, 1) * (b - a)
    rhob = norm(A.p - ptb)
    branch = "beyond_lo" if t < 0 else ("beyond_hi" if t > 1 else "mid")
    if rho < 1e-9 * (1 + norm(A.p)):
        return Answer(rho - rr, None, None, "on_axis", bias_d=abs(rhob - rho))
    n = (pt - A.p) / rho
    return Answer(rho - rr, n, rho, branch, bias_d=abs(rhob - rho), bias_n=norm((ptb - A.p) / rhob - n))


def sphere_cylinder(A, B):
    r, h, rs = B.size[0], B.size[1], A.size[0]
    l = B.local(A.p)
    x, rho = l[2], np.sqrt(l[0] * l[0] + l[1] * l[1])
    radial = B.R @ np.array([l[0], l[1], 0 * x]) / rho if rho > 0 else None
    axial = B.axis * (1 if x > 0 else -1)
    if abs(x) < h and rho < r:  # inside: the nearer of cap and side
        dc, dr = h - abs(x), r - rho
        sw = abs(dc - dr)
        if dc < dr:
            return Answer(-dc - rs, -axial, None, "inside_cap", sw)
        if rho < 1e-9 * (1 + norm(A.p)):
            return Answer(-dr - rs, None, None, "inside_side_on_axis", sw)
        return Answer(-dr - rs, -radial, rho, "inside_side", sw)
    if abs(x) < h:
        return Answer(rho - r - rs, -radial, rho, "side")
    if rho < r:
        return Answer(abs(x) - h - rs, -axial, None, "cap_on_axis" if rho < 1e-9 * (1 + norm(A.p)) else "cap")
    rim = B.p + B.axis * (h if x > 0 else -h) + radial * r
    dist = norm(rim - A.p)
    return Answer(dist - rs, (rim - A.p) / dist, dist, "rim")


def sphere_box(A, B):
    rs, c = A.size[0], B.local(A.p)
    cl = np.clip(c, -B.size, B.size)
    diff = cl - c
    dist = norm(diff)
    if dist > 0:
        region = ("face", "edge", "corner")[int(np.count_nonzero(diff)) - 1]
        n = B.R @ (diff / dist)
        near = dist <= 2 * SURFACE_SWITCH
        # within the surface switch the contract takes the interior formula: nearest face, d = -delta - r
        return Answer(dist - rs, n if (region == "face" or not near) else None, dist if not near else None,
                      region + ("_near" if near else ""), abs(dist - SURFACE_SWITCH), bias_d=2 * dist if near else 0.0)
    fd = np.concatenate([B.size - c, B.size + c])  # distances to the +x +y +z -x -y -z faces
    k = int(np.argmin(fd))
    e = np.zeros(3, dtype=A.dt)
    e[k % 3] = 1 if k < 3 else -1  # outward normal of the nearest face
    two = np.sort(fd)
    return Answer(-fd[k] - rs, -(B.R @ e), None, "inside_" + "+x+y+z-x-y-z"[2 * k:2 * k + 2], two[1] - two[0])


def box_corners(B):
    s = B.size
    return [B.p + B.R @ (np.array([sx, sy, sz], dtype=B.dt) * s) for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)]


def plane_box(A, B, box_margin):
    corners = box_corners(B)
    ds = np.sort(np.array([sdf_plane(A, c) for c in corners]))
    under = ds[ds <= box_margin]
    sw = float(np.min(np.abs(ds - box_margin)))
    if len(under) > 4:
        sw = min(sw, float(ds[4] - ds[3]))
    kept = under[:4]
    rank = np.round((ds - ds[0]) / max(1e-9, 1e-6 * norm(B.size)))
    low = int(np.sum(rank == rank[0]))
    branch = {1: "corner_down", 2: "edge_down", 4: "face_down"}.get(low, "other")
    if len(under) > 4:
        branch += "_over4"
    return Answer(ds[0], A.axis, None, branch, sw, count=len(kept), all_d=list(kept), corners=corners)


def plane_ellipsoid(A, B):
    h, _ = ellipsoid_support(B, -A.axis)
    return Answer(sdf_plane(A, B.p) - h, A.axis, None, "plane_ellipsoid")


def plane_cylinder(A, B):
    n, a = A.axis, B.axis
    c = np.dot(n, a)
    s2 = max(1 - c * c, 0 * c)
    d = sdf_plane(A, B.p) - (B.size[1] * abs(c) + B.size[0] * np.sqrt(s2))
    if s2 <= 1e-10:
        branch, count = "upright", 3  # no tilt direction: the deepest point IS the tripod's first point
    elif abs(c) >= COS_FLAT:
        branch, count = "flat", None  # the deepest rim point + the fixed tripod (3 or 4: a tripod point may coincide with it)
    else:
        branch, count = ("side" if abs(c) < 1e-6 else "rolling"), 3
    branch += "+" if c > 0 else "-"
    return Answer(d, n, None, branch, count=count, switch_rel=abs(abs(c) - COS_FLAT))


def segment_segment(p1, a1, p2, a2):
    """Closest points of the segments p1 +- a1 and p2 +- a2 -> (x1, x2, distance), parameters in [-1, 1].  The smallest of five
    candidates: the common perpendicular of the two lines where it meets both segments (cross products: no cancellation for nearly
    parallel axes), and each of the four end points against the other segment.  Valid for parallel and degenerate segments."""
    best = None
    for s in (1, -1):
        for (pa, aa, pb, ab, first) in ((p1, a1, p2, a2, True), (p2, a2, p1, a1, False)):
            e = pa + s * aa
            c, t = closest_on_segment(pb - ab, pb + ab, e)
            y = 2 * np.clip(t, 0, 1) - 1
            cand = (s, y, norm(e - c)) if first else (y, s, norm(e - c))
            if best is None or cand[2] < best[2]:
                best = cand
    cr = np.cross(a1, a2)
    den = np.dot(cr, cr)
    if den > 0:
        w = p2 - p1
        x1 = np.dot(np.cross(w, a2), cr) / den
        x2 = np.dot(np.cross(w, a1), cr) / den
        if abs(x1) <= 1 and abs(x2) <= 1:
            dist = norm(p1 + a1 * x1 - p2 - a2 * x2)
            if dist < best[2]:
                best = (x1, x2, dist)
    return best


def capsule_capsule(A, B):
    a1, a2 = A.axis * A.size[1], B.axis * B.size[1]
    rr = A.size[0] + B.size[0]
    x1, x2, dist = segment_segment(A.p, a1, B.p, a2)
    P1, P2 = A.p + a1 * x1, B.p + a2 * x2
    cr = np.cross(A.axis, B.axis)
    sin2 = np.dot(cr, cr)
    sw_rel = abs(np.sqrt(sin2) - np.sqrt(CAPSULE_PARALLEL))
    n = (P2 - P1) / dist if dist > 1e-9 * (1 + norm(A.p)) else None
    # nearly parallel axes: the distance is all but constant along the overlap, so WHICH closest pair comes out is decided by the
    # last bit of the input; the direction between any two such pairs differs by at most sin(angle) * (total length) / distance.
    # (The contact is still held to: both points on their segments, their distance the exact minimum -- check_table.)
    flat_n = float(np.sqrt(sin2)) * 2 * float(A.size[1] + B.size[1]) / float(dist) if (sin2 < 0.05 ** 2 and n is not None) else 0.0
    if sin2 > CAPSULE_PARALLEL:
        ends = int(abs(x1) == 1) + int(abs(x2) == 1)
        return Answer(dist - rr, n, dist, ("interior", "end", "end_end")[ends], bias_n=flat_n, switch_rel=sw_rel)
    # parallel: the overlap of the two segments along the common axis; a contact at each end of it
    ah = A.axis
    t0, h1, h2 = np.dot(B.p - A.p, ah), A.size[1], B.size[1]
    lo, hi = max(-h1, t0 - h2), min(h1, t0 + h2)
    sw = abs(hi - lo)
    if hi - lo <= 0:
        return Answer(dist - rr, n, dist, "parallel_apart", sw, bias_n=flat_n, switch_rel=sw_rel)
    ds, ns = [], []
    for t in (lo, hi):
        q1 = A.p + ah * t
        q2, _ = closest_on_segment(B.p - a2, B.p + a2, q1)
        q1, _ = closest_on_segment(A.p - a1, A.p + a1, q2)
        ds.append(norm(q2 - q1) - rr)
        ns.append((q2 - q1) / norm(q2 - q1))
    over = "overhang_a" if (lo > -h1 and hi < h1) else ("overhang_b" if (lo == -h1 and hi == h1) else "partial")
    # the second contact is placed with the first one's normal: its core points move by (r + |d| / 2) |n1 - n0| each
    extra = (rr + abs(max(ds))) * norm(ns[1] - ns[0])
    return Answer(min(dist - rr, min(ds)), n, dist, "parallel_" + over, sw, count=2, all_d=sorted(ds), extra_n=extra, bias_n=flat_n,
                  switch_rel=sw_rel)


PAIRS = {  # pair function -> (kind A, kind B, exact answer)
    "plane_sphere": ("plane", "sphere", plane_sphere), "sphere_sphere": ("sphere", "sphere", sphere_sphere),
    "plane_capsule": ("plane", "capsule", plane_capsule), "plane_box": ("plane", "box", plane_box),
    "plane_ellipsoid": ("plane", "ellipsoid", plane_ellipsoid), "plane_cylinder": ("plane", "cylinder", plane_cylinder),
    "sphere_capsule": ("sphere", "capsule", sphere_capsule), "sphere_cylinder": ("sphere", "cylinder", sphere_cylinder),
    "sphere_box": ("sphere", "box", sphere_box), "capsule_capsule": ("capsule", "capsule", capsule_capsule),
}


# ---------------------------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------------------------
def _unit(v):
    v = np.asarray(v, dtype=F64)
    return v / np.linalg.norm(v)


I4 = np.array([0.0, 0.0, 0.0, 1.0])
QX90 = nm.quat_from_axis_angle([1.0, 0.0, 0.0], np.pi / 2)  # z axis -> -y
QX180 = nm.quat_from_axis_angle([1.0, 0.0, 0.0], np.pi)  # z axis -> -z
QGEN = [_unit([0.3, -0.5, 0.2, 0.8]), _unit([-0.62, 0.11, 0.47, 0.35])]  # generic (non-axis-aligned) orientations
ORIENTATIONS = [I4, QX90, *QGEN]
GROUND = np.array([0.0, 0.0, 0.0, *I4])
TILTED = np.array([0.3, -0.2, 0.4, *_unit([0.25, -0.15, 0.1, 0.95])])  # a tilted, offset plane


def frame(q):
    R = rot_matrix(q, F64)
    return R[:, 0], R[:, 1], R[:, 2]


class Table:
    def __init__(self, name, pair, size_a, size_b, margins=(0.0, 0.0), gap=10.0, plane=None):
        self.name, self.pair, self.size_a, self.size_b, self.margins, self.gap, self.plane = name, pair, size_a, size_b, margins, gap, plane
        self.kind_a, self.kind_b, self.fn = PAIRS[pair]
        self.poses, self.tags = [], []
        self._answers = {}

    def add(self, tag, xa, xb):
        """One world: poses (p, q) of A and B (A ignored for plane tables), rounded to float32 here -- the reference sees what the
        kernel sees."""
        row = np.zeros((2, 7))
        row[0] = GROUND if xa is None else np.concatenate([np.asarray(xa[0], F64), np.asarray(xa[1], F64)])
        row[1] = np.concatenate([np.asarray(xb[0], F64), np.asarray(xb[1], F64)])
        self.poses.append(row.astype(F32))
        self.tags.append(tag)

    @property
    def worlds(self):
        return len(self.poses)

    @property
    def box_margin(self):  # what primitive_pair gets for plane_box: gap sum + margins, all in float32 like the model stores them
        g = F32(self.gap) if self.plane is None else F32(0.0)
        return float(F32(F32(self.gap) + g) + F32(self.margins[0]) + F32(self.margins[1]))

    def shapes(self, w, dt=F64):
        xa = self.plane.astype(F32) if self.plane is not None else self.poses[w][0]
        return (Shape(self.kind_a, np.asarray(self.size_a, F32), xa, dt), Shape(self.kind_b, np.asarray(self.size_b, F32), self.poses[w][1], dt))

    def answer(self, w, dt=F64):
        if (w, dt) not in self._answers:
            A, B = self.shapes(w, dt)
            self._answers[(w, dt)] = self.fn(A, B, dt(self.box_margin)) if self.pair == "plane_box" else self.fn(A, B)
        return self._answers[(w, dt)]

    def scale(self, w):
        """L: the largest of |position| and size."""
        A, B = self.shapes(w)
        return float(max(np.linalg.norm(A.p), np.linalg.norm(B.p), np.max(A.size), np.max(B.size)))

    def body_q(self):
        rows = [p[1:] if self.plane is not None else p for p in self.poses]
        return np.concatenate(rows).astype(F32)

    def model(self, device=None):
        """The scene: one body per non-plane shape, replicated; the plane is a global static shape."""
        env = nt.ModelBuilder()
        kinds = [(self.kind_a, self.size_a, self.margins[0]), (self.kind_b, self.size_b, self.margins[1])]
        for kind, size, margin in kinds[1:] if self.plane is not None else kinds:
            add_shape(env, env.add_body(xform=[0.0, 0.0, 0.0, *I4], mass=1.0), kind, size, margin, self.gap)
        scene = nt.ModelBuilder()
        scene.replicate(env, self.worlds)
        if self.plane is not None:
            scene.add_shape_plane(xform=[float(v) for v in self.plane], width=0.0, length=0.0,
                                  cfg=nt.ModelBuilder.ShapeConfig(margin=self.margins[0], gap=0.0))
        model = scene.finalize(device=device)
        bq = self.body_q()
        model.body_q[...] = bq
        model.joint_q.reshape(-1, 7)[...] = bq
        return model


def add_shape(b, body, kind, size, margin, gap):
    cfg = nt.ModelBuilder.ShapeConfig(margin=margin, gap=gap)
    if kind == "sphere":
        return b.add_shape_sphere(body, radius=size[0], cfg=cfg)
    if kind == "capsule":
        return b.add_shape_capsule(body, radius=size[0], half_height=size[1], cfg=cfg)
    if kind == "cylinder":
        return b.add_shape_cylinder(body, radius=size[0], half_height=size[1], cfg=cfg)
    if kind == "box":
        return b.add_shape_box(body, hx=size[0], hy=size[1], hz=size[2], cfg=cfg)
    if kind == "ellipsoid":
        return b.add_shape_ellipsoid(body, rx=size[0], ry=size[1], rz=size[2], cfg=cfg)
    raise ValueError(kind)


DIRS = [_unit(v) for v in ([1, 0, 0], [0, -1, 0], [0.3, -0.5, 0.81], [-0.6, 0.64, -0.48])]
HEIGHTS = (0.3, 1e-4, -0.02)  # above, just above, penetrating


def _plane_point(plane, u, v, hgt):
    ex, ey, ez = frame(plane[3:])
    return plane[:3] + ex * u + ey * v + ez * hgt


def _tables_sphere_sphere():
    out = []
    for name, ra, rb, mg in (("base", 0.1, 0.15, (0, 0)), ("ratio1e3", 1e-3, 1.0, (0, 0)), ("margin", 0.1, 0.15, (0.01, 0.02))):
        t = Table("sphere_sphere/" + name, "sphere_sphere", (ra, 0, 0), (rb, 0, 0), mg)
        for base in ([0, 0, 0], [0.4, -0.3, 0.2], [60.0, -64.0, 48.0]):  # the last one: |p| = 100
            base = np.asarray(base, F64)
            t.add("coincident", (base, I4), (base, I4))
            for dv in DIRS:
                for sep in (0.0, 0.3, -0.04, 1e-3 * (ra + rb)):
                    t.add("sep%g" % sep, (base, I4), (base + dv * (ra + rb + sep), I4))
        out.append(t)
    return out


def _tables_plane_sphere():
    out = []
    for name, r, mg, plane in (("ground", 0.1, (0, 0), GROUND), ("tilted_margin", 1.0, (0.01, 0.02), TILTED)):
        t = Table("plane_sphere/" + name, "plane_sphere", (0, 0, 0), (r, 0, 0), mg, plane=plane)
        for u, v in ((0, 0), (0.7, -0.4), (-30.0, 95.0)):
            for hgt in HEIGHTS:
                t.add("h%g" % hgt, None, (_plane_point(plane, u, v, r + hgt), I4))
        out.append(t)
    return out


def _tables_plane_capsule():
    out = []
    for name, r, hh, mg, plane in (("ground", 0.1, 0.5, (0, 0), GROUND), ("tilted_10to1", 0.05, 0.5, (0, 0), TILTED),
                                   ("tilted_margin", 0.1, 0.3, (0.01, 0.02), TILTED)):
        t = Table("plane_capsule/" + name, "plane_capsule", (0, 0, 0), (r, hh, 0), mg, plane=plane)
        for tilt in (0.0, np.pi / 2, np.pi, 0.4, 1.2, 2.5):  # perpendicular, parallel, flipped, oblique
            for az in (0.0, 1.1):
                q = nm.quat_mul(plane[3:], nm.quat_mul(nm.quat_from_axis_angle([0, 0, 1.0], az), nm.quat_from_axis_angle([1.0, 0, 0], tilt)))
                low = hh * abs(np.cos(tilt)) + r
                for hgt in HEIGHTS:
                    t.add("tilt%g" % tilt, None, (_plane_point(plane, 0.2, -0.1, low + hgt), q))
        out.append(t)
    return out


def _tables_plane_ellipsoid():
    out = []
    for name, size, mg, plane in (("ground", (0.12, 0.08, 0.06), (0, 0), GROUND), ("tilted_10to1", (1.0, 0.1, 0.1), (0, 0), TILTED),
                                  ("tilted_margin", (0.12, 0.08, 0.06), (0.01, 0.02), TILTED)):
        t = Table("plane_ellipsoid/" + name, "plane_ellipsoid", (0, 0, 0), size, mg, plane=plane)
        for q in ORIENTATIONS + [nm.quat_mul(plane[3:], o) for o in ORIENTATIONS]:
            R = rot_matrix(q, F64)
            n = frame(plane[3:])[2]
            h = np.linalg.norm(np.asarray(size) * (R.T @ n))
            for hgt in HEIGHTS:
                t.add("h%g" % hgt, None, (_plane_point(plane, -0.3, 0.25, h + hgt), q))
        out.append(t)
    return out


def _tables_plane_box():
    out = []
    for name, size, mg, plane in (("ground", (0.1, 0.08, 0.06), (0, 0), GROUND), ("tilted_10to1", (1.0, 0.1, 0.1), (0, 0), TILTED),
                                  ("tilted_margin", (0.1, 0.08, 0.06), (0.01, 0.02), TILTED)):
        t = Table("plane_box/" + name, "plane_box", (0, 0, 0), size, mg, gap=0.05, plane=plane)
        bm = t.box_margin
        s = np.asarray(size, F64)
        n = frame(plane[3:])[2]
        rel = [("face", I4), ("face", QX90), ("face", nm.quat_from_axis_angle([0, 1.0, 0], np.pi / 2)),
               ("edge", nm.quat_from_axis_angle([1.0, 0, 0], 0.6)), ("edge", nm.quat_from_axis_angle([0, 1.0, 0], -0.35)),
               ("corner", QGEN[0]), ("corner", QGEN[1]), ("corner", _unit([0.4, 0.3, -0.1, 0.86]))]
        for tag, qr in rel:
            for az in (0.0, 0.7):
                q = nm.quat_mul(plane[3:], nm.quat_mul(nm.quat_from_axis_angle([0, 0, 1.0], az), qr))
                R = rot_matrix(q, F64)
                low = float(np.sum(np.abs(R.T @ n) * s))  # centre height at which the deepest corner touches the plane
                # deepest corner: just above / just below the margin, touching, in the ground, and deep enough for all 8 corners
                for what, hgt in (("above", bm + 1e-4), ("below", bm - 1e-4), ("touch", 0.0), ("in", -0.01), ("deep", bm - 2 * low - 0.01)):
                    t.add(tag + "_" + what, None, (_plane_point(plane, 0.15, -0.2, low + hgt), q))
        out.append(t)
    return out


def _tables_plane_cylinder():
    out = []
    for name, r, hh, mg, plane in (("ground", 0.08, 0.1, (0, 0), GROUND), ("tilted_10to1", 0.05, 0.5, (0, 0), TILTED),
                                   ("tilted_margin", 0.08, 0.1, (0.01, 0.02), TILTED)):
        t = Table("plane_cylinder/" + name, "plane_cylinder", (0, 0, 0), (r, hh, 0), mg, plane=plane)
        flat = np.pi / 8
        tilts = [0.0, np.pi, np.pi / 2, 1.2, 2.0] + [s * (flat + d) + o for o in (0.0, np.pi) for s in (1, -1)
                                                   for d in (-0.2, -0.03, -1e-3, -1e-5, 1e-5, 1e-3, 0.03, 0.2)]
        for tilt in tilts:
            for az in (0.0, 0.9, 2.3):
                q = nm.quat_mul(plane[3:], nm.quat_mul(nm.quat_from_axis_angle([0, 0, 1.0], az), nm.quat_from_axis_angle([1.0, 0, 0], tilt)))
                low = hh * abs(np.cos(tilt)) + r * abs(np.sin(tilt))
                for hgt in (0.05, -0.01):
                    t.add("tilt%.6f" % tilt, None, (_plane_point(plane, 0.1, 0.2, low + hgt), q))
        out.append(t)
    return out


def _body_poses():
    """Poses of shape B: aligned and generic orientations, near the origin and away from it."""
    return [(np.zeros(3), I4), (np.array([0.2, -0.1, 0.3]), QX90), (np.array([0.4, 0.3, -0.2]), QGEN[0]),
            (np.array([-7.0, 5.0, 4.0]), QGEN[1])]


def _tables_sphere_capsule():
    out = []
    for name, rs, r, hh, mg in (("base", 0.1, 0.1, 0.5, (0, 0)), ("short", 0.05, 0.05, 0.02, (0, 0)), ("10to1_margin", 0.1, 0.05, 0.5, (0.01, 0.02))):
        t = Table("sphere_capsule/" + name, "sphere_capsule", (rs, 0, 0), (r, hh, 0), mg)
        for p, q in _body_poses():
            ex, ey, ez = frame(q)
            for sep in (0.2, 1e-4, -0.03):
                rho = rs + r + sep
                for ax in (0.0, 0.6 * hh, -0.95 * hh):
                    t.add("beside", (p + ez * ax + (0.6 * ex - 0.8 * ey) * rho, I4), (p, q))
                for s in (1, -1):
                    t.add("beyond", (p + ez * s * (hh + 0.6 * rho) + ey * 0.8 * rho, I4), (p, q))
                    t.add("beyond_on_axis", (p + ez * s * (hh + rho), I4), (p, q))
            for ax in (0.0, 0.5 * hh, -0.9 * hh):
                t.add("on_axis", (p + ez * ax, I4), (p, q))
        out.append(t)
    return out


def _tables_sphere_cylinder():
    out = []
    for name, rs, r, hh, mg in (("base", 0.05, 0.2, 0.3, (0, 0)), ("10to1", 0.05, 0.05, 0.5, (0, 0)), ("margin", 0.05, 0.2, 0.3, (0.01, 0.02))):
        t = Table("sphere_cylinder/" + name, "sphere_cylinder", (rs, 0, 0), (r, hh, 0), mg)
        m = min(r, hh)
        for p, q in _body_poses():
            ex, ey, ez = frame(q)
            rad = 0.6 * ex - 0.8 * ey
            for s in (1, -1):
                for sep in (0.1, 1e-4, -0.02):
                    t.add("side", (p + rad * (r + rs + sep) + ez * s * 0.5 * hh, I4), (p, q))
                    t.add("cap", (p + rad * 0.5 * r + ez * s * (hh + rs + sep), I4), (p, q))
                    t.add("cap_on_axis", (p + ez * s * (hh + rs + sep), I4), (p, q))
                    t.add("rim", (p + rad * (r + 0.6 * (rs + sep)) + ez * s * (hh + 0.8 * (rs + sep)), I4), (p, q))
                t.add("inside_side", (p + rad * (r - 0.2 * m) + ez * s * (hh - 0.6 * m), I4), (p, q))
                t.add("inside_cap", (p + rad * (r - 0.6 * m) + ez * s * (hh - 0.2 * m), I4), (p, q))
                t.add("inside_on_axis", (p + ez * s * (hh - 0.3 * m), I4), (p, q))
            t.add("inside_on_axis", (p + ez * 0.01 * m, I4), (p, q))
        out.append(t)
    return out


def _tables_sphere_box():
    out = []
    for name, rs, size, mg in (("base", 0.05, (0.1, 0.08, 0.06), (0, 0)), ("10to1", 0.05, (1.0, 0.1, 0.1), (0, 0)),
                               ("margin", 0.05, (0.1, 0.08, 0.06), (0.01, 0.02))):
        t = Table("sphere_box/" + name, "sphere_box", (rs, 0, 0), size, mg)
        s = np.asarray(size, F64)
        m = float(np.min(s))
        # the 1e-6 surface switch: centres small enough that their float32 rounding stays far below 1e-6.  A box of size 1 has an
        # allowance of about 1e-6 itself: every such case is left out there, so it gets two of them only
        for p, q in ((np.zeros(3), I4), (np.array([0.05, -0.03, 0.04]), QGEN[0])):
            R = rot_matrix(q, F64)
            for k, sg in ((0, 1), (1, -1), (2, 1)) if m == float(np.max(s)) or np.max(s) < 0.5 else ((1, -1),):
                e = np.zeros(3)
                e[k] = sg
                for delta in (5e-7, 2e-7, -5e-7, 1.6e-6, 3e-6) if np.max(s) < 0.5 else (5e-7,):
                    t.add("near_surface", (p + R @ (e * (s[k] + delta) + (1 - np.abs(e)) * s * np.array([0.3, -0.5, 0.4])), I4), (p, q))
        for p, q in _body_poses():
            R = rot_matrix(q, F64)
            put = lambda tag, l: t.add(tag, (p + R @ np.asarray(l, F64), I4), (p, q))  # noqa: E731
            for k in range(3):
                for sg in (1, -1):
                    e = np.zeros(3)
                    e[k] = sg
                    inplane = (1 - np.abs(e)) * s * np.array([0.3, -0.5, 0.4])
                    for sep in (0.1, 1e-4, -0.02):
                        put("face", e * (s[k] + rs + sep) + inplane)
                    put("inside", e * (s[k] - 0.3 * m) + inplane * 0.2)
            for sx, sy, sz in ((1, 1, 0), (1, 0, -1), (0, -1, 1), (-1, -1, 0), (1, 1, 1), (-1, 1, -1), (1, -1, -1), (-1, -1, 1)):
                sg = np.array([sx, sy, sz], F64)
                for sep in (0.1, 1e-4, -0.02):
                    off = _unit(sg * np.array([0.5, 0.7, 0.6])) * (rs + sep)
                    put("corner" if sx * sy * sz else "edge", sg * s + off + (1 - np.abs(sg)) * s * 0.3)
        out.append(t)
    return out


SWEEP = (0.0, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1)


def _tables_capsule_capsule():
    out = []
    sets = (("long_short", (0.1, 0.5), (0.1, 0.4), (0, 0)), ("short_long", (0.1, 0.4), (0.1, 0.5), (0, 0)),
            ("10to1_overhang", (0.05, 1.0), (0.05, 0.25), (0, 0)), ("overhang_swapped_margin", (0.05, 0.25), (0.05, 1.0), (0.01, 0.02)))
    for name, (r1, h1), (r2, h2), mg in sets:
        t = Table("capsule_capsule/" + name, "capsule_capsule", (r1, h1, 0), (r2, h2, 0), mg)
        lat = r1 + r2 + 0.05
        for p, q in _body_poses():
            e1, e2, a = frame(q)

            def put(tag, offset, angle=0.0, about=None, lateral=None, q2=None):
                q2 = nm.quat_mul(nm.quat_from_axis_angle(e1 if about is None else about, angle), q) if q2 is None else q2
                t.add(tag, (p, q), (p + e1 * (lat if lateral is None else lateral) + offset, q2))

            put("crossed", 0 * a, np.pi / 2)
            put("skew", a * 0.2 + e2 * 0.1, 0.7, lateral=0.3)
            put("t_shape", a * (h1 + lat), np.pi / 2, about=e2, lateral=0.0)
            put("colinear", a * (h1 + h2 + lat), lateral=0.0)
            put("colinear_flipped", -a * (h1 + h2 + lat), lateral=0.0, q2=nm.quat_mul(q, QX180))
            put("parallel_centred", 0 * a)
            put("parallel_shifted", a * 0.3 * min(h1, h2))
            put("parallel_partial", a * (max(h1, h2) + 0.2 * min(h1, h2)))
            put("parallel_partial", -a * (max(h1, h2) + 0.2 * min(h1, h2)), q2=nm.quat_mul(q, QX180))
            put("parallel_apart", a * (h1 + h2 + 0.2))
            put("parallel_penetrating", a * 0.1 * min(h1, h2), lateral=r1 + r2 - 0.03)
            # the angle between the axes swept from 0 to 0.1: about the lateral direction (skew lines whose common perpendicular sits
            # at the axial offset: interior, at capsule A's end, past it) and about the other perpendicular (converging lines)
            for angle in SWEEP:
                for tag, off in (("interior", 0.2 * h1), ("at_end", h1), ("past_end", h1 + 0.2)):
                    put("sweep_%s_%g" % (tag, angle), a * off, angle)
                    put("sweep_conv_%s_%g" % (tag, angle), a * off, angle, about=e2)
        out.append(t)
    return out


_TABLES = None


def tables():
    global _TABLES
    if _TABLES is None:
        _TABLES = (_tables_sphere_sphere() + _tables_plane_sphere() + _tables_plane_capsule() + _tables_plane_box() + _tables_plane_ellipsoid()
                   + _tables_plane_cylinder() + _tables_sphere_capsule() + _tables_sphere_cylinder() + _tables_sphere_box()
                   + _tables_capsule_capsule())
    return _TABLES


def table(name):
    return {t.name: t for t in tables()}[name]


TABLE_NAMES = [f"{p}/{s}" for p, ss in (
    ("sphere_sphere", ("base", "ratio1e3", "margin")), ("plane_sphere", ("ground", "tilted_margin")),
    ("plane_capsule", ("ground", "tilted_10to1", "tilted_margin")), ("plane_box", ("ground", "tilted_10to1", "tilted_margin")),
    ("plane_ellipsoid", ("ground", "tilted_10to1", "tilted_margin")), ("plane_cylinder", ("ground", "tilted_10to1", "tilted_margin")),
    ("sphere_capsule", ("base", "short", "10to1_margin")), ("sphere_cylinder", ("base", "10to1", "margin")),
    ("sphere_box", ("base", "10to1", "margin")),
    ("capsule_capsule", ("long_short", "short_long", "10to1_overhang", "overhang_swapped_margin"))) for s in ss]
ROLLOUT_TABLES = [n for n in TABLE_NAMES if n.split("/")[0] in ("sphere_capsule", "capsule_capsule", "sphere_box", "sphere_cylinder")]

# the branches every pair's tables must reach (decided by the reference; asserted by the host test)
REQUIRED_BRANCHES = {
    "sphere_sphere": {"coincident", "touching", "apart", "overlapping"},
    "plane_sphere": {"plane_sphere"},
    "plane_capsule": {"parallel", "perpendicular", "oblique"},
    "plane_box": {"face_down", "edge_down", "corner_down", "face_down_over4", "edge_down_over4", "corner_down_over4"},
    "plane_ellipsoid": {"plane_ellipsoid"},
    "plane_cylinder": {"upright+", "upright-", "flat+", "flat-", "rolling+", "rolling-", "side+", "side-"},
    "sphere_capsule": {"mid", "beyond_lo", "beyond_hi", "on_axis"},
    "sphere_cylinder": {"side", "cap", "rim", "inside_side", "inside_cap", "inside_side_on_axis", "cap_on_axis"},
    "sphere_box": {"face", "edge", "corner", "face_near", "inside_+x", "inside_+y", "inside_+z", "inside_-x", "inside_-y", "inside_-z"},
    "capsule_capsule": {"interior", "end", "end_end", "parallel_apart", "parallel_partial", "parallel_overhang_a",
                        "parallel_overhang_b"},
}


# ---------------------------------------------------------------------------------------------------------------------------------
# the allowance: C per pair function, from a float32 evaluation of the reference's own closed forms
# ---------------------------------------------------------------------------------------------------------------------------------
def reference_error(t, w):
    """Largest float32-vs-float64 difference of the reference's answer for one case, in units of eps32 * L: the distances and the
    normal (times its lever)."""
    a64, a32 = t.answer(w, F64), t.answer(w, F32)
    L = t.scale(w)
    if a64.branch != a32.branch or min(a64.switch, a64.switch_rel * L) < 64 * EPS32 * L:
        return 0.0  # the two evaluations may sit on different sides of a switch: not a rounding error of one closed form
    errs = [abs(float(a32.d) - float(a64.d))]
    if a64.all_d is not None and a32.all_d is not None and len(a64.all_d) == len(a32.all_d):
        errs += [abs(float(x) - float(y)) for x, y in zip(a32.all_d, a64.all_d)]
    if a64.n is not None and a32.n is not None:
        lever = L if a64.lever is None else float(a64.lever)
        errs.append(max(float(np.linalg.norm(a32.n.astype(F64) - a64.n)) - a64.bias_n, 0.0) * lever)
    return max(errs) / (EPS32 * L)


_CONSTANTS = None


def derive_constants():
    """pair function -> (C, largest reference error in eps32 * L): C is the smallest power of two with at least 4x headroom."""
    global _CONSTANTS
    if _CONSTANTS is None:
        worst = {}
        for t in tables():
            for w in range(t.worlds):
                worst[t.pair] = max(worst.get(t.pair, 0.0), reference_error(t, w))
        _CONSTANTS = {p: (float(2.0 ** np.ceil(np.log2(max(4.0 * e, 1.0)))), e) for p, e in worst.items()}
    return _CONSTANTS


def allowance(t, w):
    return derive_constants()[t.pair][0] * EPS32 * t.scale(w)


def left_out(t, w):
    a = t.answer(w)
    return bool(min(a.switch, a.switch_rel * t.scale(w)) < allowance(t, w))


# ---------------------------------------------------------------------------------------------------------------------------------
# checking the contacts of a launch
# ---------------------------------------------------------------------------------------------------------------------------------
def decode(model, body_q, flat):
    """The exported flat contact arrays -> per world, a list of dicts (p0, p1 world core points, n, margin0, margin1, d), in row order."""
    from pair_scenes import decode_world

    n = int(np.asarray(flat["count"]).reshape(-1)[0])
    s0, s1 = np.asarray(flat["shape0"])[:n], np.asarray(flat["shape1"])[:n]
    world_of = np.asarray(model.shape_world)
    out = [[] for _ in range(max(model.world_count, 1))]  # (a scene built without replicate: everything global, one world)
    body_q = np.asarray(body_q, dtype=F64).reshape(-1, 7)
    cs = decode_world(model, body_q, s0, s1, flat["point0"][:n], flat["point1"][:n], flat["normal"][:n], flat["margin0"][:n],
                      flat["margin1"][:n])
    for i, (center, nrm, d) in enumerate(cs):
        w = max(world_of[s0[i]], world_of[s1[i]], 0)
        m0, m1 = float(flat["margin0"][i]), float(flat["margin1"][i])
        half = 0.5 * (d + m0 + m1)
        out[w].append(dict(p0=center - nrm * half, p1=center + nrm * half, n=nrm, m0=m0, m1=m1, d=d))
    return out


def check_table(t, contacts, label=""):
    """Hold every world of the table to the generic invariants and, unless left out, to the exact answers.
    -> (largest distance error / allowance, largest normal error / allowance, number of worlds left out).  Raises AssertionError with
    every failing world listed."""
    bad, worst_d, worst_n, n_left = [], 0.0, 0.0, 0
    mA, mB = (float(F32(m)) for m in t.margins)
    for w in range(t.worlds):
        A, B = t.shapes(w)
        ans, allow, L = t.answer(w), allowance(t, w), t.scale(w)
        ra, rb = float(A.radius()), float(B.radius())
        cs = contacts[w]
        where = f"{t.name}[{w}] {t.tags[w]} ({ans.branch})"
        surf = []
        for k, c in enumerate(cs):
            n = c["n"]
            extra = ans.extra_n if k > 0 else 0.0
            if abs(np.linalg.norm(n) - 1.0) > allow / L:
                bad.append(f"{where}: |n| = {np.linalg.norm(n)!r}")
            if abs(c["m0"] - (ra + mA)) > 2 * EPS32 * (ra + mA) or abs(c["m1"] - (rb + mB)) > 2 * EPS32 * (rb + mB):
                bad.append(f"{where}: margins {c['m0']}, {c['m1']} are not radius + margin")
            sa, sb = SDF[t.kind_a](A, c["p0"] + n * ra), SDF[t.kind_b](B, c["p1"] - n * rb)
            if t.pair == "plane_capsule":  # one contact per END SPHERE: the upper one's lowest point is inside the capsule
                h = B.axis * B.size[1]
                sb = min((abs(np.linalg.norm(c["p1"] - n * rb - e) - rb) for e in (B.p + h, B.p - h)))
            # a surface point is its core point moved along n: it inherits n's own tolerance (allowance / lever, the one the normal
            # check uses) times the length of that move.  Where the direction is not unique at all (coincident centres, a centre on an
            # axis: the reference's fallback normal) the surface invariant says nothing and the core points and the distance remain
            turn = 2.0 if (ans.n is None and ans.lever is None and t.kind_a != "plane") else (
                0.0 if ans.lever is None else min(2.0, allow / float(ans.lever) + ans.bias_n))
            tol_a = allow + extra + ans.bias_d + ra * turn
            tol_b = allow + extra + ans.bias_d + (rb if rb > 0 else float(np.linalg.norm(c["p1"] - c["p0"]))) * turn
            if abs(sa) > tol_a or abs(sb) > tol_b:
                bad.append(f"{where}: contact {k} off the surfaces by {sa:.3e} (A), {sb:.3e} (B), allowance {tol_a:.3e}, {tol_b:.3e}")
            for S, r, pt in ((A, ra, c["p0"]), (B, rb, c["p1"])):  # the core points of round shapes: the centre, the axis segment
                if r > 0 and SDF[S.kind](S, pt) + r > allow + extra:
                    bad.append(f"{where}: contact {k}: core point {pt!r} is {SDF[S.kind](S, pt) + r:.3e} off the {S.kind}'s core")
            surf.append(c["d"] + mA + mB)  # n . (p1 - p0) - radii: the surface distance along n
        if left_out(t, w):
            n_left += 1
            if surf and min(surf) < ans.d - allow - ans.bias_d - (2 * ans.switch if np.isfinite(ans.switch) else 0.0):
                bad.append(f"{where}: left out, but a contact at {min(surf)!r} is closer than the exact {ans.d!r}")
            continue
        if ans.count is not None and len(cs) != ans.count:
            bad.append(f"{where}: {len(cs)} contacts, expected {ans.count}")
            continue
        if not cs:
            if ans.count is None:
                bad.append(f"{where}: no contact")
            continue
        e_d = max(abs(min(surf) - ans.d) - ans.bias_d, 0.0)
        if ans.all_d is not None:
            e_d = max([e_d] + [max(abs(x - y) - ans.bias_d, 0.0) for x, y in zip(sorted(surf), ans.all_d)])
        worst_d = max(worst_d, e_d / allow)
        if e_d > allow:
            bad.append(f"{where}: distances {sorted(surf)!r}, exact {ans.d!r} {ans.all_d!r}: off by {e_d / allow:.3g} allowances")
        if min(surf) < ans.d - allow - ans.bias_d:
            bad.append(f"{where}: a contact at {min(surf)!r} is closer than the exact minimum {ans.d!r}")
        if ans.n is not None:
            lever = L if ans.lever is None else float(ans.lever)
            k0 = int(np.argmin(surf)) if t.kind_a != "plane" and ans.all_d is None else 0
            e_n = max(float(np.linalg.norm(cs[k0]["n"] - ans.n)) - ans.bias_n, 0.0) * lever
            worst_n = max(worst_n, e_n / allow)
            if e_n > allow:
                bad.append(f"{where}: normal {cs[k0]['n']!r}, exact {ans.n!r}: off by {e_n / allow:.3g} allowances")
        if ans.corners is not None:  # plane-box: every contact sits on a corner of the box
            for c in cs:
                if min(np.linalg.norm(c["p1"] - q) for q in ans.corners) > allow:
                    bad.append(f"{where}: contact point {c['p1']!r} is no corner of the box")
    assert not bad, f"{label}{t.name}: {len(bad)} failures\n  " + "\n  ".join(bad[:40])
    return worst_d, worst_n, n_left


def report(label, t, ratios):
    print(f"[primitive_exact] {label} {t.name}: worlds {t.worlds}, left out {ratios[2]}, C {derive_constants()[t.pair][0]:g}, "
          f"kernel error / allowance: distance {ratios[0]:.3f}, normal {ratios[1]:.3f}")


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference-held known answers (tests/golden/primitive_known_answers.json) as scenes for the collide kernel
# ---------------------------------------------------------------------------------------------------------------------------------
def known_answer_scene(table_name, row, device=None):
    """-> (model, want...) for one row: shapes of tests/test_oracle_known_answers.py as a one-world scene, gaps wide enough that every
    candidate contact is exported (plane_box: gap 0, the row states the count under a zero margin)."""
    def q_of(axis):
        return nm.quat_between_vectors([0.0, 0.0, 1.0], axis)

    def identity(mat):
        assert np.allclose(np.asarray(mat, F64).reshape(3, 3), np.eye(3)), "tables only use identity rotations"
        return I4

    gap = 0.0 if table_name == "test_plane_box" else 10.0
    kind = table_name[len("test_"):]
    plane, bodies = None, []
    if kind == "plane_sphere":
        n, pp, sp, r, _ = row
        plane, bodies = (pp, q_of(n)), [("sphere", (r, 0, 0), sp, I4)]
    elif kind == "sphere_sphere":
        p1, r1, p2, r2, _ = row
        bodies = [("sphere", (r1, 0, 0), p1, I4), ("sphere", (r2, 0, 0), p2, I4)]
    elif kind in ("sphere_capsule", "sphere_cylinder"):
        sp, sr, cp, axis, cr, ch, _ = row
        bodies = [("sphere", (sr, 0, 0), sp, I4), (kind.split("_")[1], (cr, ch, 0), cp, q_of(axis))]
    elif kind == "capsule_capsule":
        p1, a1, r1, h1, p2, a2, r2, h2, _ = row
        bodies = [("capsule", (r1, h1, 0), p1, q_of(a1)), ("capsule", (r2, h2, 0), p2, q_of(a2))]
    elif kind in ("plane_ellipsoid", "plane_box"):
        n, pp, bp, rot, size = row[:5]
        plane, bodies = (pp, q_of(n)), [(kind.split("_")[1], size, bp, identity(rot))]
    elif kind == "sphere_box":
        sp, sr, bp, rot, size, _ = row
        bodies = [("sphere", (sr, 0, 0), sp, I4), ("box", size, bp, identity(rot))]
    elif kind in ("plane_capsule", "plane_cylinder"):
        n, pp, cp, axis, r, h, _ = row
        plane, bodies = (pp, q_of(n)), [(kind.split("_")[1], (r, h, 0), cp, q_of(axis))]
    else:
        raise ValueError(table_name)
    b = nt.ModelBuilder()
    for k, size, p, q in bodies:
        add_shape(b, b.add_body(xform=[*p, *q], mass=1.0), k, size, 0.0, gap)
    if plane is not None:
        b.add_shape_plane(xform=[*plane[0], *plane[1]], width=0.0, length=0.0, cfg=nt.ModelBuilder.ShapeConfig(margin=0.0, gap=0.0))
    return b.finalize(device=device)


def check_known_answer(table_name, row, cs):
    """The assertions of tests/test_oracle_known_answers.py on the decoded contacts `cs` of known_answer_scene(table_name, row)."""
    kind = table_name[len("test_"):]
    d = [c["d"] for c in cs]
    want = row[-1]
    if kind == "plane_sphere":
        n, pp, sp, r, _ = row
        assert len(cs) == 1 and abs(d[0] - want) < 1e-5
        assert np.allclose(cs[0]["n"], n, atol=1e-6)
        if want < 0:
            p = 0.5 * (cs[0]["p0"] + cs[0]["p1"] - cs[0]["n"] * r)  # the midpoint between the surfaces
            assert np.linalg.norm(p - sp) < r + 0.01
            assert np.dot(p - pp, n) <= np.dot(np.asarray(sp) - pp, n) + 0.01
    elif kind == "sphere_sphere":
        assert len(cs) == 1 and abs(d[0] - want) < 1e-5
        assert abs(np.linalg.norm(cs[0]["n"]) - 1.0) < 1e-5
    elif kind in ("sphere_capsule", "plane_ellipsoid", "sphere_cylinder", "sphere_box"):
        assert len(cs) == 1 and abs(d[0] - want) < 1e-4
    elif kind == "capsule_capsule":
        assert len(cs) >= 1 and abs(d[0] - want) < 1e-4
    elif kind == "plane_capsule":
        assert len(cs) == 2 and abs(min(d) - want) < 1e-4
    elif kind == "plane_box":
        n, want_count = row[0], row[5]
        assert len(cs) == want_count
        for c in cs:
            assert abs(c["d"] - want) < 0.01
            assert np.dot(c["n"], n) > 0.99
    elif kind == "plane_cylinder":
        n = row[0]
        if want <= 0.0:
            assert len(cs) > 0
        if cs:
            assert abs(min(d) - want) < 0.01
        if want <= 0.0:
            assert np.dot(cs[0]["n"], n) > 0.99
    else:
        raise ValueError(table_name)
