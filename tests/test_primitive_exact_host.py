"""The float64 reference of tests/primitive_exact.py checked on its own, without any kernel: against brute force, for the share of cases
it leaves out, for the constants C it yields, and for the branches its tables reach.

Brute force is float64 sampling of the segments / surfaces involved, refined around the best sample (the distances sampled here are
convex in the sampling parameters): every level samples 41 points per parameter and narrows the window to +-2 steps around the best, until
the step is below 1e-9 -- three orders below the smallest allowance (4 * eps32 * 0.02).  Spheres enter through their centres and planes
through their normal, so the sampled objects are segments (capsule axes), box surfaces, cylinder surfaces and ellipsoid surfaces."""
import numpy as np
import pytest

import primitive_exact as PX

BRUTE_TOL = 2e-8  # agreement asked of reference and brute force: the refinement's final step times the surface's curvature, rounded up
N = 41


def refine(f, lo, hi):
    """Minimum of f over the box [lo, hi] (arrays): sample an N^k grid, shrink around the best sample, repeat."""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    lo0, hi0 = lo.copy(), hi.copy()
    best = None
    while np.max(hi - lo) > 1e-9:
        axes = [np.linspace(a, b, N) for a, b in zip(lo, hi)]
        grid = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, len(lo))
        vals = f(grid)
        k = int(np.argmin(vals))
        best = float(vals[k])
        step = (hi - lo) / (N - 1)
        lo, hi = np.maximum(grid[k] - 2 * step, lo0), np.minimum(grid[k] + 2 * step, hi0)
    return best


def segment_points(S, s):
    """Points of a capsule's axis at parameters s in [-1, 1]."""
    return S.p + np.outer(s, S.axis * S.size[1])


def brute_point_segment(x, S):
    return refine(lambda g: np.linalg.norm(segment_points(S, g[:, 0]) - x, axis=1), [-1], [1])


def brute_segment_segment(A, B):
    """Nested: for every sampled point of A's axis the distance to B's axis by the same refinement (one window per point), and the
    refinement of that over A's axis.  (A joint refinement over both parameters loses the minimum of nearly parallel axes: on a coarse
    grid the best sample is the one nearest the valley's floor, anywhere along it.)"""
    def to_b(g):
        x = segment_points(A, g[:, 0])
        lo, hi = np.full(len(x), -1.0), np.full(len(x), 1.0)
        while np.max(hi - lo) > 1e-9:
            ts = lo[:, None] + (hi - lo)[:, None] * np.linspace(0, 1, N)[None]
            d = np.linalg.norm(x[:, None, :] - (B.p + ts[..., None] * (B.axis * B.size[1])), axis=2)
            k = np.argmin(d, axis=1)
            best, step = ts[np.arange(len(x)), k], (hi - lo) / (N - 1)
            lo, hi = np.maximum(best - 2 * step, -1), np.minimum(best + 2 * step, 1)
        return d[np.arange(len(x)), k]

    return refine(to_b, [-1], [1])


def box_faces(B):
    """The six faces as (origin, u, v): points origin + a u + b v, a, b in [-1, 1], in the world."""
    out = []
    for k in range(3):
        i, j = (k + 1) % 3, (k + 2) % 3
        for sg in (1, -1):
            out.append((B.p + B.R[:, k] * sg * B.size[k], B.R[:, i] * B.size[i], B.R[:, j] * B.size[j]))
    return out


def brute_point_box_surface(x, B):
    return min(refine(lambda g, o=o, u=u, v=v: np.linalg.norm(o + np.outer(g[:, 0], u) + np.outer(g[:, 1], v) - x, axis=1), [-1, -1], [1, 1])
               for o, u, v in box_faces(B))


def cylinder_surface(B, part, g):
    """part 0: the side (angle, height); 1 / 2: the caps (angle, radius)."""
    ex, ey, ez = B.R[:, 0], B.R[:, 1], B.R[:, 2]
    ang = g[:, 0]
    ring = np.outer(np.cos(ang), ex) + np.outer(np.sin(ang), ey)
    if part == 0:
        return B.p + ring * B.size[0] + np.outer(g[:, 1] * B.size[1], ez)
    return B.p + ring * (g[:, 1:2] * 0.5 + 0.5) * B.size[0] + ez * B.size[1] * (1 if part == 1 else -1)


def brute_over_cylinder(B, f):
    # (the window may leave [-pi, pi]: refine clips to the start window, so the angle is offered over two turns)
    return min(refine(lambda g, part=part: f(cylinder_surface(B, part, g)), [-2 * np.pi, -1], [2 * np.pi, 1]) for part in (0, 1, 2))


def ellipsoid_surface(B, g):
    th, ph = g[:, 0], g[:, 1]
    l = np.stack([np.cos(th) * np.cos(ph), np.sin(th) * np.cos(ph), np.sin(ph)], axis=1) * B.size
    return B.p + l @ B.R.T


def brute(t, w):
    """The exact answer's distance by brute force (None where the table's answer is not a plain distance between the sampled objects)."""
    A, B = t.shapes(w)
    ans = t.answer(w)
    plane_height = lambda X: (X - A.p) @ A.axis  # noqa: E731
    if t.pair == "sphere_sphere":
        return float(np.linalg.norm(B.p - A.p) - A.size[0] - B.size[0])
    if t.pair == "plane_sphere":
        return float(plane_height(B.p[None])[0] - B.size[0])
    if t.pair == "plane_capsule":
        return refine(lambda g: plane_height(segment_points(B, g[:, 0])), [-1], [1]) - B.size[0]
    if t.pair == "sphere_capsule":
        return brute_point_segment(A.p, B) - A.size[0] - B.size[0]
    if t.pair == "capsule_capsule":
        return brute_segment_segment(A, B) - A.size[0] - B.size[0]
    if t.pair == "plane_box":
        return float(min(plane_height(np.array(PX.box_corners(B)))))  # (a linear function over a polytope: a corner)
    if t.pair == "plane_ellipsoid":
        return refine(lambda g: plane_height(ellipsoid_surface(B, g)), [-2 * np.pi, -np.pi / 2], [2 * np.pi, np.pi / 2])
    if t.pair == "plane_cylinder":
        return brute_over_cylinder(B, plane_height)
    inside = PX.SDF[t.kind_b](B, A.p) < 0  # sphere against box / cylinder: the centre's distance to the surface, signed
    if t.pair == "sphere_box":
        dist = brute_point_box_surface(A.p, B)
    else:
        dist = brute_over_cylinder(B, lambda X: np.linalg.norm(X - A.p, axis=1))
    assert inside == ans.branch.startswith("inside")
    return (-dist if inside else dist) - A.size[0]


@pytest.mark.parametrize("name", PX.TABLE_NAMES)
def test_reference_against_brute_force(name):
    """A sample of every table: every 7th world, and the first world of every tag."""
    t = PX.table(name)
    first = {t.tags.index(tag) for tag in set(t.tags)}
    worst = 0.0
    for w in sorted(first | set(range(0, t.worlds, 7))):
        got, want = float(t.answer(w).d), brute(t, w)
        worst = max(worst, abs(got - want))
        assert abs(got - want) <= BRUTE_TOL, f"{name}[{w}] {t.tags[w]} ({t.answer(w).branch}): reference {got!r}, brute force {want!r}"
        assert BRUTE_TOL < 0.25 * PX.allowance(t, w) or PX.allowance(t, w) < 1e-7, "the brute force does not bound the answer within the allowance"
    print(f"[primitive_exact] {name}: reference vs brute force, worst {worst:.2e}")


def test_surface_functions():
    """The surface functions against points of known distance: a point moved off a sampled surface point along the outward normal."""
    B = PX.Shape("box", (0.3, 0.2, 0.1), [0.1, -0.2, 0.3, *PX.QGEN[0]])
    C = PX.Shape("cylinder", (0.2, 0.3, 0.0), [0.1, -0.2, 0.3, *PX.QGEN[1]])
    E = PX.Shape("ellipsoid", (0.3, 0.2, 0.1), [0.1, -0.2, 0.3, *PX.QGEN[0]])
    K = PX.Shape("capsule", (0.1, 0.4, 0.0), [0.1, -0.2, 0.3, *PX.QGEN[1]])
    rng = np.random.default_rng(0)
    for x in rng.uniform(-0.6, 0.6, size=(40, 3)) + B.p:
        assert abs(abs(PX.sdf_box(B, x)) - brute_point_box_surface(x, B)) < BRUTE_TOL
        assert abs(abs(PX.sdf_cylinder(C, x)) - brute_over_cylinder(C, lambda X: np.linalg.norm(X - x, axis=1))) < BRUTE_TOL
        assert abs(PX.sdf_capsule(K, x) - (brute_point_segment(x, K) - 0.1)) < BRUTE_TOL
    for g in rng.uniform(-1.5, 1.5, size=(40, 2)):
        x = ellipsoid_surface(E, g[None])[0]
        assert abs(PX.ellipsoid_residual(E, x)) < 1e-12
        n = E.R @ (E.local(x) / E.size ** 2)
        n /= np.linalg.norm(n)
        h, sp = PX.ellipsoid_support(E, n)  # the support point in the direction of a surface point's normal is that point
        assert np.linalg.norm(sp - x) < 1e-12 and abs(h - n @ (x - E.p)) < 1e-12
        assert abs(PX.sdf_ellipsoid(E, x + n * 1e-6) - 1e-6) < 1e-10  # (first order: exact to O(distance^2))


@pytest.mark.parametrize("name", PX.TABLE_NAMES)
def test_left_out_share(name):
    """At most 2 % of a table may sit closer to a branch switch than its allowance -- decided by the reference alone."""
    t = PX.table(name)
    n = sum(PX.left_out(t, w) for w in range(t.worlds))
    print(f"[primitive_exact] {name}: {n} of {t.worlds} worlds left out")
    assert t.worlds <= 300 and n <= PX.LEFT_OUT_CAP * t.worlds


# what derive_constants() must come out as: written down so that a change of the tables or of the reference that moves a constant is seen
CONSTANTS = {"sphere_sphere": 4, "plane_sphere": 4, "plane_capsule": 16, "plane_box": 16, "plane_ellipsoid": 2, "plane_cylinder": 8,
             "sphere_capsule": 8, "sphere_cylinder": 8, "sphere_box": 8, "capsule_capsule": 16}


def test_constants():
    """C per pair function: the smallest power of two with 4x headroom over the reference's own float32-vs-float64 error on the tables."""
    got = PX.derive_constants()
    for pair, (c, err) in sorted(got.items()):
        print(f"[primitive_exact] {pair}: reference float32 error {err:.3f} eps32 L, C = {c:g}")
        assert c >= 4 * err and (c / 2 < 4 * err or c == 1.0) and np.log2(c) == int(np.log2(c))
    assert {p: c for p, (c, _) in got.items()} == CONSTANTS


def test_branches_reached():
    reached = {}
    for t in PX.tables():
        for w in range(t.worlds):
            if not PX.left_out(t, w):
                reached.setdefault(t.pair, set()).add(t.answer(w).branch)
    for pair, need in PX.REQUIRED_BRANCHES.items():
        assert need <= reached[pair], f"{pair}: no case reaches {sorted(need - reached[pair])}"
    # the capsule sweep: every angle on both sides of the parallel switch, the closest approach interior, at an end and past it
    for t in PX.tables():
        if t.pair == "capsule_capsule":
            for angle in PX.SWEEP:
                for tag in ("interior", "at_end", "past_end"):
                    assert "sweep_%s_%g" % (tag, angle) in t.tags and "sweep_conv_%s_%g" % (tag, angle) in t.tags
            assert {"crossed", "skew", "t_shape", "colinear", "parallel_centred", "parallel_partial", "parallel_apart"} <= set(t.tags)
