"""World isolation and reset after divergence: the cases shared by tests/test_gpu_world_isolation.py (the
device) and tests/test_world_isolation_emu.py (the kernel sources on the CPU).

The contract: what a world computes does not depend on what the other worlds of its launch hold, and a world that was reset is
indistinguishable from one that never misbehaved.  Every case makes two runs of one scene: run A undisturbed, run B with other inputs in
the AGGRESSOR worlds.  Whatever run B writes for a VICTIM world (every world that is no aggressor) equals run A bit for bit: uint32
views, no tolerance anywhere.  The aggressor rows are never compared, except that they differ where a case says so.

This module holds what both files need and nothing that touches a device: the aggressor masks, the disturbed start arrays (built from the
scene's own arrays and posed through eval_fk_numpy, so that joint_q and body_q agree), the parameter edit, and the comparison of
snapshots.  A snapshot is a dict: name -> array [world, ...] or a list with one array per world (the contact rows)."""
import numpy as np

import newton_amd as nt
from newton_amd import JointType

WORLDS = 37  # ragged last tile at 4, 8, 16 and 32 worlds per workgroup
STATE_FIELDS = ("body_q", "body_qd", "joint_q", "joint_qd")
CONTROL_FIELDS = ("joint_f", "joint_target_q", "joint_target_qd")
FLAT = ("shape0", "shape1", "point0", "point1", "offset0", "offset1", "normal", "margin0", "margin1")
FINITE_KINDS = ("fast", "far", "deep", "limits")
NON_FINITE = "nonfinite"  # (the emulated file only: NaN position, Inf velocity, zero quaternion)
_SCALAR = (int(JointType.REVOLUTE), int(JointType.PRISMATIC), int(JointType.D6))


GENERIC = "16,512,1,1,0,0"  # NT_XPBD_CFG: the generic instance of the fused XPBD rollout forced (the string of tests/test_gpu_spec_tile.py)


def xpbd_cfg(cfg):
    """tests/test_gpu_spec_tile.py's context manager for NT_XPBD_CFG (None: the default dispatch), shared by the device and the emulated file."""
    from test_gpu_spec_tile import _cfg

    return _cfg(cfg)


def masks(n):
    """name -> bool [n], True = aggressor.  "mod3": w % 3 == 1; "alone": everything but three victims (first, 20/36 of the way, last:
    {0, 20, 36} of 37 worlds), so that each victim is alone among aggressors and one sits in the ragged tile; "pair": only two
    aggressors ({17, 36} of 37), one of them the last world.  Masks without an aggressor or without a victim (tiny scenes) are left out."""
    w = np.arange(n)
    alone = np.ones(n, bool)
    alone[[0, (20 * n) // 36 if n > 1 else 0, n - 1]] = False
    pair = np.zeros(n, bool)
    pair[[(17 * n) // 37, n - 1]] = True
    out = {"mod3": w % 3 == 1, "alone": alone, "pair": pair}
    return {k: m for k, m in out.items() if m.any() and not m.all()}


def combos(n, kinds):
    """Every kind under every mask."""
    return [(kind, name, m) for kind in kinds for name, m in masks(n).items()]


def rotated(n, kinds):
    """Every kind once and every mask at least once, for the heavy scenes: kind i under mask i (mod the number of masks)."""
    ms = list(masks(n).items())
    kinds = list(kinds)
    k = max(len(kinds), len(ms))
    return [(kinds[i % len(kinds)], *ms[i % len(ms)]) for i in range(k)]


def scene(name, n, device=None):
    """The smallest scenes of tests/scenes.py; the quadrupeds lowered by 0.24 so that every world stands in the ground."""
    import scenes as sc

    if name == "quadruped":
        return lower(sc.quadruped_scene(n, device=device, seed=5), 0.24)
    if name == "quadruped_low":  # every world's feet IN the ground from the first step on (the height jitter is 0 .. 0.05): contact forces
        return lower(sc.quadruped_scene(n, device=device, seed=5), 0.30)
    if name == "quadruped_convex":
        return lower(sc.quadruped_convex_scene(n, device=device, seed=5), 0.24)
    if name == "box_stack":
        return sc.box_stack_scene(n, device=device)
    if name == "mixed":
        return sc.mixed_primitive_scene(n, device=device)
    if name == "hull_bin":
        return sc.hull_bin_scene(n, 40, device=device)
    if name == "multi_art":
        return sc.multi_articulation_scene(n, device=device)
    return {"joint_zoo": sc.joint_zoo_scene, "d6_angular": sc.d6_angular_scene, "free_child": sc.free_child_scene}[name](n, device=device)


# how far "deep" lowers the first root of a world (the k-th: k + 1 times as far), chosen per scene so that its contact count changes.
# The box stack touches with all 32 contacts however hard it is squeezed, and the mixed primitives gain a contact in one world and lose
# one in the next when pressed down: there the roots are lifted instead (a negative depth), which empties the aggressors' contact lists
DEPTH = {"quadruped": 0.15, "quadruped_low": 0.15, "quadruped_convex": 0.15, "box_stack": -0.2, "mixed": -0.05, "hull_bin": 0.003, "multi_art": 1.0}


# ... and "pressed" is the gaining counterpart on the mixed primitives: 0.02 (k + 1) m down, where no world loses a contact and the
# aggressors of every mask gain some (a neighbour with MORE contacts in the convex tile)
PRESSED = {"mixed": 0.02}


def depth(name, kind):
    return PRESSED[name] if kind == "pressed" else DEPTH.get(name, 0.1)


def kinds_for(model, contacts=True):
    """The finite aggressor kinds the scene has the joints for ("far" and "deep" need a free root and something to touch, "limits" a
    revolute / prismatic / D6 joint)."""
    t = model.env
    jt, parent = np.asarray(t.joint_type), np.asarray(t.joint_parent)
    ndof = np.asarray(t.joint_lin_count) + np.asarray(t.joint_ang_count)
    free_root = bool(np.any((jt == int(JointType.FREE)) & (parent < 0)))
    scalar = bool(np.any(np.isin(jt, _SCALAR) & (ndof > 0)))
    return tuple(k for k in FINITE_KINDS if (k == "fast" or (k in ("far", "deep") and free_root and contacts and t.np > 0)
                                             or (k == "limits" and scalar)))


def lower(model, dz):
    """Feet in the ground (as tests/test_gpu_spec_tile.py): every world's root lowered by dz, posed through eval_fk_numpy."""
    model.joint_q.reshape(model.world_count, -1)[:, 2] -= dz
    model.body_q, model.body_qd = nt.articulation.eval_fk_numpy(model, model.joint_q, model.joint_qd)
    return model


def start_arrays(model, kind=None, aggressors=None, depth=0.1):
    """The start of a run: the model's own state and control arrays (kind None: run A), or those with the aggressor worlds disturbed.
      fast       root bodies at some 370 m/s and 37 rad/s; a scene without a free root: joint rates of +-1e4
      far        root bodies moved by 1e4 m along every axis (off the ground: the world loses its contacts)
      deep       root body k lowered by depth * (k + 1): more of the world in the ground (lifted out of it by a negative depth)
      limits     revolute / prismatic / D6 coordinates at +-5 (far beyond every limit), joint_f, joint_target_q and _qd of 1e3
      nonfinite  NaN in the first coordinate, Inf in the second velocity, a zero quaternion on the first free root
    Only the aggressor worlds' rows change; their body_q / body_qd come from eval_fk_numpy on the new joint arrays."""
    out = {k: np.array(getattr(model, k), dtype=np.float32, copy=True) for k in STATE_FIELDS + CONTROL_FIELDS}
    if kind is None:
        return out
    t, E = model.env, model.env.env_count
    a = np.flatnonzero(aggressors)
    jq, jqd = out["joint_q"].reshape(E, -1), out["joint_qd"].reshape(E, -1)
    jt, parent = np.asarray(t.joint_type), np.asarray(t.joint_parent)
    qs, ds, ts = np.asarray(t.joint_q_start), np.asarray(t.joint_qd_start), np.asarray(t.joint_tq_start)
    ndof = np.asarray(t.joint_lin_count) + np.asarray(t.joint_ang_count)
    roots = [j for j in range(t.nj) if jt[j] == int(JointType.FREE) and parent[j] < 0]
    scalar = [j for j in range(t.nj) if jt[j] in _SCALAR and ndof[j] > 0]
    sign = lambda n, j: np.where((np.arange(n) + j) % 2 == 0, 1.0, -1.0).astype(np.float32)  # noqa: E731
    if kind == "fast":
        for j in roots:
            jqd[a, ds[j]:ds[j] + 6] += np.array([300.0, -200.0, 100.0, 30.0, -20.0, 10.0], np.float32)
        for j in (() if roots else scalar):
            jqd[a, ds[j]:ds[j] + ndof[j]] = 1.0e4 * sign(ndof[j], j)
    elif kind == "far":
        assert roots, "far: the scene has no free root to move"
        for j in roots:
            jq[a, qs[j]:qs[j] + 3] += np.array([1.0e4, -1.0e4, 1.0e4], np.float32)
    elif kind in ("deep", "pressed"):
        assert roots, "deep: the scene has no free root to lower"
        for k, j in enumerate(roots):
            jq[a, qs[j] + 2] -= np.float32(depth * (k + 1))
    elif kind == "limits":
        assert scalar, "limits: the scene has no revolute / prismatic / D6 joint"
        jf, tq, tqd = (out[k].reshape(E, -1) for k in CONTROL_FIELDS)
        jf[a] = 1.0e3
        for j in scalar:
            jq[a, qs[j]:qs[j] + ndof[j]] = 5.0 * sign(ndof[j], j)
            tq[a, ts[j]:ts[j] + ndof[j]] = 1.0e3
            tqd[a, ds[j]:ds[j] + ndof[j]] = 1.0e3
    elif kind == NON_FINITE:
        jq[a, 0], jqd[a, min(1, jqd.shape[1] - 1)] = np.nan, np.inf
        for j in roots[:1]:
            jq[a, qs[j] + 3:qs[j] + 7] = 0.0
    else:
        raise ValueError(kind)
    with np.errstate(all="ignore"):
        bq, bqd = nt.articulation.eval_fk_numpy(model, out["joint_q"], out["joint_qd"])
    rows = aggressors.repeat(t.nb)
    out["body_q"].reshape(-1, 7)[rows], out["body_qd"].reshape(-1, 6)[rows] = bq[rows], bqd[rows]
    return out


_PARAMS = (("body_mass", 50.0), ("body_inertia", 50.0), ("body_inv_mass", 1.0 / 50.0), ("body_inv_inertia", 1.0 / 50.0))


def pristine_params(model):
    return {k: np.array(getattr(model, k), copy=True) for k in [n for n, _ in _PARAMS] + ["gravity"]}


def edit_params(model, aggressors, pristine):
    """The "params" kind: from the `pristine` (uniform) parameters, mass and inertia x 50 and another gravity in the aggressor worlds,
    then notify_model_changed.  The model then takes the per-environment parameter tile; the victims' parameter rows keep their bits."""
    t = model.env
    for k, v in pristine.items():
        getattr(model, k)[...] = v
    rows = aggressors.repeat(t.nb)
    for name, f in _PARAMS:
        arr = getattr(model, name)
        arr[rows] = (arr[rows] * np.float32(f)).astype(np.float32)
    for w in np.flatnonzero(aggressors):
        model.set_gravity(np.array([1.5, -0.5, -3.0], np.float32), world=int(w))
    model.notify_model_changed()
    return model


# -- snapshots ---------------------------------------------------------------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def by_world(arr, E):
    return np.asarray(arr).reshape(E, -1)


def contact_rows(model, flat, extra=None):
    """The live rows of the flat contact arrays (`flat`: name -> numpy array, "count" included), split by world in row order.  A row
    belongs to the world of its non-global shape: that holds in the append order (worlds' analytic rows, then their convex rows) and in
    the key-sorted order alike, where a world's rows are not one contiguous range.  `extra`: further per-row arrays (force).
    -> (snapshot entries name -> list of per-world arrays, rows: list of per-world flat row indices)"""
    E = model.env.env_count
    n = int(np.asarray(flat["count"]).reshape(-1)[0])
    world_of = np.asarray(model.shape_world)
    s0, s1 = np.asarray(flat["shape0"])[:n], np.asarray(flat["shape1"])[:n]
    assert n == 0 or (s0.min() >= 0 and s1.min() >= 0), "a live row without its shapes"
    w = np.where(world_of[s0] >= 0, world_of[s0], world_of[s1]) if n else np.zeros(0, np.int64)
    assert n == 0 or w.min() >= 0, "a contact between two global shapes"
    rows = [np.flatnonzero(w == e) for e in range(E)]
    snap = {"contact_" + k: [np.asarray(flat[k])[r] for r in rows] for k in FLAT}
    for k, v in (extra or {}).items():
        snap["contact_" + k] = [np.asarray(v)[r] for r in rows]
    return snap, rows


def match_ordinals(match_index, rows_now, rows_prev, n_prev):
    """rigid_contact_match_index (previous-frame flat row, or a negative code) per world, the row turned into its ordinal among the
    previous frame's rows of the SAME world -- a match into another world's rows is an isolation defect in itself."""
    ordinal, owner = np.full(max(n_prev, 1), -1, np.int64), np.full(max(n_prev, 1), -1, np.int64)
    for e, r in enumerate(rows_prev):
        ordinal[r], owner[r] = np.arange(len(r)), e
    out = []
    for e, r in enumerate(rows_now):
        m = np.asarray(match_index)[r].astype(np.int64)
        hit = m >= 0
        assert np.all(m[hit] < n_prev) and np.all(owner[m[hit]] == e), f"world {e}: a contact matched a row of another world"
        out.append(np.where(hit, ordinal[m.clip(min=0)], m))
    return out


def differing_worlds(A, B, worlds):
    """[(name, world)] of every snapshot entry whose bits differ in one of `worlds`."""
    assert set(A) == set(B), (sorted(A), sorted(B))
    bad = []
    for k in sorted(A):
        for w in np.flatnonzero(worlds):
            x, y = bits(A[k][w]), bits(B[k][w])
            if x.shape != y.shape or not np.array_equal(x, y):
                bad.append((k, int(w)))
    return bad


def assert_isolated(A, B, aggressors, what, differ=STATE_FIELDS):
    """The victims of run B carry run A's bits in every entry; the aggressors differ in one of `differ` (None: not asked)."""
    bad = differing_worlds(A, B, ~aggressors)
    assert not bad, f"{what}: victim worlds differ from the undisturbed run in {bad[:12]} ({len(bad)} entries)"
    if differ is not None:
        keys = [k for k in differ if k in A]
        assert keys and differing_worlds({k: A[k] for k in keys}, {k: B[k] for k in keys}, aggressors), \
            f"{what}: the aggressor worlds came out as in the undisturbed run (the case disturbs nothing)"


def assert_victims_in_contact(A, aggressors, what):
    n = np.asarray(A["contact_count"]).reshape(-1)
    assert np.all(n[~aggressors] >= 1), f"{what}: victim worlds without a live contact: {np.flatnonzero((n < 1) & ~aggressors)}"


def assert_contact_totals_differ(A, B, aggressors, what):
    a, b = (int(np.asarray(S["contact_count"]).reshape(-1)[aggressors].sum()) for S in (A, B))
    assert a != b, f"{what}: the aggressors hold {b} contacts, as in the undisturbed run"
    assert "pressed" not in what or b > a, f"{what}: the aggressors hold {b} contacts, no more than the {a} of the undisturbed run"
