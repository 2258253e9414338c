"""The key-ordered contact export and the matching report over the world groups of a heterogeneous model (newton_amd/hetero.py,
nt_contacts_export_sorted_groups / _match_report_groups / _order_save_groups in include/newton_hip_contacts.h).

CollisionPipeline(deterministic=True) on a model whose worlds differ in topology gives the default pipeline's raw heterogeneous export
under a stable sort on (shape0 << 32 | shape1) in global shape ids, bit for bit; restricted to one world group it is that group's own
deterministic export.  Matching keeps one matcher per group: rigid_contact_match_index is the group's match moved to global positions,
the new / broken lists follow their definitions over the global arrays, and a matching frame records into a hipGraph."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

FIELDS = ("shape0", "shape1", "point0", "point1", "offset0", "offset1", "normal", "margin0", "margin1")
PROPS = ("stiffness", "damping", "friction")


def _emulated():
    import torch

    return getattr(torch.cuda, "_newton_emulated", False)


def _needs_device():
    import torch

    if not torch.cuda.is_available() or _emulated():
        pytest.skip("needs the device (not emulated)")


def _mesh_model():
    """world groups with a vertex leg each (mesh box | mesh sphere + primitive box, alternating) and a global ground plane: rows,
    slot contacts and a world -1 shape (as tests/test_gpu_mesh_plane_pipeline.py::test_mesh_worlds_inside_heterogeneous_models)"""
    import newton_amd as nt

    hull = nt.Mesh.create_box(0.1, 0.08, 0.05)
    box_mesh = nt.Mesh(np.concatenate([hull.vertices] * 3), hull.indices)
    sphere_mesh = nt.Mesh.create_sphere(0.08, 8, 10)

    def env(mesh, h, extra=False):
        e = nt.ModelBuilder()
        e.default_shape_cfg.gap = 0.004
        b = e.add_body(xform=[0, 0, h - 0.0008, 0, 0, 0, 1])
        e.add_shape_mesh(b, mesh=mesh)
        if extra:
            b2 = e.add_body(xform=[0.5, 0, 0.05 - 0.0005, 0, 0, 0, 1])
            e.add_shape_box(b2, hx=0.05, hy=0.05, hz=0.05)
            e.add_shape_collision_filter_pair(0, 1)
        return e

    scene = nt.ModelBuilder()
    scene.default_shape_cfg.gap = 0.004
    for k in range(4):
        scene.add_world(env(box_mesh, 0.05) if k % 2 == 0 else env(sphere_mesh, 0.08, extra=True))
    scene.add_ground_plane()
    return scene.finalize(device="cuda:0")


def _model(name, small=None):
    """-> (model, CollisionPipeline kwargs)"""
    from test_heterogeneous_worlds import LAYOUT, mixed_model

    small = _emulated() if small is None else small
    if name == "mixed":  # quadrupeds | box stacks | pendulums (+ the ground plane)
        layout = (("quadruped", 1), ("boxes3", 2), ("pendulum", 1), ("boxes2", 1)) if small else LAYOUT
        return mixed_model(layout, device="cuda:0"), {}
    if name == "mesh":
        return _mesh_model(), {"broad_phase": "nxn"}
    raise KeyError(name)


def _host(c, name):
    v = getattr(c, "rigid_contact_" + name)
    return None if v is None else v.cpu().numpy()


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def _count(c):
    return int(c.rigid_contact_count.cpu().numpy()[0])


def _world(model, s0, s1):
    sw = np.asarray(model.shape_world)
    return np.maximum(sw[s0], sw[s1])


def _set_props(contacts, seed):
    rng = np.random.default_rng(seed)
    for c in contacts.parts:
        if c._slots:
            e = c.model.env.env_count
            c.set_slot_properties(*(rng.uniform(0.5, 2.0, size=(c._slots, e)).astype(np.float32) for _ in range(3)))


def _raw_props(raw, name):
    """a property of the default pipeline's raw export (its groups' views in the raw heterogeneous order)"""
    return raw._rows(lambda c: getattr(c, "rigid_contact_" + name)).cpu().numpy()


@pytest.mark.parametrize("name", ["mixed", "mesh"])
def test_sorted_export_is_a_stable_sort_of_the_raw_export(name):
    """Two frames: every field (per-contact properties included), the count, the fill beyond it and export_order() == the raw
    heterogeneous export under a numpy stable argsort of the global key; no row outside the buckets."""
    import torch

    import newton_amd as nt

    model, kw = _model(name)
    raw_pipe, det_pipe = nt.CollisionPipeline(model, **kw), nt.CollisionPipeline(model, deterministic=True, **kw)
    assert det_pipe.deterministic and not raw_pipe.deterministic
    raw, det = raw_pipe.contacts(per_contact_shape_properties=True), det_pipe.contacts(per_contact_shape_properties=True)
    _set_props(raw, 1)
    _set_props(det, 1)
    solver = nt.solvers.SolverXPBD(model, iterations=2)
    s0, s1 = model.state(), model.state()
    moved_total, world_glob = 0, False
    for _ in range(2):
        raw_pipe.collide(s0, raw)
        det_pipe.collide(s0, det)
        torch.cuda.synchronize()
        n = _count(raw)
        assert n > 0 and _count(det) == n
        r0, r1 = _host(raw, "shape0")[:n], _host(raw, "shape1")[:n]
        order = np.argsort(r0.astype(np.int64) * (1 << 32) + r1, kind="stable")
        for f in FIELDS:
            a, b = _bits(_host(raw, f)), _bits(_host(det, f))  # (the raw views hold the n contacts, the sorted ones every entry)
            assert len(a) == n and b.shape[0] == max(det.rigid_contact_max, 1) and a.shape[1:] == b.shape[1:], f
            assert np.array_equal(a[:n][order], b[:n]), (name, f)
            assert np.array_equal(b[n:], np.full_like(b[n:], -1 if f in ("shape0", "shape1") else 0)), (name, f)
        for f in PROPS:
            b = _bits(_host(det, f))
            assert np.all(b[n:] == 0), (name, f)
            # (the raw export places slot overrides in (env, slot) order of the live slots, which is their contacts' order only
            # while no env mixes analytic and convex contacts -- true of this layout; the mixed one is checked per group below)
            if name == "mesh":
                assert np.array_equal(_bits(_raw_props(raw, f))[order], b[:n]), (name, f)
        eo = det.export_order()
        assert (eo is None and n <= 1) or np.array_equal(eo.cpu().numpy(), order)
        assert int(det.order_unmatched_rows.cpu().numpy()[0]) == 0
        moved_total += int((order != np.arange(n)).sum())
        world_glob |= bool(np.any(np.asarray(model.shape_world)[r0] == -1))
        solver.step(s0, s1, None, raw, 1.0 / 600.0)
        s0, s1 = s1, s0
    assert moved_total > 0 and world_glob  # (really re-ordered across groups; the ground plane's contacts are in)


def test_sorted_export_of_an_empty_frame():
    """No contact anywhere, after a frame that had contacts: count 0, every entry filled, export_order() None."""
    import torch

    import newton_amd as nt

    model, kw = _model("mixed", small=True)
    pipe = nt.CollisionPipeline(model, deterministic=True, **kw)
    c, s = pipe.contacts(), model.state()
    pipe.collide(s, c)
    assert _count(c) > 0
    far = model.state()
    q = far.body_q.clone()
    q[:, 2] += 100.0 + 10.0 * torch.arange(q.shape[0], dtype=q.dtype, device=q.device)  # (apart, and off the ground)
    far.body_q = q
    pipe.collide(far, c)
    torch.cuda.synchronize()
    assert _count(c) == 0
    assert np.all(_host(c, "shape0") == -1) and np.all(_host(c, "shape1") == -1) and np.all(_host(c, "normal") == 0.0)
    assert c.export_order() is None


def _group_rows(model, g, det):
    """positions of group g's contacts in the global arrays (ascending)"""
    b, e = model.world_groups.ranges[g]
    n = _count(det)
    w = _world(model, _host(det, "shape0")[:n], _host(det, "shape1")[:n])
    return np.flatnonzero((w >= b) & (w < e))


def _check_group_geometry(model, g, det, own, fields=FIELDS):
    """the global arrays restricted to group g == the group's own deterministic export, shape ids translated"""
    gid = np.asarray(model.world_groups.parts[g]._global_shape_ids)
    pos = _group_rows(model, g, det)
    m = _count(own)
    assert len(pos) == m, (g, len(pos), m)
    for f in fields:
        a = _host(own, f)[:m]
        if f in ("shape0", "shape1"):
            a = gid[a]
        assert np.array_equal(_bits(_host(det, f))[pos], _bits(a)), (g, f)
    return pos


@pytest.mark.parametrize("name", ["mixed", "mesh"])
def test_sorted_export_restricted_to_a_group_is_the_groups_own(name):
    import torch

    import newton_amd as nt

    model, kw = _model(name)
    det_pipe = nt.CollisionPipeline(model, deterministic=True, **kw)
    det, s = det_pipe.contacts(per_contact_shape_properties=True), model.state()
    _set_props(det, 2)
    parts = model.world_groups.parts
    own = [nt.CollisionPipeline(p, deterministic=True, **kw) for p in parts]
    own_c = [p.contacts(per_contact_shape_properties=True) for p in own]
    for g, c in enumerate(own_c):  # (the same per-slot overrides as the grouped contacts)
        c._prop.copy_(det.parts[g]._prop)
    det_pipe.collide(s, det)
    for g, (p, c) in enumerate(zip(own, own_c)):
        p.collide(s.parts[g], c)
    torch.cuda.synchronize()
    total = 0
    for g in range(len(parts)):
        total += len(_check_group_geometry(model, g, det, own_c[g], FIELDS + PROPS))
    assert total == _count(det) > 0


def check_matching_against_the_groups(mode, small=None):
    """Four XPBD frames with a reset_contact_matching(mask) on worlds of two groups at frame 2: match_index == every group's own
    matcher (a standalone pipeline on the same states) composed with the global positions of this frame and the previous one;
    "sticky": the geometry is the groups' own bit for bit; "latest": new / broken follow their definitions."""
    import torch

    import newton_amd as nt
    from newton_amd.hetero import _split_world_mask

    model, kw = _model("mixed", small)
    report = mode == "latest"
    thr = {"contact_matching_pos_threshold": 0.004, "contact_matching_normal_dot_threshold": 0.9}
    pipe = nt.CollisionPipeline(model, contact_matching=mode, contact_report=report, **kw, **thr)
    assert pipe.deterministic
    c, solver = pipe.contacts(), nt.solvers.SolverXPBD(model, iterations=2)
    groups = model.world_groups
    own = [nt.CollisionPipeline(p, contact_matching=mode, contact_report=report, **kw, **thr) for p in groups.parts]
    own_c = [p.contacts() for p in own]
    st = [model.state(), model.state()]
    W = model.world_count
    reset_worlds = [groups.ranges[0][0], groups.ranges[-1][0]]  # (worlds of two different groups)
    prev, prev_pos, matched = None, None, 0
    for frame in range(4):
        st[0].clear_forces()
        if frame == 2:
            mask = np.zeros(W + 1, bool)  # (the reference's world_count + 1 form)
            mask[reset_worlds] = True
            pipe.reset_contact_matching(mask)
            for p, mk in zip(own, _split_world_mask(mask, groups)):
                p.reset_contact_matching(mk)
        pipe.collide(st[0], c)
        for g, (p, oc) in enumerate(zip(own, own_c)):
            p.collide(st[0].parts[g], oc)
        torch.cuda.synchronize()
        n = _count(c)
        m = c.rigid_contact_match_index.cpu().numpy()
        assert n > 0 and np.all(m[n:] == -1)
        m = m[:n]
        pos = [_check_group_geometry(model, g, c, oc) if mode == "sticky" else _group_rows(model, g, c) for g, oc in enumerate(own_c)]
        want = np.full(n, -100, np.int64)
        for g, oc in enumerate(own_c):
            om = oc.rigid_contact_match_index.cpu().numpy()[: len(pos[g])].astype(np.int64)
            if prev_pos is not None:
                om = np.where(om >= 0, prev_pos[g][np.maximum(om, 0)] if len(prev_pos[g]) else om, om)
            want[pos[g]] = om
        assert np.array_equal(m, want), frame
        matched += int((m >= 0).sum())
        world = _world(model, _host(c, "shape0")[:n], _host(c, "shape1")[:n])
        if report:
            nn = int(c.rigid_contact_new_count.cpu().numpy()[0])
            assert np.array_equal(c.rigid_contact_new_indices.cpu().numpy()[:nn], np.flatnonzero(m < 0))
            nb = int(c.rigid_contact_broken_count.cpu().numpy()[0])
            broken = c.rigid_contact_broken_indices.cpu().numpy()[:nb]
            if prev is None:
                assert np.all(m == -1) and nb == 0
            else:
                pn, pworld = prev
                assert np.all(m < pn) and len(np.unique(m[m >= 0])) == (m >= 0).sum()
                alive = np.ones(pn, bool) if frame != 2 else ~np.isin(pworld, reset_worlds)
                assert np.array_equal(broken, np.setdiff1d(np.flatnonzero(alive), m[m >= 0]))
        if frame == 2:
            assert np.all(m[np.isin(world, reset_worlds)] == -1)
        prev, prev_pos = (n, world), pos
        solver.step(st[0], st[1], None, c, 1.0 / 240.0)
        st[0], st[1] = st[1], st[0]
    assert matched > 0


def test_matching_latest_with_report_against_the_groups():
    check_matching_against_the_groups("latest")


def test_matching_sticky_against_the_groups():
    check_matching_against_the_groups("sticky")


def test_contact_force_rows_follow_the_global_order():
    """Contacts.force[i] of a grouped deterministic Contacts is the force of global contact i: the default pipeline's forces under
    the stable key sort of its rows."""
    import torch

    import newton_amd as nt

    frames = 20 if _emulated() else 150

    def run(deterministic):
        model, kw = _model("mixed")
        model.request_contact_attributes("force")
        pipe = nt.CollisionPipeline(model, deterministic=deterministic, **kw)
        contacts = pipe.contacts()
        solver = nt.solvers.SolverXPBD(model, iterations=2)
        s0, s1 = model.state(), model.state()
        for _ in range(frames):
            s0.clear_forces()
            pipe.collide(s0, contacts)
            solver.step(s0, s1, None, contacts, 1e-3)
            s0, s1 = s1, s0
        solver.update_contacts(contacts)
        torch.cuda.synchronize()
        n = _count(contacts)
        f = contacts.force.cpu().numpy()
        assert f.shape[0] >= n and np.all(f[n:] == 0.0)
        return (_host(contacts, "shape0")[:n], _host(contacts, "shape1")[:n], _host(contacts, "point0")[:n], f[:n])

    a0, a1, ap, af = run(False)
    d0, d1, dp, df = run(True)
    assert len(a0) == len(d0) > 0 and np.abs(af).max() > 0.0
    order = np.lexsort((np.arange(len(a0)), a1, a0))  # stable sort of the raw rows by key == the deterministic order
    assert not np.array_equal(order, np.arange(len(a0)))
    assert np.array_equal(a0[order], d0) and np.array_equal(a1[order], d1) and np.array_equal(ap[order], dp)
    assert np.array_equal(_bits(af[order]), _bits(df))


def test_two_collides_on_one_state_are_bit_identical():
    import torch

    import newton_amd as nt

    model, kw = _model("mixed")
    pipe = nt.CollisionPipeline(model, contact_matching="latest", contact_report=True, **kw)
    c, s = pipe.contacts(), model.state()
    out = []
    for _ in range(2):
        pipe.collide(s, c)
        torch.cuda.synchronize()
        out.append({f: _bits(_host(c, f)).copy() for f in FIELDS + ("count",)})
        out[-1]["order"] = c.export_order().cpu().numpy()
    assert out[0]["count"][0] > 0
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), k
    n = int(out[1]["count"][0])
    assert np.array_equal(c.rigid_contact_match_index.cpu().numpy()[:n], np.arange(n))  # (the same contacts again: each matches itself)


def test_grouped_collide_with_matching_does_not_synchronise():
    """collide() with matching + report under torch.cuda.set_sync_debug_mode("error"): nothing synchronises."""
    _needs_device()
    import torch

    import newton_amd as nt

    model, kw = _model("mesh")
    pipe = nt.CollisionPipeline(model, contact_matching="latest", contact_report=True, **kw)
    c, s = pipe.contacts(), model.state()
    pipe.collide(s, c)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        pipe.collide(s, c)
        pipe.collide(s, c)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert _count(c) > 0


@pytest.mark.parametrize("concurrent", [False, True])
def test_grouped_matching_frame_replays_bit_identically(concurrent):
    """clear_forces / collide (matching + report) / SolverXPBD.step per substep, eagerly and as one replayed hipGraph (torch
    backend), with the groups' launches serial or on sibling streams: states, views, match indices, new / broken lists agree."""
    _needs_device()
    import torch

    import newton_amd as nt

    dt, substeps, frames = 1.0 / 240.0, 2, 4
    out = {}
    for run in ("eager", "graph"):
        model, kw = _model("mixed")
        model.world_groups.concurrent = concurrent
        pipe = nt.CollisionPipeline(model, contact_matching="latest", contact_report=True, **kw)
        solver = nt.solvers.SolverXPBD(model, iterations=2)
        st, ctrl, contacts = [model.state(), model.state()], model.control(), pipe.contacts()

        def simulate():
            for _ in range(substeps):
                st[0].clear_forces()
                pipe.collide(st[0], contacts)
                solver.step(st[0], st[1], ctrl, contacts, dt)
                st[0], st[1] = st[1], st[0]

        if run == "eager":
            for _ in range(frames + 1):
                simulate()
        else:
            g = nt.graph.capture(simulate, warmup=1, contacts=contacts)  # (the warm-up frame is the eager run's first)
            for _ in range(frames):
                g.launch()
        torch.cuda.synchronize()
        n = _count(contacts)
        r = {"body_q": st[0].body_q.cpu().numpy().copy(), "body_qd": st[0].body_qd.cpu().numpy().copy(), "n": n,
             "match": contacts.rigid_contact_match_index.cpu().numpy().copy()}
        for f in FIELDS:
            r[f] = _bits(_host(contacts, f)).copy()
        nn, nb = int(contacts.rigid_contact_new_count.cpu().numpy()[0]), int(contacts.rigid_contact_broken_count.cpu().numpy()[0])
        r["new"] = contacts.rigid_contact_new_indices.cpu().numpy()[:nn].copy()
        r["broken"] = contacts.rigid_contact_broken_indices.cpu().numpy()[:nb].copy()
        out[run] = r
    e, g = out["eager"], out["graph"]
    assert e["n"] > 0 and (e["match"][: e["n"]] >= 0).any()
    for k in e:
        assert np.array_equal(np.asarray(e[k]), np.asarray(g[k])), k
