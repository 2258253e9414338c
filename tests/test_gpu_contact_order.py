"""The key-ordered contact export and the matching report on the device (include/newton_hip_contacts.h): CollisionPipeline(
deterministic=True) gives the default pipeline's raw export under a stable sort on (shape0 << 32 | shape1), bit for bit, and a frame
whose collide() matches contacts records into one hipGraph (both capture backends) and replays bit-identically to the eager frames."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

pytestmark = pytest.mark.gpu

FIELDS = ("shape0", "shape1", "point0", "point1", "offset0", "offset1", "normal", "margin0", "margin1")


def _emulated():
    import torch

    return getattr(torch.cuda, "_newton_emulated", False)


def _needs_device():
    import torch

    if not torch.cuda.is_available() or _emulated():
        pytest.skip("hipGraph capture needs the device (not emulated)")


def _scene(name, small=False):
    """-> (model, CollisionPipeline kwargs, per_contact_shape_properties)"""
    import newton_amd as nt
    import scenes

    if name == "quadruped":
        E = 4 if small else 16
        model = scenes.quadruped_scene(E, seed=3, device="cuda:0")
        model.joint_q.reshape(E, -1)[:, 2] -= 0.26  # (onto the ground, as smoke() does)
        model.body_q, model.body_qd = nt.articulation.eval_fk_numpy(model, model.joint_q, model.joint_qd)
        return model, {}, False
    if name == "box_stack":
        return scenes.box_stack_scene(2 if small else 6, n_boxes=4, seed=2, jitter=4e-3, device="cuda:0"), {}, False
    if name == "mixed":
        return scenes.mixed_primitive_scene(2 if small else 5, device="cuda:0"), {}, False
    if name == "sdf":
        from sdf_pipeline_checker import sdf_scene

        return sdf_scene(2 if small else 4, 5 if small else 6, device="cuda:0", walls=True, seed=9), {"broad_phase": "sap"}, False
    if name == "hydro":
        from test_gpu_sdf_pipeline import hydro_scene

        return (hydro_scene(2 if small else 3, device="cuda:0"),
                {"broad_phase": "sap", "sdf_hydroelastic_config": nt.geometry.HydroelasticSDF.Config()}, True)
    if name == "terrain":
        return scenes.terrain_scene(2 if small else 4, n_shapes=4 if small else 8, device="cuda:0", cells=16 if small else 64), {}, False
    raise KeyError(name)


def _host(c, name):
    v = getattr(c, "rigid_contact_" + name)
    return None if v is None else v.cpu().numpy()


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def check_sorted_against_raw(name, small=False):
    """Both pipelines on the same state: the deterministic views == the default pipeline's raw export under a numpy stable argsort
    of shape0 << 32 | shape1 -- every field, the count, the fill beyond the count, export_order()."""
    import torch

    import newton_amd as nt

    model, kw, props = _scene(name, small)
    raw_pipe, det_pipe = nt.CollisionPipeline(model, **kw), nt.CollisionPipeline(model, deterministic=True, **kw)
    s = model.state()
    raw, det = raw_pipe.contacts(per_contact_shape_properties=props), det_pipe.contacts(per_contact_shape_properties=props)
    for _ in range(2):  # (the second frame rewrites the persistent buffers: no stale entry may survive)
        raw_pipe.collide(s, raw)
        det_pipe.collide(s, det)
        torch.cuda.synchronize()
        n = int(_host(raw, "count")[0])
        assert n > 0 and int(_host(det, "count")[0]) == n
        key = _host(raw, "shape0")[:n].astype(np.int64) * (1 << 32) + _host(raw, "shape1")[:n]
        order = np.argsort(key, kind="stable")
        names = FIELDS + (("stiffness", "damping", "friction") if props else ())
        for f in names:
            a, b = _bits(_host(raw, f)), _bits(_host(det, f))
            assert a.shape == b.shape, f
            assert np.array_equal(a[:n][order], b[:n]), (name, f)
            assert np.array_equal(b[n:], np.full_like(b[n:], -1 if f in ("shape0", "shape1") else 0)), (name, f)
        eo = det.export_order()
        assert (eo is None and n <= 1) or np.array_equal(eo.cpu().numpy(), order)
        assert int(det.order_unmatched_rows.cpu().numpy()[0]) == 0
        if det._flat is not None:
            assert np.array_equal(det._flat_live.cpu().numpy(), raw._flat_live.cpu().numpy()) and det._flat_n0 == raw._flat_n0
    return n, int((order != np.arange(n)).sum())


@pytest.mark.parametrize("name", ["quadruped", "box_stack", "mixed", "sdf", "hydro", "terrain"])
def test_sorted_export_is_a_stable_sort_of_the_raw_export(name):
    n, moved = check_sorted_against_raw(name, small=_emulated())
    # (the ground / terrain contacts of the quadrupeds and primitives come out in key order already)
    assert n > 1 and (moved > 0 or name in ("quadruped", "terrain"))


def test_sorted_export_of_an_empty_frame():
    """No contact anywhere: count 0, every entry filled, also after a frame that had contacts."""
    import torch

    import newton_amd as nt

    model, kw, _ = _scene("box_stack", small=True)
    pipe = nt.CollisionPipeline(model, deterministic=True)
    c = pipe.contacts()
    s = model.state()
    pipe.collide(s, c)
    assert int(_host(c, "count")[0]) > 0
    far = model.state()
    q = far.body_q.clone()
    q[:, 2] += 100.0 + 10.0 * torch.arange(q.shape[0], dtype=q.dtype, device=q.device)  # (apart, and off the ground)
    far.body_q = q
    pipe.collide(far, c)
    torch.cuda.synchronize()
    assert int(_host(c, "count")[0]) == 0
    assert np.all(_host(c, "shape0") == -1) and np.all(_host(c, "normal") == 0.0) and c.export_order() is None


def _frame_record(pipe, contacts, st, report):
    n = int(_host(contacts, "count")[0])
    r = {"body_q": st[0].body_q.cpu().numpy().copy(), "body_qd": st[0].body_qd.cpu().numpy().copy(), "n": n,
         "match": contacts.rigid_contact_match_index.cpu().numpy().copy()}
    for f in FIELDS:
        r[f] = _bits(_host(contacts, f)).copy()
    if report:
        nn, nb = int(contacts.rigid_contact_new_count.cpu().numpy()[0]), int(contacts.rigid_contact_broken_count.cpu().numpy()[0])
        r["new"] = contacts.rigid_contact_new_indices.cpu().numpy()[:nn].copy()
        r["broken"] = contacts.rigid_contact_broken_indices.cpu().numpy()[:nb].copy()
    return r


@pytest.mark.parametrize("backend", ["torch", "abi"])
@pytest.mark.parametrize("mode", ["latest", "sticky"])
@pytest.mark.parametrize("scene", ["box_stack", "sdf"])
def test_matching_frame_replays_bit_identically(scene, mode, backend):
    """clear_forces / collide (matching, + report for "latest") / SolverXPBD.step per substep, eagerly and as one replayed hipGraph:
    states, flat views, match indices and the new / broken lists agree bit for bit."""
    _needs_device()
    import torch

    import newton_amd as nt

    model, kw, _ = _scene(scene)
    report = mode == "latest"
    dt, substeps, frames = 1.0 / 240.0, 2, 4
    out = {}
    for run in ("eager", "graph"):
        thr = {"contact_matching_pos_threshold": 0.004, "contact_matching_normal_dot_threshold": 0.9} if scene == "sdf" else {}
        pipe = nt.CollisionPipeline(model, contact_matching=mode, contact_report=report, **kw, **thr)
        solver = nt.solvers.SolverXPBD(model, iterations=2)
        st, ctrl, contacts = [model.state(), model.state()], model.control(), pipe.contacts()

        def simulate():
            for _ in range(substeps):
                st[0].clear_forces()
                pipe.collide(st[0], contacts)
                solver.step(st[0], st[1], ctrl, contacts, dt)
                st[0], st[1] = st[1], st[0]

        if run == "eager":
            for _ in range(frames):
                simulate()
        elif backend == "torch":
            g = nt.graph.capture(simulate, warmup=0, contacts=contacts)
            for _ in range(frames):
                g.launch()
        else:
            g = nt.graph.capture(simulate, warmup=1, backend="abi", contacts=contacts)
            for _ in range(frames - 1):
                g.launch()
        torch.cuda.synchronize()
        out[run] = _frame_record(pipe, contacts, st, report)
    e, g = out["eager"], out["graph"]
    assert e["n"] > 0 and e["n"] == g["n"]
    assert (e["match"][: e["n"]] >= 0).any() or scene == "sdf"  # (the stack's frames do match contacts)
    for k in e:
        assert np.array_equal(np.asarray(e[k]), np.asarray(g[k])), k


def test_collide_with_matching_does_not_synchronise():
    """collide() with contact matching + report under torch.cuda.set_sync_debug_mode("error"): nothing synchronises."""
    _needs_device()
    import torch

    import newton_amd as nt

    model, kw, _ = _scene("sdf")
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
    assert int(c.rigid_contact_count.cpu().numpy()[0]) > 0


def check_report_with_world_reset(small=False):
    """rigid_contact_match_index / new / broken through frames and a reset_contact_matching(world_mask), against the definitions:
    new = ascending positions with match < 0; broken = previous positions of worlds not reset that no contact matched."""
    import torch

    import newton_amd as nt

    model, kw, _ = _scene("sdf", small)
    E = model.env.env_count
    pipe = nt.CollisionPipeline(model, contact_matching="latest", contact_report=True, **kw)
    c, solver = pipe.contacts(), nt.solvers.SolverXPBD(model, iterations=2)
    st = [model.state(), model.state()]
    sw = np.asarray(model.shape_world)
    prev = None
    for frame in range(4):
        st[0].clear_forces()
        if frame == 2:
            mask = np.zeros(E, bool)
            mask[E - 1] = True
            pipe.reset_contact_matching(mask)
        pipe.collide(st[0], c)
        torch.cuda.synchronize()
        n = int(_host(c, "count")[0])
        m = c.rigid_contact_match_index.cpu().numpy()
        assert np.all(m[n:] == -1)
        m = m[:n]
        world = np.maximum(sw[_host(c, "shape0")[:n]], sw[_host(c, "shape1")[:n]])
        nn = int(c.rigid_contact_new_count.cpu().numpy()[0])
        assert np.array_equal(c.rigid_contact_new_indices.cpu().numpy()[:nn], np.flatnonzero(m < 0))
        nb = int(c.rigid_contact_broken_count.cpu().numpy()[0])
        broken = c.rigid_contact_broken_indices.cpu().numpy()[:nb]
        if prev is None:
            assert np.all(m == -1) and nb == 0
        else:
            pn, pworld = prev
            assert np.all(m < pn) and len(np.unique(m[m >= 0])) == (m >= 0).sum()
            alive = np.ones(pn, bool) if frame != 2 else pworld != E - 1
            assert np.array_equal(broken, np.setdiff1d(np.flatnonzero(alive), m[m >= 0]))
            if frame == 2:
                assert np.all(m[world == E - 1] == -1) and np.any(m[world != E - 1] >= 0)
        prev = (n, world)
        solver.step(st[0], st[1], None, c, 1.0 / 240.0)
        st[0], st[1] = st[1], st[0]


def test_report_with_a_world_reset():
    check_report_with_world_reset(small=_emulated())
