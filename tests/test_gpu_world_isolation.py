"""World isolation and reset after divergence on the device (the cases and the comparison are
tests/world_isolation_cases.py, the emulated twin with the non-finite aggressors is tests/test_world_isolation_emu.py).

Every case runs one scene twice through one entry point -- run A undisturbed, run B with fast / far / deep / out-of-limits / re-parametrised
AGGRESSOR worlds -- and requires everything run B wrote for the other worlds (state, per-world contact count, the world's own rows of every
flat contact array, contact forces, match ordinals, sensor and kinematics rows) to carry run A's bits.  No tolerance, no excluded world.
Each case asserts that it is not vacuous: run A is finite, every victim holds a live contact where the scene has contacts, "deep" and "far"
change the aggressors' contact total, the aggressors' state comes out different, "params" flips the model to the per-environment tile.

Every aggressor input is finite: nothing here is chosen to make a kernel spin or fault (the NaN / Inf / zero-quaternion worlds run on
the emulator only).  37 worlds: a ragged last workgroup at 4, 8, 16 and 32 worlds per workgroup."""
import numpy as np
import pytest

import world_isolation_cases as wi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = wi.WORLDS
GENERIC = wi.GENERIC
DT = {"xpbd": 1e-3, "semi_implicit": 1e-4, "featherstone": 5e-4}


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


_MODELS = {}


def _model(name, n, report=False):
    """The scene on the device, built once and never modified (report: with contacts.force and body_parent_f requested)."""
    key = (name, n, report)
    if key not in _MODELS:
        model = wi.scene(name, n, device=DEV)
        if report:
            model.request_contact_attributes("force")
            model.request_state_attributes("body_parent_f")
        _MODELS[key] = model
    return _MODELS[key]


def _state(model, start):
    s = model.state()
    for k in wi.STATE_FIELDS:
        setattr(s, k, start[k])
    return s


def _control(model, start):
    c = model.control()
    for k in wi.CONTROL_FIELDS:
        setattr(c, k, start[k])
    return c


def _solver(nt, model, which, kw):
    cls = {"xpbd": nt.solvers.SolverXPBD, "semi_implicit": nt.solvers.SolverSemiImplicit, "featherstone": nt.solvers.SolverFeatherstone}
    if which == "xpbd":
        kw = dict({"iterations": 2}, **kw)
    return cls[which](model, **kw)


def _snap_state(model, s, parent_f=False):
    E = model.env.env_count
    snap = {k: wi.by_world(_np(getattr(s, k)), E) for k in wi.STATE_FIELDS}
    if parent_f:
        snap["body_parent_f"] = wi.by_world(_np(s.body_parent_f), E)
    return snap


def _snap_contacts(model, ct, force=False):
    flat = {k: _np(getattr(ct, "rigid_contact_" + k)) for k in ("count",) + wi.FLAT}
    snap, rows = wi.contact_rows(model, flat, {"force": _np(ct.force)} if force else None)
    snap["contact_count"] = _np(ct.rigid_contact_count_per_env).copy()
    assert [len(r) for r in rows] == list(snap["contact_count"]), "the flat rows of a world are not as many as its count"
    return snap, rows, int(flat["count"][0])


def _collide_run(model, start, frames=1, **pipe_kw):
    """CollisionPipeline.collide alone; with matching, a second frame on poses moved by 0.2 mm (inside the matcher's 0.5 mm), whose match
    indices are compared as ordinals among the world's own rows of the first frame."""
    import newton_amd as nt

    pipe = nt.CollisionPipeline(model, **pipe_kw)
    ct, s = pipe.contacts(), _state(model, start)
    pipe.collide(s, ct)
    snap, rows, n = _snap_contacts(model, ct)
    for _ in range(frames - 1):
        moved = start["body_q"].copy()
        moved[:, 2] += np.float32(2e-4)
        s.body_q = moved
        pipe.collide(s, ct)
        first, (snap, rows_now, n_now) = snap, _snap_contacts(model, ct)
        snap["match"] = wi.match_ordinals(_np(ct.rigid_contact_match_index), rows_now, rows, n)
        snap.update({"first_" + k: v for k, v in first.items()})
    return snap


def _solver_run(model, start, which, mode, substeps, solver_kw=None, cfg=None, report=False):
    """`substeps` of one solver from `start`: mode "step" is the loop clear_forces; collide; step; swap launch by launch, "rollout" the
    fused launch.  -> the final state, the Contacts of the last collide (and the reported forces / joint wrenches)."""
    import newton_amd as nt

    solver, pipe = _solver(nt, model, which, solver_kw or {}), nt.CollisionPipeline(model)
    s0, s1, ctrl, ct = _state(model, start), _state(model, start), _control(model, start), pipe.contacts()
    dt = DT[which]
    with wi.xpbd_cfg(cfg):
        if mode == "rollout":
            s0 = solver.rollout(s0, s1, ctrl, ct, dt, substeps)
        else:
            for _ in range(substeps):
                s0.clear_forces()
                pipe.collide(s0, ct)
                solver.step(s0, s1, ctrl, ct, dt)
                s0, s1 = s1, s0
            if report:
                solver.update_contacts(ct)
    snap = _snap_state(model, s0, parent_f=report)
    if report:  # SensorContact on the step's impulses: the four lower legs against the ground, and their totals
        from newton_amd import sensors

        t = model.env
        legs = [b for b in range(t.nb) if model.body_label[b].endswith("_SHANK")]
        sensor = sensors.SensorContact(model, sensing_bodies=legs, counterpart_shapes=[t.ns])
        sensor.net_force.fill_(7.0)
        sensor.eval(ct)
        snap["sensor_contact"] = wi.by_world(_np(sensor.net_force), t.env_count)
        assert len(legs) == 4 and not np.any(snap["sensor_contact"] == 7.0)
    if model.env.np > 0:
        snap.update(_snap_contacts(model, ct, force=report)[0])
    return snap


def _check(name, n, run, what, contacts=True, params=True, combos=wi.combos, report=False, differ=wi.STATE_FIELDS):
    """Run A once, run B for every (kind, mask) of the scene and for the parameter edit under every mask.  differ: the snapshot entries of
    which one has to come out different in the aggressor worlds."""
    model = _model(name, n, report)
    contacts = contacts and model.env.np > 0
    A = run(model, wi.start_arrays(model))
    written = [k for k in differ if k in A]  # (collide alone writes no state)
    for k in written:
        assert np.isfinite(A[k]).all(), f"{what}: the undisturbed run is not finite in {k}"
    if contacts:
        wi.assert_victims_in_contact(A, np.zeros(n, bool), what)  # (every world is a victim under one mask or another)
    start_contacts = _collide_run(model, wi.start_arrays(model)) if contacts else None
    kinds = wi.kinds_for(model, contacts)
    assert "fast" in kinds and (not contacts or {"far", "deep"} <= set(kinds))
    for kind, mname, aggr in combos(n, kinds + (("pressed",) if name in wi.PRESSED and contacts else ())):
        tag = f"{what} [{kind}, {mname}]"
        B = run(model, wi.start_arrays(model, kind, aggr, wi.depth(name, kind)))
        wi.assert_isolated(A, B, aggr, tag, differ=written or None)
        if contacts and kind in ("far", "deep", "pressed"):  # (the live-contact lists the run starts from)
            wi.assert_contact_totals_differ(start_contacts, _collide_run(model, wi.start_arrays(model, kind, aggr, wi.depth(name, kind))), aggr, tag)
    if params:
        edited = wi.scene(name, n, device=DEV)
        if report:
            edited.request_contact_attributes("force")
            edited.request_state_attributes("body_parent_f")
        pristine = wi.pristine_params(edited)
        assert model.device_model().desc.params_uniform == 1
        for mname, aggr in wi.masks(n).items():
            wi.edit_params(edited, aggr, pristine)
            assert edited.device_model().desc.params_uniform == 0
            B = run(edited, wi.start_arrays(edited))
            wi.assert_isolated(A, B, aggr, f"{what} [params, {mname}]", differ=written)
    return A


# -- 1. CollisionPipeline.collide alone ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipe_kw", [dict(broad_phase="explicit"), dict(broad_phase="nxn"), dict(broad_phase="sap"), dict(deterministic=True),
                                     dict(contact_matching="latest"), dict(contact_matching="sticky")],
                         ids=["explicit", "nxn", "sap", "deterministic", "latest", "sticky"])
def test_collide_alone(pipe_kw):
    frames = 2 if "contact_matching" in pipe_kw else 1
    # (collide reads poses only: nothing it writes tells a fast world from a slow one, so the kinds are the two that move bodies)
    A = _check("mixed", N, lambda m, st: _collide_run(m, st, frames, **pipe_kw), f"collide {pipe_kw}", params=False,
               combos=lambda n, kinds: wi.combos(n, ("far", "deep", "pressed")))
    if frames == 2:  # (not vacuous: the second frame's contacts found their first-frame rows, in every world)
        assert all(np.any(m >= 0) for m in A["match"]), "worlds without a single matched contact"


# -- 2. SolverXPBD.step with contacts.force and body_parent_f --------------------------------------------------------------------------
def test_xpbd_step_with_reports():
    # (the robots lowered by 0.30: every world's feet are in the ground at the start, and the one step's impulses are what is reported --
    # two steps later most robots are in the air again and report zeros)
    A = _check("quadruped_low", N, lambda m, st: _solver_run(m, st, "xpbd", "step", 1, report=True), "xpbd step + reports", report=True)
    # not vacuous: every world reports a contact force, a joint wrench and a net force on a lower leg
    assert all(np.any(f != 0.0) for f in A["contact_force"]) and np.all(np.any(A["body_parent_f"] != 0.0, axis=1))
    assert np.all(np.any(A["sensor_contact"] != 0.0, axis=1)), "worlds whose contact sensor reads zero"


# -- 3. SolverXPBD.rollout -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["default", "generic", "epb4", "restitution", "convex", "box_stack", "mixed", "hull_bin"])
def test_xpbd_rollout(case):
    name, n, substeps, kw, cfg, combos, params = "quadruped", N, 6, {}, None, wi.combos, True
    if case == "generic":  # (the forced instance is the uniform-parameter one: no per-world parameter edit under it)
        cfg, params = GENERIC, False
    elif case == "epb4":
        kw = dict(envs_per_block=4)
    elif case == "restitution":
        kw = dict(enable_restitution=True)
    elif case == "convex":
        name, n, combos = "quadruped_convex", 9, wi.rotated
    elif case == "box_stack":
        name, n = "box_stack", 11
    elif case == "mixed":
        name, n = "mixed", 10
    elif case == "hull_bin":  # (the per-contact records in HBM)
        name, n, substeps, combos = "hull_bin", 3, 2, wi.rotated
        assert _model(name, n).device_model().desc.contact_scratch_in_hbm == 1
    if case in ("default", "generic"):
        import ctypes as C

        import newton_amd as nt

        model = _model(name, n)
        dm, out, p = model.device_model(), (C.c_int32 * 5)(), nt.solvers.SolverXPBD(model, iterations=2)._params()
        with wi.xpbd_cfg(cfg):
            assert dm.lib.nt_xpbd_rollout_shape(C.byref(dm.desc), C.byref(p), None, out) == 0
        assert (out[4] != 0) == (case == "default"), list(out)  # the default dispatch takes the specialised instance
    _check(name, n, lambda m, st: _solver_run(m, st, "xpbd", "rollout", substeps, kw, cfg), f"xpbd rollout {case}", combos=combos, params=params)


# -- 4. SolverSemiImplicit ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["step", "rollout"])
@pytest.mark.parametrize("name", ["quadruped", "joint_zoo", "d6_angular"])
def test_semi_implicit(name, mode):
    _check(name, N, lambda m, st: _solver_run(m, st, "semi_implicit", mode, 3 if mode == "step" else 6), f"semi-implicit {mode} {name}")


# -- 5. SolverFeatherstone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["step", "rollout"])
@pytest.mark.parametrize("epb", [0, 4])  # (16 quadrupeds do not fit one workgroup of this solver: NT_ERR_UNSUPPORTED; 16 is below)
@pytest.mark.parametrize("mass_matrix", ["tree", "dense"])
def test_featherstone_quadruped(mass_matrix, epb, mode):
    kw = dict(mass_matrix=mass_matrix, envs_per_block=epb)
    _check("quadruped", N, lambda m, st: _solver_run(m, st, "featherstone", mode, 3 if mode == "step" else 6, kw),
           f"featherstone {mode} {mass_matrix} epb {epb}", combos=wi.combos if (epb == 0 and mass_matrix == "tree") else wi.rotated)


@pytest.mark.parametrize("mode", ["step", "rollout"])
@pytest.mark.parametrize("name,kw", [("multi_art", dict(update_mass_matrix_interval=2)), ("free_child", {}),
                                     ("free_child", dict(envs_per_block=16))], ids=["multi_art_interval2", "free_child", "free_child_epb16"])
def test_featherstone_scenes(name, kw, mode):
    """multi_art with update_mass_matrix_interval = 2: the cached factor's rows are per world; 5 substeps reuse it twice.  free_child at 16
    worlds per workgroup: two full tiles and a ragged one of 5."""
    _check(name, N, lambda m, st: _solver_run(m, st, "featherstone", mode, 5, kw), f"featherstone {mode} {name}", contacts=False)


# -- 6. kinematics and dynamics entry points ---------------------------------------------------------------------------------------------
POISON = -7.25e3


def _kinematics_run(model, start):
    """eval_fk, eval_ik, eval_jacobian, eval_mass_matrix and eval_inverse_dynamics (with and without joint_qdd) into caller tensors
    pre-filled with a poison value; one articulation per world in both scenes, so every output splits by world."""
    import torch

    import newton_amd as nt

    E = model.env.env_count
    L_, D, A = model.max_joints_per_articulation, model.max_dofs_per_articulation, model.articulation_count
    assert A == E
    mk = lambda *shape: torch.full(shape, POISON, dtype=torch.float32, device=DEV)  # noqa: E731
    s = _state(model, start)
    nt.eval_fk(model, start["joint_q"], start["joint_qd"], s)
    snap = {"fk_body_q": _np(s.body_q), "fk_body_qd": _np(s.body_qd)}
    jq, jqd = mk(model.joint_coord_count), mk(model.joint_dof_count)
    nt.eval_ik(model, s, jq, jqd)
    J, H, S, I = mk(A, 6 * L_, D), mk(A, D, D), mk(model.joint_dof_count, 6), mk(model.body_count, 6, 6)  # noqa: E741
    assert nt.eval_jacobian(model, s, J, S) is J and nt.eval_mass_matrix(model, s, H, body_I_s=I) is H
    qdd = torch.from_numpy(np.random.default_rng(3).normal(0.0, 2.0, size=(A, D)).astype(np.float32)).to(DEV)
    bias, tau = mk(A, D), mk(A, D)
    nt.eval_inverse_dynamics(model, s, None, bias)
    nt.eval_inverse_dynamics(model, s, qdd, tau)
    snap.update(ik_joint_q=_np(jq), ik_joint_qd=_np(jqd), J=_np(J), H=_np(H), S=_np(S), I=_np(I), bias=_np(bias), tau=_np(tau))
    for k, v in snap.items():
        assert not np.any(v == POISON), f"{k}: the poison is still there"
    return {k: wi.by_world(v, E) for k, v in snap.items()}


@pytest.mark.parametrize("name", ["joint_zoo", "quadruped"])
def test_kinematics_entry_points(name):
    _check(name, N, _kinematics_run, f"kinematics {name}", contacts=False, differ=("fk_body_q", "fk_body_qd", "H", "tau"))


# -- 7. ik.IKSolver.step -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["quadruped", "joint_zoo_free_root"])
def test_ik_solver_step(name):
    """Ten Levenberg-Marquardt iterations in one launch; the aggressor worlds' position targets are 1e3 m away (unreachable: their damping
    climbs while the victims converge).  The solution, the cost and the damping of every victim carry the bits of the undisturbed solve."""
    import torch

    from ik_cases import ik_case, make_objectives, objective_specs
    from newton_amd import ik

    model, _, targets, start = ik_case(name, N, 5, device=DEV)
    q_in = torch.from_numpy(start.astype(np.float32)).to(DEV)

    def solve(tg):
        solver = ik.IKSolver(model, make_objectives(name, model, tg))
        out = torch.full_like(q_in, 7.0)
        solver.step(q_in, out, iterations=0)
        cost_in = _np(solver.costs).copy()
        solver.reset()
        solver.step(q_in, out, iterations=10)
        return {"joint_q": wi.by_world(_np(out), N), "cost": wi.by_world(_np(solver.costs), N), "lambda": wi.by_world(_np(solver.lambdas), N)}, cost_in

    A, cost_in = solve(targets)
    assert np.isfinite(A["joint_q"]).all() and np.all(A["cost"][:, 0] < cost_in), "the undisturbed solve did not move"
    for mname, aggr in wi.masks(N).items():
        tg = [None if t is None else np.array(t, copy=True) for t in targets]
        for (kind, _link), t in zip(objective_specs(name, model), tg):
            if kind == "position":
                t[aggr] += np.float32(1.0e3)
        B, _ = solve(tg)
        wi.assert_isolated(A, B, aggr, f"ik {name} [{mname}]", differ=("joint_q", "cost"))


# -- 8. sensors ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [3, 70])
def test_frame_sensors(rows):
    """nt_frame_sensor, the one launch behind SensorFrameTransform and SensorIMU, on the shared case of tests/frame_sensor_cases.py (four
    free bodies per world, a gravity per world): the aggressor worlds 1e4 m away, spinning at 1e3 rad/s, 300 m/s faster than a step ago."""
    import torch

    import frame_sensor_cases as fc

    def run(case):
        model = fc.sensor_model(case.E, device=DEV, varied_gravity=True)
        dm, s, sp = model.device_model(), model.state(), model.state()
        s.body_q, s.body_qd = case.body_q, case.body_qd
        sp.body_q, sp.body_qd = case.body_q, case.body_qd_prev
        call = fc.Call(case, upload=lambda a: torch.from_numpy(a).to(DEV), ptr=lambda x: x.data_ptr())
        assert call.run(dm.lib, dm.desc, s._desc(), sp._desc(), stream=dm.stream()) == 0
        torch.cuda.synchronize()
        return {k: wi.by_world(_np(v), case.E) for k, v in call.out.items()}

    A = run(fc.case(N, rows))
    assert set(A) == set(fc.OUTPUTS) and all(np.isfinite(v).all() and not np.any(v == fc.POISON) for v in A.values())
    for mname, aggr in wi.masks(N).items():
        case = fc.Case(N, rows)
        sel = aggr.repeat(case.nb)
        case.body_q[sel, :3] += np.float32(1.0e4)
        case.body_qd[sel] += np.array([300.0, -200.0, 100.0, 1.0e3, -1.0e3, 1.0e3], np.float32)
        wi.assert_isolated(A, run(case), aggr, f"frame sensors {rows} rows [{mname}]", differ=("transform", "velocity", "accel"))


@pytest.mark.parametrize("name", ["primitives"])
def test_sensor_raycast(name):
    """SensorRaycast on the primitive scene of tests/raycast_cases.py (37 worlds, 70 rays, some attached to bodies): the aggressor worlds'
    bodies 1e4 m away (every ray of theirs misses or meets the ground) or moved by a body width (other hits, other candidate lists)."""
    import torch

    import raycast_cases as rc
    from newton_amd import sensors

    make, rays, kw = rc.CASES[name]
    model = make(device=DEV)
    E = model.env.env_count
    o, d, body = rays()

    def cast(body_q):
        state = model.state()
        state.body_q = body_q
        s = sensors.SensorRaycast(model, o, d, ray_body=body, max_distance=rc.MAX_DISTANCE, **kw)
        s.distance.fill_(7.0), s.normal.fill_(7.0), s.shape.fill_(-7)
        s.eval(state)
        torch.cuda.synchronize()
        snap = {"distance": wi.by_world(_np(s.distance), E), "normal": wi.by_world(_np(s.normal), E), "shape": wi.by_world(_np(s.shape), E)}
        assert not np.any(snap["distance"] == 7.0) and not np.any(snap["shape"] == -7)
        return snap

    base = np.array(model.body_q, np.float32, copy=True)
    A = cast(base)
    assert np.all((A["shape"] >= 0).sum(axis=1) >= 10), "worlds whose rays hit next to nothing"
    for move in (np.array([1.0e4, -1.0e4, 1.0e4], np.float32), np.array([0.15, -0.1, 0.2], np.float32)):
        for mname, aggr in wi.masks(E).items():
            bq = base.copy()
            bq[aggr.repeat(model.env.nb), :3] += move
            wi.assert_isolated(A, cast(bq), aggr, f"raycast {name} {move} [{mname}]", differ=("distance", "shape"))


def test_frame_sensor_classes():
    """SensorFrameTransform (every frame in the world-fixed frame 3) and SensorIMU (velocity and projected gravity on) through their own
    eval path, on the frame table and states of the same shared case."""
    import frame_sensor_cases as fc
    from newton_amd import sensors

    model = fc.sensor_model(N, device=DEV, varied_gravity=True)

    def run(case):
        s, sp = model.state(), model.state()
        s.body_q, s.body_qd = case.body_q, case.body_qd
        sp.body_q, sp.body_qd = case.body_q, case.body_qd_prev
        frames = list(zip(case.frame_body, case.frame_xform))
        ft, imu = sensors.SensorFrameTransform(model, frames, reference_frames=[frames[3]]), sensors.SensorIMU(model, frames, True, True)
        for out in (ft.transforms, imu.velocity, imu.accelerometer, imu.projected_gravity):
            out.fill_(fc.POISON)
        ft.eval(s)
        imu.eval(s, sp, fc.DT)
        snap = {"transform": _np(ft.transforms), "velocity": _np(imu.velocity), "accel": _np(imu.accelerometer), "gravity_dir": _np(imu.projected_gravity)}
        assert not any(np.any(v == fc.POISON) for v in snap.values())
        return {k: wi.by_world(v, N) for k, v in snap.items()}

    A = run(fc.case(N, 3))
    assert all(np.isfinite(v).all() for v in A.values())
    for mname, aggr in wi.masks(N).items():
        case = fc.Case(N, 3)
        sel = aggr.repeat(case.nb)
        case.body_q[sel, :3] += np.float32(1.0e4)
        case.body_qd[sel] += np.array([300.0, -200.0, 100.0, 1.0e3, -1.0e3, 1.0e3], np.float32)
        wi.assert_isolated(A, run(case), aggr, f"frame sensor classes [{mname}]", differ=("transform", "velocity", "accel"))


# -- reset after divergence --------------------------------------------------------------------------------------------------------------
def _reset_sequence(model, start, aggr, which, matching):
    """Two rollouts of 6 substeps; state.reset(source, world_mask = aggressors) on both states of the pair (and the matcher's history of
    those worlds); two more rollouts.  With matching, a collide() follows every rollout: the fused rollout itself does not match."""
    import newton_amd as nt

    # SolverFeatherstone with update_mass_matrix_interval = 1: with a longer interval a reset world legitimately keeps the stale factor
    # until the next rebuild, as in the reference -- the one stated exception of the contract, not tested
    solver = _solver(nt, model, which, dict(update_mass_matrix_interval=1) if which == "featherstone" else {})
    pipe = nt.CollisionPipeline(model, **(dict(contact_matching=matching) if matching else {}))
    source = _state(model, wi.start_arrays(model))
    s0, s1, ctrl, ct = _state(model, start), _state(model, start), _control(model, start), pipe.contacts()
    snap, rows, n_rows = None, None, 0

    def frame():
        nonlocal s0, snap, rows, n_rows
        s0 = solver.rollout(s0, s1, ctrl, ct, DT[which], 6)
        assert s0 is not s1
        if matching:
            pipe.collide(s0, ct)
        snap, prev, n_prev = _snap_state(model, s0), rows, n_rows
        cs, rows, n_rows = _snap_contacts(model, ct)
        snap.update(cs)
        if matching and prev is not None:
            snap["match"] = wi.match_ordinals(_np(ct.rigid_contact_match_index), rows, prev, n_prev)

    frame(), frame()
    diverged = snap
    for s in (s0, s1):
        s.reset(source, world_mask=aggr)
    if matching:
        pipe.reset_contact_matching(aggr)
    frame()
    after_one = snap
    frame()
    return diverged, after_one, snap


@pytest.mark.parametrize("matching", [None, "sticky"], ids=["no_matching", "sticky"])
@pytest.mark.parametrize("name", ["quadruped", "mixed"])
@pytest.mark.parametrize("which", ["xpbd", "semi_implicit", "featherstone"])
def test_reset_after_divergence(which, name, matching):
    """BOTH runs go through the same sequence, the masked reset included: run A from the undisturbed start (its reset worlds never
    misbehaved), run B with "fast" aggressors.  Only so can every world be compared: after the reset every world of B -- aggressors
    included -- carries A's bits, state, contact rows and match ordinals."""
    model = _model(name, N)
    everyone = np.ones(N, bool)
    for mname, aggr in wi.masks(N).items():
        what = f"reset after divergence {which} {name} {matching} [{mname}]"
        A = _reset_sequence(model, wi.start_arrays(model), aggr, which, matching)
        B = _reset_sequence(model, wi.start_arrays(model, "fast", aggr), aggr, which, matching)
        assert all(np.isfinite(A[2][k]).all() for k in wi.STATE_FIELDS), what
        wi.assert_victims_in_contact(A[2], ~everyone, what)
        if matching:  # not vacuous: in the frame after the reset the worlds that kept their history match and the reset ones cannot; a
            # frame later the reset worlds match again (as every world did one frame after the start)
            hit1, hit2 = (np.array([np.any(m >= 0) for m in S["match"]]) for S in (A[1], A[2]))
            assert hit1[~aggr].any() and not hit1[aggr].any() and hit2[aggr].any(), f"{what}: matched contacts {hit1} {hit2}"
        wi.assert_isolated(A[0], B[0], aggr, what + " before the reset", differ=("body_q", "body_qd"))
        for stage, a, b in (("one frame", A[1], B[1]), ("two frames", A[2], B[2])):
            bad = wi.differing_worlds(a, b, everyone)
            assert not bad, f"{what}: {stage} after the reset worlds differ from the run that never diverged in {bad[:12]}"
