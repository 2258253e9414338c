"""World isolation on the emulator: the kernel SOURCES executed on the CPU (tests/emu), without a GPU, on the cases of
tests/world_isolation_cases.py -- the twin of tests/test_gpu_world_isolation.py for every entry point the suite drives on the emulator:
nt_collide, the three steppers and their fused rollouts (tests/emu/harness.py), nt_eval_fk / _ik / _jacobian / _mass_matrix /
_inverse_dynamics, nt_ik_solve, nt_raycast, nt_contact_sensor and nt_frame_sensor (the helpers of their own emulated files).  Contact
matching and the reset sequence have no emulated helper: they reach the emulated library through the dry run of the device file
(tests/emu/run_gpu_tests_emulated.py test_gpu_world_isolation.py).  Run A undisturbed, run B with disturbed AGGRESSOR worlds; everything
B wrote for the other worlds carries A's bits, the solver's per-slot impulse records included.

Every case runs with finite aggressors and with the non-finite ones (NaN position, Inf velocity, zero quaternion, NaN targets and
impulses), which live here and only here: a loop that does not terminate costs a time limit on the CPU and a shared machine on the
device.  Those runs are child processes with that limit.

The emulator runs a workgroup's lanes as threads that meet at every barrier, so a record indexed by tile slot, a prefix over the tile or
a block-shared value written from one world's data shows here; a barrier under a world-dependent condition deadlocks here (the time limit)
where the device would run on -- the device file is the check for that."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, HERE)

import world_isolation_cases as wi  # noqa: E402
from newton_amd import _lib as L  # noqa: E402

N = wi.WORLDS
DT = {"xpbd": 1e-3, "semi_implicit": 1e-4, "featherstone": 5e-4}
GENERIC = wi.GENERIC

# id -> (scene, worlds, entry, mode, substeps, options)
CASES = {
    "collide_explicit": ("mixed", N, "collide", None, 1, dict(broad_phase=0)),
    "collide_nxn": ("mixed", N, "collide", None, 1, dict(broad_phase=1)),
    "collide_sap": ("mixed", N, "collide", None, 1, dict(broad_phase=2)),
    "xpbd_step_reports": ("quadruped_low", N, "xpbd", "step", 1, dict(report=True)),  # (feet in the ground: impulses in every world)
    "xpbd_rollout": ("quadruped", N, "xpbd", "rollout", 6, {}),
    "xpbd_rollout_generic": ("quadruped", N, "xpbd", "rollout", 6, dict(cfg=GENERIC, params=False)),
    "xpbd_rollout_epb4": ("quadruped", N, "xpbd", "rollout", 6, dict(epb=4)),
    "xpbd_rollout_restitution": ("quadruped", N, "xpbd", "rollout", 6, dict(enable_restitution=True)),
    "xpbd_rollout_convex": ("quadruped_convex", 9, "xpbd", "rollout", 6, {}),
    "xpbd_rollout_box_stack": ("box_stack", 11, "xpbd", "rollout", 6, {}),
    "xpbd_rollout_mixed": ("mixed", 10, "xpbd", "rollout", 6, {}),
    "xpbd_rollout_hull_bin": ("hull_bin", 3, "xpbd", "rollout", 2, {}),
    "semi_step_quadruped": ("quadruped", N, "semi_implicit", "step", 3, {}),
    "semi_rollout_quadruped": ("quadruped", N, "semi_implicit", "rollout", 6, {}),
    "semi_step_joint_zoo": ("joint_zoo", N, "semi_implicit", "step", 3, {}),
    "semi_rollout_joint_zoo": ("joint_zoo", N, "semi_implicit", "rollout", 6, {}),
    "semi_step_d6": ("d6_angular", N, "semi_implicit", "step", 3, {}),
    "semi_rollout_d6": ("d6_angular", N, "semi_implicit", "rollout", 6, {}),
    "fs_step_tree": ("quadruped", N, "featherstone", "step", 3, {}),
    "fs_rollout_tree": ("quadruped", N, "featherstone", "rollout", 6, {}),
    "fs_step_tree_epb4": ("quadruped", N, "featherstone", "step", 3, dict(epb=4)),
    "fs_rollout_tree_epb4": ("quadruped", N, "featherstone", "rollout", 6, dict(epb=4)),
    "fs_step_dense": ("quadruped", N, "featherstone", "step", 3, dict(dense=True)),
    "fs_rollout_dense": ("quadruped", N, "featherstone", "rollout", 6, dict(dense=True)),
    "fs_step_dense_epb4": ("quadruped", N, "featherstone", "step", 3, dict(dense=True, epb=4)),
    "fs_rollout_dense_epb4": ("quadruped", N, "featherstone", "rollout", 6, dict(dense=True, epb=4)),
    "fs_step_multi_art_interval2": ("multi_art", N, "featherstone", "step", 5, dict(update_mass_matrix_interval=2)),
    "fs_rollout_multi_art_interval2": ("multi_art", N, "featherstone", "rollout", 5, dict(update_mass_matrix_interval=2)),
    "fs_step_free_child": ("free_child", N, "featherstone", "step", 5, {}),
    "fs_rollout_free_child": ("free_child", N, "featherstone", "rollout", 5, {}),
    "fs_step_free_child_epb16": ("free_child", N, "featherstone", "step", 5, dict(epb=16)),
    "fs_rollout_free_child_epb16": ("free_child", N, "featherstone", "rollout", 5, dict(epb=16)),
}
HEAVY = ("hull_bin", "quadruped_convex")  # (every kind once, the masks in turn; everywhere else every kind under every mask)
NO_CONTACTS = ("multi_art",)  # (in free flight: no contact in a dozen steps)


@pytest.fixture(scope="module")
def H(oracle_lib):
    import harness

    harness.lib()  # builds tests/emu/_build/libnewton_emu.so on first use
    return harness


def _semi_implicit_rollout(H, em, s0, s1, control, contacts, dt, substeps, epb=0):
    p, cp = L.nt_semi_implicit_params(0.05, 1.0, 1.0e4, 1.0e2), L.nt_collide_params(0, epb)
    d0, d1, dc, dct = s0.desc(), s1.desc(), control.desc(), contacts.desc()
    H.check(H.lib().nt_semi_implicit_rollout(C.byref(em.desc), C.byref(p), C.byref(cp), C.byref(d0), C.byref(d1), C.byref(dc), C.byref(dct),
                                             float(dt), int(substeps), None), "nt_semi_implicit_rollout")
    return s1 if substeps % 2 else s0


def _run(H, model, start, entry, mode, substeps, opt):
    """One run on the emulated library -> snapshot (state, contact rows by world, the solver's impulse records by world)."""
    em = H.EmuModel(model)
    t, E = em.t, em.t.env_count
    opt = dict(opt)
    epb, report, cfg = opt.pop("epb", 0), opt.pop("report", False), opt.pop("cfg", None)
    opt.pop("params", None)
    new_state = lambda: H.EmuState(em, **{k: start[k] for k in wi.STATE_FIELDS}, parent_f=report)  # noqa: E731
    s0, s1, ct = new_state(), new_state(), H.EmuContacts(em)
    ctrl = H.EmuControl(em, **{k: start[k] for k in wi.CONTROL_FIELDS})
    snap, dt = {}, DT.get(entry)
    with wi.xpbd_cfg(cfg):
        if entry == "collide":
            ds, dc, p = s0.desc(), ct.desc(), L.nt_collide_params(opt["broad_phase"], epb)
            H.check(H.lib().nt_collide(C.byref(em.desc), C.byref(ds), C.byref(dc), C.byref(p), None), "nt_collide")
        elif entry == "xpbd" and mode == "rollout":
            s0 = H.xpbd_rollout(em, s0, s1, ctrl, ct, dt, substeps, epb=epb, **opt)
        elif entry == "semi_implicit" and mode == "rollout":
            s0 = _semi_implicit_rollout(H, em, s0, s1, ctrl, ct, dt, substeps, epb)
        else:
            fs = {}
            if entry == "featherstone":
                fs = dict(opt)
                if opt.get("update_mass_matrix_interval", 1) > 1:  # the factor kept between rebuilds: [nd * max_art_dofs][env_stride]
                    fs["cache"] = np.zeros((max(t.nd * t.max_art_dofs, 1), t.env_stride), np.float32)
            if mode == "rollout":
                s0 = H.featherstone_rollout(em, s0, s1, ctrl, ct, dt, substeps, epb=epb, **fs)
            rep = None
            if report:
                ns = max(t.np * t.cpp, 1)
                contact_impulse = np.zeros((6, ns, t.env_stride), np.float32)
                joint_impulse = np.zeros((6, max(t.nj, 1), t.env_stride), np.float32)
                rep = L.nt_xpbd_report()
                rep.contact_impulse, rep.joint_impulse = contact_impulse.ctypes.data, joint_impulse.ctypes.data
            for i in range(substeps if mode == "step" else 0):
                s0.body_f[:] = 0
                H.collide(em, s0, ct, epb=epb)
                if entry == "xpbd":
                    H.xpbd_step(em, s0, s1, ctrl, ct, dt, epb=epb, report=rep, **opt)
                elif entry == "semi_implicit":
                    H.semi_implicit_step(em, s0, s1, ctrl, ct, dt, epb=epb)
                else:
                    H.featherstone_step(em, s0, s1, ctrl, ct, dt, epb=epb, step_index=i, **fs)
                s0, s1 = s1, s0
            if report:
                snap["contact_impulse"] = contact_impulse[:, :, :E].transpose(2, 0, 1).copy()
                snap["joint_impulse"] = joint_impulse[:, :, :E].transpose(2, 0, 1).copy()
                snap["body_parent_f"] = wi.by_world(s0.aos("body_parent_f"), E)
            if "cache" in fs:
                snap["factor_cache"] = fs["cache"][:, :E].T.copy()
    if entry != "collide":
        snap.update({k: wi.by_world(s0.aos(k), E) for k in wi.STATE_FIELDS})
    if t.np > 0:
        cs, rows = wi.contact_rows(model, ct.export())
        snap.update(cs)
        snap["contact_count"] = ct.env_count[:E].copy()
        assert [len(r) for r in rows] == list(snap["contact_count"])
    return snap


def _case(H, case, kinds=None, params=True):
    name, n, entry, mode, substeps, opt = CASES[case]
    model = wi.scene(name, n)
    run = lambda m, st: _run(H, m, st, entry, mode, substeps, opt)  # noqa: E731
    contacts = model.env.np > 0 and name not in NO_CONTACTS
    A = run(model, wi.start_arrays(model))
    written = [k for k in wi.STATE_FIELDS if k in A]
    assert all(np.isfinite(A[k]).all() for k in written), case
    if contacts:
        wi.assert_victims_in_contact(A, np.zeros(n, bool), case)
    if "contact_impulse" in A:  # (not vacuous: every world reports a contact impulse and a joint impulse)
        assert np.all(np.any(A["contact_impulse"] != 0.0, axis=(1, 2))) and np.all(np.any(A["joint_impulse"] != 0.0, axis=(1, 2))), case
    count = lambda st: _run(H, model, st, "collide", None, 1, dict(broad_phase=0))  # noqa: E731
    start_contacts = count(wi.start_arrays(model)) if contacts else None
    if kinds is None:
        kinds = ("far", "deep") if entry == "collide" else wi.kinds_for(model, contacts)
        kinds += ("pressed",) if name in wi.PRESSED and contacts else ()
    for kind, mname, aggr in (wi.rotated if name in HEAVY else wi.combos)(n, kinds):
        tag = f"{case} [{kind}, {mname}]"
        B = run(model, wi.start_arrays(model, kind, aggr, wi.depth(name, kind)))
        wi.assert_isolated(A, B, aggr, tag, differ=written or None)
        if contacts and kind in ("far", "deep", "pressed"):  # (the live-contact lists the run starts from)
            wi.assert_contact_totals_differ(start_contacts, count(wi.start_arrays(model, kind, aggr, wi.depth(name, kind))), aggr, tag)
    if params and entry != "collide" and opt.get("params", True):  # (the forced generic instance is the uniform-parameter one)
        edited = wi.scene(name, n)
        pristine = wi.pristine_params(edited)
        assert H.EmuModel(model).desc.params_uniform == 1
        for mname, aggr in list(wi.masks(n).items())[:1 if name in HEAVY else None]:
            wi.edit_params(edited, aggr, pristine)
            assert H.EmuModel(edited).desc.params_uniform == 0
            wi.assert_isolated(A, run(edited, wi.start_arrays(edited)), aggr, f"{case} [params, {mname}]")


# -- the kinematics, IK and sensor entry points: EXTRA id -> function(H, kinds) --------------------------------------------------------------
POISON = -7.25e3


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _pairs(run, n, variants, what, differ):
    """run(None) is run A; run((kind, aggressors)) run B, for every kind under every mask."""
    A = run(None)
    assert all(np.isfinite(np.asarray(A[k], np.float64)).all() for k in differ), what
    for kind in variants:
        for mname, aggr in wi.masks(n).items():
            wi.assert_isolated(A, run((kind, aggr)), aggr, f"{what} [{kind}, {mname}]", differ=differ)


def _kinematics(H, name, kinds):
    """nt_eval_fk, nt_eval_ik, nt_eval_jacobian, nt_eval_mass_matrix, nt_eval_inverse_dynamics (bias forces alone and with joint_qdd)
    into poisoned outputs; one articulation per world in both scenes."""
    model = wi.scene(name, N)
    em = H.EmuModel(model)
    t, lib, m = em.t, H.lib(), C.byref(em.desc)
    L_, D, A_ = model.max_joints_per_articulation, model.max_dofs_per_articulation, model.articulation_count
    assert A_ == N
    qdd = np.random.default_rng(3).normal(0.0, 2.0, size=(A_, D)).astype(np.float32)

    def run(variant):
        start = wi.start_arrays(model) if variant is None else wi.start_arrays(model, variant[0], variant[1], wi.depth(name, variant[0]))
        s = H.EmuState(em, **{k: start[k] for k in wi.STATE_FIELDS})
        s.body_q[:], s.body_qd[:] = POISON, POISON
        d = s.desc()
        H.check(lib.nt_eval_fk(m, _p(s.joint_q), _p(s.joint_qd), C.byref(d), None), "nt_eval_fk")
        snap = {"fk_body_q": s.aos("body_q"), "fk_body_qd": s.aos("body_qd")}
        jq, jqd = np.full_like(s.joint_q, POISON), np.full_like(s.joint_qd, POISON)
        H.check(lib.nt_eval_ik(m, C.byref(d), _p(jq), _p(jqd), None, None), "nt_eval_ik")
        snap["ik_joint_q"], snap["ik_joint_qd"] = em.to_aos(jq, 1, t.nc), em.to_aos(jqd, 1, t.nd)
        J, Hm = np.full((A_, 6 * L_, D), POISON, np.float32), np.full((A_, D, D), POISON, np.float32)
        S, I = np.full((model.joint_dof_count, 6), POISON, np.float32), np.full((model.body_count, 6, 6), POISON, np.float32)  # noqa: E741
        H.check(lib.nt_eval_jacobian(m, C.byref(d), _p(J), _p(S), None, None), "nt_eval_jacobian")
        H.check(lib.nt_eval_mass_matrix(m, C.byref(d), _p(Hm), _p(I), None, None), "nt_eval_mass_matrix")
        bias, tau = np.full((A_, D), POISON, np.float32), np.full((A_, D), POISON, np.float32)
        H.check(lib.nt_eval_inverse_dynamics(m, C.byref(d), None, 3, _p(bias), None, None), "nt_eval_inverse_dynamics")  # (3: gravity | velocity)
        H.check(lib.nt_eval_inverse_dynamics(m, C.byref(d), _p(qdd), 3, _p(tau), None, None), "nt_eval_inverse_dynamics")
        snap.update(J=J, H=Hm, S=S, I=I, bias=bias, tau=tau)
        assert not any(np.any(v == POISON) for v in snap.values()), "the poison is still there"
        return {k: wi.by_world(v, N) for k, v in snap.items()}

    _pairs(run, N, kinds or wi.kinds_for(model), f"kinematics {name}", ("fk_body_q", "fk_body_qd", "H", "tau"))


def _ik_solve(H, name, kinds):
    """nt_ik_solve_tile, ten iterations in the launch: the aggressors' position targets 1e3 m away (unreachable), or NaN targets and an
    Inf start coordinate."""
    from ik_cases import ik_case, make_objectives, objective_specs
    from ik_parity import device_problem
    from newton_amd import ik

    model, _, targets, start = ik_case(name, N, 5)
    em = H.EmuModel(model)

    def run(variant):
        tg, q_in = [None if t is None else np.array(t, copy=True) for t in targets], start.astype(np.float32)
        if variant is not None:
            for (kind, _link), t in zip(objective_specs(name, model), tg):
                if kind == "position":
                    t[variant[1]] = np.nan if variant[0] == wi.NON_FINITE else t[variant[1]] + np.float32(1.0e3)
            if variant[0] == wi.NON_FINITE:
                q_in[variant[1], 0] = np.inf
        solver = ik.IKSolver(model, make_objectives(name, model, tg))
        prob = device_problem(solver)
        q_in = np.ascontiguousarray(q_in)
        q_out, lam, cost = np.full_like(q_in, 7.0), np.full(N, solver.lambda_initial, np.float32), np.full(N, 7.0, np.float32)
        H.check(H.lib().nt_ik_solve_tile(C.byref(em.desc), C.byref(prob.desc), _p(q_in), _p(q_out), _p(lam), _p(cost), 10, 1.0, 0, None),
                "nt_ik_solve_tile")
        return {"joint_q": wi.by_world(q_out, N), "cost": wi.by_world(cost, N), "lambda": wi.by_world(lam, N)}

    _pairs(run, N, kinds or ("unreachable",), f"ik {name}", ("joint_q", "cost"))


def _raycast(H, name, kinds):
    """nt_raycast on the primitive scene of tests/raycast_cases.py (70 rays, some attached to bodies): the aggressors' bodies 1e4 m away,
    moved by a body width, or at NaN positions with zero quaternions."""
    import raycast_cases as rc

    model, rays, _kw, ref = rc.case(name)
    em = H.EmuModel(model)
    E = model.env.env_count
    moves = {"far": np.array([1.0e4, -1.0e4, 1.0e4], np.float32), "near": np.array([0.15, -0.1, 0.2], np.float32)}

    def run(variant):
        bq = np.array(model.body_q, np.float32, copy=True)
        if variant is not None:
            sel = variant[1].repeat(model.env.nb)
            if variant[0] == wi.NON_FINITE:
                bq[sel, 0], bq[sel, 3:] = np.nan, 0.0
            else:
                bq[sel, :3] += moves[variant[0]]
        args = rc.HostArgs(model, rays, ref["slots"])
        H.check(rc.emu_cast(H, em, H.EmuState(em, body_q=bq), args), "nt_raycast")
        assert not np.any(args.distance == 7.0) and not np.any(args.shape == -7)
        return {"distance": wi.by_world(args.distance, E), "normal": wi.by_world(args.normal, E), "shape": wi.by_world(args.shape, E)}

    assert E == N
    _pairs(run, E, kinds or tuple(moves), f"raycast {name}", ("distance",))


def _contact_sensor(H, name, kinds):
    """nt_contact_sensor on the synthetic exact case of tests/contact_sensor_cases.py (50 slots, ragged rows, 4 x 4 cells and totals): the
    aggressors' impulses 2^20 times as large, or NaN / Inf."""
    import contact_sensor_cases as cs

    model = cs.sensor_model(N)
    em = H.EmuModel(model)

    def run(variant):
        case = cs.exact_case(model, 50, *cs.SHAPES[name], rows="ragged", seed=4)
        if variant is not None:
            for w in np.flatnonzero(variant[1]):
                rows = slice(int(case.row_start[w]), int(case.row_start[w + 1]))
                if variant[0] == wi.NON_FINITE:
                    case.impulse[::2, :, w], case.impulse[1::2, :, w], case.rimpulse[rows, ::2], case.rimpulse[rows, 1::2] = np.nan, np.inf, np.inf, np.nan
                else:
                    case.impulse[:, :, w] *= np.float32(2.0 ** 20)
                    case.rimpulse[rows] *= np.float32(2.0 ** 20)
        call = cs.HostCall(case, em.desc)
        H.check(call.run(H.lib()), "nt_contact_sensor")
        assert not np.any(call.net_force == cs.POISON)
        return {"net_force": wi.by_world(call.net_force, N)}

    A = run(None)["net_force"]
    assert np.all(np.any(A != 0.0, axis=1)), "worlds without any net force"
    _pairs(run, N, kinds or ("large",), f"contact sensor {name}", ("net_force",))


EXTRA = {"kinematics_joint_zoo": (_kinematics, "joint_zoo"), "kinematics_quadruped": (_kinematics, "quadruped"),
         "ik_solve_quadruped": (_ik_solve, "quadruped"), "ik_solve_joint_zoo_free_root": (_ik_solve, "joint_zoo_free_root"),
         "raycast_primitives": (_raycast, "primitives"), "contact_sensor_cells20": (_contact_sensor, "cells20")}


def _any_case(H, case, non_finite=False):
    with np.errstate(all="ignore"):
        if case in EXTRA:
            fn, name = EXTRA[case]
            fn(H, name, (wi.NON_FINITE,) if non_finite else None)
        elif non_finite:
            _case(H, case, kinds=(wi.NON_FINITE,), params=False)
        else:
            _case(H, case)


@pytest.mark.parametrize("case", sorted(CASES) + sorted(EXTRA))
def test_finite_aggressors(H, case):
    _any_case(H, case)


@pytest.mark.parametrize("case", sorted(CASES) + sorted(EXTRA))
def test_non_finite_aggressors(H, case):
    """NaN / Inf / zero-quaternion aggressors, in a child process under a time limit (H: the library is built before the clock starts)."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(HERE), os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case], cwd=HERE, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "isolated" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.parametrize("kind", ["fast_far", wi.NON_FINITE])
def test_frame_sensors(H, kind):
    """nt_frame_sensor (SensorFrameTransform / SensorIMU) on the shared case of tests/frame_sensor_cases.py, 70 rows: aggressor worlds far
    away and fast, or with a NaN position, an Inf velocity and a zero quaternion.  (No loop of this kernel depends on its data: in process.)"""
    import frame_sensor_cases as fc

    def run(case):
        em = H.EmuModel(case.model)
        s, sp = H.EmuState(em, body_q=case.body_q, body_qd=case.body_qd), H.EmuState(em, body_q=case.body_q, body_qd=case.body_qd_prev)
        call = fc.Call(case)
        ds, dp = s.desc(), sp.desc()
        H.check(call.run(H.lib(), em.desc, ds, dp), "nt_frame_sensor")
        return {k: wi.by_world(v, case.E) for k, v in call.out.items()}

    A = run(fc.case(N, 70))
    assert set(A) == set(fc.OUTPUTS) and all(np.isfinite(v).all() and not np.any(v == fc.POISON) for v in A.values())
    for mname, aggr in wi.masks(N).items():
        case = fc.Case(N, 70)
        sel = aggr.repeat(case.nb)
        if kind == wi.NON_FINITE:
            case.body_q[sel, 0], case.body_q[sel, 3:], case.body_qd[sel, 1] = np.nan, 0.0, np.inf
        else:
            case.body_q[sel, :3] += np.float32(1.0e4)
            case.body_qd[sel] += np.array([300.0, -200.0, 100.0, 1.0e3, -1.0e3, 1.0e3], np.float32)
        with np.errstate(all="ignore"):
            wi.assert_isolated(A, run(case), aggr, f"frame sensors {kind} [{mname}]", differ=("transform", "velocity", "accel"))


if __name__ == "__main__":
    import harness

    harness.lib()
    _any_case(harness, sys.argv[1], non_finite=True)
    print("isolated:", sys.argv[1])
