"""newton_amd.eval_forward_dynamics on the host: the numpy path against the float64 reference of tests/forward_dynamics_reference.py on
every scene and on a heterogeneous model, closed forms (planar pendulums, a free box), the round trips with eval_inverse_dynamics, the
flags, padding, selection, a massless leaf link, the C header against the ctypes table, and the CPU oracle's Featherstone step.

The cases and the gates below are shared with tests/test_forward_dynamics_emu.py and tests/test_gpu_forward_dynamics.py.
Error measure everywhere (forward_dynamics_reference.fd_eta): the normwise backward error per articulation
  eta = |H_ref qdd - b_ref|_inf / (|H_ref|_inf |qdd|_inf + max(1, |joint_f|_inf, |h_ref|_inf, |tau_ext_ref|_inf))
  numpy path     1e-6: both sides are float64 (the result is rounded to fp32 once, 6e-8)
  fp32 kernel    FD_GATE = 4 x the largest per-scene maximum of eta measured on the emulator (37 worlds, seed 21, all three flags on,
                 every tile the same bits), the rule ID_GATE was set by.  Measured maxima, emulator:
                   d6_zoo 4.264e-08   free_child 6.871e-08   free_child_free_root 2.846e-08   joint_zoo 6.112e-08
                   joint_zoo_free_root 4.221e-08   multi_art 1.124e-07   pendulum 1.389e-07   quadruped 4.129e-09
                 (far below the 1e-5 the kernel's H is itself allowed; D 2^-24 is 1.2e-6 at D = 20.  The plain forward error on the
                 same runs is 1.2e-6 .. 2.5e-4 of max|qdd_ref| at cond(H_ref) 35 .. 3.9e4: printed, never asserted.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import newton_amd as nt
from forward_dynamics_reference import (fd_denominator, fd_eta, fd_forward_error, forward_dynamics_reference, random_forces)
from inverse_dynamics_reference import inverse_dynamics_reference, pad_dofs, random_rates
from newton_amd import _lib
from newton_amd import _np_math as nm
from newton_amd.articulation import (_eval_fk_float64, eval_fk_numpy, eval_forward_dynamics_numpy, eval_inverse_dynamics_numpy)
from test_eval_ik_host import random_joint_state
from test_eval_jacobian_host import POISON, SCENES, _host_state, planar_pendulum
from test_inverse_dynamics_host import compensation_scene, compensation_state, id_case, pendulum_lagrange

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "newton_hip_kinematics.h")
HOST_GATE = 1e-6
FD_GATE = 4 * 1.389e-07  # (see above: pendulum)
N_WORLDS = 37
SEED = 21


class FdCase:
    """id_case's scene and state (q, qd ~ U(-2, 2), eval_fk's fp32 body state) with joint_f ~ U(-10, 10) and body_f (force ~ U(-20, 20),
    torque ~ U(-2, 2)); the references are made once per flag combination and only read."""

    def __init__(self, name, E, seed, device=None):
        self.id = id_case(name, E, seed, device)
        self.model, self.D = self.id.model, self.id.D
        self.joint_f, self.body_f = random_forces(self.model, seed + 200, self.D)
        self.nda = np.array([hi - lo for lo, hi in self.id.dof_ranges])
        self._refs = {}

    def ref(self, joint_f=True, body_f=True, gravity=True, velocity_terms=True, f64=False):
        key = (joint_f, body_f, gravity, velocity_terms, f64)
        if key not in self._refs:
            c = self.id
            self._refs[key] = forward_dynamics_reference(self.model, c.bq64 if f64 else c.bq, c.jq, c.qd, self.joint_f if joint_f else None,
                                                         self.body_f if body_f else None, gravity, velocity_terms)
        return self._refs[key]

    def state(self, f64=False):
        s = self.id.state(f64)
        s.body_f = self.body_f
        return s


_CASES = {}


def fd_case(name, E=N_WORLDS, seed=SEED, device=None):
    key = (name, E, seed, device)
    if key not in _CASES:
        _CASES[key] = FdCase(name, E, seed, device)
    return _CASES[key]


def report(tag, name, qdd, ref):
    eta = fd_eta(qdd, ref)
    print(f"[eval_forward_dynamics {tag}] {name}: eta {eta:.3e}, |qdd - qdd_ref| / max(1, |qdd_ref|) {fd_forward_error(qdd, ref):.3e}, "
          f"cond(H_ref) {ref.cond.max():.3e}, max|qdd_ref| {np.abs(ref.qdd).max():.1f}")
    return eta


def massless_leaf_model(name, E, device=None):
    """The scene with one leaf link -- the child of the last joint of articulation 0 -- without mass and inertia in the worlds
    w % 3 == 1.  The builder refuses a massless link, so the arrays of the finalised model are zeroed (the "params" aggressor of
    tests/world_isolation_cases.py edits them the same way).  Returns (model, bad [E * na] bool)."""
    model = SCENES[name](E, device=device) if device else SCENES[name](E)
    t = model.env
    leaf = int(t.joint_child[int(t.art_start[1]) - 1])
    worlds = np.flatnonzero(np.arange(E) % 3 == 1)
    rows = worlds * t.nb + leaf
    for k in ("body_mass", "body_inertia", "body_inv_mass", "body_inv_inertia"):
        getattr(model, k)[rows] = 0.0
    model.notify_model_changed()
    bad = np.zeros((E, t.na), dtype=bool)
    bad[worlds, 0] = True
    return model, bad.reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the numpy path against the reference; closed forms; round trips; flags
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENES))
def test_numpy_path_matches_reference(name):
    """Both sides float64 on the same unrounded poses; the result is rounded to fp32 once."""
    c = fd_case(name, 5, 5)
    s = c.state(f64=True)
    info = np.full(c.model.articulation_count, -1, np.int32)
    qdd = nt.eval_forward_dynamics(c.model, s, c.joint_f, body_f=True, info=info)
    assert qdd.dtype == np.float32 and qdd.shape == (c.model.articulation_count, c.D) and np.all(info == 0)
    eta = report("numpy", name, qdd, c.ref(f64=True))
    assert eta <= HOST_GATE, (name, eta)
    assert all(np.all(qdd[a, n:] == 0.0) for a, n in enumerate(c.nda))
    # each of gravity, velocity terms and body_f off, against the reference with the same part removed
    for kw in (dict(gravity=False), dict(velocity_terms=False), dict(body_f=False)):
        got = nt.eval_forward_dynamics(c.model, s, c.joint_f, **{**dict(body_f=True), **kw})
        assert fd_eta(got, c.ref(f64=True, **kw)) <= HOST_GATE, (name, kw)
        assert not np.array_equal(got, qdd)  # the part is live
    got = nt.eval_forward_dynamics(c.model, s, None, body_f=True)
    assert fd_eta(got, c.ref(f64=True, joint_f=False)) <= HOST_GATE


def test_everything_off_is_exactly_zero():
    c = fd_case("joint_zoo_free_root", 5, 5)
    out = np.full((c.model.articulation_count, c.D), POISON, np.float32)
    qdd = nt.eval_forward_dynamics(c.model, c.state(), None, out, body_f=False, gravity=False, velocity_terms=False)
    assert qdd is out and np.all(qdd == 0.0)


def test_heterogeneous_model():
    from test_heterogeneous_worlds import mixed_model

    model = mixed_model((("quadruped", 2), ("boxes3", 1), ("pendulum", 2), ("quadruped", 1)))
    assert model.is_heterogeneous
    parts = model.world_groups.parts
    jq = np.concatenate([random_joint_state(p, 2 + i)[0] for i, p in enumerate(parts)])
    D = int(model.max_dofs_per_articulation)
    qd, _ = random_rates(model, 9, D)
    joint_f, body_f = random_forces(model, 10, D)
    bq, bqd = eval_fk_numpy(model, jq, qd)
    s = model.state()
    s.body_q, s.body_qd, s.joint_q, s.joint_qd, s.body_f = bq, bqd, jq, qd, body_f
    info = np.full(model.articulation_count, -1, np.int32)
    qdd = nt.eval_forward_dynamics(model, s, joint_f, body_f=True, info=info)
    assert qdd.shape == (model.articulation_count, D) and D == 18 and np.all(info == 0)
    # the reference group by group (its finite difference needs one replicated model), into the global padding
    b0 = c0 = d0 = a0 = 0
    worst = 0.0
    for p in parts:
        b1, c1, d1, a1 = b0 + p.body_count, c0 + p.joint_coord_count, d0 + p.joint_dof_count, a0 + p.articulation_count
        if p.articulation_count:
            Dp = int(p.max_dofs_per_articulation)
            ref = forward_dynamics_reference(p, bq[b0:b1], jq[c0:c1], qd[d0:d1], joint_f[a0:a1, :Dp], body_f[b0:b1])
            worst = max(worst, fd_eta(qdd[a0:a1, :Dp], ref))
            assert np.all(qdd[a0:a1, Dp:] == 0.0)
        b0, c0, d0, a0 = b1, c1, d1, a1
    print(f"[eval_forward_dynamics numpy] heterogeneous: eta {worst:.3e}")
    assert worst <= HOST_GATE
    assert np.array_equal(qdd, eval_forward_dynamics_numpy(model, bq, jq, qd, joint_f, body_f))
    sel = np.arange(model.articulation_count) % 2 == 0
    part, pinfo = np.full_like(qdd, POISON), np.full(model.articulation_count, -7, np.int32)
    nt.eval_forward_dynamics(model, s, joint_f, part, body_f=True, info=pinfo, mask=sel)
    assert np.array_equal(part[sel], qdd[sel]) and np.all(part[~sel] == POISON)
    assert np.all(pinfo[sel] == 0) and np.all(pinfo[~sel] == -7)


@pytest.mark.parametrize("links", [1, 2, 3])
def test_planar_pendulum_closed_forms(links):
    """pendulum_lagrange is linear in qdd: its columns give H, its value at qdd = 0 gives h; solved in float64."""
    model = planar_pendulum(links)
    g = np.asarray(model.gravity, dtype=np.float64).reshape(-1, 3)[0]
    q = np.array([0.7, -1.1, 0.4][:links], np.float32)
    qd = np.array([1.3, -0.8, 1.9][:links], np.float32)
    joint_f = np.array([[2.5, -4.0, 1.5][:links]], np.float32)
    bq64, _ = _eval_fk_float64(model, q, qd)
    q64, qd64 = q.astype(np.float64), qd.astype(np.float64)
    for kw, use in ((dict(), (1, 1)), (dict(velocity_terms=False), (0, 1)), (dict(gravity=False), (1, 0))):
        h = pendulum_lagrange(model, q64, qd64 * use[0], np.zeros(links), g[2] * use[1])
        H = np.stack([pendulum_lagrange(model, q64, qd64 * use[0], np.eye(links)[k], g[2] * use[1]) - h for k in range(links)], axis=1)
        want = np.linalg.solve(H, joint_f[0].astype(np.float64) - h)
        qdd = eval_forward_dynamics_numpy(model, bq64.reshape(-1, 7), q, qd, joint_f, **kw)
        assert np.abs(qdd[0] - want).max() <= 1e-6 * max(1.0, np.abs(want).max()), (links, kw, qdd, want)
        assert np.abs(want).max() > 1.0


def free_box(worlds=1, device=None):
    """One free box with three different principal inertias and an offset COM."""
    env = nt.ModelBuilder()
    cfg = nt.ModelBuilder.ShapeConfig(has_shape_collision=False)
    b = env.add_link(xform=[0.2, -0.1, 1.0, 0, 0, 0, 1])
    env.add_shape_box(b, xform=nm.transform([0.05, -0.02, 0.03]), hx=0.3, hy=0.1, hz=0.05, cfg=cfg)
    env.add_articulation([env.add_joint_free(b)])
    scene = nt.ModelBuilder()
    scene.replicate(env, worlds)
    return scene.finalize(device=device)


def test_free_box_closed_form():
    """The public FREE convention carries the COM: with joint_f = 0 the linear qdd is g and the angular one -I_w^-1 (w x I_w w); a
    body_f wrench (F, T) at the COM gives g + F / m and I_w^-1 (T - w x I_w w)."""
    from newton_amd.articulation import _qrot

    model = free_box()
    Ib = np.asarray(model.body_inertia, dtype=np.float64).reshape(3, 3)
    assert len({round(float(x), 6) for x in np.linalg.eigvalsh(Ib)}) == 3
    rng = np.random.default_rng(3)
    quat = rng.normal(size=4)
    quat /= np.linalg.norm(quat)
    jq = np.concatenate([[0.3, -0.2, 1.1], quat]).astype(np.float32)
    qd = rng.uniform(-2.0, 2.0, 6).astype(np.float32)
    bq64, _ = _eval_fk_float64(model, jq, qd)
    bq64 = bq64.reshape(-1, 7)
    R = np.stack([_qrot(bq64[:, 3:], np.eye(3)[k][None]) for k in range(3)], axis=-1)[0]
    I_w = R @ Ib @ R.T
    # the joint's angular rate is in the parent anchor frame: the world for a root joint with an identity parent anchor
    assert np.allclose(np.asarray(model.joint_X_p, dtype=np.float64).reshape(-1, 7)[0], [0, 0, 0, 0, 0, 0, 1])
    w = qd[3:].astype(np.float64)
    g = np.asarray(model.gravity, dtype=np.float64).reshape(-1, 3)[0]
    mass = float(np.asarray(model.body_mass)[0])
    gyro = np.cross(w, I_w @ w)
    qdd = eval_forward_dynamics_numpy(model, bq64, jq, qd)
    want = np.concatenate([g, -np.linalg.solve(I_w, gyro)])
    assert np.abs(qdd[0] - want).max() <= 1e-6 * max(1.0, np.abs(want).max()), (qdd, want)
    assert np.abs(want[3:]).max() > 0.1
    wrench = np.concatenate([rng.uniform(-20, 20, 3), rng.uniform(-2, 2, 3)]).astype(np.float32)[None]
    qdd = eval_forward_dynamics_numpy(model, bq64, jq, qd, None, wrench)
    want = np.concatenate([g + wrench[0, :3] / mass, np.linalg.solve(I_w, wrench[0, 3:] - gyro)])
    assert np.abs(qdd[0] - want).max() <= 1e-6 * max(1.0, np.abs(want).max()), (qdd, want)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_round_trip_through_inverse_dynamics(name):
    """ID(qdd = FD(joint_f)) == joint_f to 1e-6 of the denominator of eta (both float64 inside, each result rounded to fp32 once)."""
    c = fd_case(name, 5, 5)
    i = c.id
    qdd = eval_forward_dynamics_numpy(c.model, i.bq64, i.jq, i.qd, c.joint_f)
    back = eval_inverse_dynamics_numpy(c.model, i.bq64, i.jq, i.qd, qdd)
    den = fd_denominator(c.ref(body_f=False, f64=True), qdd)
    err = (np.abs(back.astype(np.float64) - c.joint_f).max(axis=1) / den).max()
    print(f"[eval_forward_dynamics numpy] {name}: ID(FD(joint_f)) - joint_f over the denominator {err:.3e}")
    assert err <= HOST_GATE


@pytest.mark.parametrize("name", ["pendulum", "joint_zoo", "quadruped"])
def test_converse_round_trip(name):
    """FD(ID(qdd)) == qdd: the backward error of the returned qdd against b = H_ref qdd_in is within the host gate."""
    c = fd_case(name, 5, 5)
    i = c.id
    tau = eval_inverse_dynamics_numpy(c.model, i.bq64, i.jq, i.qd, i.qdd)
    qdd = eval_forward_dynamics_numpy(c.model, i.bq64, i.jq, i.qd, tau)
    ref = c.ref(body_f=False, f64=True)
    res = np.abs(np.einsum("aij,aj->ai", ref.H, qdd.astype(np.float64) - i.qdd)).max(axis=1)
    err = (res / fd_denominator(ref, qdd)).max()
    print(f"[eval_forward_dynamics numpy] {name}: |H (FD(ID(qdd)) - qdd)| over the denominator {err:.3e}")
    assert err <= 2.0 * HOST_GATE  # (two calls, each allowed the gate)
    assert np.abs(i.qdd).max() > 1.0


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. padding, selection, refusals, the massless leaf
# ---------------------------------------------------------------------------------------------------------------------------------
def test_output_into_caller_array_and_poisoned_padding():
    c = fd_case("multi_art", 4, 2)
    s = c.state()
    qdd = nt.eval_forward_dynamics(c.model, s, c.joint_f, body_f=True)
    out = np.full_like(qdd, POISON)
    assert nt.eval_forward_dynamics(c.model, s, c.joint_f, out, body_f=True) is out
    assert np.array_equal(out, qdd)  # the padding is written (zero) on every call
    assert c.model.env.na == 3 and qdd.shape == (12, 6) and np.all(qdd[2, 2:] == 0.0) and np.all(qdd[2, :2] != 0.0)
    joint_f = c.joint_f.copy()
    joint_f[2::3, 2:] = POISON  # what the padding of joint_f holds does not matter
    assert np.array_equal(nt.eval_forward_dynamics(c.model, s, joint_f, body_f=True), qdd)


def test_mask_leaves_unselected_rows_and_info_untouched_bit_for_bit():
    c = fd_case("multi_art", 6, 4)
    s = c.state()
    qdd = nt.eval_forward_dynamics(c.model, s, c.joint_f, body_f=True)
    sel = np.random.default_rng(3).random(c.model.articulation_count) < 0.5
    assert sel.any() and not sel.all()
    part, info = np.full_like(qdd, POISON), np.full(c.model.articulation_count, -7, np.int32)
    nt.eval_forward_dynamics(c.model, s, c.joint_f, part, body_f=True, info=info, mask=sel)
    assert np.array_equal(part[sel], qdd[sel]) and np.all(part[~sel] == POISON)
    assert np.all(info[sel] == 0) and np.all(info[~sel] == -7)
    with pytest.raises(ValueError, match="mask has 3 entries"):
        nt.eval_forward_dynamics(c.model, s, mask=[True, False, True])


def test_articulation_view_world_mask():
    c = fd_case("multi_art", 4, 8)
    s = c.state()
    view = nt.selection.ArticulationView(c.model, str(list(c.model.articulation_label)[2]))  # the pendulum: third articulation of every world
    qdd = nt.eval_forward_dynamics(c.model, s, c.joint_f, body_f=True)
    got = view.eval_forward_dynamics(s, c.joint_f, body_f=True)
    assert got.shape == (4, 6) and np.array_equal(got, qdd.reshape(4, 3, 6)[:, 2])
    buf = np.full_like(qdd, POISON)
    got = view.eval_forward_dynamics(s, c.joint_f, buf, mask=[True, False, True, False], body_f=True)
    assert np.array_equal(got[[0, 2]], qdd.reshape(4, 3, 6)[[0, 2], 2]) and np.all(got[[1, 3]] == POISON)
    assert np.all(buf.reshape(4, 3, 6)[[1, 3]] == POISON)  # every articulation of an unselected world
    with pytest.raises(ValueError, match="one entry per world"):
        view.eval_forward_dynamics(s, mask=[True, False])


def test_model_without_articulations_is_refused():
    env = nt.ModelBuilder()
    b = env.add_link(xform=[0.0, 0.0, 1.0, 0, 0, 0, 1])
    env.add_shape_box(b, hx=0.1, hy=0.05, hz=0.05)
    env.add_joint_revolute(-1, b, axis=[0.0, 1.0, 0.0])
    model = env.finalize()
    with pytest.raises(NotImplementedError, match="needs articulations"):
        nt.eval_forward_dynamics(model, model.state())


def test_python_argument_errors():
    c = fd_case("multi_art", 4, 2)
    s = c.state()
    with pytest.raises(ValueError, match="joint_qdd must be a float32 numpy array of shape"):
        nt.eval_forward_dynamics(c.model, s, joint_qdd=np.zeros((12, 5), np.float32))
    with pytest.raises(ValueError, match="joint_qdd must be a float32 numpy array of shape"):
        nt.eval_forward_dynamics(c.model, s, joint_qdd=np.zeros((12, 6), np.float64))
    with pytest.raises(ValueError, match="joint_f must have shape"):
        nt.eval_forward_dynamics(c.model, s, np.zeros(c.model.joint_dof_count, np.float32))
    with pytest.raises(ValueError, match="info must be an int32 numpy array of shape"):
        nt.eval_forward_dynamics(c.model, s, info=np.zeros(12, np.int64))
    with pytest.raises(ValueError, match="info must be an int32 numpy array of shape"):
        nt.eval_forward_dynamics(c.model, s, info=np.zeros(11, np.int32))


@pytest.mark.parametrize("name", ["multi_art", "quadruped"])
def test_massless_leaf_is_reported_and_stays_in_its_articulation(name):
    c = fd_case(name, 7, 3)
    model, bad = massless_leaf_model(name, 7)
    s, s_bad = c.state(), c.state()
    good_info, info = np.full(bad.size, -1, np.int32), np.full(bad.size, -1, np.int32)
    good = nt.eval_forward_dynamics(c.model, s, c.joint_f, body_f=True, info=good_info)
    got = eval_forward_dynamics_numpy(model, s_bad.body_q, s_bad.joint_q, s_bad.joint_qd, c.joint_f, c.body_f, info=info)
    assert bad.any() and np.all(good_info == 0)
    for a in np.flatnonzero(bad):
        assert np.all(np.isnan(got[a, :c.nda[a]])) and np.all(got[a, c.nda[a]:] == 0.0) and 0 < info[a] <= c.nda[a]
    assert np.array_equal(got[~bad], good[~bad]) and np.all(info[~bad] == 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the C ABI: header vs ctypes table, argument errors
# ---------------------------------------------------------------------------------------------------------------------------------
def _declaration(name):
    text = open(HEADER).read()
    m = re.search(r"nt_status\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/newton_hip_kinematics.h"
    return [" ".join(re.sub(r"/\*.*?\*/", "", a).split()) for a in m.group(1).split(",")]


def test_header_and_ctypes_table_agree():
    name = "nt_eval_forward_dynamics"
    args = _declaration(name)
    assert args == ["const nt_model* m", "const nt_state* in", "const float* joint_f", "int32_t flags", "float* joint_qdd", "int32_t* info",
                    "const uint8_t* art_mask", "void* stream"]
    restype, argtypes = _lib.SYMBOLS[name]
    assert restype is C.c_int32
    assert argtypes == [C.POINTER(_lib.nt_model), C.POINTER(_lib.nt_state), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                        C.c_void_p]
    assert _declaration(name + "_tile") == args[:7] + ["int32_t envs_per_block", "void* stream"]
    assert _lib.SYMBOLS[name + "_tile"] == (C.c_int32, argtypes[:7] + [C.c_int32, C.c_void_p])
    text = open(HEADER).read()
    assert re.search(r"^ \*\s+" + name + r"\s", text, re.M)  # the entry-point line of the contract
    flags = dict(re.findall(r"^#define (NT_FD_\w+)\s+(\d+)", text, re.M))
    assert flags == {"NT_FD_GRAVITY": "1", "NT_FD_VELOCITY": "2", "NT_FD_BODY_F": "4"}
    assert (nt.articulation.NT_FD_GRAVITY, nt.articulation.NT_FD_VELOCITY, nt.articulation.NT_FD_BODY_F) == (1, 2, 4)
    import __graft_entry__ as g

    assert not any("newton_hip_kinematics.h" in d for d in g.UNITS["nt_kernels.hip"])  # the headline unit keeps its id


def test_abi_argument_errors():
    """Null pointers, unknown flag bits and NT_FD_BODY_F without body_f NT_ERR_INVALID_ARG (-1); no joints / no articulations
    NT_ERR_UNSUPPORTED (-3): decided before any launch, so the compiled library answers without a device."""
    lib = _lib.load()
    fn, tile = lib.nt_eval_forward_dynamics, lib.nt_eval_forward_dynamics_tile
    m, s = _lib.nt_model(), _lib.nt_state()
    m.env_count, m.env_stride, m.nb, m.nj, m.cpp, m.na, m.max_art_dofs = 4, 64, 2, 1, 4, 1, 1
    buf = (C.c_float * 16)()
    ptr = C.cast(buf, C.c_void_p)
    m.art_start = ptr
    s.body_q, s.joint_q, s.joint_qd = ptr, ptr, ptr
    ok = (C.byref(m), C.byref(s), None, 3, ptr, None, None, None)
    assert fn(None, *ok[1:]) == -1
    assert fn(ok[0], None, *ok[2:]) == -1
    assert fn(ok[0], ok[1], None, 3, None, None, None, None) == -1
    for bad in (8, 15, -1):
        assert fn(ok[0], ok[1], None, bad, ptr, None, None, None) == -1
    assert fn(ok[0], ok[1], None, 7, ptr, None, None, None) == -1  # NT_FD_BODY_F with a null body_f
    for missing in ("body_q", "joint_q", "joint_qd"):
        s2 = _lib.nt_state()
        s2.body_q, s2.joint_q, s2.joint_qd = ptr, ptr, ptr
        setattr(s2, missing, None)
        assert fn(ok[0], C.byref(s2), *ok[2:]) == -1
    m.nj = 0
    assert fn(*ok) == -3 and tile(*ok[:7], 0, None) == -3
    m.nj, m.na = 1, 0
    assert fn(*ok) == -3 and tile(*ok[:7], 16, None) == -3


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. consistency with the Featherstone solver (CPU oracle): (qd1 - qd0) / dt of one step is the joint acceleration
# ---------------------------------------------------------------------------------------------------------------------------------
FS_DT = 1e-3
FS_BOUND = 1e-3  # the bound of the bias-compensation test on the same scenes; the rounding of qd1 alone explains 2^-24 max|qd| / dt ~ 1.5e-4


def featherstone_ratio(qd0, qd1, qdd):
    """max |(qd1 - qd0) / dt - qdd| / max(1, max|qdd|) over the flat dofs."""
    acc = (np.asarray(qd1, dtype=np.float64) - qd0) / FS_DT
    want = np.asarray(qdd, dtype=np.float64).reshape(-1)
    return float(np.abs(acc - want).max() / max(1.0, np.abs(want).max()))


@pytest.mark.parametrize("kind", ["pendulum3", "rpr"])
def test_oracle_featherstone_step_moves_joint_qd_by_qdd_dt(oracle_lib, kind):
    """Fixed-base chains of 1-dof joints, where the solver's convention and the public one coincide; limits, drives, damping, friction
    and armature zero; 5 worlds, one step of 1 ms, random control.joint_f."""
    from oracle_bridge import Oracle, OracleState

    model = compensation_scene(kind, 5)
    assert model.max_dofs_per_articulation == 3 and model.env.na == 1
    q, qd = compensation_state(model, 7)
    joint_f = np.random.default_rng(11).uniform(-10.0, 10.0, size=(5, 3)).astype(np.float32)
    bq, bqd = eval_fk_numpy(model, q, qd)
    qdd = nt.eval_forward_dynamics(model, _host_state(model, bq, bqd, q, qd), joint_f)
    o = Oracle(model)
    s_in, s_out = OracleState(model, bq, bqd), OracleState(model, bq, bqd)
    s_in.joint_q[:], s_in.joint_qd[:] = q, qd
    o.featherstone_step(s_in, s_out, o.control(joint_f=joint_f.reshape(-1)), None, FS_DT, angular_damping=0.0)
    ratio = featherstone_ratio(qd, s_out.joint_qd, qdd)
    print(f"[eval_forward_dynamics] {kind}: max |(qd1 - qd0) / dt - qdd| / max(1, max|qdd|) over one oracle Featherstone step {ratio:.3e} "
          f"(max|qdd| {np.abs(qdd).max():.1f})")
    assert np.abs(qdd).max() > 1.0 and ratio <= FS_BOUND
