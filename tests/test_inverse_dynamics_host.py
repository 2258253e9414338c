"""newton_amd.eval_inverse_dynamics on the host: the float64 finite-difference reference of tests/inverse_dynamics_reference.py checks
itself (halving its step), the numpy path against it on every scene, the Lagrangian equations of the n-link planar pendulum written
out, the identities with eval_mass_matrix and eval_jacobian, padding, selection, the C header against the ctypes table, and the bias
forces fed back through the CPU oracle's Featherstone step.

The cases and the gate below are shared with tests/test_inverse_dynamics_emu.py and tests/test_gpu_inverse_dynamics.py.
Error measure everywhere: |tau - tau_ref| / max(1, max|tau_ref| of the articulation).
  numpy path     1e-6: both sides are float64 (the result is rounded to fp32 once, 6e-8), the finite difference costs ~1e-8
  fp32 kernel    ID_GATE = 4 x the largest per-scene maximum measured on the emulator (37 worlds, seed 21), the margin the ray-cast gates
                 use for fp32 evaluation-order differences.  Measured maxima, emulator (every tile the same bits):
                   d6_zoo 1.325e-06   free_child 4.797e-07   free_child_free_root 2.835e-07   joint_zoo 9.846e-07
                   joint_zoo_free_root 2.377e-07   multi_art 4.217e-07   pendulum 4.711e-07   quadruped 2.829e-07
                 (J and H sit at 2e-7 .. 1.3e-6 on this scale.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import newton_amd as nt
from inverse_dynamics_reference import art_dof_ranges, id_error, inverse_dynamics_reference, random_rates
from newton_amd import _lib
from newton_amd import _np_math as nm
from newton_amd.articulation import (_eval_fk_float64, eval_fk_numpy, eval_inverse_dynamics_numpy, eval_jacobian_numpy,
                                     eval_mass_matrix_numpy)
from test_eval_ik_host import random_joint_state
from test_eval_jacobian_host import POISON, SCENES, _host_state, planar_pendulum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "newton_hip_kinematics.h")
HOST_GATE = 1e-6
ID_GATE = 4 * 1.325e-06  # (see above: d6_zoo)
EPS = 2.0 ** -24  # one fp32 rounding, relative


class IdCase:
    """A scene, random joint coordinates, qd ~ U(-2, 2), qdd ~ U(-5, 5) (public layout) and eval_fk's fp32 body state for them."""

    def __init__(self, name, E, seed, device=None):
        self.model = SCENES[name](E, device=device) if device else SCENES[name](E)
        self.jq, _ = random_joint_state(self.model, seed)
        self.D = int(self.model.max_dofs_per_articulation)
        self.qd, self.qdd = random_rates(self.model, seed + 100, self.D)
        self.bq, self.bqd = eval_fk_numpy(self.model, self.jq, self.qd)
        self.bq64 = _eval_fk_float64(self.model, self.jq, self.qd)[0].reshape(-1, 7)  # the same poses before the rounding to fp32
        self.dof_ranges = art_dof_ranges(self.model)
        self._refs = {}

    def ref(self, qdd=True, gravity=True, velocity_terms=True, f64=False):
        """The reference on the fp32 body_q the kernels are given, or (f64) on the unrounded poses the host path can be given."""
        key = (qdd, gravity, velocity_terms, f64)
        if key not in self._refs:
            self._refs[key] = inverse_dynamics_reference(self.model, self.bq64 if f64 else self.bq, self.jq, self.qd,
                                                         self.qdd if qdd else None, gravity, velocity_terms)
        return self._refs[key]

    def state(self, f64=False):
        return _host_state(self.model, self.bq64 if f64 else self.bq, self.bqd, self.jq, self.qd)


_CASES = {}


def id_case(name, E, seed, device=None):
    key = (name, E, seed, device)
    if key not in _CASES:
        _CASES[key] = IdCase(name, E, seed, device)
    return _CASES[key]


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the reference checks itself; the numpy path against it
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENES))
def test_reference_is_converged_in_its_step(name):
    c = id_case(name, 5, 5)
    half = inverse_dynamics_reference(c.model, c.bq64, c.jq, c.qd, c.qdd, h=0.5e-4)
    err = id_error(half, c.ref(f64=True))
    print(f"[eval_inverse_dynamics reference] {name}: h = 1e-4 against h = 5e-5, change / scale {err:.3e}")
    assert err < 1e-7


@pytest.mark.parametrize("name", sorted(SCENES))
def test_numpy_path_matches_reference(name):
    """Both sides in float64 on the same unrounded poses: what differs is the finite difference (~1e-8) and the one rounding of the
    result to fp32 (6e-8)."""
    c = id_case(name, 5, 5)
    s = c.state(f64=True)
    tau = nt.eval_inverse_dynamics(c.model, s, c.qdd)
    assert tau.dtype == np.float32 and tau.shape == (c.model.articulation_count, c.D)
    ref = c.ref(f64=True)
    err = id_error(tau, ref)
    print(f"[eval_inverse_dynamics numpy] {name}: max |tau - tau_ref| / max(1, max|tau_ref|) {err:.3e}, max|tau_ref| {np.abs(ref).max():.1f}")
    assert err <= HOST_GATE, (name, err)
    for kw in (dict(), dict(velocity_terms=False), dict(gravity=False)):  # the bias forces and their two parts
        h = nt.eval_inverse_dynamics(c.model, s, **kw)
        assert id_error(h, c.ref(qdd=False, f64=True, **kw)) <= HOST_GATE, (name, kw)
    assert all(np.all(tau[a, hi - lo:] == 0.0) for a, (lo, hi) in enumerate(c.dof_ranges))


def pendulum_lagrange(model, q, qd, qdd, gz):
    """The Lagrangian equations of the n-link planar pendulum of planar_pendulum(n): links along u(phi) = (cos phi, 0, -sin phi) with the
    absolute angles phi_k = q_0 + .. + q_k (revolute about +y), COM l_c = 0.3 from the joint, the next joint l = 0.5 along, gravity
    (0, 0, gz).  With a_ki = l (i < k), l_c (i = k), 0 (i > k) the COM of link k is sum_i a_ki u(phi_i), and u'(phi_i) . u'(phi_j) =
    cos(phi_i - phi_j):
      T = 1/2 sum_ij c_ij cos(phi_i - phi_j) phi'_i phi'_j + 1/2 sum_i I_i phi'_i^2,   c_ij = sum_k m_k a_ki a_kj
      V = -sum_k m_k gz z_k,   z_k = z_0 - sum_i a_ki sin(phi_i)
      Q_i = sum_j (c_ij cos(phi_i - phi_j) + delta_ij I_i) phi''_j + sum_j c_ij sin(phi_i - phi_j) phi'_j^2 + gz cos(phi_i) sum_k m_k a_ki
    (inertial, centrifugal / Coriolis, gravity); the joint torques are tau_j = sum_{i >= j} Q_i because phi_i = sum_{j <= i} q_j."""
    n = len(q)
    m = np.asarray(model.body_mass, dtype=np.float64)[:n]
    Iyy = np.asarray(model.body_inertia, dtype=np.float64).reshape(-1, 3, 3)[:n, 1, 1]
    lc, l = 0.3, 0.5
    a = np.array([[l if i < k else (lc if i == k else 0.0) for i in range(n)] for k in range(n)])
    c = np.einsum("k,ki,kj->ij", m, a, a)
    Lm = np.tril(np.ones((n, n)))
    phi, dphi, ddphi = Lm @ q, Lm @ qd, Lm @ qdd
    diff = phi[:, None] - phi[None, :]
    Q = (c * np.cos(diff) + np.diag(Iyy)) @ ddphi + (c * np.sin(diff)) @ dphi ** 2 + gz * np.cos(phi) * (m @ a)
    return Lm.T @ Q


@pytest.mark.parametrize("links", [1, 2, 3])
def test_planar_pendulum_closed_forms(links):
    model = planar_pendulum(links)
    assert np.allclose(np.asarray(model.body_com), 0.0)
    g = np.asarray(model.gravity, dtype=np.float64).reshape(-1, 3)[0]
    assert g[0] == 0.0 and g[1] == 0.0 and g[2] < 0.0
    q = np.array([0.7, -1.1, 0.4][:links], np.float32)
    qd = np.array([1.3, -0.8, 1.9][:links], np.float32)
    qdd = np.array([[-2.0, 3.5, 1.2][:links]], np.float32)
    bq64, _ = _eval_fk_float64(model, q, qd)  # unrounded poses: what is left is the one fp32 rounding of the result
    for kw, use in ((dict(), (1, 1, 1)), (dict(velocity_terms=False), (1, 0, 1)), (dict(gravity=False), (1, 1, 0))):
        tau = eval_inverse_dynamics_numpy(model, bq64.reshape(-1, 7), q, qd, qdd, **kw)
        want = pendulum_lagrange(model, q.astype(np.float64), qd.astype(np.float64) * use[1], qdd[0].astype(np.float64), g[2] * use[2])
        assert np.abs(tau[0] - want).max() <= HOST_GATE * max(1.0, np.abs(want).max()), (links, kw, tau, want)
    # each term is live in the check above
    parts = [pendulum_lagrange(model, q.astype(np.float64), qd * s[0], qdd[0] * s[1], g[2] * s[2]) for s in ((1, 0, 0), (0, 1, 0), (0, 0, 1))]
    assert np.abs(parts[1]).max() > 0.1 and np.abs(parts[2]).max() > 0.1 and (links == 1 or np.abs(parts[0]).max() > 0.01)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_torque_difference_is_the_mass_matrix_times_the_acceleration(name):
    c = id_case(name, 5, 5)
    s = c.state()
    t1, t0 = nt.eval_inverse_dynamics(c.model, s, c.qdd), nt.eval_inverse_dynamics(c.model, s)
    H = eval_mass_matrix_numpy(c.model, c.bq, c.jq).astype(np.float64)
    want = np.einsum("aij,aj->ai", H, c.qdd.astype(np.float64))
    # three fp32 arrays enter, each rounded once: tau(qdd), tau(0) and the entries of H (times |qdd|); twice that is allowed
    bound = 2.0 * EPS * (np.abs(t1) + np.abs(t0) + np.einsum("aij,aj->ai", np.abs(H), np.abs(c.qdd.astype(np.float64))))
    assert np.all(np.abs((t1.astype(np.float64) - t0) - want) <= bound + 1e-12)
    assert np.abs(want).max() > 1.0


@pytest.mark.parametrize("name", sorted(SCENES))
def test_gravity_term_from_the_com_jacobian(name):
    """velocity_terms=False, no qdd: tau = -sum_l m_l (J_l's linear rows carried to the COM)^T g."""
    c = id_case(name, 5, 5)
    model, t = c.model, c.model.env
    tau = nt.eval_inverse_dynamics(model, c.state(), velocity_terms=False)
    J = eval_jacobian_numpy(model, c.bq, c.jq).astype(np.float64)
    bq, com = c.bq.astype(np.float64), np.asarray(model.body_com, dtype=np.float64).reshape(-1, 3)
    mass = np.asarray(model.body_mass, dtype=np.float64).reshape(-1)
    g_all, world = np.asarray(model.gravity, dtype=np.float64).reshape(-1, 3), np.asarray(model.articulation_world)
    from newton_amd.articulation import _qrot

    cw = bq[:, :3] + _qrot(bq[:, 3:], com)
    want, bound = np.zeros_like(J[:, 0]), np.zeros_like(J[:, 0])
    for a, (j0, j1) in enumerate(zip(model.articulation_start, model.articulation_end)):
        g = g_all[int(world[a])]
        for i, j in enumerate(range(int(j0), int(j1))):
            b = int(model.joint_child[j])
            cx = np.array([[0, -cw[b, 2], cw[b, 1]], [cw[b, 2], 0, -cw[b, 0]], [-cw[b, 1], cw[b, 0], 0]])
            Jl = J[a, 6 * i:6 * i + 6]
            want[a] -= mass[b] * (Jl[:3] - cx @ Jl[3:]).T @ g
            bound[a] += mass[b] * (np.abs(Jl[:3]) + np.abs(cx) @ np.abs(Jl[3:])).T @ np.abs(g)
    # J is fp32: every entry rounded once (bound: the same sum over magnitudes), tau rounded once; twice that is allowed
    assert np.all(np.abs(tau - want) <= 2.0 * EPS * (bound + np.abs(want)) + 1e-12), np.abs(tau - want).max()
    assert t.na > 0 and np.abs(want).max() > 1.0


def test_both_flags_off_and_no_acceleration_is_exactly_zero():
    c = id_case("joint_zoo_free_root", 5, 5)
    tau = nt.eval_inverse_dynamics(c.model, c.state(), tau=np.full((c.model.articulation_count, c.D), POISON, np.float32), gravity=False,
                                   velocity_terms=False)
    assert np.all(tau == 0.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. padding, selection, heterogeneous models, refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_output_into_caller_array_and_poisoned_padding():
    c = id_case("multi_art", 4, 2)
    s = c.state()
    tau = nt.eval_inverse_dynamics(c.model, s, c.qdd)
    tau2 = np.full_like(tau, POISON)
    assert nt.eval_inverse_dynamics(c.model, s, c.qdd, tau2) is tau2
    assert np.array_equal(tau2, tau)  # the padding is written (zero) on every call
    assert c.model.env.na == 3 and tau.shape == (12, 6) and np.all(tau[2, 2:] == 0.0) and np.all(tau[2, :2] != 0.0)
    # what the padding of joint_qdd holds does not matter
    qdd = c.qdd.copy()
    qdd[2::3, 2:] = POISON
    assert np.array_equal(nt.eval_inverse_dynamics(c.model, s, qdd), tau)


def test_mask_leaves_unselected_slices_untouched_bit_for_bit():
    c = id_case("multi_art", 6, 4)
    s = c.state()
    tau = nt.eval_inverse_dynamics(c.model, s, c.qdd)
    sel = np.random.default_rng(3).random(c.model.articulation_count) < 0.5
    assert sel.any() and not sel.all()
    part = np.full_like(tau, POISON)
    nt.eval_inverse_dynamics(c.model, s, c.qdd, part, mask=sel)
    assert np.array_equal(part[sel], tau[sel]) and np.all(part[~sel] == POISON)
    with pytest.raises(ValueError, match="mask has 3 entries"):
        nt.eval_inverse_dynamics(c.model, s, mask=[True, False, True])


def test_articulation_view_world_mask():
    c = id_case("multi_art", 4, 8)
    s = c.state()
    view = nt.selection.ArticulationView(c.model, str(list(c.model.articulation_label)[2]))  # the pendulum: third articulation of every world
    tau = nt.eval_inverse_dynamics(c.model, s, c.qdd, gravity=False)
    got = view.eval_inverse_dynamics(s, c.qdd, gravity=False)
    assert got.shape == (4, 6) and np.array_equal(got, tau.reshape(4, 3, 6)[:, 2])
    buf = np.full_like(tau, POISON)
    got = view.eval_inverse_dynamics(s, c.qdd, buf, mask=[True, False, True, False], gravity=False)
    assert np.array_equal(got[[0, 2]], tau.reshape(4, 3, 6)[[0, 2], 2]) and np.all(got[[1, 3]] == POISON)
    assert np.all(buf.reshape(4, 3, 6)[[1, 3]] == POISON)  # every articulation of an unselected world
    with pytest.raises(ValueError, match="one entry per world"):
        view.eval_inverse_dynamics(s, mask=[True, False])


def test_heterogeneous_model():
    from test_heterogeneous_worlds import mixed_model

    model = mixed_model((("quadruped", 2), ("boxes3", 1), ("pendulum", 2), ("quadruped", 1)))
    assert model.is_heterogeneous
    parts = model.world_groups.parts
    states = [random_joint_state(p, 2 + i) for i, p in enumerate(parts)]
    jq = np.concatenate([a for a, _ in states])
    D = int(model.max_dofs_per_articulation)
    qd, qdd = random_rates(model, 9, D)
    bq, bqd = eval_fk_numpy(model, jq, qd)
    s = model.state()
    s.body_q, s.body_qd, s.joint_q, s.joint_qd = bq, bqd, jq, qd
    tau = nt.eval_inverse_dynamics(model, s, qdd)
    assert tau.shape == (model.articulation_count, D) and D == 18
    # the reference group by group (its finite difference needs one replicated model), into the global padding
    want = np.zeros((model.articulation_count, D))
    b0 = c0 = d0 = a0 = 0
    for p in parts:
        b1, c1, d1, a1 = b0 + p.body_count, c0 + p.joint_coord_count, d0 + p.joint_dof_count, a0 + p.articulation_count
        if p.articulation_count:
            Dp = int(p.max_dofs_per_articulation)
            want[a0:a1, :Dp] = inverse_dynamics_reference(p, bq[b0:b1], jq[c0:c1], qd[d0:d1], qdd[a0:a1, :Dp])
        b0, c0, d0, a0 = b1, c1, d1, a1
    err = id_error(tau, want)
    print(f"[eval_inverse_dynamics numpy] heterogeneous: {err:.3e}")
    assert err <= HOST_GATE
    assert np.array_equal(tau, eval_inverse_dynamics_numpy(model, bq, jq, qd, qdd))
    sel = np.arange(model.articulation_count) % 2 == 0
    part = np.full_like(tau, POISON)
    nt.eval_inverse_dynamics(model, s, qdd, part, mask=sel)
    assert np.array_equal(part[sel], tau[sel]) and np.all(part[~sel] == POISON)


def test_model_without_articulations_is_refused():
    env = nt.ModelBuilder()
    b = env.add_link(xform=[0.0, 0.0, 1.0, 0, 0, 0, 1])
    env.add_shape_box(b, hx=0.1, hy=0.05, hz=0.05)
    env.add_joint_revolute(-1, b, axis=[0.0, 1.0, 0.0])
    model = env.finalize()
    with pytest.raises(NotImplementedError, match="needs articulations"):
        nt.eval_inverse_dynamics(model, model.state())


def test_python_argument_errors():
    c = id_case("multi_art", 4, 2)
    s = c.state()
    with pytest.raises(ValueError, match="tau must be a float32 numpy array of shape"):
        nt.eval_inverse_dynamics(c.model, s, tau=np.zeros((12, 5), np.float32))
    with pytest.raises(ValueError, match="tau must be a float32 numpy array of shape"):
        nt.eval_inverse_dynamics(c.model, s, tau=np.zeros((12, 6), np.float64))
    with pytest.raises(ValueError, match="joint_qdd must have shape"):
        nt.eval_inverse_dynamics(c.model, s, np.zeros(c.model.joint_dof_count, np.float32))


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the C ABI: header vs ctypes table, argument errors
# ---------------------------------------------------------------------------------------------------------------------------------
def _declaration(name):
    text = open(HEADER).read()
    m = re.search(r"nt_status\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/newton_hip_kinematics.h"
    return [" ".join(re.sub(r"/\*.*?\*/", "", a).split()) for a in m.group(1).split(",")]


def test_header_and_ctypes_table_agree():
    name = "nt_eval_inverse_dynamics"
    args = _declaration(name)
    assert args == ["const nt_model* m", "const nt_state* in", "const float* joint_qdd", "int32_t flags", "float* tau",
                    "const uint8_t* art_mask", "void* stream"]
    restype, argtypes = _lib.SYMBOLS[name]
    assert restype is C.c_int32
    assert argtypes == [C.POINTER(_lib.nt_model), C.POINTER(_lib.nt_state), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    assert _declaration(name + "_tile") == args[:6] + ["int32_t envs_per_block", "void* stream"]
    assert _lib.SYMBOLS[name + "_tile"] == (C.c_int32, argtypes[:6] + [C.c_int32, C.c_void_p])
    text = open(HEADER).read()
    assert re.search(r"^ \*\s+" + name + r"\s", text, re.M)  # the entry-point line of the contract
    flags = dict(re.findall(r"^#define (NT_ID_\w+)\s+(\d+)", text, re.M))
    assert flags == {"NT_ID_GRAVITY": "1", "NT_ID_VELOCITY": "2"}
    assert (nt.articulation.NT_ID_GRAVITY, nt.articulation.NT_ID_VELOCITY) == (1, 2)
    import __graft_entry__ as g

    assert not any("newton_hip_kinematics.h" in d for d in g.UNITS["nt_kernels.hip"])  # the headline unit keeps its id


def test_abi_argument_errors():
    """Null pointers and unknown flag bits NT_ERR_INVALID_ARG (-1); no joints / no articulations NT_ERR_UNSUPPORTED (-3): decided before
    any launch, so the compiled library answers without a device."""
    lib = _lib.load()
    fn, tile = lib.nt_eval_inverse_dynamics, lib.nt_eval_inverse_dynamics_tile
    m, s = _lib.nt_model(), _lib.nt_state()
    m.env_count, m.env_stride, m.nb, m.nj, m.cpp, m.na, m.max_art_dofs = 4, 64, 2, 1, 4, 1, 1
    buf = (C.c_float * 16)()
    ptr = C.cast(buf, C.c_void_p)
    m.art_start = ptr
    s.body_q, s.joint_q, s.joint_qd = ptr, ptr, ptr
    ok = (C.byref(m), C.byref(s), None, 3, ptr, None, None)
    assert fn(None, *ok[1:]) == -1
    assert fn(ok[0], None, *ok[2:]) == -1
    assert fn(ok[0], ok[1], None, 3, None, None, None) == -1
    for bad in (4, 7, -1):
        assert fn(ok[0], ok[1], None, bad, ptr, None, None) == -1
    for missing in ("body_q", "joint_q", "joint_qd"):
        s2 = _lib.nt_state()
        s2.body_q, s2.joint_q, s2.joint_qd = ptr, ptr, ptr
        setattr(s2, missing, None)
        assert fn(ok[0], C.byref(s2), *ok[2:]) == -1
    m.nj = 0
    assert fn(*ok) == -3 and tile(*ok[:6], 0, None) == -3
    m.nj, m.na = 1, 0
    assert fn(*ok) == -3 and tile(*ok[:6], 16, None) == -3


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the bias forces through the Featherstone solver (CPU oracle): control.joint_f = h(q, qd) cancels gravity and velocity terms
# ---------------------------------------------------------------------------------------------------------------------------------
def compensation_scene(kind, worlds, device=None):
    """A fixed-base chain of 1-dof joints -- the case where the solver's convention and the public one coincide -- with limits, drives,
    damping, friction and armature zero: "pendulum3", the geometry of planar_pendulum(3), or "rpr", a revolute - prismatic - revolute arm
    with skew axes and offset COMs."""
    env = nt.ModelBuilder()
    cfg = nt.ModelBuilder.ShapeConfig(has_shape_collision=False)
    zero = dict(limit_ke=0.0, limit_kd=0.0, target_ke=0.0, target_kd=0.0, damping=0.0, friction=0.0, armature=0.0)
    joints, prev = [], -1
    if kind == "pendulum3":
        for k in range(3):
            b = env.add_link(xform=[0.3 + 0.5 * k, 0.0, 2.0, 0, 0, 0, 1])
            env.add_shape_box(b, hx=0.3, hy=0.04, hz=0.05 + 0.01 * k, cfg=cfg)
            joints.append(env.add_joint_revolute(prev, b, axis=[0.0, 1.0, 0.0], child_xform=nm.transform([-0.3, 0.0, 0.0]),
                                                 parent_xform=nm.transform([0.0, 0.0, 2.0] if k == 0 else [0.2, 0.0, 0.0]), **zero))
            prev = b
    else:
        assert kind == "rpr"
        a, b, c = (env.add_link(xform=[0.3 * k, 0.0, 1.5, 0, 0, 0, 1]) for k in range(3))
        for k, link in enumerate((a, b, c)):
            env.add_shape_box(link, xform=nm.transform([0.03, -0.02 * k, 0.01]), hx=0.2, hy=0.05 + 0.01 * k, hz=0.04, cfg=cfg)
        joints.append(env.add_joint_revolute(-1, a, axis=[0.0, 0.6, 0.8], parent_xform=nm.transform([0.0, 0.0, 1.5], nm.quat_rpy(0.2, 0.0, 0.1)),
                                             child_xform=nm.transform([-0.2, 0.0, 0.0]), **zero))
        joints.append(env.add_joint_prismatic(a, b, axis=[1.0, 0.0, 0.0], parent_xform=nm.transform([0.1, 0.02, 0.0], nm.quat_rpy(0.0, 0.3, 0.0)),
                                              child_xform=nm.transform([-0.2, 0.0, 0.01]), **zero))
        joints.append(env.add_joint_revolute(b, c, axis=[0.8, 0.0, 0.6], parent_xform=nm.transform([0.2, 0.0, 0.0]),
                                             child_xform=nm.transform([-0.2, 0.01, 0.0], nm.quat_rpy(0.1, 0.0, 0.0)), **zero))
    env.add_articulation(joints)
    scene = nt.ModelBuilder()
    scene.replicate(env, worlds)
    return scene.finalize(device=device)


def compensation_state(model, seed):
    """Random q in (-1, 1), qd in (-2, 2) per dof (float32)."""
    rng = np.random.default_rng(seed)
    n = model.joint_dof_count
    return rng.uniform(-1.0, 1.0, n).astype(np.float32), rng.uniform(-2.0, 2.0, n).astype(np.float32)


@pytest.mark.parametrize("kind", ["pendulum3", "rpr"])
def test_bias_forces_cancel_in_the_oracle_featherstone_step(oracle_lib, kind):
    from oracle_bridge import Oracle, OracleState

    model = compensation_scene(kind, 5)
    assert model.max_dofs_per_articulation == 3 and model.env.na == 1
    q, qd = compensation_state(model, 7)
    bq, bqd = eval_fk_numpy(model, q, qd)
    h = nt.eval_inverse_dynamics(model, _host_state(model, bq, bqd, q, qd))  # [5, 3]: the dofs in order
    o = Oracle(model)
    moved = []
    for joint_f in (h.reshape(-1), np.zeros_like(qd)):
        s_in, s_out = OracleState(model, bq, bqd), OracleState(model, bq, bqd)
        s_in.joint_q[:], s_in.joint_qd[:] = q, qd
        o.featherstone_step(s_in, s_out, o.control(joint_f=joint_f), None, 1e-3, angular_damping=0.0)
        moved.append(np.abs(s_out.joint_qd.astype(np.float64) - qd).max())
    print(f"[eval_inverse_dynamics] {kind}: max|d qd| over one oracle Featherstone step with joint_f = h {moved[0]:.3e}, with joint_f = 0 "
          f"{moved[1]:.3e}, ratio {moved[0] / moved[1]:.3e}")
    assert moved[1] > 1e-3 and moved[0] <= 1e-3 * moved[1]
