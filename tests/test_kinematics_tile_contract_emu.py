"""The tile argument of the four kinematics ``_tile`` entry points (nt_eval_ik_tile, nt_eval_jacobian_tile, nt_eval_mass_matrix_tile,
nt_ik_solve_tile; include/newton_hip_kinematics.h) is ONE contract -- kin_launch in nt_featherstone.hip -- stated here once, on the
emulator (the kernel SOURCES executed on the CPU, tests/emu), without a GPU: 0 takes the widest tile, 1 / 4 / 8 / 16 name a tile and
give the same bits, anything else is NT_ERR_UNSUPPORTED and writes nothing.  19 worlds: the last workgroup of every width above 1 is
partial.  Once on replicated worlds (nt_model.params_uniform: 0 takes the uniform-parameter tile) and once with one world's link
heavier (0 takes the widest per-environment-parameter tile)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

from ik_cases import ik_case, make_objectives  # noqa: E402
from ik_parity import device_problem  # noqa: E402
from newton_amd import ik  # noqa: E402
from newton_amd.articulation import eval_fk_numpy  # noqa: E402

N_WORLDS = 19
POISON = 7.0
NT_ERR_UNSUPPORTED = -3
ENTRIES = ["nt_eval_ik_tile", "nt_eval_jacobian_tile", "nt_eval_mass_matrix_tile", "nt_ik_solve_tile"]


@pytest.fixture(scope="module")
def H(oracle_lib):
    import harness

    harness.lib()  # builds tests/emu/_build/libnewton_emu.so on first use
    return harness


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Case:
    """multi_art (three articulations of different widths per world), a random pose per world; computed once per kind of model."""

    def __init__(self, H, uniform):
        model, _q_star, targets, start = ik_case("multi_art", N_WORLDS, 5)
        if not uniform:  # one link of world 3 is heavier: the worlds' parameter rows differ
            model.body_mass = np.array(model.body_mass, copy=True)
            model.body_mass[model.env.nb * 3 + 2] *= 1.25
            model.body_inv_mass = np.where(model.body_mass > 0, 1.0 / np.maximum(model.body_mass, 1e-30), 0.0).astype(np.float32)
        self.model, self.em = model, H.EmuModel(model)
        assert self.em.desc.params_uniform == int(uniform)
        self.solver = ik.IKSolver(model, make_objectives("multi_art", model, targets))
        self.prob = device_problem(self.solver)
        self.q = np.ascontiguousarray(start, dtype=np.float32).reshape(-1)
        qd = np.random.default_rng(11).normal(size=model.joint_dof_count).astype(np.float32)
        self.bq, self.bqd = eval_fk_numpy(model, self.q, qd)


_CASES = {}


def _case(H, uniform):
    if uniform not in _CASES:
        _CASES[uniform] = Case(H, uniform)
    return _CASES[uniform]


def _call(H, c, entry, epb):
    """One call of ``entry`` at tile ``epb`` into poison-filled outputs: (status, the outputs)."""
    model, m, lib = c.model, C.byref(c.em.desc), H.lib()
    if entry == "nt_ik_solve_tile":
        q_out, cost = np.full_like(c.q, POISON), np.full(N_WORLDS, POISON, np.float32)
        lam = c.solver.lambdas.astype(np.float32).copy()
        rc = lib.nt_ik_solve_tile(m, C.byref(c.prob.desc), _ptr(c.q), _ptr(q_out), _ptr(lam), _ptr(cost), 2, 1.0, epb, None)
        return rc, (q_out, cost), (lam, c.solver.lambdas.astype(np.float32))
    if entry == "nt_eval_ik_tile":
        s = H.EmuState(c.em, body_q=c.bq, body_qd=c.bqd, joint_q=np.full(model.joint_coord_count, POISON, np.float32),
                       joint_qd=np.full(model.joint_dof_count, POISON, np.float32))
        d = s.desc()
        rc = lib.nt_eval_ik_tile(m, C.byref(d), d.joint_q, d.joint_qd, None, epb, None)
        return rc, (s.aos("joint_q"), s.aos("joint_qd")), None
    L_, D = model.max_joints_per_articulation, model.max_dofs_per_articulation
    if entry == "nt_eval_jacobian_tile":
        out = np.full((model.articulation_count, 6 * L_, D), POISON, np.float32)
        aux = np.full((model.joint_dof_count, 6), POISON, np.float32)
    else:
        out = np.full((model.articulation_count, D, D), POISON, np.float32)
        aux = np.full((model.body_count, 6, 6), POISON, np.float32)
    s = H.EmuState(c.em, body_q=c.bq, joint_q=c.q)  # (owns the arrays the descriptor points to)
    d = s.desc()
    rc = getattr(lib, entry)(m, C.byref(d), _ptr(out), _ptr(aux), None, epb, None)
    return rc, (out, aux), None


def _bits(arrays):
    return [a.view(np.uint32) for a in arrays]


@pytest.mark.parametrize("uniform", [True, False], ids=["replicated", "one_world_differs"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_tile_argument_contract(H, entry, uniform):
    c = _case(H, uniform)
    rc, want, _ = _call(H, c, entry, 0)
    assert rc == 0
    assert all(not np.any(a == POISON) for a in want)  # the launch wrote every entry of its outputs
    for epb in (1, 4, 8, 16):
        rc, got, _ = _call(H, c, entry, epb)
        assert rc == 0, (entry, epb)
        assert all(np.array_equal(a, b) for a, b in zip(_bits(got), _bits(want))), (entry, epb)
    for epb in (-1, 2, 3, 5, 32):
        rc, got, inout = _call(H, c, entry, epb)
        assert rc == NT_ERR_UNSUPPORTED, (entry, epb)
        assert all(np.all(a == POISON) for a in got), (entry, epb)
        if inout is not None:  # (nt_ik_solve's damping is in / out: it keeps its input bits)
            assert np.array_equal(inout[0], inout[1])
