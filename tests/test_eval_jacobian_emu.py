"""eval_jacobian_kernel / eval_mass_matrix_kernel (include/newton_hip_kinematics.h) on the emulator: the kernel SOURCES executed on the
CPU (tests/emu), without a GPU.  37 worlds (not a multiple of any tile), one environment per workgroup and the default tile, against
the float64 reference of tests/test_eval_jacobian_host.py on identical fp32 inputs, with that file's gates."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

from test_eval_jacobian_host import POISON, SCENES, fk_case, jm_errors, reference, structure_ok, within_gates  # noqa: E402

N_WORLDS = 37


@pytest.fixture(scope="module")
def H(oracle_lib):
    import harness

    harness.lib()  # builds tests/emu/_build/libnewton_emu.so on first use
    return harness


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Outputs:
    """Poison-filled outputs in the public layout."""

    def __init__(self, model):
        L, D = model.max_joints_per_articulation, model.max_dofs_per_articulation
        A = model.articulation_count
        self.J = np.full((A, 6 * L, D), POISON, np.float32)
        self.H = np.full((A, D, D), POISON, np.float32)
        self.S = np.full((model.joint_dof_count, 6), POISON, np.float32)
        self.I = np.full((model.body_count, 6, 6), POISON, np.float32)


def _run(H, em, state, out, epb=0, art_mask=None, tile_entry=True, aux=True):
    d = state.desc()
    mask = None if art_mask is None else np.ascontiguousarray(art_mask, dtype=np.uint8)
    lib, m = H.lib(), C.byref(em.desc)
    S, I = (_ptr(out.S), _ptr(out.I)) if aux else (None, None)  # noqa: E741
    if tile_entry:
        H.check(lib.nt_eval_jacobian_tile(m, C.byref(d), _ptr(out.J), S, _ptr(mask), epb, None), "nt_eval_jacobian_tile")
        H.check(lib.nt_eval_mass_matrix_tile(m, C.byref(d), _ptr(out.H), I, _ptr(mask), epb, None), "nt_eval_mass_matrix_tile")
    else:
        H.check(lib.nt_eval_jacobian(m, C.byref(d), _ptr(out.J), S, _ptr(mask), None), "nt_eval_jacobian")
        H.check(lib.nt_eval_mass_matrix(m, C.byref(d), _ptr(out.H), I, _ptr(mask), None), "nt_eval_mass_matrix")
    return out


def _state(H, em, bq, jq):
    return H.EmuState(em, body_q=bq, joint_q=jq)


@pytest.mark.parametrize("epb", [1, 0])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_kernels_match_reference(H, name, epb):
    model, jq, _jqd, bq, _bqd = fk_case(name, N_WORLDS, 21)
    em = H.EmuModel(model)
    s = _state(H, em, bq, jq)
    out = _run(H, em, s, Outputs(model), epb=epb)
    ref = reference(model, bq, jq)
    errs = jm_errors(model, ref, out.J, out.H, out.S, out.I)
    print(f"[eval_jacobian emu] {name} epb {epb}: error / gate scale {errs}")
    assert within_gates(errs), errs
    assert structure_ok(model, ref, out.J, out.H)  # poison gone from padding and non-ancestor entries: written as zero
    assert np.array_equal(s.aos("body_q"), bq) and np.array_equal(s.aos("joint_q"), jq)  # the state is only read
    # the entry points without a tile argument take the same tile as 0
    if epb == 0:
        out2 = _run(H, em, s, Outputs(model), tile_entry=False)
        assert all(np.array_equal(getattr(out, k), getattr(out2, k)) for k in "JHSI")


@pytest.mark.parametrize("epb", [1, 4, 8, 16])
@pytest.mark.parametrize("name", ["d6_zoo", "multi_art"])
def test_every_tile_width_gives_the_same_bits(H, name, epb):
    model, jq, _jqd, bq, _bqd = fk_case(name, N_WORLDS, 2)
    em = H.EmuModel(model)
    s = _state(H, em, bq, jq)
    a, b = _run(H, em, s, Outputs(model), epb=0), _run(H, em, s, Outputs(model), epb=epb)
    assert all(np.array_equal(getattr(a, k), getattr(b, k)) for k in "JHSI")
    d = s.desc()
    assert H.lib().nt_eval_jacobian_tile(C.byref(em.desc), C.byref(d), _ptr(b.J), None, None, 3, None) == -3  # not a compiled tile
    assert H.lib().nt_eval_mass_matrix_tile(C.byref(em.desc), C.byref(d), _ptr(b.H), None, None, 3, None) == -3


@pytest.mark.parametrize("epb", [1, 0])
def test_masked_launch_three_articulations_per_world(H, epb):
    """One byte per (world, articulation): the slices of unselected articulations keep their bits in all four outputs."""
    model, jq, _jqd, bq, _bqd = fk_case("multi_art", N_WORLDS, 6)
    em = H.EmuModel(model)
    assert model.env.na == 3
    sel = np.random.default_rng(0).random(N_WORLDS * 3) < 0.5
    s = _state(H, em, bq, jq)
    full, part = _run(H, em, s, Outputs(model), epb=epb), _run(H, em, s, Outputs(model), epb=epb, art_mask=sel)
    assert sel.any() and not sel.all()
    assert np.array_equal(part.J[sel], full.J[sel]) and np.all(part.J[~sel] == POISON)
    assert np.array_equal(part.H[sel], full.H[sel]) and np.all(part.H[~sel] == POISON)
    dsel = np.repeat(sel, np.tile([6, 6, 2], N_WORLDS))
    bsel = np.repeat(sel, np.tile([1, 1, 2], N_WORLDS))
    assert np.array_equal(part.S[dsel], full.S[dsel]) and np.all(part.S[~dsel] == POISON)
    assert np.array_equal(part.I[bsel], full.I[bsel]) and np.all(part.I[~bsel] == POISON)


def test_single_world_and_no_optional_outputs(H):
    model, jq, _jqd, bq, _bqd = fk_case("free_child_free_root", 1, 4)
    em = H.EmuModel(model)
    out = _run(H, em, _state(H, em, bq, jq), Outputs(model), aux=False)
    ref = reference(model, bq, jq)
    assert within_gates(jm_errors(model, ref, out.J, out.H)) and structure_ok(model, ref, out.J, out.H)
    assert np.all(out.S == POISON) and np.all(out.I == POISON)


def test_argument_errors(H):
    model, jq, _jqd, bq, _bqd = fk_case("pendulum", 3, 1)
    em = H.EmuModel(model)
    out = Outputs(model)
    d = _state(H, em, bq, jq).desc()
    lib = H.lib()
    for fn, buf in ((lib.nt_eval_jacobian, out.J), (lib.nt_eval_mass_matrix, out.H)):
        assert fn(None, C.byref(d), _ptr(buf), None, None, None) == -1
        assert fn(C.byref(em.desc), None, _ptr(buf), None, None, None) == -1
        assert fn(C.byref(em.desc), C.byref(d), None, None, None, None) == -1
        assert np.all(buf == POISON)
