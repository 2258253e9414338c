"""The analytic contact pairs (nt_primitives.hpp, behind primitive_pair) against exact float64 geometry, without a GPU: the kernel SOURCES
on the emulator (tests/emu), driven through nt_collide.  Reference, case tables, invariants and allowances: tests/primitive_exact.py;
the reference itself is checked against brute force by tests/test_primitive_exact_host.py; the device runs the same checks in
tests/test_gpu_primitive_exact.py.

Three kinds of test: every table against the exact answers and the generic invariants; the reference's 77 hand-computed known answers
(tests/golden/primitive_known_answers.json, so far run on the CPU oracle only) through the collide kernel; and, for the capsule,
sphere-box and sphere-cylinder tables, the contacts a 1-substep rollout of each solver leaves behind against collide's, bit for bit
(primitive_pair is instantiated again inside every fused kernel).

Allowance C * eps32 * L per case.  C comes from the host test (test_constants: the float32-vs-float64 error of the reference's own closed
forms on the tables, in eps32 * L, times 4, rounded up to a power of two), fixed before any kernel was looked at.  Measured worst kernel
error as a fraction of the allowance (distance | normal), over the size sets of each pair function; the MI355X column is printed by
tests/test_gpu_primitive_exact.py:

    pair function     reference error   C    emulator          MI355X           worlds per table   left out
    sphere_sphere          0.895         4   0.616 | 0.168     0.616 | 0.168    51, 51, 51         0
    plane_sphere           0.627         4   0.560 | 0.196     0.560 | 0.196    9, 9               0
    plane_capsule          2.516        16   0.271 | 0.049     0.271 | 0.049    36, 36, 36         0
    plane_box              2.102        16   0.347 | 0.049     0.347 | 0.049    80, 80, 80         0
    plane_ellipsoid        0.403         2   0.832 | 0.392     0.832 | 0.392    24, 24, 24         0
    plane_cylinder         1.257         8   0.282 | 0.098     0.282 | 0.098    222, 222, 222      0
    sphere_capsule         1.225         8   0.382 | 0.221     0.382 | 0.221    96, 96, 96         0
    sphere_cylinder        1.414         8   0.218 | 0.134     0.218 | 0.134    124, 124, 124      0
    sphere_box             1.414         8   0.196 | 0.135     0.196 | 0.135    222, 194, 222      0, 2 (1.0 %), 0
    capsule_capsule        3.135        16   0.210 | 0.146     0.210 | 0.146    236 x 4            0

Left out (closer to a branch switch than the allowance, held to the generic invariants only): two worlds of sphere_box/10to1, a centre
5e-7 outside a face of a box of size 1, whose allowance (9.5e-7) reaches the 1e-6 surface switch.  Every other table: none.

Explicit terms on top of C (derived from the contract formulas, primitive_exact.Answer): the 1e-6 regulariser of closest_segment_point
(sphere-capsule: up to 2.5e-5 for the capsule of half-height 0.02), the interior formula within 1e-6 outside a box face (2 delta), the
shared normal of the two contacts of parallel capsules, and the freedom of the closest pair along nearly parallel capsule axes (the
direction is compared up to sin(angle) * total length / distance; the contact is still held to both points on their segments at the exact
minimum distance).

Before capsule_capsule was rewritten all four capsule tables failed here, e.g. long_short: parallel_centred
reported 0.0693 for the exact 0.05 with a normal 21.8 degrees off; parallel_partial's second contact 0.5245 for 0.05; sweep_interior at
angle 0: second contact 0.1202 for 0.05; colinear / parallel_apart: 2 contacts, one on no capsule's axis, for the expected 1; and
plane_ellipsoid/tilted_10to1 missed its allowance by a factor 1.14 (2.28 eps32 L against C = 2).

Mutations of nt_primitives.hpp that make these tests fail (run by hand): the absolute `det >= 1e-15` test instead of the relative one
(capsule tables: one contact where two are expected), the sign of a sphere_box interior normal, the 0.5 of plane_sphere's contact position.
"""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import primitive_exact as PX  # noqa: E402
import world_isolation_cases as wi  # noqa: E402

KNOWN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "primitive_known_answers.json")))["tables"]
DT = {"xpbd": 2e-3, "semi_implicit": 1e-4, "featherstone": 1e-3}


@pytest.fixture(scope="module")
def H(oracle_lib):
    import harness

    harness.lib()  # builds tests/emu/_build/libnewton_emu.so on first use
    return harness


def emu_collide(H, model):
    em = H.EmuModel(model)
    s, ct = H.EmuState(em), H.EmuContacts(em)
    H.collide(em, s, ct)
    return ct.export()


@pytest.mark.parametrize("name", PX.TABLE_NAMES)
def test_table_against_exact_geometry(H, name):
    t = PX.table(name)
    model = t.model()
    flat = emu_collide(H, model)
    PX.report("emulator", t, PX.check_table(t, PX.decode(model, model.body_q, flat)))


@pytest.mark.parametrize("table_name", sorted(KNOWN))
def test_known_answers_through_the_kernel(H, table_name):
    """tests/golden/primitive_known_answers.json (the reference's hand-computed tables) with the assertions of
    tests/test_oracle_known_answers.py, on the collide kernel instead of the oracle."""
    for row in KNOWN[table_name]:
        model = PX.known_answer_scene(table_name, row)
        PX.check_known_answer(table_name, row, PX.decode(model, model.body_q, emu_collide(H, model))[0])


@pytest.mark.parametrize("solver", sorted(DT))
@pytest.mark.parametrize("name", PX.ROLLOUT_TABLES)
def test_rollout_contacts_equal_collide_bits(H, name, solver):
    """primitive_pair is instantiated again inside every fused rollout kernel: the contacts a 1-substep rollout leaves behind are
    collide's on the same state, bit for bit."""
    import ctypes as C

    from newton_amd import _lib as L

    model = PX.table(name).model()
    want = emu_collide(H, model)
    em = H.EmuModel(model)
    s0, s1, ctrl, ct = H.EmuState(em), H.EmuState(em), H.EmuControl(em), H.EmuContacts(em)
    if solver == "xpbd":
        H.xpbd_rollout(em, s0, s1, ctrl, ct, DT[solver], 1)
    elif solver == "featherstone":
        H.featherstone_rollout(em, s0, s1, ctrl, ct, DT[solver], 1)
    else:
        p, cp = L.nt_semi_implicit_params(0.05, 1.0, 1.0e4, 1.0e2), L.nt_collide_params(0, 0)
        d0, d1, dc, dct = s0.desc(), s1.desc(), ctrl.desc(), ct.desc()
        H.check(H.lib().nt_semi_implicit_rollout(C.byref(em.desc), C.byref(p), C.byref(cp), C.byref(d0), C.byref(d1), C.byref(dc),
                                                 C.byref(dct), float(DT[solver]), 1, None), "nt_semi_implicit_rollout")
    got = ct.export()
    n = int(want["count"][0])
    assert n > 0 and int(got["count"][0]) == n
    for k in wi.FLAT:
        assert np.array_equal(wi.bits(got[k][:n]), wi.bits(want[k][:n])), f"{name} {solver}: {k} differs from collide's"
