"""contact_sensor_kernel (nt_contact_sensor, include/newton_hip_contacts.h) on the emulator: the kernel SOURCE executed on the CPU
(tests/emu), without a GPU, on the synthetic sets of tests/contact_sensor_cases.py -- the exact set bit for bit against the float64
host reference, the order set against the float32 sequential sum in the contracted order.  1, 5 and 37 worlds (no multiple of the
worlds per workgroup; the emulated grid is four workgroups, so 37 worlds also take the grid-stride loop), 4 to 289 output cells per
world (16 / 8 / 4 / 2 / 1 worlds per workgroup, and more cells than a world has lanes), more entries than a round stages."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import contact_sensor_cases as cs  # noqa: E402


@pytest.fixture(scope="module")
def H(oracle_lib):
    import harness

    harness.lib()  # builds tests/emu/_build/libnewton_emu.so on first use
    return harness


_EM = {}


def _em(H, worlds):
    if worlds not in _EM:
        _EM[worlds] = H.EmuModel(cs.sensor_model(worlds))
    return _EM[worlds]


def _run(H, case, mask=None):
    call = cs.HostCall(case, _em(H, case.E).desc, mask=mask)
    before = [x.tobytes() for x in (case.shape0, case.shape1, case.impulse)]
    H.check(call.run(H.lib()), "nt_contact_sensor")
    assert before == [x.tobytes() for x in (case.shape0, case.shape1, case.impulse)]  # the inputs are only read
    return call.net_force


EXACT = cs.EXACT_CASES


@pytest.mark.parametrize("name", list(EXACT))
def test_exact_set_bit_for_bit(H, name):
    worlds, shape, nslot, rows = EXACT[name]
    case = cs.exact_case(cs.sensor_model(worlds), nslot, *cs.SHAPES[shape], rows=rows, seed=len(name))
    wpb, lanes, chunk = cs.launch_shape(case.S * case.cols)
    if "cells289" in name:
        assert lanes < case.S * case.cols and case.entries(0) > chunk
    if name == "37_worlds_cells4":
        assert nslot > lanes and nslot > chunk and worlds % wpb
    cs.check_exact(case, _run(H, case))


ORDER = cs.ORDER_CASES


@pytest.mark.parametrize("name", list(ORDER))
def test_order_set_is_the_float32_sequential_sum(H, name):
    worlds, shape, nslot, rows, designed_all = ORDER[name]
    case = cs.order_case(cs.sensor_model(worlds), nslot, *cs.SHAPES[shape], rows=rows, seed=len(name))
    if rows is not None:
        assert np.any(case.rshape0 >= 0)  # the contributions of a cell are spread over slots and rows
    cs.check_order(case, _run(H, case), designed_all)


def test_world_without_contacts_and_empty_row_ranges_write_zeros(H):
    case = cs.exact_case(cs.sensor_model(5), 40, *cs.SHAPES["cells20"], rows="ragged", seed=3)
    assert case.row_start[0] == case.row_start[1] and case.row_start[4] == case.row_start[5]  # empty ranges
    case.shape0[:, 4], case.shape1[:, 4] = -1, -1  # world 4: no contact at all
    got = _run(H, case)
    assert np.all(got[4] == 0.0) and np.any(got[3] != 0.0)
    cs.check_exact(case, got)


def test_masked_worlds_inside_a_live_workgroup(H):
    """Worlds 1, 4 and 30 off: each shares its workgroup with live worlds.  Masked rows keep the poison, live rows the bits of the
    unmasked run."""
    case = cs.exact_case(cs.sensor_model(37), 50, *cs.SHAPES["cells20"], rows="ragged", seed=4)
    assert cs.launch_shape(20)[0] == 8
    full = _run(H, case)
    mask = np.ones(37, bool)
    mask[[1, 4, 30]] = False
    got = _run(H, case, mask=mask)
    cs.check_exact(case, got, mask=mask)
    assert np.array_equal(cs.bits(got[mask]), cs.bits(full[mask]))


@pytest.mark.parametrize("shape", ["cells4", "cells65"])
def test_replicated_worlds_give_equal_bits(H, shape):
    case = cs.exact_case(cs.sensor_model(37), 60, *cs.SHAPES[shape], rows=20, seed=5, replicated=True)
    got = _run(H, case)
    assert np.any(got[0] != 0.0) and np.all(cs.bits(got) == cs.bits(got[:1]))
    case = cs.order_case(cs.sensor_model(5), 300, *cs.SHAPES[shape], rows=None, seed=6)
    for w in range(1, 5):  # world 0's contacts in every world, ids shifted
        live = case.shape0[:, 0] >= 0
        for arr in (case.shape0, case.shape1):
            local = live & (arr[:, 0] >= case.t.shape_local0) & (arr[:, 0] < case.t.shape_local0 + case.t.ns)
            arr[:, w] = np.where(local, arr[:, 0] + w * case.t.ns, arr[:, 0])
        case.impulse[:, :, w] = case.impulse[:, :, 0]
    got = _run(H, case)
    assert np.all(cs.bits(got) == cs.bits(got[:1]))
    assert np.array_equal(cs.bits(got), cs.bits(cs.order_alternatives(case)[0]))


def test_errors(H):
    case = cs.exact_case(cs.sensor_model(5), 40, *cs.SHAPES["cells20"], rows="ragged", seed=7)
    em, lib = _em(H, 5), H.lib()
    call = cs.HostCall(case, em.desc)
    a = call.args
    assert lib.nt_contact_sensor(None, C.byref(call.contacts), call.ptr(call.impulse), cs.DT, C.byref(a), None) == -1
    assert lib.nt_contact_sensor(C.byref(call.desc), None, call.ptr(call.impulse), cs.DT, C.byref(a), None) == -1
    assert lib.nt_contact_sensor(C.byref(call.desc), C.byref(call.contacts), call.ptr(call.impulse), cs.DT, None, None) == -1
    assert lib.nt_contact_sensor(C.byref(call.desc), C.byref(call.contacts), None, cs.DT, C.byref(a), None) == -1
    for dt in (0.0, -1.0, float("nan"), float("inf")):
        assert call.run(lib, dt=dt) == -1
    for field, bad in (("net_force", None), ("slot_sensing", None), ("slot_sensing_host", None), ("slot_counterpart", None),
                       ("slot_counterpart_host", None), ("sensing_count", 0), ("counterpart_count", -1), ("include_total", 2),
                       ("row_capacity", -1)):
        saved = getattr(a, field)
        setattr(a, field, bad)
        assert call.run(lib) == -1, field
        setattr(a, field, saved)
    saved, call.contacts.flat.row_start = call.contacts.flat.row_start, None  # rows with impulses, without their ranges
    assert call.run(lib) == -1
    call.contacts.flat.row_start = saved
    sens, cpart = call.host_tables  # entries outside their range, in the host copies
    for table, k, bad in ((sens, 3, case.S), (sens, 0, -2), (cpart, 22, case.C), (cpart, 1, -2)):
        saved, table[k] = table[k], bad
        assert call.run(lib) == -1
        table[k] = saved
    a.include_total, a.counterpart_count = 0, 0  # no column at all
    assert call.run(lib) == -1
    a.include_total, a.counterpart_count = case.tot, case.C
    assert np.all(call.net_force == cs.POISON)  # refused before any launch
    H.check(call.run(lib), "nt_contact_sensor")
    cs.check_exact(case, call.net_force)
