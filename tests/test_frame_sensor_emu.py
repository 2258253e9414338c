"""frame_sensor_kernel (nt_frame_sensor, include/newton_hip_kinematics.h) on the emulator: the kernel SOURCE executed on the CPU
(tests/emu), without a GPU, on the shared cases of tests/frame_sensor_cases.py against the float64 reference within the derived
tolerance.  1, 5 and 37 worlds (no multiple of the 64 worlds a workgroup takes, env_stride > env_count), 1, 3 and 70 rows: the emulated
grid is four workgroups, so everything above four rows takes the grid-stride loop."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import frame_sensor_cases as fc  # noqa: E402


@pytest.fixture(scope="module")
def H(oracle_lib):
    import harness

    harness.lib()  # builds tests/emu/_build/libnewton_emu.so on first use
    return harness


_EM = {}


def _em(H, case):
    key = (case.E, case.varied_gravity)
    if key not in _EM:
        _EM[key] = H.EmuModel(case.model)
    return _EM[key]


def _states(H, case):
    em = _em(H, case)
    return H.EmuState(em, body_q=case.body_q, body_qd=case.body_qd), H.EmuState(em, body_q=case.body_q, body_qd=case.body_qd_prev)


def _run(H, case, mask=None, only=tuple(fc.OUTPUTS)):
    em = _em(H, case)
    s, sp = _states(H, case)
    call = fc.Call(case, mask=mask, only=only)
    read = [s.body_q, s.body_qd, sp.body_qd, em.keep["body_param"], em.keep["gravity"], *call.keep[:4]]
    before = [x.tobytes() for x in read]
    ds, dp = s.desc(), sp.desc()
    H.check(call.run(H.lib(), em.desc, ds, dp if "accel" in only else None), "nt_frame_sensor")
    assert before == [x.tobytes() for x in read]  # the inputs are only read
    return call.out


@pytest.mark.parametrize("rows", fc.ROWS)
@pytest.mark.parametrize("worlds", fc.WORLDS)
def test_shared_cases_within_the_tolerance(H, worlds, rows):
    case = fc.case(worlds, rows)
    assert case.model.env.env_stride > worlds and worlds % fc.FR_THREADS
    ratios = fc.check(case.reference(), _run(H, case), what=f"emulator {worlds} worlds {rows} rows")
    assert set(ratios) == set(fc.OUTPUTS)


@pytest.mark.parametrize("only", list(fc.OUTPUTS))
def test_every_output_alone(H, only):
    """Every optional output NULL but one; the one that is there has the bits of the call with all four."""
    case = fc.case(5, 3)
    full = _run(H, case)
    got = _run(H, case, only=(only,))
    assert list(got) == [only]
    fc.check(case.reference(), got, what=f"emulator only {only}")
    assert np.array_equal(fc.bits(got[only]), fc.bits(full[only]))


def test_masked_worlds_keep_the_poison(H):
    """Worlds 1, 4 and 30 off, inside a live wave: their rows keep the poison, the live rows the bits of the unmasked run."""
    case = fc.case(37, 3)
    full = _run(H, case)
    mask = np.ones(37, bool)
    mask[[1, 4, 30]] = False
    got = _run(H, case, mask=mask)
    fc.check(case.reference(), got, mask=mask, what="emulator masked")
    for k in fc.OUTPUTS:
        assert np.array_equal(fc.bits(got[k][mask]), fc.bits(full[k][mask])) and np.all(got[k][~mask] == fc.POISON)


def test_worlds_in_equal_states_give_equal_bits(H):
    """One gravity for every world; the state of world 0 copied into worlds 2 and 36."""
    base = fc.case(37, 70, varied_gravity=False)
    case = fc.Case(37, 70, varied_gravity=False)
    nb = case.nb
    for w in (2, 36):
        for arr in (case.body_q, case.body_qd, case.body_qd_prev):
            arr[w * nb:(w + 1) * nb] = arr[:nb]
    assert not np.array_equal(base.body_q[:nb], base.body_q[nb:2 * nb])
    got = _run(H, case)
    fc.check(case.reference(), got, what="emulator replicated")
    for k in fc.OUTPUTS:
        assert np.array_equal(fc.bits(got[k][2]), fc.bits(got[k][0])) and np.array_equal(fc.bits(got[k][36]), fc.bits(got[k][0]))
        assert not np.array_equal(got[k][1], got[k][0])


def test_errors(H):
    case = fc.case(5, 3)
    em, lib = _em(H, case), H.lib()
    s, sp = _states(H, case)
    ds, dp = s.desc(), sp.desc()
    call = fc.Call(case)
    a = call.args
    INVALID = -1
    assert lib.nt_frame_sensor(None, C.byref(ds), C.byref(dp), fc.DT, C.byref(a), None) == INVALID
    assert lib.nt_frame_sensor(C.byref(em.desc), None, C.byref(dp), fc.DT, C.byref(a), None) == INVALID
    assert lib.nt_frame_sensor(C.byref(em.desc), C.byref(ds), C.byref(dp), fc.DT, None, None) == INVALID
    assert call.run(lib, em.desc, ds, None) == INVALID  # accel without the previous state
    for dt in (0.0, -1.0, float("nan"), float("inf")):
        assert call.run(lib, em.desc, ds, dp, dt=dt) == INVALID, dt
    for field, bad in (("frame_body", None), ("frame_xform", None), ("out_frame", None), ("out_ref", None), ("frame_body_host", None),
                       ("frame_xform_host", None), ("out_frame_host", None), ("out_ref_host", None), ("frame_count", 0), ("frame_count", -1),
                       ("out_count", 0), ("out_count", -3)):
        saved = getattr(a, field)
        setattr(a, field, bad)
        assert call.run(lib, em.desc, ds, dp) == INVALID, field
        setattr(a, field, saved)
    saved = {k: getattr(a, k) for k in fc.OUTPUTS}  # every output NULL
    for k in fc.OUTPUTS:
        setattr(a, k, None)
    assert call.run(lib, em.desc, ds, dp) == INVALID
    for k, v in saved.items():
        setattr(a, k, v)
    fbody, fxform, oframe, oref = call.host  # entries outside their range, in the host copies
    for table, idx, bad in ((fbody, 2, case.nb), (fbody, 0, -2), (oframe, 1, case.M), (oframe, 0, -1), (oref, 2, case.M), (oref, 0, -2),
                            (fxform, (1, 6), np.float32(fxform[1, 6] + 0.01)), (fxform, (0, 6), np.float32(1.0 - 2.0e-4)),
                            (fxform, (4, 0), np.float32(np.nan)), (fxform, (4, 5), np.float32(np.inf))):
        saved, table[idx] = table[idx], bad
        assert call.run(lib, em.desc, ds, dp) == INVALID, (idx, bad)
        table[idx] = saved
    no_qd = s.desc()
    no_qd.body_qd = None
    assert call.run(lib, em.desc, no_qd, dp) == INVALID  # velocity / accel without body_qd
    no_q = s.desc()
    no_q.body_q = None
    assert call.run(lib, em.desc, no_q, dp) == INVALID
    for out in call.out.values():
        assert np.all(out == fc.POISON)  # refused before any launch
    fxform[0, 6] = np.float32(1.0 + 5.0e-5)  # inside the 1e-4 bound of the quaternion norm (the device copy keeps 1)
    H.check(call.run(lib, em.desc, ds, dp), "nt_frame_sensor")
    fc.check(case.reference(), call.out, what="emulator after the refusals")
