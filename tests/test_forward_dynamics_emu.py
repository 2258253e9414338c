"""eval_forward_dynamics_kernel (include/newton_hip_kinematics.h) on the emulator: the kernel SOURCE executed on the CPU (tests/emu),
without a GPU.  37 worlds (not a multiple of any tile), one environment per workgroup and the default tile, against the float64
reference of tests/forward_dynamics_reference.py on identical fp32 inputs.

Gate: the backward error eta <= FD_GATE (test_forward_dynamics_host.py, where the per-scene maxima measured here are listed)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

from forward_dynamics_reference import fd_eta  # noqa: E402
from test_eval_jacobian_host import POISON, SCENES  # noqa: E402
from test_forward_dynamics_host import FD_GATE, N_WORLDS, fd_case, massless_leaf_model, report  # noqa: E402

ALL = 7  # NT_FD_GRAVITY | NT_FD_VELOCITY | NT_FD_BODY_F
INFO_POISON = -7


@pytest.fixture(scope="module")
def H(oracle_lib):
    import harness

    harness.lib()  # builds tests/emu/_build/libnewton_emu.so on first use
    return harness


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _run(H, em, state, model, joint_f, flags=ALL, epb=None, art_mask=None, want_info=True):
    """(joint_qdd, info) into poisoned arrays through nt_eval_forward_dynamics_tile (epb given) or nt_eval_forward_dynamics."""
    qdd = np.full((model.articulation_count, model.max_dofs_per_articulation), POISON, np.float32)
    info = np.full(model.articulation_count, INFO_POISON, np.int32) if want_info else None
    d = state.desc()
    mask = None if art_mask is None else np.ascontiguousarray(art_mask, dtype=np.uint8)
    lib, m = H.lib(), C.byref(em.desc)
    if epb is None:
        H.check(lib.nt_eval_forward_dynamics(m, C.byref(d), _ptr(joint_f), flags, _ptr(qdd), _ptr(info), _ptr(mask), None),
                "nt_eval_forward_dynamics")
    else:
        H.check(lib.nt_eval_forward_dynamics_tile(m, C.byref(d), _ptr(joint_f), flags, _ptr(qdd), _ptr(info), _ptr(mask), epb, None),
                "nt_eval_forward_dynamics_tile")
    return qdd, info


def _state(H, em, case):
    i = case.id
    return H.EmuState(em, body_q=i.bq, body_qd=i.bqd, joint_q=i.jq, joint_qd=i.qd, body_f=case.body_f)


def _setup(H, name, seed=21, E=N_WORLDS):
    case = fd_case(name, E, seed)
    em = H.EmuModel(case.model)
    return case, em, _state(H, em, case)


@pytest.mark.parametrize("epb", [1, 0])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_kernel_matches_reference(H, name, epb):
    case, em, s = _setup(H, name)
    joint_f = case.joint_f.copy()
    qdd, info = _run(H, em, s, case.model, joint_f, epb=epb)
    eta = report(f"emu epb {epb}", name, qdd, case.ref())
    assert eta <= FD_GATE, (name, eta)
    assert np.all(info == 0)
    assert all(np.all(qdd[a, n:] == 0.0) for a, n in enumerate(case.nda))  # the poison is gone from the padding: written as zero
    i = case.id
    assert np.array_equal(joint_f, case.joint_f) and np.array_equal(s.aos("body_f"), case.body_f)  # the inputs are only read
    assert np.array_equal(s.aos("joint_qd"), i.qd) and np.array_equal(s.aos("body_q"), i.bq) and np.array_equal(s.aos("joint_q"), i.jq)
    if epb == 0:  # the entry point without a tile argument takes the same tile as 0
        assert np.array_equal(_run(H, em, s, case.model, joint_f)[0], qdd)
        assert np.array_equal(_run(H, em, s, case.model, joint_f, want_info=False)[0], qdd)  # info NULL


@pytest.mark.parametrize("name", ["joint_zoo_free_root", "multi_art"])
def test_flag_combinations_and_null_joint_f(H, name):
    case, em, s = _setup(H, name)
    for flags, kw in ((6, dict(gravity=False)), (5, dict(velocity_terms=False)), (3, dict(body_f=False)), (4, dict(gravity=False, velocity_terms=False))):
        qdd, _ = _run(H, em, s, case.model, case.joint_f, flags=flags)
        assert fd_eta(qdd, case.ref(**kw)) <= FD_GATE, (name, flags)
    qdd, _ = _run(H, em, s, case.model, None)
    assert fd_eta(qdd, case.ref(joint_f=False)) <= FD_GATE
    qdd, info = _run(H, em, s, case.model, None, flags=0)
    assert np.all(qdd == 0.0) and np.all(info == 0)
    # NT_FD_BODY_F clear: body_f is not read and may be NULL
    i = case.id
    s0 = H.EmuState(em, body_q=i.bq, body_qd=i.bqd, joint_q=i.jq, joint_qd=i.qd)
    d = s0.desc()
    d.body_f = None
    want, _ = _run(H, em, s, case.model, case.joint_f, flags=3)
    got = np.full_like(want, POISON)
    assert H.lib().nt_eval_forward_dynamics(C.byref(em.desc), C.byref(d), _ptr(case.joint_f), 3, _ptr(got), None, None, None) == 0
    assert np.array_equal(got, want)
    assert H.lib().nt_eval_forward_dynamics(C.byref(em.desc), C.byref(d), _ptr(case.joint_f), 7, _ptr(got), None, None, None) == -1


@pytest.mark.parametrize("epb", [1, 4, 8, 16])
@pytest.mark.parametrize("name", ["d6_zoo", "multi_art"])
def test_every_tile_width_gives_the_same_bits(H, name, epb):
    case, em, s = _setup(H, name, seed=2)
    a, b = _run(H, em, s, case.model, case.joint_f, epb=0), _run(H, em, s, case.model, case.joint_f, epb=epb)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    d = s.desc()
    assert H.lib().nt_eval_forward_dynamics_tile(C.byref(em.desc), C.byref(d), None, ALL, _ptr(b[0]), None, None, 3, None) == -3  # not a compiled tile


@pytest.mark.parametrize("name", ["quadruped", "joint_zoo_free_root"])
def test_replicated_worlds_give_equal_bits(H, name):
    """Every world in the state of world 0: every articulation row equals its twin of world 0 bit for bit, in both tiles."""
    case, em, _ = _setup(H, name, seed=4)
    t, model, i = case.model.env, case.model, case.id
    E = t.env_count
    rep = lambda x, n: np.tile(np.asarray(x).reshape(E, n, -1)[0], (E, 1, 1)).reshape(np.asarray(x).shape)  # noqa: E731
    s = H.EmuState(em, body_q=rep(i.bq, t.nb), body_qd=rep(i.bqd, t.nb), joint_q=rep(i.jq, t.nc), joint_qd=rep(i.qd, t.nd),
                   body_f=rep(case.body_f, t.nb))
    joint_f = np.ascontiguousarray(rep(case.joint_f, t.na))
    for epb in (0, 1):
        qdd = _run(H, em, s, model, joint_f, epb=epb)[0].reshape(E, t.na, -1)
        assert np.all(qdd == qdd[:1]) and np.abs(qdd).max() > 1.0


@pytest.mark.parametrize("epb", [1, 0])
def test_masked_articulations_inside_a_live_workgroup_keep_their_poison(H, epb):
    case, em, s = _setup(H, "multi_art", seed=6)
    assert case.model.env.na == 3
    sel = np.random.default_rng(0).random(N_WORLDS * 3) < 0.5
    assert sel.any() and not sel.all()
    full, part = _run(H, em, s, case.model, case.joint_f, epb=epb), _run(H, em, s, case.model, case.joint_f, epb=epb, art_mask=sel)
    assert np.array_equal(part[0][sel], full[0][sel]) and np.all(part[0][~sel] == POISON)
    assert np.all(part[1][sel] == 0) and np.all(part[1][~sel] == INFO_POISON)


@pytest.mark.parametrize("epb", [1, 0, 8])
@pytest.mark.parametrize("name", ["multi_art", "quadruped"])
def test_massless_leaf_is_reported_and_stays_in_its_articulation(H, name, epb):
    """A leaf link without mass and inertia in the worlds w % 3 == 1 (multi_art: the bad articulation sits beside two good ones of the
    same world, in the same workgroup): its articulation comes back all-NaN with info > 0, every other articulation carries the bits
    of the run without the edit and info 0 -- a leaked pivot fallback or a workgroup-wide failure flag shows here."""
    case, em, s = _setup(H, name, seed=3)
    good, good_info = _run(H, em, s, case.model, case.joint_f, epb=epb)
    model, bad = massless_leaf_model(name, N_WORLDS)
    em_bad = H.EmuModel(model)
    got, info = _run(H, em_bad, _state(H, em_bad, case), model, case.joint_f, epb=epb)
    assert bad.any() and np.all(good_info == 0) and np.all(np.isfinite(good))
    for a in np.flatnonzero(bad):
        assert np.all(np.isnan(got[a, :case.nda[a]])) and np.all(got[a, case.nda[a]:] == 0.0) and 0 < info[a] <= case.nda[a]
    assert np.array_equal(got[~bad], good[~bad]) and np.all(info[~bad] == 0)


def test_argument_errors(H):
    case, em, s = _setup(H, "pendulum", seed=1, E=3)
    qdd = np.full((3, case.D), POISON, np.float32)
    d = s.desc()
    fn = H.lib().nt_eval_forward_dynamics
    assert fn(None, C.byref(d), None, ALL, _ptr(qdd), None, None, None) == -1
    assert fn(C.byref(em.desc), None, None, ALL, _ptr(qdd), None, None, None) == -1
    assert fn(C.byref(em.desc), C.byref(d), None, ALL, None, None, None, None) == -1
    assert fn(C.byref(em.desc), C.byref(d), None, 8, _ptr(qdd), None, None, None) == -1  # an unknown flag bit
    assert np.all(qdd == POISON)
