"""eval_inverse_dynamics_kernel (include/newton_hip_kinematics.h) on the emulator: the kernel SOURCE executed on the CPU (tests/emu),
without a GPU.  37 worlds (not a multiple of any tile), one environment per workgroup and the default tile, against the float64
finite-difference reference of tests/inverse_dynamics_reference.py on identical fp32 inputs.

Gate: |tau - tau_ref| / max(1, max|tau_ref| of the articulation) <= ID_GATE (test_inverse_dynamics_host.py, where the per-scene
maxima measured here are listed)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

from inverse_dynamics_reference import id_error  # noqa: E402
from test_eval_jacobian_host import POISON, SCENES  # noqa: E402
from test_inverse_dynamics_host import ID_GATE, id_case  # noqa: E402

N_WORLDS = 37
BOTH = 3  # NT_ID_GRAVITY | NT_ID_VELOCITY


@pytest.fixture(scope="module")
def H(oracle_lib):
    import harness

    harness.lib()  # builds tests/emu/_build/libnewton_emu.so on first use
    return harness


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _run(H, em, state, model, qdd, flags=BOTH, epb=None, art_mask=None):
    """tau into a poisoned array through nt_eval_inverse_dynamics_tile (epb given) or nt_eval_inverse_dynamics."""
    tau = np.full((model.articulation_count, model.max_dofs_per_articulation), POISON, np.float32)
    d = state.desc()
    mask = None if art_mask is None else np.ascontiguousarray(art_mask, dtype=np.uint8)
    lib, m = H.lib(), C.byref(em.desc)
    if epb is None:
        H.check(lib.nt_eval_inverse_dynamics(m, C.byref(d), _ptr(qdd), flags, _ptr(tau), _ptr(mask), None), "nt_eval_inverse_dynamics")
    else:
        H.check(lib.nt_eval_inverse_dynamics_tile(m, C.byref(d), _ptr(qdd), flags, _ptr(tau), _ptr(mask), epb, None),
                "nt_eval_inverse_dynamics_tile")
    return tau


def _setup(H, name, seed=21, E=N_WORLDS):
    case = id_case(name, E, seed)
    em = H.EmuModel(case.model)
    return case, em, H.EmuState(em, body_q=case.bq, body_qd=case.bqd, joint_q=case.jq, joint_qd=case.qd)


@pytest.mark.parametrize("epb", [1, 0])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_kernel_matches_reference(H, name, epb):
    case, em, s = _setup(H, name)
    tau = _run(H, em, s, case.model, case.qdd, epb=epb)
    err = id_error(tau, case.ref())
    print(f"[eval_inverse_dynamics emu] {name} epb {epb}: max |tau - tau_ref| / max(1, max|tau_ref|) {err:.3e}")
    assert err <= ID_GATE, (name, err)
    nda = np.asarray([hi - lo for lo, hi in case.dof_ranges])
    assert all(np.all(tau[a, n:] == 0.0) for a, n in enumerate(nda))  # the poison is gone from the padding: written as zero
    assert np.array_equal(s.aos("joint_qd"), case.qd) and np.array_equal(s.aos("body_q"), case.bq)  # the state is only read
    if epb == 0:  # the entry point without a tile argument takes the same tile as 0
        assert np.array_equal(_run(H, em, s, case.model, case.qdd), tau)
        # bias forces alone (joint_qdd NULL) and the flag combinations, against the reference, on the scale of the whole result
        for flags, kw in ((3, {}), (1, dict(velocity_terms=False)), (2, dict(gravity=False))):
            h = _run(H, em, s, case.model, None, flags=flags)
            assert id_error(h, case.ref(qdd=False, **kw), scale_ref=case.ref()) <= ID_GATE, (name, flags)
        assert np.all(_run(H, em, s, case.model, None, flags=0) == 0.0)


@pytest.mark.parametrize("epb", [1, 4, 8, 16])
@pytest.mark.parametrize("name", ["d6_zoo", "multi_art"])
def test_every_tile_width_gives_the_same_bits(H, name, epb):
    case, em, s = _setup(H, name, seed=2)
    a, b = _run(H, em, s, case.model, case.qdd, epb=0), _run(H, em, s, case.model, case.qdd, epb=epb)
    assert np.array_equal(a, b)
    d = s.desc()
    assert H.lib().nt_eval_inverse_dynamics_tile(C.byref(em.desc), C.byref(d), None, BOTH, _ptr(b), None, 3, None) == -3  # not a compiled tile


@pytest.mark.parametrize("name", ["quadruped", "joint_zoo_free_root"])
def test_replicated_worlds_give_equal_bits(H, name):
    """Every world in the state of world 0: every articulation row equals its twin of world 0 bit for bit, in both tiles."""
    case, em, _ = _setup(H, name, seed=4)
    t, model = case.model.env, case.model
    E = t.env_count
    rep = lambda x, n: np.tile(np.asarray(x).reshape(E, n, -1)[0], (E, 1, 1)).reshape(np.asarray(x).shape)  # noqa: E731
    s = H.EmuState(em, body_q=rep(case.bq, t.nb), body_qd=rep(case.bqd, t.nb), joint_q=rep(case.jq, t.nc), joint_qd=rep(case.qd, t.nd))
    qdd = np.ascontiguousarray(rep(case.qdd, t.na))
    for epb in (0, 1):
        tau = _run(H, em, s, model, qdd, epb=epb).reshape(E, t.na, -1)
        assert np.all(tau == tau[:1]) and np.abs(tau).max() > 1.0


@pytest.mark.parametrize("epb", [1, 0])
def test_masked_articulations_inside_a_live_workgroup_keep_their_poison(H, epb):
    case, em, s = _setup(H, "multi_art", seed=6)
    assert case.model.env.na == 3
    sel = np.random.default_rng(0).random(N_WORLDS * 3) < 0.5
    assert sel.any() and not sel.all()
    full, part = _run(H, em, s, case.model, case.qdd, epb=epb), _run(H, em, s, case.model, case.qdd, epb=epb, art_mask=sel)
    assert np.array_equal(part[sel], full[sel]) and np.all(part[~sel] == POISON)


def test_argument_errors(H):
    case, em, s = _setup(H, "pendulum", seed=1, E=3)
    tau = np.full((3, 1), POISON, np.float32)
    d = s.desc()
    fn = H.lib().nt_eval_inverse_dynamics
    assert fn(None, C.byref(d), None, BOTH, _ptr(tau), None, None) == -1
    assert fn(C.byref(em.desc), None, None, BOTH, _ptr(tau), None, None) == -1
    assert fn(C.byref(em.desc), C.byref(d), None, BOTH, None, None, None) == -1
    assert fn(C.byref(em.desc), C.byref(d), None, 4, _ptr(tau), None, None) == -1  # an unknown flag bit
    assert np.all(tau == POISON)
