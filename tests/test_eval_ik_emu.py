"""eval_ik_kernel (nt_eval_ik / nt_eval_ik_tile, include/newton_hip_kinematics.h) on the emulator: the kernel SOURCES executed on the
CPU (tests/emu), without a GPU.  37 worlds (not a multiple of any tile), one environment per workgroup and the default tile, against
the float64 reference of tests/test_eval_ik_host.py on identical fp32 body states.  Gates: the standing single-call kinematics gate
of test_eval_fk_device_matches_oracle -- 1e-5 on coordinates, 1e-5 * max(1, V) on rates (see test_eval_ik_host.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import newton_amd as nt  # noqa: E402
from test_eval_ik_host import SCENES, fk_case, ik_errors, ik_reference, within_gates  # noqa: E402

N_WORLDS = 37
POISON_Q, POISON_QD = 7.0, -7.0


@pytest.fixture(scope="module")
def H(oracle_lib):
    import harness

    harness.lib()  # builds tests/emu/_build/libnewton_emu.so on first use
    return harness


def _eval_ik(H, em, state, epb=0, art_mask=None, tile_entry=True):
    """In place into the state's own joint arrays; returns the status."""
    d = state.desc()
    mask = None if art_mask is None else np.ascontiguousarray(art_mask, dtype=np.uint8)
    mp = None if mask is None else mask.ctypes.data_as(C.c_void_p)
    if tile_entry:
        return H.lib().nt_eval_ik_tile(C.byref(em.desc), C.byref(d), d.joint_q, d.joint_qd, mp, epb, None)
    return H.lib().nt_eval_ik(C.byref(em.desc), C.byref(d), d.joint_q, d.joint_qd, mp, None)


def _state(H, em, bq, bqd):
    m = em.model
    return H.EmuState(em, body_q=bq, body_qd=bqd, joint_q=np.full(m.joint_coord_count, POISON_Q, np.float32),
                      joint_qd=np.full(m.joint_dof_count, POISON_QD, np.float32))


@pytest.mark.parametrize("epb", [1, 0])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_kernel_matches_reference(H, name, epb):
    model, _jq, _jqd, bq, bqd = fk_case(name, N_WORLDS, 21)
    em = H.EmuModel(model)
    s = _state(H, em, bq, bqd)
    H.check(_eval_ik(H, em, s, epb=epb), "nt_eval_ik_tile")
    rq, rqd, wq, wqd = ik_reference(model, bq, bqd)
    gq, gqd = s.aos("joint_q"), s.aos("joint_qd")
    assert wq.all() and wqd.all() and not np.any(gq == POISON_Q) and not np.any(gqd == POISON_QD)
    errs = ik_errors(model, gq, gqd, rq, rqd, bqd)
    print(f"[eval_ik emu] {name} epb {epb}: coord err {errs[0]:.3e} rate err/scale {errs[1]:.3e}")
    assert within_gates(errs)
    assert np.array_equal(s.aos("body_q"), bq) and np.array_equal(s.aos("body_qd"), bqd)  # the body state is only read
    # every tile computes the same bits, and so does the host mirror's selection of entries
    s2 = _state(H, em, bq, bqd)
    H.check(_eval_ik(H, em, s2, tile_entry=False), "nt_eval_ik")
    assert np.array_equal(s2.joint_q, s.joint_q) and np.array_equal(s2.joint_qd, s.joint_qd)


@pytest.mark.parametrize("epb", [1, 4, 8, 16])
def test_every_tile_width_gives_the_same_bits(H, epb):
    model, _jq, _jqd, bq, bqd = fk_case("d6_zoo", N_WORLDS, 2)
    em = H.EmuModel(model)
    a, b = _state(H, em, bq, bqd), _state(H, em, bq, bqd)
    H.check(_eval_ik(H, em, a, epb=0), "nt_eval_ik_tile")
    H.check(_eval_ik(H, em, b, epb=epb), "nt_eval_ik_tile")
    assert np.array_equal(a.joint_q, b.joint_q) and np.array_equal(a.joint_qd, b.joint_qd)
    assert _eval_ik(H, em, b, epb=3) == -3  # not a compiled tile


@pytest.mark.parametrize("epb", [1, 0])
def test_masked_launch(H, epb):
    """One byte per (world, articulation): the joints of unselected articulations keep their bits, the others equal the full launch."""
    model, _jq, _jqd, bq, bqd = fk_case("free_child", N_WORLDS, 6)
    em = H.EmuModel(model)
    t = model.env
    assert t.na == 1
    rng = np.random.default_rng(0)
    sel = rng.random(N_WORLDS * t.na) < 0.5
    full, part = _state(H, em, bq, bqd), _state(H, em, bq, bqd)
    H.check(_eval_ik(H, em, full, epb=epb), "nt_eval_ik_tile")
    H.check(_eval_ik(H, em, part, epb=epb, art_mask=sel), "nt_eval_ik_tile")
    fq, fqd = full.aos("joint_q").reshape(N_WORLDS, -1), full.aos("joint_qd").reshape(N_WORLDS, -1)
    pq, pqd = part.aos("joint_q").reshape(N_WORLDS, -1), part.aos("joint_qd").reshape(N_WORLDS, -1)
    assert sel.any() and not sel.all()
    assert np.array_equal(pq[sel], fq[sel]) and np.array_equal(pqd[sel], fqd[sel])
    assert np.all(pq[~sel] == POISON_Q) and np.all(pqd[~sel] == POISON_QD)
    # the padding columns behind the last world are never written
    assert np.all(part.joint_q[:, :, N_WORLDS:] == 0.0) and np.all(full.joint_q[:, :, N_WORLDS:] == 0.0)


def test_masked_launch_three_articulations_per_world(H):
    from scenes import box_stack_scene

    model = box_stack_scene(N_WORLDS, n_boxes=3)  # three free bodies = three articulations per world
    t = model.env
    assert t.na == 3
    em = H.EmuModel(model)
    rng = np.random.default_rng(5)
    bqd = rng.normal(0, 1, size=(model.body_count, 6)).astype(np.float32)
    sel = rng.random(N_WORLDS * t.na) < 0.5
    full, part = _state(H, em, model.body_q, bqd), _state(H, em, model.body_q, bqd)
    H.check(_eval_ik(H, em, full), "nt_eval_ik_tile")
    H.check(_eval_ik(H, em, part, art_mask=sel), "nt_eval_ik_tile")
    fq, pq = full.aos("joint_q").reshape(-1, 7), part.aos("joint_q").reshape(-1, 7)
    fqd, pqd = full.aos("joint_qd").reshape(-1, 6), part.aos("joint_qd").reshape(-1, 6)
    assert np.array_equal(pq[sel], fq[sel]) and np.array_equal(pqd[sel], fqd[sel])
    assert np.all(pq[~sel] == POISON_Q) and np.all(pqd[~sel] == POISON_QD)
    rq, rqd, _, _ = ik_reference(model, model.body_q, bqd)
    assert within_gates(ik_errors(model, full.aos("joint_q"), full.aos("joint_qd"), rq, rqd, bqd))


def test_state_after_xpbd_substeps_with_contacts(H):
    """20 XPBD substeps with live contacts leave the joints slightly violated: eval_ik projects, the reference does the same."""
    from scenes import quadruped_scene

    model = quadruped_scene(N_WORLDS)
    model.joint_q.reshape(N_WORLDS, -1)[:, 2] -= 0.26  # lowered into contact
    model.body_q, model.body_qd = nt.articulation.eval_fk_numpy(model, model.joint_q, model.joint_qd)
    em = H.EmuModel(model)
    s0, s1 = H.EmuState(em), H.EmuState(em)
    rng = np.random.default_rng(3)
    ctrl = H.EmuControl(em, joint_f=rng.normal(0, 1.0, size=model.joint_dof_count).astype(np.float32))
    ct = H.EmuContacts(em)
    out = H.xpbd_rollout(em, s0, s1, ctrl, ct, 1e-3, 20)
    assert int(ct.env_count[:N_WORLDS].sum()) > 0
    bq, bqd = out.aos("body_q"), out.aos("body_qd")
    before = out.aos("joint_q").copy()
    H.check(_eval_ik(H, em, out), "nt_eval_ik_tile")
    rq, rqd, _, _ = ik_reference(model, bq, bqd)
    errs = ik_errors(model, out.aos("joint_q"), out.aos("joint_qd"), rq, rqd, bqd)
    print(f"[eval_ik emu] after 20 XPBD substeps: coord err {errs[0]:.3e} rate err/scale {errs[1]:.3e}")
    assert within_gates(errs)
    assert np.abs(out.aos("joint_q") - before).max() > 1e-3  # the solver had left the initial pose there


def test_identical_worlds_give_identical_bits(H):
    from scenes import quadruped_scene

    model = quadruped_scene(N_WORLDS, seed=None)
    one = SCENES["quadruped"](1)
    jq = np.tile(np.asarray(one.joint_q, dtype=np.float32) + np.float32(0.1), N_WORLDS)
    jqd = np.tile(np.random.default_rng(9).normal(size=one.joint_dof_count).astype(np.float32), N_WORLDS)
    bq, bqd = nt.articulation.eval_fk_numpy(model, jq, jqd)
    assert np.array_equal(bq.reshape(N_WORLDS, -1), np.tile(bq.reshape(N_WORLDS, -1)[:1], (N_WORLDS, 1)))
    em = H.EmuModel(model)
    for epb in (1, 0):
        s = _state(H, em, bq, bqd)
        H.check(_eval_ik(H, em, s, epb=epb), "nt_eval_ik_tile")
        q, qd = s.aos("joint_q").reshape(N_WORLDS, -1), s.aos("joint_qd").reshape(N_WORLDS, -1)
        assert np.array_equal(q, np.tile(q[:1], (N_WORLDS, 1))) and np.array_equal(qd, np.tile(qd[:1], (N_WORLDS, 1)))


def test_argument_errors(H):
    model, _jq, _jqd, bq, bqd = fk_case("pendulum", 3, 1)
    em = H.EmuModel(model)
    s = _state(H, em, bq, bqd)
    d = s.desc()
    lib = H.lib()
    assert lib.nt_eval_ik(None, C.byref(d), d.joint_q, d.joint_qd, None, None) == -1
    assert lib.nt_eval_ik(C.byref(em.desc), None, d.joint_q, d.joint_qd, None, None) == -1
    assert lib.nt_eval_ik(C.byref(em.desc), C.byref(d), None, d.joint_qd, None, None) == -1
    assert lib.nt_eval_ik(C.byref(em.desc), C.byref(d), d.joint_q, None, None, None) == -1
    assert np.all(s.aos("joint_q") == POISON_Q)
