"""The tile image (nt_model.tile_image_words, found at nt_model.body_flags; include/newton_hip.h; packed by nt_model_create / nt_model_refresh_params in csrc/nt_model_build.hip, copied by
the Ctx constructor of csrc/nt_ctx.hpp): the block-shared region of the kernels' LDS tile as ONE host-packed image, on the emulator
(the kernel SOURCES executed on the CPU, tests/emu), without a GPU.

 * the image, word for word, against numpy restatements of the layout -- table order and lengths, joint_inc, pair_desc, the parameter
   block of a uniform-parameter tile with the kinematic zeroing -- on models with a kinematic body, with global shapes, with convex
   pairs and on the pair-heavy tile;
 * every kernel family with the image against the same launch under NT_TILE_IMAGE=0 (the table-by-table staging), bit for bit;
 * after nt_model_refresh_params the image equals a freshly created model's, and so do the results.

The emulated descriptor (tests/emu/harness.py: EmuModel) is built in Python and carries no image; the tests create the C handle beside
it (host memory, on_device = 0, as tests/test_model_build.py does) and copy the image over: body_flags, which then points at the image,
and the word count."""
import ctypes as C
import os
import sys
from contextlib import contextmanager

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))

NB_F, NJ_F, ND_F, NS_F = 23, 14, 11, 20  # NT_*_PARAM_FLOATS
BP_INV_MASS, BP_INV_INERTIA = 3, 13
KINEMATIC = 2


@pytest.fixture(scope="module")
def H():
    import harness

    harness.lib()
    return harness


@contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class _Handle:
    """nt_model_create(src, 0, ...) of the emulated library: the image lives in the handle's host memory."""

    def __init__(self, H, model):
        from newton_amd.model import newton_model_struct

        self.lib = H.lib()
        src, self.keep = newton_model_struct(model)
        self.h = C.c_void_p()
        rc = self.lib.nt_model_create(C.byref(src), 0, C.byref(self.h))
        assert rc == 0, self.lib.nt_model_last_error()
        self.d = self.lib.nt_model_get(self.h).contents

    def refresh(self, model):
        from newton_amd.model import newton_model_struct

        src, keep = newton_model_struct(model)
        assert self.lib.nt_model_refresh_params(self.h, C.byref(src)) == 0, self.lib.nt_model_last_error()

    def image(self):
        n = int(self.d.tile_image_words)
        assert self.d.body_flags and self.d.body_flags % 16 == 0 and n > 0  # (the image starts at body_flags)
        return np.ctypeslib.as_array(C.cast(self.d.body_flags, C.POINTER(C.c_int32)), shape=(n,)).copy()

    def attach(self, em):
        em.desc.body_flags, em.desc.tile_image_words = self.d.body_flags, self.d.tile_image_words
        return em

    def close(self):
        self.lib.nt_model_destroy(self.h)


def _emu_model(H, model):
    """EmuModel with the C handle's image attached; the handle stays alive with it."""
    em = H.EmuModel(model)
    em.image_handle = _Handle(H, model)
    assert em.desc.tile_image_words == 0  # the Python-built descriptor: no image
    return em.image_handle.attach(em)


# ------------------------------------------------------------------------------------------------
# scenes
# ------------------------------------------------------------------------------------------------
def _lowered_quadrupeds(n, seed=5, kinematic_body=None):
    import newton_amd as nt
    from scenes import quadruped_builder

    q = quadruped_builder()
    if kinematic_body is not None:
        q.body_flags[kinematic_body] = int(nt.BodyFlags.KINEMATIC)
    scene = nt.ModelBuilder()
    scene.replicate(q, n)
    scene.add_ground_plane(cfg=q.default_shape_cfg)
    model = scene.finalize(device=None)
    jq = model.joint_q.reshape(n, -1)
    jq[:, 2] += np.random.default_rng(seed).uniform(0.0, 0.05, size=n).astype(np.float32) - 0.24  # feet in the ground: live contacts
    model.body_q, model.body_qd = nt.articulation.eval_fk_numpy(model, model.joint_q, model.joint_qd)
    return model


def _heavier(model, body, worlds, factor=2.0):
    """body `body` of the given worlds gets `factor` times its mass (mass and inverse mass: the dynamics follow)"""
    nb = model.env.nb
    model.body_mass = np.array(model.body_mass, copy=True)
    model.body_inv_mass = np.array(model.body_inv_mass, copy=True)
    for w in worlds:
        model.body_mass[w * nb + body] *= factor
        model.body_inv_mass[w * nb + body] /= factor
    return model


# ------------------------------------------------------------------------------------------------
# the image, word for word
# ------------------------------------------------------------------------------------------------
def _expected_image(model, t, desc):
    from newton_amd.model import pack_param_arrays, params_uniform

    i32 = lambda a, n: np.asarray(a, dtype=np.int32).reshape(-1)[:n]  # noqa: E731
    nsg = t.ns + t.ng
    tables = [("body_flags", t.nb)] + [(k, t.nj) for k in (
        "joint_type", "joint_enabled", "joint_parent", "joint_child", "joint_q_start", "joint_qd_start", "joint_tq_start",
        "joint_lin_count", "joint_ang_count")] + [("shape_body", nsg), ("tile_shape_type", nsg), ("shape_flags", nsg), ("shape_group", nsg),
                                                  ("pair_a", t.np), ("pair_b", t.np), ("body_joint_start", t.nb + 1),
                                                  ("body_joint_list", 2 * t.nj), ("body_pair_start", t.nb + 1), ("body_pair_list", 2 * t.np),
                                                  ("shape_mesh_start", nsg), ("shape_mesh_count", nsg), ("gshape_id", t.ng)]
    assert len(tables) == 23
    parts = [i32(getattr(t, k), n) for k, n in tables]
    packed = pack_param_arrays(model, t)
    parts.append(np.ascontiguousarray(packed["gshape_param"], dtype=np.float32).reshape(-1)[:NS_F * t.ng].view(np.int32))
    parts.append(np.zeros(13 * t.ng, dtype=np.int32))  # gworld: the kernels fill it
    # joint_inc: position of (joint j, side) in the real entries of body_joint_list, the last match; -1 for the world side
    nlist = int(t.body_joint_start[t.nb]) if t.nj else 0
    inc = np.full(2 * t.nj, -1, dtype=np.int32)
    for k in range(nlist):
        inc[int(t.body_joint_list[k])] = k
    parts.append(inc)
    if desc.contact_scratch_in_hbm:
        parts.append(np.zeros(1 + t.np, dtype=np.int32))  # hit_count + hit_list: the pair-heavy kernels fill them
    else:
        ty, body = np.asarray(t.tile_shape_type), np.asarray(t.shape_body)
        pd = np.zeros((t.np, 4), dtype=np.int32)
        for p in range(t.np):
            sa, sb, swapped = int(t.pair_a[p]), int(t.pair_b[p]), 0
            if ty[sa] > ty[sb]:
                sa, sb, swapped = sb, sa, 1
            pd[p] = (sa, sb, body[sa], (int(body[sb]) & 0x3fffffff) | (swapped << 30))
        parts.append(pd.reshape(-1))
    topo = np.concatenate(parts)
    if not params_uniform(packed, t.env_count):
        return topo, None
    odd = lambda n: n | 1  # noqa: E731  (LDS fields have odd strides)
    blocks = []
    for key, n, nf in (("body_param", t.nb, NB_F), ("joint_param", t.nj, NJ_F), ("dof_param", t.nd, ND_F), ("shape_param", t.ns, NS_F)):
        col0 = np.ascontiguousarray(packed[key], dtype=np.float32).reshape(-1, t.env_stride)[:nf * max(n, 0), 0].reshape(nf, n) if n else np.zeros((nf, 0), np.float32)
        blk = np.zeros((n, odd(nf)), dtype=np.float32)
        blk[:, :nf] = col0.T
        if key == "body_param":
            kin = (np.asarray(t.body_flags)[:n] & KINEMATIC) != 0
            blk[kin, BP_INV_MASS] = 0.0
            blk[kin, BP_INV_INERTIA:BP_INV_INERTIA + 9] = 0.0
        blocks.append(blk.reshape(-1))
    return topo, np.concatenate(blocks).view(np.int32)


def _image_scenes():
    from scenes import box_stack_scene, hull_bin_scene, mixed_primitive_scene, pendulum_scene

    return {
        "quadruped": lambda: _lowered_quadrupeds(5),                               # ng = 1 (the ground plane is a global shape)
        "quadruped_kinematic": lambda: _lowered_quadrupeds(3, kinematic_body=4),   # zeroed inverse mass / inertia in the block
        "quadruped_one_heavy": lambda: _heavier(_lowered_quadrupeds(4), 2, [1]),   # not uniform: topology only
        "mixed_primitives": lambda: mixed_primitive_scene(4),
        "box_stack": lambda: box_stack_scene(3, n_boxes=4, seed=1),                # convex pairs
        "pendulum": lambda: pendulum_scene(6, seed=2),                             # no pairs at all
        "hull_bin_pair_heavy": lambda: hull_bin_scene(1, 40),                      # contact_scratch_in_hbm: hit list instead of pair_desc
    }


@pytest.mark.parametrize("name", ["quadruped", "quadruped_kinematic", "quadruped_one_heavy", "mixed_primitives", "box_stack", "pendulum",
                                  "hull_bin_pair_heavy"])
def test_image_is_the_block_shared_region_word_for_word(H, name):
    model = _image_scenes()[name]()
    em = H.EmuModel(model)
    t = model.env
    hd = _Handle(H, model)
    try:
        assert hd.d.contact_scratch_in_hbm == em.desc.contact_scratch_in_hbm and hd.d.params_uniform == em.desc.params_uniform
        topo, params = _expected_image(model, t, em.desc)
        got = hd.image()
        assert len(got) == len(topo) + (0 if params is None else len(params))
        assert np.array_equal(got[:len(topo)], topo)
        if params is not None:
            assert np.array_equal(got[len(topo):], params)
        if name == "quadruped_kinematic":
            assert (np.asarray(t.body_flags) & KINEMATIC).any() and params is not None
        if name == "quadruped_one_heavy":
            assert params is None
        if name == "hull_bin_pair_heavy":
            assert em.desc.contact_scratch_in_hbm == 1
        if name.startswith("quadruped"):
            assert t.ng > 0
    finally:
        hd.close()


# ------------------------------------------------------------------------------------------------
# with the image == without, bit for bit
# ------------------------------------------------------------------------------------------------
def _bits(x):
    return x.view(np.int32) if x.dtype == np.float32 else x


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(_bits(x), _bits(y))


def _xpbd_rollout(H, em, cfg, image, substeps=6, dt=1e-3, iterations=2, epb=0):
    a, b, ct, ctrl = H.EmuState(em), H.EmuState(em), H.EmuContacts(em), H.EmuControl(em)
    ctrl.joint_f[:] = 0.3
    with _env(NT_XPBD_CFG=cfg, NT_TILE_IMAGE=None if image else "0"):
        out = H.xpbd_rollout(em, a, b, ctrl, ct, dt, substeps, epb=epb, iterations=iterations)
    live = np.broadcast_to((ct.shape0 >= 0)[None, ...], ct.data.shape)  # (a dead slot's record is whatever was there)
    return out.body_q.copy(), out.body_qd.copy(), ct.shape0.copy(), ct.env_count.copy(), np.where(live, ct.data.view(np.int32), 0)


@pytest.fixture(scope="module")
def quadrupeds40(H):
    em = _emu_model(H, _lowered_quadrupeds(40))  # three workgroups of 16, the last one ragged
    yield em
    em.image_handle.close()


@pytest.fixture(scope="module")
def quadrupeds40_reference(H, quadrupeds40):
    """the generic uniform tile of 16 without the image: what every instance must reproduce"""
    return _xpbd_rollout(H, quadrupeds40, "16,512,1,1,0,0", image=False)


@pytest.mark.parametrize("cfg", ["16,512,1,1,0,1", "16,512,1,1,0,0"])
def test_xpbd_rollout_with_image_is_bitwise_the_staged_one(H, quadrupeds40, quadrupeds40_reference, cfg):
    em = quadrupeds40
    assert em.desc.params_uniform == 1
    got = _xpbd_rollout(H, em, cfg, image=True)
    _same(got, quadrupeds40_reference)
    assert np.abs(got[1]).max() > 0.0 and got[3][:40].min() > 0  # moving, in contact
    if cfg.endswith(",1"):  # the specialised instance's own staged path as well
        _same(_xpbd_rollout(H, em, cfg, image=False), quadrupeds40_reference)


def test_per_environment_tile_takes_the_topology_part_only(H):
    model = _heavier(_lowered_quadrupeds(40), 2, [7])
    em = _emu_model(H, model)
    try:
        assert em.desc.params_uniform == 0
        from newton_amd.model import pack_param_arrays  # noqa: F401

        assert em.desc.tile_image_words == len(_expected_image(model, model.env, em.desc)[0])
        _same(_xpbd_rollout(H, em, None, image=True), _xpbd_rollout(H, em, None, image=False))
    finally:
        em.image_handle.close()


def test_hand_flipped_uniform_flag_falls_back_to_loading_the_parameters(H, quadrupeds40, quadrupeds40_reference):
    """A descriptor whose image has no parameter block while params_uniform says 1 (flipped by hand): the uniform tile loads its
    parameter copy from the tables as it does without an image."""
    em = quadrupeds40
    words = em.desc.tile_image_words
    try:
        em.desc.tile_image_words = len(_expected_image(em.model, em.t, em.desc)[0])
        _same(_xpbd_rollout(H, em, "16,512,1,1,0,1", image=True), quadrupeds40_reference)
    finally:
        em.desc.tile_image_words = words


def test_convex_rollout_with_image_is_bitwise_the_staged_one(H):
    from scenes import box_stack_scene

    em = _emu_model(H, box_stack_scene(19, n_boxes=4, seed=7, jitter=2e-3))
    try:
        assert em.t.np_analytic < em.t.np
        for cfg, epb in ((None, 8), ("16,512,1,1,1", 0)):
            _same(_xpbd_rollout(H, em, cfg, True, substeps=4, dt=1.0 / 240.0, iterations=4, epb=epb),
                  _xpbd_rollout(H, em, cfg, False, substeps=4, dt=1.0 / 240.0, iterations=4, epb=epb))
    finally:
        em.image_handle.close()


def test_collide_and_step_call_by_call(H, quadrupeds40):
    em = quadrupeds40

    def loop(image, substeps=3):
        a, b, ct, ctrl = H.EmuState(em), H.EmuState(em), H.EmuContacts(em), H.EmuControl(em)
        ctrl.joint_f[:] = 0.3
        with _env(NT_XPBD_CFG=None, NT_TILE_IMAGE=None if image else "0"):
            for _ in range(substeps):
                a.body_f[:] = 0
                H.collide(em, a, ct)
                H.xpbd_step(em, a, b, ctrl, ct, 1e-3, iterations=2)
                a, b = b, a
        return a.body_q.copy(), a.body_qd.copy(), ct.shape0.copy(), ct.env_count.copy(), ct.data.copy()

    got = loop(True)
    _same(got, loop(False))
    assert got[3][:40].min() > 0


def test_tables_longer_than_the_workgroup(H):
    """The pair-heavy scene: pair tables, incidence list and image are longer than one trip of the workgroup (at most 384 lanes), so
    the table-by-table staging runs its tail loops and the image copy its trips beyond the two issued at once.  One collide launch."""
    from scenes import hull_bin_scene

    em = _emu_model(H, hull_bin_scene(1, 40))
    try:
        assert em.desc.contact_scratch_in_hbm == 1
        assert em.t.np > 384 and em.desc.tile_image_words > 2 * 384 * 4

        def collide(image):
            a, ct = H.EmuState(em), H.EmuContacts(em)
            with _env(NT_XPBD_CFG=None, NT_TILE_IMAGE=None if image else "0"):
                H.collide(em, a, ct)
            live = np.broadcast_to((ct.shape0 >= 0)[None, ...], ct.data.shape)  # (a dead slot's record is whatever was there)
            return ct.shape0.copy(), ct.env_count.copy(), np.where(live, ct.data.view(np.int32), 0)

        got = collide(True)
        _same(got, collide(False))
        assert got[1][0] > 0
    finally:
        em.image_handle.close()


def test_semi_implicit_and_featherstone_rollouts(H):
    from newton_amd import _lib as L

    em = _emu_model(H, _lowered_quadrupeds(19))
    try:
        def semi(image):
            a, b, ct, ctrl = H.EmuState(em), H.EmuState(em), H.EmuContacts(em), H.EmuControl(em)
            p, cp = L.nt_semi_implicit_params(0.05, 1.0, 1.0e4, 1.0e2), L.nt_collide_params(0, 0)
            d0, d1, dc, dct = a.desc(), b.desc(), ctrl.desc(), ct.desc()
            with _env(NT_TILE_IMAGE=None if image else "0"):
                H.check(H.lib().nt_semi_implicit_rollout(C.byref(em.desc), C.byref(p), C.byref(cp), C.byref(d0), C.byref(d1), C.byref(dc),
                                                         C.byref(dct), 1e-4, 4, None), "nt_semi_implicit_rollout")
            return a.body_q.copy(), a.body_qd.copy(), ct.shape0.copy(), ct.env_count.copy()

        def featherstone(image, epb=0):
            a, b, ct, ctrl = H.EmuState(em), H.EmuState(em), H.EmuContacts(em), H.EmuControl(em)
            with _env(NT_TILE_IMAGE=None if image else "0"):
                out = H.featherstone_rollout(em, a, b, ctrl, ct, 1e-3, 4, epb=epb)
            return out.body_q.copy(), out.body_qd.copy(), out.joint_q.copy(), out.joint_qd.copy(), ct.shape0.copy(), ct.env_count.copy()

        def featherstone_uniform_tile(image):
            # the uniform-parameter tile of 16: this solver's own tables sit behind the topology and its parameter copy behind those,
            # so it takes the image's topology part and loads the parameters itself
            return featherstone(image, epb=16)

        assert em.desc.params_uniform == 1
        for run in (semi, featherstone, featherstone_uniform_tile):
            got = run(True)
            _same(got, run(False))
            assert np.isfinite(got[0][:, :, :19]).all() and np.abs(got[1]).max() > 0.0
    finally:
        em.image_handle.close()


# ------------------------------------------------------------------------------------------------
# nt_model_refresh_params rewrites the image
# ------------------------------------------------------------------------------------------------
def _edit_heavier_everywhere(model):
    _heavier(model, 3, range(model.env.env_count))


def _edit_heavier_in_one_world(model):
    _heavier(model, 3, [5])


def _edit_last_joint_off(model):
    nj = model.env.nj
    model.joint_enabled = np.array(model.joint_enabled, copy=True)
    model.joint_enabled[nj - 1::nj] = False
    model.env.joint_enabled = np.asarray(model.joint_enabled, dtype=np.int32)[:nj].copy()  # (the template the emulated descriptor reads)


@pytest.mark.parametrize("edit", [_edit_heavier_everywhere, _edit_heavier_in_one_world, _edit_last_joint_off])
def test_refreshed_image_equals_a_freshly_created_models(H, edit):
    model = _lowered_quadrupeds(20)
    refreshed = _Handle(H, model)
    before = refreshed.image()
    edit(model)
    refreshed.refresh(model)
    fresh = _Handle(H, model)
    try:
        assert refreshed.d.tile_image_words == fresh.d.tile_image_words and refreshed.d.params_uniform == fresh.d.params_uniform
        assert np.array_equal(refreshed.image(), fresh.image())
        topo, params = _expected_image(model, model.env, H.EmuModel(model).desc)
        if edit is _edit_heavier_in_one_world:  # the uniform flag drops, the image loses its parameter block
            assert fresh.d.params_uniform == 0 and params is None and len(fresh.image()) == len(topo) < len(before)
        else:
            assert fresh.d.params_uniform == 1 and not np.array_equal(fresh.image(), before)
        if edit is _edit_last_joint_off:
            assert not np.array_equal(fresh.image()[:len(topo)], before[:len(topo)])
        # ... and the launches through the refreshed image give what the staged tables of the edited model give
        em = refreshed.attach(H.EmuModel(model))
        cfg = None if edit is _edit_heavier_in_one_world else "16,512,1,1,0,1"
        _same(_xpbd_rollout(H, em, cfg, True, substeps=3), _xpbd_rollout(H, em, cfg, False, substeps=3))
    finally:
        refreshed.close()
        fresh.close()
