"""raycast_kernel (nt_raycast, include/newton_hip_mesh.h) on the emulator: the kernel SOURCES executed on the CPU (tests/emu), without a
GPU, against the float64 host path of newton_amd.sensors on identical fp32 inputs.  37 worlds (not a multiple of any tile), 70 rays (two
waves, the second partial: two worlds per workgroup), scenes and comparison rule of tests/raycast_cases.py; the closed forms of
tests/raycast_known_answers.py; the layout scenes (5 worlds) and the launch shapes of raycast_cases.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import raycast_known_answers as known  # noqa: E402
import tolerances  # noqa: E402
import raycast_cases as rc  # noqa: E402
from raycast_cases import CASES, DISTANCE_GATE, MAX_DISTANCE, N_WORLDS, NORMAL_GATE, HostArgs, case, compare, emu_cast  # noqa: E402
from newton_amd.enums import GeoType  # noqa: E402


@pytest.fixture(scope="module")
def H(oracle_lib):
    import harness

    harness.lib()  # builds tests/emu/_build/libnewton_emu.so on first use
    return harness


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _run(H, model, rays, slots, **kw):
    em = H.EmuModel(model)
    state = H.EmuState(em)
    before = state.body_q.copy()
    args = HostArgs(model, rays, slots, **kw)
    H.check(emu_cast(H, em, state, args), "nt_raycast")
    assert np.array_equal(_bits(state.body_q), _bits(before))  # body_q is only read
    return args


@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_the_host_reference(H, name):
    model, rays, kw, ref = case(name)
    args = _run(H, model, rays, ref["slots"])
    assert not np.any(args.distance == 7.0) and not np.any(args.normal == 7.0) and not np.any(args.shape == -7)  # every row was written
    err_d, err_n = compare(ref, args.distance, args.normal, args.shape, f"emu {name}")
    tolerances.record(f"raycast_emu_{name}", {"distance_rel": {"max": err_d}, "normal_angle": {"max": err_n}},
                      {"distance_rel": DISTANCE_GATE, "normal_angle": NORMAL_GATE})
    assert err_d <= DISTANCE_GATE and err_n <= NORMAL_GATE


_KNOWN_MODELS = {}


@pytest.mark.parametrize("name", list(known.CASES))
def test_known_answers(H, name):
    """The closed forms of tests/raycast_known_answers.py on the kernel: hit / miss and shape id exact, distance and normal within the
    gates of the comparison scenes, measured against the closed form."""
    from newton_amd import sensors

    c = known.CASES[name]
    if c["scene"] not in _KNOWN_MODELS:
        _KNOWN_MODELS[c["scene"]] = known.SCENES[c["scene"]]()
    model = _KNOWN_MODELS[c["scene"]]
    o, d, body = c["rays"]
    kw = c["kw"](model)
    s = sensors.SensorRaycast(model, o, d, ray_body=body, **kw)  # (the host sensor: for the slot list and max_distance)
    em = H.EmuModel(model)
    state = H.EmuState(em, body_q=None if c["pose"] is None else c["pose"](model))
    args = HostArgs(model, c["rays"], s.slots, max_distance=s.max_distance)
    H.check(emu_cast(H, em, state, args), "nt_raycast")
    err_t, err_n = known.compare_known(c, model, args.distance, args.normal, args.shape, t_rel=DISTANCE_GATE, n_angle=NORMAL_GATE, label=f"emu {name}")
    tolerances.record(f"raycast_known_emu_{name}", {"distance_rel": {"max": err_t}, "normal_angle": {"max": err_n}},
                      {"distance_rel": DISTANCE_GATE, "normal_angle": NORMAL_GATE})


def test_world_mask_leaves_unselected_worlds_untouched(H):
    model, rays, kw, ref = case("primitives")
    full = _run(H, model, rays, ref["slots"])
    mask = (np.arange(N_WORLDS) % 3 != 1)
    em = H.EmuModel(model)
    args = HostArgs(model, rays, ref["slots"])
    args.set_world_mask(mask)
    H.check(emu_cast(H, em, H.EmuState(em), args), "nt_raycast")
    for got, want in ((args.distance, full.distance), (args.normal, full.normal), (args.shape, full.shape)):
        assert np.all(np.abs(got[~mask]) == 7) and np.array_equal(_bits(got[mask]), _bits(want[mask]))


@pytest.mark.parametrize("name", ["primitives", "terrain_scan", "hfield_scan"])
def test_replicated_worlds_give_equal_rows(H, name):
    make, rays, kw = CASES[name]
    model = make(jitter=False)
    ref_slots = case(name)[3]["slots"]
    args = _run(H, model, rays(), ref_slots)
    assert np.any(args.distance[0] >= 0.0)
    # (ids of env-local shapes differ by world * ns)
    local = (args.shape >= model.env.shape_local0) & (args.shape < model.env.shape_local0 + N_WORLDS * model.env.ns)
    rel = np.where(local, args.shape - np.arange(N_WORLDS)[:, None] * model.env.ns, args.shape)
    for a in (args.distance, args.normal, rel):
        assert np.all(_bits(a) == _bits(a[:1]))


@pytest.mark.parametrize("name", ["primitives", "hfield_skim"])
def test_shared_pattern_equals_the_pattern_expanded_per_world(H, name):
    model, rays, kw, ref = case(name)
    a, b = _run(H, model, rays, ref["slots"]), _run(H, model, rays, ref["slots"], per_world=True)
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in ((a.distance, b.distance), (a.normal, b.normal), (a.shape, b.shape)))


@pytest.mark.parametrize("name", ["terrain_scan", "terrain_skim", "mesh_two"])
def test_block_skip_keeps_every_bit(H, name):
    model, rays, kw, ref = case(name)
    a, b = _run(H, model, rays, ref["slots"]), _run(H, model, rays, ref["slots"], block_bounds=False)
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in ((a.distance, b.distance), (a.normal, b.normal), (a.shape, b.shape)))


def test_optional_outputs_and_many_rays_per_lane(H):
    """Outputs asked for one at a time equal the full call; 300 rays per world (one world per workgroup, lanes take two rays)."""
    model, rays, kw, ref = case("primitives")
    full = _run(H, model, rays, ref["slots"])
    only_d = _run(H, model, rays, ref["slots"], want_normal=False, want_shape=False)
    only_n = _run(H, model, rays, ref["slots"], want_shape=False)
    assert np.array_equal(_bits(only_d.distance), _bits(full.distance)) and np.array_equal(_bits(only_n.normal), _bits(full.normal))
    o, d, body = rays
    reps = 5
    many = (np.tile(o, (reps, 1))[:300], np.tile(d, (reps, 1))[:300], np.tile(body, reps)[:300])
    big = _run(H, model, many, ref["slots"])
    for k in range(0, 300, 70):
        n = min(70, 300 - k)
        assert np.array_equal(_bits(big.distance[:, k:k + n]), _bits(full.distance[:, :n]))
        assert np.array_equal(big.shape[:, k:k + n], full.shape[:, :n])


# ---------------------------------------------------------------------------------------------------------------------------------
# launch shapes: 4 / 2 / 1 worlds per workgroup, a second ray per lane, dynamic LDS beyond 48 KB, the halving of wpb
# ---------------------------------------------------------------------------------------------------------------------------------
_FULL = {}


def _launch_run(H, extra, ray_count, mask=None):
    model, rays, ref = rc.launch_case(extra, ray_count)
    em = H.EmuModel(model)
    args = HostArgs(model, rays, ref["slots"])
    if mask is not None:
        args.set_world_mask(mask)
    H.check(emu_cast(H, em, H.EmuState(em), args), "nt_raycast")
    return model, ref, args


def _launch_full(H):
    """P, all 257 rays, against the eight bodies and the ground: compared with the host reference once, then shared."""
    if "full" not in _FULL:
        model, ref, args = _launch_run(H, 0, rc.LAUNCH_RAYS)
        err_d, err_n = compare(ref, args.distance, args.normal, args.shape, "emu launch R = 257")
        assert err_d <= DISTANCE_GATE and err_n <= NORMAL_GATE
        _FULL["full"] = args
    return _FULL["full"]


def test_launch_constants_are_the_kernels():
    assert rc.kernel_constants() == (rc.RC_REC, rc.RC_THREADS, rc.RC_LDS_BYTES_PER_CU)


@pytest.mark.parametrize("R", rc.LAUNCH_PREFIXES)
def test_ray_count_prefixes_keep_every_bit(H, R):
    """P[:R] gives the first R columns of P's result bit for bit: 4 / 2 / 1 worlds per workgroup (64 / 128 / 256 lanes each), and the
    lanes' second ray at R = 257."""
    full = _launch_full(H)
    K = len(rc.launch_case(0, R)[2]["slots"])
    assert K == 9 and rc.launch_shape(R, K)[:2] == ((4, 64) if R <= 64 else (2, 128) if R <= 128 else (1, 256))
    assert rc.launch_shape(257, K)[1] < 257  # a lane of the widest shape takes ray 256 after ray 0
    model, ref, args = _launch_run(H, 0, R)
    for got, want in ((args.distance, full.distance), (args.normal, full.normal), (args.shape, full.shape)):
        assert np.array_equal(_bits(got), _bits(want[:, :R]))
    assert not np.any(args.distance == 7.0)


@pytest.mark.parametrize("name", list(rc.LAUNCH_TARGETS))
def test_many_targets_keep_every_bit(H, name):
    """64 rays against 309 / 909 targets: the staged records outgrow 48 KB with four worlds per workgroup, then force two worlds per
    workgroup.  Parity with the host reference, late targets are hit, and every ray that does not end on a small sphere has
    the bits it has at R = 257 against the nine shared targets."""
    R, extra, wpb, large = rc.LAUNCH_TARGETS[name]
    full = _launch_full(H)
    model, ref, args = _launch_run(H, extra, R)
    K = len(ref["slots"])
    got_wpb, lanes, lds = rc.launch_shape(R, K)
    assert K == 9 + extra and got_wpb == wpb and (lds > rc.RC_DEFAULT_LDS) == large and lds <= rc.RC_LDS_BYTES_PER_CU
    assert rc.launch_shape(R, 9)[0] == 4 and (wpb == 4 or 2 * wpb * K * rc.RC_REC * 4 > rc.RC_LDS_BYTES_PER_CU)
    err_d, err_n = compare(ref, args.distance, args.normal, args.shape, f"emu launch {name}")
    assert err_d <= DISTANCE_GATE and err_n <= NORMAL_GATE
    small = rc.small_sphere_ids(model)
    on_small = np.isin(args.shape, small)
    assert np.any(args.shape[ref["clear"]] == small[-1]) and np.any(on_small[:, 7]) and np.any(~on_small & (args.shape >= 0))
    for got, want in ((args.distance, full.distance), (args.normal, full.normal), (args.shape, full.shape)):
        assert np.array_equal(_bits(got)[~on_small], _bits(want[:, :R])[~on_small])


def test_masked_worlds_inside_a_live_workgroup(H):
    """Worlds 1 and 4 off at R = 64: world 1 shares its workgroup with three live worlds.  Masked rows keep their poison, live rows
    the bits of the unmasked run."""
    full = _launch_full(H)
    mask = np.array([1, 0, 1, 1, 0], bool)
    assert rc.launch_shape(64, 9)[0] == 4
    model, ref, args = _launch_run(H, 0, 64, mask=mask)
    for got, want in ((args.distance, full.distance), (args.normal, full.normal), (args.shape, full.shape)):
        assert np.all(np.abs(got[~mask]) == 7) and np.array_equal(_bits(got[mask]), _bits(want[mask][:, :64]))


def test_errors(H):
    model, rays, kw, ref = case("primitives")
    em = H.EmuModel(model)
    state = H.EmuState(em)
    lib = H.lib()
    d = state.desc()
    args = HostArgs(model, rays, ref["slots"])
    assert lib.nt_raycast(None, C.byref(d), C.byref(args.desc), None) == -1
    assert lib.nt_raycast(C.byref(em.desc), C.byref(d), None, None) == -1
    saved, args.desc.distance = args.desc.distance, None
    assert emu_cast(H, em, state, args) == -1
    args.desc.distance = saved
    saved, args.desc.ray_count = args.desc.ray_count, 0
    assert emu_cast(H, em, state, args) == -1
    args.desc.ray_count = saved
    # an unsupported type in the (host) target table: refused before any launch, the outputs keep their poison
    table = args.keep["targets"]
    kept = table[0, 1]
    for bad in (int(GeoType.CONVEX_MESH), int(GeoType.GAUSSIAN), 0):
        table[0, 1] = bad
        assert emu_cast(H, em, state, args) == -3
    table[0, 1] = kept
    table[[0, 1]] = table[[1, 0]]  # not ascending
    assert emu_cast(H, em, state, args) == -1
    table[[0, 1]] = table[[1, 0]]
    assert np.all(args.distance == 7.0)
    # a mesh target without its tables
    model, rays, kw, ref = case("terrain_scan")
    em = H.EmuModel(model)
    args = HostArgs(model, rays, ref["slots"])
    args.desc.vertices = None
    assert emu_cast(H, em, H.EmuState(em), args) == -1
    # more staged targets than the LDS of a CU holds (48 B each): refused from the count alone
    args = HostArgs(model, rays, ref["slots"])
    n = 160 * 1024 // 48 + 1
    big = np.zeros((n, 2), np.int32)
    args.desc.target_count, args.desc.targets, args.desc.targets_host = n, big.ctypes.data, big.ctypes.data
    assert emu_cast(H, em, H.EmuState(em), args) in (-1, -3)  # (the table is not ascending either: whichever check comes first)
