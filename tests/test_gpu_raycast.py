"""newton_amd.sensors.SensorRaycast on the device (nt_raycast, include/newton_hip_mesh.h) against its float64 host path on the same fp32
inputs: parity on the scenes of tests/raycast_cases.py (37 worlds, 70 rays), in-place ray updates through a captured graph, a cast
after the stepper, outputs asked for one at a time; the closed forms of tests/raycast_known_answers.py, the layout scenes and the
launch shapes of raycast_cases.py (4 / 2 / 1 worlds per workgroup, a second ray per lane, dynamic LDS beyond 48 KB)."""
import numpy as np
import pytest

import raycast_cases as rc
import raycast_known_answers as known
import tolerances
from raycast_cases import CASES, DISTANCE_GATE, MAX_DISTANCE, N_WORLDS, NORMAL_GATE, case, compare, reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_GPU = {}


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _bits(x):
    return np.ascontiguousarray(_np(x)).view(np.uint32)


def _gpu_case(name, **extra):
    """(GPU model, its state, a SensorRaycast on it); the model and state are built once per scene."""
    from newton_amd import sensors

    make, rays, kw = CASES[name]
    if name not in _GPU:
        model = make(device=DEV)
        _GPU[name] = (model, model.state())
    model, state = _GPU[name]
    o, d, body = rays()
    return model, state, sensors.SensorRaycast(model, o, d, ray_body=body, max_distance=MAX_DISTANCE, **kw, **extra)


@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_the_host_reference(name):
    """SensorRaycast's own device tables (the layout scenes: a second heightfield record, a second mesh with its vertex, triangle and
    block starts and a scale per axis) give the reference's -- hence the emulator's -- hit / miss and shape ids on every clear ray."""
    import torch

    host_model, rays, kw, ref = case(name)
    model, state, s = _gpu_case(name)
    assert np.array_equal(np.asarray(model.body_q), np.asarray(host_model.body_q))
    s.distance.fill_(7.0), s.normal.fill_(7.0), s.shape.fill_(-7)
    before = _np(state.body_q).copy()
    s.eval(state)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(state.body_q), before.view(np.uint32))
    dist, normal, shape = _np(s.distance), _np(s.normal), _np(s.shape)
    assert not np.any(dist == 7.0) and not np.any(normal == 7.0) and not np.any(shape == -7)
    err_d, err_n = compare(ref, dist, normal, shape, f"gpu {name}")
    tolerances.record(f"raycast_{name}", {"distance_rel": {"max": err_d}, "normal_angle": {"max": err_n}},
                      {"distance_rel": DISTANCE_GATE, "normal_angle": NORMAL_GATE})
    assert err_d <= DISTANCE_GATE and err_n <= NORMAL_GATE
    # a world mask: the other rows keep what they hold
    mask = np.arange(model.env.env_count) % 3 != 1
    s.distance.fill_(7.0), s.normal.fill_(7.0), s.shape.fill_(-7)
    s.eval(state, world_mask=mask)
    torch.cuda.synchronize()
    for got, want in ((s.distance, dist), (s.normal, normal), (s.shape, shape)):
        got = _np(got)
        assert np.all(np.abs(got[~mask]) == 7) and np.array_equal(got[mask].view(np.uint32), want[mask].view(np.uint32))


@pytest.mark.parametrize("name", list(known.CASES))
def test_known_answers(name):
    """The closed forms of tests/raycast_known_answers.py on the device: hit / miss and shape id exact, distance and normal within the
    gates of the comparison scenes, measured against the closed form (not against another backend)."""
    import torch

    from newton_amd import sensors

    c = known.CASES[name]
    key = ("known", c["scene"])
    if key not in _GPU:
        model = known.SCENES[c["scene"]](device=DEV)
        _GPU[key] = (model, model.state())
    model, rest = _GPU[key]
    state = rest
    if c["pose"] is not None:
        state = model.state()
        state.body_q = c["pose"](model)
    o, d, body = c["rays"]
    s = sensors.SensorRaycast(model, o, d, ray_body=body, **c["kw"](model))
    s.distance.fill_(7.0), s.normal.fill_(7.0), s.shape.fill_(-7)
    s.eval(state)
    torch.cuda.synchronize()
    err_t, err_n = known.compare_known(c, model, _np(s.distance), _np(s.normal), _np(s.shape), t_rel=DISTANCE_GATE, n_angle=NORMAL_GATE, label=f"gpu {name}")
    tolerances.record(f"raycast_known_{name}", {"distance_rel": {"max": err_t}, "normal_angle": {"max": err_n}},
                      {"distance_rel": DISTANCE_GATE, "normal_angle": NORMAL_GATE})


# ---------------------------------------------------------------------------------------------------------------------------------
# launch shapes: 4 / 2 / 1 worlds per workgroup, a second ray per lane, dynamic LDS beyond 48 KB, the halving of wpb
# ---------------------------------------------------------------------------------------------------------------------------------
def _launch_run(extra, ray_count, mask=None):
    """P[:ray_count] against the launch scene with `extra` small spheres, through SensorRaycast's own tables: (host model,
    reference, distance, normal, shape), the outputs poisoned before the call."""
    import torch

    from newton_amd import sensors

    host_model, rays, ref = rc.launch_case(extra, ray_count)
    key = ("launch", extra)
    if key not in _GPU:
        model = rc.launch_model(extra, device=DEV)
        _GPU[key] = (model, model.state())
    model, state = _GPU[key]
    assert np.array_equal(np.asarray(model.body_q), np.asarray(host_model.body_q))
    o, d, body = rays
    s = sensors.SensorRaycast(model, o, d, ray_body=body, max_distance=MAX_DISTANCE)
    assert np.array_equal(s.slots, ref["slots"])
    s.distance.fill_(7.0), s.normal.fill_(7.0), s.shape.fill_(-7)
    s.eval(state, world_mask=mask)
    torch.cuda.synchronize()
    return host_model, ref, _np(s.distance).copy(), _np(s.normal).copy(), _np(s.shape).copy()


def _launch_full():
    """P, all 257 rays, against the eight bodies and the ground: compared with the host reference once, then shared."""
    if "launch_full" not in _GPU:
        model, ref, dist, normal, shape = _launch_run(0, rc.LAUNCH_RAYS)
        err_d, err_n = compare(ref, dist, normal, shape, "gpu launch R = 257")
        tolerances.record("raycast_launch_257", {"distance_rel": {"max": err_d}, "normal_angle": {"max": err_n}},
                          {"distance_rel": DISTANCE_GATE, "normal_angle": NORMAL_GATE})
        assert err_d <= DISTANCE_GATE and err_n <= NORMAL_GATE
        _GPU["launch_full"] = (dist, normal, shape)
    return _GPU["launch_full"]


def test_launch_constants_are_the_kernels():
    assert rc.kernel_constants() == (rc.RC_REC, rc.RC_THREADS, rc.RC_LDS_BYTES_PER_CU)


@pytest.mark.parametrize("R", rc.LAUNCH_PREFIXES)
def test_ray_count_prefixes_keep_every_bit(R):
    """P[:R] gives the first R columns of P's result bit for bit: 4 / 2 / 1 worlds per workgroup (64 / 128 / 256 lanes each), and the
    lanes' second ray at R = 257 -- the launch geometry does not change a bit."""
    full = _launch_full()
    K = len(rc.launch_case(0, R)[2]["slots"])
    assert K == 9 and rc.launch_shape(R, K)[:2] == ((4, 64) if R <= 64 else (2, 128) if R <= 128 else (1, 256))
    assert rc.launch_shape(257, K)[1] < 257
    got = _launch_run(0, R)[2:]
    for a, b in zip(got, full):
        assert np.array_equal(_bits(a), _bits(b[:, :R]))
    assert not np.any(got[0] == 7.0)


@pytest.mark.parametrize("name", list(rc.LAUNCH_TARGETS))
def test_many_targets_keep_every_bit(name):
    """64 rays against 309 / 909 targets: the staged records outgrow 48 KB with four worlds per workgroup (the dynamic LDS request
    goes through hipFuncSetAttribute), then force two worlds per workgroup.  Parity with the host reference, late targets are hit, and
    every ray that does not end on a small sphere has the bits it has at R = 257 against the nine shared targets."""
    R, extra, wpb, large = rc.LAUNCH_TARGETS[name]
    full = _launch_full()
    model, ref, dist, normal, shape = _launch_run(extra, R)
    K = len(ref["slots"])
    got_wpb, lanes, lds = rc.launch_shape(R, K)
    assert K == 9 + extra and got_wpb == wpb and (lds > rc.RC_DEFAULT_LDS) == large and lds <= rc.RC_LDS_BYTES_PER_CU
    assert rc.launch_shape(R, 9)[0] == 4 and (wpb == 4 or 2 * wpb * K * rc.RC_REC * 4 > rc.RC_LDS_BYTES_PER_CU)
    err_d, err_n = compare(ref, dist, normal, shape, f"gpu launch {name}")
    tolerances.record(f"raycast_launch_{name}", {"distance_rel": {"max": err_d}, "normal_angle": {"max": err_n}},
                      {"distance_rel": DISTANCE_GATE, "normal_angle": NORMAL_GATE})
    assert err_d <= DISTANCE_GATE and err_n <= NORMAL_GATE
    small = rc.small_sphere_ids(model)
    on_small = np.isin(shape, small)
    assert np.any(shape[ref["clear"]] == small[-1]) and np.any(on_small[:, 7]) and np.any(~on_small & (shape >= 0))
    for a, b in zip((dist, normal, shape), full):
        assert np.array_equal(_bits(a)[~on_small], _bits(b[:, :R])[~on_small])


def test_masked_worlds_inside_a_live_workgroup():
    """Worlds 1 and 4 off at R = 64: world 1 shares its workgroup with three live worlds.  Masked rows keep their poison, live rows
    the bits of the unmasked run."""
    full = _launch_full()
    mask = np.array([1, 0, 1, 1, 0], bool)
    assert rc.launch_shape(64, 9)[0] == 4
    got = _launch_run(0, 64, mask=mask)[2:]
    for a, b in zip(got, full):
        assert np.all(np.abs(a[~mask]) == 7) and np.array_equal(_bits(a[mask]), _bits(b[mask][:, :64]))


@pytest.mark.parametrize("backend", ["torch", "abi"])
def test_set_rays_in_place_and_graph_replay(backend):
    import torch

    import newton_amd as nt

    host_model, rays, kw, ref = case("hfield_scan")
    model, state, s = _gpu_case("hfield_scan")
    o, d, body = rays
    s.eval(state)
    torch.cuda.synchronize()
    direct = [_np(x).copy() for x in (s.distance, s.normal, s.shape)]
    g = nt.graph.capture(lambda: s.eval(state), warmup=1, backend=backend)
    s.distance.fill_(float("nan"))
    g.launch()
    torch.cuda.synchronize()
    assert all(np.array_equal(a.view(np.uint32), _bits(b)) for a, b in zip(direct, (s.distance, s.normal, s.shape)))
    # new rays written in place (the grid turned a quarter and moved): the replay casts them
    store = s.origins.data_ptr()
    o2 = (o[:, [1, 0, 2]] * np.array([-1.0, 1.0, 1.0]) + np.array([0.1, -0.05, 0.0])).astype(np.float32)
    s.set_rays(o2, d)
    assert s.origins.data_ptr() == store
    before = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]
    g.launch()
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats(DEV)["allocation.all.allocated"] == before
    ref2 = reference(host_model, host_model.body_q, (o2, d, body), **kw)
    err_d, err_n = compare(ref2, _np(s.distance), _np(s.normal), _np(s.shape), f"gpu hfield_scan replay ({backend})")
    assert err_d <= DISTANCE_GATE and err_n <= NORMAL_GATE
    assert not np.array_equal(_np(s.distance), direct[0])


def test_cast_after_six_xpbd_substeps():
    """The sensor reads the state the stepper left: the reference is the host path on the copied-back body_q."""
    import torch

    import newton_amd as nt
    from newton_amd import sensors

    make, rays, kw = CASES["terrain_scan"]
    model = make(device=DEV)
    pipe = nt.CollisionPipeline(model)
    contacts, solver = pipe.contacts(), nt.solvers.SolverXPBD(model, iterations=2)
    s0, s1, ctrl = model.state(), model.state(), model.control()
    solver.rollout(s0, s1, ctrl, contacts, 1e-3, 6)  # (even: the result is in s0)
    o, d, body = rays()
    s = sensors.SensorRaycast(model, o, d, ray_body=body, max_distance=MAX_DISTANCE, **kw)
    s.eval(s0)
    torch.cuda.synchronize()
    bq = _np(s0.body_q)
    assert not np.array_equal(bq, np.asarray(model.body_q))  # the bodies moved (the carrier falls)
    host_model = case("terrain_scan")[0]
    ref = reference(host_model, bq, (o, d, body), **kw)
    assert ref["clear"].mean() >= 0.9
    err_d, err_n = compare(ref, _np(s.distance), _np(s.normal), _np(s.shape), "gpu terrain_scan after 6 substeps")
    assert err_d <= DISTANCE_GATE and err_n <= NORMAL_GATE


def test_outputs_one_at_a_time_and_per_world_rays():
    import torch

    model, state, full = _gpu_case("primitives")
    full.eval(state)
    only_d = _gpu_case("primitives", want_normal=False, want_shape=False)[2]
    only_n = _gpu_case("primitives", want_shape=False)[2]
    only_s = _gpu_case("primitives", want_normal=False)[2]
    for s in (only_d, only_n, only_s):
        s.eval(state)
    torch.cuda.synchronize()
    assert only_d.normal is None and only_d.shape is None and only_n.shape is None and only_s.normal is None
    assert all(np.array_equal(_bits(s.distance), _bits(full.distance)) for s in (only_d, only_n, only_s))
    assert np.array_equal(_bits(only_n.normal), _bits(full.normal)) and np.array_equal(_bits(only_s.shape), _bits(full.shape))
    # the pattern expanded per world: the same bits
    from newton_amd import sensors

    o, d, body = CASES["primitives"][1]()
    pw = sensors.SensorRaycast(model, np.tile(o, (N_WORLDS, 1, 1)), np.tile(d, (N_WORLDS, 1, 1)), ray_body=body, max_distance=MAX_DISTANCE)
    pw.eval(state)
    torch.cuda.synchronize()
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in ((pw.distance, full.distance), (pw.normal, full.normal), (pw.shape, full.shape)))


def test_unsupported_target_is_refused_before_any_launch():
    import newton_amd as nt
    from newton_amd import sensors

    env = nt.ModelBuilder()
    b = env.add_body(xform=[0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0])
    env.add_shape_convex_hull(b, mesh=nt.Mesh.create_box(0.1, 0.1, 0.1))
    scene = nt.ModelBuilder()
    scene.replicate(env, 3)
    scene.add_ground_plane()
    model = scene.finalize(device=DEV)
    with pytest.raises(NotImplementedError, match="CONVEX_MESH"):
        sensors.SensorRaycast(model, np.zeros((1, 3)), np.ones((1, 3)))
    s = sensors.SensorRaycast(model, [[0.0, 0.0, 2.0]], [[0.0, 0.0, -1.0]], exclude_bodies=(0,))
    # the C entry point refuses the type too (the host table names it)
    s._targets_host[0, 1] = int(nt.GeoType.CONVEX_MESH)
    s.distance.fill_(7.0)
    with pytest.raises(NotImplementedError, match="NT_ERR_UNSUPPORTED"):
        s.eval(model.state())
    assert np.all(_np(s.distance) == 7.0)
