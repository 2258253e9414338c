"""SolverFeatherstone(update_mass_matrix_interval > 1) with SEVERAL articulations per world, on the emulated kernels (tests/emu).

Between rebuilds the factor of H lives in a caller-owned buffer documented as [nd * max_art_dofs][env_stride].  With one articulation
per world (every earlier test of this path) max_art_dofs == nd and any row bound up to nd (nd + 1) / 2 fits; with na > 1 the tree
mode's packed triangles end at sum_k n_k (n_k + 1) / 2 <= nd * max_art_dofs while the old bound nd (nd + 1) / 2 runs past the
buffer.  Every launch here gets a cache with sentinel-filled guard rows behind the documented ones, so a wrong bound lands in memory
the test owns, and the stale-factor steps are compared with the oracle's (its cache is the reference solver's dense L per
articulation) on scenes where a stale factor measurably differs from a fresh one.

19 worlds: no multiple of 4, 8 or 16, so the last workgroup of every tile width has idle environments."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

from test_gpu_parity_xpbd import _rel  # noqa: E402  (the gates below are test_free_bodies_single_step's, in its metric)

N_ENV, DT, INTERVAL = 19, 2e-3, 3
SENTINEL = np.float32(-1.2345e30)
FIELDS = ("joint_q", "joint_qd", "body_q", "body_qd")
GATES = {"joint_q": 1e-5, "body_q": 1e-5, "joint_qd": 1e-4, "body_qd": 1e-4}  # test_free_bodies_single_step
SENSITIVITY = 50.0  # a scene can show a stale factor when the oracle's own interval-1 and interval-k results are this many gates apart


@pytest.fixture(scope="module")
def H(oracle_lib):
    import harness

    harness.lib()
    return harness


@functools.lru_cache(maxsize=None)
def scene(name):
    from scenes import multi_articulation_scene, quadruped_scene

    if name == "quadruped":
        return quadruped_scene(2)
    return multi_articulation_scene(N_ENV, variant=name)


@functools.lru_cache(maxsize=None)
def emu_model(name):
    import harness

    return harness.EmuModel(scene(name))


def used_rows(t, dense):
    """Rows of the cache a launch may touch: dense nd W; tree the packed lower triangles of the articulations."""
    if dense:
        return t.nd * t.max_art_dofs
    qd_start = [int(t.joint_qd_start[int(j)]) for j in t.art_start[:t.na]] + [t.nd]
    return sum((b - a) * (b - a + 1) // 2 for a, b in zip(qd_start[:-1], qd_start[1:]))


def factor_rows(t, dense):
    """Rows of the cache that hold entries of the factor, for models whose articulations are single dof chains (every scene of
    multi_articulation_scene): tree all rows of the packed triangles; dense row d W + jl for jl <= d's index in its articulation --
    the kernels never write the upper triangle of the [nd][W] region, so those rows carry whatever the LDS held (on the emulator
    the same bytes in every run, on a device not)."""
    if not dense:
        return np.arange(used_rows(t, False))
    qd_start = [int(t.joint_qd_start[int(j)]) for j in t.art_start[:t.na]] + [t.nd]
    return np.array([d * t.max_art_dofs + jl for a, b in zip(qd_start[:-1], qd_start[1:]) for d in range(a, b) for jl in range(d - a + 1)])


def guard_cache(t):
    """The documented [nd W][ES] rows, the rows the old tree bound reached and 8 more, every element a sentinel."""
    rows = max(t.nd * t.max_art_dofs, t.nd * (t.nd + 1) // 2) + 8
    return np.full((rows, t.env_stride), SENTINEL, dtype=np.float32)


def check_guard(big, t, dense):
    touched = big != SENTINEL
    doc = t.nd * t.max_art_dofs
    rows = np.flatnonzero(touched.any(axis=1))
    assert rows.size, "the launch never wrote the cache"
    highest = int(rows.max())
    assert not touched[doc:].any(), f"rows behind the documented {doc} were written: highest touched row {highest}"
    assert not touched[:, t.env_count:].any(), "columns of environments that do not exist were written"
    assert highest == used_rows(t, dense) - 1, (highest, used_rows(t, dense))


@functools.lru_cache(maxsize=None)
def oracle_run(name, steps, interval, forced=()):
    """Open loop {clear body_f; collide; step; swap} on the oracle; forced: the steps whose factor is rebuilt out of cadence."""
    from oracle_bridge import Oracle, OracleState

    model = scene(name)
    o = Oracle(model)
    os0, os1, oc, c = OracleState(model), OracleState(model), o.contacts(), o.control()
    for k in range(steps):
        os0.body_f[:] = 0
        o.collide(os0.body_q, oc)
        o.featherstone_step(os0, os1, c, oc, DT, update_mass_matrix_interval=interval, force_update=k in forced)
        os0, os1 = os1, os0
    out = {f: getattr(os0, f).copy() for f in FIELDS}
    for v in out.values():
        v.flags.writeable = False
    return out


def assert_sensitive(name, fresh, stale, what):
    """The scene must be able to show a wrong factor: the oracle's own two results lie >= 50 gates apart in every gated field."""
    ratios = {f: _rel(fresh[f], stale[f]) / GATES[f] for f in FIELDS}
    print(f"[sensitivity] {name} {what}: " + ", ".join(f"{f} {r:.0f}x gate" for f, r in ratios.items()))
    for f, r in ratios.items():
        assert r >= SENSITIVITY, (name, what, f, r)


def emu_loop(H, em, steps, dense, epb, cache, forced=(), start=0, states=None):
    ctrl, ct = H.EmuControl(em), H.EmuContacts(em)
    a, b = states if states is not None else (H.EmuState(em), H.EmuState(em))
    for k in range(steps):
        a.body_f[:] = 0
        H.collide(em, a, ct)
        H.featherstone_step(em, a, b, ctrl, ct, DT, epb=epb, dense=dense, update_mass_matrix_interval=INTERVAL, step_index=start + k,
                            force_update=k in forced, cache=cache)
        a, b = b, a
    return a, b


@functools.lru_cache(maxsize=None)
def emu_open_loop(name, dense, epb):
    """7 steps at interval 3 (rebuilds at 0, 3, 6) behind a guard cache."""
    import harness as H

    em = emu_model(name)
    big = guard_cache(em.t)
    out, _ = emu_loop(H, em, 7, dense, epb, big)
    check_guard(big, em.t, dense)
    return {f: out.aos(f) for f in FIELDS}


@pytest.mark.parametrize("dense", [False, True], ids=["tree", "dense"])
@pytest.mark.parametrize("name", ["mixed", "free3", "quadruped"])
def test_cache_writes_stay_inside_the_documented_rows(H, name, dense):
    """4 steps at interval 3 (save at steps 0 and 3, reload at 1 and 2).  The highest row written is the end of the last articulation's
    packed triangle in tree mode -- 44 of 84 documented rows on "mixed", 62 of 108 on "free3", 170 of 324 on the quadruped, whose 117
    non-zero entries end there too: copying "the first nnz rows" would stop short -- and nd W - 1 in dense mode."""
    em = emu_model(name)
    t = em.t
    assert {"mixed": (3, 14, 6, 45), "free3": (3, 18, 6, 63), "quadruped": (1, 18, 18, 171)}[name] == \
        (t.na, t.nd, t.max_art_dofs, used_rows(t, False))
    big = guard_cache(t)
    emu_loop(H, em, 4, dense, 0, big)
    check_guard(big, t, dense)


@pytest.mark.parametrize("epb", [0, 1, 4, 8, 16])
@pytest.mark.parametrize("dense", [False, True], ids=["tree", "dense"])
@pytest.mark.parametrize("name", ["mixed", "free3"])
def test_stale_factor_steps_match_the_oracle(H, name, dense, epb):
    """7 open-loop steps at interval 3 vs the oracle at interval 3.  Emulator and oracle run the same x86 arithmetic without
    contraction: the dense order is the oracle's, bit for bit; the tree order measured 1.9e-7 (joint_q) and 3.3e-5 (joint_qd) here and is
    held to test_free_bodies_single_step's gates."""
    want = oracle_run(name, 7, INTERVAL)
    assert_sensitive(name, oracle_run(name, 7, 1), want, "interval 1 vs 3, 7 steps")
    got = emu_open_loop(name, dense, epb)
    for f in FIELDS:
        if dense:
            assert np.array_equal(got[f], want[f]), (f, _rel(got[f], want[f]))
        else:
            assert _rel(got[f], want[f]) <= GATES[f], (f, _rel(got[f], want[f]))


@pytest.mark.parametrize("name", ["mixed", "free3"])
def test_tree_mode_is_bitwise_the_same_at_every_tile_width(H, name):
    ref = emu_open_loop(name, False, 0)
    for epb in (1, 4, 8, 16):
        other = emu_open_loop(name, False, epb)
        for f in FIELDS:
            assert np.array_equal(ref[f], other[f]), (epb, f)


@pytest.mark.parametrize("epb", [0, 1, 8, 16])
@pytest.mark.parametrize("dense", [False, True], ids=["tree", "dense"])
@pytest.mark.parametrize("name", ["mixed", "free3"])
def test_fused_rollout_is_the_step_loop_across_two_calls(H, name, dense, epb):
    """rollout(7) + rollout(4, step_index = 7) == 11 launches of {clear body_f; collide; step; swap}, bit for bit: the cadence runs on
    step_index + substep, so the second call reloads at its substeps 0 and 1 what the first saved at its substep 6."""
    em = emu_model(name)
    if epb == 16 and not dense:  # the uniform-parameter tile of 16 (512 lanes) needs these
        assert em.desc.params_uniform == 1 and em.desc.np_analytic == em.desc.np
    big = guard_cache(em.t)
    ctrl, ct = H.EmuControl(em), H.EmuContacts(em)
    kw = dict(epb=epb, dense=dense, update_mass_matrix_interval=INTERVAL, cache=big)
    s0, s1 = H.EmuState(em), H.EmuState(em)
    out = H.featherstone_rollout(em, s0, s1, ctrl, ct, DT, 7, step_index=0, **kw)
    assert out is s1
    out = H.featherstone_rollout(em, s1, s0, ctrl, ct, DT, 4, step_index=7, **kw)
    assert out is s1
    check_guard(big, em.t, dense)
    big_loop = guard_cache(em.t)
    want, _ = emu_loop(H, em, 11, dense, epb, big_loop)
    check_guard(big_loop, em.t, dense)
    for f in FIELDS:
        assert np.array_equal(getattr(out, f), getattr(want, f)), f
    assert np.array_equal(big, big_loop)


@pytest.mark.parametrize("dense", [False, True], ids=["tree", "dense"])
def test_forced_refresh_matches_the_oracle_and_only_forces_the_first_substep(H, dense):
    """force_update (the reference's _mass_matrix_dirty) at steps 1 and 5 of 6 on "mixed", vs the oracle forced at the same steps;
    then a rollout of 4 substeps from step_index 1 with force_update set: substep 0 rebuilds, 1 reloads, 2 rebuilds by cadence,
    3 reloads -- the loop with only step 1 forced, bit for bit."""
    name, forced = "mixed", (1, 5)
    want = oracle_run(name, 6, INTERVAL, forced)
    assert_sensitive(name, want, oracle_run(name, 6, INTERVAL), "forced at steps 1 and 5 vs unforced, 6 steps")
    em = emu_model(name)
    big = guard_cache(em.t)
    out, _ = emu_loop(H, em, 6, dense, 0, big, forced=forced)
    check_guard(big, em.t, dense)
    for f in FIELDS:
        if dense:
            assert np.array_equal(out.aos(f), want[f]), (f, _rel(out.aos(f), want[f]))
        else:
            assert _rel(out.aos(f), want[f]) <= GATES[f], (f, _rel(out.aos(f), want[f]))

    big_loop, big_roll = guard_cache(em.t), guard_cache(em.t)
    a, b = emu_loop(H, em, 1, dense, 0, big_loop)  # step 0, then fork
    big_roll[:] = big_loop
    r0, r1 = H.EmuState(em), H.EmuState(em)
    for f in FIELDS:
        getattr(r0, f)[:] = getattr(a, f)
        getattr(r1, f)[:] = getattr(b, f)
    res = H.featherstone_rollout(em, r0, r1, H.EmuControl(em), H.EmuContacts(em), DT, 4, dense=dense,
                                 update_mass_matrix_interval=INTERVAL, step_index=1, force_update=True, cache=big_roll)
    loop, _ = emu_loop(H, em, 4, dense, 0, big_loop, forced=(0,), start=1, states=(a, b))
    unforced_cache = guard_cache(em.t)
    u, ub = emu_loop(H, em, 1, dense, 0, unforced_cache)
    unforced, _ = emu_loop(H, em, 4, dense, 0, unforced_cache, start=1, states=(u, ub))
    for f in FIELDS:
        assert np.array_equal(getattr(res, f), getattr(loop, f)), f
    assert np.array_equal(big_roll, big_loop)
    assert not np.array_equal(loop.joint_qd, unforced.joint_qd)  # (the flag did something)
    check_guard(big_roll, em.t, dense)
