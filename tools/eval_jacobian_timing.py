#!/usr/bin/env python
"""MEASUREMENT TOOL -- nt_eval_jacobian, nt_eval_mass_matrix, nt_eval_inverse_dynamics and nt_eval_forward_dynamics beside nt_eval_fk and
nt_eval_ik on the same model, same process.

    python tools/eval_jacobian_timing.py [--worlds 4096] [--calls 40] [--repeats 7] [--warmup 20] [--peak-gbs X] [--out FILE]

Quadruped scene, outputs in caller tensors.  One HIP event pair around a batch of `--calls` back-to-back launches of one kernel gives a
per-call time; the kernels take turns batch by batch, `--repeats` (>= 5) batches each; the median and the spread (min .. max) of the
batches are reported.  Beside each call stand the bytes it must write (J: worlds * 6 L * D * 4; H: worlds * D * D * 4; tau:
worlds * D * 4; joint_qdd and info: worlds * (D + 1) * 4) and read (body_q, joint_q; inverse dynamics: joint_qd and joint_qdd too;
forward dynamics: joint_qd, joint_f and body_f -- all three flags are on), the time those bytes take at the streaming
peak (`--peak-gbs`: what `bench.py --full` prints for this box; default: a device-to-device copy measured here, read + write counted)
and the ratio of the measured time to that floor.  Prints ONE JSON line and writes it to --out (default
profiles/eval_jacobian_timing.json; the run with the inverse-dynamics row is profiles/eval_inverse_dynamics_timing.json, the one with
the forward-dynamics row profiles/eval_forward_dynamics_timing.json)."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def copy_peak_gbs():
    """Device-to-device copy of 256 MB: bytes read + written per second."""
    import numpy as np
    import torch

    a = torch.empty(64 * 1024 * 1024, dtype=torch.float32, device="cuda:0")
    b = torch.empty_like(a)
    for _ in range(3):
        b.copy_(a)
    rates = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        rates.append(2 * a.numel() * 4 / (e0.elapsed_time(e1) * 1e-3) / 1e9)
    return float(np.median(rates))


def measure(worlds, calls, repeats, warmup, peak_gbs):
    import numpy as np
    import torch

    import scenes
    from newton_amd import _lib
    from newton_amd.state import pack_soa

    model = scenes.quadruped_scene(worlds, device="cuda:0")
    t, dm = model.env, model.device_model()
    lib = dm.lib
    rng = np.random.default_rng(0)
    jq = np.asarray(model.joint_q, dtype=np.float32).copy()
    jq.reshape(worlds, -1)[:, 7:] += rng.uniform(-0.5, 0.5, size=(worlds, t.nc - 7)).astype(np.float32)
    jqd = rng.normal(0, 1.0, size=model.joint_dof_count).astype(np.float32)
    src_q, src_qd = pack_soa(model, jq, 1, t.nc), pack_soa(model, jqd, 1, t.nd)
    state = model.state()
    state.joint_q, state.joint_qd = jq, jqd
    state.body_f = np.concatenate([rng.uniform(-20.0, 20.0, size=(model.body_count, 3)), rng.uniform(-2.0, 2.0, size=(model.body_count, 3))],
                                  axis=1).astype(np.float32)
    d = state._desc()
    out_q, out_qd = torch.zeros_like(src_q), torch.zeros_like(src_qd)
    L, D = model.max_joints_per_articulation, model.max_dofs_per_articulation
    J = torch.zeros((worlds * t.na, 6 * L, D), dtype=torch.float32, device="cuda:0")
    H = torch.zeros((worlds * t.na, D, D), dtype=torch.float32, device="cuda:0")
    tau = torch.zeros((worlds * t.na, D), dtype=torch.float32, device="cuda:0")
    qdd = torch.from_numpy(rng.uniform(-5.0, 5.0, size=(worlds * t.na, D)).astype(np.float32)).to("cuda:0")
    joint_f = torch.from_numpy(rng.uniform(-10.0, 10.0, size=(worlds * t.na, D)).astype(np.float32)).to("cuda:0")
    fd_qdd, fd_info = torch.zeros_like(tau), torch.zeros(worlds * t.na, dtype=torch.int32, device="cuda:0")
    m, s, st = C.byref(dm.desc), C.byref(d), dm.stream()
    legs = {
        "eval_fk": lambda: _lib.check(lib.nt_eval_fk(m, src_q.data_ptr(), src_qd.data_ptr(), s, st), "nt_eval_fk"),
        "eval_ik": lambda: _lib.check(lib.nt_eval_ik(m, s, out_q.data_ptr(), out_qd.data_ptr(), None, st), "nt_eval_ik"),
        "eval_jacobian": lambda: _lib.check(lib.nt_eval_jacobian(m, s, J.data_ptr(), None, None, st), "nt_eval_jacobian"),
        "eval_mass_matrix": lambda: _lib.check(lib.nt_eval_mass_matrix(m, s, H.data_ptr(), None, None, st), "nt_eval_mass_matrix"),
        "eval_inverse_dynamics": lambda: _lib.check(lib.nt_eval_inverse_dynamics(m, s, qdd.data_ptr(), 3, tau.data_ptr(), None, st),
                                                    "nt_eval_inverse_dynamics"),
        "eval_forward_dynamics": lambda: _lib.check(lib.nt_eval_forward_dynamics(m, s, joint_f.data_ptr(), 7, fd_qdd.data_ptr(),
                                                                                 fd_info.data_ptr(), None, st), "nt_eval_forward_dynamics"),
    }
    state_bytes = worlds * 4 * (7 * t.nb + t.nc)
    traffic = {"eval_fk": (worlds * 4 * (t.nc + t.nd), worlds * 52 * t.nb), "eval_ik": (worlds * 52 * t.nb, worlds * 4 * (t.nc + t.nd)),
               "eval_jacobian": (state_bytes, J.numel() * 4), "eval_mass_matrix": (state_bytes, H.numel() * 4),
               "eval_inverse_dynamics": (state_bytes + worlds * 4 * t.nd + qdd.numel() * 4, tau.numel() * 4),
               "eval_forward_dynamics": (state_bytes + worlds * 4 * (t.nd + 6 * t.nb) + joint_f.numel() * 4, (fd_qdd.numel() + fd_info.numel()) * 4)}
    for _ in range(warmup):
        for f in legs.values():
            f()
    torch.cuda.synchronize()
    per_call = {n: [] for n in legs}
    for _ in range(repeats):
        for n, f in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                f()
            e1.record()
            torch.cuda.synchronize()
            per_call[n].append(e0.elapsed_time(e1) * 1e3 / calls)
    out = {"worlds": worlds, "calls_per_batch": calls, "batches": repeats, "warmup_calls": warmup, "L": L, "D": D,
           "params_uniform": int(dm.desc.params_uniform), "streaming_peak_gbytes_per_s": round(peak_gbs, 1)}
    for n, us in per_call.items():
        us = np.array(us)
        rd, wr = traffic[n]
        floor_us = (rd + wr) / (peak_gbs * 1e9) * 1e6
        out[n] = {"us_median": round(float(np.median(us)), 3), "us_min": round(float(us.min()), 3), "us_max": round(float(us.max()), 3),
                  "bytes_read": int(rd), "bytes_written": int(wr), "traffic_floor_us": round(floor_us, 3),
                  "time_over_traffic_floor": round(float(np.median(us)) / floor_us, 2)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worlds", default="4096")
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--peak-gbs", type=float, default=0.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_jacobian_timing.json"))
    args = ap.parse_args()
    if args.repeats < 5:
        sys.exit("--repeats must be at least 5")
    import torch

    if not torch.cuda.is_available():
        sys.exit("eval_jacobian_timing.py measures on the device: no GPU found")
    from newton_amd import _lib

    peak = args.peak_gbs or copy_peak_gbs()
    result = {"tool": "eval_jacobian_timing", "device": torch.cuda.get_device_name(0), "build": _lib.load().nt_build_info().decode(),
              "timer": "one HIP event pair per batch of back-to-back calls, the kernels taking turns batch by batch; median (min .. max) "
                       "of the batches",
              "streaming_peak_source": "--peak-gbs" if args.peak_gbs else "device-to-device copy of 256 MB measured in this process",
              "sizes": [measure(int(w), args.calls, args.repeats, args.warmup, peak) for w in args.worlds.split(",")]}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
