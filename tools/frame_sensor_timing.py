#!/usr/bin/env python
"""MEASUREMENT TOOL -- SensorFrameTransform.eval and SensorIMU.eval (nt_frame_sensor, one launch each) on the quadruped scene, beside
the same quantities composed from state.body_q / state.body_qd with torch ops (what a user writes without the sensors).

    python tools/frame_sensor_timing.py [--worlds 4096] [--calls 20] [--repeats 7] [--warmup 10] [--out FILE]

Scene: quadruped_scene lowered onto the ground (as in smoke()), 8 XPBD steps; 5 frames: the base and the four shanks.  Legs:
`frame_transform_eval` (the shanks and the base in the base frame), `imu_eval` (5 IMUs with linear velocity and projected gravity),
`torch_frame_transform` and `torch_imu`: the AoS reads state.body_q / state.body_qd (one nt_unpack_aos launch and one allocation
each) followed by torch elementwise ops for the same outputs.  One HIP event pair around a batch of `--calls` back-to-back calls gives
a per-call time; the legs take turns batch by batch, `--repeats` (>= 5) batches each; median and spread (min .. max) are reported.
Nothing gates on these numbers.  Prints ONE JSON line and writes it to --out (default profiles/frame_sensor_timing.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def measure(worlds, calls, repeats, warmup):
    import numpy as np
    import torch

    import newton_amd as nt
    from newton_amd import sensors
    from scenes import quadruped_scene

    model = quadruped_scene(worlds, device="cuda:0")
    model.joint_q.reshape(worlds, -1)[:, 2] -= 0.26  # onto the ground, so that contacts are active
    model.body_q, model.body_qd = nt.articulation.eval_fk_numpy(model, model.joint_q, model.joint_qd)
    t = model.env
    base = [b for b in range(t.nb) if model.body_label[b].endswith("base")][0]
    bodies = [base] + [b for b in range(t.nb) if model.body_label[b].endswith("_SHANK")]
    pipe = nt.CollisionPipeline(model)
    contacts, solver = pipe.contacts(), nt.solvers.SolverXPBD(model)
    s0, s1, ctrl = model.state(), model.state(), model.control()
    dt = 1e-3
    for _ in range(8):
        s0.clear_forces()
        pipe.collide(s0, contacts)
        solver.step(s0, s1, ctrl, contacts, dt)
        s0, s1 = s1, s0
    new, old = s0, s1
    frames = [(b, None) for b in bodies]
    ft = sensors.SensorFrameTransform(model, frames, reference_frames=[(base, None)])
    imu = sensors.SensorIMU(model, frames, want_velocity=True, want_projected_gravity=True)
    dev = ft.transforms.device
    idx = torch.tensor(bodies, device=dev)
    com = torch.from_numpy(np.asarray(model.body_com, np.float32).reshape(worlds, t.nb, 3)[:, bodies]).to(dev)
    g = torch.from_numpy(np.asarray(model.gravity, np.float32)[:worlds]).to(dev)[:, None, :]

    def rot(q, v, sign=1.0):
        qv, w = q[..., :3], q[..., 3:4]
        return v * (2.0 * w * w - 1.0) + sign * torch.linalg.cross(qv, v) * w * 2.0 + qv * (qv * v).sum(-1, keepdim=True) * 2.0

    def qmul_inv_left(a, b):  # a^-1 * b
        a = a * torch.tensor([-1.0, -1.0, -1.0, 1.0], device=dev)
        av, aw, bv, bw = a[..., :3], a[..., 3:4], b[..., :3], b[..., 3:4]
        return torch.cat([aw * bv + bw * av + torch.linalg.cross(av, bv), aw * bw - (av * bv).sum(-1, keepdim=True)], dim=-1)

    torch_out = {}

    def torch_ft():
        bq = new.body_q.reshape(worlds, t.nb, 7)[:, idx]
        ref = bq[:, :1]
        torch_out["transform"] = torch.cat([rot(ref[..., 3:], bq[..., :3] - ref[..., :3], -1.0), qmul_inv_left(ref[..., 3:], bq[..., 3:])], dim=-1)

    def torch_imu():
        bq = new.body_q.reshape(worlds, t.nb, 7)[:, idx]
        qd, qd0 = new.body_qd.reshape(worlds, t.nb, 6)[:, idx], old.body_qd.reshape(worlds, t.nb, 6)[:, idx]
        q = bq[..., 3:]
        r = rot(q, -com)
        w = qd[..., 3:]
        acc = (qd[..., :3] - qd0[..., :3]) / dt + torch.linalg.cross((w - qd0[..., 3:]) / dt, r) + torch.linalg.cross(w, torch.linalg.cross(w, r)) - g
        torch_out["accel"] = rot(q, acc, -1.0)
        torch_out["gyro"] = rot(q, w, -1.0)
        torch_out["lin"] = rot(q, qd[..., :3] + torch.linalg.cross(w, r), -1.0)
        torch_out["gdir"] = rot(q, (g / g.norm(dim=-1, keepdim=True).clamp(min=1e-30)).expand_as(w), -1.0)

    legs = {"frame_transform_eval": lambda: ft.eval(new), "imu_eval": lambda: imu.eval(new, old, dt),
            "torch_frame_transform": torch_ft, "torch_imu": torch_imu}
    for f in legs.values():
        f()
    torch.cuda.synchronize()
    agree = {"transform": float((torch_out["transform"] - ft.transforms).abs().max().item()),
             "accelerometer": float((torch_out["accel"] - imu.accelerometer).abs().max().item()),
             "gyroscope": float((torch_out["gyro"] - imu.gyroscope).abs().max().item()),
             "linear_velocity": float((torch_out["lin"] - imu.linear_velocity).abs().max().item()),
             "projected_gravity": float((torch_out["gdir"] - imu.projected_gravity).abs().max().item())}
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
    out = {"worlds": worlds, "frames": len(bodies), "largest_accelerometer_reading": float(imu.accelerometer.abs().max().item()),
           "max_abs_difference_sensor_vs_torch": agree, "calls_per_batch": calls, "batches": repeats, "warmup_calls": warmup}
    for n, us in per_call.items():
        us = np.array(us)
        out[n] = {"us_median": round(float(np.median(us)), 3), "us_min": round(float(us.min()), 3), "us_max": round(float(us.max()), 3)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worlds", default="4096")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_sensor_timing.json"))
    args = ap.parse_args()
    if args.repeats < 5:
        sys.exit("--repeats must be at least 5")
    import torch

    if not torch.cuda.is_available():
        sys.exit("frame_sensor_timing.py measures on the device: no GPU found")
    from newton_amd import _lib

    result = {"tool": "frame_sensor_timing", "device": torch.cuda.get_device_name(0), "build": _lib.load().nt_build_info().decode(),
              "timer": "one HIP event pair per batch of back-to-back calls, the legs taking turns batch by batch; median (min .. max) of "
                       "the batches",
              "sizes": [measure(int(w), args.calls, args.repeats, args.warmup) for w in args.worlds.split(",")]}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
