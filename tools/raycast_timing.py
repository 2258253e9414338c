#!/usr/bin/env python
"""MEASUREMENT TOOL -- SensorRaycast.eval (nt_raycast, one launch) on the flagship-size scenes, beside one rollout frame of the same build.

    python tools/raycast_timing.py [--worlds 4096] [--calls 20] [--repeats 7] [--warmup 10] [--out FILE]

Legs: a height scan of 187 rays (11 x 17, pointing down from body 0, 0.5 m above it so that the body's own shape is below the origins
and excluded) on terrain_scene as a mesh and as a heightfield, and on quadruped_scene over its ground plane; and one frame of
SolverXPBD.rollout on the quadruped scene (4 substeps of 1 ms, the bench.py default frame) as the context figure.  One HIP event pair
around a batch of `--calls` back-to-back launches gives a per-call time; the legs take turns batch by batch, `--repeats` (>= 5) batches
each; median and spread (min .. max) are reported, and rays per second from the median.  Nothing gates on these numbers.  Prints ONE
JSON line and writes it to --out (default profiles/raycast_timing.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def scan_pattern():
    import numpy as np

    xs, ys = np.linspace(-0.5, 0.5, 11), np.linspace(-0.8, 0.8, 17)
    o = np.array([[x, y, 0.5] for x in xs for y in ys], np.float32)
    return o, np.tile(np.array([0.0, 0.0, -1.0], np.float32), (len(o), 1))


def measure(worlds, calls, repeats, warmup):
    import numpy as np
    import torch

    import newton_amd as nt
    from newton_amd import sensors
    from scenes import quadruped_scene, terrain_scene

    o, d = scan_pattern()
    legs, info = {}, {}
    for name, model in (("terrain_mesh", terrain_scene(worlds, device="cuda:0")), ("terrain_hfield", terrain_scene(worlds, heightfield=True, device="cuda:0")),
                        ("quadruped_plane", quadruped_scene(worlds, device="cuda:0"))):
        s = sensors.SensorRaycast(model, o, d, ray_body=0, max_distance=10.0, exclude_bodies=(0,))
        state = model.state()
        legs[name] = (lambda s=s, state=state: s.eval(state))
        info[name] = {"targets": int(len(s.slots)), "sensor": s}
        if name == "quadruped_plane":
            pipe = nt.CollisionPipeline(model)
            contacts, solver = pipe.contacts(), nt.solvers.SolverXPBD(model)
            s0, s1, ctrl = model.state(), model.state(), model.control()
            legs["xpbd_rollout_frame_4_substeps"] = (lambda: solver.rollout(s0, s1, ctrl, contacts, 1e-3, 4))
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
    out = {"worlds": worlds, "rays_per_world": len(o), "calls_per_batch": calls, "batches": repeats, "warmup_calls": warmup}
    for n, us in per_call.items():
        us = np.array(us)
        out[n] = {"us_median": round(float(np.median(us)), 3), "us_min": round(float(us.min()), 3), "us_max": round(float(us.max()), 3)}
        if n in info:
            hit = float((info[n]["sensor"].distance >= 0).float().mean().item())
            out[n].update(targets=info[n]["targets"], hit_fraction=round(hit, 4),
                          rays_per_second=round(worlds * len(o) / (float(np.median(us)) * 1e-6), 1))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worlds", default="4096")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raycast_timing.json"))
    args = ap.parse_args()
    if args.repeats < 5:
        sys.exit("--repeats must be at least 5")
    import torch

    if not torch.cuda.is_available():
        sys.exit("raycast_timing.py measures on the device: no GPU found")
    from newton_amd import _lib

    result = {"tool": "raycast_timing", "device": torch.cuda.get_device_name(0), "build": _lib.load().nt_build_info().decode(),
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
