#!/usr/bin/env python
"""MEASUREMENT TOOL -- SensorTiledCamera.eval (nt_camera_render, one launch) beside SensorRaycast.eval over the very same rays.

    python tools/camera_timing.py [--calls 20] [--repeats 7] [--warmup 10] [--out FILE]

Shapes: (a) 4 096 quadrupeds on their plane, one 64 x 64 camera on the base (body 0) looking down and ahead, the base excluded; (b) 16
such worlds with one 256 x 256 camera.  Legs per shape: the camera with the cull on, with the cull off, and SensorRaycast with the
camera's H * W rays as one shared pattern (raycast_kernel, the same build).  One HIP event pair around a batch of `--calls` back-to-back
launches gives a per-call time; the legs take turns batch by batch, `--repeats` (>= 5) batches each; median and spread (min .. max) are
reported, and rays per second from the median.  Nothing gates on these numbers.  Prints ONE JSON line and writes it to --out (default
profiles/camera_timing.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = {"a_4096_worlds_64x64": (4096, 64), "b_16_worlds_256x256": (16, 256)}


def measure(worlds, size, calls, repeats, warmup):
    import numpy as np
    import torch

    import newton_amd as nt
    from newton_amd import sensors
    from scenes import quadruped_scene

    model = quadruped_scene(worlds, device="cuda:0")
    state = model.state()
    cam = [(0, [0.25, 0.0, 0.05, *nt._np_math.quat_rpy(0.0, -0.9, 0.0)])]  # at the front of the base, pitched 0.9 rad forward off straight down
    kw = dict(fov_y=np.deg2rad(60.0), max_distance=10.0, exclude_bodies=(0,))
    on = sensors.SensorTiledCamera(model, cam, size, size, cull=True, **kw)
    off = sensors.SensorTiledCamera(model, cam, size, size, cull=False, **kw)
    n = size * size
    ray = sensors.SensorRaycast(model, np.repeat(on.ray_origins, n, axis=0), on.ray_directions[0], ray_body=0, max_distance=10.0, exclude_bodies=(0,))
    legs = {"camera_cull_on": lambda: on.eval(state), "camera_cull_off": lambda: off.eval(state), "raycast_same_rays": lambda: ray.eval(state)}
    for _ in range(warmup):
        for f in legs.values():
            f()
    torch.cuda.synchronize()
    same = bool(torch.equal(on.distance.reshape(worlds, -1), ray.distance) and torch.equal(off.distance, on.distance))
    per_call = {k: [] for k in legs}
    for _ in range(repeats):
        for k, f in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                f()
            e1.record()
            torch.cuda.synchronize()
            per_call[k].append(e0.elapsed_time(e1) * 1e3 / calls)
    out = {"worlds": worlds, "width": size, "height": size, "targets": int(len(on.slots)), "calls_per_batch": calls, "batches": repeats,
           "warmup_calls": warmup, "hit_fraction": round(float((on.distance >= 0).float().mean().item()), 4),
           "camera_distance_equals_raycast": same}
    for k, us in per_call.items():
        us = np.array(us)
        out[k] = {"us_median": round(float(np.median(us)), 3), "us_min": round(float(us.min()), 3), "us_max": round(float(us.max()), 3),
                  "rays_per_second": round(worlds * n / (float(np.median(us)) * 1e-6), 1)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "camera_timing.json"))
    args = ap.parse_args()
    if args.repeats < 5:
        sys.exit("--repeats must be at least 5")
    import torch

    if not torch.cuda.is_available():
        sys.exit("camera_timing.py measures on the device: no GPU found")
    from newton_amd import _lib

    result = {"tool": "camera_timing", "device": torch.cuda.get_device_name(0), "build": _lib.load().nt_build_info().decode(),
              "timer": "one HIP event pair per batch of back-to-back calls, the legs taking turns batch by batch; median (min .. max) of "
                       "the batches",
              "shapes": {name: measure(w, s, args.calls, args.repeats, args.warmup) for name, (w, s) in SHAPES.items()}}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
