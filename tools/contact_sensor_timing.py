#!/usr/bin/env python
"""MEASUREMENT TOOL -- SensorContact.eval (nt_contact_sensor, one launch) on the quadruped scene, beside the route it replaces and one
rollout frame of the same build.

    python tools/contact_sensor_timing.py [--worlds 4096] [--calls 20] [--repeats 7] [--warmup 10] [--out FILE]

Scene: quadruped_scene lowered onto the ground (as in smoke()), stepped until the feet carry force; the four lower legs are the sensing
bodies, the ground plane the counterpart.  Legs: `sensor_eval` (the one launch); `update_contacts_export_scatter`, the route without the
sensor on a fresh frame -- SolverXPBD.update_contacts, the flat rigid_contact_shape0/1 export (which reads the count back to the host)
and a torch index_add_ of the forces onto (world, foot); and one frame of SolverXPBD.rollout (4 substeps of 1 ms; with Contacts.force
requested it runs launch by launch) as the context figure.  One HIP event pair around a batch of `--calls` back-to-back calls gives a
per-call time; the legs take turns batch by batch, `--repeats` (>= 5) batches each; median and spread (min .. max) are reported.
Nothing gates on these numbers.  Prints ONE JSON line and writes it to --out (default profiles/contact_sensor_timing.json)."""
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
    model.request_contact_attributes("force")
    t = model.env
    feet = [b for b in range(t.nb) if model.body_label[b].endswith("_SHANK")]
    pipe = nt.CollisionPipeline(model)
    contacts, solver = pipe.contacts(), nt.solvers.SolverXPBD(model)
    s0, s1, ctrl = model.state(), model.state(), model.control()
    for _ in range(8):
        s0.clear_forces()
        pipe.collide(s0, contacts)
        solver.step(s0, s1, ctrl, contacts, 1e-3)
        s0, s1 = s1, s0
    sensor = sensors.SensorContact(model, sensing_bodies=feet, counterpart_shapes=[t.ns])
    dev = sensor.net_force.device
    foot_of_slot = torch.from_numpy(sensor.slot_sensing.astype(np.int64)).to(dev)
    ground_id = int(np.asarray(t.gshape_id)[0])
    scattered = torch.zeros((worlds * len(feet), 3), dtype=torch.float32, device=dev)

    def route():
        contacts.invalidate_views()  # a fresh frame: the export runs again
        solver.update_contacts(contacts)
        n = int(contacts.rigid_contact_count.item())
        a, b, f = contacts.rigid_contact_shape0[:n].long(), contacts.rigid_contact_shape1[:n].long(), contacts.force[:n, :3]
        scattered.zero_()
        for mine, other, sign in ((a, b, 1.0), (b, a, -1.0)):
            local = (mine >= t.shape_local0) & (mine < t.shape_local0 + worlds * t.ns) & (other == ground_id)
            rel = (mine - t.shape_local0).clamp(min=0)
            foot = foot_of_slot[rel % t.ns]
            keep = local & (foot >= 0)
            scattered.index_add_(0, ((rel // t.ns) * len(feet) + foot)[keep], sign * f[keep])

    r0, r1 = model.state(), model.state()
    legs = {"sensor_eval": lambda: sensor.eval(contacts), "update_contacts_export_scatter": route,
            "xpbd_rollout_frame_4_substeps": lambda: solver.rollout(r0, r1, ctrl, contacts, 1e-3, 4)}
    sensor.eval(contacts)
    route()
    torch.cuda.synchronize()
    agree = float((scattered.reshape(worlds, len(feet), 3) - sensor.net_force[:, :, 1]).abs().max().item())
    in_contact = float((sensor.net_force[:, :, 0].abs().sum(dim=(1, 2)) > 0).float().mean().item())
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
    out = {"worlds": worlds, "sensing_objects": len(feet), "columns": sensor.shape[1], "contact_slots_per_world": int(t.np * t.cpp),
           "worlds_with_foot_force": round(in_contact, 4), "max_abs_difference_sensor_vs_route": agree, "calls_per_batch": calls,
           "batches": repeats, "warmup_calls": warmup}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contact_sensor_timing.json"))
    args = ap.parse_args()
    if args.repeats < 5:
        sys.exit("--repeats must be at least 5")
    import torch

    if not torch.cuda.is_available():
        sys.exit("contact_sensor_timing.py measures on the device: no GPU found")
    from newton_amd import _lib

    result = {"tool": "contact_sensor_timing", "device": torch.cuda.get_device_name(0), "build": _lib.load().nt_build_info().decode(),
              "timer": "one HIP event pair per batch of back-to-back calls, the legs taking turns batch by batch; median (min .. max) of "
                       "the batches; the route leg includes its host read of the contact count",
              "sizes": [measure(int(w), args.calls, args.repeats, args.warmup) for w in args.worlds.split(",")]}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
