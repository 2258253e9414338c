#!/usr/bin/env python
"""MEASUREMENT TOOL -- SolverSemiImplicit: one frame of substeps as (a) the per-call loop `clear_forces; collide; step; swap`,
(b) the same loop recorded once and replayed as ONE hipGraph, (c) `SolverSemiImplicit.rollout` (one launch).

    python tools/semi_implicit_rollout_ab.py [--worlds 4096] [--substeps 10] [--frames 100] [--rounds 5] [--out FILE]

Scenes: tests/scenes.py quadruped_scene (lowered into ground contact, dt 1e-4) and pendulum_scene (dt 1e-3).  Every leg starts from
the same state, is warmed up, then timed with HIP events over `frames` frames per round; the legs alternate inside a round and the
reported time is the median round (min / max are kept beside it).  Before timing, the three legs are run for the same number of
frames and must agree bit for bit.  Prints ONE JSON line and writes it to --out (default profiles/semi_implicit_rollout_ab.json).
Through tools/with_lib.py with a library that lacks nt_semi_implicit_rollout, leg (c) is reported as null: that is how the loop
legs of an older build are measured with this tool."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _scene(name, worlds):
    import numpy as np

    import newton_amd as nt
    import scenes

    if name == "pendulum":
        return scenes.pendulum_scene(worlds, device="cuda:0", seed=11), 1e-3
    model = scenes.quadruped_scene(worlds, device="cuda:0")
    model.joint_q.reshape(worlds, -1)[:, 2] -= 0.26
    model.body_q, model.body_qd = nt.articulation.eval_fk_numpy(model, model.joint_q, model.joint_qd)
    rng = np.random.default_rng(3)
    model.body_qd = (model.body_qd + rng.normal(0, 0.3, size=model.body_qd.shape)).astype(np.float32)
    return model, 1e-4


class Leg:
    def __init__(self, name, model, dt, substeps):
        import newton_amd as nt

        assert substeps % 2 == 0, "a replayed frame must leave the state objects where it found them"
        self.name, self.model = name, model
        self.solver, self.pipe = nt.solvers.SolverSemiImplicit(model), nt.CollisionPipeline(model)
        self.s0, self.s1, self.ctrl, self.contacts = model.state(), model.state(), model.control(), self.pipe.contacts()
        self.start = model.state()  # (never stepped: State.assign copies it back before every run)
        s0, s1, ctrl, ct, solver, pipe = self.s0, self.s1, self.ctrl, self.contacts, self.solver, self.pipe

        def loop():
            a, b = s0, s1
            for _ in range(substeps):
                a.clear_forces()
                pipe.collide(a, ct)
                solver.step(a, b, ctrl, ct, dt)
                a, b = b, a

        if name == "loop":
            self.frame = loop
        elif name == "graph":
            self.frame = nt.graph.capture(loop, warmup=1, contacts=ct).launch
        else:
            self.frame = lambda: solver.rollout(s0, s1, ctrl, ct, dt, substeps)

    def reset(self):
        self.s0.assign(self.start)

    def time_ms(self, frames):
        import torch

        self.reset()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(frames):
            self.frame()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / frames


def measure(scene, worlds, substeps, frames, rounds, check_frames):
    import numpy as np
    import torch

    from newton_amd import _lib

    model, dt = _scene(scene, worlds)
    names = ["loop", "graph"] + (["rollout"] if "nt_semi_implicit_rollout" in _lib.SYMBOLS else [])
    legs = [Leg(n, model, dt, substeps) for n in names]
    # same inputs, same frames -> same bits, before anything is timed (also the warm-up of every leg)
    finals = []
    for leg in legs:
        leg.reset()
        for _ in range(check_frames):
            leg.frame()
        torch.cuda.synchronize()
        finals.append((leg.s0.body_q.cpu().numpy().view(np.uint32), leg.s0.body_qd.cpu().numpy().view(np.uint32)))
    identical = all(np.array_equal(f[0], finals[0][0]) and np.array_equal(f[1], finals[0][1]) for f in finals)
    finite = bool(np.isfinite(finals[0][0].view(np.float32)).all())
    times = {n: [] for n in names}
    for _ in range(rounds):
        for leg in legs:
            times[leg.name].append(leg.time_ms(frames))
    out = {"worlds": worlds, "substeps": substeps, "dt": dt, "frames_per_round": frames, "rounds": rounds,
           "legs_bitwise_identical": identical, "state_finite": finite,
           "contacts": int(legs[0].contacts.rigid_contact_count.cpu().numpy()[0])}
    for n in ("loop", "graph", "rollout"):
        if n not in times:
            out[n] = None
            continue
        ms = statistics.median(times[n])
        out[n] = {"ms_per_frame": round(ms, 5), "ms_min": round(min(times[n]), 5), "ms_max": round(max(times[n]), 5),
                  "env_steps_per_s": round(worlds * substeps / (ms * 1e-3), 1)}
    if out["rollout"]:
        out["rollout_vs_graph"] = round(out["graph"]["ms_per_frame"] / out["rollout"]["ms_per_frame"], 3)
        out["rollout_vs_loop"] = round(out["loop"]["ms_per_frame"] / out["rollout"]["ms_per_frame"], 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worlds", type=int, default=4096)
    ap.add_argument("--substeps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--check-frames", type=int, default=3)
    ap.add_argument("--scenes", default="quadruped,pendulum")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "semi_implicit_rollout_ab.json"))
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("semi_implicit_rollout_ab.py measures on the device: no GPU found")
    from newton_amd import _lib

    result = {"tool": "semi_implicit_rollout_ab", "device": torch.cuda.get_device_name(0),
              "build": _lib.load().nt_build_info().decode(), "timer": "HIP events around frames_per_round frames, median of rounds"}
    for scene in args.scenes.split(","):
        result[scene] = measure(scene, args.worlds, args.substeps, args.frames, args.rounds, args.check_frames)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not all(result[s]["legs_bitwise_identical"] for s in args.scenes.split(",")):
        sys.exit("the legs disagree: the timings above do not compare the same computation")


if __name__ == "__main__":
    main()
