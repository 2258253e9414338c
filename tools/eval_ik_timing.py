#!/usr/bin/env python
"""MEASUREMENT TOOL -- nt_eval_ik against its sibling nt_eval_fk on the same model, same box.

    python tools/eval_ik_timing.py [--worlds 4096,262144] [--calls 200] [--warmup 20] [--out FILE]

Scene: tests/scenes.py quadruped_scene.  Both entry points are called through the C ABI on resident SoA buffers (no packing, no
copies in the timed region), alternating call by call, each call between its own pair of HIP events; `calls` calls per kernel after
`warmup`.  Reported per kernel: median, min, p10 / p90 and max of the per-call times, and the bytes per second of the algorithmic
traffic -- 52 B per body read plus 4 (nc + nd) B written per world for eval_ik, the same bytes the other way round for eval_fk.  A
third leg times eval_ik on the per-environment-parameter tile (nt_eval_ik_tile, 16 environments per workgroup), the tile eval_fk
uses.  Before timing, eval_ik(eval_fk(q, qd)) must return (q, qd) within 1e-5.  Prints ONE JSON line and writes it to --out (default
profiles/eval_ik_timing.json)."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def measure(worlds, calls, warmup):
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
    d = state._desc()
    out_q, out_qd = torch.zeros_like(src_q), torch.zeros_like(src_qd)

    def fk():
        _lib.check(lib.nt_eval_fk(C.byref(dm.desc), src_q.data_ptr(), src_qd.data_ptr(), C.byref(d), dm.stream()), "nt_eval_fk")

    def ik():
        _lib.check(lib.nt_eval_ik(C.byref(dm.desc), C.byref(d), out_q.data_ptr(), out_qd.data_ptr(), None, dm.stream()), "nt_eval_ik")

    def ik_env_tile():
        _lib.check(lib.nt_eval_ik_tile(C.byref(dm.desc), C.byref(d), out_q.data_ptr(), out_qd.data_ptr(), None, 16, dm.stream()),
                   "nt_eval_ik_tile")

    legs = {"eval_fk": fk, "eval_ik": ik, "eval_ik_per_env_tile": ik_env_tile}
    fk()
    ik()
    torch.cuda.synchronize()
    err_q = float((out_q[0, :, :worlds] - src_q[0, :, :worlds]).abs().max())
    err_qd = float((out_qd[0, :, :worlds] - src_qd[0, :, :worlds]).abs().max())
    for _ in range(warmup):
        for f in legs.values():
            f()
    torch.cuda.synchronize()
    events = {n: [] for n in legs}
    for _ in range(calls):
        for n, f in legs.items():  # alternating, call by call
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            events[n].append((e0, e1))
    torch.cuda.synchronize()
    nbytes = worlds * (52 * t.nb + 4 * (t.nc + t.nd))
    out = {"worlds": worlds, "calls_per_kernel": calls, "warmup_calls": warmup, "bytes_per_call": nbytes,
           "round_trip_max_abs_err": {"joint_q": err_q, "joint_qd": err_qd}, "params_uniform": int(dm.desc.params_uniform)}
    for n, ev in events.items():
        us = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
        out[n] = {"us_median": round(float(np.median(us)), 3), "us_min": round(float(us.min()), 3),
                  "us_p10": round(float(np.percentile(us, 10)), 3), "us_p90": round(float(np.percentile(us, 90)), 3),
                  "us_max": round(float(us.max()), 3), "gbytes_per_s": round(nbytes / (float(np.median(us)) * 1e-6) / 1e9, 2)}
    out["eval_ik_over_eval_fk"] = round(out["eval_ik"]["us_median"] / out["eval_fk"]["us_median"], 4)
    out["within_10_percent_margin"] = bool(out["eval_ik"]["us_median"] <= 1.10 * out["eval_fk"]["us_median"])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worlds", default="4096,262144")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_ik_timing.json"))
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("eval_ik_timing.py measures on the device: no GPU found")
    from newton_amd import _lib

    result = {"tool": "eval_ik_timing", "device": torch.cuda.get_device_name(0), "build": _lib.load().nt_build_info().decode(),
              "timer": "one HIP event pair per call, the kernels alternating call by call", "sizes": []}
    for w in args.worlds.split(","):
        result["sizes"].append(measure(int(w), args.calls, args.warmup))
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    for s in result["sizes"]:
        if max(s["round_trip_max_abs_err"].values()) > 1e-5:
            sys.exit("eval_ik(eval_fk(q, qd)) != (q, qd): the timings above do not compare inverse computations")


if __name__ == "__main__":
    main()
