#!/usr/bin/env python
"""MEASUREMENT TOOL -- nt_ik_solve (one launch, all iterations inside) beside the composition it replaces, on the same model in the same
process: per iteration one nt_eval_fk and one nt_eval_jacobian into caller tensors (the batched solve, the retraction and the accept /
reject decision a user would add on top are NOT counted: the composition's figure is a lower bound).

    python tools/ik_solver_timing.py [--worlds 4096] [--calls 20] [--repeats 7] [--warmup 10] [--out FILE]

Quadruped scene: four foot position objectives, one base rotation objective, the joint-limit objective.  One HIP event pair around a
batch of `--calls` back-to-back launches gives a per-call time; the legs take turns batch by batch, `--repeats` (>= 5) batches each;
median and spread (min .. max) are reported.  Prints ONE JSON line and writes it to --out (default profiles/ik_solver_timing.json)."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def measure(worlds, calls, repeats, warmup):
    import numpy as np
    import torch

    from ik_cases import ik_case, make_objectives
    from newton_amd import _lib, ik
    from newton_amd.state import pack_soa

    model, q_star, targets, start = ik_case("quadruped", worlds, 5, device="cuda:0")
    t, dm = model.env, model.device_model()
    lib = dm.lib
    solver = ik.IKSolver(model, make_objectives("quadruped", model, targets))
    q_in = torch.from_numpy(start.astype(np.float32)).to("cuda:0")
    q_out = torch.empty_like(q_in)
    jq = start.astype(np.float32).reshape(-1)
    jqd = np.zeros(model.joint_dof_count, np.float32)
    src_q, src_qd = pack_soa(model, jq, 1, t.nc), pack_soa(model, jqd, 1, t.nd)
    state = model.state()
    state.joint_q, state.joint_qd = jq, jqd
    d = state._desc()
    L, D = model.max_joints_per_articulation, model.max_dofs_per_articulation
    J = torch.zeros((worlds * t.na, 6 * L, D), dtype=torch.float32, device="cuda:0")
    m, s, st = C.byref(dm.desc), C.byref(d), dm.stream()

    def composition():
        _lib.check(lib.nt_eval_fk(m, src_q.data_ptr(), src_qd.data_ptr(), s, st), "nt_eval_fk")
        _lib.check(lib.nt_eval_jacobian(m, s, J.data_ptr(), None, None, st), "nt_eval_jacobian")

    def fused(iterations):
        def call():
            solver.lambdas.fill_(solver.lambda_initial)  # (every call does the same work; the fill is the lambda_fill_only leg, ~6 us of the figure)
            solver.step(q_in, q_out, iterations=iterations)
        return call

    legs = {"eval_fk_plus_eval_jacobian": composition, "ik_solve_0_iterations": fused(0), "ik_solve_1_iteration": fused(1),
            "ik_solve_10_iterations": fused(10), "lambda_fill_only": lambda: solver.lambdas.fill_(solver.lambda_initial)}
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
    out = {"worlds": worlds, "calls_per_batch": calls, "batches": repeats, "warmup_calls": warmup, "nd": int(t.nd),
           "objectives": len(solver.objectives), "params_uniform": int(dm.desc.params_uniform), "J_bytes": int(J.numel() * 4)}
    for n, us in per_call.items():
        us = np.array(us)
        out[n] = {"us_median": round(float(np.median(us)), 3), "us_min": round(float(us.min()), 3), "us_max": round(float(us.max()), 3)}
    med = lambda n: out[n]["us_median"]  # noqa: E731
    out["fused_us_per_iteration"] = round((med("ik_solve_10_iterations") - med("ik_solve_1_iteration")) / 9.0, 3)
    out["composition_us_per_iteration"] = med("eval_fk_plus_eval_jacobian")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worlds", default="4096")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ik_solver_timing.json"))
    args = ap.parse_args()
    if args.repeats < 5:
        sys.exit("--repeats must be at least 5")
    import torch

    if not torch.cuda.is_available():
        sys.exit("ik_solver_timing.py measures on the device: no GPU found")
    from newton_amd import _lib

    result = {"tool": "ik_solver_timing", "device": torch.cuda.get_device_name(0), "build": _lib.load().nt_build_info().decode(),
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
