#!/usr/bin/env python3
"""Throughput of the operational-space kernels (k_opspace / k_opspace_torque, csrc/mp_opspace.h), on one GPU.

    python tools/opspace_bench.py [--rows 1048576] [--reps 9] [--robots ur5,iiwa14,panda,xarm6] [--out profiles/r11_opspace_bench.json]

Prints one JSON line (and writes it to --out).  Per robot, hipEvent timing, the median over --reps launches after a warm-up launch:
  torque_<frame>_ms:  mp_opspace_torque_f64, task "full", tau0 = NULL (reads q, qd, a*; writes tau), hybrid and body frame;
  opspace_ms:         mp_opspace_f64 writing all seven outputs, hybrid / full;
  rows/s and the HBM GB/s each achieves (bytes the entry point has to move / time);
  composed_ms:        the only route to the same tau without these kernels, timed in the same process: mp_fd_derivatives_f64 (for M^-1
                      and, with tau = 0, qdd0 = -M^-1 h), mp_fk_jac_vjp_f64 (for the body Jacobian), then batched torch linear algebra on
                      the same stream: A = J M^-1 J^T, f = solve(A, a* - J qdd0), tau = J^T f.  Jdot qd is left out of it (it has no
                      way to compute it), in its favour;
  speedup:            composed_ms / torque_body_ms;   agreement_at_rest: the largest relative difference of the two torques on 4096
                      rows with qd = 0, where Jdot qd vanishes and both compute the same thing.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (first: the HIP runtime torch loads serves the library too)

import manipulapy_amd as mp  # noqa: E402
from manipulapy_amd import _hip, registry  # noqa: E402


def _median_ms(ctx, fn, reps):
    fn()
    ctx.synchronize()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = _hip.HipEvent(ctx), _hip.HipEvent(ctx)
        a.record()
        fn()
        b.record()
        ctx.synchronize()
        out.append(b.elapsed_ms_since(a))
        a.destroy(); b.destroy()
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--robots", default="ur5,iiwa14,panda,xarm6")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    ctx = registry.get_context()
    dev = torch.device("cuda", ctx.device_id)
    ext = torch.cuda.ExternalStream(ctx.stream())   # (a measurement process: handing the stream out is fine here)
    res = {"rows": args.rows, "reps": args.reps, "statistic": "median of hipEvent times after one warm-up launch",
           "device": ctx.properties()["name"], "task": "full", "baseline_omits_Jdot_qd": True, "robots": {}}
    for name in args.robots.split(","):
        dyn = mp.load_robot(name)[1]
        m = dyn._derivative_model("opspace_bench")
        n, R = m.n, args.rows
        rng = np.random.default_rng(0)
        t = lambda a: torch.tensor(a, device=dev)  # noqa: E731
        q, qd, acc = t(rng.uniform(-3, 3, (R, n))), t(rng.normal(size=(R, n))), t(rng.normal(size=(R, 6)))
        tau = torch.empty((R, n), dtype=torch.float64, device=dev)
        r = {"n": n}
        tb = R * 8 * (3 * n + 6)
        for frame in ("hybrid", "body"):
            ms = _median_ms(ctx, lambda: ctx.opspace_torque(m, frame, "full", 0.0, q.data_ptr(), qd.data_ptr(), acc.data_ptr(), None, R,
                                                            tau.data_ptr()), args.reps)
            r[f"torque_{frame}_ms"] = round(ms, 4)
            r[f"torque_{frame}_rows_per_s"] = round(R / ms * 1e3)
            r[f"torque_{frame}_GB_per_s"] = round(tb / ms / 1e6, 1)
        sizes = (16, 6 * n, 6, 36, 6 * n, 6, 6)
        outs = [torch.empty((R, k), dtype=torch.float64, device=dev) for k in sizes]
        ob = R * 8 * (2 * n + sum(sizes))
        ms = _median_ms(ctx, lambda: ctx.opspace(m, "hybrid", "full", 0.0, q.data_ptr(), qd.data_ptr(), R, None,
                                                 *[o.data_ptr() for o in outs]), args.reps)
        r.update(opspace_ms=round(ms, 4), opspace_rows_per_s=round(R / ms * 1e3), opspace_GB_per_s=round(ob / ms / 1e6, 1))
        del outs
        # the composition the library offered before
        zero = torch.zeros((R, n), dtype=torch.float64, device=dev)
        qdd0 = torch.empty((R, n), dtype=torch.float64, device=dev)
        dq, dqd, Minv = (torch.empty((R, n, n), dtype=torch.float64, device=dev) for _ in range(3))
        J = torch.empty((R, 6, n), dtype=torch.float64, device=dev)
        tau_c = torch.empty((R, n), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()

        def composed(rows=R, qd_=qd):
            ctx.fd_derivatives(m, q.data_ptr(), qd_.data_ptr(), zero.data_ptr(), rows, dq.data_ptr(), dqd.data_ptr(), qdd0.data_ptr(),
                               Minv.data_ptr())
            ctx.fk_jac_vjp(m, "body", q.data_ptr(), None, None, rows, None, J.data_ptr(), None)
            with torch.cuda.stream(ext):
                Jr, Mi = J[:rows], Minv[:rows]
                A = Jr @ Mi @ Jr.transpose(1, 2)
                rhs = acc[:rows] - (Jr @ qdd0[:rows, :, None])[:, :, 0]
                f = torch.linalg.solve_ex(A, rhs[:, :, None])[0]   # (no singularity check: no host synchronisation)
                tau_c[:rows] = (Jr.transpose(1, 2) @ f)[:, :, 0]

        ms = _median_ms(ctx, composed, max(3, args.reps // 2))
        r["composed_ms"] = round(ms, 3)
        r["speedup"] = round(ms / r["torque_body_ms"], 1)
        K = 4096
        composed(K, zero)
        ctx.opspace_torque(m, "body", "full", 0.0, q.data_ptr(), zero.data_ptr(), acc.data_ptr(), None, K, tau.data_ptr())
        ctx.synchronize()
        torch.cuda.synchronize()
        a, b = tau[:K].cpu().numpy(), tau_c[:K].cpu().numpy()
        ok = np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1)
        rel = np.abs(a[ok] - b[ok]).max(axis=1) / np.maximum(1.0, np.abs(a[ok]).max(axis=1))
        r["agreement_at_rest"] = {"rows": int(ok.sum()), "median_rel_diff": float(np.median(rel)), "p99_rel_diff": float(np.quantile(rel, 0.99))}
        res["robots"][name] = r
        del q, qd, acc, tau, zero, qdd0, dq, dqd, Minv, J, tau_c
        torch.cuda.empty_cache()
    res["fused_faster_on_every_robot"] = all(v["speedup"] > 1.0 for v in res["robots"].values())
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
