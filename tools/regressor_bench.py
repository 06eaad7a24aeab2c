#!/usr/bin/env python3
"""Time of the dynamics regressor kernels (csrc/mp_regressor.h) against the unfused alternative, on one GPU.

    python tools/regressor_bench.py [--rows 4000000] [--reps 5] [--robots ur5,panda] [--out profiles/r09_regressor_bench.json]

Prints one JSON line (and writes it to --out).  Per robot, over `rows` random float64 rows with a tip wrench, each timed with events
on the launch stream after one warm-up call, `reps` repeats, median and spread reported:
  regressor_ms        mp_id_regressor_f64 (Y and tau_ext to HBM); its output bytes as a fraction of 8 TB/s
  normal_ms           mp_id_regressor_normal_f64 (A, b, rr; Y never stored)
  normal_vjp_ms       the same without A (the autograd backward pass)
  unfused_ms          the regressor to HBM, then torch.matmul(Y^T, Y) over all rows on the device
  cpu_normal_ms       the CPU twin (mp_id_regressor_normal_cpu_f64) at 16 threads on rows / 16 rows, scaled to `rows`
  fused_A_rel_err     worst |A - A_host| / sqrt(A_ii A_jj) against a float64 host recomputation (NumPy sums of the CPU twin's Y) on a
                      subsample of the rows
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from manipulapy_amd import _hip, robots  # noqa: E402


def _model(name):
    t = robots.robot_tables(name)
    return _hip.HipModel(t["S_list"], t["Mlist_per_link"], t["Glist"], t["M_ee"], t["joint_limits"])


def _scale(A):
    """sqrt(A_ii A_jj), diagonals floored at 1e-10 of the largest (parameters the joints cannot excite have A_ii ~ 0)"""
    dg = np.maximum(np.diag(A), 1e-10 * np.diag(A).max())
    return np.sqrt(np.outer(dg, dg))


def _time(ctx, fn, reps):
    fn()
    ctx.synchronize()
    out = []
    for _ in range(reps):
        a, b = _hip.HipEvent(ctx), _hip.HipEvent(ctx)
        a.record()
        fn()
        b.record()
        ctx.synchronize()
        out.append(b.elapsed_ms_since(a))
        a.destroy(); b.destroy()
    return {"median": float(np.median(out)), "min": float(np.min(out)), "max": float(np.max(out))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--robots", default="ur5,panda")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_regressor_bench.json"))
    args = ap.parse_args()
    import torch

    ctx = _hip.HipContext(0)
    R = args.rows
    g, F = np.array([0.0, 0.0, -9.81]), np.array([1.0, -2.0, 0.5, 3.0, -1.5, 0.75])
    res = {"rows": R, "reps": args.reps, "device": ctx.properties()["name"], "robots": {}}
    for name in args.robots.split(","):
        m = _model(name)
        n, w = m.n, 10 * m.n
        rng = np.random.default_rng(0)
        x = [rng.uniform(-2, 2, (R, n)) for _ in range(3)] + [rng.uniform(-20, 20, (R, n))]
        d = [ctx.to_device(a) for a in x]
        work = ctx.alloc(_hip.id_regressor_normal_workspace_bytes(m, R))
        A, b, rr = ctx.alloc(w * w * 8), ctx.alloc(w * 8), ctx.alloc(16)
        te = ctx.alloc(R * n * 8)
        r = {}
        r["normal_ms"] = _time(ctx, lambda: ctx.id_regressor_normal(m, d[0], d[1], d[2], d[3], R, work, A, b, rr, g, F), args.reps)
        r["normal_vjp_ms"] = _time(ctx, lambda: ctx.id_regressor_normal(m, d[0], d[1], d[2], d[3], R, work, None, b, rr, g, None),
                                   args.reps)
        ctx.id_regressor_normal(m, d[0], d[1], d[2], d[3], R, work, A, b, rr, g, F)
        ctx.synchronize()
        A_dev = A.download((w, w), np.float64)
        # unfused: Y to HBM (a torch tensor the library writes on its own stream), then one GEMM over all rows
        Yt = torch.empty((R * n, w), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        r["regressor_ms"] = _time(ctx, lambda: ctx.id_regressor(m, d[0], d[1], d[2], R, Yt.data_ptr(), te, g, F), args.reps)
        r["regressor_out_GBps"] = (R * n * w * 8 + R * n * 8) / (r["regressor_ms"]["median"] * 1e-3) / 1e9
        r["regressor_frac_of_8TBps"] = r["regressor_out_GBps"] / 8000.0
        ts = []
        for _ in range(args.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.id_regressor(m, d[0], d[1], d[2], R, Yt.data_ptr(), te, g, F)
            ctx.synchronize()
            Au = torch.matmul(Yt.mT, Yt)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts = ts[1:]
        r["unfused_ms"] = {"median": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts)),
                           "note": "wall clock incl. one stream hand-over"}
        r["unfused_Y_bytes"] = R * n * w * 8
        Au = Au.cpu().numpy()
        dg = _scale(Au)
        r["fused_vs_unfused_A_rel"] = float(np.max(np.abs(A_dev - Au) / dg))
        del Yt, Au
        torch.cuda.empty_cache()
        # float64 host recomputation on a subsample
        S = 20000
        sub = [a[:S] for a in x]
        Ys, tes = _hip.cpu_id_regressor(m, sub[0], sub[1], sub[2], g, F)
        Ys = Ys.reshape(-1, w)
        A_host = Ys.T @ Ys
        sd = [ctx.to_device(a) for a in sub]
        ws = ctx.alloc(_hip.id_regressor_normal_workspace_bytes(m, S))
        ctx.id_regressor_normal(m, sd[0], sd[1], sd[2], sd[3], S, ws, A, b, rr, g, F)
        ctx.synchronize()
        A_sub = A.download((w, w), np.float64)
        dg = _scale(A_host)
        r["fused_A_rel_err"] = float(np.max(np.abs(A_sub - A_host) / dg))
        Rc = R // 16
        t0 = time.perf_counter()
        _hip.cpu_id_regressor_normal(m, x[0][:Rc], x[1][:Rc], x[2][:Rc], x[3][:Rc], g, F, nthreads=16)
        r["cpu_normal_ms"] = (time.perf_counter() - t0) * 1e3 * 16
        for bb in d + sd + [work, ws, A, b, rr, te]:
            bb.free()
        res["robots"][name] = r
        print(name, json.dumps(r), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
