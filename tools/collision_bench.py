#!/usr/bin/env python3
"""Times of the sphere-model collision kernel (csrc/mp_collision.h) on one GPU, beside two baselines.

    python tools/collision_bench.py [--B 131072] [--N 100] [--reps 3] [--robots xarm6,panda] [--cpu-rows 262144] [--out FILE]

Prints one JSON line and writes it to --out (profiles/r14_collision_bench.json unless given).  Per robot, B N rows of the case of
tests/collision_cases.py (from_urdf spheres of radius 0.06 and a base sphere, 12 obstacles, q uniform in the joint limits), device arrays:
  dist_ms       mp_collision_f64 with the distances, the witnesses and the cost (the instance without gradients);
  grad_ms       the same with all eight outputs (the gradient instance);
  cost_grad_ms  cost and its gradient only (what an optimiser asks for);
  fk_jac_ms     the existing mp_fk_jac_vjp_f64 launch over the same rows writing T and J: FK + the Jacobian alone, the floor this
                kernel sits on (it writes 16 + 6 n values a row where the collision kernel writes at most 2 n + 8);
  cpu_ms        the CPU twin mp_collision_cpu_f64 with all outputs on --cpu-rows rows (the machine's default thread count), scaled to
                B N rows; cpu_rows_per_s is what was measured.
Every GPU time is the median of single launches timed one by one with HIP events after a warm-up launch; *_min_ms / *_max_ms /
*_launches give the spread.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from manipulapy_amd import _hip  # noqa: E402


def _time(ctx, fn, reps, window_ms=400.0, cap=40):
    a, b = _hip.HipEvent(ctx), _hip.HipEvent(ctx)

    def once():
        a.record()
        fn()
        b.record()
        ctx.synchronize()
        return b.elapsed_ms_since(a)

    first = once()
    n = int(min(cap, max(reps, np.ceil(window_ms / max(first, 1e-3)))))
    t = np.array([once() for _ in range(n)])
    a.destroy(); b.destroy()
    return float(np.median(t)), float(t.min()), float(t.max()), n


def main():
    import collision_cases as cc

    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=131072)
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--robots", default="xarm6,panda")
    ap.add_argument("--cpu-rows", type=int, default=262144)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_collision_bench.json"))
    args = ap.parse_args()
    ctx = _hip.HipContext(0)
    rows = args.B * args.N
    res = {"B": args.B, "N": args.N, "rows": rows, "device": (ctx.properties().get("name") or "unknown").strip("() "), "robots": {}}
    for name in args.robots.split(","):
        case = cc.make_case(name, rows=4096)
        cm = case["cm"]
        n = cm.n
        lo, hi = case["q"].min(axis=0), case["q"].max(axis=0)
        q = np.random.default_rng(1).uniform(lo, hi, (rows, n))
        bufs = []

        def keep(b):
            bufs.append(b)
            return b

        d_q = keep(ctx.to_device(q))
        col, vec = rows * 8, rows * n * 8
        d = {"dist_world": keep(ctx.alloc(col)), "arg_world": keep(ctx.alloc(col)), "dist_self": keep(ctx.alloc(col)),
             "arg_self": keep(ctx.alloc(col)), "grad_dist_world": keep(ctx.alloc(vec)), "grad_dist_self": keep(ctx.alloc(vec)),
             "cost": keep(ctx.alloc(col)), "grad": keep(ctx.alloc(vec))}
        d_T, d_J = keep(ctx.alloc(rows * 16 * 8)), keep(ctx.alloc(6 * vec))
        cm.sync_world(ctx)
        r = {"n": n, "spheres": int(len(cm.links)), "pairs": int(len(cm.pairs)), "obstacles": int(len(cm.kinds))}

        def put(key, t):
            r[f"{key}_ms"], r[f"{key}_min_ms"], r[f"{key}_max_ms"], r[f"{key}_launches"] = t

        def run(keys):
            ctx.collision(cm.model, cm.handle, d_q, rows, cc.EPS_WORLD, cc.EPS_SELF, **{"d_" + k: d[k] for k in keys})

        put("dist", _time(ctx, lambda: run(("dist_world", "arg_world", "dist_self", "arg_self", "cost")), args.reps))
        put("grad", _time(ctx, lambda: run(tuple(d)), args.reps))
        put("cost_grad", _time(ctx, lambda: run(("cost", "grad")), args.reps))
        put("fk_jac", _time(ctx, lambda: ctx.fk_jac_vjp(cm.model, "space", d_q, None, None, rows, d_T, d_J, None), args.reps))
        cr = min(args.cpu_rows, rows)
        t0 = time.perf_counter()
        _hip.cpu_collision(cm.model, cm.handle, q[:cr], cc.EPS_WORLD, cc.EPS_SELF)
        dt = time.perf_counter() - t0
        r["cpu_threads"] = _hip.cpu_threads(cr)
        r["cpu_rows_per_s"] = cr / dt
        r["cpu_ms"] = 1e3 * rows / r["cpu_rows_per_s"]
        r["grad_rows_per_s"] = rows / (1e-3 * r["grad_ms"])
        r["grad_over_fk_jac"] = r["grad_ms"] / r["fk_jac_ms"]
        r["dist_over_fk_jac"] = r["dist_ms"] / r["fk_jac_ms"]
        r["cpu_over_grad"] = r["cpu_ms"] / r["grad_ms"]
        for k, v in list(r.items()):
            if isinstance(v, float):
                r[k] = round(v, 4) if abs(v) < 1e4 else float(f"{v:.4e}")
        res["robots"][name] = r
        for b in bufs:
            b.free()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
