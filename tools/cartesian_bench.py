#!/usr/bin/env python3
"""Times of the Cartesian straight-line operator (csrc/mp_cartesian.h: k_cart_track, k_cart_span, k_cart_reduce) on one GPU.

    python tools/cartesian_bench.py [--base 1024] [--copies 128] [--grid 65] [--reps 5] [--robots xarm6,panda] [--out FILE]

Prints one JSON line and writes it to --out (profiles/cartesian_bench.json unless given).  Per robot --base problems drawn by the
recipe of tests/cartesian_cases.py (task "full", margin 0.02, tol 1e-3, eomg = ev = 1e-6, damping 0.01, max_iters 20, max_joint_step
0.5, max_steps 64) and --copies copies of them (a problem's result depends on its content only): 131 072 problems at N = --grid.
  call_ms              mp_cartesian_path_f64 with every output: the three launches and the queue head's reset, the median of --reps
                       single calls timed one by one with HIP events after a warm-up call;
  problems_per_s       problems / call_ms;
  pose_evals_per_s     (sum of `iterations` + sum of `reached`) / call_ms: one pose evaluation for every Newton step and one for every
                       accepted point (the evaluations of a point that then fails are not counted: a lower bound);
  collision_evals_per_s  sum of `evaluations` / call_ms;
  grid_bytes           what the tracking writes into q, dq, ddq: 24 n bytes a grid row;
  probe_GB_per_s       a write-only streaming probe of grid_bytes in the same process (mp_stream_bandwidth_mix, 0 reads : 1 write).
call_ms is the whole call; the three kernels' own times come from a kernel trace of this tool
(rocprofv3 --kernel-trace --stats -- python tools/cartesian_bench.py --reps 1), dispatch by dispatch.
Without a device the tool fails: it has no other path.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from manipulapy_amd import _hip  # noqa: E402

WHOLE = ("status", "reached", "span", "iterations", "evaluations", "span_status")
SETTINGS = dict(task="full", eomg=1e-6, ev=1e-6, damping=0.01, max_iters=20, max_joint_step=0.5, max_steps=64)


def _median_ms(ctx, fn, reps):
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
        a.destroy()
        b.destroy()
    return float(np.median(out)), float(min(out)), float(max(out))


def _run(ctx, cm, q0, Tg, lo, hi, grid, reps, margin, tol):
    B, n = q0.shape
    shape = {"q": (B, grid, n), "dq": (B, grid, n), "ddq": (B, grid, n), "span_status": (B, grid - 1), "span_clearance": (B, grid - 1)}
    dq0, dTg = ctx.to_device(np.ascontiguousarray(q0)), ctx.to_device(np.ascontiguousarray(Tg))
    ws_bytes = _hip.cartesian_path_workspace_bytes(B, grid)
    ws = ctx.alloc(ws_bytes)
    bufs = {k: ctx.alloc(int(np.prod(shape.get(k, (B,)))) * (4 if k in WHOLE else 8)) for k in _hip.CARTESIAN_OUTPUTS}
    try:
        cm.sync_world(ctx)
        call = lambda: ctx.cartesian_path(cm.model, cm.handle, dq0, dTg, B, lo, hi, grid, margin, tol, d_workspace=ws,  # noqa: E731
                                          workspace_bytes=ws_bytes, **SETTINGS, **{"d_" + k: b for k, b in bufs.items()})
        ms = _median_ms(ctx, call, reps)
        st = bufs["status"].download((B,), np.int32)
        it = bufs["iterations"].download((B,), np.int32).astype(np.int64)
        re = bufs["reached"].download((B,), np.int32).astype(np.int64)
        ev = bufs["evaluations"].download((B,), np.int32).astype(np.int64)
        nbytes = 3 * B * grid * n * 8
        probe = ctx.stream_bandwidth_mix(nbytes, 0, 1, reps=reps, nontemporal=True)
        sec = 1e-3 * ms[0]
        r = {"problems": B, "grid": grid, "call_ms": ms[0], "call_min_ms": ms[1], "call_max_ms": ms[2], "problems_per_s": B / sec,
             "pose_evals": int(it.sum() + re.sum()), "pose_evals_per_s": float((it.sum() + re.sum()) / sec),
             "collision_evals": int(ev.sum()), "collision_evals_per_s": float(ev.sum() / sec),
             "status_share": {str(int(s)): round(float((st == s).mean()), 4) for s in np.unique(st)},
             "grid_bytes": nbytes, "grid_GB_per_s_over_the_call": nbytes / sec / 1e9, "probe_GB_per_s": probe}
        return {k: (round(v, 4) if isinstance(v, float) and abs(v) < 1e4 else float(f"{v:.4e}") if isinstance(v, float) else v)
                for k, v in r.items()}
    finally:
        for b in (dq0, dTg, ws, *bufs.values()):
            b.free()


def main():
    import cartesian_cases as cs
    import goal_cases as gc
    import rrt_cases as rc

    ap = argparse.ArgumentParser()
    ap.add_argument("--base", type=int, default=1024)
    ap.add_argument("--copies", type=int, default=128)
    ap.add_argument("--grid", type=int, default=65)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--robots", default="xarm6,panda")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cartesian_bench.json"))
    args = ap.parse_args()
    ctx = _hip.HipContext(0)
    props = ctx.properties()
    res = {"device": (props.get("name") or "unknown").strip("() "), "reps": args.reps, "statistic": "median after one warm-up",
           "margin": cs.MARGIN, "tol": cs.TOL, **SETTINGS, "robots": {}}
    planted = {k: v for k, v in cs.PLANTED.items() if k != "SINGULAR_ROW"}
    for name in args.robots.split(","):
        cm, S_list, lo, hi = rc.make_plan_model(name)
        case = cs._draw(cm, S_list, rc.oracle_model(name), gc.tool_of(name), lo, hi, 61, args.base, planted, "full", 5,
                        cs.ROBOT_REACH.get(name, cs.REACH))
        q0, Tg = np.tile(case["q0"], (args.copies, 1)), np.tile(case["Tg"], (args.copies, 1))
        res["robots"][name] = {"n": cm.n, "spheres": int(len(cm.links)),
                               "batch": _run(ctx, cm, q0, Tg, lo, hi, args.grid, args.reps, cs.MARGIN, cs.TOL)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
