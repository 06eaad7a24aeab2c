#!/usr/bin/env python3
"""Times of the two corner-blending launches, k_path_blend and k_path_blend_sample (csrc/mp_blend.h), on one GPU.

    python tools/blend_bench.py [--copies 512] [--grid 129] [--reps 5] [--robots ur5,panda,chain3] [--out FILE]

Prints one JSON line and writes it to --out (profiles/blend_bench.json unless given).  Per robot the 139 problems of
tests/blend_cases.py (base run: margin 0.02, tol 1e-3, blend 0.5, max_halvings 6, max_steps 64) at their own size with N = 33, and
--copies copies of them (a problem's result depends on its content only) with N = --grid:
  corners_ms       mp_path_blend_f64 with the ten per-problem outputs and no grid array: k_path_blend alone (and the queue head's
                   reset); evals_per_s from the sum of the returned `evaluations`;
  both_ms          the same call with q, dq, ddq as well: both launches;
  sample_bytes     what k_path_blend_sample writes, 24 n bytes a grid row;
  probe_GB_per_s   a write-only streaming probe of sample_bytes in the same run (mp_stream_bandwidth_mix, 0 reads : 1 write,
                   non-temporal).
Every time is the median of --reps single calls timed one by one with HIP events after a warm-up call.  k_path_blend_sample is a
hundredth of the corner launch and is lost in the difference of the two medians: its own time is read from a kernel trace of this
tool (rocprofv3 --kernel-trace -- python tools/blend_bench.py), dispatch by dispatch, and set against sample_bytes and the probe.
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

WHOLE = ("status", "corner", "count", "halvings", "evaluations")
GRID_KEYS = ("q", "dq", "ddq")


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


def _run(ctx, cm, wp, cnt, grid, reps, bc):
    B, w_in, n = wp.shape
    shape = {"points": (B, w_in, n), "cut": (B, w_in), "knot": (B, w_in), "q": (B, grid, n), "dq": (B, grid, n), "ddq": (B, grid, n)}
    dw, dc = ctx.to_device(np.ascontiguousarray(wp)), ctx.to_device(np.ascontiguousarray(cnt))
    bufs = {k: ctx.alloc(int(np.prod(shape.get(k, (B,)))) * (4 if k in WHOLE else 8)) for k in _hip.BLEND_OUTPUTS}
    try:
        cm.sync_world(ctx)
        call = lambda keys: ctx.path_blend(cm.model, cm.handle, dw, dc, B, w_in, grid, bc.RUNS["base"], bc.TOL,  # noqa: E731
                                           **bc.params_of(), **{"d_" + k: bufs[k] for k in keys})
        tables = tuple(k for k in _hip.BLEND_OUTPUTS if k not in GRID_KEYS)
        corners = _median_ms(ctx, lambda: call(tables), reps)
        both = _median_ms(ctx, lambda: call(_hip.BLEND_OUTPUTS), reps)
        ev = bufs["evaluations"].download((B,), np.int32).astype(np.int64)
        st = bufs["status"].download((B,), np.int32)
        nbytes = 3 * B * grid * n * 8
        probe = ctx.stream_bandwidth_mix(nbytes, 0, 1, reps=reps, nontemporal=True)
        r = {"problems": B, "grid": grid, "corners_ms": corners[0], "corners_min_ms": corners[1], "corners_max_ms": corners[2],
             "both_ms": both[0], "both_min_ms": both[1], "both_max_ms": both[2], "evals": int(ev.sum()),
             "evals_per_s": float(ev.sum() / (1e-3 * corners[0])), "done": float((st == _hip.BLEND_DONE).mean()),
             "sample_bytes": nbytes, "probe_GB_per_s": probe}
        return {k: (round(v, 4) if isinstance(v, float) and abs(v) < 1e4 else float(f"{v:.4e}") if isinstance(v, float) else v)
                for k, v in r.items()}
    finally:
        for b in (dw, dc, *bufs.values()):
            b.free()


def main():
    import blend_cases as bc

    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=512)
    ap.add_argument("--grid", type=int, default=129)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--robots", default="ur5,panda,chain3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blend_bench.json"))
    args = ap.parse_args()
    ctx = _hip.HipContext(0)
    props = ctx.properties()
    res = {"device": (props.get("name") or "unknown").strip("() "), "reps": args.reps, "statistic": "median after one warm-up",
           "margin": bc.RUNS["base"], "tol": bc.TOL, **bc.params_of(), "robots": {}}
    for name in args.robots.split(","):
        case = bc.make_blend_case(name)
        cm, wp, cnt = case["cm"], case["waypoints"], case["count"]
        res["robots"][name] = {"n": cm.n, "spheres": int(len(cm.links)),
                               "cases": _run(ctx, cm, wp, cnt, bc.GRID, args.reps, bc),
                               "batch": _run(ctx, cm, np.tile(wp, (args.copies, 1, 1)), np.tile(cnt, args.copies), args.grid, args.reps, bc)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
