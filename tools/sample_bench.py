#!/usr/bin/env python3
"""Times of the trajectory-sampling launch k_traj_sample (csrc/mp_sample.h) on one GPU, device arrays.

    python tools/sample_bench.py [--B 131072] [--N 100] [--rows 100,1000] [--copies 512] [--grid 129] [--reps 5]
                                 [--robots xarm6,panda] [--curve-robots ur5,panda,chain3] [--out FILE]

Prints one JSON line and writes it to --out (profiles/sample_bench.json unless given).
Grid source: the paths of tools/toppra_bench.py (DESIGN 4.8's case) - 2048 distinct ones, timed by mp_toppra_host_f64 under the URDF's
velocity and effort limits, repeated to --B paths (a path's result depends on its content only) - at a dt that gives the longest path
each of --rows rows (M = that many).  Curve source: the 139 problems of tests/blend_cases.py (base run) blended at N = --grid, timed
with velocity limits 2 and acceleration limits 40, --copies copies, 100 rows.  Per configuration:
  fused_ms      mp_trajectory_sample_f64 with every output, the torques among them, in one launch - up to 6 joints, where the entry
                has that form; from 7 joints on it no longer dispatches the torque instances and this is entry_ms again;
  plain_ms      the same without the torques;
  id_ms         mp_id_trajectory_f64 over the B M rows the plain launch wrote;
  split_ms      the plain launch and the inverse-dynamics launch, timed together: the split form;
  entry_ms      the same call as fused_ms as the entry runs it by itself (fused up to 6 joints, split from 7 on);
  bytes         what the fused launch writes, (4 n + 3) doubles a row;
  probe_GB_per_s  a write-only streaming probe of `bytes` in the same process (mp_stream_bandwidth_mix, 0 reads : 1 write,
                non-temporal), and `of_probe` = bytes / fused_ms against it.
Every time is the median of single launches timed one by one between HIP events after a warm-up launch, with min, max and the launch
count.  Without a device the tool fails: it has no other path.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from manipulapy_amd import _hip  # noqa: E402

UNIQUE = 2048
G = np.array([0.0, 0.0, -9.81])


def _time(ctx, fn, reps, window_ms=300.0, cap=40):
    """(median, min, max, launches) in ms, as tools/toppra_bench.py takes them"""
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
    a.destroy()
    b.destroy()
    return float(np.median(t)), float(t.min()), float(t.max()), n


def _measure(ctx, model, t, x, dt, M, reps, path=None, curve=None):
    """one configuration: host arrays up, the four timings, the probe"""
    B, N = t.shape
    n = model.n
    ins = {"d_t": ctx.to_device(t), "d_x": ctx.to_device(x)}
    w_in = 0
    if path is not None:
        for k, a in zip(("d_q", "d_dq", "d_ddq"), path):
            ins[k] = ctx.to_device(a)
    else:
        w_in = curve["points"].shape[1]
        names = {"status": "d_blend_status", "count": "d_blend_count"}
        for k in _hip.SAMPLE_CURVE_TABLES:
            ins[names.get(k, "d_" + k)] = ctx.to_device(np.ascontiguousarray(curve[k], dtype=np.int32 if k in names else np.float64))
    rows = B * M
    size = {"status": 4 * B, "count": 4 * B, "needed": 4 * B, "s": 8 * rows, "sd": 8 * rows, "sdd": 8 * rows}
    outs = {k: ctx.alloc(size.get(k, 8 * rows * n)) for k in _hip.SAMPLE_OUTPUTS}
    extra = {k: v for k, v in ins.items() if k not in ("d_t", "d_x")}
    try:
        def sample(keys):
            ctx.trajectory_sample(model, ins["d_t"], ins["d_x"], B, N, dt, M, w_in=w_in, g=G, **extra, **{"d_" + k: outs[k] for k in keys})

        plain_keys = tuple(k for k in _hip.SAMPLE_OUTPUTS if k != "torques")
        plain = lambda: sample(plain_keys)  # noqa: E731
        ident = lambda: ctx.id_trajectory(model, outs["positions"], outs["velocities"], outs["accelerations"], rows, outs["torques"], g=G,  # noqa: E731
                                          dtype=np.float64)

        def split():
            plain()
            ident()

        r = {"paths": B, "grid": N, "rows": M, "n": n, "dt": dt}
        def fused():   # every output in one call: the fused kernel up to 6 joints, the entry's split form beyond
            sample(_hip.SAMPLE_OUTPUTS)

        for key, fn in (("fused", fused), ("plain", plain), ("id", ident), ("split", split), ("entry", lambda: sample(_hip.SAMPLE_OUTPUTS))):
            r[f"{key}_ms"], r[f"{key}_min_ms"], r[f"{key}_max_ms"], r[f"{key}_launches"] = _time(ctx, fn, reps)
        st = outs["status"].download((B,), np.int32)
        cnt = outs["count"].download((B,), np.int32)
        r["ok"] = float((st == _hip.SAMPLE_OK).mean())
        r["mean_count"] = float(cnt.mean())
        r["bytes"] = nbytes = rows * (4 * n + 3) * 8
        r["probe_GB_per_s"] = probe = float(ctx.stream_bandwidth_mix(nbytes, 0, 1, reps=reps, nontemporal=True))
        r["fused_GB_per_s"] = nbytes / (1e-3 * r["fused_ms"]) / 1e9
        r["of_probe"] = r["fused_GB_per_s"] / probe
        r["fused_over_split"] = r["fused_ms"] / r["split_ms"]
        return {k: (float(f"{v:.5g}") if isinstance(v, float) else v) for k, v in r.items()}
    finally:
        for b in (*ins.values(), *outs.values()):
            b.free()


def main():
    import blend_cases as bc
    import toppra_bench as tb

    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=131072)
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--rows", default="100,1000")
    ap.add_argument("--copies", type=int, default=512)
    ap.add_argument("--grid", type=int, default=129)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--robots", default="xarm6,panda")
    ap.add_argument("--curve-robots", default="ur5,panda,chain3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_bench.json"))
    args = ap.parse_args()
    ctx = _hip.HipContext(0)
    props = ctx.properties()
    res = {"device": (props.get("name") or "unknown").strip("() "), "reps": args.reps, "statistic": "median of single launches after one warm-up",
           "grid_source": {}, "curve_source": {}}
    for name in [r for r in args.robots.split(",") if r]:
        model, lim, vlim, tlim = tb._model(name)
        U = min(UNIQUE, args.B)
        q, dq, ddq = (np.ascontiguousarray(np.swapaxes(a, 0, 1)) for a in tb._paths(lim, U, args.N))
        timing = ctx.toppra_host(model, q, dq, ddq, vlim, tlim, None, g=G, want_rows=False)
        assert not timing["status"].any()
        rep = -(-args.B // U)
        tile = lambda a: np.ascontiguousarray(np.tile(a, (rep,) + (1,) * (a.ndim - 1))[:args.B])  # noqa: E731
        t, x, path = tile(timing["time"]), tile(timing["sd2"]), tuple(tile(a) for a in (q, dq, ddq))
        res["grid_source"][name] = {}
        for rows in [int(r) for r in args.rows.split(",")]:
            dt = float(timing["duration"].max() / (rows - 1))
            M = int(_hip.sample_rows_needed(timing["duration"], dt).max())
            res["grid_source"][name][str(rows)] = _measure(ctx, model, t, x, dt, M, args.reps, path=path)
    for name in [r for r in args.curve_robots.split(",") if r]:
        case = bc.make_blend_case(name)
        cm = case["cm"]
        n = cm.n
        cm.sync_world(ctx)
        bl = ctx.path_blend_arrays(cm.model, cm.handle, case["waypoints"], case["count"], args.grid, bc.RUNS["base"], bc.TOL, **bc.params_of())
        live = np.flatnonzero((bl["status"] == _hip.BLEND_DONE) | (bl["status"] == _hip.BLEND_STRAIGHT))
        part = ctx.toppra_host(cm.model, bl["q"][live], bl["dq"][live], bl["ddq"][live], np.full(n, 2.0), np.tile([-np.inf, np.inf], (n, 1)),
                               np.full(n, 40.0), g=G, want_rows=False)
        t, x = np.full((len(bl["status"]), args.grid), np.nan), np.full((len(bl["status"]), args.grid), np.nan)
        t[live], x[live] = part["time"], part["sd2"]
        dur = part["duration"][np.isfinite(part["duration"])]
        dt = float(np.median(dur) * 2 / 99)
        M = 100
        tile = lambda a: np.ascontiguousarray(np.tile(a, (args.copies,) + (1,) * (a.ndim - 1)))  # noqa: E731
        curve = {k: tile(bl[k]) for k in _hip.SAMPLE_CURVE_TABLES}
        res["curve_source"][name] = _measure(ctx, cm.model, tile(t), tile(x), dt, M, args.reps, curve=curve)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
