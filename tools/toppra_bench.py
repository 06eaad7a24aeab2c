#!/usr/bin/env python3
"""Times of the time-optimal path parameterisation (csrc/mp_toppra.h), split into its launches, on one GPU.

    python tools/toppra_bench.py [--B 131072] [--N 100] [--reps 3] [--robots xarm6,panda] [--out profiles/r13_toppra_bench.json]

Prints one JSON line and writes it to --out (profiles/r13_toppra_bench.json unless given).  Per robot, B paths q(s) = q0 + s D + A sin^2(pi s) of N grid points (the paths of
tests/toppra_cases.py), the URDF's own velocity and effort limits, sd = 0 at both ends, time-major device arrays:
  id3_ms          three mp_id_trajectory_f64 launches over the same N B rows - (q, 0, q'), (q, q', q''), (q, 0, 0) - the form the fused
                  coefficient pass replaces (gravity is not switched off per launch: the time does not depend on it), same process;
  coeffs_ms       mp_path_dynamics_f64 (k_path_coeffs), one launch;
  sweep_ms        mp_toppra_tm_f64 without row outputs (k_toppra_sweep): backward and forward pass;
  sweep_acc_ms    the same with acceleration limits (2 n more rows an LP, q' and q'' read as well);
  rows_ms         the row-parallel epilogue k_path_rows alone, NOT timed itself: the difference of the medians sweep_rows_ms - sweep_ms;
  sweep_fused_ms  mp_toppra_tm_f64 with the three row outputs: the forward pass writes the rows - what ships;
  sweep_rows_ms   the same call under MANIPULAPY_HIP_TOPPRA_EPILOGUE=separate: the epilogue as a launch of its own behind the sweep;
  total_ms        coeffs_ms + sweep_fused_ms, and the ratios named in the keys.
Every time is the median of single launches timed one by one after a warm-up launch; *_min_ms / *_max_ms / *_launches give the spread.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from manipulapy_amd import _hip, robots  # noqa: E402
from manipulapy_amd.urdf import extract_tables  # noqa: E402


def _model(name):
    t = robots.robot_tables(name)
    lim = np.asarray(t["joint_limits"], dtype=np.float64)
    u = extract_tables(robots.robot_urdf(name))
    eff = np.asarray(u["effort_limits"], dtype=np.float64)
    return (_hip.HipModel(t["S_list"], t["Mlist_per_link"], t["Glist"], t["M_ee"], lim), lim, np.asarray(u["velocity_limits"], dtype=np.float64),
            np.stack([-eff, eff], axis=1))


def _paths(lim, B, N, seed=7):
    """(N, B, n) time-major q, q', q'' of the test paths."""
    n = lim.shape[0]
    rng = np.random.default_rng(seed)
    mid, half = 0.5 * (lim[:, 0] + lim[:, 1]), np.minimum(0.5 * (lim[:, 1] - lim[:, 0]), 1.5)
    q0 = mid + rng.uniform(-1, 1, (B, n)) * half
    D = (mid + rng.uniform(-1, 1, (B, n)) * half - q0)[None]
    A = rng.uniform(-0.2, 0.2, (B, n))[None]
    s = (np.arange(N, dtype=np.float64) / (N - 1))[:, None, None]
    return (q0[None] + s * D + A * np.sin(np.pi * s) ** 2, D + A * np.pi * np.sin(2 * np.pi * s),
            A * 2 * np.pi ** 2 * np.cos(2 * np.pi * s) + 0.0 * D)


def _time(ctx, fn, reps, window_ms=400.0, cap=60):
    """(median, min, max, launches) in ms: one warm-up launch, then each launch timed on its own with hipEvents; short kernels get more
    launches than `reps`, enough to fill `window_ms`."""
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
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=131072)
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--robots", default="xarm6,panda")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_toppra_bench.json"))
    args = ap.parse_args()
    ctx = _hip.HipContext(0)
    B, N = args.B, args.N
    g = np.array([0.0, 0.0, -9.81])
    props = ctx.properties()
    device = (props.get("name") or "").strip()
    if not device or device.startswith("("):
        device = device.strip("() ") or "unknown"
    res = {"B": B, "N": N, "reps": args.reps, "device": device, "epilogue_variant": "fused (the forward pass writes the rows)", "robots": {}}
    for name in args.robots.split(","):
        m, lim, vlim, tlim = _model(name)
        n = m.n
        bufs = []

        def keep(b):
            bufs.append(b)
            return b

        rows, col = N * B * n * 8, N * B * 8
        d_q, d_dq, d_ddq = (keep(ctx.to_device(a)) for a in _paths(lim, B, N))
        d_zero = keep(ctx.alloc(rows))
        ctx.memset(d_zero, 0, rows)
        d_a, d_b, d_c, d_xb = keep(ctx.alloc(rows)), keep(ctx.alloc(rows)), keep(ctx.alloc(rows)), keep(ctx.alloc(col))
        d_s0, d_s1 = keep(ctx.to_device(np.zeros(B))), keep(ctx.to_device(np.zeros(B)))
        d_K, d_x, d_u, d_t = keep(ctx.alloc(2 * col)), keep(ctx.alloc(col)), keep(ctx.alloc(col)), keep(ctx.alloc(col))
        d_dur, d_st = keep(ctx.alloc(B * 8)), keep(ctx.alloc(B * 4))
        d_o = [keep(ctx.alloc(rows)) for _ in range(3)]
        r = {"n": n}

        def put(key, t):
            r[f"{key}_ms"], r[f"{key}_min_ms"], r[f"{key}_max_ms"], r[f"{key}_launches"] = t

        def id3():
            ctx.id_trajectory(m, d_q, d_zero, d_dq, N * B, d_o[0], g=g, dtype=np.float64)
            ctx.id_trajectory(m, d_q, d_dq, d_ddq, N * B, d_o[1], g=g, dtype=np.float64)
            ctx.id_trajectory(m, d_q, d_zero, d_zero, N * B, d_o[2], g=g, dtype=np.float64)

        def sweep(alim=None, outs=(None, None, None)):
            ctx.toppra(m, d_a, d_b, d_c, d_xb, d_dq, d_ddq, tlim, alim, d_s0, d_s1, B, N, d_K, d_x, d_u, d_t, d_dur, d_st, *outs)

        put("id3", _time(ctx, id3, args.reps))
        put("coeffs", _time(ctx, lambda: ctx.path_dynamics(m, d_q, d_dq, d_ddq, N * B, vlim, d_a, d_b, d_c, d_xb, g), args.reps))
        put("sweep", _time(ctx, sweep, args.reps))
        st = d_st.download((B,), np.int32)
        dur = d_dur.download((B,), np.float64)
        r["status_nonzero"] = int((st != 0).sum())
        r["duration_median_s"] = float(np.median(dur[st == 0]))
        os.environ["MANIPULAPY_HIP_TOPPRA_EPILOGUE"] = "separate"
        put("sweep_rows", _time(ctx, lambda: sweep(None, d_o), args.reps))
        os.environ.pop("MANIPULAPY_HIP_TOPPRA_EPILOGUE")
        tau_sep = d_o[2].download((N, B, n), np.float64)
        put("sweep_fused", _time(ctx, lambda: sweep(None, d_o), args.reps))
        tau_fused = d_o[2].download((N, B, n), np.float64)
        fine = st == 0
        r["epilogue_variants_tau_max_diff"] = float(np.abs(tau_sep[:, fine] - tau_fused[:, fine]).max())
        del tau_sep, tau_fused
        acc = d_o[1].download((N, B, n), np.float64)
        alim = np.maximum(np.abs(acc[:-1][:, fine]).max(axis=(0, 1)) / 3.0, 1e-3)
        del acc
        put("sweep_acc", _time(ctx, lambda: sweep(alim), args.reps))
        r["status_nonzero_acc"] = int((d_st.download((B,), np.int32) != 0).sum())
        r["rows_ms"] = r["sweep_rows_ms"] - r["sweep_ms"]
        r["total_ms"] = r["coeffs_ms"] + r["sweep_fused_ms"]
        r["coeffs_over_id3"] = r["coeffs_ms"] / r["id3_ms"]
        r["sweep_over_coeffs"] = r["sweep_ms"] / r["coeffs_ms"]
        r["sweep_fused_over_sweep_rows"] = r["sweep_fused_ms"] / r["sweep_rows_ms"]
        for k, v in list(r.items()):
            if isinstance(v, float):
                r[k] = round(v, 4) if abs(v) > 1e-3 else float(f"{v:.3e}")
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
