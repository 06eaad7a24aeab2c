#!/usr/bin/env python3
"""Time of the roll-out gradient kernel (csrc/mp_rollout_vjp.h) against the forward roll-out and the alternatives, on one GPU.

    python tools/rollout_vjp_bench.py [--B 131072] [--N 100] [--intRes 1] [--reps 5] [--robots xarm6,panda] [--out FILE]

Prints one JSON line (and writes it to --out).  Per robot, at config c5's shape (B trajectories of N steps, dt 0.01, per-step wrench,
time-major device arrays, float64 state):
  vjp_ms             mp_fd_trajectory_vjp_tm_f64 with all three cotangents;
  forward_f64_ms     mp_fd_trajectory_tm_f64 on the same inputs (same process), and vjp / forward;
  forward_f32_ms     mp_fd_trajectory_tm_f32 (the robot-specialised float32 roll-out bench.py's c5 runs, when hiprtc is there);
  deriv_ceiling_ms   one mp_fd_derivatives_f64 launch over B N intRes rows - the per-sub-step work the reverse pass repeats, the
                     expected ceiling of this design;
  fwd_diff_ms        the forward-difference alternative priced from the float64 roll-out: ((N - 1) n + 2n + 1) roll-outs.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from manipulapy_amd import _hip, robots  # noqa: E402


def _model(name):
    t = robots.robot_tables(name)
    return _hip.HipModel(t["S_list"], t["Mlist_per_link"], t["Glist"], t["M_ee"], t["joint_limits"])


def _time(ctx, fn, reps):
    fn()
    ctx.synchronize()
    a, b = _hip.HipEvent(ctx), _hip.HipEvent(ctx)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    ctx.synchronize()
    ms = b.elapsed_ms_since(a) / reps
    a.destroy(); b.destroy()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=131072)
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--intRes", type=int, default=1)
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--robots", default="xarm6,panda")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = _hip.HipContext(0)
    B, N, R, dt = args.B, args.N, args.intRes, args.dt
    g = np.array([0.0, 0.0, -9.81])
    res = {"B": B, "N": N, "intRes": R, "dt": dt, "reps": args.reps, "device": ctx.properties()["name"], "robots": {}}
    for name in args.robots.split(","):
        m = _model(name)
        n = m.n
        rng = np.random.default_rng(0)
        th, dth = rng.uniform(-0.5, 0.5, (B, n)), rng.uniform(-0.2, 0.2, (B, n))
        tm, F = rng.uniform(-1, 1, (N, B, n)), rng.uniform(-1, 1, (N, B, 6))
        bufs = []

        def keep(b):
            bufs.append(b)
            return b

        d_th, d_dth, d_tm, d_F = (keep(ctx.to_device(a)) for a in (th, dth, tm, F))
        d_G = [keep(ctx.to_device(rng.uniform(-1, 1, (N, B, n)))) for _ in range(3)]
        d_o = [keep(ctx.alloc(B * n * 8)), keep(ctx.alloc(B * n * 8)), keep(ctx.alloc(N * B * n * 8))]
        wbytes = _hip.fd_trajectory_vjp_workspace_bytes(m, B, N, R)
        d_w = keep(ctx.alloc(wbytes))
        r = {"n": n, "workspace_bytes": wbytes}
        r["vjp_ms"] = _time(ctx, lambda: ctx.fd_trajectory_vjp(m, d_th, d_dth, d_tm, d_F, B, N, g, dt, R, *d_G, d_w, *d_o), args.reps)
        d_rows = [keep(ctx.alloc(N * B * n * 4)) for _ in range(3)]
        r["forward_f64_ms"] = _time(ctx, lambda: ctx.fd_trajectory(m, d_th, d_dth, d_tm, d_F, B, N, g, dt, R, *d_rows, dtype=np.float64,
                                                                   time_major=True), args.reps)
        r["vjp_over_forward_f64"] = r["vjp_ms"] / r["forward_f64_ms"]
        try:
            ctx.specialize(m)
            f32 = [keep(ctx.to_device(a.astype(np.float32))) for a in (th, dth, tm, F)]
            r["forward_f32_ms"] = _time(ctx, lambda: ctx.fd_trajectory(m, *f32, B, N, g, dt, R, *d_rows, dtype=np.float32,
                                                                       time_major=True), args.reps)
            r["vjp_over_forward_f32"] = r["vjp_ms"] / r["forward_f32_ms"]
        except Exception as exc:  # pragma: no cover - depends on the hiprtc installation
            r["forward_f32_error"] = str(exc)
        for b in d_rows:
            b.free()
        bufs = [b for b in bufs if b not in d_rows]
        rows = B * N * R
        q = [keep(ctx.to_device(rng.uniform(-1, 1, (rows, n)))) for _ in range(3)]
        jac = [keep(ctx.alloc(rows * n * n * 8)) for _ in range(2)]
        r["deriv_ceiling_ms"] = _time(ctx, lambda: ctx.fd_derivatives(m, q[0], q[1], q[2], rows, jac[0], jac[1]), args.reps)
        r["vjp_over_deriv_ceiling"] = r["vjp_ms"] / r["deriv_ceiling_ms"]
        launches = (N - 1) * n + 2 * n + 1
        r["fwd_diff_launches"] = launches
        r["fwd_diff_ms"] = launches * r["forward_f64_ms"]
        r["fwd_diff_over_vjp"] = r["fwd_diff_ms"] / r["vjp_ms"]
        r["traj_steps_per_s"] = B * N / (r["vjp_ms"] * 1e-3)
        for k, v in list(r.items()):
            if isinstance(v, float):
                r[k] = round(v, 4)
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
