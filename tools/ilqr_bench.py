#!/usr/bin/env python3
"""Time of one batched iLQR iteration (csrc/mp_ilqr.h), split into its parts, on one GPU.

    python tools/ilqr_bench.py [--B 131072] [--N 100] [--reps 3] [--robots xarm6,panda] [--out profiles/r12_ilqr_bench.json]

Prints one JSON line (and writes it to --out).  Per robot, B trajectories of N rows, dt 0.01, time-major device arrays, the weights and
the start of tests/ilqr_cases.py (gravity compensation as the nominal torque, a goal 0.3 rad away):
  deriv_ms        one mp_fd_derivatives_f64 launch over the (N - 1) B rows of the nominal - the yardstick of the same run;
  rollout_ms      mp_ilqr_rollout_tm_f64, A = 1, writing the float64 rows (the accepted step / the nominal);
  backward_ms     mp_ilqr_backward_tm_f64, the cooperative kernel that ships (16 lanes a trajectory, value matrix in LDS);
  backward_lane_ms  the same entry under MANIPULAPY_HIP_ILQR_BACKWARD=lane: one lane a trajectory, value matrix in a global workspace;
  linesearch_ms   mp_ilqr_rollout_tm_f64, A = 8 candidates, costs only;
  iteration_ms    their sum (with the shipped backward kernel), and every part over deriv_ms.
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


def _model(name):
    t = robots.robot_tables(name)
    lim = np.asarray(t["joint_limits"], dtype=np.float64)
    return _hip.HipModel(t["S_list"], t["Mlist_per_link"], t["Glist"], t["M_ee"], lim), lim


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
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--robots", default="xarm6,panda")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = _hip.HipContext(0)
    B, N, dt, A = args.B, args.N, args.dt, 8
    g = np.array([0.0, 0.0, -9.81])
    props = ctx.properties()
    device = (props.get("name") or "").strip()
    if not device or device.startswith("("):   # no marketing name on this driver: the architecture alone
        device = device.strip("() ") or "unknown"
    res = {"B": B, "N": N, "dt": dt, "reps": args.reps, "candidates": A, "device": device,
           "backward_variant": "cooperative (16 lanes a trajectory, LDS)", "robots": {}}
    for name in args.robots.split(","):
        m, lim = _model(name)
        n = m.n
        rng = np.random.default_rng(5)
        mid, half = 0.5 * (lim[:, 0] + lim[:, 1]), 0.5 * (lim[:, 1] - lim[:, 0])
        q0 = mid + rng.uniform(-0.5, 0.5, (B, n)) * np.minimum(half, 1.0)
        qd0 = rng.uniform(-0.5, 0.5, (B, n))
        goal = np.clip(q0 + rng.uniform(-0.3, 0.3, (B, n)), lim[:, 0], lim[:, 1])
        xref = np.zeros((N, B, 2 * n))
        xref[:, :, :n] = goal[None]
        z = np.zeros((B, n))
        tau = np.repeat(_hip.cpu_id_trajectory(m, q0, z, z, g, None, dtype=np.float64)[None], N, axis=0)
        w = (np.concatenate([np.full(n, 10.0), np.full(n, 1.0)]), np.full(n, 1e-2), np.concatenate([np.full(n, 1000.0), np.full(n, 10.0)]))
        bufs = []

        def keep(b):
            bufs.append(b)
            return b

        rows, blk = N * B * n * 8, (N - 1) * B * n * n * 8
        d_th, d_dth, d_tau, d_xr = (keep(ctx.to_device(a)) for a in (q0, qd0, tau, xref))
        d_pos, d_vel, d_tout = (keep(ctx.alloc(rows)) for _ in range(3))
        d_blk = [keep(ctx.alloc(blk)) for _ in range(3)]
        d_K, d_k = keep(ctx.alloc(2 * rows * n)), keep(ctx.alloc(rows))
        os.environ["MANIPULAPY_HIP_ILQR_BACKWARD"] = "lane"
        wbytes = _hip.ilqr_backward_workspace_bytes(m, B, N)
        os.environ.pop("MANIPULAPY_HIP_ILQR_BACKWARD")
        d_w = keep(ctx.alloc(wbytes))
        d_reg, d_dV, d_st = keep(ctx.to_device(np.full(B, 1e-6))), keep(ctx.alloc(2 * B * 8)), keep(ctx.alloc(4 * B))
        d_a1, d_a8 = keep(ctx.to_device(np.zeros((1, B)))), keep(ctx.to_device(np.repeat(2.0 ** -np.arange(8.0)[:, None], B, axis=1)))
        d_cost = keep(ctx.alloc(A * B * 8))
        d_p2, d_v2, d_t2 = (keep(ctx.alloc(rows)) for _ in range(3))
        # the nominal, once: open loop into (pos, vel)
        ctx.ilqr_rollout(m, d_th, d_dth, d_tau, None, None, None, None, d_a1, d_xr, *w, 1, B, N, g, dt, d_cost, d_pos, d_vel, d_tout)
        tau1 = d_tau.offset(B * n * 8)
        if (B * n) % 2:
            d_c = keep(ctx.alloc((N - 1) * B * n * 8))
            ctx.transpose_rows(tau1, 1, (N - 1) * B, n * 8, d_c)
            tau1 = d_c
        r = {"n": n, "lane_workspace_bytes": wbytes, "workspace_bytes": _hip.ilqr_backward_workspace_bytes(m, B, N)}

        def put(key, t):
            r[f"{key}_ms"], r[f"{key}_min_ms"], r[f"{key}_max_ms"], r[f"{key}_launches"] = t

        def backward():
            ctx.ilqr_backward(m, d_pos, d_vel, d_tau, *d_blk, d_xr, *w, d_reg, B, N, dt, d_w, d_K, d_k, d_dV, d_st)

        put("deriv", _time(ctx, lambda: ctx.fd_derivatives(m, d_pos, d_vel, tau1, (N - 1) * B, d_blk[0], d_blk[1], d_Minv=d_blk[2], g=g),
                           args.reps))
        os.environ["MANIPULAPY_HIP_ILQR_BACKWARD"] = "lane"
        put("backward_lane", _time(ctx, backward, args.reps))
        dV_lane = d_dV.download((B, 2), np.float64)
        os.environ.pop("MANIPULAPY_HIP_ILQR_BACKWARD")
        put("backward", _time(ctx, backward, args.reps))
        st, dV = d_st.download((B,), np.int32), d_dV.download((B, 2), np.float64)
        r["status_nonzero"] = int((st != 0).sum())
        fine = st == 0
        r["variants_dV_rel_diff"] = float(np.abs(dV[fine] - dV_lane[fine]).max() / np.abs(dV[fine]).max())
        put("linesearch", _time(ctx, lambda: ctx.ilqr_rollout(m, d_th, d_dth, d_tau, d_pos, d_vel, d_K, d_k, d_a8, d_xr, *w, A, B, N, g, dt,
                                                              d_cost), args.reps))
        d_one = keep(ctx.to_device(np.ones((1, B))))
        put("rollout", _time(ctx, lambda: ctx.ilqr_rollout(m, d_th, d_dth, d_tau, d_pos, d_vel, d_K, d_k, d_one, d_xr, *w, 1, B, N, g, dt,
                                                           d_cost, d_p2, d_v2, d_t2), args.reps))
        r["iteration_ms"] = r["deriv_ms"] + r["backward_ms"] + r["linesearch_ms"] + r["rollout_ms"]
        for part in ("rollout", "backward", "backward_lane", "linesearch", "iteration"):
            r[f"{part}_over_deriv"] = r[f"{part}_ms"] / r["deriv_ms"]
        r["backward_lane_over_backward"] = r["backward_lane_ms"] / r["backward_ms"]
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
