#!/usr/bin/env python3
"""Throughput of the analytical derivative kernels (csrc/mp_deriv.h) against the obvious alternative, on one GPU.

    python tools/derivatives_bench.py [--rows 4000000] [--reps 10] [--valu-csv counter_collection.csv] [--issue-cyc 5.55]

Prints one JSON line.  Per robot (UR5 n = 6, Panda n = 8) and per entry (inverse / forward dynamics derivatives, the two required
outputs dtau_dq / dtau_dqd or dqdd_dq / dqdd_dqd):
  ms per launch, rows/s; algorithmic bytes (inputs + outputs) and their fraction of the 8 TB/s peak;
  VALU instructions per row (SQ_INSTS_VALU x 64 / rows from a counter-only rocprofv3 run, --valu-csv) and the fraction of the f64
  issue ceiling that implies - the ceiling in cycles per wave-instruction per SIMD at the kernels' occupancy comes from
  tools/ubench_valu.hip (--issue-cyc), the clock from the device's peak;
  the same rows' time of finite differences: 2n + 1 launches of mp_id_trajectory_f64 (forward) and 4n (central);
  accuracy of all three against the reference's autograd Jacobians (tests/golden/derivatives.npz: max |err| / max |J|);
  the CPU twin's rate on 16 threads.
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from manipulapy_amd import _hip, robots  # noqa: E402

PEAK_BPS = 8.0e12
CLOCK_HZ = 2.4e9
CUS = 256


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


def _valu_per_row(path, kernel_key, rows):
    if not path:
        return None
    best = 0.0   # the largest dispatch of the kernel: the full-size launch (the accuracy pass launches it on single rows too)
    with open(path) as f:
        for r in csv.DictReader(f):
            if kernel_key in r.get("Kernel_Name", "") and r.get("Counter_Name") == "SQ_INSTS_VALU":
                best = max(best, float(r["Counter_Value"]))
    return None if best == 0 else best * 64.0 / rows


def _fd_jac(ctx, m, q, qd, qdd, g, F, h, central):
    """dtau_dq, dtau_dqd by differences of the product's own float64 inverse dynamics (host rows)."""
    n = q.shape[1]
    f = lambda a, b: ctx.id_trajectory_host(m, a, b, qdd, g, F, dtype=np.float64)  # noqa: E731
    base = None if central else f(q, qd)
    out = []
    for which in (0, 1):
        J = np.empty((q.shape[0], n, n))
        for j in range(n):
            e = np.zeros(n); e[j] = h
            a = [q, qd]
            p = [x + e if k == which else x for k, x in enumerate(a)]
            if central:
                mm = [x - e if k == which else x for k, x in enumerate(a)]
                J[:, :, j] = (f(*p) - f(*mm)) / (2 * h)
            else:
                J[:, :, j] = (f(*p) - base) / h
        out.append(J)
    return out


def _rel(got, want):
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--valu-csv", default=None)
    ap.add_argument("--valu-rows", type=int, default=None, help="rows of the counter run's launches (default: --rows)")
    ap.add_argument("--issue-cyc", type=float, default=None, help="f64 FMA cycles per wave-instruction per SIMD at this occupancy")
    ap.add_argument("--robots", default="ur5,panda")
    ap.add_argument("--cpu-threads", type=int, default=16)
    args = ap.parse_args()
    ctx = _hip.HipContext(0)
    gold = np.load(os.path.join(ROOT, "tests", "golden", "derivatives.npz"))
    res = {"rows": args.rows, "reps": args.reps, "device": ctx.properties()["name"], "robots": {}}
    g, F = np.array([0.0, 0.0, -9.81]), np.array([1.0, -2.0, 0.5, 3.0, -1.5, 0.75])
    for name in args.robots.split(","):
        m = _model(name)
        n, R = m.n, args.rows
        rng = np.random.default_rng(0)
        lim = robots.robot_tables(name)["joint_limits"]
        x = [rng.uniform(lim[:, 0], lim[:, 1], (R, n)), rng.uniform(-1, 1, (R, n)), rng.uniform(-1, 1, (R, n))]
        d = [ctx.to_device(a) for a in x]
        o = [ctx.alloc(R * n * n * 8) for _ in range(2)]
        r = {"n": n}
        for key, fn, kern in (("id", ctx.id_derivatives, "k_id_deriv"), ("fd", ctx.fd_derivatives, "k_fd_deriv")):
            ms = _time(ctx, lambda: fn(m, d[0], d[1], d[2], R, o[0], o[1], g=g, Ftip=F), args.reps)
            nbytes = R * (3 * n + 2 * n * n) * 8
            e = {"ms": round(ms, 4), "rows_per_s": R / ms * 1e3, "bytes": nbytes, "bytes_per_row": nbytes // R,
                 "frac_peak_hbm": round(nbytes / (ms * 1e-3) / PEAK_BPS, 4)}
            v = _valu_per_row(args.valu_csv, f"{kern}<{n}", args.valu_rows or R)
            if v is not None:
                e["valu_per_row"] = round(v, 1)
                if args.issue_cyc:
                    ceiling_rows = CUS * 4 * CLOCK_HZ / args.issue_cyc * 64 / v
                    e["valu_ceiling_rows_per_s"] = ceiling_rows
                    e["frac_valu_ceiling"] = round((R / ms * 1e3) / ceiling_rows, 4)
            r[key] = e
        # finite differences of the float64 ID kernel on the same rows: every perturbed input prepared before the clock starts
        tau = [ctx.alloc(R * n * 8) for _ in range(4 * n + 1)]
        hq = 1e-6
        pert = []
        for which in (0, 1):
            for j in range(n):
                for s in (1.0, -1.0):
                    y = x[which].copy(); y[:, j] += s * hq
                    pert.append((which, ctx.to_device(y)))

        def launches(central):
            k = 0
            if not central:
                ctx.id_trajectory(m, d[0], d[1], d[2], R, tau[-1], g, F, dtype=np.float64)
            for idx, (which, buf) in enumerate(pert):
                if not central and idx % 2:
                    continue
                a = [buf if w == which else d[w] for w in range(3)]
                ctx.id_trajectory(m, a[0], a[1], a[2], R, tau[k], g, F, dtype=np.float64)
                k += 1
        r["fd_forward_launches"] = 2 * n + 1
        r["fd_forward_ms"] = round(_time(ctx, lambda: launches(False), args.reps), 4)
        r["fd_central_launches"] = 4 * n
        r["fd_central_ms"] = round(_time(ctx, lambda: launches(True), args.reps), 4)
        for b in tau + [p[1] for p in pert] + d + o:
            b.free()
        # accuracy against the reference's autograd Jacobians (25 fixture rows)
        z = np.load(os.path.join(ROOT, "tests", "golden", f"dynamics_{name}.npz"))
        acc = {"analytic": 0.0, "fd_forward": 0.0, "fd_central": 0.0}
        for i in range(z["thetas"].shape[0]):
            sl = slice(i, i + 1)
            q, qd, qdd, Fi = z["thetas"][sl], z["dthetas"][sl], z["ddthetas"][sl], z["ftips"][i]
            want = (gold[f"{name}_id_dq"][sl], gold[f"{name}_id_dqd"][sl])
            _, aq, aqd, _ = ctx.id_derivatives_host(m, q, qd, qdd, z["g"], Fi)
            fw = _fd_jac(ctx, m, q, qd, qdd, z["g"], Fi, 1.5e-8, False)
            ce = _fd_jac(ctx, m, q, qd, qdd, z["g"], Fi, 6e-6, True)
            for k, got in (("analytic", (aq, aqd)), ("fd_forward", fw), ("fd_central", ce)):
                acc[k] = max(acc[k], _rel(got[0], want[0]), _rel(got[1], want[1]))
        r["max_rel_err_vs_reference_autograd"] = acc
        # the CPU twin
        Rc = 200_000
        t0 = time.perf_counter()
        _hip.cpu_id_derivatives(m, x[0][:Rc], x[1][:Rc], x[2][:Rc], g, F, nthreads=args.cpu_threads)
        r["cpu_twin_id_rows_per_s"] = Rc / (time.perf_counter() - t0)
        r["cpu_threads"] = args.cpu_threads
        r["speedup_vs_fd_forward"] = round(r["fd_forward_ms"] / r["id"]["ms"], 3)
        res["robots"][name] = r
    print(json.dumps(res), flush=True)
    ctx.destroy()


if __name__ == "__main__":
    main()
