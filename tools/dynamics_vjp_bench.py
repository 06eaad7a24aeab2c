#!/usr/bin/env python3
"""Throughput of the reverse-mode vector-Jacobian kernels (csrc/mp_adjoint.h) against the Jacobian route, on one GPU.

    python tools/dynamics_vjp_bench.py [--rows 4000000] [--reps 7] [--torch-rows 1000000] [--valu-csv counter_collection.csv]
                                       [--issue-cyc 5.55] [--no-torch]

Prints one JSON line.  Per robot (UR5 n = 6, Panda n = 8; g and a tip wrench) and per direction (inverse / forward dynamics), the
median over --reps timed launches after a warm-up launch:
  vjp_ms:              k_id_vjp / k_fd_vjp (mp_{id,fd}_vjp_f64: gq, gqd and gqdd / gtau);
  jac_contract_ms:     mp_{id,fd}_derivatives_f64 (the two (rows, n, n) Jacobians + M / M^-1) followed by three torch.bmm
                       contractions with the cotangent on the device - the same three gradients the Jacobian way;
  VALU instructions per row (SQ_INSTS_VALU x 64 / rows of a counter-only rocprofv3 run, --valu-csv) and the fraction of the f64
  issue ceiling that implies (--issue-cyc as in tools/derivatives_bench.py).
Then one torch forward + backward (mpa.forward_dynamics / inverse_dynamics, --torch-rows rows): device tensors (this route) against
CPU tensors under the "hip" backend (the CPU-tensor route: host rows, Jacobians copied back, np.einsum).
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
import torch  # noqa: E402  (first: the HIP runtime torch loads serves the library too)

import manipulapy_amd as mp  # noqa: E402
from manipulapy_amd import _hip, registry, robots  # noqa: E402

CLOCK_HZ = 2.4e9
CUS = 256


def _model(name):
    t = robots.robot_tables(name)
    return _hip.HipModel(t["S_list"], t["Mlist_per_link"], t["Glist"], t["M_ee"], t["joint_limits"])


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


def _wall_median_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def _valu_per_row(path, kernel_key, rows):
    if not path:
        return None
    best = 0.0
    with open(path) as f:
        for r in csv.DictReader(f):
            if kernel_key in r.get("Kernel_Name", "") and r.get("Counter_Name") == "SQ_INSTS_VALU":
                best = max(best, float(r["Counter_Value"]))
    return None if best == 0 else best * 64.0 / rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--torch-rows", type=int, default=1_000_000)
    ap.add_argument("--valu-csv", default=None)
    ap.add_argument("--valu-rows", type=int, default=None)
    ap.add_argument("--issue-cyc", type=float, default=5.55)
    ap.add_argument("--robots", default="ur5,panda")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-jacobian", action="store_true")
    args = ap.parse_args()
    ctx = registry.get_context()
    res = {"rows": args.rows, "reps": args.reps, "statistic": "median after one warm-up", "device": ctx.properties()["name"],
           "robots": {}}
    g, F = np.array([0.0, 0.0, -9.81]), np.array([1.0, -2.0, 0.5, 3.0, -1.5, 0.75])
    dev = torch.device("cuda", ctx.device_id)
    for name in args.robots.split(","):
        m = _model(name)
        n, R = m.n, args.rows
        rng = np.random.default_rng(0)
        lim = robots.robot_tables(name)["joint_limits"]
        x = [torch.tensor(a, device=dev) for a in (rng.uniform(lim[:, 0], lim[:, 1], (R, n)), rng.uniform(-1, 1, (R, n)),
                                                   rng.uniform(-1, 1, (R, n)), rng.normal(size=(R, n)))]
        p = [t.data_ptr() for t in x]
        outs = [torch.empty((R, n), dtype=torch.float64, device=dev) for _ in range(4)]
        o = [t.data_ptr() for t in outs]
        torch.cuda.synchronize()
        r = {"n": n}
        for key, kern in (("id", "k_id_vjp"), ("fd", "k_fd_vjp")):
            if key == "id":
                launch = lambda: ctx.id_vjp(m, p[0], p[1], p[2], p[3], R, o[0], o[1], o[2], g=g, Ftip=F)  # noqa: E731
            else:
                launch = lambda: ctx.fd_vjp(m, p[0], p[1], p[2], p[3], R, o[0], o[1], d_gtau=o[2], g=g, Ftip=F)  # noqa: E731
            e = {"vjp_ms": round(_median_ms(ctx, launch, args.reps), 4)}
            e["vjp_rows_per_s"] = R / e["vjp_ms"] * 1e3
            v = _valu_per_row(args.valu_csv, f"{kern}<{n}", args.valu_rows or R)
            if v is not None:
                e["valu_per_row"] = round(v, 1)
                ceiling = CUS * 4 * CLOCK_HZ / args.issue_cyc * 64 / v
                e["valu_ceiling_rows_per_s"] = ceiling
                e["frac_valu_ceiling"] = round(e["vjp_rows_per_s"] / ceiling, 4)
            r[key] = e
        if not args.no_jacobian:
            J = [torch.empty((R, n, n), dtype=torch.float64, device=dev) for _ in range(3)]
            s = ctx.stream()   # (a measurement process: handing the stream out is fine here)
            torch.cuda.synchronize()
            lam = x[3].unsqueeze(1)
            for key in ("id", "fd"):
                def jac_route(key=key):
                    fn = ctx.id_derivatives if key == "id" else ctx.fd_derivatives
                    kw = {"d_M": J[2].data_ptr()} if key == "id" else {"d_Minv": J[2].data_ptr()}
                    fn(m, p[0], p[1], p[2], R, J[0].data_ptr(), J[1].data_ptr(), g=g, Ftip=F, **kw)
                    with torch.cuda.stream(torch.cuda.ExternalStream(s)):
                        for k in range(3):
                            torch.bmm(lam, J[k], out=outs[k].view(R, 1, n))
                r[key]["jac_contract_ms"] = round(_median_ms(ctx, jac_route, args.reps), 4)
                r[key]["speedup_vs_jac_contract"] = round(r[key]["jac_contract_ms"] / r[key]["vjp_ms"], 3)
            del J
        res["robots"][name] = r
        del x, outs
        torch.cuda.empty_cache()
    if not args.no_torch:
        from manipulapy_amd import autograd as mpa

        sm, dyn, _ = mp.load_robot("panda")
        T = args.torch_rows
        rng = np.random.default_rng(1)
        arrs = [rng.uniform(-1, 1, (T, 8)) for _ in range(3)]
        base = {d: [torch.tensor(a, device=d) for a in arrs] for d in (dev, "cpu")}
        tr = {"robot": "panda", "rows": T, "statistic": "wall-clock median, inputs already in place"}
        for kind, fn in (("inverse", mpa.inverse_dynamics), ("forward", mpa.forward_dynamics)):
            def step(device):
                ins = [b.detach().requires_grad_(True) for b in base[device]]
                fn(dyn, *ins, g, F).sum().backward()
                return ins[0].grad

            dev_ms = _wall_median_ms(lambda: step(dev), args.reps)
            with mp.use_backend("hip"):
                cpu_ms = _wall_median_ms(lambda: step("cpu"), max(3, args.reps // 2))
            tr[kind] = {"device_tensors_ms": round(dev_ms, 3), "cpu_tensors_ms": round(cpu_ms, 3),
                        "speedup": round(cpu_ms / dev_ms, 2)}
        res["torch_forward_backward"] = tr
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
