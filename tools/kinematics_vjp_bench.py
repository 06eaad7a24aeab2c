#!/usr/bin/env python3
"""Throughput of the reverse-mode kernel through FK + Jacobian (k_fk_jac_vjp, csrc/mp_kin_vjp.h), on one GPU.

    python tools/kinematics_vjp_bench.py [--rows 4000000] [--reps 7] [--torch-rows 1000000] [--robots ur5,panda] [--no-torch]

Prints one JSON line.  Per robot (UR5 n = 6, Panda n = 8) the median over --reps timed launches after a warm-up launch:
  vjp_ms[frame]:       mp_fk_jac_vjp_f64 with both cotangents, gq only (reads q, gT, gJ; writes gq), space and body frame;
  bytes, GB/s and the fraction of a same-run streaming probe with the nearest whole-array read/write mix (mp_stream_bandwidth_mix:
                       round(read bytes / write bytes) arrays read per array written, non-temporal);
  fk_jac_ms:           mp_fk_jac_id_f64 writing T + J alone at the same size, for scale;
  central_diff_ms:     today's alternative without this kernel: 2n launches of mp_fk_jac_id_f64 at q +- h e_j and a device
                       contraction with (gT, gJ) per joint (torch ops on the same stream).
Then one torch forward + backward of a task-space loss through mpa.fk_jacobian (--torch-rows rows): device tensors against CPU
tensors under the "hip" backend (host rows through the _host form).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (first: the HIP runtime torch loads serves the library too)

import manipulapy_amd as mp  # noqa: E402
from manipulapy_amd import _hip, registry  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--torch-rows", type=int, default=1_000_000)
    ap.add_argument("--robots", default="ur5,panda")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-central", action="store_true")
    args = ap.parse_args()
    ctx = registry.get_context()
    res = {"rows": args.rows, "reps": args.reps, "statistic": "median after one warm-up", "device": ctx.properties()["name"],
           "robots": {}}
    dev = torch.device("cuda", ctx.device_id)
    for name in args.robots.split(","):
        sm, _, lim = mp.load_robot(name)
        m = sm._kin_model()
        n, R = m.n, args.rows
        rng = np.random.default_rng(0)
        lim = np.asarray(lim, dtype=np.float64)
        q = torch.tensor(rng.uniform(lim[:, 0], lim[:, 1], (R, n)), device=dev)
        gT = torch.tensor(rng.normal(size=(R, 4, 4)), device=dev)
        gJ = torch.tensor(rng.normal(size=(R, 6, n)), device=dev)
        gq = torch.empty((R, n), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        r = {"n": n}
        rd, wr = R * 8 * (n + 16 + 6 * n), R * 8 * n
        k = max(1, round(rd / wr))
        probe = ctx.stream_bandwidth_mix(wr, k, 1, reps=args.reps, nontemporal=True)
        r["probe"] = {"reads_per_write": k, "GB_per_s": round(probe, 1)}
        r["bytes"] = rd + wr
        for frame in ("space", "body"):
            launch = lambda: ctx.fk_jac_vjp(m, frame, q.data_ptr(), gT.data_ptr(), gJ.data_ptr(), R, None, None, gq.data_ptr())  # noqa: E731
            ms = _median_ms(ctx, launch, args.reps)
            gbs = (rd + wr) / ms / 1e6
            r[f"vjp_{frame}_ms"] = round(ms, 4)
            r[f"vjp_{frame}_GB_per_s"] = round(gbs, 1)
            r[f"vjp_{frame}_frac_probe"] = round(gbs / probe, 3)
            r[f"vjp_{frame}_x_hbm_floor"] = round(ms / ((rd + wr) / 6.3e12 * 1e3), 3)
        T = torch.empty((R, 4, 4), dtype=torch.float64, device=dev)
        J = torch.empty((R, 6, n), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        r["fk_jac_ms"] = round(_median_ms(ctx, lambda: ctx.fk_jac_id(m, q.data_ptr(), None, None, R, T.data_ptr(), J.data_ptr(), None),
                                          args.reps), 4)
        if not args.no_central:
            h = 1e-6
            T2 = torch.empty_like(T)
            J2 = torch.empty_like(J)
            qs = torch.empty_like(q)
            s = ctx.stream()   # (a measurement process: handing the stream out is fine here)
            ext = torch.cuda.ExternalStream(s)
            torch.cuda.synchronize()

            def central():
                for j in range(n):
                    with torch.cuda.stream(ext):
                        qs.copy_(q)
                        qs[:, j] += h
                    ctx.fk_jac_id(m, qs.data_ptr(), None, None, R, T.data_ptr(), J.data_ptr(), None)
                    with torch.cuda.stream(ext):
                        qs[:, j] -= 2 * h
                    ctx.fk_jac_id(m, qs.data_ptr(), None, None, R, T2.data_ptr(), J2.data_ptr(), None)
                    with torch.cuda.stream(ext):
                        gq[:, j] = ((gT * (T - T2)).sum((1, 2)) + (gJ * (J - J2)).sum((1, 2))) / (2 * h)

            r["central_diff_ms"] = round(_median_ms(ctx, central, max(3, args.reps // 2)), 3)
            r["speedup_vs_central_diff"] = round(r["central_diff_ms"] / r["vjp_space_ms"], 1)
            del T2, J2, qs
        res["robots"][name] = r
        del q, gT, gJ, gq, T, J
        torch.cuda.empty_cache()
    if not args.no_torch:
        from manipulapy_amd import autograd as mpa

        sm = mp.load_robot("panda")[0]
        TR = args.torch_rows
        rng = np.random.default_rng(1)
        q0 = rng.uniform(-2, 2, (TR, 8))
        tgt0 = rng.uniform(-0.5, 0.5, (TR, 3))
        base = {d: (torch.tensor(q0, device=d), torch.tensor(tgt0, device=d)) for d in (dev, "cpu")}
        tr = {"robot": "panda", "rows": TR, "loss": "|p - p*|^2 + 1e-2 |J_b|^2", "statistic": "wall-clock median, inputs in place"}

        def step(device):
            qq, tgt = base[device]
            x = qq.detach().requires_grad_(True)
            T, J = mpa.fk_jacobian(sm, x, "body")
            (((T[:, :3, 3] - tgt) ** 2).sum() + 1e-2 * (J * J).sum()).backward()
            return x.grad

        dev_ms = _wall_median_ms(lambda: step(dev), args.reps)
        with mp.use_backend("hip"):
            cpu_ms = _wall_median_ms(lambda: step("cpu"), max(3, args.reps // 2))
        tr.update(device_tensors_ms=round(dev_ms, 3), cpu_tensors_ms=round(cpu_ms, 3), speedup=round(cpu_ms / dev_ms, 2))
        res["torch_forward_backward"] = tr
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
