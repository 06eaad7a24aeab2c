#!/usr/bin/env python3
"""Times of the continuous edge check k_collision_edges (csrc/mp_collision.h) on one GPU, beside the plain distance kernel.

    python tools/collision_edges_bench.py [--edges 131072] [--max-steps 512] [--reps 3] [--robots xarm6,panda] [--out FILE]

Prints one JSON line and writes it to --out (profiles/r15_collision_edges_bench.json unless given).  Per robot, --edges edges by the
recipe of tests/collision_edge_cases.py (margin 0.02, tol 1e-3, max_steps 512 unless --max-steps says otherwise), device arrays:
  edges_ms          mp_collision_edges_f64 with all five outputs; edges_per_s and evals_per_s (configurations evaluated = the sum of
                    the returned `steps`) follow from it;
  lockstep_ratio    sum over the waves of 64 consecutive edges of 64 x their largest `steps`, over the sum of `steps`: the work a
                    wave that keeps its 64 edges until the slowest is done would do, relative to the queue's;
  ns_per_eval       edges_ms over the evaluated configurations;
  dist_ms           mp_collision_f64 with dist_world and dist_self only over as many rows as configurations were evaluated (rows drawn
                    from the edges' own end points), in the same process; dist_ns_per_row beside ns_per_eval.
Every time is the median of single launches timed one by one with HIP events after a warm-up launch; *_min_ms / *_max_ms /
*_launches give the spread.  Without a device the tool fails: it has no other path.
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
    import collision_edge_cases as ec

    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", type=int, default=131072)
    ap.add_argument("--max-steps", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--robots", default="xarm6,panda")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_collision_edges_bench.json"))
    args = ap.parse_args()
    ctx = _hip.HipContext(0)
    E = args.edges
    max_steps = args.max_steps or ec.MAX_STEPS
    res = {"edges": E, "margin": ec.MARGIN, "tol": ec.TOL, "max_steps": max_steps,
           "device": (ctx.properties().get("name") or "unknown").strip("() "), "robots": {}}
    for name in args.robots.split(","):
        case = ec.make_edge_case(name, E)
        cm, qa, qb = case["cm"], case["qa"], case["qb"]
        n = cm.n
        bufs = []

        def keep(b):
            bufs.append(b)
            return b

        d_a, d_b = keep(ctx.to_device(qa)), keep(ctx.to_device(qb))
        d = {"status": keep(ctx.alloc(E * 4)), "t": keep(ctx.alloc(E * 8)), "steps": keep(ctx.alloc(E * 4)),
             "clearance": keep(ctx.alloc(E * 8)), "witness": keep(ctx.alloc(E * 12))}
        cm.sync_world(ctx)
        r = {"n": n, "spheres": int(len(cm.links)), "pairs": int(len(cm.pairs)), "obstacles": int(len(cm.kinds))}

        def put(key, t):
            r[f"{key}_ms"], r[f"{key}_min_ms"], r[f"{key}_max_ms"], r[f"{key}_launches"] = t

        put("edges", _time(ctx, lambda: ctx.collision_edges(cm.model, cm.handle, d_a, d_b, E, ec.MARGIN, ec.TOL, max_steps,
                                                            **{"d_" + k: b for k, b in d.items()}), args.reps))
        ctx.synchronize()
        steps = d["steps"].download((E,), np.int32).astype(np.int64)
        status = d["status"].download((E,), np.int32)
        evals = int(steps.sum())
        full = (E // 64) * 64
        waves = steps[:full].reshape(-1, 64)
        r["evals"] = evals
        r["steps_mean"], r["steps_p95"], r["steps_max"] = float(steps.mean()), float(np.percentile(steps, 95)), int(steps.max())
        r["free"], r["blocked"], r["undecided"] = (float((status == s).mean()) for s in (ec.FREE, ec.BLOCKED, ec.UNDECIDED))
        r["lockstep_ratio"] = float(64 * waves.max(axis=1).sum() / waves.sum())
        r["edges_per_s"] = E / (1e-3 * r["edges_ms"])
        r["evals_per_s"] = evals / (1e-3 * r["edges_ms"])
        r["ns_per_eval"] = 1e6 * r["edges_ms"] / evals
        # the plain kernel over as many rows as configurations were evaluated
        rng = np.random.default_rng(2)
        q = np.concatenate([qa, qb])[rng.integers(0, 2 * E, evals)]
        d_q = keep(ctx.to_device(q))
        d_dw, d_ds = keep(ctx.alloc(evals * 8)), keep(ctx.alloc(evals * 8))
        put("dist", _time(ctx, lambda: ctx.collision(cm.model, cm.handle, d_q, evals, 1.0, 1.0, d_dist_world=d_dw, d_dist_self=d_ds), args.reps))
        r["dist_ns_per_row"] = 1e6 * r["dist_ms"] / evals
        r["eval_over_dist_row"] = r["ns_per_eval"] / r["dist_ns_per_row"]
        for k, v in list(r.items()):
            if isinstance(v, float):
                r[k] = round(v, 4) if abs(v) < 1e4 else float(f"{v:.4e}")
        res["robots"][name] = r
        for b in bufs:
            b.free()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
