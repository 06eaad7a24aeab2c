#!/usr/bin/env python3
"""Times of the batched RRT-Connect kernel k_rrt_connect (csrc/mp_rrt.h) on one GPU, beside the edge kernel it is built on.

    python tools/rrt_bench.py [--problems 131072] [--reps 2] [--robots xarm6,panda] [--max-iters N] [--out FILE]

Prints one JSON line and writes it to --out (profiles/r16_rrt_bench.json unless given).  Per robot, --problems problems by the
recipe of tests/rrt_cases.py without the planted rows (starts and goals uniform in the box with clearance above margin + 0.03, here
filtered by the library's own distance twin; margin 0.02, tol 1e-3, max_steps 64, step 1.0, the robot's max_iters / max_nodes of that
module - xarm6 runs with ur5's), device arrays, a workspace for every resident block:
  plan_ms            mp_rrt_connect_f64 with all six outputs; problems_per_s and evals_per_s (the sum of the returned `evaluations`)
                     follow from it;
  solved, exhausted  fractions of the problems; iterations / nodes / evaluations: mean and largest;
  edges_ms           mp_collision_edges_f64 in the same process over the problems' own start -> goal motions, repeated until their
                     evaluations sum to the planner's (same margin, tol and max_steps); edge_evals_per_s from its returned `steps`;
  overhead           edge_evals_per_s over evals_per_s: what the nearest scans, the selection work and the divergence between the
                     lanes of a wave cost over the bare edge kernel.
Every time is the median of single launches timed one by one with HIP events after a warm-up launch.  Without a device the tool fails:
it has no other path.
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


def _time(ctx, fn, reps):
    a, b = _hip.HipEvent(ctx), _hip.HipEvent(ctx)

    def once():
        a.record()
        fn()
        b.record()
        ctx.synchronize()
        return b.elapsed_ms_since(a)

    once()
    t = np.array([once() for _ in range(max(1, reps))])
    a.destroy(); b.destroy()
    return float(np.median(t)), float(t.min()), float(t.max()), len(t)


def _problems(cm, lo, hi, B, margin, seed):
    rng = np.random.default_rng(seed)
    rows = []
    while sum(map(len, rows)) < 2 * B:
        pool = rng.uniform(lo, hi, (1 << 16, len(lo)))
        r = _hip.cpu_collision(cm.model, cm.handle, pool, 1.0, 1.0, want=("dist_world", "dist_self"))
        rows.append(pool[np.minimum(r["dist_world"], r["dist_self"]) > margin + 0.03])
    free = np.concatenate(rows)
    return np.ascontiguousarray(free[:B]), np.ascontiguousarray(free[B:2 * B])


def main():
    import rrt_cases as rc

    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=131072)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--robots", default="xarm6,panda")
    ap.add_argument("--max-iters", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_rrt_bench.json"))
    args = ap.parse_args()
    ctx = _hip.HipContext(0)
    B = args.problems
    props = ctx.properties()
    res = {"problems": B, "margin": rc.MARGIN, "tol": rc.TOL, "max_steps": rc.MAX_STEPS, "step": rc.STEP, "min_advance": rc.MIN_ADVANCE,
           "device": (props.get("name") or "unknown").strip("() "), "robots": {}}
    for name in args.robots.split(","):
        cm, _, lo, hi = rc.make_plan_model(name)
        p = rc.params_of(name if name in rc.SETUP else "ur5")
        if args.max_iters:
            p["max_iters"] = args.max_iters
        n, W = cm.n, p["max_waypoints"]
        qs, qg = _problems(cm, lo, hi, B, rc.MARGIN, 41)
        bufs = []

        def keep(b):
            bufs.append(b)
            return b

        blocks = min((B + 63) // 64, 4 * int(props.get("multiprocessor_count") or 256))
        ws_bytes = _hip.rrt_connect_workspace_bytes(n, p["max_nodes"], blocks)
        d_s, d_g, ws = keep(ctx.to_device(qs)), keep(ctx.to_device(qg)), keep(ctx.alloc(ws_bytes))
        d = {"status": keep(ctx.alloc(B * 4)), "count": keep(ctx.alloc(B * 4)), "waypoints": keep(ctx.alloc(B * W * n * 8)),
             "iterations": keep(ctx.alloc(B * 4)), "nodes": keep(ctx.alloc(B * 8)), "evaluations": keep(ctx.alloc(B * 4))}
        cm.sync_world(ctx)
        r = {"n": n, "spheres": int(len(cm.links)), "pairs": int(len(cm.pairs)), "obstacles": int(len(cm.kinds)),
             "max_iters": p["max_iters"], "max_nodes": p["max_nodes"], "max_waypoints": W, "workspace_blocks": blocks,
             "workspace_bytes": ws_bytes}

        def put(key, t):
            r[f"{key}_ms"], r[f"{key}_min_ms"], r[f"{key}_max_ms"], r[f"{key}_launches"] = t

        put("plan", _time(ctx, lambda: ctx.rrt_connect(cm.model, cm.handle, d_s, d_g, B, lo, hi, rc.MARGIN, rc.TOL, d_workspace=ws,
                                                       workspace_bytes=ws_bytes, **p, **{"d_" + k: b for k, b in d.items()}), args.reps))
        ctx.synchronize()
        status = d["status"].download((B,), np.int32)
        its = d["iterations"].download((B,), np.int32)
        nodes = d["nodes"].download((B, 2), np.int32)
        ev = d["evaluations"].download((B,), np.int32).astype(np.int64)
        evals = int(ev.sum())
        r["evals"] = evals
        r["solved"], r["exhausted"] = float((status == rc.SOLVED).mean()), float((status == rc.EXHAUSTED).mean())
        r["solved_directly"] = float(((status == rc.SOLVED) & (its == 0)).mean())
        r["iterations_mean"], r["iterations_max"] = float(its.mean()), int(its.max())
        r["nodes_mean"], r["nodes_max"] = float(nodes.sum(axis=1).mean()), int(nodes.max())
        r["evaluations_mean"], r["evaluations_max"] = float(ev.mean()), int(ev.max())
        r["problems_per_s"] = B / (1e-3 * r["plan_ms"])
        r["evals_per_s"] = evals / (1e-3 * r["plan_ms"])
        # the edge kernel over the direct motions, repeated until the evaluations match
        probe = _hip.cpu_collision_edges(cm.model, cm.handle, qs[:4096], qg[:4096], rc.MARGIN, rc.TOL, rc.MAX_STEPS, want=("steps",))
        E = int(min(1 << 24, max(B, np.ceil(evals / probe["steps"].mean()))))
        idx = np.arange(E) % B
        d_a, d_b = keep(ctx.to_device(qs[idx])), keep(ctx.to_device(qg[idx]))
        d_st, d_sp = keep(ctx.alloc(E * 4)), keep(ctx.alloc(E * 4))
        put("edges", _time(ctx, lambda: ctx.collision_edges(cm.model, cm.handle, d_a, d_b, E, rc.MARGIN, rc.TOL, rc.MAX_STEPS, d_status=d_st,
                                                            d_steps=d_sp), args.reps))
        ctx.synchronize()
        edge_evals = int(d_sp.download((E,), np.int32).astype(np.int64).sum())
        r["edges"], r["edge_evals"] = E, edge_evals
        r["edge_evals_per_s"] = edge_evals / (1e-3 * r["edges_ms"])
        r["overhead"] = r["edge_evals_per_s"] / r["evals_per_s"]
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
