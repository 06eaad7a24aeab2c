#!/usr/bin/env python3
"""Times of the batched path-shortcutting kernel k_path_shortcut (csrc/mp_shortcut.h) on one GPU, beside the edge kernel it is built on.

    python tools/shortcut_bench.py [--problems 131072] [--reps 3] [--robots xarm6,panda] [--iters 50,200] [--out FILE]

Prints one JSON line and writes it to --out (profiles/shortcut_bench.json unless given).  Per robot, --problems planner outputs:
the problems of tools/rrt_bench.py (its recipe and seed; margin 0.02, tol 1e-3, max_steps 64, the planner settings of
tests/rrt_cases.py - xarm6 runs with ur5's) planned on the device by mp_rrt_connect_f64, whose `waypoints` and `count` stay on the
device and go into mp_path_shortcut_f64 as they are - the rows that were not solved included (they come back skipped).  min_gain
1e-3, max_waypoints 64, a workspace for every resident block.  Per max_iters of --iters:
  shortcut_ms          mp_path_shortcut_f64 with all nine outputs; problems_per_s and evals_per_s (the sum of the returned
                       `evaluations`) follow from it;
  ratio_mean / _median length_out / length_in over the paths (status done or straight);
  waypoints_in / _out  the mean waypoint count of those paths before and after; accepted_mean, skipped_full;
  edges_ms             mp_collision_edges_f64 in the same process over the problems' own start -> goal motions, repeated until their
                       evaluations sum to the shortcutter's (same margin, tol and max_steps); edge_evals_per_s from its `steps`;
  overhead             edge_evals_per_s over evals_per_s: what the locate scans, the selection work, the splices and the divergence
                       between the lanes of a wave cost over the bare edge kernel.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from manipulapy_amd import _hip  # noqa: E402


def main():
    import rrt_cases as rc
    from rrt_bench import _problems, _time

    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=131072)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--robots", default="xarm6,panda")
    ap.add_argument("--iters", default="50,200")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shortcut_bench.json"))
    args = ap.parse_args()
    ctx = _hip.HipContext(0)
    B = args.problems
    props = ctx.properties()
    min_gain, W = 1e-3, 64
    res = {"problems": B, "margin": rc.MARGIN, "tol": rc.TOL, "max_steps": rc.MAX_STEPS, "min_gain": min_gain, "max_waypoints": W,
           "device": (props.get("name") or "unknown").strip("() "), "robots": {}}
    for name in args.robots.split(","):
        cm, _, lo, hi = rc.make_plan_model(name)
        plan = rc.params_of(name if name in rc.SETUP else "ur5")
        n = cm.n
        qs, qg = _problems(cm, lo, hi, B, rc.MARGIN, 41)
        bufs = []

        def keep(b):
            bufs.append(b)
            return b

        blocks = min((B + 63) // 64, 4 * int(props.get("multiprocessor_count") or 256))
        cm.sync_world(ctx)
        # the planner's outputs, left on the device
        pws_bytes = _hip.rrt_connect_workspace_bytes(n, plan["max_nodes"], blocks)
        d_s, d_g, pws = ctx.to_device(qs), ctx.to_device(qg), ctx.alloc(pws_bytes)
        d_wp_in, d_cnt_in = keep(ctx.alloc(B * plan["max_waypoints"] * n * 8)), keep(ctx.alloc(B * 4))
        ctx.rrt_connect(cm.model, cm.handle, d_s, d_g, B, lo, hi, rc.MARGIN, rc.TOL, d_workspace=pws, workspace_bytes=pws_bytes,
                        d_waypoints=d_wp_in, d_count=d_cnt_in, **plan)
        ctx.synchronize()
        for b in (d_s, d_g, pws):
            b.free()
        count_in = d_cnt_in.download((B,), np.int32)
        ws_bytes = _hip.path_shortcut_workspace_bytes(n, W, blocks)
        ws = keep(ctx.alloc(ws_bytes))
        real = ("waypoints", "length_in", "length_out")
        d = {k: keep(ctx.alloc(B * (W * n * 8 if k == "waypoints" else 8 if k in real else 4))) for k in _hip.SHORTCUT_OUTPUTS}
        probe = _hip.cpu_collision_edges(cm.model, cm.handle, qs[:4096], qg[:4096], rc.MARGIN, rc.TOL, rc.MAX_STEPS, want=("steps",))
        r = {"n": n, "spheres": int(len(cm.links)), "pairs": int(len(cm.pairs)), "obstacles": int(len(cm.kinds)),
             "planned": float((count_in >= 2).mean()), "workspace_blocks": blocks, "workspace_bytes": ws_bytes, "runs": {}}
        for iters in (int(x) for x in args.iters.split(",")):
            q = {"max_iters": iters}

            def put(key, t):
                q[f"{key}_ms"], q[f"{key}_min_ms"], q[f"{key}_max_ms"], q[f"{key}_launches"] = t

            put("shortcut", _time(ctx, lambda: ctx.path_shortcut(cm.model, cm.handle, d_wp_in, d_cnt_in, B, plan["max_waypoints"], rc.MARGIN,
                                                                 rc.TOL, max_iters=iters, min_gain=min_gain, max_waypoints=W,
                                                                 max_steps=rc.MAX_STEPS, seed=1, d_workspace=ws, workspace_bytes=ws_bytes,
                                                                 **{"d_" + k: b for k, b in d.items()}), args.reps))
            ctx.synchronize()
            status = d["status"].download((B,), np.int32)
            path = (status == _hip.SHORTCUT_DONE) | (status == _hip.SHORTCUT_STRAIGHT)
            ev = d["evaluations"].download((B,), np.int32).astype(np.int64)
            li, lo_ = d["length_in"].download((B,), np.float64)[path], d["length_out"].download((B,), np.float64)[path]
            moved = li > 0
            ratio = lo_[moved] / li[moved]
            evals = int(ev.sum())
            q["evals"], q["evaluations_mean"], q["evaluations_max"] = evals, float(ev.mean()), int(ev.max())
            q["paths"], q["straight"] = float(path.mean()), float((status == _hip.SHORTCUT_STRAIGHT).mean())
            q["ratio_mean"], q["ratio_median"] = float(ratio.mean()), float(np.median(ratio))
            q["waypoints_in"] = float(count_in[path].mean())
            q["waypoints_out"] = float(d["count"].download((B,), np.int32)[path].mean())
            q["accepted_mean"] = float(d["accepted"].download((B,), np.int32)[path].mean())
            q["skipped_full"] = int(d["skipped_full"].download((B,), np.int32).sum())
            q["problems_per_s"] = B / (1e-3 * q["shortcut_ms"])
            q["evals_per_s"] = evals / (1e-3 * q["shortcut_ms"])
            # the edge kernel over the direct motions, repeated until the evaluations match
            E = int(min(1 << 24, max(B, np.ceil(evals / probe["steps"].mean()))))
            idx = np.arange(E) % B
            d_a, d_b = ctx.to_device(qs[idx]), ctx.to_device(qg[idx])
            d_st, d_sp = ctx.alloc(E * 4), ctx.alloc(E * 4)
            put("edges", _time(ctx, lambda: ctx.collision_edges(cm.model, cm.handle, d_a, d_b, E, rc.MARGIN, rc.TOL, rc.MAX_STEPS,
                                                                d_status=d_st, d_steps=d_sp), args.reps))
            ctx.synchronize()
            edge_evals = int(d_sp.download((E,), np.int32).astype(np.int64).sum())
            for b in (d_a, d_b, d_st, d_sp):
                b.free()
            q["edges"], q["edge_evals"] = E, edge_evals
            q["edge_evals_per_s"] = edge_evals / (1e-3 * q["edges_ms"])
            q["overhead"] = q["edge_evals_per_s"] / q["evals_per_s"]
            for k, v in list(q.items()):
                if isinstance(v, float):
                    q[k] = round(v, 4) if abs(v) < 1e4 else float(f"{v:.4e}")
            r["runs"][str(iters)] = q
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
