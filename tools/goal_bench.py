#!/usr/bin/env python3
"""Times of the goal-configuration kernel k_goal_ik (csrc/mp_goal.h) on one GPU, beside the IK kernel on the same targets and seeds.

    python tools/goal_bench.py [--problems 131072] [--reps 3] [--robots xarm6,panda] [--out FILE]

Prints one JSON line and writes it to --out (profiles/goal_bench.json unless given).  Per robot, --problems pose goals in the model,
world and box of tests/rrt_cases.py (margin 0.02, tol 1e-3): a target is the forward kinematics of a uniform sample of the box, the
seed another uniform sample (the recipe of tests/goal_cases.py without its planted rows, seed 41).  eomg = ev = 1e-6, damping 0.02,
step_cap 0.5, max_iters x max_attempts of tests/goal_cases.py (xarm6 runs with ur5's).  Device arrays throughout:
  goal_ms              mp_goal_ik_f64 with all eight outputs; problems_per_s follows from it;
  pose_evals           the pose evaluations of the launch, iterations + attempts summed over the problems (an attempt evaluates the
                       pose once more than it steps); collision_evals: the sum of `converged`; both per second of goal_ms;
  found / in_collision / unreached   the shares of the statuses; attempts_mean, iterations_mean;
  ik_ms                mp_inverse_kinematics_f64 in the same process on the same targets and seeds, with the same box as joint limits,
                       tolerances, damping and step cap, max_iterations = max_iters x max_attempts, adaptive_tuning and backtracking
                       off; it knows no obstacles.  ik_success: the share it reports solved; ik_iterations_per_s from its counts.
                       Context, not a comparison of like with like: the two iterations differ (the header says how).
Every time is the median of --reps single launches timed one by one with HIP events after a warm-up launch; the smallest and the
largest are recorded beside it.  Hardware counters are not collected.  Without a device the tool fails: it has no other path.
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
    import goal_cases as gc
    import rrt_cases as rc
    from rrt_bench import _time

    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=131072)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--robots", default="xarm6,panda")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "goal_bench.json"))
    args = ap.parse_args()
    ctx = _hip.HipContext(0)
    B = args.problems
    props = ctx.properties()
    res = {"problems": B, "margin": gc.MARGIN, "tol": gc.TOL, "eomg": gc.EOMG, "ev": gc.EV, "damping": gc.DAMPING, "step_cap": gc.STEP_CAP,
           "reps": args.reps, "device": (props.get("name") or "unknown").strip("() "), "counters": "not collected", "robots": {}}
    for name in args.robots.split(","):
        cm, S_list, lo, hi = rc.make_plan_model(name)
        p = gc.params_of(name if name in gc.SETUP else "ur5")
        n = cm.n
        rng = np.random.default_rng(41)
        qt, q0 = rng.uniform(lo, hi, (B, n)), np.ascontiguousarray(rng.uniform(lo, hi, (B, n)))
        Tg = np.ascontiguousarray(gc.fk_jacobian(S_list, gc.tool_of(name), qt, np.float64)[0].reshape(B, 16))
        cm.sync_world(ctx)
        d_T, d_q0 = ctx.to_device(Tg), ctx.to_device(q0)
        shape = {"status": 1, "q": n, "attempts": 1, "iterations": 1, "converged": 1, "pose_error": 2, "clearance": 1, "witness": 3}
        real = ("q", "pose_error", "clearance")
        d = {k: ctx.alloc(B * shape[k] * (8 if k in real else 4)) for k in _hip.GOAL_OUTPUTS}
        r = {"n": n, "spheres": int(len(cm.links)), "pairs": int(len(cm.pairs)), "obstacles": int(len(cm.kinds)),
             "max_iters": p["max_iters"], "max_attempts": p["max_attempts"]}

        def put(key, t):
            r[f"{key}_ms"], r[f"{key}_min_ms"], r[f"{key}_max_ms"], r[f"{key}_launches"] = t

        put("goal", _time(ctx, lambda: ctx.goal_ik(cm.model, cm.handle, d_T, d_q0, B, lo, hi, gc.MARGIN, gc.TOL, **p,
                                                    **{"d_" + k: b for k, b in d.items()}), args.reps))
        ctx.synchronize()
        status = d["status"].download((B,), np.int32)
        attempts = d["attempts"].download((B,), np.int32).astype(np.int64)
        iters = d["iterations"].download((B,), np.int32).astype(np.int64)
        conv = d["converged"].download((B,), np.int32).astype(np.int64)
        sec = 1e-3 * r["goal_ms"]
        r["found"], r["in_collision"] = float((status == _hip.GOAL_FOUND).mean()), float((status == _hip.GOAL_IN_COLLISION).mean())
        r["unreached"] = float((status == _hip.GOAL_UNREACHED).mean())
        r["found_first_attempt"] = float(((status == _hip.GOAL_FOUND) & (attempts == 1)).mean())
        r["attempts_mean"], r["iterations_mean"], r["iterations_max"] = float(attempts.mean()), float(iters.mean()), int(iters.max())
        r["pose_evals"], r["collision_evals"] = int((iters + attempts).sum()), int(conv.sum())
        r["problems_per_s"] = B / sec
        r["pose_evals_per_s"], r["collision_evals_per_s"] = r["pose_evals"] / sec, r["collision_evals"] / sec
        # the IK kernel on the same targets and seeds, as context
        d_th, d_ok, d_it, d_rs = ctx.alloc(B * n * 8), ctx.alloc(B * 4), ctx.alloc(B * 4), ctx.alloc(B * 4)
        lim = np.ascontiguousarray(np.stack([lo, hi], axis=1))
        budget = p["max_iters"] * p["max_attempts"]
        put("ik", _time(ctx, lambda: ctx.inverse_kinematics(cm.model, d_T, d_q0, B, d_th, d_ok, d_it, d_rs, joint_limits=lim, eomg=gc.EOMG,
                                                            ev=gc.EV, max_iterations=budget, damping=gc.DAMPING, step_cap=gc.STEP_CAP,
                                                            adaptive_tuning=False, backtracking=False, seed=1), args.reps))
        ctx.synchronize()
        ik_it = d_it.download((B,), np.int32).astype(np.int64)
        r["ik_max_iterations"] = budget
        r["ik_success"] = float((d_ok.download((B,), np.int32) != 0).mean())
        r["ik_iterations"] = int(ik_it.sum())
        r["ik_iterations_per_s"] = r["ik_iterations"] / (1e-3 * r["ik_ms"])
        for b in (d_T, d_q0, d_th, d_ok, d_it, d_rs, *d.values()):
            b.free()
        for k, v in list(r.items()):
            if isinstance(v, float):
                r[k] = round(v, 4) if abs(v) < 1e4 else float(f"{v:.4e}")
        res["robots"][name] = r
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
