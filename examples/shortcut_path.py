#!/usr/bin/env python3
"""Plan, shortcut, validate: the raw RRT-Connect paths of plan_path.py shortened by randomised shortcutting, every new segment proven
free by conservative advancement, then checked by `batch_validate_path`, which shares nothing with either but the edge check.

    python examples/shortcut_path.py [hip]      (NumPy backend unless "hip" is given, which needs an MI355X)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import manipulapy_amd as mp  # noqa: E402

backend = "hip" if "hip" in sys.argv[1:] else "numpy"
proc = mp.URDFToSerialManipulator(mp.robot_urdf("xarm6"))
mp.set_backend(backend)
planner = mp.OptimizedTrajectoryPlanning(proc.serial_manipulator, proc.urdf_name, proc.dynamics, proc.robot_data["joint_limits"],
                                         use_cuda=None if backend == "hip" else False)

# the arm, the world and the problems of plan_path.py: keep 2 cm from everything
margin, tol = 0.02, 1e-3
arm = mp.SphereCollisionModel.from_urdf(proc, radius=0.06, base_radius=0.1, pair_clearance=0.05)
tilt = np.array([[np.cos(0.3), -np.sin(0.3), 0.0], [np.sin(0.3), np.cos(0.3), 0.0], [0.0, 0.0, 1.0]])
arm.set_world(boxes=[([0.55, 0.0, 0.10], np.eye(3), [0.20, 0.40, 0.10]),
                     ([0.10, 0.55, 0.40], tilt, [0.05, 0.05, 0.40]),
                     ([-0.30, -0.45, 0.75], np.eye(3), [0.25, 0.15, 0.02])])
rng = np.random.default_rng(0)
lim = proc.joint_limits_array
lo, hi = np.clip(lim[:, 0], -3.0, 3.0), np.clip(lim[:, 1], -3.0, 3.0)
pool = rng.uniform(lo, hi, (8192, 6))
d = arm.distances(pool)
pool = pool[np.minimum(d["dist_world"], d["dist_self"]) > margin + 0.03]
start, goal = pool[:64], pool[64:128]

plan = planner.batch_plan_path(start, goal, arm, margin, tol, step=1.0, max_iters=200, max_nodes=256, max_waypoints=48, finite_limit=3.0)
print(f"planned: {(plan['status'] == 0).sum()} of 64 solved, {(plan['count'] > 2).sum()} of them with more than two waypoints")

# the planner's padded waypoints and its count go in as they are; the rows it did not solve come back skipped
short = planner.batch_shortcut_path(plan["waypoints"], plan["count"], arm, margin, tol, max_iters=100, min_gain=1e-3)
names = {0: "done", 1: "straight", 2: "skipped", -1: "invalid"}
print(", ".join(f"{(short['status'] == s).sum()} {names[s]}" for s in sorted(set(short["status"].tolist()))))
path = (short["status"] == 0) | (short["status"] == 1)
bent = path & (plan["count"] > 2)
ratio = short["length_out"][bent] / short["length_in"][bent]
print(f"paths with more than two waypoints: length {short['length_in'][bent].mean():.2f} -> {short['length_out'][bent].mean():.2f} rad on "
      f"average (ratio mean {ratio.mean():.2f}, best {ratio.min():.2f}); waypoints {plan['count'][bent].mean():.1f} -> "
      f"{short['count'][bent].mean():.1f}; {short['accepted'][bent].mean():.1f} shortcuts accepted and "
      f"{short['evaluations'][bent].mean():.0f} configurations evaluated a path")
for b in np.flatnonzero(bent)[:6]:
    print(f"problem {b}: {plan['count'][b]} waypoints, length {short['length_in'][b]:.2f} -> {short['count'][b]} waypoints, "
          f"length {short['length_out'][b]:.2f} ({short['accepted'][b]} shortcuts of {short['iterations'][b]} iterations)")

# the output is padded like the planner's, so the whole array goes into the validator as it is
v = planner.batch_validate_path(short["waypoints"][path], arm, margin, tol)
print(f"{v['free'].sum()} of {path.sum()} shortened paths are proven free over their whole length; "
      f"smallest clearance on them {v['clearance'].min():+.3f} m")
