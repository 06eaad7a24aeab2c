#!/usr/bin/env python3
"""Collision-free joint-space paths for a batch of (start, goal) pairs by bidirectional RRT-Connect, every tree edge proven free by
conservative advancement; then the same paths through `batch_validate_path`, which shares nothing with the planner but the edge check.

    python examples/plan_path.py [hip]      (NumPy backend unless "hip" is given, which needs an MI355X)
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

# the arm and the world of validate_path.py: keep 2 cm from everything
margin, tol = 0.02, 1e-3
arm = mp.SphereCollisionModel.from_urdf(proc, radius=0.06, base_radius=0.1, pair_clearance=0.05)
tilt = np.array([[np.cos(0.3), -np.sin(0.3), 0.0], [np.sin(0.3), np.cos(0.3), 0.0], [0.0, 0.0, 1.0]])
arm.set_world(boxes=[([0.55, 0.0, 0.10], np.eye(3), [0.20, 0.40, 0.10]),
                     ([0.10, 0.55, 0.40], tilt, [0.05, 0.05, 0.40]),
                     ([-0.30, -0.45, 0.75], np.eye(3), [0.25, 0.15, 0.02])])

# 64 problems between random free configurations
rng = np.random.default_rng(0)
lim = proc.joint_limits_array
lo, hi = np.clip(lim[:, 0], -3.0, 3.0), np.clip(lim[:, 1], -3.0, 3.0)
pool = rng.uniform(lo, hi, (8192, 6))
d = arm.distances(pool)
pool = pool[np.minimum(d["dist_world"], d["dist_self"]) > margin + 0.03]
start, goal = pool[:64], pool[64:128]

# max_iters bounds the slowest problem, and the launch lasts as long as that one
r = planner.batch_plan_path(start, goal, arm, margin, tol, step=1.0, max_iters=200, max_nodes=256, max_waypoints=48, finite_limit=3.0)
names = {0: "solved", 1: "exhausted", 2: "tree full", 3: "start blocked", 4: "goal blocked", 5: "path too long", -1: "invalid"}
solved = r["status"] == 0
print(", ".join(f"{(r['status'] == s).sum()} {names[s]}" for s in sorted(set(r["status"].tolist()))))
print(f"solved directly: {(solved & (r['iterations'] == 0)).sum()}; waypoints of the others: mean "
      f"{r['count'][solved & (r['iterations'] > 0)].mean():.1f}, most {r['count'].max()}")
print(f"evaluations per problem: mean {r['evaluations'].mean():.0f}, most {r['evaluations'].max()}; largest tree {r['nodes'].max()} nodes")
for b in range(6):
    print(f"problem {b}: {names[int(r['status'][b])]} after {r['iterations'][b]} iterations, {r['count'][b]} waypoints, "
          f"trees of {r['nodes'][b][0]} + {r['nodes'][b][1]} nodes, {r['evaluations'][b]} evaluations")

# the paths are padded by repeating the goal, so the whole array goes into the validator as it is
v = planner.batch_validate_path(r["waypoints"][solved], arm, margin, tol)
print(f"{v['free'].sum()} of {solved.sum()} returned paths are proven free over their whole length; "
      f"smallest clearance on them {v['clearance'].min():+.3f} m")
