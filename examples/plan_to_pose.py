#!/usr/bin/env python3
"""From end-effector poses to collision-free paths: `batch_goal_configurations` turns 64 pose goals into joint configurations the
planner accepts as goals - damped Newton attempts, each one that reaches the pose decided by the planner's own zero-edge check - and
`batch_plan_path_to_pose` does that and plans to them in one call.

    python examples/plan_to_pose.py [hip]      (NumPy backend unless "hip" is given, which needs an MI355X)
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

# the arm and the world of plan_path.py: keep 2 cm from everything
margin, tol = 0.02, 1e-3
arm = mp.SphereCollisionModel.from_urdf(proc, radius=0.06, base_radius=0.1, pair_clearance=0.05)
tilt = np.array([[np.cos(0.3), -np.sin(0.3), 0.0], [np.sin(0.3), np.cos(0.3), 0.0], [0.0, 0.0, 1.0]])
arm.set_world(boxes=[([0.55, 0.0, 0.10], np.eye(3), [0.20, 0.40, 0.10]),
                     ([0.10, 0.55, 0.40], tilt, [0.05, 0.05, 0.40]),
                     ([-0.30, -0.45, 0.75], np.eye(3), [0.25, 0.15, 0.02])])

# 64 free start configurations, and 64 poses the arm can reach: the tool poses of other random configurations, free or not.  One pose
# is moved out of reach.
rng = np.random.default_rng(0)
lim = proc.joint_limits_array
lo, hi = np.clip(lim[:, 0], -3.0, 3.0), np.clip(lim[:, 1], -3.0, 3.0)
pool = rng.uniform(lo, hi, (8192, 6))
d = arm.distances(pool)
start = pool[np.minimum(d["dist_world"], d["dist_self"]) > margin + 0.03][:64]
T_goal = np.array([proc.serial_manipulator.forward_kinematics(q) for q in rng.uniform(lo, hi, (64, 6))])
T_goal[7, 0, 3] += 5.0

# the goal configurations alone, seeded by the starts
g = planner.batch_goal_configurations(T_goal, start, arm, margin, tol, max_iters=50, max_attempts=8, finite_limit=3.0)
goal_names = {0: "found", 1: "in collision", 2: "unreached", -1: "invalid"}
print("goals: " + ", ".join(f"{(g['status'] == s).sum()} {goal_names[s]}" for s in sorted(set(g["status"].tolist()))))
found = g["status"] == 0
print(f"found on the first attempt: {(found & (g['attempts'] == 1)).sum()}; attempts of the others: mean "
      f"{g['attempts'][found & (g['attempts'] > 1)].mean():.1f}; steps per problem: mean {g['iterations'].mean():.0f}, most {g['iterations'].max()}")
print(f"pose error of the found: rotation up to {g['pose_error'][found, 0].max():.1e} rad, position up to "
      f"{g['pose_error'][found, 1].max():.1e} m; their clearance: smallest {g['clearance'][found].min():+.3f} m")

# poses in, paths out: a found goal is never refused by the planner, one in collision comes back goal-blocked, an unreached one invalid
r = planner.batch_plan_path_to_pose(start, T_goal, arm, margin, tol, goal_max_iters=50, max_attempts=8, step=1.0, max_iters=200,
                                    max_nodes=256, max_waypoints=48, finite_limit=3.0)
plan_names = {0: "solved", 1: "exhausted", 2: "tree full", 3: "start blocked", 4: "goal blocked", 5: "path too long", -1: "invalid"}
print("paths: " + ", ".join(f"{(r['status'] == s).sum()} {plan_names[s]}" for s in sorted(set(r["status"].tolist()))))
for b in (0, 1, 7):
    print(f"problem {b}: goal {goal_names[int(r['goal_status'][b])]} after {r['goal_attempts'][b]} attempts, path "
          f"{plan_names[int(r['status'][b])]} with {r['count'][b]} waypoints")
solved = r["status"] == 0
v = planner.batch_validate_path(r["waypoints"][solved], arm, margin, tol)
print(f"{v['free'].sum()} of {solved.sum()} returned paths are proven free over their whole length")
