#!/usr/bin/env python3
"""Clearance of a batch of quintic joint trajectories in a world of a few boxes, with a sphere model of the arm.

    python examples/collision_check.py [hip]      (NumPy backend unless "hip" is given, which needs an MI355X)
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

# spheres of 6 cm along the arm, one of 10 cm on the base; a table edge, a post and a shelf
arm = mp.SphereCollisionModel.from_urdf(proc, radius=0.06, base_radius=0.1)
tilt = np.array([[np.cos(0.3), -np.sin(0.3), 0.0], [np.sin(0.3), np.cos(0.3), 0.0], [0.0, 0.0, 1.0]])
arm.set_world(boxes=[([0.55, 0.0, 0.10], np.eye(3), [0.20, 0.40, 0.10]),
                     ([0.10, 0.55, 0.40], tilt, [0.05, 0.05, 0.40]),
                     ([-0.30, -0.45, 0.75], np.eye(3), [0.25, 0.15, 0.02])])
print(f"{len(arm.links)} spheres, {len(arm.pairs)} self-collision pairs, {len(arm.kinds)} obstacles")

# 64 quintic moves between random poses, 50 steps each
rng = np.random.default_rng(0)
lim = proc.joint_limits_array
mid, half = lim.mean(axis=1), np.minimum(0.5 * (lim[:, 1] - lim[:, 0]), 0.8)
start, end = mid + rng.uniform(-1, 1, (2, 64, 6)) * half
traj = np.asarray(planner.batch_joint_trajectory(start, end, 2.0, 50, 5)["positions"], dtype=np.float64)
r = planner.batch_trajectory_clearance(traj, arm, margin=0.0)
free = r["first_violation"] < 0
print(f"{free.sum()} of 64 trajectories are collision-free")
for b in range(8):
    hit = "free" if free[b] else f"below the margin from step {r['first_violation'][b]}"
    print(f"trajectory {b}: world {r['world_clearance'][b]:+.3f} m at step {r['world_step'][b]}, "
          f"self {r['self_clearance'][b]:+.3f} m at step {r['self_step'][b]}: {hit}")

# the smooth penalty an optimiser would descend: cost and gradient at the worst step of the first colliding trajectory
if (~free).any():
    b = int(np.flatnonzero(~free)[0])
    cost, grad = arm.cost(traj[b, r["first_violation"][b]], 0.1, 0.1)
    print(f"trajectory {b}, step {r['first_violation'][b]}: cost {cost:.4f}, gradient", np.round(grad, 3))
