#!/usr/bin/env python3
"""A sensed world: an occupancy grid instead of hand-placed shapes.  The occupied voxels become a point cloud of the sphere collision
model (`set_cloud_from_voxels`: one ball a voxel, covering its cube), and the chain of the other examples runs on it unchanged:
plan, shortcut, then blend, time and sample at 1 kHz, with the clearance of the sampled configurations at the end.

    python examples/point_cloud_world.py [hip]      (NumPy backend unless "hip" is given, which needs an MI355X)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import manipulapy_amd as mp  # noqa: E402

backend = "hip" if "hip" in sys.argv[1:] else "numpy"
proc = mp.URDFToSerialManipulator(mp.robot_urdf("xarm6"))
mp.set_backend(backend)
effort = np.asarray(proc.effort_limits, dtype=np.float64)
planner = mp.OptimizedTrajectoryPlanning(proc.serial_manipulator, proc.urdf_name, proc.dynamics, proc.robot_data["joint_limits"],
                                         torque_limits=np.stack([-effort, effort], axis=1), use_cuda=None if backend == "hip" else False)

# a 4 cm occupancy grid over [-0.8, 0.8]^2 x [0, 1.2]: a table top in front of the arm, a post beside it, a shelf behind
pitch, origin = 0.04, np.array([-0.8, -0.8, 0.0])
occ = np.zeros((40, 40, 30), dtype=bool)
cell = lambda p: np.floor((np.asarray(p) - origin) / pitch).astype(int)  # noqa: E731
(x0, y0, z0), (x1, y1, z1) = cell([0.35, -0.40, 0.16]), cell([0.75, 0.40, 0.20])
occ[x0:x1, y0:y1, z0:z1 + 1] = True
(x0, y0, z0), (x1, y1, z1) = cell([0.05, 0.50, 0.00]), cell([0.15, 0.60, 0.80])
occ[x0:x1, y0:y1, z0:z1] = True
(x0, y0, z0), (x1, y1, z1) = cell([-0.55, -0.60, 0.72]), cell([-0.05, -0.30, 0.76])
occ[x0:x1, y0:y1, z0:z1 + 1] = True

margin, tol, d_max = 0.02, 1e-3, 0.25
arm = mp.SphereCollisionModel.from_urdf(proc, radius=0.06, base_radius=0.1, pair_clearance=0.05)
arm.set_cloud_from_voxels(occ, origin, pitch, d_max)      # no primitive table at all: the cloud is the world
c = arm.cloud
print(f"{occ.sum()} occupied voxels -> {len(c['points'])} points of radius {c['radius']:.4f} m, distances cut off at {c['d_max']} m, "
      f"grid cell {c['cell']:.3f} m")

rng = np.random.default_rng(0)
lim = proc.joint_limits_array
lo, hi = np.clip(lim[:, 0], -3.0, 3.0), np.clip(lim[:, 1], -3.0, 3.0)
pool = rng.uniform(lo, hi, (8192, 6))
d = arm.distances(pool)
hit = d["dist_world"] < 0
print(f"{hit.sum()} of {len(pool)} random configurations touch the cloud; the witness of the first: sphere {d['arg_world'][hit][0, 0]}, "
      f"point {d['arg_world'][hit][0, 1]} of {len(c['points'])}")
pool = pool[np.minimum(d["dist_world"], d["dist_self"]) > margin + 0.03]
start, goal = pool[:64], pool[64:128]

plan = planner.batch_plan_path(start, goal, arm, margin, tol, step=1.0, max_iters=200, max_nodes=256, max_waypoints=48, finite_limit=3.0)
print(f"planned: {(plan['status'] == 0).sum()} of 64 solved, {(plan['count'] > 2).sum()} of them with more than two waypoints")
short = planner.batch_shortcut_path(plan["waypoints"], plan["count"], arm, margin, tol, max_iters=100, min_gain=1e-3)
path = (short["status"] == 0) | (short["status"] == 1)
bent = path & (plan["count"] > 2)
if bent.any():
    print(f"shortcut: length {short['length_in'][bent].mean():.2f} -> {short['length_out'][bent].mean():.2f} rad on the paths with "
          f"more than two waypoints")
v = planner.batch_validate_path(short["waypoints"][path], arm, margin, tol)
print(f"{v['free'].sum()} of {path.sum()} shortened paths are proven free of the cloud over their whole length; smallest clearance "
      f"{v['clearance'].min():+.3f} m")

vmax, amax, dt = np.full(6, 2.0), np.full(6, 8.0), 1e-3
out = planner.batch_time_optimal_trajectory(short["waypoints"], short["count"], arm, 129, dt, vmax, acceleration_limits=amax, margin=margin,
                                            tol=tol, blend=0.5, max_halvings=6, max_samples=20000)   # at most 20 s a trajectory
sm = out["samples"]
ok = sm["status"] == 0
names = {0: "ok", 1: "truncated", 2: "stops", 3: "untimed", -1: "invalid"}
print(", ".join(f"{(sm['status'] == s).sum()} {names[s]}" for s in sorted(set(sm["status"].tolist()))))
print(f"{ok.sum()} trajectories timed and sampled: {sm['count'][ok].sum()} rows at {1 / dt:.0f} Hz, the longest {sm['count'][ok].max() * dt:.2f} s")
done = ok & (out["blend"]["status"] == 0)
if done.any():
    dist = arm.distances(sm["positions"][done])
    print(f"smallest clearance over the sampled configurations of the blended paths: "
          f"{min(dist['dist_world'].min(), dist['dist_self'].min()):+.3f} m (margin {margin})")

arm.clear_cloud()                                          # the world is empty again
print(f"after clear_cloud: dist_world of the first configuration is {arm.distances(pool[:1])['dist_world'][0]}")
