#!/usr/bin/env python3
"""Plan, shortcut, blend, time: the shortened paths of shortcut_path.py turned into twice-differentiable curves - every corner
replaced by a quintic blend that conservative advancement proves free - and timed as fast as the velocity and acceleration limits
allow, without a stop at any waypoint.

    python examples/smooth_and_time.py [hip]      (NumPy backend unless "hip" is given, which needs an MI355X)
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
short = planner.batch_shortcut_path(plan["waypoints"], plan["count"], arm, margin, tol, max_iters=100, min_gain=1e-3)
print(f"planned: {(plan['status'] == 0).sum()} of 64 solved; shortened to {short['count'][short['count'] > 0].mean():.1f} waypoints on average")

# the shortcutter's padded waypoints and its count go in as they are; the grid is fine enough to put points inside the blends
N, vmax, amax = 257, np.full(6, 2.0), np.full(6, 8.0)
free = np.tile([-np.inf, np.inf], (6, 1))   # no torque limits here: velocity and acceleration only
out = planner.batch_time_optimal_path(short["waypoints"], short["count"], arm, N, vmax, torque_limits=free, acceleration_limits=amax,
                                      margin=margin, tol=tol, blend=0.5, max_halvings=6)
bl, tm = out["blend"], out["timing"]
names = {0: "done", 1: "straight", 2: "skipped", 3: "point", 4: "blocked", 5: "reversal", -1: "invalid"}
print("blend: " + ", ".join(f"{(bl['status'] == s).sum()} {names[s]}" for s in sorted(set(bl["status"].tolist()))))
done = bl["status"] == 0
if done.any():
    corners = bl["count"][done] - 2
    print(f"{corners.sum()} corners blended on {done.sum()} paths: cut {bl['cut'][done][bl['cut'][done] > 0].mean():.3f} rad on average, "
          f"{bl['halvings'][done].sum()} halvings, {bl['evaluations'][done].mean():.0f} configurations evaluated a path, smallest "
          f"clearance met {bl['clearance'][done].min():+.3f} m")
    dist = arm.distances(bl["q"][done])
    print(f"smallest clearance over the {done.sum() * N} grid configurations: {min(dist['dist_world'].min(), dist['dist_self'].min()):+.3f} m")
timed = (bl["status"] == 0) | (bl["status"] == 1)
ok = timed & (tm["status"] == 0) & np.isfinite(tm["duration"])
print(f"timed: {ok.sum()} of {timed.sum()} curves; duration {tm['duration'][ok].mean():.2f} s on average")

# against a full stop at every waypoint: the same limits on each segment by itself
for b in np.flatnonzero(ok & done)[:4]:
    m = bl["count"][b]
    seg = planner.batch_time_optimal_joint_trajectory(bl["points"][b, :m - 1], bl["points"][b, 1:m], 65, vmax, free, amax)
    print(f"problem {b}: {m} waypoints, {bl['length'][b]:.2f} rad: {tm['duration'][b]:.2f} s through the blends, "
          f"{seg['duration'].sum():.2f} s with a stop at every waypoint")
