#!/usr/bin/env python3
"""Pose goal -> straight line -> timing -> fixed-rate samples: 64 approach moves of 10 to 25 cm along the tool's own z axis with the
orientation held, tracked in joint space, proven collision-free on the curve that is executed, timed as fast as the velocity and
acceleration limits allow and sampled at 1 kHz.

    python examples/cartesian_line.py [hip]      (NumPy backend unless "hip" is given, which needs an MI355X)
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
rng = np.random.default_rng(0)
lim = proc.joint_limits_array
lo, hi = np.clip(lim[:, 0], -3.0, 3.0), np.clip(lim[:, 1], -3.0, 3.0)
pool = rng.uniform(lo + 0.2 * (hi - lo), hi - 0.2 * (hi - lo), (8192, 6))
d = arm.distances(pool)
start = pool[np.minimum(d["dist_world"], d["dist_self"]) > margin + 0.03][:64]

# the goal: the start pose moved along its own z axis
T_start = np.stack([proc.serial_manipulator.forward_kinematics(q) for q in start])
T_goal = T_start.copy()
T_goal[:, :3, 3] += rng.uniform(0.10, 0.25, 64)[:, None] * T_start[:, :3, 2]

N, dt, vmax, amax = 33, 1e-3, np.full(6, 2.0), np.full(6, 8.0)
free = np.tile([-np.inf, np.inf], (6, 1))   # no torque limits here: velocity and acceleration only
out = planner.batch_time_optimal_cartesian_trajectory(start, T_goal, arm, N, dt, vmax, torque_limits=free, acceleration_limits=amax,
                                                      margin=margin, tol=tol, finite_limit=3.0)
line, timing, samples = out["line"], out["timing"], out["samples"]
names = {0: "done", 1: "stalled", 2: "singular", 3: "limit", 4: "jump", 5: "blocked", 6: "undecided", -1: "invalid"}
print("line: " + ", ".join(f"{(line['status'] == s).sum()} {names[s]}" for s in sorted(set(line["status"].tolist()))))
done = line["status"] == 0
if done.any():
    print(f"{done.sum()} lines proven free: smallest clearance met {line['clearance'][done].min():+.3f} m, "
          f"{line['evaluations'][done].mean():.0f} configurations evaluated a line, the curve leaves the line by at most "
          f"{line['deviation_pos'][done].max():.1e} m and {line['deviation_rot'][done].max():.1e} rad between grid points")
    ok = done & (timing["status"] == 0) & (samples["status"] == 0)
    print(f"timed and sampled: {ok.sum()} of {done.sum()}; duration {timing['duration'][ok].mean():.2f} s on average, "
          f"{samples['count'][ok].mean():.0f} samples a line at {1 / dt:.0f} Hz")
    for b in np.flatnonzero(ok)[:4]:
        pos = samples["positions"][b, :samples["count"][b]]
        tip = np.stack([proc.serial_manipulator.forward_kinematics(q)[:3, 3] for q in pos[::50]])
        a, v = T_start[b, :3, 3], T_goal[b, :3, 3] - T_start[b, :3, 3]
        off = np.linalg.norm(np.cross(tip - a, v / np.linalg.norm(v)), axis=1).max()
        dist = arm.distances(pos)
        print(f"problem {b}: {np.linalg.norm(v):.3f} m in {timing['duration'][b]:.2f} s, the sampled tool point stays within {off:.1e} m of "
              f"the line, clearance over the samples {min(dist['dist_world'].min(), dist['dist_self'].min()):+.3f} m")
for b in np.flatnonzero((line["status"] == 5) | (line["status"] == 6))[:4]:
    print(f"problem {b}: {names[int(line['status'][b])]} on span {line['span'][b]} at u = {line['t'][b]:.2f}")
