#!/usr/bin/env python3
"""The fastest timing of joint-space paths within the URDF's own effort and velocity limits.

    python examples/time_optimal.py [hip]      (NumPy backend unless "hip" is given, which needs an MI355X)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import manipulapy_amd as mp  # noqa: E402

backend = "hip" if "hip" in sys.argv[1:] else "numpy"
proc = mp.URDFToSerialManipulator(mp.robot_urdf("xarm6"))
effort, vmax = proc.effort_limits, proc.velocity_limits
mp.set_backend(backend)
planner = mp.OptimizedTrajectoryPlanning(proc.serial_manipulator, proc.urdf_name, proc.dynamics, proc.robot_data["joint_limits"],
                                         torque_limits=np.stack([-effort, effort], axis=1), use_cuda=None if backend == "hip" else False)

# 256 straight lines between random poses, 100 grid points each: rest to rest, as fast as the actuators allow
rng = np.random.default_rng(0)
lim = proc.joint_limits_array
mid, half = lim.mean(axis=1), np.minimum(0.5 * (lim[:, 1] - lim[:, 0]), 1.5)
start, end = mid + rng.uniform(-1, 1, (2, 256, 6)) * half
r = planner.batch_time_optimal_joint_trajectory(start, end, 100, vmax)
ok = r["status"] == 0
print(f"{ok.sum()} of 256 lines feasible; duration {r['duration'][ok].min():.2f} .. {r['duration'][ok].max():.2f} s")
print("peak |tau| / effort per joint:", (np.abs(r["torques"][ok][:, :-1]).max(axis=(0, 1)) / effort).round(3))
print("peak |qd| / vmax per joint:   ", (np.abs(r["velocities"][ok]).max(axis=(0, 1)) / vmax).round(3))

# for comparison, the fixed-time quintic of the same duration against the same limits (it is not held to them)
b = int(np.flatnonzero(ok)[0])
quintic = planner.joint_trajectory(start[b], end[b], Tf=float(r["duration"][b]), N=100, method=5)
free = mp.OptimizedTrajectoryPlanning(proc.serial_manipulator, proc.urdf_name, proc.dynamics, proc.robot_data["joint_limits"],
                                      use_cuda=None if backend == "hip" else False)
tau_q = free.inverse_dynamics_trajectory(np.asarray(quintic["positions"], dtype=np.float64), np.asarray(quintic["velocities"], dtype=np.float64),
                                         np.asarray(quintic["accelerations"], dtype=np.float64))
print(f"path {b}: {r['duration'][b]:.2f} s; a quintic of that duration peaks at", (np.abs(tau_q).max(axis=0) / effort).round(2), "of the effort and",
      (np.abs(np.asarray(quintic["velocities"])).max(axis=0) / vmax).round(2), "of the velocity limits")
