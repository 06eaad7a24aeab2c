#!/usr/bin/env python3
"""Plan, shortcut, blend, time, sample: the timed curves of smooth_and_time.py turned into what a controller takes - q, qd, qdd and
the feed-forward torque at 1 kHz - with the torque and the speed looked at between the grid points of the parameterisation.

    python examples/sample_trajectory.py [hip]      (NumPy backend unless "hip" is given, which needs an MI355X)
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

# blend, time under this planner's torque limits (the URDF's effort limits) and sample at 1 kHz, in one call
vmax, amax, dt = np.full(6, 2.0), np.full(6, 8.0), 1e-3
names = {0: "ok", 1: "truncated", 2: "stops", 3: "untimed", -1: "invalid"}
for N in (65, 257):
    out = planner.batch_time_optimal_trajectory(short["waypoints"], short["count"], arm, N, dt, vmax, acceleration_limits=amax, margin=margin,
                                                tol=tol, blend=0.5, max_halvings=6)
    tm, sm = out["timing"], out["samples"]
    st = sm["status"]
    ok = st == 0
    print(f"N = {N}: " + ", ".join(f"{(st == s).sum()} {names[s]}" for s in sorted(set(st.tolist()))) +
          f"; {sm['count'][ok].sum()} rows at {1 / dt:.0f} Hz, the longest trajectory {sm['count'].max() * dt:.2f} s")
    if not ok.any():
        continue
    # the limits hold at the grid points; between them only as far as the grid is fine
    grid_t = np.nanmax(np.abs(tm["torques"][ok]) / effort, axis=(1, 2))
    print(f"    torque / limit: {grid_t.max():.3f} at the grid points, {sm['peak_torque_ratio'][ok].max():.3f} over the samples; "
          f"speed / limit over the samples {sm['peak_velocity_ratio'][ok].max():.3f}")
    over = ok & ((sm["peak_torque_ratio"] > 1.01) | (sm["peak_velocity_ratio"] > 1.01))
    print(f"    {over.sum()} of {ok.sum()} trajectories leave a limit by more than 1 % between grid points" +
          (" - raise N for them" if over.any() else ""))
    dist = arm.distances(sm["positions"][ok & (out["blend"]["status"] == 0)])
    print(f"    smallest clearance over the sampled configurations of the blended paths: "
          f"{min(dist['dist_world'].min(), dist['dist_self'].min()):+.3f} m (margin {margin})")

# the rows go straight into the controller: row k is t = k dt, the rows behind a trajectory's count hold its goal at rest
b = int(np.flatnonzero(ok)[0])
c = sm["count"][b]
print(f"trajectory {b}: {c} rows; q[0] = start {np.array_equal(sm['positions'][b, 0], out['blend']['points'][b, 0])}, "
      f"q[count - 1] = goal at rest {not sm['velocities'][b, c - 1].any()}, holding torque {np.round(sm['torques'][b, c - 1], 2)}")
