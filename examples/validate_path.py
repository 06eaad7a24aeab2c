#!/usr/bin/env python3
"""Continuous validation of piecewise-linear joint-space paths: is every segment free over its whole length, and if not, where does
the path stop?  Conservative advancement proves the answer with a few dozen evaluations a segment where sampling would need hundreds to thousands.

    python examples/validate_path.py [hip]      (NumPy backend unless "hip" is given, which needs an MI355X)
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

# keep 2 cm from everything and stop within 1 mm of that; pairs that sit closer than 5 cm at home would block every motion, so they
# are left out of the model
margin, tol = 0.02, 1e-3
arm = mp.SphereCollisionModel.from_urdf(proc, radius=0.06, base_radius=0.1, pair_clearance=0.05)
tilt = np.array([[np.cos(0.3), -np.sin(0.3), 0.0], [np.sin(0.3), np.cos(0.3), 0.0], [0.0, 0.0, 1.0]])
arm.set_world(boxes=[([0.55, 0.0, 0.10], np.eye(3), [0.20, 0.40, 0.10]),
                     ([0.10, 0.55, 0.40], tilt, [0.05, 0.05, 0.40]),
                     ([-0.30, -0.45, 0.75], np.eye(3), [0.25, 0.15, 0.02])])
print(f"{len(arm.links)} spheres, {len(arm.pairs)} self-collision pairs, {len(arm.kinds)} obstacles")

# 64 paths of 5 random waypoints that are themselves free
rng = np.random.default_rng(0)
lim = proc.joint_limits_array
mid, half = lim.mean(axis=1), np.minimum(0.5 * (lim[:, 1] - lim[:, 0]), 2.0)
pool = mid + rng.uniform(-1, 1, (8192, 6)) * half
d = arm.distances(pool)
pool = pool[np.minimum(d["dist_world"], d["dist_self"]) > margin + 0.03]
paths = pool[:64 * 5].reshape(64, 5, 6)

r = planner.batch_validate_path(paths, arm, margin, tol)
print(f"{r['free'].sum()} of 64 paths are free over their whole length (every waypoint is)")
for b in range(8):
    if r["free"][b]:
        print(f"path {b}: free, smallest clearance met {r['clearance'][b]:+.3f} m")
    else:
        seg = r["first_blocked_segment"][b]
        print(f"path {b}: stops at {r['blocked_at'][b]:.3f} (segment {seg}), clearance {r['clearance'][b]:+.3f} m")

# one edge in detail: the evaluations it took and what came closest
e = arm.check_edges(paths[:, 0], paths[:, 1], margin, tol)
kinds = {0: "sphere / obstacle", 1: "sphere / sphere"}
for b in range(4):
    w = e["witness"][b]
    print(f"edge {b}: status {e['status'][b]}, t {e['t'][b]:.4f} after {e['steps'][b]} evaluations; closest: {kinds.get(w[0], 'none')} {w[1:]}")
print(f"evaluations per edge: mean {e['steps'].mean():.1f}, max {e['steps'].max()}")
