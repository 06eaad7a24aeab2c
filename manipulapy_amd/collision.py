"""Sphere-model collision checking for batches of configurations: signed distances to primitive obstacles and between the robot's
own spheres, the CHOMP hinge cost and its gradient (csrc/mp_collision.h; the conventions are those of include/manipula_hip.h).

The robot is S spheres, each fixed to a link (0 = the base .. n) and given by its centre in the space frame at q = 0; the world is a
table of spheres, capsules and oriented boxes that can be replaced at any time, and optionally a point cloud - a sensed scene as
points or occupied voxels with one radius, one more obstacle after the table's (`set_cloud`, `set_cloud_from_voxels`;
csrc/mp_cloud.h).  Every query and planner of the model sees both.  No meshes: `potential_field.CollisionChecker` keeps mirroring
the reference's mesh-less checker and is not touched by this module.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import _hip
from .registry import execute_registered_kernel

__all__ = ["SphereCollisionModel", "COLLISION_OP", "EDGES_OP", "PLAN_OP", "SHORTCUT_OP", "GOAL_OP", "BLEND_OP"]

# The registry's sorted name list starts with "control.pd_regulation" (the unknown-name message is pinned by a test), so the operation
# lives in the "planning" family rather than in one of its own that would sort ahead of it.
COLLISION_OP = "planning.collision_spheres"
EDGES_OP = "planning.collision_edges"
PLAN_OP = "planning.rrt_connect"
SHORTCUT_OP = "planning.shortcut_paths"
GOAL_OP = "planning.goal_configurations"
BLEND_OP = "planning.blend_paths"
CARTESIAN_OP = "planning.cartesian_paths"


def _hip_model_of(obj) -> _hip.HipModel:
    if isinstance(obj, _hip.HipModel):
        return obj
    if hasattr(obj, "_kin_model"):            # SerialManipulator
        return obj._kin_model()
    if hasattr(obj, "_derivative_model"):     # ManipulatorDynamics
        return obj._derivative_model("SphereCollisionModel")
    raise TypeError(f"expected a SerialManipulator, a ManipulatorDynamics or a compiled model, got {type(obj).__name__}")


class SphereCollisionModel:
    """links (S,) in 0..n, centres (S, 3) in the space frame at the home configuration, radii (S,), pairs (P, 2) of sphere indices
    checked against each other (None: no self-collision pairs)."""

    def __init__(self, serial_manipulator_or_dynamics, links, centres, radii, pairs=None):
        self.model = _hip_model_of(serial_manipulator_or_dynamics)
        self.n = self.model.n
        self.links = np.asarray(links, dtype=np.int32).reshape(-1).copy()
        self.centres = np.asarray(centres, dtype=np.float64).reshape(-1, 3).copy()
        self.radii = np.asarray(radii, dtype=np.float64).reshape(-1).copy()
        self.pairs = np.zeros((0, 2), dtype=np.int32) if pairs is None else np.asarray(pairs, dtype=np.int32).reshape(-1, 2).copy()
        self.handle = _hip.HipCollision(self.model, self.links, self.centres, self.radii, self.pairs)
        self.kinds = np.zeros(0, dtype=np.int32)
        self.params = np.zeros((0, 16))
        self._cloud = None  # (points (M, 3), radius, d_max, cell) as given, or None
        self._version = 0
        self._cloud_version = 0
        self._uploaded = {}  # id(context) -> (world version, cloud version) on its device

    # ------------------------------------------------------------------ construction from a kinematic chain
    @classmethod
    def from_points(cls, serial_manipulator_or_dynamics, points, radius, spacing=None, base_radius=None, base_centre=None,
                    pair_clearance: float = 0.0):
        """Spheres of `radius` strung along the segments points[i] -> points[i + 1], i = 0..n-1 (home positions in the space frame);
        segment i moves with link i + 1.  A segment of length L gets max(1, ceil(L / spacing)) spheres, evenly spread (spacing
        defaults to the radius); a zero-length segment gets one.  `base_radius` adds one sphere on link 0 at `base_centre` (default:
        the origin).  Default pairs: all pairs on links at least two apart whose home clearance exceeds `pair_clearance`."""
        pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
        n = pts.shape[0] - 1
        radius = float(radius)
        step = radius if spacing is None else float(spacing)
        if not (radius > 0 and step > 0):
            raise ValueError("radius and spacing must be positive")
        links, centres, radii = [], [], []
        if base_radius is not None:
            links.append(0)
            centres.append(np.zeros(3) if base_centre is None else np.asarray(base_centre, dtype=np.float64).reshape(3))
            radii.append(float(base_radius))
        for i in range(n):
            a, b = pts[i], pts[i + 1]
            m = max(1, int(np.ceil(np.linalg.norm(b - a) / step - 1e-9)))
            for k in range(m):
                links.append(i + 1)
                centres.append(a + (k + 0.5) / m * (b - a))
                radii.append(radius)
        links, centres, radii = np.array(links, dtype=np.int32), np.array(centres), np.array(radii)
        if len(links) > _hip.MP_COLLISION_MAX_SPHERES:
            raise ValueError(f"{len(links)} spheres, more than {_hip.MP_COLLISION_MAX_SPHERES}: raise the spacing")
        return cls(serial_manipulator_or_dynamics, links, centres, radii, cls.default_pairs(links, centres, radii, pair_clearance))

    @staticmethod
    def default_pairs(links, centres, radii, pair_clearance: float = 0.0) -> np.ndarray:
        """All pairs (a < b) on links at least two apart whose clearance |c_a - c_b| - r_a - r_b at the home configuration exceeds
        `pair_clearance` (0: the spheres do not overlap).  A pair that sits permanently below margin + tol blocks every edge of
        `check_edges` at t = 0: give a `pair_clearance` above that sum to leave such pairs out."""
        out = []
        for a in range(len(links)):
            for b in range(a + 1, len(links)):
                if abs(int(links[a]) - int(links[b])) >= 2 and np.linalg.norm(centres[a] - centres[b]) > radii[a] + radii[b] + pair_clearance:
                    out.append((a, b))
        return np.array(out, dtype=np.int32).reshape(-1, 2)

    @classmethod
    def from_urdf(cls, processor, radius, spacing=None, base_radius=None, pair_clearance: float = 0.0):
        """From a URDFToSerialManipulator: the points are the home origins of the child links of consecutive actuated joints, then
        the end effector (processor.link_fk(zeros)); the base sphere, if asked for, sits at the root link's origin.  Link k is the
        child link of actuated joint k (a gripper's mimic finger is not modelled: the screw model holds it still)."""
        by_child = {j.child: j for j in processor._tree["chain"]}
        prev = None
        for j in processor._tree["actuated"]:  # each actuated joint must hang off the previous one's child through fixed joints
            cur = j.parent
            while prev is not None and cur != prev.child:
                up = by_child.get(cur)
                if up is None or up in processor._tree["actuated"] or up.mimic is not None:
                    raise ValueError(f"from_urdf: joint {j.name} is not downstream of {prev.name}: the actuated joints are not one chain")
                cur = up.parent
            prev = j
        home = processor.link_fk(np.zeros(processor.num_dofs))
        names = [j.child for j in processor._tree["actuated"]] + [processor.end_effector_name]
        pts = np.array([home[name][:3, 3] for name in names])
        root = processor._tree["roots"][0]
        return cls.from_points(processor.serial_manipulator, pts, radius, spacing, base_radius, home[root][:3, 3], pair_clearance)

    # ------------------------------------------------------------------ the world
    def set_world(self, spheres=None, capsules=None, boxes=None) -> None:
        """spheres (k, 4) rows [centre, r]; capsules (k, 7) rows [p0, p1, r]; boxes (k, 15) rows [centre, R row-major, half-extents]
        or a list of (centre, R (3, 3), half_extents) triples.  The table holds the spheres, then the capsules, then the boxes:
        obstacle indices in `arg_world` count in that order.  Replaces the previous world; the sphere model is not rebuilt."""
        kinds, rows = [], []
        for kind, data, width in ((_hip.OBSTACLE_SPHERE, spheres, 4), (_hip.OBSTACLE_CAPSULE, capsules, 7), (_hip.OBSTACLE_BOX, boxes, 15)):
            if data is None or len(data) == 0:
                continue
            if kind == _hip.OBSTACLE_BOX and not isinstance(data, np.ndarray):
                data = [np.concatenate([np.asarray(c, dtype=np.float64).reshape(3), np.asarray(R, dtype=np.float64).reshape(9),
                                        np.asarray(h, dtype=np.float64).reshape(3)]) for c, R, h in data]
            arr = np.asarray(data, dtype=np.float64).reshape(-1, width)
            for r in arr:
                kinds.append(kind)
                rows.append(np.concatenate([r, np.zeros(16 - width)]))
        self.set_world_table(kinds, np.array(rows).reshape(-1, 16))

    def set_world_table(self, kinds, params) -> None:
        """The obstacle table as the C interface takes it: kinds (O,), params (O, 16)."""
        kinds = np.asarray(kinds, dtype=np.int32).reshape(-1)
        params = np.asarray(params, dtype=np.float64).reshape(-1, 16)
        self.handle.set_world(kinds, params)   # validates; the CPU twin reads this copy
        self.kinds, self.params = kinds.copy(), params.copy()
        self._version += 1

    def set_cloud(self, points, radius: float, d_max: float, cell: Optional[float] = None) -> None:
        """A point cloud as one more obstacle after the table's: points (M, 3), every one a ball of `radius` (>= 0), the distance cut
        off at `d_max` (> 0): sd(p) = min(d_max, min_i |p - x_i| - radius), exact for the union of the balls below d_max and never
        above the true distance.  `arg_world`'s obstacle index is O + i for point i, O + M where the value is the cut-off one.  The
        cost has one hinge term per (robot sphere, cloud), exact whenever d_max >= eps_world + the largest sphere radius; the edge
        check and every planner treat the cloud like any obstacle, and far from it a step of theirs is limited by d_max.  `cell`
        (None: d_max + radius) is the edge of the grid the points are sorted into; it may be as small as a quarter of the default
        (fewer points per cell, up to 729 cells a query instead of 27).  Replaces the previous cloud; the primitive table stays.
        CAPTURED GRAPHS: a launch picks the kernels that look at the cloud only when the model has one at that moment.  A graph
        captured while a cloud was set sees every later cloud (and a cleared one) when replayed; a graph captured BEFORE the first
        `set_cloud` keeps running without the cloud and ignores it silently - capture again after setting one."""
        pts = np.array(points, dtype=np.float64).reshape(-1, 3)
        if pts.shape[0] == 0:
            return self.clear_cloud()
        self.handle.set_cloud(pts, radius, d_max, 0.0 if cell is None else cell)   # validates; the CPU twin reads this copy
        self._cloud = (pts, float(radius), float(d_max), self.handle.cloud_info()["cell"])
        self._cloud_version += 1

    def clear_cloud(self) -> None:
        """Removes the point cloud: the world is the primitive table alone again."""
        self.handle.set_cloud(np.zeros((0, 3)), 0.0, 1.0)
        self._cloud = None
        self._cloud_version += 1

    def set_cloud_from_voxels(self, occupancy, origin, pitch: float, d_max: float, cell: Optional[float] = None) -> None:
        """The occupied voxels of a (nx, ny, nz) bool grid as a cloud: voxel (i, j, k) is the cube of edge `pitch` whose lowest corner
        is origin + pitch (i, j, k); its centre becomes a point and radius = pitch sqrt(3) / 2, so the balls cover the cubes."""
        occ = np.asarray(occupancy, dtype=bool)
        if occ.ndim != 3:
            raise ValueError(f"occupancy must be (nx, ny, nz); got {occ.shape}")
        pitch = float(pitch)
        if not (pitch > 0 and np.isfinite(pitch)):
            raise ValueError("pitch must be positive and finite")
        centres = np.asarray(origin, dtype=np.float64).reshape(3) + pitch * (np.argwhere(occ) + 0.5)
        self.set_cloud(centres, pitch * np.sqrt(3.0) / 2.0, d_max, cell)

    @property
    def cloud(self) -> Optional[dict]:
        """{"points" (M, 3), "radius", "d_max", "cell"} of the current cloud, or None."""
        if self._cloud is None:
            return None
        pts, radius, d_max, cell = self._cloud
        return {"points": pts.copy(), "radius": radius, "d_max": d_max, "cell": cell}

    def sync_world(self, ctx) -> None:
        """Makes the world on `ctx`'s device the current one, table and cloud (copies behind the launches already on its stream;
        no-op when it is)."""
        have = self._uploaded.get(id(ctx), (None, 0))
        if have[0] != self._version:
            self.handle.set_world(self.kinds, self.params, ctx=ctx)
        if have[1] != self._cloud_version:
            if self._cloud is None:
                self.handle.set_cloud(np.zeros((0, 3)), 0.0, 1.0, ctx=ctx)
            else:
                pts, radius, d_max, cell = self._cloud
                self.handle.set_cloud(pts, radius, d_max, cell, ctx=ctx)
        self._uploaded[id(ctx)] = (self._version, self._cloud_version)

    # ------------------------------------------------------------------ queries
    def _run(self, q, eps_world, eps_self, want):
        q = np.asarray(q, dtype=np.float64)
        if q.ndim not in (1, 2, 3) or q.shape[-1] != self.n:
            raise ValueError(f"q must be ({self.n},), (rows, {self.n}) or (B, N, {self.n}); got {q.shape}")
        lead = q.shape[:-1]
        out = execute_registered_kernel(COLLISION_OP, self, np.ascontiguousarray(q.reshape(-1, self.n)), eps_world, eps_self, want)
        return {k: v.reshape(lead + v.shape[1:]) for k, v in out.items()}

    def distances(self, q, want_grad: bool = False) -> dict:
        """dist_world, arg_world, dist_self, arg_self of every row of q ((rows, n) or (B, N, n)); with `want_grad` also
        grad_dist_world and grad_dist_self.
        The world is the obstacle table of `set_world` and the point cloud of `set_cloud`, if one is set."""
        want = ("dist_world", "arg_world", "dist_self", "arg_self") + (("grad_dist_world", "grad_dist_self") if want_grad else ())
        return self._run(q, 1.0, 1.0, want)

    def cost(self, q, eps_world, eps_self, want_grad: bool = True):
        """The hinge cost of every row, and its gradient with `want_grad`: cost, or (cost, grad).
        The world is the obstacle table of `set_world` and the point cloud of `set_cloud`, if one is set."""
        r = self._run(q, eps_world, eps_self, ("cost", "grad") if want_grad else ("cost",))
        return (r["cost"], r["grad"]) if want_grad else r["cost"]

    def in_collision(self, q, margin: float = 0.0) -> np.ndarray:
        """True where the world or the self clearance of a row is below `margin`."""
        r = self._run(q, 1.0, 1.0, ("dist_world", "dist_self"))
        return (r["dist_world"] < margin) | (r["dist_self"] < margin)

    # ------------------------------------------------------------------ edges
    def motion_bounds(self) -> np.ndarray:
        """rho (n, n + 1): rho[j - 1, k] = the largest distance a sphere centre of link k can have from the axis of the revolute
        joint j <= k (prismatic joints between them not counted); 0 for a prismatic j, for k < j and for a link without spheres."""
        return self.handle.motion_bounds()

    def check_edges(self, q_from, q_to, margin: float = 0.0, tol: float = 1e-3, max_steps: int = 512, want=None) -> dict:
        """Continuous check of the straight joint-space motions q_from -> q_to ((E, n) or any common leading shape) by conservative
        advancement: {"status" (0 free, 1 blocked, 2 undecided, -1 invalid), "t", "steps", "clearance", "witness" (.., 3)} or the
        subset named in `want`.  FREE proves clearance > margin on the whole edge; BLOCKED stops at the first evaluated t whose
        clearance is <= margin + tol, with [0, t) proven; UNDECIDED (max_steps evaluations) proves [0, t).
        The world is the obstacle table of `set_world` and the point cloud of `set_cloud`, if one is set."""
        qa, qb = np.asarray(q_from, dtype=np.float64), np.asarray(q_to, dtype=np.float64)
        if qa.shape != qb.shape or qa.ndim < 1 or qa.shape[-1] != self.n:
            raise ValueError(f"q_from and q_to must have one shape (..., {self.n}); got {qa.shape} and {qb.shape}")
        lead = qa.shape[:-1]
        out = execute_registered_kernel(EDGES_OP, self, np.ascontiguousarray(qa.reshape(-1, self.n)),
                                        np.ascontiguousarray(qb.reshape(-1, self.n)), margin, tol, max_steps, want)
        return {k: v.reshape(lead + v.shape[1:]) for k, v in out.items()}

    # ------------------------------------------------------------------ planning
    def plan_paths(self, q_start, q_goal, lo, hi, margin: float = 0.0, tol: float = 1e-3, *, step: float, min_advance=None,
                   max_iters: int, max_nodes: int, max_waypoints: int, max_steps: int = 64, seed: int = 0, want=None) -> dict:
        """Bidirectional RRT-Connect for B independent problems q_start -> q_goal ((B, n) or any common leading shape) in the
        sampling box lo, hi (n): {"status" (0 solved, 1 exhausted, 2 tree full, 3 start blocked, 4 goal blocked, 5 path too long,
        -1 invalid), "count", "waypoints" (.., max_waypoints, n), "iterations", "nodes" (.., 2), "evaluations"} or the subset named
        in `want`.  Every tree edge, and so every segment of a returned path, is proven free by `check_edges`' conservative
        advancement with this margin, tol and max_steps; a path is padded by repeating its last waypoint.  `min_advance` defaults
        to step / 8.  A problem's result depends on its content and `seed` only.  The launch lasts as long as its slowest problem:
        `max_iters` is the latency knob.
        The world is the obstacle table of `set_world` and the point cloud of `set_cloud`, if one is set."""
        qs, qg = np.asarray(q_start, dtype=np.float64), np.asarray(q_goal, dtype=np.float64)
        if qs.shape != qg.shape or qs.ndim < 1 or qs.shape[-1] != self.n:
            raise ValueError(f"q_start and q_goal must have one shape (..., {self.n}); got {qs.shape} and {qg.shape}")
        lead = qs.shape[:-1]
        out = execute_registered_kernel(PLAN_OP, self, np.ascontiguousarray(qs.reshape(-1, self.n)),
                                        np.ascontiguousarray(qg.reshape(-1, self.n)), lo, hi, margin, tol, step=step,
                                        min_advance=min_advance, max_iters=max_iters, max_nodes=max_nodes, max_waypoints=max_waypoints,
                                        max_steps=max_steps, seed=seed, want=want)
        return {k: v.reshape(lead + v.shape[1:]) for k, v in out.items()}

    def shortcut_paths(self, waypoints, count, margin: float = 0.0, tol: float = 1e-3, *, max_iters: int, min_gain: float = 0.0,
                       max_waypoints=None, max_steps: int = 64, seed: int = 0, want=None) -> dict:
        """Randomised shortcutting of B piecewise-linear paths, waypoints (B, W, n) with count (B,) real rows each (any common leading
        shape; `plan_paths`' "waypoints" and "count" go straight in): {"status" (0 done, 1 straight, 2 skipped: fewer than two
        waypoints, -1 invalid), "count", "waypoints" (.., max_waypoints, n), "length_in", "length_out", "iterations", "accepted",
        "skipped_full", "evaluations"} or the subset named in `want`.  Per iteration two points are drawn on the path by arc length;
        if the straight motion between them is shorter by more than `min_gain` and is proven free by `check_edges`' conservative
        advancement with this margin, tol and max_steps, it replaces the piece between them.  `max_waypoints` (None: the input's W)
        is the room of an output path: a shortcut inside one segment pair can add a waypoint, and one that would not fit is counted
        in "skipped_full".  Every new segment is proven free and pieces of input segments are kept, so the output is as free as the
        input; THE INPUT IS NOT CHECKED (OptimizedTrajectoryPlanning.batch_validate_path does that).  A path is padded by repeating
        its last waypoint.  A problem's result depends on its content and `seed` only.
        The world is the obstacle table of `set_world` and the point cloud of `set_cloud`, if one is set."""
        wp, cnt = np.asarray(waypoints, dtype=np.float64), np.asarray(count)
        if wp.ndim < 3 or wp.shape[-1] != self.n or cnt.shape != wp.shape[:-2]:
            raise ValueError(f"waypoints must be (..., W, {self.n}) and count its leading shape; got {wp.shape} and {cnt.shape}")
        lead = wp.shape[:-2]
        out = execute_registered_kernel(SHORTCUT_OP, self, np.ascontiguousarray(wp.reshape((-1,) + wp.shape[-2:])),
                                        cnt.reshape(-1), margin, tol, max_iters=max_iters,
                                        min_gain=min_gain, max_waypoints=max_waypoints, max_steps=max_steps, seed=seed, want=want)
        return {k: v.reshape(lead + v.shape[1:]) for k, v in out.items()}

    def blend_paths(self, waypoints, count, N: int, margin: float = 0.0, tol: float = 1e-3, *, blend: float = 0.5, max_halvings: int = 6,
                    max_steps: int = 64, want=None) -> dict:
        """C2 corner blending of B piecewise-linear paths, waypoints (B, W, n) with count (B,) real rows each (any common leading
        shape; `plan_paths`' or `shortcut_paths`' "waypoints" and "count" go straight in), sampled on the N grid points s_i = i / (N -
        1): {"status" (0 done, 1 straight, 2 skipped: fewer than two waypoints, 3 point, 4 blocked, 5 reversal, -1 invalid), "corner",
        "count", "points" (.., W, n), "cut", "knot" (.., W), "length", "halvings", "evaluations", "clearance", "q", "dq", "ddq" (.., N,
        n)} or the subset named in `want`.  Repeated waypoints are dropped; every interior corner is then replaced by a quintic blend
        that leaves the two segments at most `blend` (joint-space length) from the corner and is proven free by `check_edges`'
        conservative advancement with this margin, tol and max_steps; a blend that is not proven is tried again at half the cut, up
        to `max_halvings` times, and a corner that is never proven makes the path blocked ("corner": its index in "points").  A
        path that doubles back on itself is a reversal.  "q", "dq", "ddq" are the curve and its first two derivatives in s, the
        arguments of OptimizedTrajectoryPlanning.batch_time_optimal_parameterization; rows without a curve are NaN.  The linear
        pieces are pieces of input segments and ARE NOT CHECKED (OptimizedTrajectoryPlanning.batch_validate_path does that).  A
        problem's result depends on its content only.
        The world is the obstacle table of `set_world` and the point cloud of `set_cloud`, if one is set."""
        wp, cnt = np.asarray(waypoints, dtype=np.float64), np.asarray(count)
        if wp.ndim < 3 or wp.shape[-1] != self.n or cnt.shape != wp.shape[:-2]:
            raise ValueError(f"waypoints must be (..., W, {self.n}) and count its leading shape; got {wp.shape} and {cnt.shape}")
        lead = wp.shape[:-2]
        out = execute_registered_kernel(BLEND_OP, self, np.ascontiguousarray(wp.reshape((-1,) + wp.shape[-2:])), cnt.reshape(-1), N,
                                        margin, tol, blend=blend, max_halvings=max_halvings, max_steps=max_steps, want=want)
        return {k: v.reshape(lead + v.shape[1:]) for k, v in out.items()}

    # ------------------------------------------------------------------ Cartesian lines
    def cartesian_paths(self, q_start, T_goal, lo, hi, N: int, margin: float = 0.0, tol: float = 1e-3, *, task: str = "full",
                        eomg: float = 1e-6, ev: float = 1e-6, damping: float = 0.01, max_iters: int = 20, max_joint_step: float = 0.5,
                        max_steps: int = 64, want=None) -> dict:
        """Straight tool lines from B start configurations q_start (B, n) to B poses T_goal ((B, 4, 4), or any common leading shape)
        inside the box lo, hi (n), on the N grid points s_i = i / (N - 1): {"status" (0 done, 1 stalled, 2 singular, 3 limit, 4 jump,
        5 blocked, 6 undecided, -1 invalid), "reached", "span", "t", "clearance", "deviation_pos", "deviation_rot", "pose_error",
        "iterations", "evaluations", "q", "dq", "ddq" (.., N, n), "span_status", "span_clearance" (.., N - 1)} or the subset named in
        `want`.  The tool origin moves on the segment from its start to the goal's while (task "full") the orientation turns about
        one axis at a constant rate; task "position" leaves the orientation free.  Every grid point is tracked from its predecessor
        by at most `max_iters` damped Newton steps to within `eomg` / `ev`; a point that does not converge (stalled), leaves the box
        (limit), moves a joint by more than `max_joint_step` (jump) or is singular ends the problem, "reached" points in.  "q", "dq",
        "ddq" are the joint curve and its derivatives in s, the arguments of
        OptimizedTrajectoryPlanning.batch_time_optimal_parameterization and of batch_sample_time_optimal(path=...); every span of
        their quintic Hermite interpolant - the curve that sampler executes - is proven free by `check_edges`' conservative
        advancement with this margin, tol and max_steps, or the problem is blocked / undecided at "span", "t".  "deviation_pos" /
        "deviation_rot": how far the interpolant leaves the line at the spans' midpoints (raise N when it is too much).  A problem's
        result depends on its content only.
        The world is the obstacle table of `set_world` and the point cloud of `set_cloud`, if one is set."""
        Tg, q0 = np.asarray(T_goal, dtype=np.float64), np.asarray(q_start, dtype=np.float64)
        if Tg.ndim < 2 or Tg.shape[-2:] != (4, 4) or q0.ndim < 1 or q0.shape[-1] != self.n or Tg.shape[:-2] != q0.shape[:-1]:
            raise ValueError(f"T_goal must be (..., 4, 4) and q_start (..., {self.n}) with one leading shape; got {Tg.shape} and {q0.shape}")
        lead = q0.shape[:-1]
        out = execute_registered_kernel(CARTESIAN_OP, self, np.ascontiguousarray(q0.reshape(-1, self.n)),
                                        np.ascontiguousarray(Tg.reshape(-1, 16)), lo, hi, N, margin, tol, task=task, eomg=eomg, ev=ev,
                                        damping=damping, max_iters=max_iters, max_joint_step=max_joint_step, max_steps=max_steps, want=want)
        return {k: v.reshape(lead + v.shape[1:]) for k, v in out.items()}

    # ------------------------------------------------------------------ pose goals
    def goal_configurations(self, T_goal, q_seed, lo, hi, margin: float = 0.0, tol: float = 1e-3, *, eomg: float, ev: float,
                            damping: float, step_cap: float, max_iters: int, max_attempts: int, seed: int = 0, want=None) -> dict:
        """Collision-free joint configurations for B end-effector poses T_goal ((B, 4, 4) with seeds q_seed (B, n), or any common
        leading shape) inside the box lo, hi (n): {"status" (0 found, 1 in collision, 2 unreached, -1 invalid), "q" (.., n),
        "attempts", "iterations", "converged", "pose_error" (.., 2: rotation angle, distance), "clearance", "witness" (.., 3)} or the
        subset named in `want`.  Up to `max_attempts` damped Newton attempts of at most `max_iters` steps each on the hybrid Jacobian
        (damping `damping`, steps capped at `step_cap`, clamped into the box), the first from the clamped seed and the later ones
        from random points of the box; an attempt converges when the rotation error is below `eomg` and the position error below
        `ev`.  Every converged attempt gets the zero-edge decision of `check_edges(q, q)` with this margin and tol - the decision
        `plan_paths` makes for its q_goal: the first FREE one is returned as found; if none is free, the converged configuration of
        the largest clearance comes back as in collision; if none converged, NaN as unreached.  "q" goes straight into `plan_paths`
        as q_goal: a found row is never goal-blocked there under the same margin and tol.  A problem's result depends on its content
        and `seed` only.
        The world is the obstacle table of `set_world` and the point cloud of `set_cloud`, if one is set."""
        Tg, q0 = np.asarray(T_goal, dtype=np.float64), np.asarray(q_seed, dtype=np.float64)
        if Tg.ndim < 2 or Tg.shape[-2:] != (4, 4) or q0.ndim < 1 or q0.shape[-1] != self.n or Tg.shape[:-2] != q0.shape[:-1]:
            raise ValueError(f"T_goal must be (..., 4, 4) and q_seed (..., {self.n}) with one leading shape; got {Tg.shape} and {q0.shape}")
        lead = q0.shape[:-1]
        out = execute_registered_kernel(GOAL_OP, self, np.ascontiguousarray(Tg.reshape(-1, 16)), np.ascontiguousarray(q0.reshape(-1, self.n)),
                                        lo, hi, margin, tol, eomg=eomg, ev=ev, damping=damping, step_cap=step_cap, max_iters=max_iters,
                                        max_attempts=max_attempts, seed=seed, want=want)
        return {k: v.reshape(lead + v.shape[1:]) for k, v in out.items()}
