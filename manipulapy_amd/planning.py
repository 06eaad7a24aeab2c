"""OptimizedTrajectoryPlanning — host-side mirror of the reference planner facade for the hot path.

Reference: ManipulaPy/planning/trajectory_planning.py:116-399 (constructor, routing),
planning/trajectory.py:103-502 (joint / batch trajectories), planning/trajectory_dynamics.py:31-90,
:308-380 (inverse_dynamics_trajectory), :710-735 (calculate_derivatives).

What is kept: the constructor signature (positional + keyword-only arguments), float32 limits,
`performance_stats`, the `_should_use_gpu` routing rule (forced CPU pin -> live routing predicate ->
work threshold), result dtypes / shapes (float32 (N, n) / (B, N, n)), joint-limit and torque-limit
clipping, default gravity / zero wrench.

What is different, on purpose:
  * a failing GPU launch raises instead of silently recomputing on the CPU
    (reference planning/trajectory.py:270-274, trajectory_dynamics.py:292-302);
  * with the NumPy backend active (or use_cuda=False) every operation runs its registered CPU launcher
    (NumPy for trajectory generation, the C ABI's *_cpu twins for the dynamics), as the reference's
    planner runs its _*_cpu methods; with the "hip" backend active and no usable GPU it raises instead
    of quietly computing on the host;
  * with the "hip" backend the dynamics always go to the device (the reference applies its work
    threshold to them too; a launch costs microseconds here, so the threshold only steers trajectory
    generation, whose NumPy path is BASELINE config 0);
  * collision avoidance: the mesh-less checker (never a collision, like the reference's without mesh files) and `plan_trajectory`'s
    potential-field waypoint push are in; mesh loading is not;
  * `batch_inverse_dynamics_trajectory` is new: joint_trajectory -> inverse_dynamics_trajectory fused
    on the device for B start/end pairs; `batch_forward_dynamics_trajectory` is new: B roll-outs of
    forward_dynamics_trajectory (planning/trajectory_dynamics.py:580-708) in one launch.
"""
from __future__ import annotations

import logging
import os
import time
import warnings
from typing import Dict, Optional, Tuple

import numpy as np

from . import _hip
from . import registry as _reg
from .backend import get_backend

__all__ = ["OptimizedTrajectoryPlanning", "TrajectoryPlanning"]

logger = logging.getLogger("ManipulaPy.planning.trajectory_planning")  # name kept


class OptimizedTrajectoryPlanning:
    def __init__(self, serial_manipulator, urdf_path, dynamics, joint_limits, torque_limits=None, *,
                 use_cuda: Optional[bool] = None, cuda_threshold: int = 10, memory_pool_size_mb: Optional[int] = None,
                 enable_profiling: bool = False, auto_optimize: bool = True, kernel_type: str = "auto",
                 target_speedup: float = 40.0) -> None:
        self.serial_manipulator = serial_manipulator
        self.dynamics = dynamics
        self.urdf_path = urdf_path
        self.joint_limits = np.asarray(joint_limits, dtype=np.float32)
        self.torque_limits = (np.asarray(torque_limits, dtype=np.float32) if torque_limits is not None
                              else np.array([[-np.inf, np.inf]] * len(joint_limits), dtype=np.float32))
        # the limits as given, unrounded: what the float64 time-optimal parameterisation takes for torque_limits=None
        self._torque_limits_f64 = (np.array(torque_limits, dtype=np.float64) if torque_limits is not None
                                   else self.torque_limits.astype(np.float64))
        self.kernel_type = kernel_type if kernel_type is not None else "auto"
        self.target_speedup = target_speedup if target_speedup is not None else 40.0
        self.enable_profiling = bool(enable_profiling)
        # collision helpers as the reference sets them up (planning/trajectory_planning.py:229-238): both, or neither when the
        # URDF cannot be read.  The checker is the mesh-less one (potential_field.py): it never reports a collision.
        try:
            from .potential_field import CollisionChecker, PotentialField

            self.collision_checker = CollisionChecker(urdf_path)
            self.potential_field = PotentialField()
        except Exception as exc:
            logger.warning("Could not initialise collision checker: %s", exc)
            self.collision_checker = None
            self.potential_field = None
        self._last_cpu_time = 0.0
        self.performance_stats = {"gpu_calls": 0, "cpu_calls": 0, "total_gpu_time": 0.0, "total_cpu_time": 0.0,
                                  "memory_transfers": 0, "kernel_launches": 0, "speedup_achieved": 0.0,
                                  "best_kernel_used": "none"}
        self.performance_stats.update({"gpu_kernel_ms_total": 0.0, "gpu_kernel_ms_last": 0.0, "gpu_timed_calls": 0})
        del auto_optimize, memory_pool_size_mb  # CUDA-environment knobs with no HIP counterpart

        physical = _reg.check_hip_availability()
        detected = _reg._hip_routing_enabled(physical)
        self._physical_cuda = physical
        self._forced_cpu = use_cuda is False
        if use_cuda is None:
            self.cuda_available = detected
        elif use_cuda and not detected:
            raise RuntimeError("use_cuda=True requested but no GPU-capable backend with a HIP device is active. "
                               "Select the 'hip' backend on a machine with an MI355X.")
        else:
            self.cuda_available = bool(use_cuda)
        self.gpu_properties = _reg.get_gpu_properties() if self.cuda_available else None
        if self.cuda_available and self.gpu_properties:
            cus = self.gpu_properties["multiprocessor_count"]
            per_cu = 1000 if self.target_speedup >= 40 else 500
            self.cpu_threshold = max(int(cuda_threshold), int(cus * per_cu / len(joint_limits)))
        else:
            self.cpu_threshold = int(cuda_threshold)
        self._model = None
        # reference planning/trajectory_planning.py:295-296 (profile_start): here a timed HIP event pair and an roctx
        # range around every launch of the context, read back into performance_stats after each GPU call
        self._profiling_held = False
        self._prof_base = {"kernel_ms_total": 0.0, "timed_calls": 0}
        if self.enable_profiling and self.cuda_available and self._gpu_routed():
            _reg.acquire_profiling()          # released by close() / __del__: the flag belongs to the shared context
            self._profiling_held = True
            self._prof_base = _reg.get_context().profile()   # this planner reports what was timed SINCE, not the context's totals

    # ------------------------------------------------------------------ plumbing
    def _hip_model(self):
        """Dynamics tables + THIS planner's float32 joint / torque limits, compiled once."""
        if self._model is None:
            self._model = self.dynamics.hip_model(self.joint_limits.astype(np.float64), self.torque_limits.astype(np.float64))
            if self._gpu_routed() and os.environ.get("MANIPULAPY_HIP_SPECIALIZE", "1") != "0" and self._model.n <= _hip.MP_MAX_DOF:
                # float32 kernels with this robot's constants baked in (hiprtc, ~1.5 s once, cached on disk);
                # purely an optimisation: the generic kernels compute the same values
                try:
                    _reg.get_context().specialize(self._model)
                except Exception as exc:  # pragma: no cover - depends on the hiprtc installation
                    logger.warning("kernel specialisation unavailable (%s); using the generic kernels", exc)
        return self._model

    def _should_use_gpu(self, N: int, num_joints: int) -> bool:
        """reference planning/trajectory_planning.py:356-399."""
        if getattr(self, "_forced_cpu", False):
            return False
        physical = getattr(self, "_physical_cuda", self.cuda_available)
        if not _reg._hip_routing_enabled(physical):
            return False
        return N * num_joints >= self.cpu_threshold

    def _gpu_routed(self) -> bool:
        """Routing for operations that exist only on the device (no work threshold)."""
        if getattr(self, "_forced_cpu", False):
            return False
        return _reg._hip_routing_enabled(getattr(self, "_physical_cuda", self.cuda_available))

    def _count(self, kind: str, t0: float) -> None:
        dt = time.time() - t0
        self.performance_stats[f"{kind}_calls"] += 1
        self.performance_stats[f"total_{kind}_time"] += dt
        if kind == "gpu":
            self.performance_stats["kernel_launches"] += 1
            self.performance_stats["best_kernel_used"] = "hip"
            if self.enable_profiling and self._profiling_held:
                p = _reg.get_context().profile()
                self.performance_stats.update({"gpu_kernel_ms_total": p["kernel_ms_total"] - self._prof_base["kernel_ms_total"],
                                               "gpu_kernel_ms_last": p["kernel_ms_last"],
                                               "gpu_timed_calls": p["timed_calls"] - self._prof_base["timed_calls"]})
        else:
            self._last_cpu_time = dt

    def _dispatch(self, name: str, *args, **kwargs):
        """Run a registered operation where the routing rule sends it: the GPU launcher when the "hip" backend is active
        and a device is there, otherwise the CPU launcher (NumPy backend, or this planner pinned to the CPU with
        use_cuda=False).  "hip" backend without a usable device: raises (registry._refuse_silent_cpu)."""
        entry = _reg.get_registered_kernel(name)
        t0 = time.time()
        if self._gpu_routed():
            out, route = _reg.run_gpu_launcher(entry, *args, **kwargs)   # "cpu" only under MANIPULAPY_HIP_FALLBACK=1 after a failed launch
            self._count(route, t0)
        else:
            if not self._forced_cpu:
                _reg._refuse_silent_cpu(name)
            out = entry.cpu_launcher(*args, **kwargs)
            self._count("cpu", t0)
        return out

    def _clip_positions(self, pos: np.ndarray) -> np.ndarray:
        return np.clip(pos, self.joint_limits[:, 0], self.joint_limits[:, 1])

    # ------------------------------------------------------------------ trajectories
    def joint_trajectory(self, thetastart, thetaend, Tf, N, method, kernel_type=None, enable_monitoring=None) -> Dict[str, np.ndarray]:
        """positions / velocities / accelerations, each (N, n) float32 (reference planning/trajectory.py:103-169)."""
        del enable_monitoring
        backend = get_backend()
        start = np.array(backend.to_numpy(backend.asarray(thetastart)), dtype=np.float32)
        end = np.array(backend.to_numpy(backend.asarray(thetaend)), dtype=np.float32)
        t0 = time.time()
        if self._should_use_gpu(int(N), len(start)):
            variant = kernel_type or self.kernel_type or "auto"
            entry = _reg.get_registered_kernel(f"trajectory.{variant}")  # fail-closed on unknown names
            (pos, vel, acc), route = _reg.run_gpu_launcher(entry, self._hip_model(), start, end, Tf, int(N), int(method))
            self._count(route, t0)
        else:
            pos, vel, acc = _reg.trajectory_cpu(start, end, float(Tf), int(N), int(method))
            pos = self._clip_positions(pos)
            self._count("cpu", t0)
        return {"positions": backend.asarray(pos), "velocities": backend.asarray(vel), "accelerations": backend.asarray(acc)}

    def batch_joint_trajectory(self, thetastart_batch, thetaend_batch, Tf, N, method, kernel_type=None) -> Dict[str, np.ndarray]:
        """(B, N, n) float32 arrays (reference planning/trajectory.py:335-502)."""
        del kernel_type
        backend = get_backend()
        sb = np.asarray(backend.to_numpy(backend.asarray(thetastart_batch)), dtype=np.float32)
        eb = np.asarray(backend.to_numpy(backend.asarray(thetaend_batch)), dtype=np.float32)
        if sb.ndim != 2 or sb.shape != eb.shape:
            raise ValueError(f"start/end batches must both be (B, n); got {sb.shape} and {eb.shape}")
        B, n = sb.shape
        t0 = time.time()
        if B == 0:
            z = np.zeros((0, int(N), n), dtype=np.float32)
            return {"positions": z, "velocities": z.copy(), "accelerations": z.copy()}
        if self._gpu_routed():
            (pos, vel, acc), route = _reg.run_gpu_launcher(_reg.get_registered_kernel("trajectory.batch"), self._hip_model(), sb, eb, Tf,
                                                           int(N), int(method))
            self._count(route, t0)
        else:
            pos, vel, acc = _reg.trajectory_cpu(sb, eb, float(Tf), int(N), int(method))
            pos = self._clip_positions(pos)
            self._count("cpu", t0)
        return {"positions": backend.asarray(pos), "velocities": backend.asarray(vel), "accelerations": backend.asarray(acc)}

    def cartesian_trajectory(self, Xstart, Xend, Tf, N, method) -> Dict[str, np.ndarray]:
        """Straight-line Cartesian trajectory between two SE(3) poses (reference planning/trajectory.py:504-594):
        positions / velocities / accelerations (N, 3) and orientations (N, 3, 3), float32."""
        Xs, Xe = np.asarray(Xstart, dtype=np.float64), np.asarray(Xend, dtype=np.float64)
        N = int(N)
        if N < 0:
            raise ValueError("negative dimensions are not allowed")
        if N == 0:  # the reference's empty shapes (:555-559, :727-730)
            return {"positions": np.zeros((0,), np.float32), "velocities": np.zeros((0, 3), np.float32),
                    "accelerations": np.zeros((0, 3), np.float32), "orientations": np.zeros((0, 3, 3), np.float32)}
        if N == 1:
            raise ZeroDivisionError("float division by zero")  # timegap = Tf / (N - 1.0), as in the reference
        r = self.batch_cartesian_trajectory(Xs[None], Xe[None], Tf, N, method)
        return {k: v[0] for k, v in r.items()}

    def batch_cartesian_trajectory(self, Xstart_batch, Xend_batch, Tf, N, method) -> Dict[str, np.ndarray]:
        """B pose pairs (B, 4, 4) in one launch -> (B, N, 3) / (B, N, 3, 3) float32 arrays.  New."""
        pos, vel, acc, ori = self._dispatch("trajectory.cartesian", Xstart_batch, Xend_batch, Tf, int(N), int(method))
        b = get_backend()
        return {"positions": b.asarray(pos), "velocities": b.asarray(vel), "accelerations": b.asarray(acc),
                "orientations": b.asarray(ori)}

    # ------------------------------------------------------------------ dynamics over trajectories
    def inverse_dynamics_trajectory(self, thetalist_trajectory, dthetalist_trajectory, ddthetalist_trajectory,
                                    gravity_vector=None, Ftip=None) -> np.ndarray:
        """(rows, n) float32 torques, clipped to the torque limits
        (reference planning/trajectory_dynamics.py:31-90, :308-380).  Rows are independent, so a
        flattened (B*N, n) history is a valid input.  float64 inputs are evaluated in float64 and
        then stored float32 exactly as the reference does (:354); float32 inputs run the float32 kernel."""
        if gravity_vector is None:
            gravity_vector = np.array([0.0, 0.0, -9.81])
        if Ftip is None:
            Ftip = [0, 0, 0, 0, 0, 0]
        q = np.asarray(thetalist_trajectory)
        if q.ndim != 2:
            raise ValueError(f"trajectories must be (N, n); got {q.shape}")
        if q.shape[0] == 0:
            return np.zeros(q.shape, dtype=np.float32)
        if getattr(self.dynamics, "_legacy", False):
            return get_backend().asarray(self._legacy_inverse_dynamics(q, np.asarray(dthetalist_trajectory),
                                                                       np.asarray(ddthetalist_trajectory), gravity_vector, Ftip))
        dtype = np.float64 if q.dtype == np.float64 else np.float32
        tau = self._dispatch("dynamics.inverse_trajectory", self._hip_model(), q, dthetalist_trajectory,
                             ddthetalist_trajectory, gravity_vector, Ftip, dtype=dtype)
        return get_backend().asarray(tau.astype(np.float32, copy=False))

    def batch_inverse_dynamics_trajectory(self, thetastart_batch, thetaend_batch, Tf, N, method, gravity_vector=None,
                                          Ftip=None) -> np.ndarray:
        """(B, N, n) float32 torques of the time-scaled trajectories between B start/end pairs, i.e.
        inverse_dynamics_trajectory(**batch_joint_trajectory(...)) without materialising the histories."""
        sb = np.asarray(thetastart_batch, dtype=np.float32)
        eb = np.asarray(thetaend_batch, dtype=np.float32)
        if sb.ndim != 2 or sb.shape != eb.shape:
            raise ValueError(f"start/end batches must both be (B, n); got {sb.shape} and {eb.shape}")
        if sb.shape[0] == 0:
            return np.zeros((0, int(N), sb.shape[1]), dtype=np.float32)
        tau = self._dispatch("dynamics.fused_trajectory_inverse", self._hip_model(), sb, eb, Tf, int(N), int(method),
                             gravity_vector, Ftip)
        return get_backend().asarray(tau)

    def forward_dynamics_trajectory(self, thetalist, dthetalist, taumat, g, Ftipmat, dt, intRes) -> Dict[str, np.ndarray]:
        """Semi-implicit Euler roll-out of ONE trajectory (reference planning/trajectory_dynamics.py:382-423,
        :580-708): positions / velocities / accelerations, each (N, n) float32.  The state is integrated in the
        dtype of `thetalist` (float32 stays float32, everything else float64), as the reference does."""
        th = np.asarray(thetalist)
        tm = np.asarray(taumat)
        if tm.ndim != 2:
            raise ValueError(f"taumat must be (N, n); got {tm.shape}")
        if tm.shape[0] == 0:  # the reference seeds row 0 unconditionally (:614-617)
            raise IndexError("index 0 is out of bounds for axis 0 with size 0")
        if getattr(self.dynamics, "_legacy", False):
            b = get_backend()
            return {k: b.asarray(v) for k, v in self._legacy_forward_dynamics(th, np.asarray(dthetalist), tm, g, Ftipmat, dt, intRes).items()}
        Fm = None if Ftipmat is None else np.asarray(Ftipmat)[None]
        r = self.batch_forward_dynamics_trajectory(th[None], np.asarray(dthetalist)[None], tm[None], g, Fm, dt, intRes)
        return {k: v[0] for k, v in r.items()}

    def batch_forward_dynamics_trajectory(self, theta0_batch, dtheta0_batch, taumat_batch, g, Ftipmat_batch, dt, intRes,
                                          layout: str = "batch_major", device_layout: Optional[str] = None) -> Dict[str, np.ndarray]:
        """B independent roll-outs in one launch: theta0 / dtheta0 (B, n), taumat (B, N, n), Ftipmat (B, N, 6) or
        None -> (B, N, n) float32 arrays.  New (the reference integrates one trajectory per call).

        layout="time_major": taumat / Ftipmat and the three results are (N, B, *) - the layout of the faster device kernel
        (mp_fd_trajectory_tm_*: every step touches whole cache lines), for callers that build their histories step by step.
        device_layout ("batch_major" / "time_major") picks the kernel independently of the host layout (converted on the
        device); from host arrays the call is PCIe-bound either way (profiles/r03_time_ops.jsonl), so the default is the
        host layout's own kernel."""
        if layout not in ("batch_major", "time_major"):
            raise ValueError("layout must be 'batch_major' or 'time_major'")
        th = np.asarray(theta0_batch)
        if th.ndim != 2:
            raise ValueError(f"initial states must be (B, n); got {th.shape}")
        dtype = np.float32 if th.dtype == np.float32 else np.float64
        if int(intRes) == 0:
            raise ZeroDivisionError("float division by zero")  # dt_step = dt / intRes, as in the reference (:627)
        if int(intRes) < 0:
            raise ValueError("intRes must be positive")
        if g is None:
            g = np.array([0.0, 0.0, -9.81])
        pos, vel, acc = self._dispatch("dynamics.forward_trajectory", self._hip_model(), th, dtheta0_batch, taumat_batch, g,
                                       Ftipmat_batch, dt, int(intRes), dtype=dtype, layout=layout, device_layout=device_layout)
        b = get_backend()
        return {"positions": b.asarray(pos), "velocities": b.asarray(vel), "accelerations": b.asarray(acc)}

    def _vjp_model(self, what: str):
        """The compiled model for the roll-out gradients: refused, in the analytical derivatives' words, for legacy dynamics objects and
        for models of more than MP_MAX_DOF joints."""
        if getattr(self.dynamics, "_legacy", False):
            raise NotImplementedError(f"{what}: needs Mlist_per_link - the legacy approximation has no analytical derivatives")
        model = self._hip_model()
        if model.n > _hip.MP_MAX_DOF:
            raise NotImplementedError(f"{what}: the analytical derivatives cover models of up to {_hip.MP_MAX_DOF} joints "
                                      f"(this one has {model.n})")
        return model

    def batch_forward_dynamics_trajectory_vjp(self, theta0_batch, dtheta0_batch, taumat_batch, g, Ftipmat_batch, dt, intRes,
                                              grad_positions=None, grad_velocities=None, grad_accelerations=None,
                                              layout: str = "batch_major") -> Dict[str, np.ndarray]:
        """Gradients of batch_forward_dynamics_trajectory: given the cotangents of its positions / velocities / accelerations (each
        shaped like them, None = zero), returns {"theta0": (B, n), "dtheta0": (B, n), "taumat": shaped like taumat_batch} =
        dL/d(input) of L = sum(G * rows), float64.  One reverse pass through the sub-steps (csrc/mp_rollout_vjp.h) instead of a roll-out
        per perturbed input.  The state is float64 (float32 inputs are refused); the clip's gradient is torch.clamp's; the rows' float32
        cast counts as the identity; g and Ftipmat are constants.  New (the reference differentiates its torch roll-out with autograd).
        layout="time_major": taumat / Ftipmat / the cotangents / the taumat gradient are (N, B, *)."""
        what = "batch_forward_dynamics_trajectory_vjp"
        if layout not in ("batch_major", "time_major"):
            raise ValueError("layout must be 'batch_major' or 'time_major'")
        for name, a in (("theta0_batch", theta0_batch), ("dtheta0_batch", dtheta0_batch), ("taumat_batch", taumat_batch)):
            if np.asarray(a).dtype == np.float32:
                raise TypeError(f"{what}: {name} is float32 - the roll-out gradients are computed on float64 state only")
        th = np.asarray(theta0_batch, dtype=np.float64)
        if th.ndim != 2:
            raise ValueError(f"initial states must be (B, n); got {th.shape}")
        if int(intRes) == 0:
            raise ZeroDivisionError("float division by zero")  # dt_step = dt / intRes, as the forward roll-out
        if int(intRes) < 0:
            raise ValueError("intRes must be positive")
        model = self._vjp_model(what)
        if g is None:
            g = np.array([0.0, 0.0, -9.81])
        gth, gdth, gtau = self._dispatch("dynamics.forward_trajectory_vjp", model, th, dtheta0_batch, taumat_batch, g, Ftipmat_batch, dt,
                                         int(intRes), grad_positions, grad_velocities, grad_accelerations, layout=layout)
        return {"theta0": gth, "dtheta0": gdth, "taumat": gtau}

    def forward_dynamics_trajectory_vjp(self, thetalist, dthetalist, taumat, g, Ftipmat, dt, intRes, grad_positions=None,
                                        grad_velocities=None, grad_accelerations=None) -> Dict[str, np.ndarray]:
        """Gradients of forward_dynamics_trajectory for ONE trajectory: cotangents (N, n) (None = zero) -> {"theta0": (n,),
        "dtheta0": (n,), "taumat": (N, n)}, float64; see batch_forward_dynamics_trajectory_vjp."""
        tm = np.asarray(taumat)
        if tm.ndim != 2:
            raise ValueError(f"taumat must be (N, n); got {tm.shape}")
        one = lambda a: None if a is None else np.asarray(a)[None]  # noqa: E731
        r = self.batch_forward_dynamics_trajectory_vjp(one(thetalist), one(dthetalist), tm[None], g, one(Ftipmat), dt, intRes,
                                                       one(grad_positions), one(grad_velocities), one(grad_accelerations))
        return {k: v[0] for k, v in r.items()}

    # ------------------------------------------------------------------ batched LQR / iLQR about a roll-out (csrc/mp_ilqr.h)
    def _ilqr_problem(self, what, theta0, dtheta0, taumat, x_ref, wq, wr, wf, dt, g, layout):
        """Checks the arguments of batch_lqr_gains / batch_ilqr and returns (the four primitives behind one interface, "gpu" | "cpu"):
        device-resident (_IlqrDevice) when the call is routed to the GPU, host arrays through the registered CPU launchers (_IlqrHost)
        otherwise.  The callers count the whole operation - set-up, launches, driver - as one call of that kind once it is done."""
        if layout not in ("batch_major", "time_major"):
            raise ValueError("layout must be 'batch_major' or 'time_major'")
        for name, a in (("theta0", theta0), ("dtheta0", dtheta0), ("taumat", taumat), ("x_ref", x_ref)):
            if np.asarray(a).dtype == np.float32:
                raise TypeError(f"{what}: {name} is float32 - the roll-out gradients are computed on float64 state only")
        model = self._vjp_model(what)
        n = model.n
        th = np.ascontiguousarray(theta0, dtype=np.float64)
        if th.ndim != 2 or th.shape[1] != n:
            raise ValueError(f"initial states must be (B, {n}); got {th.shape}")
        B = th.shape[0]
        dth = _hip._as_c(dtheta0, np.float64, (B, n), "dtheta0")
        tm, xr = np.asarray(taumat, dtype=np.float64), np.asarray(x_ref, dtype=np.float64)
        if layout == "time_major":
            tm, xr = np.swapaxes(tm, 0, 1), np.swapaxes(xr, 0, 1)
        if tm.ndim != 3 or tm.shape[0] != B or tm.shape[2] != n:
            raise ValueError(f"taumat must be (B, N, {n}) (or (N, B, {n}) time-major); got {np.asarray(taumat).shape}")
        N = tm.shape[1]
        if N < 2:
            raise ValueError(f"{what}: N must be >= 2 (got {N})")
        if xr.shape != (B, N, 2 * n):
            raise ValueError(f"x_ref must be (B, N, {2 * n}) (or (N, B, {2 * n}) time-major); got {np.asarray(x_ref).shape}")
        bc = lambda w, m, name: _hip._as_c(np.broadcast_to(np.asarray(w, dtype=np.float64), (m,)), np.float64, (m,), name)  # noqa: E731
        wq, wr, wf = bc(wq, 2 * n, "wq"), bc(wr, n, "wr"), bc(wf, 2 * n, "wf")
        if g is None:
            g = np.array([0.0, 0.0, -9.81])
        args = (model, th, dth, np.ascontiguousarray(tm), np.ascontiguousarray(xr), wq, wr, wf, np.asarray(g, dtype=np.float64), float(dt))
        if self._gpu_routed():
            return _IlqrDevice(_reg.get_context(), *args), "gpu"
        if not self._forced_cpu:
            _reg._refuse_silent_cpu("dynamics.ilqr_backward")
        return _IlqrHost(*args), "cpu"

    @staticmethod
    def _ilqr_layout(a, layout):
        return a if layout == "batch_major" else np.ascontiguousarray(np.swapaxes(a, 0, 1))

    def batch_lqr_gains(self, theta0, dtheta0, taumat, x_ref, wq, wr, wf, dt, g=None, reg=0.0, layout: str = "batch_major"):
        """Time-varying LQR about the roll-out of `taumat` from (theta0, dtheta0) for B trajectories at once: one float64 roll-out, one
        launch of the forward-dynamics derivatives and one Riccati backward pass (csrc/mp_ilqr.h; conventions in
        include/manipula_hip.h).  theta0 / dtheta0 (B, n), taumat (B, N, n), x_ref (B, N, 2n); wq / wf (2n), wr (n) diagonal weights
        (scalars broadcast); reg a scalar or (B,).  Returns {"K": (B, N, n, 2n), "k": (B, N, n), "expected_reduction": (B, 2) = (dV1,
        dV2), "status": (B,) int32, "positions", "velocities": (B, N, n) float64, "cost": (B,)}; rows 0 of K and k are zero.
        layout="time_major": taumat, x_ref and the row outputs are (N, B, ...)."""
        t0 = time.time()
        prob, route = self._ilqr_problem("batch_lqr_gains", theta0, dtheta0, taumat, x_ref, wq, wr, wf, dt, g, layout)
        try:
            J = prob.nominal()
            dV, status = prob.backward(np.broadcast_to(np.asarray(reg, dtype=np.float64), (prob.B,)))
            r = prob.result()
        finally:
            prob.close()
            self._count(route, t0)
        out = {"K": r["K"], "k": r["k"], "positions": r["positions"], "velocities": r["velocities"]}
        out = {key: self._ilqr_layout(v, layout) for key, v in out.items()}
        out.update({"expected_reduction": dV, "status": status, "cost": J})
        return out

    def batch_ilqr(self, theta0, dtheta0, taumat, x_ref, wq, wr, wf, dt, g=None, max_iter: int = 50, tol: float = 1e-9,
                   reg0: float = 1e-6, layout: str = "batch_major"):
        """iLQR for B problems at once from the nominal torques `taumat` (arguments as batch_lqr_gains).  The driver below is shared by
        both backends - only the four primitives (nominal roll-out, backward pass, candidate costs, accepted roll-out) dispatch - and on
        the GPU the states, derivative blocks and gains stay on the device: an iteration brings back the costs, dV and status.
        Rules: candidates alpha = 2^0 .. 2^-7, the largest with J - J_alpha >= 1e-4 (-(alpha dV1 + alpha^2 dV2)) is taken and reg <-
        max(reg / 10, 1e-9); none, or status > 0: reg <- 10 reg and alpha = 0.  A trajectory is converged, and frozen at alpha = 0 from
        then on, once an accepted step lowers J by at most tol (1 + |J|) or -dV1 <= tol (1 + |J|).  Stops when all are converged or at
        max_iter.  Returns {"taumat", "positions", "velocities": (B, N, n), "K": (B, N, n, 2n), "k": (B, N, n), "cost": (B,),
        "iterations": (B,), "converged": (B,), "cost_history": (iterations + 1, B), "alpha_history": (iterations, B)}."""
        t0 = time.time()
        prob, route = self._ilqr_problem("batch_ilqr", theta0, dtheta0, taumat, x_ref, wq, wr, wf, dt, g, layout)
        try:
            out = _ilqr_drive(prob, max_iter, tol, reg0)
            r = prob.result()
        finally:
            prob.close()
            self._count(route, t0)
        out.update({key: self._ilqr_layout(r[key], layout) for key in ("taumat", "positions", "velocities", "K", "k")})
        return out

    # ------------------------------------------------------------------ time-optimal path parameterisation (csrc/mp_toppra.h)
    def batch_time_optimal_parameterization(self, path_q, path_dq, path_ddq, velocity_limits, torque_limits=None,
                                            acceleration_limits=None, sd_start=0.0, sd_end=0.0, g=None, Ftip=None,
                                            layout: str = "batch_major") -> Dict[str, np.ndarray]:
        """The fastest timing s(t) of B geometric paths q(s) within the torque, velocity and (optional) acceleration limits, by
        reachability analysis on the grid s_i = i / (N - 1) (conventions in include/manipula_hip.h).  path_q / path_dq / path_ddq
        (B, N, n) float64: q, dq/ds, d2q/ds2 at the grid points, N >= 3; velocity_limits (n) finite and positive; torque_limits (n, 2),
        entries may be infinite, None = this planner's own (as given to the constructor, in float64); acceleration_limits (n) or None; sd_start / sd_end the path speeds at both
        ends, scalars or (B,).  Returns {"sd2", "sdd", "time": (B, N), "duration": (B,), "velocities", "accelerations", "torques":
        (B, N, n), "controllable": (B, N, 2), "status": (B,) int32}; status 0 fine, i + 1 the controllable set is empty at grid point
        i, -2 a boundary speed is not admissible, -1 a non-finite input or a grid row whose dq/ds is all zero - the results of such a
        path are NaN, other paths are untouched.  layout="time_major": the paths and every (B, N, ...) output are (N, B, ...).  One
        row-parallel dynamics launch and one sequential sweep a path; on the "hip" backend the coefficients never leave the device."""
        if layout not in ("batch_major", "time_major"):
            raise ValueError("layout must be 'batch_major' or 'time_major'")
        for name, a in (("path_q", path_q), ("path_dq", path_dq), ("path_ddq", path_ddq)):
            if np.asarray(a).dtype == np.float32:
                raise TypeError(f"batch_time_optimal_parameterization: {name} is float32 - the parameterisation is float64 only")
        model = self._vjp_model("batch_time_optimal_parameterization")
        n = model.n
        q, dq, ddq = (np.asarray(a, dtype=np.float64) for a in (path_q, path_dq, path_ddq))
        if layout == "time_major":
            q, dq, ddq = (np.swapaxes(a, 0, 1) if a.ndim == 3 else a for a in (q, dq, ddq))
        if q.ndim != 3 or q.shape[2] != n or dq.shape != q.shape or ddq.shape != q.shape:
            raise ValueError(f"path_q, path_dq and path_ddq must all be (B, N, {n}) (or (N, B, {n}) time-major); got "
                             f"{np.asarray(path_q).shape}, {np.asarray(path_dq).shape}, {np.asarray(path_ddq).shape}")
        if q.shape[1] < 3:
            raise ValueError(f"batch_time_optimal_parameterization: N must be >= 3 (got {q.shape[1]})")
        vl = np.asarray(velocity_limits, dtype=np.float64)
        if vl.shape != (n,) or not (np.isfinite(vl) & (vl > 0)).all():
            raise ValueError(f"velocity_limits must be ({n},), finite and positive")
        tl = np.asarray(self._torque_limits_f64 if torque_limits is None else torque_limits, dtype=np.float64)
        if tl.shape != (n, 2) or np.isnan(tl).any() or (tl[:, 0] > tl[:, 1]).any():
            raise ValueError(f"torque_limits must be ({n}, 2) pairs (lo <= hi, either may be infinite)")
        al = None
        if acceleration_limits is not None:
            al = np.asarray(acceleration_limits, dtype=np.float64)
            if al.shape != (n,) or not (al > 0).all():
                raise ValueError(f"acceleration_limits must be ({n},) and positive")
        out = self._dispatch("planning.time_optimal", model, np.ascontiguousarray(q), np.ascontiguousarray(dq), np.ascontiguousarray(ddq),
                             vl, tl, al, sd_start, sd_end, g, Ftip)
        if layout == "time_major":
            out = {k: (np.ascontiguousarray(np.swapaxes(v, 0, 1)) if v.ndim >= 2 else v) for k, v in out.items()}
        return out

    def batch_time_optimal_joint_trajectory(self, thetastart_batch, thetaend_batch, N, velocity_limits, torque_limits=None,
                                            acceleration_limits=None, sd_start=0.0, sd_end=0.0, g=None, Ftip=None) -> Dict[str, np.ndarray]:
        """batch_time_optimal_parameterization of the straight joint-space lines q(s) = start + s (end - start) of B (start, end)
        pairs (B, n), on N grid points: dq/ds = end - start, d2q/ds2 = 0.  Adds "positions" (B, N, n) to the result."""
        sb, eb = np.asarray(thetastart_batch, dtype=np.float64), np.asarray(thetaend_batch, dtype=np.float64)
        if sb.ndim != 2 or sb.shape != eb.shape:
            raise ValueError(f"start/end batches must both be (B, n); got {sb.shape} and {eb.shape}")
        N = int(N)
        if N < 3:
            raise ValueError(f"batch_time_optimal_joint_trajectory: N must be >= 3 (got {N})")
        s = np.arange(N, dtype=np.float64) / (N - 1)
        d = eb - sb
        q = sb[:, None, :] + s[None, :, None] * d[:, None, :]
        dq = np.broadcast_to(d[:, None, :], q.shape)
        out = self.batch_time_optimal_parameterization(q, dq, np.zeros_like(q), velocity_limits, torque_limits, acceleration_limits,
                                                       sd_start, sd_end, g, Ftip)
        out["positions"] = q
        return out

    def time_optimal_joint_trajectory(self, thetastart, thetaend, N, velocity_limits, torque_limits=None, acceleration_limits=None,
                                      sd_start=0.0, sd_end=0.0, g=None, Ftip=None) -> Dict[str, np.ndarray]:
        """batch_time_optimal_joint_trajectory for one (start, end) pair: every result without its leading batch axis."""
        s, e = np.asarray(thetastart, dtype=np.float64), np.asarray(thetaend, dtype=np.float64)
        if s.ndim != 1 or s.shape != e.shape:
            raise ValueError(f"thetastart and thetaend must both be (n,); got {s.shape} and {e.shape}")
        r = self.batch_time_optimal_joint_trajectory(s[None], e[None], N, velocity_limits, torque_limits, acceleration_limits,
                                                     float(sd_start), float(sd_end), g, Ftip)
        return {k: v[0] for k, v in r.items()}

    def batch_trajectory_clearance(self, positions, collision_model, margin: float = 0.0) -> Dict[str, np.ndarray]:
        """Clearance of B trajectories (B, N, n) under a collision.SphereCollisionModel (whose world is the obstacle table last given
        to its set_world together with the point cloud last given to its set_cloud, if any - here and in every function of this
        planner that takes a collision model): {"world_clearance", "self_clearance": (B,) the smallest signed distance along each trajectory (+inf where the
        model has no obstacle / no pair), "world_step", "self_step": (B,) the first step at which it occurs, "first_violation": (B,)
        the first step whose world or self clearance is below `margin`, -1 if there is none}.  A trajectory with a non-finite row
        reports NaN clearances.  One row-parallel launch; the reduction over the steps is done on the host."""
        pos = np.asarray(positions, dtype=np.float64)
        n = collision_model.n
        if pos.ndim != 3 or pos.shape[2] != n:
            raise ValueError(f"positions must be (B, N, {n}); got {pos.shape}")
        B, N = pos.shape[:2]
        want = ("dist_world", "dist_self")
        r = self._dispatch("planning.collision_spheres", collision_model, np.ascontiguousarray(pos.reshape(B * N, n)), 1.0, 1.0, want)
        dw, ds = r["dist_world"].reshape(B, N), r["dist_self"].reshape(B, N)
        out = {}
        for key, d in (("world", dw), ("self", ds)):
            bad = np.isnan(d).any(axis=1)
            step = np.argmin(np.where(np.isnan(d), np.inf, d), axis=1)
            out[f"{key}_clearance"] = np.where(bad, np.nan, d[np.arange(B), step])
            out[f"{key}_step"] = step.astype(np.int64)
        below = (dw < margin) | (ds < margin)
        out["first_violation"] = np.where(below.any(axis=1), np.argmax(below, axis=1), -1).astype(np.int64)
        return out

    def batch_validate_path(self, waypoints, collision_model, margin: float = 0.0, tol: float = 1e-3,
                            max_steps: int = 512) -> Dict[str, np.ndarray]:
        """Continuous validation of B piecewise-linear joint-space paths (B, W, n) under a collision.SphereCollisionModel: every
        segment waypoint[i] -> waypoint[i + 1] is checked over its whole length by conservative advancement (SphereCollisionModel.
        check_edges), all B (W - 1) segments in one launch.  {"free": (B,) every segment proven free (an UNDECIDED or INVALID segment
        counts as not free), "first_blocked_segment": (B,) the first segment that is not free, -1 if none, "blocked_at": (B,) that
        segment's index + its t (NaN for a free path or an invalid segment), "segment_status": (B, W - 1), "clearance": (B,) the
        smallest clearance over the configurations evaluated on the path (NaN with an invalid segment)}.
        The collision model's world is its obstacle table and its point cloud (SphereCollisionModel.set_cloud), if one is set."""
        wp = np.asarray(waypoints, dtype=np.float64)
        n = collision_model.n
        if wp.ndim != 3 or wp.shape[2] != n or wp.shape[1] < 2:
            raise ValueError(f"waypoints must be (B, W >= 2, {n}); got {wp.shape}")
        B, W = wp.shape[:2]
        qa = np.ascontiguousarray(wp[:, :-1].reshape(B * (W - 1), n))
        qb = np.ascontiguousarray(wp[:, 1:].reshape(B * (W - 1), n))
        r = self._dispatch("planning.collision_edges", collision_model, qa, qb, margin, tol, max_steps, ("status", "t", "clearance"))
        status, t, clear = (r[k].reshape(B, W - 1) for k in ("status", "t", "clearance"))
        stopped = status != 0
        free = ~stopped.any(axis=1)
        first = np.where(free, -1, np.argmax(stopped, axis=1)).astype(np.int64)
        at = t[np.arange(B), np.maximum(first, 0)]
        bad = np.isnan(clear)
        return {"free": free, "first_blocked_segment": first, "blocked_at": np.where(free, np.nan, first + at),
                "segment_status": status,
                "clearance": np.where(bad.any(axis=1), np.nan, np.where(bad, np.inf, clear).min(axis=1))}

    def batch_plan_path(self, start, goal, collision_model, margin: float = 0.0, tol: float = 1e-3, *, step: float = 1.0,
                        min_advance=None, max_iters: int = 200, max_nodes: int = 256, max_waypoints: int = 64, max_steps: int = 64,
                        seed: int = 0, finite_limit: float = 2 * np.pi) -> Dict[str, np.ndarray]:
        """Collision-free piecewise-linear joint-space paths for B (start, goal) pairs (B, n) under a collision.SphereCollisionModel,
        by bidirectional RRT-Connect (SphereCollisionModel.plan_paths), all B problems in one launch.  The sampling box is this
        planner's joint limits, an open or non-finite limit clipped to +-`finite_limit`.  {"status", "count", "waypoints" (B,
        max_waypoints, n), "iterations", "nodes", "evaluations"}: "waypoints" can go straight into `batch_validate_path`.
        The collision model's world is its obstacle table and its point cloud (SphereCollisionModel.set_cloud), if one is set."""
        sb, gb = np.asarray(start, dtype=np.float64), np.asarray(goal, dtype=np.float64)
        n = collision_model.n
        if sb.ndim != 2 or sb.shape != gb.shape or sb.shape[1] != n:
            raise ValueError(f"start and goal must both be (B, {n}); got {sb.shape} and {gb.shape}")
        lo, hi = self._planning_box(finite_limit)
        return self._dispatch("planning.rrt_connect", collision_model, np.ascontiguousarray(sb), np.ascontiguousarray(gb), lo, hi, margin,
                              tol, step=step, min_advance=min_advance, max_iters=max_iters, max_nodes=max_nodes,
                              max_waypoints=max_waypoints, max_steps=max_steps, seed=seed)

    def batch_shortcut_path(self, waypoints, count, collision_model, margin: float = 0.0, tol: float = 1e-3, *, max_iters: int = 100,
                            min_gain: float = 0.0, max_waypoints=None, max_steps: int = 64, seed: int = 0) -> Dict[str, np.ndarray]:
        """Shortens B piecewise-linear joint-space paths (B, W, n) with `count` (B,) real waypoints each - `batch_plan_path`'s
        "waypoints" and "count" - by randomised shortcutting under a collision.SphereCollisionModel (SphereCollisionModel.
        shortcut_paths), all B paths in one launch.  {"status", "count", "waypoints" (B, max_waypoints or W, n), "length_in",
        "length_out", "iterations", "accepted", "skipped_full", "evaluations"}: rows that were not solved come back skipped, and
        "waypoints" can go straight into `batch_validate_path`.  The input paths themselves are not checked.
        The collision model's world is its obstacle table and its point cloud (SphereCollisionModel.set_cloud), if one is set."""
        wp = np.asarray(waypoints, dtype=np.float64)
        cnt = np.asarray(count)
        n = collision_model.n
        if wp.ndim != 3 or wp.shape[2] != n or cnt.shape != (wp.shape[0],):
            raise ValueError(f"waypoints must be (B, W, {n}) and count (B,); got {wp.shape} and {cnt.shape}")
        return self._dispatch("planning.shortcut_paths", collision_model, np.ascontiguousarray(wp),
                              cnt, margin, tol, max_iters=max_iters, min_gain=min_gain,
                              max_waypoints=max_waypoints, max_steps=max_steps, seed=seed)

    def batch_blend_path(self, waypoints, count, collision_model, N: int, margin: float = 0.0, tol: float = 1e-3, *, blend: float = 0.5,
                         max_halvings: int = 6, max_steps: int = 64) -> Dict[str, np.ndarray]:
        """Turns B piecewise-linear joint-space paths (B, W, n) with `count` (B,) real waypoints each - `batch_plan_path`'s or
        `batch_shortcut_path`'s "waypoints" and "count" - into twice-differentiable curves under a collision.SphereCollisionModel
        (SphereCollisionModel.blend_paths) and samples them on N grid points, all B paths in one call.  {"status", "corner", "count",
        "points", "cut", "knot", "length", "halvings", "evaluations", "clearance", "q", "dq", "ddq" (B, N, n)}: rows that were not
        solved come back skipped, and "q", "dq", "ddq" go straight into `batch_time_optimal_parameterization`.  The input paths
        themselves are not checked.
        The collision model's world is its obstacle table and its point cloud (SphereCollisionModel.set_cloud), if one is set."""
        wp = np.asarray(waypoints, dtype=np.float64)
        cnt = np.asarray(count)
        n = collision_model.n
        if wp.ndim != 3 or wp.shape[2] != n or cnt.shape != (wp.shape[0],):
            raise ValueError(f"waypoints must be (B, W, {n}) and count (B,); got {wp.shape} and {cnt.shape}")
        return self._dispatch("planning.blend_paths", collision_model, np.ascontiguousarray(wp), cnt, N, margin, tol, blend=blend,
                              max_halvings=max_halvings, max_steps=max_steps)

    def batch_time_optimal_path(self, waypoints, count, collision_model, N: int, velocity_limits, torque_limits=None,
                                acceleration_limits=None, margin: float = 0.0, tol: float = 1e-3, *, blend: float = 0.5,
                                max_halvings: int = 6, max_steps: int = 64, sd_start=0.0, sd_end=0.0, g=None,
                                Ftip=None) -> Dict[str, Dict[str, np.ndarray]]:
        """`batch_blend_path`, then `batch_time_optimal_parameterization` of the curves it made: {"blend": its dict, "timing": the
        parameterisation's dict over all B rows}.  Only the rows whose blend status is 0 (done) or 1 (straight) are timed; every
        other row - skipped, a point, blocked, a reversal, invalid - keeps its blend status and comes back with NaN in every real
        timing output and -1 in the timing status.  sd_start / sd_end: scalars or (B,)."""
        bl = self.batch_blend_path(waypoints, count, collision_model, N, margin, tol, blend=blend, max_halvings=max_halvings,
                                   max_steps=max_steps)
        B = bl["status"].shape[0]
        rows = np.flatnonzero((bl["status"] == 0) | (bl["status"] == 1))
        pick = lambda v: v if np.ndim(v) == 0 else np.asarray(v, dtype=np.float64)[rows]  # noqa: E731
        n, G = bl["q"].shape[2], bl["q"].shape[1]
        shapes = {"sd2": (G,), "sdd": (G,), "time": (G,), "duration": (), "velocities": (G, n), "accelerations": (G, n),
                  "torques": (G, n), "controllable": (G, 2)}
        timing = {k: np.full((B,) + shape, np.nan) for k, shape in shapes.items()}
        timing["status"] = np.full(B, -1, dtype=np.int32)
        if len(rows):
            part = self.batch_time_optimal_parameterization(bl["q"][rows], bl["dq"][rows], bl["ddq"][rows], velocity_limits,
                                                            torque_limits, acceleration_limits, pick(sd_start), pick(sd_end), g, Ftip)
            for k, v in part.items():
                timing[k][rows] = v
        return {"blend": bl, "timing": timing}

    def batch_sample_time_optimal(self, timing, dt: float, *, path=None, curve=None, max_samples: Optional[int] = None,
                                  velocity_limits=None, g=None, Ftip=None) -> Dict[str, np.ndarray]:
        """Turns B timed paths into B trajectories at the fixed period dt: row k is the time k dt (conventions in
        include/manipula_hip.h, mp_trajectory_sample_*).  `timing`: the dict of `batch_time_optimal_parameterization` ("time", "sd2",
        "duration" are read).  The geometry is either `path` = (q, dq, ddq), the (B, N, n) arrays that were timed - the samples lie
        on their quintic Hermite interpolant - or `curve` = the dict of `batch_blend_path` - the samples lie on the blended curve
        itself.  max_samples: the rows M a path gets; None takes the largest "needed" over the paths with a finite duration (1 if
        there is none), so that no path is truncated.  Returns {"status" (0 ok, 1 truncated: more than M rows were needed, 2 stops:
        the timing has an interior stop, 3 untimed: no timing or no curve, -1 invalid), "count", "needed" (B,) int32, "s", "sd",
        "sdd" (B, M), "positions", "velocities", "accelerations", "torques" (B, M, n), "peak_torque_ratio" (B,)} and, with
        `velocity_limits` (n), "peak_velocity_ratio" (B,).  Rows from "count" on repeat the path's end point at rest; a path without
        samples is NaN.  "torques" is the inverse dynamics at every sample (g, Ftip as elsewhere), not an interpolation of the grid's
        torques: "peak_torque_ratio" - the largest |torque_j| / limit_j over a path's samples against this planner's torque limits,
        an infinite limit counting 0, NaN for a path without samples - above 1 says that the grid was too coarse for the path (raise
        N).  "peak_velocity_ratio" is the same for |velocity_j| / velocity_limits_j."""
        model = self._vjp_model("batch_sample_time_optimal")
        t, x = np.asarray(timing["time"], dtype=np.float64), np.asarray(timing["sd2"], dtype=np.float64)
        if t.ndim != 2 or x.shape != t.shape:
            raise ValueError(f"timing['time'] and timing['sd2'] must both be (B, N); got {t.shape} and {x.shape}")
        if (path is None) == (curve is None):
            raise ValueError("batch_sample_time_optimal: give exactly one of path=(q, dq, ddq) and curve=<the dict of batch_blend_path>")
        if not (np.isfinite(dt) and dt > 0):
            raise ValueError("batch_sample_time_optimal: dt must be positive and finite")
        if max_samples is None:
            need = _hip.sample_rows_needed(np.asarray(timing["duration"], dtype=np.float64), dt)
            max_samples = max(int(need.max()) if need.size else 0, 1)
        if curve is not None:
            curve = {k: curve[k] for k in _hip.SAMPLE_CURVE_TABLES}
        out = self._dispatch("planning.time_optimal_samples", model, np.ascontiguousarray(t), np.ascontiguousarray(x), float(dt),
                             int(max_samples), path=path, curve=curve, g=g, Ftip=Ftip)
        tl = self._torque_limits_f64
        out["peak_torque_ratio"] = self._peak_ratio(out["torques"], out["count"], tl[:, 1], tl[:, 0])
        if velocity_limits is not None:
            out["peak_velocity_ratio"] = self._peak_ratio(out["velocities"], out["count"], np.asarray(velocity_limits, dtype=np.float64))
        return out

    @staticmethod
    def _peak_ratio(values, count, hi, lo=None) -> np.ndarray:
        """max over a path's first `count` rows and the joints of value_j / hi_j (value_j >= 0) or value_j / lo_j (value_j < 0; lo =
        -hi by default), 0 for an infinite limit; NaN for a path without rows."""
        B, M, n = values.shape
        hi = np.asarray(hi, dtype=np.float64)
        lim = np.where(values >= 0, hi, -hi if lo is None else np.asarray(lo, dtype=np.float64))
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(np.isinf(lim), 0.0, values / lim)
        live = np.arange(M)[None, :] < np.asarray(count)[:, None]
        peak = np.where(live[:, :, None], ratio, -np.inf).reshape(B, -1).max(axis=1)
        return np.where(np.asarray(count) > 0, peak, np.nan)

    def batch_time_optimal_trajectory(self, waypoints, count, collision_model, N: int, dt: float, velocity_limits, torque_limits=None,
                                      acceleration_limits=None, margin: float = 0.0, tol: float = 1e-3, *, blend: float = 0.5,
                                      max_halvings: int = 6, max_steps: int = 64, max_samples: Optional[int] = None, g=None,
                                      Ftip=None) -> Dict[str, Dict[str, np.ndarray]]:
        """`batch_time_optimal_path` (blend, then time from rest to rest), then `batch_sample_time_optimal` of its result on the
        blended curves at the period dt: {"blend", "timing", "samples"}, the three dicts over all B rows.  A row without a curve or
        without a timing keeps its earlier status and comes back untimed (3) with NaN samples."""
        both = self.batch_time_optimal_path(waypoints, count, collision_model, N, velocity_limits, torque_limits, acceleration_limits,
                                            margin, tol, blend=blend, max_halvings=max_halvings, max_steps=max_steps, g=g, Ftip=Ftip)
        both["samples"] = self.batch_sample_time_optimal(both["timing"], dt, curve=both["blend"], max_samples=max_samples,
                                                         velocity_limits=velocity_limits, g=g, Ftip=Ftip)
        return both

    def batch_cartesian_path(self, q_start, T_goal, collision_model, N: int, margin: float = 0.0, tol: float = 1e-3, *,
                             task: str = "full", eomg: float = 1e-6, ev: float = 1e-6, damping: float = 0.01, max_iters: int = 20,
                             max_joint_step: float = 0.5, max_steps: int = 64, finite_limit: float = 2 * np.pi) -> Dict[str, np.ndarray]:
        """Straight tool lines from B start configurations q_start (B, n) to B poses T_goal (B, 4, 4) under a
        collision.SphereCollisionModel (SphereCollisionModel.cartesian_paths), all B problems in one call.  The box is this planner's
        joint limits, clipped as `batch_plan_path` clips its sampling box.  {"status" (0 done, 1 stalled, 2 singular, 3 limit, 4
        jump, 5 blocked, 6 undecided, -1 invalid), "reached", "span", "t", "clearance", "deviation_pos", "deviation_rot",
        "pose_error", "iterations", "evaluations", "q", "dq", "ddq" (B, N, n), "span_status", "span_clearance" (B, N - 1)}: "q",
        "dq", "ddq" of a done row go straight into `batch_time_optimal_parameterization` and `batch_sample_time_optimal(path=...)`,
        whose samples lie on the curve that was proven free.
        The collision model's world is its obstacle table and its point cloud (SphereCollisionModel.set_cloud), if one is set."""
        q0, Tg = np.asarray(q_start, dtype=np.float64), np.asarray(T_goal, dtype=np.float64)
        n = collision_model.n
        if q0.ndim != 2 or q0.shape[1] != n or Tg.shape != (q0.shape[0], 4, 4):
            raise ValueError(f"q_start must be (B, {n}) and T_goal (B, 4, 4); got {q0.shape} and {Tg.shape}")
        lo, hi = self._planning_box(finite_limit)
        return self._dispatch("planning.cartesian_paths", collision_model, np.ascontiguousarray(q0),
                              np.ascontiguousarray(Tg.reshape(-1, 16)), lo, hi, N, margin, tol, task=task, eomg=eomg, ev=ev,
                              damping=damping, max_iters=max_iters, max_joint_step=max_joint_step, max_steps=max_steps)

    def batch_time_optimal_cartesian_path(self, q_start, T_goal, collision_model, N: int, velocity_limits, torque_limits=None,
                                          acceleration_limits=None, margin: float = 0.0, tol: float = 1e-3, *, task: str = "full",
                                          eomg: float = 1e-6, ev: float = 1e-6, damping: float = 0.01, max_iters: int = 20,
                                          max_joint_step: float = 0.5, max_steps: int = 64, sd_start=0.0, sd_end=0.0, g=None, Ftip=None,
                                          finite_limit: float = 2 * np.pi) -> Dict[str, Dict[str, np.ndarray]]:
        """`batch_cartesian_path`, then `batch_time_optimal_parameterization` of the lines it made: {"line": its dict, "timing": the
        parameterisation's dict over all B rows}.  Only the rows whose line status is 0 (done) are timed; every other row keeps its
        line status and comes back with NaN in every real timing output and -1 in the timing status, as `batch_time_optimal_path`
        returns the rows without a curve.  sd_start / sd_end: scalars or (B,).  N >= 3 (the parameterisation's grid)."""
        ln = self.batch_cartesian_path(q_start, T_goal, collision_model, N, margin, tol, task=task, eomg=eomg, ev=ev, damping=damping,
                                       max_iters=max_iters, max_joint_step=max_joint_step, max_steps=max_steps,
                                       finite_limit=finite_limit)
        B = ln["status"].shape[0]
        rows = np.flatnonzero(ln["status"] == 0)
        pick = lambda v: v if np.ndim(v) == 0 else np.asarray(v, dtype=np.float64)[rows]  # noqa: E731
        n, G = ln["q"].shape[2], ln["q"].shape[1]
        shapes = {"sd2": (G,), "sdd": (G,), "time": (G,), "duration": (), "velocities": (G, n), "accelerations": (G, n),
                  "torques": (G, n), "controllable": (G, 2)}
        timing = {k: np.full((B,) + shape, np.nan) for k, shape in shapes.items()}
        timing["status"] = np.full(B, -1, dtype=np.int32)
        if len(rows):
            part = self.batch_time_optimal_parameterization(ln["q"][rows], ln["dq"][rows], ln["ddq"][rows], velocity_limits,
                                                            torque_limits, acceleration_limits, pick(sd_start), pick(sd_end), g, Ftip)
            for k, v in part.items():
                timing[k][rows] = v
        return {"line": ln, "timing": timing}

    def batch_time_optimal_cartesian_trajectory(self, q_start, T_goal, collision_model, N: int, dt: float, velocity_limits,
                                                torque_limits=None, acceleration_limits=None, margin: float = 0.0, tol: float = 1e-3, *,
                                                task: str = "full", eomg: float = 1e-6, ev: float = 1e-6, damping: float = 0.01,
                                                max_iters: int = 20, max_joint_step: float = 0.5, max_steps: int = 64,
                                                max_samples: Optional[int] = None, g=None, Ftip=None,
                                                finite_limit: float = 2 * np.pi) -> Dict[str, Dict[str, np.ndarray]]:
        """`batch_time_optimal_cartesian_path` (line, then time from rest to rest), then `batch_sample_time_optimal` of its result at
        the period dt on the grid rows themselves (path=(q, dq, ddq)): {"line", "timing", "samples"}, the three dicts over all B
        rows.  The samples lie on the quintic Hermite interpolant whose spans the line proved free.  A row that is not done keeps
        its line status and comes back untimed (3) with NaN samples."""
        both = self.batch_time_optimal_cartesian_path(q_start, T_goal, collision_model, N, velocity_limits, torque_limits,
                                                      acceleration_limits, margin, tol, task=task, eomg=eomg, ev=ev, damping=damping,
                                                      max_iters=max_iters, max_joint_step=max_joint_step, max_steps=max_steps, g=g,
                                                      Ftip=Ftip, finite_limit=finite_limit)
        ln = both["line"]
        # (a row that is not done has NaN timing, which the sampler screens - untimed - before it looks at the grid rows)
        both["samples"] = self.batch_sample_time_optimal(both["timing"], dt, path=(ln["q"], ln["dq"], ln["ddq"]), max_samples=max_samples,
                                                         velocity_limits=velocity_limits, g=g, Ftip=Ftip)
        return both

    def _planning_box(self, finite_limit: float):
        """This planner's joint limits as a finite box: an open or non-finite limit clipped to +-`finite_limit` (batch_plan_path's rule)."""
        lim = np.nan_to_num(np.asarray(self.joint_limits, dtype=np.float64), nan=0.0, posinf=finite_limit, neginf=-finite_limit)
        return np.clip(lim[:, 0], -finite_limit, finite_limit), np.clip(lim[:, 1], -finite_limit, finite_limit)

    def batch_goal_configurations(self, T_goal, q_seed, collision_model, margin: float = 0.0, tol: float = 1e-3, *, eomg: float = 1e-6,
                                  ev: float = 1e-6, damping: float = 0.02, step_cap: float = 0.5, max_iters: int = 50,
                                  max_attempts: int = 8, seed: int = 0, finite_limit: float = 2 * np.pi) -> Dict[str, np.ndarray]:
        """Collision-free joint configurations for B end-effector poses T_goal (B, 4, 4), seeded by q_seed (B, n), under a
        collision.SphereCollisionModel (SphereCollisionModel.goal_configurations), all B problems in one launch.  The box is this
        planner's joint limits, clipped as `batch_plan_path` clips its sampling box.  {"status" (0 found, 1 in collision, 2
        unreached, -1 invalid), "q" (B, n), "attempts", "iterations", "converged", "pose_error" (B, 2), "clearance", "witness"
        (B, 3)}: "q" can go straight into `batch_plan_path` as the goal.
        The collision model's world is its obstacle table and its point cloud (SphereCollisionModel.set_cloud), if one is set."""
        Tg, q0 = np.asarray(T_goal, dtype=np.float64), np.asarray(q_seed, dtype=np.float64)
        n = collision_model.n
        if q0.ndim != 2 or q0.shape[1] != n or Tg.shape != (q0.shape[0], 4, 4):
            raise ValueError(f"T_goal must be (B, 4, 4) and q_seed (B, {n}); got {Tg.shape} and {q0.shape}")
        lo, hi = self._planning_box(finite_limit)
        return self._dispatch("planning.goal_configurations", collision_model, np.ascontiguousarray(Tg.reshape(-1, 16)),
                              np.ascontiguousarray(q0), lo, hi, margin, tol, eomg=eomg, ev=ev, damping=damping, step_cap=step_cap,
                              max_iters=max_iters, max_attempts=max_attempts, seed=seed)

    def batch_plan_path_to_pose(self, start, T_goal, collision_model, margin: float = 0.0, tol: float = 1e-3, *, eomg: float = 1e-6,
                                ev: float = 1e-6, damping: float = 0.02, step_cap: float = 0.5, goal_max_iters: int = 50,
                                max_attempts: int = 8, step: float = 1.0, min_advance=None, max_iters: int = 200, max_nodes: int = 256,
                                max_waypoints: int = 64, max_steps: int = 64, seed: int = 0,
                                finite_limit: float = 2 * np.pi) -> Dict[str, np.ndarray]:
        """Collision-free paths from B start configurations (B, n) to B end-effector poses T_goal (B, 4, 4): `batch_goal_configurations`
        seeded by `start`, then `batch_plan_path` to its "q", both with this margin, tol, seed and `finite_limit`.  Returns
        `batch_plan_path`'s dict and "goal_status", "q_goal", "goal_attempts".  No masking between the two: under one margin and tol
        a found goal is never goal-blocked, a goal in collision comes back goal-blocked, and an unreached or invalid one (NaN) comes
        back invalid."""
        goal = self.batch_goal_configurations(T_goal, start, collision_model, margin, tol, eomg=eomg, ev=ev, damping=damping,
                                              step_cap=step_cap, max_iters=goal_max_iters, max_attempts=max_attempts, seed=seed,
                                              finite_limit=finite_limit)
        out = dict(self.batch_plan_path(start, goal["q"], collision_model, margin, tol, step=step, min_advance=min_advance,
                                        max_iters=max_iters, max_nodes=max_nodes, max_waypoints=max_waypoints, max_steps=max_steps,
                                        seed=seed, finite_limit=finite_limit))
        out["goal_status"], out["q_goal"], out["goal_attempts"] = goal["status"], goal["q"], goal["attempts"]
        return out

    # ------------------------------------------------------------------ legacy dynamics objects (Mlist_per_link=None)
    # The reference's approximation for such objects is not rigid-body dynamics (dynamics/mass_matrix.py:101-132), so there
    # is no compiled model and no kernel for it: the planner walks the rows on the host exactly as the reference's CPU
    # paths do (planning/trajectory_dynamics.py:308-380, :580-708), under every backend.
    def _legacy_inverse_dynamics(self, q, qd, qdd, g, Ftip) -> np.ndarray:
        t0 = time.time()
        rows = []
        with warnings.catch_warnings():   # one warning for the call instead of one per row and term
            warnings.simplefilter("ignore")
            for i in range(q.shape[0]):
                try:
                    rows.append(np.asarray(self.dynamics.inverse_dynamics(q[i], qd[i], qdd[i], g, Ftip), dtype=np.float32))
                except Exception as exc:  # the reference's per-row semantics: a row that raises becomes zeros (:345-358)
                    logger.warning("Error in inverse dynamics at point %d: %s", i, exc)
                    rows.append(np.zeros(q.shape[1], dtype=np.float32))
        warnings.warn("inverse_dynamics_trajectory on a ManipulatorDynamics without Mlist_per_link \u2014 using the reference's "
                      "legacy approximation on the host (incorrect for non-trivial robots).", stacklevel=3)
        tau = np.clip(np.stack(rows), self.torque_limits[:, 0], self.torque_limits[:, 1])
        self._count("cpu", t0)
        return tau

    def _legacy_forward_dynamics(self, theta0, dtheta0, taumat, g, Ftipmat, dt, intRes) -> Dict[str, np.ndarray]:
        t0 = time.time()
        N, n = taumat.shape[0], theta0.shape[0]
        th, dth = np.array(theta0), np.array(dtheta0)       # the state keeps the caller's dtype (:619-624)
        lo, hi = self.joint_limits[:, 0], self.joint_limits[:, 1]
        P, V, A = [th.astype(np.float32)], [dth.astype(np.float32)], [np.zeros(n, np.float32)]
        if int(intRes) == 0:
            raise ZeroDivisionError("float division by zero")
        h = dt / intRes
        Fm = np.zeros((N, 6)) if Ftipmat is None else np.asarray(Ftipmat)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for i in range(1, N):
                acc = np.zeros(n, np.float32)
                for _ in range(int(intRes)):
                    try:
                        dd = self.dynamics.forward_dynamics(th, dth, taumat[i], g, Fm[i])
                    except Exception as exc:  # only the dynamics call is tolerated (:640-650)
                        logger.warning("Error in forward dynamics at step %d: %s", i, exc)
                        acc = np.zeros(n)
                        continue
                    dth = (dth + dd * h).astype(dth.dtype)
                    th = np.clip((th + dth * h).astype(th.dtype), lo, hi)
                    acc = dd
                P.append(th.astype(np.float32)); V.append(dth.astype(np.float32)); A.append(np.asarray(acc, dtype=np.float32))
        warnings.warn("forward_dynamics_trajectory on a ManipulatorDynamics without Mlist_per_link \u2014 using the reference's "
                      "legacy approximation on the host (incorrect for non-trivial robots).", stacklevel=3)
        self._count("cpu", t0)
        return {"positions": np.stack(P), "velocities": np.stack(V), "accelerations": np.stack(A)}

    # ------------------------------------------------------------------ helpers kept from the reference
    def plan_trajectory(self, start_position, target_position, obstacle_points):
        """Six joint-space waypoints on the straight line start -> target; with obstacles (points in joint space) and a
        potential field each waypoint is pushed down the field's gradient, 0.01 per step, until the collision checker reports it
        free (at once, with the mesh-less checker) or ten steps have passed (reference planning/collision_host.py:90-152).
        Host arithmetic throughout, like the reference's.  Returns a list of joint lists."""
        start = np.asarray(start_position, dtype=np.float64)
        target = np.asarray(target_position, dtype=np.float64)
        logger.info("Planning trajectory from %d to %d DOF", len(start), len(target))
        num_waypoints = 5
        out = []
        for i in range(num_waypoints + 1):
            alpha = i / num_waypoints
            waypoint = (1 - alpha) * start + alpha * target
            if obstacle_points and self.potential_field:
                obstacles = [np.asarray(o, dtype=np.float64) for o in obstacle_points]
                for _ in range(10):
                    waypoint = waypoint - 0.01 * self.potential_field.compute_gradient(waypoint, target, obstacles)
                    if self.collision_checker and not self.collision_checker.check_collision(waypoint):
                        break
            out.append(waypoint.tolist())
        logger.info("Planned trajectory with %d waypoints", len(out))
        return out

    def calculate_derivatives(self, positions, dt) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """First differences (reference planning/trajectory_dynamics.py:710-735)."""
        p = np.asarray(positions)
        v = (p[1:] - p[:-1]) / dt
        a = (v[1:] - v[:-1]) / dt
        j = (a[1:] - a[:-1]) / dt
        return v, a, j

    # ---- the planner's own timing helpers (reference planning/trajectory_planning.py:526-658, :660-830), without the console tables
    def benchmark_all_kernels(self, N: int = 5000, num_joints: int = 6, num_runs: int = 5) -> Dict[str, Dict[str, object]]:
        """Times `joint_trajectory` under each of the reference's five trajectory-kernel names - on gfx950 they are one kernel, the
        names stay valid registry entries - and returns {name: mean / std / min / max / all_times / success_rate / trajectory_shape};
        {} when the GPU is not routed to (as the reference returns without CUDA)."""
        if not self._gpu_routed():
            logger.warning("GPU not available for benchmarking")
            return {}
        start = np.random.uniform(-1, 1, num_joints).astype(np.float32)
        end = np.random.uniform(-1, 1, num_joints).astype(np.float32)
        results: Dict[str, Dict[str, object]] = {}
        for kernel_type in ("standard", "vectorized", "memory_optimized", "warp_optimized", "cache_friendly"):
            self.reset_performance_stats()
            times, shape = [], None
            for _ in range(num_runs):
                t0 = time.time()
                try:
                    shape = self.joint_trajectory(start, end, 2.0, N, 5, kernel_type=kernel_type, enable_monitoring=False)["positions"].shape
                    times.append(time.time() - t0)
                except Exception as exc:
                    logger.warning("Kernel %s failed: %s", kernel_type, exc)
                    times.append(float("inf"))
            if times and min(times) < float("inf"):
                good = [t for t in times if t < float("inf")]
                results[kernel_type] = {"mean_time": float(np.mean(good)), "std_time": float(np.std(good)), "min_time": float(np.min(good)),
                                        "max_time": float(np.max(good)), "all_times": times, "success_rate": len(good) / len(times),
                                        "trajectory_shape": shape}
        return results

    def benchmark_performance(self, test_cases=None, include_cpu_comparison: bool = True) -> Dict[str, Dict[str, object]]:
        """Times `joint_trajectory` on a list of {"N", "joints", "name"} cases (three runs each; default: four sizes at this
        robot's joint count) and, when the GPU is routed to and asked for, the CPU launcher of the same call for a speed-up."""
        n = len(self.joint_limits)
        if test_cases is None:
            test_cases = [{"N": 100, "joints": n, "name": "Small"}, {"N": 1000, "joints": n, "name": "Medium"},
                          {"N": 5000, "joints": n, "name": "Large"}, {"N": 10000, "joints": n, "name": "Very Large"}]
        results: Dict[str, Dict[str, object]] = {}
        for case in test_cases:
            N, joints, name = case["N"], case["joints"], case["name"]
            start = np.random.uniform(-1, 1, joints).astype(np.float32)
            end = np.random.uniform(-1, 1, joints).astype(np.float32)
            self.reset_performance_stats()
            times = []
            for _ in range(3):
                t0 = time.time()
                traj = self.joint_trajectory(start, end, 2.0, N, 5)
                times.append(time.time() - t0)
            stats = self.get_performance_stats()
            mean = float(np.mean(times))
            results[name] = {"mean_time": mean, "std_time": float(np.std(times)), "min_time": min(times), "max_time": max(times), "N": N,
                             "joints": joints, "stats": stats, "used_gpu": stats["gpu_calls"] > 0,
                             "trajectory_shape": traj["positions"].shape, "speedup_achieved": stats.get("speedup_achieved", 0),
                             "kernel_used": stats.get("best_kernel_used", "unknown"), "elements_per_second": (N * joints) / mean if mean > 0 else 0.0}
            if include_cpu_comparison and results[name]["used_gpu"]:
                old = self.cpu_threshold
                self.cpu_threshold = float("inf")   # the routing rule then picks the CPU launcher
                try:
                    t0 = time.time()
                    self.joint_trajectory(start, end, 2.0, N, 5)
                    cpu_time = time.time() - t0
                finally:
                    self.cpu_threshold = old
                results[name]["cpu_time"] = cpu_time
                results[name]["actual_speedup"] = cpu_time / mean if mean > 0 else 0
            logger.info("%s benchmark: %.4fs, GPU: %s", name, mean, results[name]["used_gpu"])
        return results

    def reset_performance_stats(self) -> None:
        """reference planning/trajectory_planning.py:489-500."""
        self.performance_stats = {"gpu_calls": 0, "cpu_calls": 0, "total_gpu_time": 0.0, "total_cpu_time": 0.0,
                                  "memory_transfers": 0, "kernel_launches": 0, "speedup_achieved": 0.0, "best_kernel_used": "none",
                                  "gpu_kernel_ms_total": 0.0, "gpu_kernel_ms_last": 0.0, "gpu_timed_calls": 0}
        if self.enable_profiling and getattr(self, "_profiling_held", False):
            self._prof_base = _reg.get_context().profile()   # re-base this planner; other users of the context keep their totals

    def close(self) -> None:
        """Give back what this planner holds on the shared context (its profiling reference)."""
        if getattr(self, "_profiling_held", False):
            self._profiling_held = False
            _reg.release_profiling()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def cleanup_gpu_memory(self) -> None:
        """Return the context's pooled device buffers to the driver (reference planning/trajectory_planning.py:502-524)."""
        if self._gpu_routed():
            ctx = _reg.get_context()
            ctx.synchronize()
            ctx.trim_pool()

    def get_performance_stats(self) -> Dict[str, float]:
        """reference planning/trajectory_planning.py:440-487: the counters plus averages, GPU share, overall speed-up and
        the EWMA adaptation of the CPU / GPU work threshold (kept within the reference's [50, 5000] band)."""
        stats = dict(self.performance_stats)
        stats["avg_gpu_time"] = stats["total_gpu_time"] / stats["gpu_calls"] if stats["gpu_calls"] > 0 else 0.0
        stats["avg_cpu_time"] = stats["total_cpu_time"] / stats["cpu_calls"] if stats["cpu_calls"] > 0 else 0.0
        total = stats["gpu_calls"] + stats["cpu_calls"]
        stats["gpu_usage_percent"] = stats["gpu_calls"] / total * 100 if total > 0 else 0.0
        stats["overall_speedup"] = (stats["total_cpu_time"] / stats["total_gpu_time"]
                                    if stats["total_gpu_time"] > 0 and stats["total_cpu_time"] > 0 else 0.0)
        if stats["avg_gpu_time"] > 0 and stats["avg_cpu_time"] > 0:
            ratio = stats["avg_cpu_time"] / stats["avg_gpu_time"]
            self.cpu_threshold = int(0.9 * self.cpu_threshold + 0.1 * ratio * self.cpu_threshold)
            self.cpu_threshold = max(50, min(self.cpu_threshold, 5000))
        return stats


TrajectoryPlanning = OptimizedTrajectoryPlanning  # alias kept by the reference (planning/__init__.py)


def _ilqr_drive(prob, max_iter, tol, reg0):
    """The iLQR iteration of batch_ilqr over a set of primitives (nominal / backward / costs / accept): every decision is taken here, on
    the host, from costs, dV and status alone."""
    B = prob.B
    alphas = 2.0 ** -np.arange(8.0)
    J = prob.nominal()
    reg = np.full(B, float(reg0))
    conv, dead = np.zeros(B, dtype=bool), ~np.isfinite(J)
    iters = np.zeros(B, dtype=np.int64)
    hist, ahist = [J.copy()], []
    for _ in range(int(max_iter)):
        if (conv | dead).all():
            break
        dV, status = prob.backward(reg)
        Jc = prob.costs(np.repeat(alphas[:, None], B, axis=1))
        active = ~(conv | dead)
        with np.errstate(invalid="ignore"):
            pred = -(alphas[:, None] * dV[None, :, 0] + alphas[:, None] ** 2 * dV[None, :, 1])
            ok = np.isfinite(Jc) & (J[None] - Jc >= 1e-4 * pred) & (status == 0)[None] & active[None]
        took = ok.any(axis=0)
        alpha = np.where(took, alphas[np.argmax(ok, axis=0)], 0.0)
        Jn = prob.accept(alpha)
        scale = tol * (1.0 + np.abs(J))
        with np.errstate(invalid="ignore"):
            flat = (status == 0) & (-dV[:, 0] <= scale)
            newly = active & ((took & (J - Jn <= scale)) | flat)
        reg = np.where(active, np.where(took, np.maximum(reg / 10.0, 1e-9), reg * 10.0), reg)
        iters[active] += 1
        dead |= status < 0
        conv |= newly
        J = np.where(took, Jn, J)
        hist.append(J.copy())
        ahist.append(alpha)
    return {"cost": J, "iterations": iters, "converged": conv, "cost_history": np.array(hist),
            "alpha_history": np.array(ahist).reshape(len(ahist), B)}


class _IlqrHost:
    """The iLQR primitives on host arrays through the registered launchers' CPU side (the C ABI's *_cpu twins)."""

    def __init__(self, model, th, dth, tm, xr, wq, wr, wf, g, dt):
        self.model, self.th, self.dth, self.tau, self.xr = model, th, dth, tm, xr
        self.w, self.g, self.dt = (wq, wr, wf), g, dt
        self.B, self.N, self.n = tm.shape
        self.pos = self.vel = None
        self.K, self.k = np.zeros((self.B, self.N, self.n, 2 * self.n)), np.zeros(tm.shape)
        self._roll = _reg.get_registered_kernel("dynamics.ilqr_rollout").cpu_launcher
        self._back = _reg.get_registered_kernel("dynamics.ilqr_backward").cpu_launcher

    def nominal(self):
        cost, pos, vel, _ = self._roll(self.model, self.th, self.dth, self.tau, None, None, None, None, np.zeros((1, self.B)), self.xr,
                                       *self.w, self.g, self.dt, True)
        self.pos, self.vel = pos[0], vel[0]
        return cost[0]

    def backward(self, reg):
        self.K, self.k, dV, status = self._back(self.model, self.pos, self.vel, self.tau, self.xr, *self.w, reg, self.g, self.dt)
        return dV, status

    def costs(self, alpha):
        return self._roll(self.model, self.th, self.dth, self.tau, self.pos, self.vel, self.K, self.k, alpha, self.xr, *self.w, self.g,
                          self.dt, False)[0]

    def accept(self, alpha):
        cost, pos, vel, tau = self._roll(self.model, self.th, self.dth, self.tau, self.pos, self.vel, self.K, self.k, alpha[None], self.xr,
                                         *self.w, self.g, self.dt, True)
        self.pos, self.vel, self.tau = pos[0], vel[0], tau[0]
        return cost[0]

    def result(self):
        return {"taumat": self.tau, "positions": self.pos, "velocities": self.vel, "K": self.K, "k": self.k}

    def close(self):
        pass


class _IlqrDevice:
    """The same primitives on device buffers (time-major): states, derivative blocks and gains never leave the device; a call brings
    back costs, dV and status only, and result() the final arrays."""

    def __init__(self, ctx, model, th, dth, tm, xr, wq, wr, wf, g, dt):
        self.ctx, self.model, self.w, self.g, self.dt = ctx, model, (wq, wr, wf), g, dt
        self.B, self.N, self.n = B, N, n = tm.shape
        self.bufs = []
        f8 = 8
        rows = N * B * n * f8
        try:
            self.th, self.dth = self._up(th), self._up(dth)
            self.tau = [self._up(np.swapaxes(tm, 0, 1)), self._new(rows)]
            self.pos, self.vel = [self._new(rows), self._new(rows)], [self._new(rows), self._new(rows)]
            self.xr = self._up(np.swapaxes(xr, 0, 1))
            blk = (N - 1) * B * n * n * f8
            self.dq, self.dqd, self.mi = self._new(blk), self._new(blk), self._new(blk)
            self.K, self.k = self._new(2 * rows * n), self._new(rows)
            self.work = self._new(_hip.ilqr_backward_workspace_bytes(model, B, N))
            self.reg, self.dV, self.status = self._new(B * f8), self._new(2 * B * f8), self._new(B * 4)
            self.alpha, self.cost = self._new(8 * B * f8), self._new(8 * B * f8)
            self.tau1 = self._new((N - 1) * B * n * f8) if (B * n) % 2 else None
            ctx.memset(self.K, 0, 2 * rows * n)
            ctx.memset(self.k, 0, rows)
        except Exception:
            self.close()
            raise
        self.cur = 0

    def _new(self, nbytes):
        self.bufs.append(self.ctx.alloc(nbytes))
        return self.bufs[-1]

    def _up(self, a):
        self.bufs.append(self.ctx.to_device(np.ascontiguousarray(a)))
        return self.bufs[-1]

    def _rollout(self, alpha, closed, rows):
        A, c, o = alpha.shape[0], self.cur, 1 - self.cur
        if A > 8:
            raise ValueError("at most 8 step sizes a launch")
        self.alpha.upload(alpha)
        loop = (self.pos[c], self.vel[c], self.K, self.k) if closed else (None, None, None, None)
        outs = (self.pos[o], self.vel[o], self.tau[o]) if rows else (None, None, None)
        self.ctx.ilqr_rollout(self.model, self.th, self.dth, self.tau[c], *loop, self.alpha, self.xr, *self.w, A, self.B, self.N, self.g,
                              self.dt, self.cost, *outs)
        if rows:
            self.cur = o
        return self.cost.download((A, self.B), np.float64)

    def nominal(self):
        return self._rollout(np.zeros((1, self.B)), False, True)[0]

    def backward(self, reg):
        B, N, n, c = self.B, self.N, self.n, self.cur
        self.reg.upload(np.ascontiguousarray(reg, dtype=np.float64))
        tau1 = self.tau[c].offset(B * n * 8)    # torque rows 1..N-1
        if (B * n) % 2:                         # 8 bytes off the 16-byte boundary the derivative entry asks for: a device copy
            self.ctx.transpose_rows(tau1, 1, (N - 1) * B, n * 8, self.tau1)
            tau1 = self.tau1
        self.ctx.fd_derivatives(self.model, self.pos[c], self.vel[c], tau1, (N - 1) * B, self.dq, self.dqd, d_Minv=self.mi, g=self.g)
        self.ctx.ilqr_backward(self.model, self.pos[c], self.vel[c], self.tau[c], self.dq, self.dqd, self.mi, self.xr, *self.w, self.reg, B,
                               N, self.dt, self.work, self.K, self.k, self.dV, self.status)
        return self.dV.download((B, 2), np.float64), self.status.download((B,), np.int32)

    def costs(self, alpha):
        return self._rollout(np.ascontiguousarray(alpha, dtype=np.float64), True, False)

    def accept(self, alpha):
        return self._rollout(np.ascontiguousarray(alpha, dtype=np.float64)[None], True, True)[0]

    def result(self):
        B, N, n, c = self.B, self.N, self.n, self.cur
        bm = lambda buf, tail: np.ascontiguousarray(np.swapaxes(buf.download((N, B) + tail, np.float64), 0, 1))  # noqa: E731
        return {"taumat": bm(self.tau[c], (n,)), "positions": bm(self.pos[c], (n,)), "velocities": bm(self.vel[c], (n,)),
                "K": bm(self.K, (n, 2 * n)), "k": bm(self.k, (n,))}

    def close(self):
        for b in self.bufs:
            b.free()
        self.bufs = []
