"""ManipulatorDynamics — host-side mirror of ManipulaPy/dynamics/manipulator_dynamics.py.

Same constructor signature (dynamics/manipulator_dynamics.py:43-86) and the same public methods:
mass_matrix (mass_matrix.py:16-99), velocity_quadratic_forces / gravity_forces (forces.py:26-133),
inverse_dynamics / forward_dynamics (id_fd.py:16-83), partial_derivative (forces.py:16-24).
Every method runs a registered operation through the kernel registry (float64): its HIP kernel with the "hip" backend
active, its CPU launcher (the C ABI's *_cpu twin, same per-row code) with the NumPy backend active:

    inverse_dynamics(q, qd, qdd, g, F)      "dynamics.inverse_trajectory"   ID(q, qd, qdd, g, F)
    gravity_forces(q, g)                    "dynamics.inverse_trajectory"   ID(q, 0, 0, g, 0)
    velocity_quadratic_forces(q, qd)        "dynamics.inverse_trajectory"   ID(q, qd, 0, 0, 0)
    mass_matrix(q)                          "dynamics.mass_matrix"          columns ID(q, 0, e_j, 0, 0), symmetrised
    forward_dynamics(q, qd, tau, g, F)      "dynamics.forward"              solve(M, tau - ID(q, qd, 0, g, F))

which are exact identities of tau = M qdd + c + g + Js^T F.  2-D inputs (rows, n) evaluate all rows
in one launch.  There is no value-keyed cache (the
reference's caches exist to amortise its 1 + 2n mass-matrix evaluations per point, which the
analytic recursion does not need).

The legacy object (Mlist_per_link=None: what URDF.to_manipulator_dynamics() and hand-built models give,
reference urdf/core.py:795-817) is reproduced, not rejected: the reference evaluates it with an approximation it documents
as incorrect and warns about (dynamics/mass_matrix.py:45-57, :101-132, forces.py:81-95, :136-154).  That
approximation is not rigid-body dynamics, so it cannot be a compiled link-frame model; it runs on the host in NumPy under
every backend (same formulas, same warnings, pinned by tests/golden/legacy_dynamics.npz).
"""
from __future__ import annotations

import logging
import os
import warnings
from typing import Optional

import numpy as np

from . import _hip
from .kinematics import SerialManipulator
from .registry import execute_registered_kernel

__all__ = ["ManipulatorDynamics"]

logger = logging.getLogger("ManipulaPy.dynamics")

_ZERO3 = np.zeros(3)


class ManipulatorDynamics(SerialManipulator):
    def __init__(self, M_list, omega_list, r_list, b_list, S_list, B_list, Glist, Mlist_per_link=None) -> None:
        super().__init__(M_list, omega_list, r_list, b_list, S_list, B_list)
        self.Glist = Glist
        self.Mlist_per_link = Mlist_per_link
        self._dyn_model: Optional[_hip.HipModel] = None
        self._spec_tried = False

    # ---- compiled model
    def hip_model(self, joint_limits=None, torque_limits=None) -> _hip.HipModel:
        """Compile (once) the model the kernels consume.  Limits, if given, build a separate model
        (the planner passes its own float32 limits)."""
        if self.Mlist_per_link is None:
            raise NotImplementedError(
                "ManipulatorDynamics without Mlist_per_link has no compiled model: its legacy approximation "
                "(dynamics/mass_matrix.py:101-132) is evaluated on the host (mass_matrix / gravity_forces / inverse_dynamics / "
                "forward_dynamics and the planner's trajectory methods do that by themselves)")
        if joint_limits is None and torque_limits is None:
            if self._dyn_model is None:
                self._dyn_model = _hip.HipModel(self.S_list, np.asarray(self.Mlist_per_link), np.asarray(self.Glist), self._M_ee)
            return self._dyn_model
        return _hip.HipModel(self.S_list, np.asarray(self.Mlist_per_link), np.asarray(self.Glist), self._M_ee,
                             joint_limits, torque_limits)

    def _model_for(self, rows: int) -> _hip.HipModel:
        """The shared model; for big batches it is specialised first (~2 s once, cached on disk: the per-row forward
        dynamics kernel runs 3x faster with this robot's constants baked in)."""
        model = self.hip_model()
        if (rows >= 16384 and os.environ.get("MANIPULAPY_HIP_SPECIALIZE", "1") != "0" and not self._spec_tried
                and model.n <= _hip.MP_MAX_DOF):   # (9..32 joints run the looped generic kernels: nothing to specialise)
            from .registry import _hip_routing_enabled, get_context

            if _hip_routing_enabled():
                self._spec_tried = True
                try:
                    get_context().specialize(model)
                except _hip.HipError as exc:  # e.g. no hiprtc on this machine: the generic GPU kernels serve
                    logger.warning("kernel specialisation unavailable (%s); using the generic kernels", exc)
        return model

    def _id(self, q, qd, qdd, g, Ftip) -> np.ndarray:
        return execute_registered_kernel("dynamics.inverse_trajectory", self._model_for(np.shape(q)[0]), q, qd, qdd, g, Ftip,
                                         dtype=np.float64)

    # ---- the legacy (Mlist_per_link=None) approximation, on the host
    @property
    def _legacy(self) -> bool:
        return self.Mlist_per_link is None

    def _mass_matrix_legacy(self, q: np.ndarray) -> np.ndarray:
        """Row i = J_i^T (Ad_i^T G_i Ad_i) J_s with Ad_i = Ad(FK(q[:i + 1])), symmetrised
        (reference dynamics/mass_matrix.py:101-132; documented there as incorrect, kept for hand-built models)."""
        from .utils import adjoint_transform

        n = len(q)
        J = self.jacobian(q, frame="space")
        M = np.zeros((n, n))
        for i in range(n):
            Ad = adjoint_transform(self.forward_kinematics(q[: i + 1], frame="space"))
            M[i] = J[:, i] @ (Ad.T @ np.asarray(self.Glist[i], dtype=np.float64) @ Ad) @ J
        return 0.5 * (M + M.T)

    def _gravity_forces_legacy(self, q: np.ndarray, g: np.ndarray) -> np.ndarray:
        """(R_i^T g) . (column sums of G_i's inertia block), R_i from FK(q[:i + 1]) (reference dynamics/forces.py:136-154)."""
        out = np.zeros(len(q))
        for i in range(len(q)):
            R = self.forward_kinematics(q[: i + 1], "space")[:3, :3]
            out[i] = (R.T @ g[:3]) @ np.asarray(self.Glist[i], dtype=np.float64)[:3, :3].sum(axis=0)
        return out

    def _warn_legacy(self, what: str, fix: str) -> None:
        warnings.warn(f"{what} called without Mlist_per_link \u2014 using legacy approximation (incorrect for non-trivial "
                      f"robots). Construct ManipulatorDynamics via URDFToSerialManipulator to get accurate {fix}.", stacklevel=3)

    def _velocity_quadratic_legacy(self, q: np.ndarray, qd: np.ndarray, epsilon: float = 1e-6) -> np.ndarray:
        """Christoffel form on the central difference of the (legacy) mass matrix (reference dynamics/cache.py:23-56,
        forces.py:45-59)."""
        n = len(q)
        dM = np.zeros((n, n, n))
        for k in range(n):
            e = np.zeros(n)
            e[k] = epsilon
            dM[:, :, k] = (self.mass_matrix(q + e) - self.mass_matrix(q - e)) / (2.0 * epsilon)
        c = np.zeros(n)
        for i in range(n):
            gamma = 0.5 * (dM[i] + dM[i].T - dM[:, :, i])
            c[i] = qd @ gamma @ qd
        return c

    # ---- public API
    def mass_matrix(self, thetalist) -> np.ndarray:
        """(n, n) mass matrix, or (rows, n, n) for a 2-D `thetalist`."""
        if self._legacy:
            self._warn_legacy("mass_matrix", "mass matrix")
            q = np.asarray(thetalist, dtype=np.float64)
            return self._mass_matrix_legacy(q) if q.ndim == 1 else np.stack([self._mass_matrix_legacy(r) for r in q])
        q = np.atleast_2d(np.asarray(thetalist, dtype=np.float64))
        M = execute_registered_kernel("dynamics.mass_matrix", self._model_for(q.shape[0]), q)
        return M if np.ndim(thetalist) == 2 else M[0]

    def velocity_quadratic_forces(self, thetalist, dthetalist) -> np.ndarray:
        if self._legacy:
            self._warn_legacy("mass_matrix", "mass matrix")   # (the reference warns once per uncached evaluation: 2n times here)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                return self._velocity_quadratic_legacy(np.asarray(thetalist, dtype=np.float64), np.asarray(dthetalist, dtype=np.float64))
        q = np.asarray(thetalist, dtype=np.float64)[None, :]
        qd = np.asarray(dthetalist, dtype=np.float64)[None, :]
        return self._id(q, qd, np.zeros_like(q), _ZERO3, None)[0]

    def gravity_forces(self, thetalist, g=None) -> np.ndarray:
        g = [0.0, 0.0, -9.81] if g is None else g
        if self._legacy:
            self._warn_legacy("gravity_forces", "gravity compensation")
            return self._gravity_forces_legacy(np.asarray(thetalist, dtype=np.float64), np.asarray(g, dtype=np.float64))
        q = np.asarray(thetalist, dtype=np.float64)[None, :]
        z = np.zeros_like(q)
        return self._id(q, z, z, g, None)[0]

    def _legacy_terms(self, q, qd, g):
        """M, c, g-forces and Js^T of the legacy model (each warns as the reference's does)."""
        M = self.mass_matrix(q)
        c = self.velocity_quadratic_forces(q, qd)
        gf = self.gravity_forces(q, g)
        return M, c, gf, self.jacobian(q).T

    def inverse_dynamics(self, thetalist, dthetalist, ddthetalist, g, Ftip) -> np.ndarray:
        if self._legacy:   # M qdd + c + g + Js^T Ftip on the legacy terms (reference dynamics/id_fd.py:36-48)
            q, qd = np.asarray(thetalist, dtype=np.float64), np.asarray(dthetalist, dtype=np.float64)
            M, c, gf, Jt = self._legacy_terms(q, qd, g)
            return M @ np.asarray(ddthetalist, dtype=np.float64) + c + gf + Jt @ np.asarray(Ftip, dtype=np.float64)
        q = np.asarray(thetalist, dtype=np.float64)[None, :]
        qd = np.asarray(dthetalist, dtype=np.float64)[None, :]
        qdd = np.asarray(ddthetalist, dtype=np.float64)[None, :]
        return self._id(q, qd, qdd, g, Ftip)[0]

    def forward_dynamics(self, thetalist, dthetalist, taulist, g, Ftip) -> np.ndarray:
        """qdd (n,), or (rows, n) for 2-D inputs (one g / Ftip for all rows)."""
        if self._legacy:   # solve(M, tau - c - g - Js^T Ftip) (reference dynamics/id_fd.py:71-83)
            q, qd = np.asarray(thetalist, dtype=np.float64), np.asarray(dthetalist, dtype=np.float64)
            M, c, gf, Jt = self._legacy_terms(q, qd, g)
            return np.linalg.solve(M, np.asarray(taulist, dtype=np.float64) - c - gf - Jt @ np.asarray(Ftip, dtype=np.float64))
        q = np.atleast_2d(np.asarray(thetalist, dtype=np.float64))
        qd = np.atleast_2d(np.asarray(dthetalist, dtype=np.float64))
        tau = np.atleast_2d(np.asarray(taulist, dtype=np.float64))
        qdd = execute_registered_kernel("dynamics.forward", self._model_for(q.shape[0]), q, qd, tau, g, Ftip)
        return qdd if np.ndim(thetalist) == 2 else qdd[0]

    # ---- analytical derivatives (float64, n <= 8; csrc/mp_deriv.h)
    def _derivative_model(self, what: str) -> _hip.HipModel:
        if self._legacy:
            raise NotImplementedError(f"{what}: needs Mlist_per_link - the legacy approximation has no analytical derivatives")
        model = self.hip_model()
        if model.n > _hip.MP_MAX_DOF:
            raise NotImplementedError(f"{what}: the analytical derivatives cover models of up to {_hip.MP_MAX_DOF} joints "
                                      f"(this one has {model.n})")
        return model

    def _derivatives(self, op, what, q, qd, x, g, Ftip):
        model = self._derivative_model(what)
        one = np.ndim(q) == 1
        q2, qd2, x2 = (np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in (q, qd, x))
        _, dq, dqd, mat = execute_registered_kernel(op, model, q2, qd2, x2, g, Ftip)
        return (dq[0], dqd[0], mat[0]) if one else (dq, dqd, mat)

    def inverse_dynamics_derivatives(self, thetalist, dthetalist, ddthetalist, g, Ftip):
        """(dtau_dq, dtau_dqd, dtau_dqdd = M) of tau = inverse_dynamics(...), [.., i, j] = d tau_i / d x_j: (n, n) each for 1-D
        inputs, (rows, n, n) for 2-D ones (one g / Ftip for all rows).  Derivatives of the unclipped torque."""
        return self._derivatives("dynamics.inverse_derivatives", "inverse_dynamics_derivatives", thetalist, dthetalist, ddthetalist,
                                 g, Ftip)

    def forward_dynamics_derivatives(self, thetalist, dthetalist, taulist, g, Ftip):
        """(dqdd_dq, dqdd_dqd, dqdd_dtau = M^-1) of qdd = forward_dynamics(...), [.., i, j] = d qdd_i / d x_j: (n, n) each for 1-D
        inputs, (rows, n, n) for 2-D ones (one g / Ftip for all rows)."""
        return self._derivatives("dynamics.fwd_derivatives", "forward_dynamics_derivatives", thetalist, dthetalist, taulist, g, Ftip)

    # ---- vector-Jacobian products (float64, n <= 8; csrc/mp_adjoint.h): reverse mode, no Jacobian formed
    def _vjp(self, op, what, q, qd, x, cot, g, Ftip):
        model = self._derivative_model(what)
        one = np.ndim(q) == 1
        q2, qd2, x2, c2 = (np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in (q, qd, x, cot))
        out = execute_registered_kernel(op, model, q2, qd2, x2, c2, g, Ftip)
        return tuple(o[0] for o in out) if one else tuple(out)

    def inverse_dynamics_vjp(self, thetalist, dthetalist, ddthetalist, gtau, g, Ftip):
        """(gq, gqd, gqdd) = (dtau_dq^T gtau, dtau_dqd^T gtau, M gtau) of tau = inverse_dynamics(...) for the cotangent gtau: (n,)
        each for 1-D inputs, (rows, n) for 2-D ones (one g / Ftip for all rows).  Derivatives of the unclipped torque."""
        return self._vjp("dynamics.inverse_vjp", "inverse_dynamics_vjp", thetalist, dthetalist, ddthetalist, gtau, g, Ftip)

    def forward_dynamics_vjp(self, thetalist, dthetalist, taulist, gqdd, g, Ftip):
        """(gq, gqd, gtau) = (dqdd_dq^T gqdd, dqdd_dqd^T gqdd, M^-1 gqdd) of qdd = forward_dynamics(...) for the cotangent gqdd;
        shapes as inverse_dynamics_vjp."""
        _, gq, gqd, gtau = self._vjp("dynamics.fwd_vjp", "forward_dynamics_vjp", thetalist, dthetalist, taulist, gqdd, g, Ftip)
        return gq, gqd, gtau

    # ---- operational-space dynamics and task-space torque (float64, n <= 8; csrc/mp_opspace.h)
    def operational_space_dynamics(self, thetalist, dthetalist, g, frame: str = "hybrid", task: str = "full", damping: float = 0.0) -> dict:
        """{"T", "J", "Jdot_qd", "Lambda", "Jbar", "mu", "p"} of the tool in `frame` ("space", "body", or "hybrid": angular and
        tool-origin velocity in space axes) for the rows of `task` ("full": [w; v], m = 6; "linear": v; "angular": w; m = 3):
        Lambda = (J M^-1 J^T + damping^2 1)^-1, Jbar = M^-1 J^T Lambda, mu = Lambda (J M^-1 c - Jdot qd), p = Lambda J M^-1 g.
        Shapes (4, 4), (m, n), (m,), (m, m), (n, m), (m,), (m,) for 1-D inputs, with a leading rows axis for 2-D ones (one g for all
        rows).  With damping = 0, a row whose factorisation of J M^-1 J^T meets a non-positive pivot is NaN in Lambda, Jbar, mu and p (that
        row only), and so is every row of a task with more rows than the chain has joints; a nearly singular pose may also come back
        finite and huge (include/manipula_hip.h)."""
        model = self._derivative_model("operational_space_dynamics")
        one = np.ndim(thetalist) == 1
        q, qd = (np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in (thetalist, dthetalist))
        out = execute_registered_kernel("dynamics.operational_space", model, q, qd, g, frame, task, damping)
        return {k: v[0] for k, v in out.items()} if one else out

    def operational_space_torque(self, thetalist, dthetalist, task_acceleration, g, tau_null=None, frame: str = "hybrid",
                                 task: str = "full", damping: float = 0.0) -> np.ndarray:
        """tau = J^T (Lambda a* + mu + p) + (1 - J^T Jbar^T) tau_null for the task acceleration a* ((m,) or (rows, m)): with
        damping = 0, forward_dynamics of it gives J qdd + Jdot qd = a* whatever tau_null is.  One launch; no Jacobian, mass matrix or
        Lambda leaves the device.  A tip wrench F is the caller's J^T F."""
        model = self._derivative_model("operational_space_torque")
        one = np.ndim(thetalist) == 1
        q, qd, acc = (np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in (thetalist, dthetalist, task_acceleration))
        t0 = None if tau_null is None else np.atleast_2d(np.asarray(tau_null, dtype=np.float64))
        tau = execute_registered_kernel("dynamics.operational_space_torque", model, q, qd, acc, g, t0, frame, task, damping)
        return tau[0] if one else tau

    # ---- dynamics regressor and inertial-parameter identification (float64, n <= 8; csrc/mp_regressor.h)
    # pi_i = [m, hx, hy, hz, Ixx, Ixy, Ixz, Iyy, Iyz, Izz] in link i's CoM frame at the home pose (Mlist_per_link[i]): h = m c with c
    # the centre of mass from that frame's origin, I the inertia about that origin.  tau = Y pi + tau_ext (tau_ext: the tip wrench's
    # share).
    def inertial_parameters(self) -> np.ndarray:
        """(n, 10) inertial parameters of the model as loaded: [m, 0, 0, 0, Ic entries] (Glist[i] = blockdiag(Ic, m 1))."""
        model = self._derivative_model("inertial_parameters")
        out = np.zeros((model.n, 10))
        for i, G in enumerate(np.asarray(self.Glist, dtype=np.float64)):
            Ic = 0.5 * (G[:3, :3] + G[:3, :3].T)
            out[i] = [G[3, 3], 0.0, 0.0, 0.0, Ic[0, 0], Ic[0, 1], Ic[0, 2], Ic[1, 1], Ic[1, 2], Ic[2, 2]]
        return out

    def inverse_dynamics_regressor(self, thetalist, dthetalist, ddthetalist, g, Ftip=None):
        """(Y, tau_ext) with tau = Y @ inertial_parameters().ravel() + tau_ext: (n, 10n) and (n,) for 1-D inputs, (rows, n, 10n) and
        (rows, n) for 2-D ones (one g / Ftip for all rows).  Y[.., j, 10 k + c] = d tau_j / d pi_k[c]."""
        model = self._derivative_model("inverse_dynamics_regressor")
        one = np.ndim(thetalist) == 1
        q, qd, qdd = (np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in (thetalist, dthetalist, ddthetalist))
        Y, te = execute_registered_kernel("dynamics.inverse_regressor", model, q, qd, qdd, g, Ftip)
        return (Y[0], te[0]) if one else (Y, te)

    def identify_inertial_parameters(self, thetalist, dthetalist, ddthetalist, taulist, g, Ftip=None, prior=None,
                                     ridge: float = 1e-8) -> dict:
        """Least-squares inertial parameters from (rows, n) samples of (q, qd, qdd, tau): the normal equations A = sum Y^T Y,
        b = sum Y^T (tau - tau_ext) are reduced on the device without forming Y, then (A + ridge s 1) pi = b + ridge s prior is solved
        on the host (float64, eigh), s = mean(diag(A)).  The ridge pulls the parameters that the data cannot identify (Y is
        rank-deficient for every real arm: only base parameters are identifiable) towards `prior` (default inertial_parameters()).
        Returns {"params" (n, 10), "A", "b", "rows", "rank" (eigenvalues of A above 1e-10 max), "residual_rms"}."""
        model = self._derivative_model("identify_inertial_parameters")
        q, qd, qdd, tau = (np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in (thetalist, dthetalist, ddthetalist, taulist))
        A, b, rr = execute_registered_kernel("dynamics.inverse_regressor_normal", model, q, qd, qdd, tau, g, Ftip)
        w = 10 * model.n
        p0 = (self.inertial_parameters() if prior is None else np.asarray(prior, dtype=np.float64)).reshape(w)
        s = float(np.mean(np.diag(A))) or 1.0
        lam, V = np.linalg.eigh(0.5 * (A + A.T) + ridge * s * np.eye(w))
        pi = V @ ((V.T @ (b + ridge * s * p0)) / lam)
        ev = np.linalg.eigvalsh(0.5 * (A + A.T))
        rank = int(np.sum(ev > 1e-10 * max(float(ev.max()), 0.0))) if ev.size and ev.max() > 0 else 0
        rows = q.shape[0]
        res2 = max(rr - 2.0 * float(pi @ b) + float(pi @ A @ pi), 0.0)
        return {"params": pi.reshape(model.n, 10), "A": A, "b": b, "rows": rows, "rank": rank,
                "residual_rms": float(np.sqrt(res2 / max(rows * model.n, 1)))}

    def with_inertial_parameters(self, params) -> "ManipulatorDynamics":
        """A new ManipulatorDynamics with the inertial parameters `params` ((n, 10) or (10n,), this model's convention): per link
        c = h / m, Ic = I - m (|c|^2 1 - c c^T), the CoM frame moved by c along its own axes, Glist = blockdiag(Ic, m 1)."""
        model = self._derivative_model("with_inertial_parameters")
        P = np.asarray(params, dtype=np.float64).reshape(model.n, 10)
        Ml = np.array(self.Mlist_per_link, dtype=np.float64)
        Gl = []
        for i, (m, hx, hy, hz, Ixx, Ixy, Ixz, Iyy, Iyz, Izz) in enumerate(P):
            if not m > 0.0:
                raise ValueError(f"with_inertial_parameters: link {i} has mass {m}; masses must be positive")
            c = np.array([hx, hy, hz]) / m
            I = np.array([[Ixx, Ixy, Ixz], [Ixy, Iyy, Iyz], [Ixz, Iyz, Izz]])
            G = np.zeros((6, 6))
            G[:3, :3] = I - m * (np.dot(c, c) * np.eye(3) - np.outer(c, c))
            G[3:, 3:] = m * np.eye(3)
            Gl.append(G)
            Ml[i, :3, 3] = Ml[i, :3, 3] + Ml[i, :3, :3] @ c
        out = type(self)(self.M_list, self.omega_list, self.r_list, self.b_list, self.S_list, self.B_list, Gl, list(Ml))
        out.joint_limits = self.joint_limits
        return out

    def partial_derivative(self, i: int, j: int, k: int, thetalist, epsilon: float = 1e-6) -> float:
        """dM[i, j] / dtheta_k by the reference's central difference (dynamics/cache.py:39-52)."""
        q = np.asarray(thetalist, dtype=np.float64)
        e = np.zeros_like(q)
        e[k] = epsilon
        return float((self.mass_matrix(q + e)[i, j] - self.mass_matrix(q - e)[i, j]) / (2.0 * epsilon))
