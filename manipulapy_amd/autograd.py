"""torch.autograd access to the analytical dynamics derivatives (csrc/mp_deriv.h).

    from manipulapy_amd import autograd as mpa
    tau = mpa.inverse_dynamics(dyn, q, qd, qdd, g, Ftip)          # q, qd, qdd: CPU float64 tensors, (n,) or (rows, n)
    J = torch.autograd.functional.jacobian(lambda q: mpa.inverse_dynamics(dyn, q, qd, qdd, g, Ftip), q)
    pos, vel, acc = mpa.forward_dynamics_trajectory(planner, theta0, dtheta0, taumat, g, Ftipmat, dt=0.01, intRes=1)
    tau = mpa.inverse_dynamics_parameters(dyn, params, q, qd, qdd, g, Ftip)   # differentiable in params (n, 10)

The forward value is the registered inverse / forward dynamics operation, the backward pass the vector-Jacobian product with the
registered derivative operation ("dynamics.inverse_derivatives" / "dynamics.fwd_derivatives"): the GPU under the "hip" backend,
the CPU twin otherwise.  forward_dynamics_trajectory is a planner's roll-out ("dynamics.forward_trajectory") whose backward pass is
the reverse pass through its sub-steps ("dynamics.forward_trajectory_vjp", csrc/mp_rollout_vjp.h).  Once differentiable (no second derivatives).  g and Ftip are constants: a tensor among them that
requires grad is refused.  inverse_dynamics_parameters is tau = Y(q, qd, qdd) pi + tau_ext ("dynamics.inverse_regressor"), whose
backward pass is sum Y^T g_tau from the normal-equations operation ("dynamics.inverse_regressor_normal", no A, rhs = g_tau): Y is
never formed.  Imported on demand only - never from the package's __init__ (torch stays optional).
"""
from __future__ import annotations

import numpy as np
import torch

from .registry import execute_registered_kernel

__all__ = ["inverse_dynamics", "forward_dynamics", "forward_dynamics_trajectory", "inverse_dynamics_parameters"]


def _const(v, name):
    if v is None:
        return None
    if isinstance(v, torch.Tensor):
        if v.requires_grad:
            raise ValueError(f"{name}: gradients with respect to g and Ftip are not provided - pass a tensor without requires_grad")
        v = v.detach().cpu().numpy()
    return np.asarray(v, dtype=np.float64)


def _rows(t: torch.Tensor, name: str) -> np.ndarray:
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t, dtype=torch.float64)
    if t.dtype != torch.float64 or t.device.type != "cpu":
        raise TypeError(f"{name}: expected a CPU float64 tensor, got {t.dtype} on {t.device}")
    return np.atleast_2d(t.detach().numpy()).astype(np.float64, copy=False)


def _derivatives(op, dyn, q, qd, x, g, F):
    model = dyn._derivative_model(op)
    return execute_registered_kernel(op, model, q, qd, x, g, F)


def _vjp(gy: torch.Tensor, J: np.ndarray, one: bool) -> torch.Tensor:
    g2 = np.atleast_2d(gy.detach().cpu().numpy().astype(np.float64))
    out = torch.from_numpy(np.einsum("ri,rij->rj", g2, J))
    return out[0] if one else out


class _InverseDynamics(torch.autograd.Function):
    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gtau):
        dq, dqd, M = ctx.jac
        return None, _vjp(gtau, dq, ctx.one), _vjp(gtau, dqd, ctx.one), _vjp(gtau, M, ctx.one), None, None

    @staticmethod
    def forward(ctx, dyn, q, qd, qdd, g, Ftip):
        one = q.dim() == 1
        a, b, c = _rows(q, "q"), _rows(qd, "qd"), _rows(qdd, "qdd")
        tau, dq, dqd, M = _derivatives("dynamics.inverse_derivatives", dyn, a, b, c, g, Ftip)
        ctx.jac, ctx.one = (dq, dqd, M), one
        out = torch.from_numpy(tau)
        return out[0] if one else out


class _ForwardDynamics(torch.autograd.Function):
    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gqdd):
        dq, dqd, Minv = ctx.jac
        return None, _vjp(gqdd, dq, ctx.one), _vjp(gqdd, dqd, ctx.one), _vjp(gqdd, Minv, ctx.one), None, None

    @staticmethod
    def forward(ctx, dyn, q, qd, tau, g, Ftip):
        one = q.dim() == 1
        a, b, c = _rows(q, "q"), _rows(qd, "qd"), _rows(tau, "tau")
        qdd, dq, dqd, Minv = _derivatives("dynamics.fwd_derivatives", dyn, a, b, c, g, Ftip)
        ctx.jac, ctx.one = (dq, dqd, Minv), one
        out = torch.from_numpy(qdd)
        return out[0] if one else out


def _as_tensor(x):
    return x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, dtype=np.float64))


def inverse_dynamics(dyn, q, qd, qdd, g=None, Ftip=None) -> torch.Tensor:
    """tau = ID(q, qd, qdd, g, Ftip) of a ManipulatorDynamics (with Mlist_per_link, n <= 8), differentiable in q, qd, qdd.
    (n,) inputs give (n,), (rows, n) inputs (rows, n); one g / Ftip for every row."""
    return _InverseDynamics.apply(dyn, _as_tensor(q), _as_tensor(qd), _as_tensor(qdd), _const(g, "g"), _const(Ftip, "Ftip"))


def forward_dynamics(dyn, q, qd, tau, g=None, Ftip=None) -> torch.Tensor:
    """qdd = FD(q, qd, tau, g, Ftip), differentiable in q, qd, tau; shapes as inverse_dynamics."""
    return _ForwardDynamics.apply(dyn, _as_tensor(q), _as_tensor(qd), _as_tensor(tau), _const(g, "g"), _const(Ftip, "Ftip"))


class _ForwardDynamicsTrajectory(torch.autograd.Function):
    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gpos, gvel, gacc):
        planner, th, dth, tm, g, F, dt, intRes = ctx.args
        cot = [None if x is None else x.detach().cpu().numpy().astype(np.float64).reshape(tm.shape) for x in (gpos, gvel, gacc)]
        r = planner.batch_forward_dynamics_trajectory_vjp(th, dth, tm, g, F, dt, intRes, *cot)
        out = [torch.from_numpy(np.ascontiguousarray(r[k], dtype=np.float64)) for k in ("theta0", "dtheta0", "taumat")]
        if ctx.one:
            out = [o[0] for o in out]
        return (None, *out, None, None, None, None)

    @staticmethod
    def forward(ctx, planner, theta0, dtheta0, taumat, g, Ftipmat, dt, intRes):
        one = taumat.dim() == 2
        tm = _rows(taumat, "taumat")
        tm = tm[None] if one else tm
        th, dth = (_rows(a, n).reshape(tm.shape[0], tm.shape[2]) for a, n in ((theta0, "theta0"), (dtheta0, "dtheta0")))
        F = None if Ftipmat is None else Ftipmat.reshape(tm.shape[:2] + (6,))
        r = planner.batch_forward_dynamics_trajectory(th, dth, tm, g, F, dt, intRes)
        ctx.args, ctx.one = (planner, th, dth, tm, g, F, dt, intRes), one
        out = [torch.as_tensor(np.asarray(r[k], dtype=np.float32)) for k in ("positions", "velocities", "accelerations")]
        return tuple(o[0] for o in out) if one else tuple(out)


def forward_dynamics_trajectory(planner, theta0, dtheta0, taumat, g=None, Ftipmat=None, dt: float = 0.01, intRes: int = 1):
    """(positions, velocities, accelerations) float32 rows of an OptimizedTrajectoryPlanning's forward-dynamics roll-out, differentiable
    in theta0, dtheta0 and taumat (CPU float64 tensors).  taumat (N, n) with theta0 / dtheta0 (n,), or (B, N, n) with (B, n);
    Ftipmat (N, 6) / (B, N, 6) or None.  The float32 cast of the rows counts as the identity; g and Ftipmat are constants."""
    return _ForwardDynamicsTrajectory.apply(planner, _as_tensor(theta0), _as_tensor(dtheta0), _as_tensor(taumat), _const(g, "g"),
                                            _const(Ftipmat, "Ftipmat"), float(dt), int(intRes))


class _InverseDynamicsParameters(torch.autograd.Function):
    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gtau):
        dyn, q, qd, qdd, g = ctx.args
        gt = np.ascontiguousarray(np.atleast_2d(gtau.detach().cpu().numpy()).astype(np.float64))
        model = dyn._derivative_model("inverse_dynamics_parameters")
        _, b, _ = execute_registered_kernel("dynamics.inverse_regressor_normal", model, q, qd, qdd, gt, g, None, want_A=False)
        return None, torch.from_numpy(b.reshape(ctx.shape)), None, None, None, None, None

    @staticmethod
    def forward(ctx, dyn, params, q, qd, qdd, g, Ftip):
        one = q.dim() == 1
        a, b, c = _rows(q, "q"), _rows(qd, "qd"), _rows(qdd, "qdd")
        pi = _rows(params, "params").reshape(-1)
        Y, te = dyn.inverse_dynamics_regressor(a, b, c, g, Ftip)
        ctx.args, ctx.shape = (dyn, a, b, c, g), tuple(params.shape)
        out = torch.from_numpy(np.einsum("rjp,p->rj", Y, pi) + te)
        return out[0] if one else out


def inverse_dynamics_parameters(dyn, params, q, qd, qdd, g=None, Ftip=None) -> torch.Tensor:
    """tau = Y(q, qd, qdd, g) pi + tau_ext(q, Ftip) of a ManipulatorDynamics (with Mlist_per_link, n <= 8) at the inertial parameters
    `params` ((n, 10) or (10n,), ManipulatorDynamics.inertial_parameters()'s convention), differentiable in params only.  (n,) inputs
    give (n,), (rows, n) inputs (rows, n).  Gradients with respect to q, qd, qdd are not provided here (inverse_dynamics has them)."""
    for x, name in ((q, "q"), (qd, "qd"), (qdd, "qdd")):
        if isinstance(x, torch.Tensor) and x.requires_grad:
            raise ValueError(f"inverse_dynamics_parameters: {name} requires grad - this function is differentiable in params only "
                             "(use inverse_dynamics for gradients with respect to the state)")
    return _InverseDynamicsParameters.apply(dyn, _as_tensor(params), _as_tensor(q), _as_tensor(qd), _as_tensor(qdd), _const(g, "g"),
                                            _const(Ftip, "Ftip"))
