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

Device tensors.  inverse_dynamics / forward_dynamics also take ROCm float64 tensors (q, qd and qdd / tau all on the device of the
library's context, MANIPULAPY_HIP_DEVICE, default 0).  Placing the tensors there is the opt-in: they run on the GPU whatever
set_backend says.  The forward value comes from the float64 inverse / forward dynamics kernels (unclipped tau; qdd), the backward
pass from the reverse-mode vector-Jacobian kernels ("dynamics.inverse_vjp" / "dynamics.fwd_vjp", csrc/mp_adjoint.h): only the
inputs are saved, no Jacobian is formed, and no row or gradient leaves the device.  Every launch is ordered on
torch.cuda.current_stream() (the library's compute stream waits for it before the launch, and it waits for the compute stream after).
float32 device tensors, a mix of host and device tensors and a device other than the context's are refused (TypeError / ValueError).
g and Ftip are per-call constants: a device tensor among them is copied to the host (3 / 6 numbers, a synchronising copy).
inverse_dynamics_parameters and forward_dynamics_trajectory take CPU tensors only.

Kinematics.  fk_jacobian(sm, q, frame) returns (T, J) = (SerialManipulator.forward_kinematics(q), .jacobian(q, frame)) of a chain of
at most 8 joints, differentiable in q; forward_kinematics / jacobian are its two halves.  The forward value and the backward pass are
one registered operation ("kinematics.fk_jacobian_vjp", csrc/mp_kin_vjp.h): the backward pass takes both cotangents in one launch
(a cotangent torch does not provide is not read), O(n) per row, no Jacobian of T or J formed.  CPU float64 tensors and ROCm float64
tensors, with the same rules and the same stream order as the dynamics above; only q is saved.  A truncated q and frame="body" on a
model whose B_list is not Ad(M^-1) S_list are refused (no gradient there).

    T, J = mpa.fk_jacobian(sm, q, "body")          # q: (n,) or (rows, n)
    w = torch.sqrt(torch.det(J @ J.transpose(-1, -2)))
"""
from __future__ import annotations

import numpy as np
import torch

from .registry import execute_registered_kernel

__all__ = ["inverse_dynamics", "forward_dynamics", "forward_dynamics_trajectory", "inverse_dynamics_parameters", "fk_jacobian",
           "forward_kinematics", "jacobian", "collision_cost"]


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


def _on_device(*ts) -> bool:
    return any(isinstance(t, torch.Tensor) and t.device.type == "cuda" for t in ts)


def _device_rows(ts, names):
    """(context, contiguous 16-byte-aligned detached tensors) of ROCm float64 state tensors on the library context's device."""
    from .registry import get_context

    hctx = get_context()
    shape = ts[0].shape
    out = []
    for t, name in zip(ts, names):
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            dev = t.device if isinstance(t, torch.Tensor) else "host"
            raise ValueError(f"{name}: mixed devices - every state tensor must be on the GPU when one is (got {dev})")
        if t.dtype != torch.float64:
            raise TypeError(f"{name}: device tensors must be float64, got {t.dtype}")
        if t.device.index != hctx.device_id:
            raise ValueError(f"{name}: on {t.device}, but the library's context is on cuda:{hctx.device_id} "
                             f"(set {_device_env()} to choose it)")
        if t.shape != shape:
            raise ValueError(f"{name}: shape {tuple(t.shape)} differs from {tuple(shape)}")
        t = t.detach().contiguous()
        if t.data_ptr() % 16:
            t = t.clone()
        out.append(t)
    return hctx, out


def _device_env():
    from .registry import HIP_DEVICE_ENV

    return HIP_DEVICE_ENV


def _device_launch(hctx, launch):
    """`launch()` ordered on torch's current stream: the compute stream waits for it before, and it waits for the compute stream
    after - so the inputs are ready when the kernel starts and torch's caching allocator cannot hand an input or output to a later
    op before the kernel is done with it."""
    s = torch.cuda.current_stream().cuda_stream
    hctx.wait_for_stream(s)
    launch()
    hctx.stream_wait_for_ctx(s)


def _device_forward(fn_ctx, kind, dyn, q, qd, x, g, Ftip):
    model = dyn._derivative_model(f"autograd.{kind}_dynamics")
    hctx, (a, b, c) = _device_rows((q, qd, x), ("q", "qd", "qdd" if kind == "inverse" else "tau"))
    n = model.n
    if a.shape[-1] != n or a.dim() not in (1, 2):
        raise ValueError(f"q must be ({n},) or (rows, {n}), got {tuple(a.shape)}")
    rows = a.numel() // n
    out = torch.empty_like(a)
    if kind == "inverse":
        _device_launch(hctx, lambda: hctx.id_trajectory(model, a.data_ptr(), b.data_ptr(), c.data_ptr(), rows, out.data_ptr(), g, Ftip,
                                                        dtype=np.float64))
    else:
        _device_launch(hctx, lambda: hctx.forward_dynamics(model, a.data_ptr(), b.data_ptr(), c.data_ptr(), rows, out.data_ptr(), g,
                                                           Ftip, dtype=np.float64))
    fn_ctx.save_for_backward(q, qd, x)
    fn_ctx.device, fn_ctx.model, fn_ctx.consts = True, model, (g, Ftip)
    return out


def _device_backward(fn_ctx, kind, gy):
    q, qd, x = fn_ctx.saved_tensors
    g, Ftip = fn_ctx.consts
    model = fn_ctx.model
    hctx, (a, b, c, cot) = _device_rows((q, qd, x, gy.to(torch.float64)), ("q", "qd", "x", "cotangent"))
    rows = a.numel() // model.n
    gq, gqd = torch.empty_like(a), torch.empty_like(a)
    gx = torch.empty_like(a) if fn_ctx.needs_input_grad[3] else None
    p = (lambda t: None if t is None else t.data_ptr())  # noqa: E731
    if kind == "inverse":
        launch = lambda: hctx.id_vjp(model, a.data_ptr(), b.data_ptr(), c.data_ptr(), cot.data_ptr(), rows, gq.data_ptr(),  # noqa: E731
                                     gqd.data_ptr(), p(gx), g, Ftip)
    else:
        launch = lambda: hctx.fd_vjp(model, a.data_ptr(), b.data_ptr(), c.data_ptr(), cot.data_ptr(), rows, gq.data_ptr(),  # noqa: E731
                                     gqd.data_ptr(), None, p(gx), g, Ftip)
    _device_launch(hctx, launch)
    return None, gq, gqd, gx, None, None


class _InverseDynamics(torch.autograd.Function):
    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gtau):
        if ctx.device:
            return _device_backward(ctx, "inverse", gtau)
        dq, dqd, M = ctx.jac
        return None, _vjp(gtau, dq, ctx.one), _vjp(gtau, dqd, ctx.one), _vjp(gtau, M, ctx.one), None, None

    @staticmethod
    def forward(ctx, dyn, q, qd, qdd, g, Ftip):
        if _on_device(q, qd, qdd):
            return _device_forward(ctx, "inverse", dyn, q, qd, qdd, g, Ftip)
        ctx.device = False
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
        if ctx.device:
            return _device_backward(ctx, "forward", gqdd)
        dq, dqd, Minv = ctx.jac
        return None, _vjp(gqdd, dq, ctx.one), _vjp(gqdd, dqd, ctx.one), _vjp(gqdd, Minv, ctx.one), None, None

    @staticmethod
    def forward(ctx, dyn, q, qd, tau, g, Ftip):
        if _on_device(q, qd, tau):
            return _device_forward(ctx, "forward", dyn, q, qd, tau, g, Ftip)
        ctx.device = False
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
    (n,) inputs give (n,), (rows, n) inputs (rows, n); one g / Ftip for every row.  CPU float64 tensors, or ROCm float64 tensors on
    the library context's device (computed there, module docstring); a device g / Ftip is copied to the host."""
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


class _FkJacobian(torch.autograd.Function):
    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gT, gJ):
        if not ctx.needs_input_grad[1] or (gT is None and gJ is None):
            return None, None, None
        (q,) = ctx.saved_tensors
        model, frame = ctx.model, ctx.frame
        if ctx.device:
            hctx, (a,) = _device_rows((q,), ("q",))
            cot = [None if c is None else _device_rows((c.to(torch.float64),), (name,))[1][0] for c, name in ((gT, "gT"), (gJ, "gJ"))]
            gq = torch.empty_like(a)
            p = (lambda t: None if t is None else t.data_ptr())  # noqa: E731
            _device_launch(hctx, lambda: hctx.fk_jac_vjp(model, frame, a.data_ptr(), p(cot[0]), p(cot[1]), a.numel() // model.n,
                                                         None, None, gq.data_ptr()))
            return None, gq, None
        rows = q.numel() // model.n
        cT, cJ = (None if c is None else np.ascontiguousarray(c.detach().cpu().numpy(), dtype=np.float64).reshape(rows, *tail)
                  for c, tail in ((gT, (4, 4)), (gJ, (6, model.n))))
        _, _, gq = execute_registered_kernel("kinematics.fk_jacobian_vjp", model, _rows(q, "q"), cT, cJ, frame)
        return None, torch.from_numpy(gq.reshape(q.shape)), None

    @staticmethod
    def forward(ctx, sm, q, frame):
        model = sm._gradient_model(q.shape[-1] if q.dim() else 0, frame, "autograd.fk_jacobian")
        n = model.n
        if q.dim() not in (1, 2):
            raise ValueError(f"q must be ({n},) or (rows, {n}), got {tuple(q.shape)}")
        ctx.set_materialize_grads(False)
        ctx.model, ctx.frame = model, frame
        lead = tuple(q.shape[:-1])
        if _on_device(q):
            hctx, (a,) = _device_rows((q,), ("q",))
            T = a.new_empty(lead + (4, 4))
            J = a.new_empty(lead + (6, n))
            _device_launch(hctx, lambda: hctx.fk_jac_vjp(model, frame, a.data_ptr(), None, None, a.numel() // n, T.data_ptr(),
                                                         J.data_ptr(), None))
            ctx.device = True
        else:
            T, J, _ = execute_registered_kernel("kinematics.fk_jacobian_vjp", model, _rows(q, "q"), None, None, frame, want_T=True,
                                                want_J=True, want_gq=False)
            T, J = torch.from_numpy(T.reshape(lead + (4, 4))), torch.from_numpy(J.reshape(lead + (6, n)))
            ctx.device = False
        ctx.save_for_backward(q)
        return T, J


def fk_jacobian(sm, q, frame: str = "space"):
    """(T, J): the end-effector pose (4, 4) and the Jacobian (6, n) in `frame` of a SerialManipulator (or ManipulatorDynamics) with at
    most 8 joints, differentiable in q; (rows, 4, 4) / (rows, 6, n) for (rows, n) joint values.  CPU float64 tensors, or ROCm float64
    tensors on the library context's device (computed there, module docstring)."""
    return _FkJacobian.apply(sm, _as_tensor(q), frame)


def forward_kinematics(sm, q, frame: str = "space") -> torch.Tensor:
    """T of fk_jacobian: SerialManipulator.forward_kinematics(q, frame), differentiable in q."""
    return fk_jacobian(sm, q, frame)[0]


def jacobian(sm, q, frame: str = "space") -> torch.Tensor:
    """J of fk_jacobian: SerialManipulator.jacobian(q, frame), differentiable in q."""
    return fk_jacobian(sm, q, frame)[1]


class _CollisionCost(torch.autograd.Function):
    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gcost):
        if gcost is None or not ctx.needs_input_grad[1]:
            return None, None, None, None
        (grad,) = ctx.saved_tensors
        return None, grad * gcost.to(grad.dtype).unsqueeze(-1), None, None

    @staticmethod
    def forward(ctx, cm, q, eps_world, eps_self):
        n = cm.n
        if q.dim() not in (1, 2, 3) or q.shape[-1] != n:
            raise ValueError(f"q must be ({n},), (rows, {n}) or (B, N, {n}), got {tuple(q.shape)}")
        lead = tuple(q.shape[:-1])
        if _on_device(q):
            hctx, (a,) = _device_rows((q,), ("q",))
            cm.sync_world(hctx)
            cost, grad = a.new_empty(lead), torch.empty_like(a)
            _device_launch(hctx, lambda: hctx.collision(cm.model, cm.handle, a.data_ptr(), a.numel() // n, eps_world, eps_self,
                                                        d_cost=cost.data_ptr(), d_grad=grad.data_ptr()))
        else:
            r = execute_registered_kernel("planning.collision_spheres", cm, _rows(q, "q").reshape(-1, n), eps_world, eps_self,
                                          ("cost", "grad"))
            cost, grad = torch.from_numpy(r["cost"].reshape(lead)), torch.from_numpy(r["grad"].reshape(lead + (n,)))
        ctx.save_for_backward(grad)
        return cost


def collision_cost(model, q, eps_world: float, eps_self: float) -> torch.Tensor:
    """The hinge collision cost of a collision.SphereCollisionModel at q ((n,), (rows, n) or (B, N, n)), one value a row,
    differentiable in q: the backward pass is the kernel's own gradient times the incoming cotangent.  CPU float64 tensors, or ROCm
    float64 tensors on the library context's device (computed there on torch's current stream, module docstring).  Once
    differentiable: a second derivative is not provided and asking for one raises."""
    return _CollisionCost.apply(model, _as_tensor(q), float(eps_world), float(eps_self))
