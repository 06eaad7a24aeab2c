#!/usr/bin/env python3
"""Generate tests/golden/rollout_grad.npz by IMPORTING the reference (ManipulaPy v1.4.1) under its own torch backend.

    PYTHONHASHSEED=0 python tests/golden/make_golden_rollout_grad.py

Runs only where the reference is importable (the build container); the fixture it writes holds numbers only.  Like
make_golden_derivatives.py it puts a throw-away `numba` stub on the path and pins PYTHONHASHSEED=0 (by running itself again as a
child process with that environment).

For each case the reference planner's forward_dynamics_trajectory (OptimizedTrajectoryPlanning(use_cuda=False), whose CPU
roll-out is differentiable under the torch backend) runs on float64 tensors that require grad, and torch.autograd gives the
gradient of  L = <Gp, positions> + <Gv, velocities> + <Ga, accelerations>  with respect to theta0, dtheta0 and taumat.
The cotangents are multiples of 1/64 in [-1, 1]: exact in float32, so the float32 rows' cast does not round them.

    <case>_joint_limits (n,2)  <case>_theta0, <case>_dtheta0 (n)  <case>_taumat (N,n)  <case>_Ftipmat (N,6)  <case>_g (3)
    <case>_dt, <case>_intRes   <case>_Gp, <case>_Gv, <case>_Ga (N,n)
    <case>_positions, <case>_velocities, <case>_accelerations (N,n) float32    the reference's rows
    <case>_grad_theta0, <case>_grad_dtheta0 (n), <case>_grad_taumat (N,n)      float64

Cases: xarm6 with the inputs of fd_trajectory_xarm6.npz (N = 8, intRes 2, per-step wrench); UR5 with tight limits on three joints
so the clip engages on some sub-steps (N = 5, intRes 2); Panda (8 joints), N = 3, intRes 1.
"""
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
NUMBA_STUB = '''
def _ident(*a, **k):
    if len(a) == 1 and callable(a[0]) and not k:
        return a[0]
    return lambda f: f
njit = jit = vectorize = guvectorize = _ident
prange = range
class _Cfg: pass
config = _Cfg()
float32 = int32 = float64 = int64 = None
'''
SEED = 20260520


def _run_pinned() -> None:
    stub = tempfile.mkdtemp(prefix="mp_numba_stub_")
    os.makedirs(os.path.join(stub, "numba"))
    with open(os.path.join(stub, "numba", "__init__.py"), "w") as f:
        f.write(NUMBA_STUB)
    env = dict(os.environ)
    env.update(_MP_GOLDEN_CHILD="1", PYTHONHASHSEED="0", NUMBA_DISABLE_CUDA="1", MPLBACKEND="Agg", MANIPULAPY_QUIET="1",
               PYTHONPATH=os.pathsep.join([stub, REF, env.get("PYTHONPATH", "")]))
    sys.exit(subprocess.run([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env).returncode)


def _finite_limits(sm, n):
    import numpy as np

    lims = getattr(sm, "joint_limits", None) or [(None, None)] * n
    out = np.empty((n, 2))
    for i in range(n):
        lo, hi = lims[i] if i < len(lims) else (None, None)
        out[i, 0] = -np.pi if lo is None else float(lo)
        out[i, 1] = np.pi if hi is None else float(hi)
    return out


def main() -> None:
    import warnings

    import numpy as np
    import torch

    warnings.simplefilter("ignore")
    from ManipulaPy.backend import use_backend
    from ManipulaPy.ManipulaPy_data import get_robot_urdf
    from ManipulaPy.planning import OptimizedTrajectoryPlanning
    from ManipulaPy.urdf_processor import URDFToSerialManipulator

    rng = np.random.default_rng(SEED)
    cot = lambda shape: rng.integers(-64, 65, shape).astype(np.float64) / 64.0  # noqa: E731  (exact in float32)
    cases = {}

    x = np.load(os.path.join(HERE, "fd_trajectory_xarm6.npz"))
    cases["xarm6"] = dict(robot="xarm6", joint_limits=x["joint_limits"], theta0=x["theta0"], dtheta0=x["dtheta0"], taumat=x["taumat"],
                          Ftipmat=x["Ftipmat"], g=x["g"], dt=float(x["dt"]), intRes=int(x["intRes"]))

    proc = URDFToSerialManipulator(get_robot_urdf("ur5"), load_meshes=False)
    n = proc.serial_manipulator.S_list.shape[1]
    lims = _finite_limits(proc.serial_manipulator, n)
    th0 = rng.uniform(-0.3, 0.3, n)
    dth0 = rng.uniform(-0.3, 0.3, n)
    dth0[[0, 2, 4]] = [1.5, -1.5, 2.0]
    for j, side in ((0, 1), (2, 0), (4, 1)):  # a limit ~2.5 sub-steps of travel away (h = 0.005): the clip engages in step 2
        lims[j, side] = float(np.float32(th0[j] + (0.021 if side else -0.021)))
    N = 5
    cases["ur5_tight"] = dict(robot="ur5", joint_limits=lims, theta0=th0, dtheta0=dth0, taumat=rng.uniform(-2, 2, (N, n)),
                              Ftipmat=rng.uniform(-3, 3, (N, 6)), g=np.array([0.0, 0.0, -9.81]), dt=0.01, intRes=2)

    proc = URDFToSerialManipulator(get_robot_urdf("panda"), load_meshes=False)
    n = proc.serial_manipulator.S_list.shape[1]
    N = 3
    cases["panda"] = dict(robot="panda", joint_limits=_finite_limits(proc.serial_manipulator, n), theta0=rng.uniform(-0.5, 0.5, n),
                          dtheta0=rng.uniform(-0.3, 0.3, n), taumat=rng.uniform(-1, 1, (N, n)), Ftipmat=rng.uniform(-2, 2, (N, 6)),
                          g=np.array([0.0, 0.0, -9.81]), dt=0.01, intRes=1)

    out = {}
    for name, c in cases.items():
        proc = URDFToSerialManipulator(get_robot_urdf(c["robot"]), load_meshes=False)
        sm, dyn = proc.serial_manipulator, proc.dynamics
        planner = OptimizedTrajectoryPlanning(sm, get_robot_urdf(c["robot"]), dyn, c["joint_limits"].tolist(), use_cuda=False)
        N, n = c["taumat"].shape
        G = {k: cot((N, n)) for k in ("Gp", "Gv", "Ga")}
        dyn._mass_matrix_cache.clear()
        dyn._mass_matrix_derivative_cache.clear()
        with use_backend("torch"):
            T = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)  # noqa: E731
            th, dth, tm = T(c["theta0"]).requires_grad_(), T(c["dtheta0"]).requires_grad_(), T(c["taumat"]).requires_grad_()
            r = planner.forward_dynamics_trajectory(th, dth, tm, T(c["g"]), T(c["Ftipmat"]), c["dt"], c["intRes"])
            loss = ((r["positions"].double() * T(G["Gp"])).sum() + (r["velocities"].double() * T(G["Gv"])).sum() +
                    (r["accelerations"].double() * T(G["Ga"])).sum())
            loss.backward()
        for k in ("joint_limits", "theta0", "dtheta0", "taumat", "Ftipmat", "g"):
            out[f"{name}_{k}"] = np.asarray(c[k], dtype=np.float64)
        out[f"{name}_dt"], out[f"{name}_intRes"] = np.float64(c["dt"]), np.int64(c["intRes"])
        for k, v in G.items():
            out[f"{name}_{k}"] = v
        for k in ("positions", "velocities", "accelerations"):
            out[f"{name}_{k}"] = r[k].detach().numpy().astype(np.float32)
        out[f"{name}_grad_theta0"] = th.grad.numpy().copy()
        out[f"{name}_grad_dtheta0"] = dth.grad.numpy().copy()
        out[f"{name}_grad_taumat"] = tm.grad.numpy().copy()
        print(name, "done", flush=True)
    np.savez(os.path.join(HERE, "rollout_grad.npz"), **out)


if __name__ == "__main__":
    if os.environ.get("_MP_GOLDEN_CHILD") != "1":
        _run_pinned()
    main()
