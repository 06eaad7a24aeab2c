#!/usr/bin/env python3
"""Generate tests/golden/derivatives.npz by IMPORTING the reference (ManipulaPy v1.4.1) under its own torch backend.

    PYTHONHASHSEED=0 python tests/golden/make_golden_derivatives.py

Runs only where the reference is importable (the build container); the fixture it writes holds numbers only.  Like
make_golden.py it puts a throw-away `numba` stub on the path and pins PYTHONHASHSEED=0 (here by running itself again as a child
process with that environment).  For every robot and every configuration of dynamics_<robot>.npz (25 rows: nonzero qd, random
Ftip) it stores the reference's torch.autograd Jacobians

    <robot>_id_dq, <robot>_id_dqd, <robot>_id_dqdd      of inverse_dynamics(q, qd, qdd, g, Ftip)
    <robot>_fd_dq, <robot>_fd_dqd, <robot>_fd_dtau      of forward_dynamics(q, qd, tau, g, Ftip), tau = the fixture's
                                                        inverse_dynamics of the same row
each (25, n, n), [row, i, j] = d out_i / d in_j.
"""
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
ROBOTS = ["ur5", "iiwa14", "panda", "xarm6"]
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


def _run_pinned() -> None:
    stub = tempfile.mkdtemp(prefix="mp_numba_stub_")
    os.makedirs(os.path.join(stub, "numba"))
    with open(os.path.join(stub, "numba", "__init__.py"), "w") as f:
        f.write(NUMBA_STUB)
    env = dict(os.environ)
    env.update(_MP_GOLDEN_CHILD="1", PYTHONHASHSEED="0", NUMBA_DISABLE_CUDA="1", MPLBACKEND="Agg", MANIPULAPY_QUIET="1",
               PYTHONPATH=os.pathsep.join([stub, REF, env.get("PYTHONPATH", "")]))
    sys.exit(subprocess.run([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env).returncode)


def main() -> None:
    import warnings

    import numpy as np
    import torch

    warnings.simplefilter("ignore")
    from ManipulaPy.backend import use_backend
    from ManipulaPy.ManipulaPy_data import get_robot_urdf
    from ManipulaPy.urdf_processor import URDFToSerialManipulator

    out = {}
    T = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)  # noqa: E731
    for robot in ROBOTS:
        dyn = URDFToSerialManipulator(get_robot_urdf(robot), load_meshes=False).dynamics
        z = np.load(os.path.join(HERE, f"dynamics_{robot}.npz"))
        g = z["g"]
        acc = {k: [] for k in ("id_dq", "id_dqd", "id_dqdd", "fd_dq", "fd_dqd", "fd_dtau")}
        for i in range(z["thetas"].shape[0]):
            q, qd, qdd, F, tau = z["thetas"][i], z["dthetas"][i], z["ddthetas"][i], z["ftips"][i], z["inverse_dynamics"][i]
            dyn._mass_matrix_cache.clear()
            dyn._mass_matrix_derivative_cache.clear()
            with use_backend("torch"):
                fid = lambda a, b, c: dyn.inverse_dynamics(a, b, c, T(g), T(F))  # noqa: E731
                ffd = lambda a, b, c: dyn.forward_dynamics(a, b, c, T(g), T(F))  # noqa: E731
                jid = torch.autograd.functional.jacobian(fid, (T(q), T(qd), T(qdd)))
                jfd = torch.autograd.functional.jacobian(ffd, (T(q), T(qd), T(tau)))
            for k, v in zip(("id_dq", "id_dqd", "id_dqdd"), jid):
                acc[k].append(v.detach().numpy())
            for k, v in zip(("fd_dq", "fd_dqd", "fd_dtau"), jfd):
                acc[k].append(v.detach().numpy())
        for k, v in acc.items():
            out[f"{robot}_{k}"] = np.array(v, dtype=np.float64)
        print(robot, "done", flush=True)
    np.savez(os.path.join(HERE, "derivatives.npz"), **out)


if __name__ == "__main__":
    if os.environ.get("_MP_GOLDEN_CHILD") != "1":
        _run_pinned()
    main()
