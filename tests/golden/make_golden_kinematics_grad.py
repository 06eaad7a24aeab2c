#!/usr/bin/env python3
"""Generate tests/golden/kinematics_grad.npz by IMPORTING the reference (ManipulaPy v1.4.1) under its own torch backend.

    PYTHONHASHSEED=0 python tests/golden/make_golden_kinematics_grad.py

Runs only where the reference is importable (the build container); the fixture it writes holds numbers only.  Like
make_golden_derivatives.py it puts a throw-away `numba` stub on the path and pins PYTHONHASHSEED=0 (by running itself again as a
child process with that environment).  For every robot and the first 10 configurations of dynamics_<robot>.npz it stores the
reference's torch.autograd Jacobians

    <robot>_dT    of forward_kinematics(q)          (10, 4, 4, n)
    <robot>_dJs   of jacobian(q, frame="space")     (10, 6, n, n)
    <robot>_dJb   of jacobian(q, frame="body")      (10, 6, n, n)
[row, ..., j] = d out[...] / d q_j.
"""
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
ROBOTS = ["ur5", "iiwa14", "panda", "xarm6"]
ROWS = 10
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
    for robot in ROBOTS:
        sm = URDFToSerialManipulator(get_robot_urdf(robot), load_meshes=False).serial_manipulator
        z = np.load(os.path.join(HERE, f"dynamics_{robot}.npz"))
        acc = {"dT": [], "dJs": [], "dJb": []}
        for q in z["thetas"][:ROWS]:
            x = torch.tensor(np.asarray(q), dtype=torch.float64)
            with use_backend("torch"):
                acc["dT"].append(torch.autograd.functional.jacobian(lambda v: sm.forward_kinematics(v), x))
                acc["dJs"].append(torch.autograd.functional.jacobian(lambda v: sm.jacobian(v, frame="space"), x))
                acc["dJb"].append(torch.autograd.functional.jacobian(lambda v: sm.jacobian(v, frame="body"), x))
        for k, v in acc.items():
            out[f"{robot}_{k}"] = np.array([t.detach().numpy() for t in v], dtype=np.float64)
        print(robot, "done", flush=True)
    np.savez(os.path.join(HERE, "kinematics_grad.npz"), **out)


if __name__ == "__main__":
    if os.environ.get("_MP_GOLDEN_CHILD") != "1":
        _run_pinned()
    main()
