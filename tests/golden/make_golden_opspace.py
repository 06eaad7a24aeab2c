#!/usr/bin/env python3
"""Generate tests/golden/opspace.npz by IMPORTING the reference (ManipulaPy v1.4.1).

    PYTHONHASHSEED=0 python tests/golden/make_golden_opspace.py

Runs only where the reference is importable (the build container); the fixture it writes holds numbers only.  Like
make_golden_kinematics_grad.py it puts a throw-away `numba` stub on the path and pins PYTHONHASHSEED=0.  For every robot and the 21
seeded rows 4..24 of dynamics_<robot>.npz (thetas, dthetas, g) it stores what the reference computes

    <robot>_T, _Js, _Jb     forward_kinematics(q), jacobian(q, "space" / "body")
    <robot>_M, _c, _g       mass_matrix(q), velocity_quadratic_forces(q, qd), gravity_forces(q, g)
    <robot>_Jdqd_s, _Jdqd_b torch.autograd's dJ/dq of jacobian(q, frame) contracted twice with qd

and what NumPy forms from those for frame f in (space, body, hybrid) and task t in (full, linear, angular), key <robot>_<f>_<t>_*:
J, Jdqd, A = J M^-1 J^T, Lambda = A^-1, Jbar = M^-1 J^T Lambda, mu = Lambda (J M^-1 c - Jdqd), p = Lambda J M^-1 g, cond = cond_2(A).
The hybrid frame: J_h = blkdiag(R, R) J_b, Jdot_h qd = blkdiag(R, R) Jdot_b qd + blkdiag([w]x R, [w]x R) J_b qd, w = R w_b.
"""
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
ROBOTS = ["ur5", "iiwa14", "panda", "xarm6"]
ROWS = slice(4, 25)  # rows 0..3 of dynamics_<robot>.npz are the zero and joint-limit poses: singular
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


def _skew(w):
    return [[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]]


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
        proc = URDFToSerialManipulator(get_robot_urdf(robot), load_meshes=False)
        sm, dyn = proc.serial_manipulator, proc.dynamics
        z = np.load(os.path.join(HERE, f"dynamics_{robot}.npz"))
        g = z["g"]
        acc = {}

        def put(key, value):
            acc.setdefault(key, []).append(np.asarray(value, dtype=np.float64))

        for q, qd in zip(z["thetas"][ROWS], z["dthetas"][ROWS]):
            dyn._mass_matrix_cache.clear()
            T = np.asarray(sm.forward_kinematics(q), dtype=np.float64)
            Js = np.asarray(sm.jacobian(q, frame="space"), dtype=np.float64)
            Jb = np.asarray(sm.jacobian(q, frame="body"), dtype=np.float64)
            M = np.asarray(dyn.mass_matrix(q), dtype=np.float64)
            c = np.asarray(dyn.velocity_quadratic_forces(q, qd), dtype=np.float64)
            gv = np.asarray(dyn.gravity_forces(q, g), dtype=np.float64)
            x = torch.tensor(np.asarray(q), dtype=torch.float64)
            with use_backend("torch"):
                dJs = torch.autograd.functional.jacobian(lambda v: sm.jacobian(v, frame="space"), x).detach().numpy()
                dJb = torch.autograd.functional.jacobian(lambda v: sm.jacobian(v, frame="body"), x).detach().numpy()
            jd_s, jd_b = np.einsum("aij,i,j->a", dJs, qd, qd), np.einsum("aij,i,j->a", dJb, qd, qd)
            for k, v in (("T", T), ("Js", Js), ("Jb", Jb), ("M", M), ("c", c), ("g", gv), ("Jdqd_s", jd_s), ("Jdqd_b", jd_b)):
                put(k, v)
            R = T[:3, :3]
            RR = np.zeros((6, 6))
            RR[:3, :3] = RR[3:, 3:] = R
            w = R @ (Jb @ qd)[:3]
            WR = np.zeros((6, 6))
            WR[:3, :3] = WR[3:, 3:] = np.asarray(_skew(w)) @ R
            frames = {"space": (Js, jd_s), "body": (Jb, jd_b), "hybrid": (RR @ Jb, RR @ jd_b + WR @ (Jb @ qd))}
            Minv = np.linalg.inv(M)
            for f, (J6, jd6) in frames.items():
                for t, sel in (("full", slice(0, 6)), ("linear", slice(3, 6)), ("angular", slice(0, 3))):
                    J, jd = J6[sel], jd6[sel]
                    A = J @ Minv @ J.T
                    Lam = np.linalg.inv(A)
                    pre = f"{f}_{t}_"
                    put(pre + "J", J)
                    put(pre + "Jdqd", jd)
                    put(pre + "A", A)
                    put(pre + "Lambda", Lam)
                    put(pre + "Jbar", Minv @ J.T @ Lam)
                    put(pre + "mu", Lam @ (J @ Minv @ c - jd))
                    put(pre + "p", Lam @ (J @ Minv @ gv))
                    put(pre + "cond", np.linalg.cond(A))
        for k, v in acc.items():
            out[f"{robot}_{k}"] = np.array(v, dtype=np.float64)
        print(robot, "done, worst cond(A) body/full %.3g" % out[f"{robot}_body_full_cond"].max(), flush=True)
    np.savez_compressed(os.path.join(HERE, "opspace.npz"), **out)


if __name__ == "__main__":
    if os.environ.get("_MP_GOLDEN_CHILD") != "1":
        _run_pinned()
    main()
