#!/usr/bin/env python3
"""Generate tests/golden/regressor.npz by IMPORTING the reference (ManipulaPy v1.4.1).

    PYTHONHASHSEED=0 python tests/golden/make_golden_regressor.py

Runs only where the reference is importable (the build container); the fixture it writes holds numbers only.  Like
make_golden_rollout_grad.py it puts a throw-away `numba` stub on the path and pins PYTHONHASHSEED=0 (by running itself again as a
child process with that environment).

For each robot (UR5, xArm6, Panda, iiwa14) six rows of (q, qd, qdd, g, Ftip) are evaluated by the reference's own
ManipulatorDynamics.inverse_dynamics at the nominal model and at three perturbed ones:

    mass    every link mass scaled by a factor in [0.8, 1.25]
    inertia every Ic replaced by L Ic L^T, L = 1 + 0.15 U(-1, 1)^(3x3) (symmetric positive definite), masses scaled as well
    com     every centre of mass moved by up to 5 cm along its own CoM-frame axes: Mlist_per_link[i] translated by c_i,
            Glist[i] = blockdiag(Ic_i, m_i 1) unchanged

Every case stores the public-convention inertial parameters pi (n, 10) [m, hx, hy, hz, Ixx, Ixy, Ixz, Iyy, Iyz, Izz] in the NOMINAL
CoM frames (h = m c, I about the nominal frame's origin) and the reference's torques.  tau is linear in pi, so these torques pin
the regressor Y and the frame map D independently of the code under test.

    <robot>_q, <robot>_qd, <robot>_qdd (rows, n)   <robot>_g (rows, 3)   <robot>_Ftip (rows, 6)
    <robot>_<case>_pi (n, 10)   <robot>_<case>_tau (rows, n)            case in nominal, mass, inertia, com

Autograd Jacobians d tau / d m_i, d tau / d Ic_i are not stored and not attempted (whether the reference's torch backend keeps a
graph through Glist was not established here): the perturbed cases above pin the same derivatives, exactly, through the linearity
of tau in pi.
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
SEED = 20261016
ROBOTS = ("ur5", "xarm6", "panda", "iiwa14")
ROWS = 6


def _run_pinned() -> None:
    stub = tempfile.mkdtemp(prefix="mp_numba_stub_")
    os.makedirs(os.path.join(stub, "numba"))
    with open(os.path.join(stub, "numba", "__init__.py"), "w") as f:
        f.write(NUMBA_STUB)
    env = dict(os.environ)
    env.update(_MP_GOLDEN_CHILD="1", PYTHONHASHSEED="0", NUMBA_DISABLE_CUDA="1", MPLBACKEND="Agg", MANIPULAPY_QUIET="1",
               PYTHONPATH=os.pathsep.join([stub, REF, env.get("PYTHONPATH", "")]))
    sys.exit(subprocess.run([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env).returncode)


def _pi(m, c, Ic):
    """public parameters in the nominal CoM frame of a link whose centre of mass sits at c in it, Ic about the centre of mass"""
    import numpy as np

    I = Ic + m * (np.dot(c, c) * np.eye(3) - np.outer(c, c))
    h = m * c
    return np.array([m, h[0], h[1], h[2], I[0, 0], I[0, 1], I[0, 2], I[1, 1], I[1, 2], I[2, 2]])


def main() -> None:
    import warnings

    import numpy as np

    warnings.simplefilter("ignore")
    from ManipulaPy.dynamics import ManipulatorDynamics
    from ManipulaPy.ManipulaPy_data import get_robot_urdf
    from ManipulaPy.urdf_processor import URDFToSerialManipulator

    rng = np.random.default_rng(SEED)
    out = {}
    for robot in ROBOTS:
        proc = URDFToSerialManipulator(get_robot_urdf(robot), load_meshes=False)
        dyn = proc.dynamics
        n = dyn.S_list.shape[1]
        G0 = [np.asarray(G, dtype=np.float64) for G in dyn.Glist]
        M0 = [np.asarray(M, dtype=np.float64) for M in dyn.Mlist_per_link]
        m0 = np.array([G[3, 3] for G in G0])
        Ic0 = [0.5 * (G[:3, :3] + G[:3, :3].T) for G in G0]
        q = rng.uniform(-1.5, 1.5, (ROWS, n))
        qd = rng.uniform(-1.0, 1.0, (ROWS, n))
        qdd = rng.uniform(-1.0, 1.0, (ROWS, n))
        g = np.tile([0.0, 0.0, -9.81], (ROWS, 1))
        g[1::2] = rng.uniform(-3.0, 3.0, (ROWS // 2, 3)) + [0.0, 0.0, -9.0]
        F = rng.uniform(-5.0, 5.0, (ROWS, 6))
        F[0] = 0.0
        out.update({f"{robot}_q": q, f"{robot}_qd": qd, f"{robot}_qdd": qdd, f"{robot}_g": g, f"{robot}_Ftip": F})

        s = rng.uniform(0.8, 1.25, n)
        L = [np.eye(3) + 0.15 * rng.uniform(-1.0, 1.0, (3, 3)) for _ in range(n)]
        cs = rng.uniform(-0.05, 0.05, (n, 3))
        cases = {
            "nominal": (m0, Ic0, np.zeros((n, 3))),
            "mass": (m0 * s, Ic0, np.zeros((n, 3))),
            "inertia": (m0 * s[::-1], [Li @ Ic @ Li.T for Li, Ic in zip(L, Ic0)], np.zeros((n, 3))),
            "com": (m0, Ic0, cs),
        }
        for case, (m, Ic, c) in cases.items():
            Gl, Ml = [], []
            for i in range(n):
                G = np.zeros((6, 6))
                G[:3, :3] = Ic[i]
                G[3:, 3:] = m[i] * np.eye(3)
                Gl.append(G)
                Mi = M0[i].copy()
                Mi[:3, 3] += Mi[:3, :3] @ c[i]
                Ml.append(Mi)
            d = ManipulatorDynamics(dyn.M_list, dyn.omega_list, dyn.r_list, dyn.b_list, dyn.S_list, dyn.B_list, Gl, Ml)
            tau = np.array([np.asarray(d.inverse_dynamics(q[r], qd[r], qdd[r], g[r], F[r]), dtype=np.float64) for r in range(ROWS)])
            out[f"{robot}_{case}_pi"] = np.array([_pi(m[i], c[i], Ic[i]) for i in range(n)])
            out[f"{robot}_{case}_tau"] = tau
        print(robot, "done", flush=True)
    np.savez(os.path.join(HERE, "regressor.npz"), **out)


if __name__ == "__main__":
    if os.environ.get("_MP_GOLDEN_CHILD") != "1":
        _run_pinned()
    main()
