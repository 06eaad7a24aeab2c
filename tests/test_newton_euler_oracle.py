"""Pins oracle/newton_euler.py (the exact Newton-Euler oracle the 9..32-joint tests are held to):
  1. the reference's fixtures tests/golden/dynamics_{ur5,panda,xarm6,iiwa14}.npz - mass matrix, inverse dynamics with a tip wrench,
     forward dynamics - at the tolerances tests/test_oracle_golden.py holds oracle/ref_numpy.py to;
  2. ref_numpy on random chains of 1..8 joints, every flavour of test_random_robots.FLAVOURS (prismatic joints included), at
     ref_numpy's own central-difference noise: 1e-9 of max|tau|;
  3. itself in longdouble, on the chains of 9..32 joints that tests/dyn_cases.py uses.  These float64-against-longdouble figures are
     printed (pytest -s): the bounds of dyn_cases.py are 100 x figures of this kind, measured there on the lanes they apply to."""
import numpy as np
import pytest

from conftest import ROBOTS
from oracle import newton_euler as ne
from oracle import ref_numpy as ref
from test_random_robots import FLAVOURS, random_robot

RTOL = 1e-7   # tests/test_oracle_golden.py
GOLDEN_FD_ROWS = [0, 1, 2, 5, 9, 17, 24]   # tests/test_oracle_golden.py, test_generated_fixtures_dynamics
REF_NUMPY_NOISE = 1e-9   # of max|tau|: ref_numpy's velocity term is a central difference (eps 1e-6) of mass matrices


@pytest.mark.parametrize("robot", ROBOTS)
def test_against_the_reference_fixtures(robot, tables, dyn_golden):
    tab, z = tables[robot], dyn_golden[robot]
    th, dth, ddth, ft = z["thetas"], z["dthetas"], z["ddthetas"], z["ftips"]
    np.testing.assert_allclose(ne.mass_matrix(tab, th), z["mass_matrix"], rtol=RTOL, atol=1e-9)
    np.testing.assert_allclose(ne.inverse_dynamics(tab, th, dth, ddth, z["g"], ft), z["inverse_dynamics"], rtol=RTOL, atol=1e-8)
    # The fixture's forward dynamics inverts the fixture's own torques, which carry the reference's central-difference noise (~1e-8):
    # an exact solve of them sits noise x M^-1 from the fixture - up to 4.1e-7 on a wrist joint (ur5 row 7, xarm6 row 16), under 1e-7
    # on the rows tests/test_oracle_golden.py holds ref_numpy to.  Those rows at its tolerance; every row at the reference's 1e-5 and,
    # from the oracle's own torques, back to the accelerations at 1e-9.
    qdd = ne.forward_dynamics(tab, th, dth, z["inverse_dynamics"], z["g"], ft)
    np.testing.assert_allclose(qdd[GOLDEN_FD_ROWS], z["forward_dynamics"][GOLDEN_FD_ROWS], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(qdd, ddth, atol=1e-5)
    own = ne.forward_dynamics(tab, th, dth, ne.inverse_dynamics(tab, th, dth, ddth, z["g"], ft), z["g"], ft)
    np.testing.assert_allclose(own, ddth, rtol=0, atol=1e-9)
    np.testing.assert_array_equal(ne.inverse_dynamics(tab, th[3], dth[3], ddth[3], z["g"], ft[3]),     # a single row is a row
                                  ne.inverse_dynamics(tab, th[3:4], dth[3:4], ddth[3:4], z["g"], ft[3:4])[0])


def test_against_ref_numpy_on_every_flavour_of_chain():
    seen, worst = set(), 0.0
    for n in range(1, 9):
        for seed in range(2):
            k = (n + 4 * seed) % len(FLAVOURS)
            seen.add(k)
            rng = np.random.default_rng(6100 + 10 * n + seed)
            tab = random_robot(rng, n, FLAVOURS[k])
            rows = 2
            q = rng.uniform(-2.0, 2.0, (rows, n))
            q[:, np.abs(tab.S[:3]).sum(axis=0) == 0] *= 0.1
            qd, qdd = rng.uniform(-1, 1, (rows, n)), rng.uniform(-2, 2, (rows, n))
            g, F = np.array([0.4, -0.3, -9.81]), rng.uniform(-3, 3, 6)
            got = ne.inverse_dynamics(tab, q, qd, qdd, g, F)
            M = ne.mass_matrix(tab, q)
            for r in range(rows):
                want = ref.inverse_dynamics(tab, q[r], qd[r], qdd[r], g, F)
                worst = max(worst, float(np.abs(got[r] - want).max() / np.abs(want).max()))
                np.testing.assert_allclose(M[r], ref.mass_matrix(tab, q[r]), rtol=1e-12, atol=1e-13)
    assert seen == set(range(len(FLAVOURS)))
    print(f"\nnewton_euler vs ref_numpy, ID on chains of 1..8 joints: worst {worst:.2e} of max|tau| (bound {REF_NUMPY_NOISE})")
    assert worst <= REF_NUMPY_NOISE, worst


@pytest.mark.parametrize("n", [9, 14, 16, 17, 32])
def test_float64_against_longdouble(n):
    """The oracle's own rounding: float64 against longdouble, relative to max(1, scale), on the suite's chain 8800 + n.  Asserted at
    1e-12 (a factor ~25 over the largest figure seen, 4.2e-14 for forward dynamics at n = 16, cond(M) 3.5e3) so that a change that makes the
    oracle noisier is noticed; the figures themselves are printed."""
    rng = np.random.default_rng(8800 + n)
    tab = random_robot(rng, n, FLAVOURS[n % len(FLAVOURS)])
    rows = 4
    q = rng.uniform(-2.0, 2.0, (rows, n))
    q[:, np.abs(tab.S[:3]).sum(axis=0) == 0] *= 0.1
    qd, x = rng.uniform(-1, 1, (rows, n)), rng.uniform(-2, 2, (rows, n))
    g, F = np.array([0.4, -0.3, -9.81]), rng.uniform(-3, 3, 6)
    L = np.longdouble

    def rel(a, b):
        return float(np.abs(a - b).max() / max(1.0, float(np.abs(b).max())))

    fig = {"ID": rel(ne.inverse_dynamics(tab, q, qd, x, g, F), ne.inverse_dynamics(tab, q, qd, x, g, F, dtype=L)),
           "M": rel(ne.mass_matrix(tab, q), ne.mass_matrix(tab, q, dtype=L)),
           "FD": rel(ne.forward_dynamics(tab, q, qd, x, g, F), ne.forward_dynamics(tab, q, qd, x, g, F, dtype=L))}
    lim = np.tile([-2.5, 2.5], (n, 1))
    tm, Fm = rng.uniform(-1, 1, (rows, 6, n)), np.tile(F * 0.1, (rows, 6, 1))
    a = ne.fd_rollout(tab, q * 0.3, qd * 0.2, tm, g, Fm, 1e-3, 2, lim)
    b = ne.fd_rollout(tab, q * 0.3, qd * 0.2, tm, g, Fm, 1e-3, 2, lim, dtype=L)
    for key in ("positions", "velocities", "accelerations"):
        fig["roll-out " + key[:3]] = rel(a[key], b[key])
    cond = float(np.linalg.cond(ne.mass_matrix(tab, q)).max())
    print(f"\nn = {n}: float64 vs longdouble " + ", ".join(f"{k} {v:.1e}" for k, v in fig.items()) + f"; cond(M) up to {cond:.0f}")
    assert max(fig.values()) <= 1e-12, fig
    assert ne.inverse_dynamics(tab, q, qd, x, g, F, dtype=np.float32).dtype == np.float32       # float32 stays float32 throughout


def test_rollout_is_the_reference_loop():
    """fd_rollout against ref_numpy.forward_dynamics_trajectory on a 5-joint chain with a limit that engages: same loop, same clip
    (limits rounded to float32), same recorded acceleration; ref_numpy's forward dynamics carries its difference noise (1e-6 here)."""
    rng = np.random.default_rng(6200)
    tab = random_robot(rng, 5, FLAVOURS[5])
    q0, qd0 = rng.uniform(-0.3, 0.3, 5), rng.uniform(-0.5, 0.5, 5)
    lim = np.tile([-2.5, 2.5], (5, 1))
    lim[2] = [q0[2] - 0.0013, q0[2] + 0.0007]
    tm, Fm = rng.uniform(-2, 2, (6, 5)), rng.uniform(-1, 1, (6, 6))
    g = np.array([0.4, -0.3, -9.81])
    want = ref.forward_dynamics_trajectory(tab, q0, qd0, tm, g, Fm, 0.004, 2, joint_limits=lim)
    got = ne.fd_rollout(tab, q0[None], qd0[None], tm[None], g, Fm[None], 0.002, 2, lim)
    l32 = lim.astype(np.float32).astype(np.float64)
    assert (got["positions"][0, 1:, 2] == l32[2, 0]).any() or (got["positions"][0, 1:, 2] == l32[2, 1]).any()
    for key in ("positions", "velocities", "accelerations"):
        np.testing.assert_allclose(got[key][0], want[key], rtol=0, atol=1e-6 * max(1.0, float(np.abs(want[key]).max())))
    assert (got["accelerations"][0, 0] == 0).all()
