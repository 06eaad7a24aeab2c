"""The float32 forward-dynamics template (csrc/mp_core.h mp_forward_dynamics: bias recursion + CRBA + float32 Cholesky) built for
the host, against a float64 reference that shares none of its code (oracle/oracle.c, and oracle/newton_euler.py past 8 joints).

Two bounds, the same ones tests/test_gpu_row_dynamics.py holds the kernels to (include/manipula_hip.h, mp_forward_dynamics_f32):
  forward   max|qdd - qdd_ref| <= 1e-4 * max|qdd_ref|  per row, on the four suite arms (M's condition number reaches ~3e4 there);
  backward  max|M_ref qdd - (tau - bias_ref)| <= 1e-5 * (max|M_ref| max|qdd| + max|tau| + max|bias_ref|)  per row, on any chain:
            a badly conditioned random chain amplifies float32 rounding by cond(M) in qdd, not in the torque it balances.
The float32 inputs are rounded to float32 first and the reference sees those same values in float64."""
import numpy as np
import pytest

from conftest import ROBOTS
from oracle import c_oracle
from oracle import newton_euler as ne
from oracle import ref_numpy as ref
from test_host_logic import hostsim  # noqa: F401  (fixture: clang++ build of the device templates)
from test_random_robots import FLAVOURS, random_robot

FWD_F32 = 1e-4   # forward bound of the float32 entry on the suite arms
BWD_F32 = 1e-5   # backward bound of the float32 entry on any chain
G_ALT = np.array([0.4, -0.3, -9.81])
F_ALT = np.array([1.0, -2.0, 0.5, 3.0, -1.5, 0.75])


def prismatic(tab):
    return np.abs(tab.S[:3]).sum(axis=0) == 0


def fd_rows(rng, tab, rows, suite):
    """(q, qd, tau) float64 rows already rounded to float32: inside the joint limits on a suite arm, +-2 rad (+-0.2 m on a
    prismatic joint) on a random chain."""
    n = tab.n
    if suite:
        q = rng.uniform(tab.joint_limits[:, 0], tab.joint_limits[:, 1], (rows, n))
    else:
        q = rng.uniform(-2.0, 2.0, (rows, n))
        q[:, prismatic(tab)] *= 0.1
    qd = rng.uniform(-2.0, 2.0, (rows, n))
    tau = rng.uniform(-10.0, 10.0, (rows, n))
    return tuple(a.astype(np.float32).astype(np.float64) for a in (q, qd, tau))


class Reference:
    """M_ref and bias_ref = ID(q, qd, 0, g, F) of float64 rows, and qdd_ref = solve(M_ref, tau - bias_ref), on every row (or on the
    rows listed in `sample`).  Up to 8 joints the C oracle evaluates them; past that the exact Newton-Euler oracle
    (oracle/newton_euler.py, pinned by tests/test_newton_euler_oracle.py; its float64 differs from its longdouble by 4e-14 at most in
    forward dynamics on these chains), in blocks of rows so that the n recursions of a block's mass matrices stay small."""
    BLOCK = 64

    def __init__(self, tab, q, qd, sample=None):
        self.tab, self.n = tab, tab.n
        self.idx = np.arange(len(q)) if sample is None else np.asarray(sample)
        self.q, self.qd = q[self.idx], qd[self.idx]
        if self.n <= 8:
            self.M = c_oracle.mass_matrix_rows(tab, self.q)
        else:
            self.M = np.concatenate([ne.mass_matrix(tab, self.q[i:i + self.BLOCK]) for i in range(0, len(self.q), self.BLOCK)])

    def bias(self, g=None, F=None):
        g = ref.G_DEFAULT if g is None else np.asarray(g, dtype=np.float64)
        F = np.zeros(6) if F is None else np.asarray(F, dtype=np.float64)
        if self.n <= 8:
            return c_oracle.inverse_dynamics_rows(self.tab, self.q, self.qd, np.zeros_like(self.q), g, F)[0]
        return ne.inverse_dynamics(self.tab, self.q, self.qd, np.zeros_like(self.q), g, F)

    def qdd(self, tau, g=None, F=None):
        return np.linalg.solve(self.M, (tau[self.idx] - self.bias(g, F))[..., None])[..., 0]


def forward_ratio(got, want, bound=FWD_F32):
    """Worst per-row max|got - want| / (bound * max|want|): <= 1 passes."""
    err = np.abs(got - want).max(axis=1)
    return float((err / (bound * np.abs(want).max(axis=1))).max())


def backward_ratio(M, qdd, rhs, bias, tau, bound=BWD_F32):
    """Worst per-row max|M qdd - rhs| / (bound * (max|M| max|qdd| + max|tau| + max|bias|)): <= 1 passes."""
    res = np.abs(np.einsum("rij,rj->ri", M, qdd) - rhs).max(axis=1)
    scale = np.abs(M).max(axis=(1, 2)) * np.abs(qdd).max(axis=1) + np.abs(tau).max(axis=1) + np.abs(bias).max(axis=1)
    return float((res / (bound * scale)).max())


def f64_ratio(got, want):
    """Worst |got - want| / (1e-6 |want| + 1e-7 max|want row|), the suite's float64 rule with the row's scale: <= 1 passes."""
    tol = 1e-6 * np.abs(want) + 1e-7 * np.abs(want).max(axis=1, keepdims=True) + 1e-300
    return float((np.abs(got - want) / tol).max())


def random_chain(n, seed):
    rng = np.random.default_rng(4400 + 31 * n + seed)
    return rng, random_robot(rng, n, FLAVOURS[(n + seed) % len(FLAVOURS)])


@pytest.mark.parametrize("robot", ROBOTS)
def test_float32_forward_dynamics_template_on_the_suite_arms(robot, tables, hostsim):  # noqa: F811
    tab = tables[robot]
    rng = np.random.default_rng(90 + ROBOTS.index(robot))
    q, qd, tau = fd_rows(rng, tab, 500, suite=True)
    R = Reference(tab, q, qd)
    for g, F in ((None, None), (G_ALT, F_ALT)):
        gg = ref.G_DEFAULT if g is None else g
        got = hostsim.fd(tab, 1, len(q), q, qd, tau, gg, np.zeros(6) if F is None else F, f32=1, outshape=q.shape)
        want = R.qdd(tau, g, F)
        assert forward_ratio(got, want) <= 1.0, (robot, g is None, forward_ratio(got, want))
        bias = R.bias(g, F)
        assert backward_ratio(R.M, got, tau - bias, bias, tau) <= 1.0
        # and the float64 instantiation of the same template at the suite's float64 rule
        got64 = hostsim.fd(tab, 1, len(q), q, qd, tau, gg, np.zeros(6) if F is None else F, f32=0, outshape=q.shape)
        assert f64_ratio(got64, want) <= 1.0, f64_ratio(got64, want)


@pytest.mark.parametrize("n", range(1, 9))
def test_float32_forward_dynamics_template_on_random_chains(n, hostsim):  # noqa: F811
    """Five chains per joint count, every flavour of tests/test_random_robots (prismatic joints included): the backward bound."""
    worst = 0.0
    for seed in range(5):
        rng, tab = random_chain(n, seed)
        q, qd, tau = fd_rows(rng, tab, 200, suite=False)
        R = Reference(tab, q, qd)
        for g, F in ((None, None), (G_ALT, F_ALT)):
            gg = ref.G_DEFAULT if g is None else g
            got = hostsim.fd(tab, 1, len(q), q, qd, tau, gg, np.zeros(6) if F is None else F, f32=1, outshape=q.shape)
            assert np.isfinite(got).all()
            bias = R.bias(g, F)
            worst = max(worst, backward_ratio(R.M, got, tau - bias, bias, tau))
    assert worst <= 1.0, worst
