"""Shared by test_opspace_host.py and test_gpu_opspace.py: the comparison rules of the operational-space operators.

T, J and Jdot qd follow the project's float64 rules (1e-10 scale against the CPU twin, 1e-6 |ref| + 1e-7 scale against a fixture).  The
Lambda-dependent outputs (Lambda, Jbar, mu, p, tau) inherit the conditioning of A = J M^-1 J^T + damping^2 1, which mixes rad and m and
a light wrist: they are held to max(floor, 32 eps kappa) scale, kappa = cond_2(A) - the c eps kappa bound of two Cholesky solves with
c = 32 for m <= 6.  Rows with kappa > 1e10 are left out of the Lambda-dependent comparison only; callers assert how many that may be.
scale = max(1, largest |reference value| of the row)."""
import numpy as np

EPS = 2.0 ** -52
KAPPA_MAX = 1e10
ROBOTS = ("ur5", "iiwa14", "panda", "xarm6")
FRAMES = ("space", "body", "hybrid")
TASKS = ("full", "linear", "angular")
KIN = ("T", "J", "Jdot_qd")
LAM = ("Lambda", "Jbar", "mu", "p")


def _rows(a):
    a = np.asarray(a)
    return a.reshape(a.shape[0], -1)


def _scale(want):
    return np.maximum(1.0, np.abs(np.nan_to_num(_rows(want))).max(axis=1, keepdims=True))


def kappa_of(J, M, damping=0.0):
    """cond_2(J M^-1 J^T + damping^2 1) per row; inf where J or M is not finite."""
    out = np.full(J.shape[0], np.inf)
    ok = np.isfinite(J).all(axis=(1, 2)) & np.isfinite(M).all(axis=(1, 2))
    A = J[ok] @ np.linalg.solve(M[ok], J[ok].transpose(0, 2, 1)) + damping * damping * np.eye(J.shape[1])
    out[ok] = np.linalg.cond(A)
    return out


def tight(got, want, what):
    err = np.abs(_rows(got) - _rows(want))
    assert (err <= 1e-10 * _scale(want)).all(), f"{what}: worst {err.max():.3e}"


def f64_rule(got, want, what):
    g, w = _rows(got), _rows(want)
    bad = np.abs(g - w) > 1e-6 * np.abs(w) + 1e-7 * _scale(want)
    assert not bad.any(), f"{what}: {int(bad.sum())} entries outside the bound, worst {np.abs(g - w).max():.3e}"


def kappa_rule(got, want, kappa, what, fixture=False):
    """|got - want| <= max(floor, 32 eps kappa) scale (+ 1e-6 |want| against a fixture) on the rows with kappa <= KAPPA_MAX, all of
    which must be finite.  Returns the worst error / bound, which the callers print."""
    g, w = _rows(got), _rows(want)
    use = kappa <= KAPPA_MAX
    floor = 1e-7 if fixture else 1e-10
    bound = np.maximum(floor, 32.0 * EPS * kappa[:, None]) * _scale(want) + (1e-6 * np.abs(w) if fixture else 0.0)
    err = np.abs(g - w)
    assert np.isfinite(g[use]).all(), f"{what}: non-finite values on well-conditioned rows"
    ratio = (err[use] / bound[use]).max() if use.any() else 0.0
    assert ratio <= 1.0, f"{what}: worst error / bound {ratio:.3g} (worst error {err[use].max():.3e})"
    return ratio


def left_out_share(kappa):
    return float(np.mean(kappa > KAPPA_MAX))
