"""The CPU launchers of the run-time-n kernels that loop over time (csrc/mp_dyn.h: mp_dyn_rollout, mp_dyn_pd_regulation_run, compiled
for the host in csrc/mp_cpu.cpp) on robots of 9..32 joints, against the exact Newton-Euler oracle (oracle/newton_euler.py) on the
cases of tests/dyn_cases.py, whose docstring states every bound and where it comes from.  tests/test_gpu_long_chain_trajectories.py
holds the kernels to the same cases and bounds.

The module prints (pytest -s) the figures behind the bounds: the oracle's float64-against-longdouble and float32-against-longdouble
differences per case, and the worst error / bound of each family."""
import numpy as np
import pytest

import dyn_cases as dc
from manipulapy_amd import _hip

WORST = {}


def record(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), float(ratio))
    return ratio


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    if WORST:
        print("\nworst error / bound:", ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())))


def fmt(d):
    return " ".join(f"{k[:3]} {v:.1e}" for k, v in d.items())


@pytest.mark.parametrize("name", dc.MODELS)
def test_cpu_fd_trajectory_against_the_oracle(name):
    """mp_fd_trajectory_cpu_{f64,f32}: every roll-out case, both state types."""
    for case in dc.ROLLOUT_CASES:
        c = dc.rollout(name, case)
        print(f"\n{name} {case}: oracle float64 - longdouble {fmt(c.diff64)}; max|acc| {np.abs(c.o64['accelerations']).max():.1f}"
              + (f"; float32 - longdouble {fmt(c.diff32)}" if c.intRes > 1 else ""))
        model = dc.hip_model(name, c.limits)
        try:
            th, dth, tm, Fm = c.inputs()
            for dtype in (np.float64, np.float32):
                got = _hip.cpu_fd_trajectory(model, th, dth, tm, c.g, Fm, c.dt, c.intRes, dtype=dtype)
                dc.check_rollout(c, got, dtype, record, "cpu_fd_trajectory")
        finally:
            model.destroy()


@pytest.mark.parametrize("name", ["n14", "n17"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_cpu_fd_trajectory_nan_lane(name, dtype):
    c = dc.rollout(name, "wrench")
    model = dc.hip_model(name, c.limits)
    try:
        dc.check_nan_lane(c, lambda th, dth, tm, Fm: _hip.cpu_fd_trajectory(model, th, dth, tm, c.g, Fm, c.dt, c.intRes, dtype=dtype),
                          "cpu_fd_trajectory")
    finally:
        model.destroy()


@pytest.mark.parametrize("name", dc.MODELS)
def test_cpu_pd_regulation_against_the_oracle(name):
    c = dc.regulation(name)
    d = c.lanes.index(dc.PD_DIVERGING)
    print(f"\n{name}: oracle float64 - longdouble {c.diff:.1e} on the converging runs' errors (up to {np.abs(c.e64[c.converging]).max():.2f});"
          f" diverging run stops at step {c.stop} with {c.e64[d, c.stop]:.2e} after {c.e64[d, c.stop - 1]:.2e}, steady for {c.steady} steps")
    model = dc.hip_model(name)
    try:
        err, count = _hip.cpu_pd_regulation(model, c.theta0, c.des, c.kp, c.kd, c.g, dc.PD_DT, dc.PD_STEPS)
        dc.check_regulation(c, err, count, record, "cpu_pd_regulation")
    finally:
        model.destroy()


@pytest.mark.parametrize("name", dc.MODELS)
def test_trajectory_cases_are_what_they_claim(name):
    """The generated-trajectory cases (no CPU twin generates trajectories past 8 joints: the GPU module runs them): the position clip
    engages, about a tenth of the rows exceed a torque limit, under 5 % of the rows lie within the float32 rule's tolerance of one."""
    for case, (Nt, method, wrench) in dc.TRAJ_CASES.items():
        c = dc.trajectory(name, case)
        assert c.rows["positions"].shape == (dc.TRAJ_B, Nt, c.n) and (c.F is not None) == wrench
        tau = c.torques(c.rows["positions"], c.rows["velocities"], c.rows["accelerations"])
        over = (np.abs(tau) > c.torque_limits[:, 1]).any(axis=-1).mean()
        print(f"\n{name} {case}: {over:.3f} of the rows exceed a torque limit, {c.near_limit(tau).mean():.3f} lie near one")
