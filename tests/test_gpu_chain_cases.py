"""GPU: every joint count 1..8 of the twelve later kernel families on chain_cases.chain(n) - prismatic joints included - through the
DEVICE forms, each output buffer filled with 0xFF (a row the kernel skipped reads as NaN) and followed by a 4096-byte guard of 0xA5
that must come back untouched (a store past the last valid row).  Kernels are held to their CPU twins under each family's existing
kernel-against-twin rule and, where test_chain_cases_host.py has one, to the independent oracle.

Row counts: 1 (a single lane), 63, 64 (a full wave: whole-line input staging), 65 and 197 (three waves and five lanes: the per-lane
tail and the chunk of the row store that straddles the last row).

The two planning families (test_rrt_connect, test_path_shortcut) run chain_cases.plan_case / shortcut_case: 1, 64, 65 and all 67 / 73
problems, the full count again on a grid of one block and on a workspace sized for one block, the limits (max_nodes 4 and 2,
max_waypoints 3 and 2, max_iters 0, the tight run, w_in = max_waypoints) and non-finite problems; their workspaces are sized exactly
and guarded like the outputs.  Measured on an MI355X, seconds a test (the oracle's NumPy run on the host included for n = 2, 5, 8):
    n              1     2     3     4     5     6     7     8
    rrt_connect    0.6   3.5   0.8   3.2   7.5   4.5   3.9   6.9
    path_shortcut  0.1   2.1   1.0   <2.2  5.3   3.4   2.5   5.1
(at max_iters 48 / 50 on every chain the same tests took 7 to 16 s on n = 4..8, which is why chain_cases cuts those chains' max_iters.)

Corner blending and fixed-rate sampling (test_path_blend, test_trajectory_sample, test_trajectory_sample_torque_variants,
test_blend_time_sample_chain) run chain_cases.blend_case / sample_curve_case / sample_grid_case through the device runs of
test_gpu_blend.py and test_gpu_sample.py, guard bands included: 40 tests, under a second each, 8 s together."""
import numpy as np
import pytest

import blend_cases as bc
import chain_cases as ch
import collision_cases as cc
import collision_edge_cases as ec
import ilqr_cases as ic
import opspace_cases as oc
import sample_cases as sp
import test_gpu_blend as gb
import test_gpu_sample as gs
import toppra_cases as tc
from manipulapy_amd import _hip, registry

pytestmark = pytest.mark.gpu
ROWS = (1, 63, 64, 65, 197)
BAD = np.array([0, 63, 64])          # the poisoned lanes of the 197-row launch: both ends of the first wave, the start of the second
GUARD = 4096


@pytest.fixture(scope="module")
def ctx():
    c = registry.get_context()
    c.selftest()
    return c


class Out:
    """A device output of `shape` with the payload preset to 0xFF and a guard band of 0xA5 behind it."""

    def __init__(self, ctx, shape, dtype=np.float64):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self.buf = ctx.alloc(self.nbytes + GUARD)
        ctx.memset(self.buf, 0xA5, self.nbytes + GUARD)
        ctx.memset(self.buf, 0xFF, self.nbytes)

    def take(self, what=""):
        """The payload, after checking the guard; frees the buffer."""
        raw = self.buf.download((self.nbytes + GUARD,), np.uint8)
        self.buf.free()
        assert (raw[self.nbytes:] == 0xA5).all(), f"{what}: bytes written past the last valid row"
        return raw[:self.nbytes].view(self.dtype).reshape(self.shape)


class Inputs:
    """Host arrays on the device; None stays None."""

    def __init__(self, ctx, *arrays):
        self.bufs = [None if a is None else ctx.to_device(np.ascontiguousarray(a)) for a in arrays]

    def __iter__(self):
        return iter(self.bufs)

    def free(self):
        for b in self.bufs:
            if b is not None:
                b.free()


def _tight(got, want, what):
    """the kernel-against-twin rule of the VJP families (test_gpu_dynamics_vjp.py)"""
    got, want = got.reshape(len(got), -1), want.reshape(len(want), -1)
    scale = np.maximum(1.0, np.abs(want).max(axis=-1, keepdims=True))
    err = np.abs(got - want)
    assert (err <= 1e-10 * scale).all(), f"{what}: worst {np.nanmax(err):.3e}"


def _poisoned_rows_alone(clean, dirty, what, nan=True):
    keep = np.setdiff1d(np.arange(len(clean)), BAD)
    if nan:
        assert np.isnan(dirty[BAD]).all(), f"{what}: a poisoned row is NaN everywhere"
    assert np.array_equal(dirty[keep], clean[keep]), f"{what}: a poisoned row changed its neighbours"


# ------------------------------------------------------------------------------------------------ mp_id_vjp_f64 / mp_fd_vjp_f64
def _dyn_vjp(ctx, model, d, rows, F):
    n = model.n
    x = Inputs(ctx, d["q"][:rows], d["qd"][:rows], d["x"][:rows], d["lam"][:rows])
    o = [Out(ctx, (rows, n)) for _ in range(7)]
    a, b, c, lam = x
    ctx.id_vjp(model, a, b, c, lam, rows, o[0].buf, o[1].buf, o[2].buf, g=d["g"], Ftip=F)
    ctx.fd_vjp(model, a, b, c, lam, rows, o[4].buf, o[5].buf, d_qdd=o[3].buf, d_gtau=o[6].buf, g=d["g"], Ftip=F)
    ctx.synchronize()
    x.free()
    return [v.take(f"n={n} rows={rows}") for v in o]


@pytest.mark.parametrize("n", ch.NS)
def test_dynamics_vjp(ctx, n):
    model = ch.chain(n)[3]
    d = ch.dynamics_rows(n)
    for F in (None, d["F"]):
        for rows in ROWS:
            got = _dyn_vjp(ctx, model, d, rows, F)
            args = (model, d["q"][:rows], d["qd"][:rows], d["x"][:rows], d["lam"][:rows], d["g"], F)
            want = list(_hip.cpu_id_vjp(*args)) + list(_hip.cpu_fd_vjp(*args))
            for a, b, k in zip(got, want, ("id gq", "id gqd", "id gqdd", "fd qdd", "fd gq", "fd gqd", "fd gtau")):
                _tight(a, b, f"n={n} rows={rows} F={F is not None} {k}")
    clean = got
    bad = dict(d, q=d["q"].copy())
    bad["q"][BAD, np.arange(3) % n] = np.nan
    for a, b in zip(clean, _dyn_vjp(ctx, model, bad, 197, d["F"])):
        _poisoned_rows_alone(a, b, f"n={n}")


# ------------------------------------------------------------------------------------------------ mp_fk_jac_vjp_f64
def _kin_vjp(ctx, model, frame, q, gT, gJ, want=("T", "J", "gq")):
    rows, n = q.shape
    shapes = {"T": (rows, 4, 4), "J": (rows, 6, n), "gq": (rows, n)}
    x = Inputs(ctx, q, gT, gJ)
    o = {k: Out(ctx, shapes[k]) for k in want}
    ctx.fk_jac_vjp(model, frame, *x, rows, **{"d_" + k: v.buf for k, v in o.items()})
    ctx.synchronize()
    x.free()
    return {k: v.take(f"n={n} rows={rows} {frame} {k}") for k, v in o.items()}


@pytest.mark.parametrize("n", ch.NS)
def test_kinematics_vjp(ctx, n):
    model = ch.chain(n)[3]
    d = ch.dynamics_rows(n)
    for frame in ("space", "body"):
        for rows in ROWS:
            q, gT, gJ = d["q"][:rows], d["gT"][:rows], d["gJ"][:rows]
            for cT, cJ in ((gT, gJ), (gT, None), (None, gJ)):
                got = _kin_vjp(ctx, model, frame, q, cT, cJ)
                want = dict(zip(("T", "J", "gq"), _hip.cpu_fk_jac_vjp(model, q, cT, cJ, frame, want_T=True, want_J=True)))
                for k in got:
                    _tight(got[k], want[k], f"n={n} rows={rows} {frame} {k} gT={cT is not None} gJ={cJ is not None}")
            for k in ("T", "J", "gq"):      # each output alone: the same numbers (got: the launch with gJ only)
                one = _kin_vjp(ctx, model, frame, q, None, gJ, want=(k,))
                assert np.array_equal(one[k], got[k]), f"n={n} rows={rows} {frame} {k} alone"
        clean = _kin_vjp(ctx, model, frame, d["q"], d["gT"], d["gJ"])
        bad = d["q"].copy()
        bad[BAD, np.arange(3) % n] = np.nan
        dirty = _kin_vjp(ctx, model, frame, bad, d["gT"], d["gJ"])
        for k in clean:
            _poisoned_rows_alone(clean[k], dirty[k], f"n={n} {frame} {k}")


# ------------------------------------------------------------------------------------------------ mp_fd_trajectory_vjp_tm_f64
def _close(got, want, what, rtol=1e-8):
    """the kernel-against-twin rule of test_gpu_rollout_vjp.py"""
    scale = max(1.0, float(np.abs(want).max(initial=0.0)))
    bad = ~(np.abs(got - want) <= rtol * np.abs(want) + rtol * 0.1 * scale)
    assert not bad.any(), f"{what}: {int(bad.sum())} entries outside the bound, worst {np.nanmax(np.abs(got - want), initial=0.0):.3e}"


def _tm(a):
    return None if a is None else np.ascontiguousarray(np.swapaxes(a, 0, 1))


def _rollout_vjp(ctx, model, th, dth, tm, F, intRes, G):
    """The device (time-major) form on batch-major host arrays: (gtheta0, gdtheta0, gtaumat (B, N, n))."""
    (B, N, n) = tm.shape
    x = Inputs(ctx, th, dth, _tm(tm), _tm(F), *[_tm(g) for g in G])
    work = ctx.alloc(max(16, _hip.fd_trajectory_vjp_workspace_bytes(model, B, N, intRes)))
    o = [Out(ctx, (B, n)), Out(ctx, (B, n)), Out(ctx, (N, B, n))]
    b = x.bufs
    ctx.fd_trajectory_vjp(model, b[0], b[1], b[2], b[3], B, N, ch.G9, 0.01, intRes, b[4], b[5], b[6], work, *[v.buf for v in o])
    ctx.synchronize()
    x.free()
    work.free()
    got = [v.take(f"n={n} roll-out VJP") for v in o]
    return got[0], got[1], np.swapaxes(got[2], 0, 1)


@pytest.mark.parametrize("n", ch.NS)
def test_rollout_vjp(ctx, n):
    model, prismatic = ch.chain(n)[3], ch.chain(n)[1]
    rng = np.random.default_rng(9200 + n)
    B, N = 197, 4
    span = np.where(prismatic, 0.2, 0.5)
    th, dth, tm = rng.uniform(-1, 1, (B, n)) * span, rng.uniform(-0.5, 0.5, (B, n)), rng.uniform(-1, 1, (B, N, n))
    G = [rng.uniform(-1, 1, (B, N, n)) for _ in range(3)]
    for F in (None, rng.uniform(-1, 1, (B, N, 6))):
        for intRes in (1, 3):
            want = _hip.cpu_fd_trajectory_vjp(model, th, dth, tm, ch.G9, F, 0.01, intRes, *G)
            got = _rollout_vjp(ctx, model, th, dth, tm, F, intRes, G)
            host = ctx.fd_trajectory_vjp_host(model, th, dth, tm, ch.G9, F, 0.01, intRes, *G)      # batch-major: converted on the device
            for a, b, c, k in zip(got, host, want, ("theta0", "dtheta0", "taumat")):
                _close(a, c, f"n={n} F={F is not None} intRes={intRes} time-major d/d{k}")
                _close(b, c, f"n={n} F={F is not None} intRes={intRes} batch-major d/d{k}")
    bad = th.copy()
    bad[BAD, np.arange(3) % n] = np.nan
    for a, b in zip(got, _rollout_vjp(ctx, model, bad, dth, tm, F, 3, G)):
        _poisoned_rows_alone(a, b, f"n={n} roll-out VJP")


# ------------------------------------------------------------------------------------------------ mp_opspace_f64 / mp_opspace_torque_f64
def _opspace(ctx, model, frame, task, damping, q, qd, acc, t0):
    rows, n = q.shape
    m = ch.opspace_dim(task)
    shapes = {"T": (rows, 4, 4), "J": (rows, m, n), "Jdot_qd": (rows, m), "Lambda": (rows, m, m), "Jbar": (rows, n, m), "mu": (rows, m),
              "p": (rows, m)}
    x = Inputs(ctx, q, qd, acc, t0)
    o = {k: Out(ctx, shapes[k]) for k in _hip.OPSPACE_OUTPUTS}
    tau = [Out(ctx, (rows, n)), Out(ctx, (rows, n))]
    b = x.bufs
    ctx.opspace(model, frame, task, damping, b[0], b[1], rows, ch.G9, *[o[k].buf for k in _hip.OPSPACE_OUTPUTS])
    ctx.opspace_torque(model, frame, task, damping, b[0], b[1], b[2], b[3], rows, tau[0].buf, ch.G9)
    ctx.opspace_torque(model, frame, task, damping, b[0], b[1], b[2], None, rows, tau[1].buf, ch.G9)
    ctx.synchronize()
    x.free()
    what = f"n={n} rows={rows} {frame} {task} damping {damping}"
    got = {k: v.take(what + " " + k) for k, v in o.items()}
    got["tau"], got["tau_no_tau0"] = tau[0].take(what + " tau"), tau[1].take(what + " tau")
    return got


def _opspace_twin(model, frame, task, damping, q, qd, acc, t0):
    want = _hip.cpu_opspace(model, q, qd, ch.G9, frame, task, damping)
    want["tau"] = _hip.cpu_opspace_torque(model, q, qd, acc, ch.G9, t0, frame, task, damping)
    want["tau_no_tau0"] = _hip.cpu_opspace_torque(model, q, qd, acc, ch.G9, None, frame, task, damping)
    return want


@pytest.mark.parametrize("n", ch.NS)
def test_opspace(ctx, n):
    model = ch.chain(n)[3]
    q, qd = (a[:197] for a in ch.opspace_inputs(n))
    rng = np.random.default_rng(9300 + n)
    acc6, t0 = rng.normal(size=(197, 6)), rng.normal(size=(197, n))
    M = _hip.cpu_mass_matrix(model, q)
    worst, last = 0.0, None
    for frame in oc.FRAMES:
        for task in oc.TASKS:
            m = ch.opspace_dim(task)
            acc = np.ascontiguousarray(acc6[:, :m])
            for damping in (ch.OPSPACE_DAMPING, 0.0):
                wider = damping == 0.0 and m > n
                if damping == 0.0 and not wider and (frame, task) not in ch.opspace_damping0_runs(n):
                    continue
                ref = ch.opspace_oracle(n, frame, task, damping, rows=ch.OPSPACE_GPU_ORACLE_ROWS)
                for rows in ROWS:
                    what = f"n={n} rows={rows} {frame} {task} damping {damping}"
                    a = (q[:rows], qd[:rows], acc[:rows], t0[:rows])
                    got, want = _opspace(ctx, model, frame, task, damping, *a), _opspace_twin(model, frame, task, damping, *a)
                    held = rows <= ch.OPSPACE_GPU_ORACLE_ROWS       # the launches that are held to the oracle as well as to the twin
                    for k in oc.KIN:
                        oc.tight(got[k], want[k], f"{what} {k}")
                        if held:
                            oc.f64_rule(got[k], ref[k][:rows], f"{what} {k} against the oracle")
                    if wider:   # a task wider than the chain: NaN by (m, n), on the device as on the host
                        assert all(np.isnan(got[k]).all() for k in oc.LAM + ("tau", "tau_no_tau0")), what
                        assert all(np.isfinite(got[k]).all() for k in oc.KIN), what
                        continue
                    kappa = oc.kappa_of(want["J"], M[:rows], damping)
                    assert oc.left_out_share(kappa) <= 0.02, f"{what}: {oc.left_out_share(kappa):.2%} of the rows have cond(A) > 1e10"
                    for k in oc.LAM + ("tau", "tau_no_tau0"):
                        worst = max(worst, oc.kappa_rule(got[k], want[k], kappa, f"{what} {k}"))
                    for k in oc.LAM if held else ():
                        worst = max(worst, oc.kappa_rule(got[k], ref[k][:rows], ref["kappa"][:rows], f"{what} {k} against the oracle",
                                                         fixture=True))
                if damping:
                    last = (frame, task, damping, acc, got)
    frame, task, damping, acc, clean = last               # 197 rows, the last combination with damping
    bad = q.copy()
    bad[BAD, np.arange(3) % n] = np.nan
    dirty = _opspace(ctx, model, frame, task, damping, bad, qd, acc, t0)
    for k in clean:
        _poisoned_rows_alone(clean[k], dirty[k], f"n={n} {k}")
    print(f"\nopspace n={n}: kernel against twin and oracle, worst error / bound {worst:.3g}")


# ------------------------------------------------------------------------------------------------ mp_collision_f64
_INT = ("arg_world", "arg_self")
LEAN = ("dist_world", "arg_world", "dist_self", "arg_self", "cost")           # the instance without gradients


def _collision(ctx, cm, q, want=_hip.COLLISION_OUTPUTS):
    rows, n = q.shape
    shapes = {"dist_world": (rows,), "arg_world": (rows, 2), "dist_self": (rows,), "arg_self": (rows, 2), "grad_dist_world": (rows, n),
              "grad_dist_self": (rows, n), "cost": (rows,), "grad": (rows, n)}
    x = Inputs(ctx, q)
    o = {k: Out(ctx, shapes[k], np.int32 if k in _INT else np.float64) for k in want}
    cm.sync_world(ctx)
    ctx.collision(cm.model, cm.handle, x.bufs[0], rows, cc.EPS_WORLD, cc.EPS_SELF, **{"d_" + k: v.buf for k, v in o.items()})
    ctx.synchronize()
    x.free()
    return {k: v.take(f"n={n} rows={rows} {k}") for k, v in o.items()}


_collision_refs = {}


def _collision_ref(n):
    if n not in _collision_refs:
        case = ch.collision_case(n)
        cm = case["cm"]
        _collision_refs[n] = (case, _hip.cpu_collision(cm.model, cm.handle, case["q"], cc.EPS_WORLD, cc.EPS_SELF), cc.oracle_of(case))
    return _collision_refs[n]


@pytest.mark.parametrize("n", ch.NS)
def test_collision(ctx, n):
    case, twin, ref = _collision_ref(n)
    cm, q = case["cm"], case["q"]
    for rows in ROWS:
        got = _collision(ctx, cm, q[:rows])
        head = {k: v[:rows] for k, v in ref.items() if k in _hip.COLLISION_OUTPUTS or k.startswith("gap_")}
        cc.check_against_oracle(got, head, f"n={n} kernel against the oracle, {rows} rows", show=False, case=ref)
        tw = {k: v[:rows] for k, v in twin.items()}
        tw.update({f"gap_{key}": ref[f"gap_{key}"][:rows] for key in ("world", "self")})
        cc.check_against_oracle(got, tw, f"n={n} kernel against the twin, {rows} rows", show=False, case=twin)
        lean = _collision(ctx, cm, q[:rows], want=LEAN)
        cc.check_against_oracle(lean, tw, f"n={n} kernel without gradients against the twin, {rows} rows", show=False, case=twin)
        assert np.array_equal(lean["arg_world"], got["arg_world"]) and np.array_equal(lean["arg_self"], got["arg_self"])
    bad = q[:197].copy()
    bad[BAD, np.arange(3) % n] = np.nan
    dirty = _collision(ctx, cm, bad)
    keep = np.setdiff1d(np.arange(197), BAD)
    for k in got:
        assert (dirty[k][BAD] == -1).all() if k in _INT else np.isnan(dirty[k][BAD]).all(), f"n={n} {k}"
        assert np.array_equal(dirty[k][keep], got[k][keep]), f"n={n} {k}"


# ------------------------------------------------------------------------------------------------ mp_collision_edges_f64
_EDGE_SHAPE = {"status": (1, np.int32), "t": (1, np.float64), "steps": (1, np.int32), "clearance": (1, np.float64), "witness": (3, np.int32)}
_edge_refs = {}


def _edges(ctx, cm, qa, qb):
    E, n = qa.shape
    x = Inputs(ctx, qa, qb)
    o = {k: Out(ctx, (E, 3) if k == "witness" else (E,), _EDGE_SHAPE[k][1]) for k in ec.EDGE_KEYS}
    cm.sync_world(ctx)
    ctx.collision_edges(cm.model, cm.handle, x.bufs[0], x.bufs[1], E, ec.MARGIN, ec.TOL, ec.MAX_STEPS, **{"d_" + k: v.buf for k, v in o.items()})
    ctx.synchronize()
    x.free()
    return {k: v.take(f"n={n} edges {k}") for k, v in o.items()}


@pytest.mark.parametrize("n", ch.NS)
def test_collision_edges(ctx, n):
    if n not in _edge_refs:
        case = ch.edge_case(n)
        cm = case["cm"]
        _edge_refs[n] = (case, _hip.cpu_collision_edges(cm.model, cm.handle, case["qa"], case["qb"], ec.MARGIN, ec.TOL, ec.MAX_STEPS),
                         ch.edge_oracle(n))
    case, twin, ref = _edge_refs[n]
    cm = case["cm"]
    got = _edges(ctx, cm, case["qa"], case["qb"])
    ec.check_against_oracle(got, ref, f"n={n} kernel against the oracle", show=False)
    ec.check_against_oracle(got, dict(twin, gap=ref["gap"]), f"n={n} kernel against the twin", show=False)
    qa = case["qa"].copy()
    qa[BAD, np.arange(3) % n] = np.nan
    dirty = _edges(ctx, cm, qa, case["qb"])
    assert (dirty["status"][BAD] == ec.INVALID).all() and (dirty["steps"][BAD] == 0).all() and (dirty["witness"][BAD] == -1).all()
    assert np.isnan(dirty["t"][BAD]).all() and np.isnan(dirty["clearance"][BAD]).all()
    keep = np.setdiff1d(np.arange(len(qa)), BAD)
    for k in got:
        assert np.array_equal(dirty[k][keep], got[k][keep]), f"n={n} {k}"


# ------------------------------------------------------------------------------------------------ mp_ilqr_backward_tm_f64 / mp_ilqr_rollout_tm_f64
IB, IA = 197, 3
ALPHA = np.array([1.0, 0.25, 0.0])[:, None] * np.ones((1, IB))
_ilqr_refs = {}


def _ilqr_ref(n):
    """model, limits, case and the twins' results (nominal, backward at reg 1e-6, closed loop at ALPHA): built once, never written to."""
    if n not in _ilqr_refs:
        model, lim, case = ch.ilqr_case(n, IB)
        pos, vel, _, blocks = ic.nominal_and_blocks(model, case)
        w = (case["wq"], case["wr"], case["wf"])
        back = _hip.cpu_ilqr_backward(model, pos, vel, case["taumat"], case["xref"], *w, 1e-6, ic.G9, ic.DT)
        roll = _hip.cpu_ilqr_rollout(model, case["theta0"], case["dtheta0"], case["taumat"], pos, vel, back[0], back[1], ALPHA,
                                     case["xref"], *w, ic.G9, ic.DT)
        _ilqr_refs[n] = (model, lim, case, w, pos, vel, blocks, back, roll)
    return _ilqr_refs[n]


def _ilqr_backward(ctx, model, case, w, pos, vel):
    """The derivative launch and the backward pass on device buffers: (K (B, N, n, 2n), k (B, N, n), dV (B, 2), status (B))."""
    n, N, B = model.n, ch.ILQR_N, IB
    x = Inputs(ctx, _tm(pos), _tm(vel), _tm(case["taumat"]), _tm(case["xref"]), np.full(B, 1e-6),
               _tm(case["taumat"])[1:])                  # rows 1..N-1 on their own: a 16-byte aligned start whatever B n is
    dpos, dvel, dtau, dxr, dreg, dtau1 = x.bufs
    blk = [Out(ctx, ((N - 1) * B, n, n)) for _ in range(3)]
    work = ctx.alloc(max(16, _hip.ilqr_backward_workspace_bytes(model, B, N)))
    o = [Out(ctx, (N, B, n, 2 * n)), Out(ctx, (N, B, n)), Out(ctx, (B, 2)), Out(ctx, (B,), np.int32)]
    ctx.fd_derivatives(model, dpos, dvel, dtau1, (N - 1) * B, blk[0].buf, blk[1].buf, d_Minv=blk[2].buf, g=ic.G9)
    ctx.ilqr_backward(model, dpos, dvel, dtau, blk[0].buf, blk[1].buf, blk[2].buf, dxr, *w, dreg, B, N, ic.DT, work, *[v.buf for v in o])
    ctx.synchronize()
    x.free()
    work.free()
    for v in blk:
        v.take(f"n={n} derivative blocks")
    K, k, dV, status = (v.take(f"n={n} ilqr backward") for v in o)
    return np.swapaxes(K, 0, 1), np.swapaxes(k, 0, 1), dV, status


def _ilqr_rollout(ctx, model, case, w, pos, vel, K, k, theta0=None, rows=True):
    n, N, B, A = model.n, ch.ILQR_N, IB, IA
    x = Inputs(ctx, case["theta0"] if theta0 is None else theta0, case["dtheta0"], _tm(case["taumat"]), _tm(pos), _tm(vel), _tm(K), _tm(k),
               ALPHA, _tm(case["xref"]))
    cost = Out(ctx, (A, B))
    o = [Out(ctx, (N, A * B, n)) for _ in range(3)] if rows else []
    b = x.bufs
    ctx.ilqr_rollout(model, b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7], b[8], *w, A, B, N, ic.G9, ic.DT, cost.buf, *[v.buf for v in o])
    ctx.synchronize()
    x.free()
    return (cost.take(f"n={n} ilqr cost"),) + tuple(np.swapaxes(v.take(f"n={n} ilqr rows"), 0, 1).reshape(A, B, N, n) for v in o)


@pytest.mark.parametrize("n", ch.NS)
def test_ilqr(ctx, n, monkeypatch):
    model, lim, case, w, pos, vel, blocks, back, roll = _ilqr_ref(n)
    Ko, ko, dVo, _ = ic.oracle_batch(lim, case, pos, vel, blocks, 1e-6)
    for variant in ("cooperative", "lane"):
        if variant == "lane":
            monkeypatch.setenv("MANIPULAPY_HIP_ILQR_BACKWARD", "lane")
            assert _hip.ilqr_backward_workspace_bytes(model, IB, ch.ILQR_N) == 12 * n * n * IB * 8
        K, k, dV, status = _ilqr_backward(ctx, model, case, w, pos, vel)
        assert np.array_equal(status, back[3]) and (status == 0).all() and not K[:, 0].any() and not k[:, 0].any()
        worst = max(ic.within_bound(K, back[0], "K"), ic.within_bound(k, back[1], "k"), ic.within_bound(dV, back[2], "dV"),
                    ic.within_bound(K, Ko, "K against the oracle"), ic.within_bound(k, ko, "k against the oracle"),
                    ic.within_bound(dV, dVo, "dV against the oracle"))
        print(f"\nilqr n={n} {variant}: backward kernel against twin and oracle {worst:.3e} of max|.| (bound {ic.BOUND:.1e})")
        bad = pos.copy()
        bad[BAD] = np.nan
        K2, k2, dV2, status2 = _ilqr_backward(ctx, model, case, w, bad, vel)
        keep = np.setdiff1d(np.arange(IB), BAD)
        assert (status2[BAD] == -1).all() and np.isnan(K2[BAD, 1:]).all() and np.isnan(dV2[BAD]).all()
        for a, b in zip((K2, k2, dV2, status2), (K, k, dV, status)):
            assert np.array_equal(a[keep], b[keep])
    monkeypatch.delenv("MANIPULAPY_HIP_ILQR_BACKWARD")
    got = _ilqr_rollout(ctx, model, case, w, pos, vel, back[0], back[1])      # on the twin's gains, as test_gpu_ilqr.py does
    for a, b, what in zip(got, roll, ("cost", "pos", "vel", "tau")):
        ic.f64_rule(a, b, f"n={n} {what}")
    assert np.array_equal(_ilqr_rollout(ctx, model, case, w, pos, vel, back[0], back[1], rows=False)[0], got[0])
    bad = case["theta0"].copy()
    bad[BAD, np.arange(3) % n] = np.nan
    dirty = _ilqr_rollout(ctx, model, case, w, pos, vel, back[0], back[1], theta0=bad)
    for a, b in zip(dirty, got):
        assert np.isnan(a[:, BAD]).all() and np.array_equal(np.delete(a, BAD, axis=1), np.delete(b, BAD, axis=1))


# ------------------------------------------------------------------------------------------------ mp_path_dynamics_f64 / mp_toppra_tm_f64
TB = 67
TROWS = ("velocities", "accelerations", "torques")
_toppra_refs = {}


def _toppra_ref(n, N):
    """The case, the oracle's coefficients and the twin's sweeps on them without and with acceleration limits; the oracle's own result
    on the first 6 paths."""
    if (n, N) not in _toppra_refs:
        model, vlim, tlim, (q, dq, ddq) = ch.toppra_case(n, TB, N)
        co = tc.oracle_coeffs(model, q, dq, ddq, vlim)
        twin = _hip.cpu_toppra_sweep(*co, dq, ddq, tlim, None)
        alim = np.maximum(np.abs(twin["accelerations"][twin["status"] == 0][:, :-1]).max(axis=(0, 1)) / 3.0, 1e-3)
        head = tuple(c[:6] for c in co)
        _toppra_refs[n, N] = (model, vlim, tlim, alim, (q, dq, ddq), co, {False: twin, True: _hip.cpu_toppra_sweep(*co, dq, ddq, tlim, alim)},
                              {False: tc.oracle_batch(*head, dq[:6], ddq[:6], tlim), True: tc.oracle_batch(*head, dq[:6], ddq[:6], tlim, alim)})
    return _toppra_refs[n, N]


def _path_dynamics(ctx, model, paths, vlim):
    q, dq, ddq = paths
    B, N, n = q.shape
    x = Inputs(ctx, _tm(q), _tm(dq), _tm(ddq))
    o = [Out(ctx, (N, B, n)) for _ in range(3)] + [Out(ctx, (N, B))]
    ctx.path_dynamics(model, *x, B * N, vlim, *[v.buf for v in o], tc.G9, None)
    ctx.synchronize()
    x.free()
    return tuple(np.swapaxes(v.take(f"n={n} path dynamics"), 0, 1) for v in o)


def _toppra_sweep(ctx, model, co, dq, ddq, tlim, alim):
    B, N, n = dq.shape
    x = Inputs(ctx, *[_tm(c) for c in co], _tm(dq), _tm(ddq), np.zeros(B), np.zeros(B))
    names = ("controllable", "sd2", "sdd", "time", "duration", "status") + TROWS
    shapes = ((N, B, 2), (N, B), (N, B), (N, B), (B,), (B,), (N, B, n), (N, B, n), (N, B, n))
    o = [Out(ctx, s, np.int32 if k == "status" else np.float64) for k, s in zip(names, shapes)]
    b = x.bufs
    ctx.toppra(model, b[0], b[1], b[2], b[3], b[4], b[5], tlim, alim, b[6], b[7], B, N, *[v.buf for v in o])
    ctx.synchronize()
    x.free()
    got = {k: v.take(f"n={n} toppra {k}") for k, v in zip(names, o)}
    return {k: v if v.ndim == 1 else np.swapaxes(v, 0, 1) for k, v in got.items()}


@pytest.mark.parametrize("N", (33, 3))
@pytest.mark.parametrize("n", ch.NS)
def test_toppra(ctx, n, N, monkeypatch):
    model, vlim, tlim, alim, paths, co, twins, oracles = _toppra_ref(n, N)
    q, dq, ddq = paths
    twin_co = _hip.cpu_path_dynamics(model, q.reshape(-1, n), dq.reshape(-1, n), ddq.reshape(-1, n), vlim, tc.G9)
    for got, want, ora, what in zip(_path_dynamics(ctx, model, paths, vlim), twin_co, co, ("a", "b", "c", "xbar")):     # (b)
        tc.f64_rule(got, want.reshape(got.shape), f"n={n} {what}")
        tc.f64_rule(got, ora, f"n={n} {what} against the three-call form")
    for epilogue in ("fused", "separate"):
        if epilogue == "separate":
            monkeypatch.setenv("MANIPULAPY_HIP_TOPPRA_EPILOGUE", "separate")
        for acc in (False, True):
            what = f"toppra n={n} N {N} acc {acc} {epilogue} epilogue"
            want, ora = twins[acc], oracles[acc]
            got = _toppra_sweep(ctx, model, co, dq, ddq, tlim, alim if acc else None)                                # (a)
            assert np.array_equal(got["status"], want["status"])
            ok = want["status"] == 0
            fine = ch.toppra_not_stalling(want)
            need = ch.TOPPRA_NOT_STALLING_OF_67[N][acc][n - 1]
            assert ok.all() and fine.sum() >= need, f"{what}: {int(ok.sum())} feasible, {int(fine.sum())} without a stall (recorded: {need})"
            tc.rule_a({k: v[fine] for k, v in got.items()}, {k: v[fine] for k, v in want.items()}, what)
            for key in TROWS:
                tc.f64_rule(got[key][ok], want[key][ok], key)
            for key in ("sd2", "sdd", "time", "duration") + TROWS:
                assert np.isnan(got[key][~ok]).all()
            assert np.array_equal(np.isnan(got["controllable"]), np.isnan(want["controllable"]))
            head = fine[:6] & ch.toppra_not_stalling(ora)
            tc.rule_a({k: v[:6][head] for k, v in got.items()}, {k: v[head] for k, v in ora.items()}, what + " against the oracle")
    monkeypatch.delenv("MANIPULAPY_HIP_TOPPRA_EPILOGUE")
    bad = q.copy()
    bad[BAD, 1, np.arange(3) % n] = np.nan                # a NaN in q: status -1, that path alone
    co_bad = _path_dynamics(ctx, model, (bad, dq, ddq), vlim)
    co_ok = _path_dynamics(ctx, model, paths, vlim)
    clean, dirty = (_toppra_sweep(ctx, model, c, dq, ddq, tlim, alim) for c in (co_ok, co_bad))
    keep = np.setdiff1d(np.arange(TB), BAD)
    assert (dirty["status"][BAD] == -1).all()
    for k in clean:
        assert np.array_equal(dirty[k][keep], clean[k][keep], equal_nan=True), k
        assert k == "status" or np.isnan(dirty[k][BAD]).all(), k


# ------------------------------------------------------------------------------------------------ mp_rrt_connect_f64
# Only the kernel runs MpRrtTreeLanes ([tree][node][dim][lane], the int32 parents behind the doubles, blockIdx.x * block_words), the
# wave-wide loops with divergent lanes and the per-instance raise of the dynamic-LDS limit; the twin cannot stand in for them.  So
# every output AND the workspace - sized exactly as mp_rrt_connect_workspace_bytes says - carry a guard band, and every discrete
# output of every problem must equal the twin's (gap = inf: nobody is excused).
PLAN_COUNTS = (1, 64, 65, ch.PLAN_PROBLEMS)
ORACLE_NS = (2, 5, 8)             # the chains on which the kernel is held to the oracle too (the host test holds the twin to it everywhere)
_PLAN_SHAPE = {"status": 1, "count": 1, "iterations": 1, "evaluations": 1, "nodes": 2}


def _rrt(ctx, n, qs, qg, max_blocks=0, blocks=None, **over):
    import rrt_cases as rc

    case, p = ch.plan_case(n), ch.plan_params(n, **over)
    cm = case["cm"]
    B = len(qs)
    ws_bytes = _hip.rrt_connect_workspace_bytes(n, p["max_nodes"], (B + 63) // 64 if blocks is None else blocks)
    x = Inputs(ctx, qs, qg)
    ws = Out(ctx, (ws_bytes,), np.uint8)                  # stale 0xFF nodes everywhere, and nothing behind the last block's parents
    o = {k: Out(ctx, (B,) if w == 1 else (B, w), np.int32) for k, w in _PLAN_SHAPE.items()}
    o["waypoints"] = Out(ctx, (B, p["max_waypoints"], n))
    cm.sync_world(ctx)
    ctx.rrt_connect(cm.model, cm.handle, x.bufs[0], x.bufs[1], B, case["lo"], case["hi"], rc.MARGIN, rc.TOL, d_workspace=ws.buf,
                    workspace_bytes=ws_bytes, max_blocks=max_blocks, **p, **{"d_" + k: v.buf for k, v in o.items()})
    ctx.synchronize()
    x.free()
    what = f"rrt n={n} problems={B} {over}"
    ws.take(what + " workspace")
    return {k: v.take(f"{what} {k}") for k, v in o.items()}


def _identical(a, b, what, rows=None):
    for k in a:
        x, y = (a[k], b[k]) if rows is None else (a[k][rows], b[k][rows])
        assert np.array_equal(x, y, equal_nan=True), f"{what}: {k}"


def _held_to_plan_twin(got, twin, B, case, what):
    import rrt_cases as rc

    ref = {k: v[:B] for k, v in twin.items()}
    ref["gap"] = np.full(B, np.inf)
    err = rc.check_against_oracle(got, ref, what, show=False)
    solved = got["status"] == rc.SOLVED
    assert np.array_equal(got["waypoints"][solved][:, 0], case["qs"][:B][solved]), what
    assert np.array_equal(got["waypoints"][solved][:, -1], case["qg"][:B][solved]), what
    return err


@pytest.mark.parametrize("n", ch.NS)
def test_rrt_connect(ctx, n):
    import rrt_cases as rc

    case, twin = ch.plan_case(n), ch.plan_twin(n)
    qs, qg = case["qs"], case["qg"]
    worst = 0.0
    for B in PLAN_COUNTS:
        full = _rrt(ctx, n, qs[:B], qg[:B])
        worst = max(worst, _held_to_plan_twin(full, twin, B, case, f"rrt n={n} kernel against the twin, {B} problems"))
    _identical(_rrt(ctx, n, qs, qg, max_blocks=1), full, f"rrt n={n} max_blocks 1")          # 67 problems on 64 lanes: workspaces reused
    _identical(_rrt(ctx, n, qs, qg, blocks=1), full, f"rrt n={n} workspace of one block")
    if n in ORACLE_NS:
        worst = max(worst, rc.check_against_oracle(full, ch.plan_oracle(n), f"rrt n={n} kernel against the oracle", show=False))
    for over in ({"max_nodes": 4}, {"max_nodes": 2}, {"max_waypoints": 3}, {"max_waypoints": 2}, {"max_iters": 0}):
        got = _rrt(ctx, n, qs, qg, **over)
        _held_to_plan_twin(got, ch.plan_twin(n, **over), len(qs), case, f"rrt n={n} {over} kernel against the twin")
    bad_s, bad_g = qs.copy(), qg.copy()
    bad_s[BAD[0], 0], bad_g[BAD[1], (n - 1) // 2], bad_s[BAD[2], n - 1] = np.nan, np.inf, -np.inf
    dirty = _rrt(ctx, n, bad_s, bad_g)
    assert (dirty["status"][BAD] == rc.INVALID).all() and np.isnan(dirty["waypoints"][BAD]).all()
    for k in ("count", "iterations", "nodes", "evaluations"):
        assert (dirty[k][BAD] == 0).all(), k
    _identical(dirty, full, f"rrt n={n} beside non-finite problems", np.setdiff1d(np.arange(len(qs)), BAD))
    print(f"\nrrt n={n}: kernel against twin{' and oracle' if n in ORACLE_NS else ''}: waypoints {worst:.3g} (bound {rc.WAYPOINT_BOUND:.3g})")


# ------------------------------------------------------------------------------------------------ mp_path_shortcut_f64
SHORTCUT_COUNTS = (1, 64, 65, ch.SHORTCUT_PROBLEMS)
_SC_REAL = ("waypoints", "length_in", "length_out")


@pytest.fixture(scope="module")
def planner():
    import manipulapy_amd as mp

    sm, dyn, lim = mp.load_robot("ur5")  # (batch_validate_path takes the joint count from the collision model)
    return mp.OptimizedTrajectoryPlanning(sm, None, dyn, lim, use_cuda=False)


def _shortcut(ctx, n, wp, cnt, max_blocks=0, blocks=None, **over):
    import shortcut_cases as sc

    cm, p = ch.shortcut_case(n)["cm"], ch.shortcut_params(n, **over)
    wp, cnt = np.ascontiguousarray(wp, dtype=np.float64), np.ascontiguousarray(cnt, dtype=np.int32)
    B, w_in, _ = wp.shape
    W = p["max_waypoints"]
    ws_bytes = _hip.path_shortcut_workspace_bytes(n, W, (B + 63) // 64 if blocks is None else blocks)
    x = Inputs(ctx, wp, cnt)
    ws = Out(ctx, (ws_bytes,), np.uint8)
    o = {k: Out(ctx, (B, W, n) if k == "waypoints" else (B,), np.float64 if k in _SC_REAL else np.int32) for k in sc.KEYS}
    cm.sync_world(ctx)
    ctx.path_shortcut(cm.model, cm.handle, x.bufs[0], x.bufs[1], B, w_in, sc.MARGIN, sc.TOL, d_workspace=ws.buf, workspace_bytes=ws_bytes,
                      max_blocks=max_blocks, **p, **{"d_" + k: v.buf for k, v in o.items()})
    ctx.synchronize()
    x.free()
    what = f"shortcut n={n} problems={B} {over}"
    ws.take(what + " workspace")
    return {k: v.take(f"{what} {k}") for k, v in o.items()}


def _held_to_shortcut_twin(got, twin, B, what):
    import shortcut_cases as sc

    ref = {k: v[:B] for k, v in twin.items()}
    ref["gap"] = np.full(B, np.inf)
    return sc.check_against_oracle(got, ref, what, show=False)


@pytest.mark.parametrize("n", ch.NS)
def test_path_shortcut(ctx, planner, n):
    import shortcut_cases as sc

    case = ch.shortcut_case(n)
    wp, cnt, P = case["waypoints"], case["count"], ch.SHORTCUT_PROBLEMS
    worst = {}

    def note(fig):
        for k, v in fig.items():
            worst[k] = max(worst.get(k, 0.0), v)

    for tight in (False, True):
        over = {"max_waypoints": case["tight"]} if tight else {}
        twin = ch.shortcut_twin(n, tight)
        what = f"shortcut n={n}{' tight' if tight else ''}"
        for B in SHORTCUT_COUNTS if not tight else (P,):
            full = _shortcut(ctx, n, wp[:B], cnt[:B], **over)
            note(_held_to_shortcut_twin(full, twin, B, f"{what} kernel against the twin, {B} problems"))
        assert full["waypoints"].shape[1] == (case["tight"] if tight else sc.MAX_WAYPOINTS)
        sc.check_sound(planner, case, full, f"{what} kernel")
        _identical(_shortcut(ctx, n, wp, cnt, max_blocks=1, **over), full, f"{what} max_blocks 1")   # 73 problems on 64 lanes
        _identical(_shortcut(ctx, n, wp, cnt, blocks=1, **over), full, f"{what} workspace of one block")
        if n in ORACLE_NS:
            note(sc.check_against_oracle(full, ch.shortcut_oracle(n, tight=tight), f"{what} kernel against the oracle", show=False))
        if tight:
            assert (full["skipped_full"].sum() > 0) == (n >= 2)
        else:
            clean = full
    cm = case["cm"]
    narrow = np.ascontiguousarray(wp[:, :sc.MAX_WAYPOINTS])                 # w_in = max_waypoints: no input row to spare
    want = _hip.cpu_path_shortcut(cm.model, cm.handle, narrow, cnt, sc.MARGIN, sc.TOL, **ch.shortcut_params(n))
    note(_held_to_shortcut_twin(_shortcut(ctx, n, narrow, cnt), want, P, f"shortcut n={n} w_in = max_waypoints"))
    none = _shortcut(ctx, n, wp, cnt, max_iters=0)
    _held_to_shortcut_twin(none, ch.shortcut_twin(n, max_iters=0), P, f"shortcut n={n} max_iters 0")
    assert none["evaluations"].max() == 0 and none["iterations"].max() == 0
    src = int(np.argmax(cnt[:ch.PLAN_PROBLEMS]))          # the longest solved path stands on the three poisoned rows
    base, bad = wp.copy(), cnt.copy()
    base[BAD], bad[BAD] = wp[src], cnt[src]
    ok = _shortcut(ctx, n, base, bad)
    assert (ok["status"][BAD] == clean["status"][src]).all() and (ok["count"][BAD] == clean["count"][src]).all()
    base[BAD[0], 0, 0], base[BAD[1], 1, (n - 1) // 2], base[BAD[2], cnt[src] - 1, n - 1] = np.nan, np.inf, -np.inf
    dirty = _shortcut(ctx, n, base, bad)
    assert (dirty["status"][BAD] == sc.INVALID).all()
    for k in sc.KEYS:
        assert np.isnan(dirty[k][BAD]).all() if k in _SC_REAL else k == "status" or (dirty[k][BAD] == 0).all(), k
    _identical(dirty, ok, f"shortcut n={n} beside non-finite problems", np.setdiff1d(np.arange(P), BAD))
    _identical(ok, clean, f"shortcut n={n} beside replaced problems", np.setdiff1d(np.arange(P), BAD))
    print(f"\nshortcut n={n}: kernel against twin{' and oracle' if n in ORACLE_NS else ''}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items())
          + f" (bounds {sc.WAYPOINT_BOUND:.3g}, {sc.LENGTH_BOUND:.3g})")


# ------------------------------------------------------------------------------------------------ mp_path_blend_f64
# k_path_blend<n> and k_path_blend_sample<n> on chain_cases.blend_case(n): 145 problems (two waves and 17 lanes), 145 x 33 grid rows of
# 8 n bytes each - for n = 1, 3, 5, 7 no multiple of 16 bytes - stored whole tiles at a time.  The device runs are test_gpu_blend.py's
# (fresh 0xFF buffers, a guard band behind every output).
def _shares(figures, bound):
    return ", ".join(f"{k} {v / bound[k] if bound[k] else 0.0:.2g}" for k, v in figures.items())


@pytest.mark.parametrize("run", ("base", "raised"))
@pytest.mark.parametrize("n", ch.NS)
def test_path_blend(ctx, n, run):
    """Every discrete output of every problem equals the twin's (gap = inf: nobody is excused) and the float64 oracle's, the real ones
    lie within blend_cases.BOUND of both; NaN outside DONE / STRAIGHT / POINT; the end rows of the grid are the input's end waypoints
    bit for bit; 64 lanes serving all 145 problems give the full launch's bits."""
    case, B = ch.blend_case(n), ch.BLEND_PROBLEMS
    got = gb.device_run(ctx, case, run=run)
    what = f"blend n={n} {run} kernel against the"
    tw = bc.check_against_oracle(got, dict(ch.blend_twin(n, run), gap=np.full(B, np.inf)), f"{what} twin", show=False)
    ora = bc.check_against_oracle(got, ch.blend_oracle(n, run), f"{what} oracle", show=False)
    print(f"\nblend n={n} {run}: share of the bound: against the twin {_shares(tw, bc.BOUND)}; against the oracle {_shares(ora, bc.BOUND)}")
    st = got["status"]
    assert st[ch.BLEND_PLANTED_COLLINEAR] == bc.DONE and (n == 1 or {bc.DONE, bc.STRAIGHT, bc.SKIPPED, bc.POINT, bc.REVERSAL, bc.INVALID}
                                                           <= set(st.tolist()))
    assert n == 1 or (run == "raised") == bool((st == bc.BLOCKED).any())
    path = np.isin(st, (bc.DONE, bc.STRAIGHT, bc.POINT))
    for k in bc.REAL:
        assert np.isnan(got[k][~path]).all(), k
    curve = np.flatnonzero((st == bc.DONE) | (st == bc.STRAIGHT))
    assert np.array_equal(got["q"][curve, 0], case["waypoints"][curve, 0])
    assert np.array_equal(got["q"][curve, -1], case["waypoints"][curve, case["count"][curve] - 1])
    gb._same(gb.device_run(ctx, case, run=run, max_blocks=1), got)


# ------------------------------------------------------------------------------------------------ mp_trajectory_sample_f64
# k_traj_sample<n, source, torques> on chain_cases.sample_curve_case / sample_grid_case through test_gpu_sample.py's device run.
SAMPLE_GPU_KEYS = (("curve",), ("grid", 33, True), ("grid", 3, False))
WRENCH = np.array([0.3, -0.2, 0.1, 4.0, -3.0, 2.0])


@pytest.mark.parametrize("n", ch.NS)
def test_trajectory_sample(ctx, n):
    """Both sources at M and at M_SMALL: status, count and needed equal the twin's and the oracle's on every path, the real outputs lie
    within sample_cases.BOUND of both, the torques follow the existing inverse dynamics at the returned rows, dead paths are NaN and
    live ones finite; one block walking all the tiles gives the full launch's bits."""
    worst = {}
    for short in SAMPLE_GPU_KEYS:
        key = short[:1] + (n,) + short[1:]
        case = ch.sample_case(key)
        for small in (False, True):
            got = gs.device_run(ctx, case, sp.M_SMALL if small else None)
            label = f"{case['name']} M {got['s'].shape[1]} kernel"
            figs = (sp.check(got, ch.sample_twin(key, small), label + " against the twin", show=False),
                    sp.check(got, ch.sample_oracle(key, small), label + " against the oracle", show=False))
            for k in sp.REAL:
                worst[k] = max(worst.get(k, 0.0), figs[0][k], figs[1][k])
            sp.check_torques(case, got, label)
            dead = ~np.isin(got["status"], (sp.OK, sp.TRUNCATED))
            assert dead.any() and not dead.all()
            for k in sp.REAL:
                assert np.isnan(got[k][dead]).all() and np.isfinite(got[k][~dead]).all(), k
            if not small:
                gs._same(gs.device_run(ctx, case, max_blocks=1), got)
    print(f"\nsampling n={n}: kernel against twin and oracle, share of the bound: {_shares(worst, sp.BOUND)}")


# The torques: up to 6 joints k_traj_sample's torque instances write them in the same launch; from 7 joints on the entry runs
# k_traj_sample without torques and k_id over its rows, whatever outputs the caller asks for (rows it did not ask for live in the
# context's pool for the call), and dispatches no torque instance: k_traj_sample<8, grid, torques with a wrench> wrote behind its
# arrays, and MANIPULAPY_HIP_SAMPLE_TORQUES, which used to force such an instance, is no longer read.
@pytest.mark.parametrize("n", ch.NS)
def test_trajectory_sample_torque_variants(ctx, n, monkeypatch):
    """Three ways to the torques on the N = 33 grid case, without and with a tip wrench: the full call, a torques-only call, and the
    full call with MANIPULAPY_HIP_SAMPLE_TORQUES=fused in the environment.  Up to 6 joints the three torque arrays agree bit for bit.
    From 7 joints on the last two agree bit for bit, follow the inverse-dynamics twin at the returned rows and lie within the rule's
    bound of the full call.  s, sd, sdd and the rows are the same bits in every variant, the launch without torques, a call for the
    positions and the torques alone and the call with the wrench included."""
    case = ch.sample_grid_case(n, 33, True)
    rest = tuple(k for k in sp.KEYS if k != "torques")
    bare = None
    for F in (None, WRENCH):
        what = f"sampling n={n} wrench {F is not None}"
        full = gs.device_run(ctx, case, Ftip=F)
        alone = gs.device_run(ctx, case, want=("torques",), Ftip=F)
        monkeypatch.setenv("MANIPULAPY_HIP_SAMPLE_TORQUES", "fused")
        forced = gs.device_run(ctx, case, Ftip=F)
        monkeypatch.delenv("MANIPULAPY_HIP_SAMPLE_TORQUES")
        gs._same(forced, full, rest)
        gs._same(gs.device_run(ctx, case, want=rest, Ftip=F), full, rest)
        gs._same(gs.device_run(ctx, case, want=("positions", "torques"), Ftip=F), forced, ("positions", "torques"))
        gs._same(alone, forced, ("torques",))
        sp.check_torques(case, full, what + " full call", Ftip=F)
        if n <= 6:
            gs._same(forced, full, ("torques",))
        else:
            for got, how in ((forced, "with the variable set"), (dict(full, torques=alone["torques"]), "torques alone")):
                sp.check_torques(case, got, f"{what} {how}", Ftip=F)
                sp.check({"torques": got["torques"]}, full, f"{what} {how} against the full call", show=False, keys=("torques",))
        if F is None:
            bare = full
    gs._same(full, bare, rest)
    assert not np.array_equal(full["torques"], bare["torques"], equal_nan=True)
    curve = ch.sample_curve_case(n)     # the curve source with the wrench
    full = gs.device_run(ctx, curve, Ftip=WRENCH)
    sp.check_torques(curve, full, f"sampling n={n} curve with the wrench", Ftip=WRENCH)
    gs._same(gs.device_run(ctx, curve, want=("torques",), Ftip=WRENCH), full, ("torques",))


# ------------------------------------------------------------------------------------------------ blend -> time -> sample
def _chain_planner(n, backend):
    import manipulapy_amd as mp

    tb, _, lim, _ = ch.chain(n)
    dyn = mp.ManipulatorDynamics(M_list=tb.M_ee, omega_list=None, r_list=None, b_list=None, S_list=tb.S, B_list=tb.S.copy(), Glist=tb.G,
                                 Mlist_per_link=tb.Mcom)
    return mp.OptimizedTrajectoryPlanning(dyn, None, dyn, lim, use_cuda=None if backend == "hip" else False)


@pytest.mark.parametrize("n", ch.NS)
def test_blend_time_sample_chain(ctx, n, monkeypatch):
    """batch_time_optimal_trajectory - batch_blend_path, the TOPP-RA parameterisation of its DONE / STRAIGHT rows, then
    batch_sample_time_optimal on the blended curves - on the first 16 inputs of blend_case(n), "hip" backend against "numpy": the blend
    under blend_cases' rule with nobody excused, the timing's status and sd2, and the sampler on "hip" on the NumPy backend's blend and
    timing under sample_cases' rule (the two timings differ by rounding, which the sampler's rule does not cover)."""
    import manipulapy_amd as mp

    monkeypatch.setenv("MANIPULAPY_HIP_SPECIALIZE", "0")       # (the float32 specialisation has no part in these float64 families)
    case, B = ch.blend_case(n), 16
    wp, cnt, cm = case["waypoints"][:B], case["count"][:B], case["cm"]
    dt, vl, inf = ch.sample_curve_case(n)["dt"], np.full(n, 2.0), np.tile([-np.inf, np.inf], (n, 1))
    runs = {}
    for backend in ("numpy", "hip"):
        with mp.use_backend(backend):
            pl = _chain_planner(n, backend)
            before = pl.performance_stats["gpu_calls"]
            runs[backend] = pl.batch_time_optimal_trajectory(wp, cnt, cm, bc.GRID, dt, vl, torque_limits=inf, acceleration_limits=np.full(n, 10.0),
                                                             margin=bc.RUNS["base"], tol=bc.TOL, g=ch.G9, **bc.params_of())
            assert (pl.performance_stats["gpu_calls"] - before >= 3) == (backend == "hip")      # three launches, none on the host
    cpu, gpu = runs["numpy"], runs["hip"]
    gb._same(cpu["blend"], {k: v[:B] for k, v in ch.blend_twin(n).items()})
    bc.check_against_oracle(gpu["blend"], dict(cpu["blend"], gap=np.full(B, np.inf)), f"n={n} planner blend on hip against numpy", show=False)
    st = gpu["blend"]["status"]
    curve = (st == bc.DONE) | (st == bc.STRAIGHT)
    assert curve.any() and (~curve).any()        # (12, 5, 14, 7, 2, 5, 6, 1 of the 16 rows have a curve, n = 1..8)
    assert np.array_equal(gpu["timing"]["status"], cpu["timing"]["status"]) and (gpu["timing"]["status"][curve] == 0).all()
    assert (gpu["timing"]["status"][~curve] == -1).all()
    tc.f64_rule(gpu["timing"]["sd2"][curve], cpu["timing"]["sd2"][curve], f"n={n} planner sd2 on hip against numpy")
    moving = np.isfinite(cpu["timing"]["duration"])
    assert np.array_equal(moving, np.isfinite(gpu["timing"]["duration"])) and moving.any()
    sam = gpu["samples"]["status"]
    assert (sam[moving] == sp.OK).all() and (sam[curve & ~moving] == sp.STOPS).all() and (sam[~curve] == sp.UNTIMED).all()
    with mp.use_backend("hip"):
        again = pl.batch_sample_time_optimal(cpu["timing"], dt, curve=cpu["blend"], velocity_limits=vl, g=ch.G9)
    sp.check({k: again[k] for k in sp.KEYS}, {k: cpu["samples"][k] for k in sp.KEYS}, f"n={n} planner samples on hip against numpy", show=False)
    sp.check_torques(dict(ch.sample_curve_case(n), model=pl._hip_model()), again, f"n={n} planner samples on hip")
