"""The per-row device entries mp_forward_dynamics_{f32,f64}, mp_mass_matrix_f32 and mp_fk_jac_id_f32 on every kernel family they
dispatch to: the unrolled generic kernels (1..8 joints), the run-time-specialised ones (mp_model_specialize: mp_spec_fd_s / fd_d; the
mass matrix and float32 FK + Jacobian + ID have none and fall back to the generic kernels) and the run-time-n kernels (9..16 and
17..32 joints).  Every model runs as a generic model, specialised (up to 8 joints), and with a tip wrench (the HAS_FTIP = true
instantiations) and a non-default g.

The checker is a float64 reference that shares no code with the kernels: oracle/oracle.c up to 8 joints, the exact Newton-Euler
oracle oracle/newton_euler.py past that, on every row.  The bounds are those of
tests/test_row_dynamics_host.py (forward bound on the suite arms, backward bound on random chains); every launch's outputs have a
guard band behind them that must come back untouched.  Float32 inputs are rounded to float32 before the reference sees them."""
import numpy as np
import pytest

from conftest import ROBOTS
from oracle import c_oracle
from oracle import ref_numpy as ref
from test_gpu_parity import assert_f32
from test_random_robots import FLAVOURS, random_robot
from test_row_dynamics_host import (BWD_F32, F_ALT, FWD_F32, G_ALT, Reference, backward_ratio, f64_ratio, fd_rows,
                                    forward_ratio)

pytestmark = pytest.mark.gpu

ROWS = 1031                      # odd, past four 256-thread blocks
CHAINS = [f"n{n}" for n in range(1, 9)]
BIG = ["n9", "n12", "n14", "n16", "n17", "n32"]   # n14, n17, n32: prismatic joints (7, 12, 16) in both run-time-n instantiations
SPEC_CHAINS = (1, 5, 8)          # random chains also run specialised (hiprtc compiles each in 2-9 s; build() warms the suite arms only)
MODELS = ROBOTS + CHAINS + BIG
GUARD, PATTERN = 4096, 0xA5
WORST = {}                       # bound -> worst measured error ratio (printed when the module ends: pytest -s)


def record(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), float(ratio))
    return ratio


@pytest.fixture(scope="module")
def ctx():
    from manipulapy_amd import _hip

    c = _hip.HipContext(0)
    c.selftest()
    yield c
    c.destroy()
    if WORST:
        print("\nworst error / bound:", ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())))


class Case:
    """One robot: its tables, a generic and a specialised model (up to 8 joints), ROWS float32-exact rows and their reference."""

    def __init__(self, ctx, name, tables):
        from manipulapy_amd import _hip

        self.name = name
        if name in ROBOTS:
            self.tab, suite = tables[name], True
            rng = np.random.default_rng(300 + ROBOTS.index(name))
        else:
            n = int(name[1:])
            rng = np.random.default_rng(8800 + n)
            self.tab, suite = random_robot(rng, n, FLAVOURS[n % len(FLAVOURS)]), False   # n = 5, 6, 8, 17, 32: prismatic joints
        self.suite, self.n = suite, self.tab.n
        tab = self.tab
        self.model = _hip.HipModel(tab.S, tab.Mcom, tab.G, tab.M_ee, tab.joint_limits)
        self.spec = None
        if name in ROBOTS or self.n in SPEC_CHAINS:
            self.spec = _hip.HipModel(tab.S, tab.Mcom, tab.G, tab.M_ee, tab.joint_limits)
            ctx.specialize(self.spec)
            assert ctx.is_specialized(self.spec) and not ctx.is_specialized(self.model)
        self.q, self.qd, self.tau = fd_rows(rng, tab, ROWS, suite)
        self.qdd = rng.uniform(-3.0, 3.0, (ROWS, self.n)).astype(np.float32).astype(np.float64)
        self.ref = Reference(tab, self.q, self.qd)     # every row, at every joint count

    def variants(self):
        """(label, model, g, Ftip): generic, specialised (if it is), and both with a tip wrench + a non-default g."""
        out = [("generic", self.model, None, None), ("wrench", self.model, G_ALT, F_ALT)]
        if self.spec is not None:
            out += [("spec", self.spec, None, None), ("spec+wrench", self.spec, G_ALT, F_ALT)]
        return out


@pytest.fixture(scope="module")
def cases(ctx, tables):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(ctx, name, tables)
        return made[name]

    yield get
    for c in made.values():
        c.model.destroy()
        if c.spec is not None:
            c.spec.destroy()


def run(ctx, op, model, ins, outs, dtype, g=None, Ftip=None, rows=None):
    """Upload `ins` as `dtype`, launch `op` ("fd", "mm" or "fkjid") into outputs of shapes `outs` (None: not asked for), each
    followed by a GUARD-byte band filled with PATTERN; check the bands and return the outputs."""
    dtype = np.dtype(dtype)
    rows = ins[0].shape[0] if rows is None else rows
    d_in = [None if a is None else ctx.to_device(np.ascontiguousarray(a, dtype)) for a in ins]
    d_out, sizes = [], []
    for shp in outs:
        nb = 0 if shp is None else int(np.prod(shp)) * dtype.itemsize
        b = None if shp is None else ctx.alloc(nb + GUARD)
        if b is not None:
            ctx.memset(b, PATTERN, nb + GUARD)
        d_out.append(b)
        sizes.append(nb)
    try:
        if op == "fd":
            ctx.forward_dynamics(model, d_in[0], d_in[1], d_in[2], rows, d_out[0], g, Ftip, dtype=dtype)
        elif op == "mm":
            ctx.mass_matrix(model, d_in[0], rows, d_out[0], dtype=dtype)
        else:
            ctx.fk_jac_id(model, d_in[0], d_in[1], d_in[2], rows, *d_out, g=g, Ftip=Ftip, dtype=dtype)
        ctx.synchronize()
        res = []
        for b, nb, shp in zip(d_out, sizes, outs):
            if b is None:
                res.append(None)
                continue
            raw = b.download((nb + GUARD,), np.uint8)
            assert (raw[nb:] == PATTERN).all(), f"{op}: bytes written past the end of an output ({rows} rows)"
            res.append(raw[:nb].view(dtype).reshape(shp).copy())
        return res
    finally:
        for b in d_in + d_out:
            if b is not None:
                b.free()


def fd(ctx, model, q, qd, tau, dtype, g=None, Ftip=None):
    return run(ctx, "fd", model, (q, qd, tau), [q.shape], dtype, g, Ftip)[0]


# ------------------------------------------------------------------------------------------------ forward dynamics
@pytest.mark.parametrize("name", MODELS)
def test_forward_dynamics_f32_against_the_reference(name, ctx, cases):
    """mp_forward_dynamics_f32 on every family: the forward bound on the suite arms, the backward bound everywhere; the specialised
    kernel (mp_spec_fd_s) also against the generic float32 kernel."""
    c = cases(name)
    R, idx = c.ref, c.ref.idx
    got = {}
    for label, m, g, F in c.variants():
        qdd = fd(ctx, m, c.q, c.qd, c.tau, np.float32, g, F)
        got[label] = qdd
        assert np.isfinite(qdd).all(), label
        x = qdd[idx].astype(np.float64)
        bias = R.bias(g, F)
        r = record("fd_f32 backward", backward_ratio(R.M, x, c.tau[idx] - bias, bias, c.tau[idx]))
        assert r <= 1.0, f"{name} {label}: backward error {r:.3g} x the bound ({BWD_F32})"
        if c.suite:
            r = record("fd_f32 forward (suite)", forward_ratio(x, R.qdd(c.tau, g, F)))
            assert r <= 1.0, f"{name} {label}: forward error {r:.3g} x the bound ({FWD_F32})"
    for plain, special in (("generic", "spec"), ("wrench", "spec+wrench")) if c.spec is not None else ():
        a, b = got[plain].astype(np.float64), got[special].astype(np.float64)
        if c.suite:
            r = record("fd_f32 spec vs generic", (np.abs(b - a).max(axis=1) / (2e-5 * np.abs(a).max(axis=1))).max())
        else:
            r = record("fd_f32 spec vs generic (backward)", _spec_backward(R, a, b, c.tau))
        assert r <= 1.0, f"{name} {special}: specialised vs generic float32 {r:.3g} x the bound"


def _spec_backward(R, a, b, tau):
    """max|M_ref (b - a)| / (2e-5 * (max|M_ref| max|a| + max|tau|)) per row: two float32 solves of one ill-conditioned system agree
    in the torque they balance, not in qdd."""
    res = np.abs(np.einsum("rij,rj->ri", R.M, b - a)).max(axis=1)
    scale = np.abs(R.M).max(axis=(1, 2)) * np.abs(a).max(axis=1) + np.abs(tau).max(axis=1)
    return float((res / (2e-5 * scale)).max())


@pytest.mark.parametrize("name", MODELS)
def test_forward_dynamics_f64_device_form(name, ctx, cases):
    """mp_forward_dynamics_f64 called on device buffers: the suite's float64 rule against the reference, the specialised kernel
    (mp_spec_fd_d) within 1e-9 of the generic one, and the same bits as the host form (forward_dynamics_host)."""
    c = cases(name)
    R, idx = c.ref, c.ref.idx
    got = {}
    for label, m, g, F in c.variants():
        qdd = fd(ctx, m, c.q, c.qd, c.tau, np.float64, g, F)
        got[label] = qdd
        want = R.qdd(c.tau, g, F)
        if c.n <= 8:
            r = record("fd_f64 rule", f64_ratio(qdd[idx], want))
            assert r <= 1.0, f"{name} {label}: {r:.3g} x the float64 rule"
        else:   # the backward form at the float64 rule's 1e-7, as before, and (the oracle is exact past 8 joints too) the forward rule
            bias = R.bias(g, F)
            r = record("fd_f64 backward (9..32)", backward_ratio(R.M, qdd[idx], c.tau[idx] - bias, bias, c.tau[idx], 1e-7))
            assert r <= 1.0, f"{name} {label}: backward error {r:.3g} x 1e-7"
            r = record("fd_f64 rule (9..32)", f64_ratio(qdd[idx], want))
            assert r <= 1.0, f"{name} {label}: {r:.3g} x the float64 rule"
        host = ctx.forward_dynamics_host(m, c.q, c.qd, c.tau, g, F)
        np.testing.assert_array_equal(qdd, host, err_msg=f"{name} {label}: device form != host form")
    for plain, special in (("generic", "spec"), ("wrench", "spec+wrench")) if c.spec is not None else ():
        a, b = got[plain], got[special]
        np.testing.assert_allclose(b, a, rtol=1e-9, atol=1e-9 * max(1.0, float(np.abs(a).max())), err_msg=f"{name} {special}")


@pytest.mark.parametrize("name", ["ur5", "n3", "n8", "n12", "n17"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_forward_dynamics_row_counts(name, dtype, ctx, cases):
    """Row counts around the 256-thread blocks: each launch writes exactly its rows (guard band) and each row the same bits as in
    the full launch."""
    c = cases(name)
    for label, m, g, F in c.variants():
        full = fd(ctx, m, c.q, c.qd, c.tau, dtype, g, F)
        for rows in (1, 63, 64, 65, 255, 256, 257):
            part = fd(ctx, m, c.q[:rows], c.qd[:rows], c.tau[:rows], dtype, g, F)
            np.testing.assert_array_equal(part, full[:rows], err_msg=f"{name} {label} rows={rows}")


BAD_ROWS = [0, 1, 63, 64, 255, 256, 257, 511, 512, 700, ROWS - 1]


def _poison(x, rows):
    """Copies of the arrays in `x` with one NaN / +inf / -inf in each of `rows`, cycling over the arrays, the values and the joints."""
    x = [a.copy() for a in x]
    for i, r in enumerate(rows):
        x[i % len(x)][r, (3 * i) % x[0].shape[1]] = (np.nan, np.inf, -np.inf)[(i // len(x) + i) % 3]
    return x


@pytest.mark.parametrize("name", ["ur5", "iiwa14", "n5", "n8", "n9", "n17"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_forward_dynamics_nonfinite_rows(name, dtype, ctx, cases):
    """A NaN / inf in q, qd or tau of a row gives a NaN row; every other row keeps the bits of a clean launch.  The specialised
    kernels are compiled with -ffinite-math-only: the verdict must still hold there."""
    c = cases(name)
    q, qd, tau = _poison((c.q, c.qd, c.tau), BAD_ROWS)
    mask = np.zeros(ROWS, bool)
    mask[BAD_ROWS] = True
    for label, m, g, F in c.variants():
        clean = fd(ctx, m, c.q, c.qd, c.tau, dtype, g, F)
        dirty = fd(ctx, m, q, qd, tau, dtype, g, F)
        assert np.isnan(dirty[mask]).all(), f"{name} {label}: a row with a non-finite input is not NaN"
        np.testing.assert_array_equal(dirty[~mask], clean[~mask], err_msg=f"{name} {label}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_forward_dynamics_refusals(dtype, ctx, cases):
    from manipulapy_amd import _hip

    c = cases("ur5")
    item = np.dtype(dtype).itemsize
    rows, n = 64, c.n
    nb = rows * n * item
    bufs = [ctx.to_device(np.zeros(nb + 64, np.uint8)) for _ in range(4)]
    try:
        for m in (c.model, c.spec):
            for k in range(4):
                for off in (4, 8):
                    if off % item:
                        continue
                    ptr = [b.offset(off) if i == k else b for i, b in enumerate(bufs)]
                    with pytest.raises(_hip.HipError, match="16-byte aligned"):
                        ctx.forward_dynamics(m, ptr[0], ptr[1], ptr[2], rows, ptr[3], dtype=dtype)
            ctx.memset(bufs[3], PATTERN, nb + 64)
            ctx.forward_dynamics(m, bufs[0], bufs[1], bufs[2], 0, bufs[3], G_ALT, F_ALT, dtype=dtype)   # rows == 0: nothing happens
            ctx.synchronize()
            assert (bufs[3].download((nb + 64,), np.uint8) == PATTERN).all()
    finally:
        for b in bufs:
            b.free()


# ------------------------------------------------------------------------------------------------ mass matrix, float32
@pytest.mark.parametrize("name", ROBOTS + CHAINS)
def test_mass_matrix_f32_against_the_reference(name, ctx, cases):
    """mp_mass_matrix_f32 up to 8 joints: every row against the C oracle and a sample against ref_numpy at 3e-5 of the matrix's
    largest entry; a specialised model (no specialised mass-matrix kernel: the generic one) gives the same bits."""
    c = cases(name)
    shape = (ROWS, c.n, c.n)
    M = run(ctx, "mm", c.model, (c.q,), [shape], np.float32)[0].astype(np.float64)
    scale = np.abs(c.ref.M).max(axis=(1, 2), keepdims=True)
    r = record("mm_f32 (oracle)", (np.abs(M - c.ref.M) / (3e-5 * (np.abs(c.ref.M) + scale))).max())
    assert r <= 1.0, f"{name}: {r:.3g} x the bound"
    for i in range(0, ROWS, 97):
        want = ref.mass_matrix(c.tab, c.q[i])
        np.testing.assert_allclose(M[i], want, rtol=3e-5, atol=3e-5 * np.abs(want).max(), err_msg=f"{name} row {i}")
    if c.spec is not None:
        np.testing.assert_array_equal(run(ctx, "mm", c.spec, (c.q,), [shape], np.float32)[0], M.astype(np.float32))


@pytest.mark.parametrize("name", BIG)
def test_mass_matrix_f32_run_time_n(name, ctx, cases):
    """The run-time-n float32 mass matrix (9..16 and 17..32 joints): the store-path test's row counts with a guard band, against the
    float64 CPU launcher; every row against the Newton-Euler oracle."""
    from manipulapy_amd import _hip

    c = cases(name)
    n = c.n
    full = run(ctx, "mm", c.model, (c.q,), [(ROWS, n, n)], np.float32)[0].astype(np.float64)
    for i, r in enumerate(c.ref.idx):
        want = c.ref.M[i]
        rr = record("mm_f32 run-time n (oracle)", np.abs(full[r] - want).max() / (3e-5 * np.abs(want).max()))
        assert rr <= 1.0, f"{name} row {r}: {rr:.3g} x the bound"
    want = _hip.cpu_mass_matrix(c.model, c.q[:333])
    for rows in (1, 15, 16, 17, 31, 33, 63, 64, 65, 130, 333):
        got = run(ctx, "mm", c.model, (c.q[:rows],), [(rows, n, n)], np.float32)[0]
        np.testing.assert_allclose(got, want[:rows], rtol=3e-5, atol=3e-5 * np.abs(want[:rows]).max(), err_msg=f"{name} rows={rows}")
        np.testing.assert_array_equal(got, full[:rows].astype(np.float32))


@pytest.mark.parametrize("name", ["ur5", "panda", "n1", "n6", "n9", "n17", "n32"])
def test_mass_matrix_f32_nonfinite_rows(name, ctx, cases):
    c = cases(name)
    (q,) = _poison((c.q,), BAD_ROWS)
    mask = np.zeros(ROWS, bool)
    mask[BAD_ROWS] = True
    for m in (c.model,) if c.spec is None else (c.model, c.spec):
        clean = run(ctx, "mm", m, (c.q,), [(ROWS, c.n, c.n)], np.float32)[0]
        dirty = run(ctx, "mm", m, (q,), [(ROWS, c.n, c.n)], np.float32)[0]
        assert np.isnan(dirty[mask]).all()
        np.testing.assert_array_equal(dirty[~mask], clean[~mask])


# ------------------------------------------------------------------------------------------------ FK + Jacobian + ID, float32
def _tau_ref(c, g, F):
    """Reference torques of the case's rows (q, qd, qdd): the C oracle up to 8 joints, else M_ref qdd + bias_ref of the Newton-Euler
    oracle; every row."""
    if c.n <= 8:
        return c_oracle.inverse_dynamics_rows(c.tab, c.q, c.qd, c.qdd, ref.G_DEFAULT if g is None else g, F)[0]
    return np.einsum("rij,rj->ri", c.ref.M, c.qdd[c.ref.idx]) + c.ref.bias(g, F)


@pytest.mark.parametrize("name", ROBOTS + CHAINS + ["n9", "n14", "n16", "n17", "n32"])
def test_fk_jac_id_f32_against_the_reference(name, ctx, cases):
    """mp_fk_jac_id_f32 at ordinary sizes: T and J within 2e-5 (x max(1, max|J|) on random chains) of ref_numpy, tau under the
    suite's element-wise float32 rule against the reference; every output subset gives the bits of the full launch, each with its
    own guard band; a specialised model (no specialised float32 kernel) gives the generic bits."""
    c = cases(name)
    n = c.n
    shapes = [(ROWS, 4, 4), (ROWS, 6, n), (ROWS, n)]
    ins = (c.q, c.qd, c.qdd)
    sample = range(0, ROWS, 7)
    full = {}
    for label, m, g, F in c.variants():
        T, J, tau = full[label] = run(ctx, "fkjid", m, ins, shapes, np.float32, g, F)
        for i in sample:
            Tw, Jw = ref.fk_space(c.tab, c.q[i]), ref.jacobian_space(c.tab, c.q[i])
            tol = 2e-5 * (1.0 if c.suite else max(1.0, float(np.abs(Jw).max())))
            r = record("fkjid_f32 T, J", max(np.abs(T[i] - Tw).max(), np.abs(J[i] - Jw).max()) / tol)
            assert r <= 1.0, f"{name} {label} row {i}: T / J {r:.3g} x the bound"
        assert_f32(tau[c.ref.idx], _tau_ref(c, g, F))
        if label.startswith("spec"):
            plain = "generic" if label == "spec" else "wrench"
            for a, b in zip(full[label], full[plain]):
                np.testing.assert_array_equal(a, b, err_msg=f"{name} {label} vs {plain}")
            continue
        for k in range(3):
            sub = [s if j == k else None for j, s in enumerate(shapes)]
            part = run(ctx, "fkjid", m, ins if k == 2 else (c.q, None, None), sub, np.float32, g, F)
            np.testing.assert_array_equal(part[k], full[label][k], err_msg=f"{name} {label}: output {k} alone")


# ------------------------------------------------------------------------------------------------ graph capture
def test_float32_forward_dynamics_and_mass_matrix_in_a_graph(ctx, cases):
    """One float32 forward-dynamics launch and one mass-matrix launch on an 8-joint model captured into a graph (one stream, no
    parallel branches), replayed twice on new inputs: the bits of eager launches."""
    c = cases("panda")
    rng = np.random.default_rng(5)
    rows, n = 700, c.n
    item = 4
    d = [ctx.alloc(rows * n * item) for _ in range(3)]
    d_qdd, d_M = ctx.alloc(rows * n * item), ctx.alloc(rows * n * n * item)
    try:
        d[0].upload(c.q[:rows].astype(np.float32)); d[1].upload(c.qd[:rows].astype(np.float32)); d[2].upload(c.tau[:rows].astype(np.float32))
        with ctx.capture() as cap:
            ctx.forward_dynamics(c.model, d[0], d[1], d[2], rows, d_qdd, G_ALT, F_ALT, dtype=np.float32)
            ctx.mass_matrix(c.model, d[0], rows, d_M, dtype=np.float32)
        ctx.synchronize()
        for _ in range(2):
            q, qd, tau = fd_rows(rng, c.tab, rows, suite=True)
            for b, a in zip(d, (q, qd, tau)):
                b.upload(a.astype(np.float32))
            cap.graph.launch()
            ctx.synchronize()
            np.testing.assert_array_equal(d_qdd.download((rows, n), np.float32), fd(ctx, c.model, q, qd, tau, np.float32, G_ALT, F_ALT))
            np.testing.assert_array_equal(d_M.download((rows, n, n), np.float32), run(ctx, "mm", c.model, (q,), [(rows, n, n)], np.float32)[0])
        cap.graph.destroy()
    finally:
        for b in d + [d_qdd, d_M]:
            b.free()
