"""Shared by test_entry_faults_host.py and test_gpu_entry_faults.py: the single-fault calls of the float64 entries that came before the
sphere model (operational space, derivatives, VJPs, kinematics VJP, regressor, roll-out VJP, iLQR, TOPP-RA, inverse kinematics, PD
regulation, mass matrix, forward dynamics) in their three flavours - the CPU twins (`cpu`), the host-array entries of a context
(`host`) and the device-pointer entries (`device`) - with the code and the exact text each must answer.  sphere_entry_faults.py
holds the same for the sphere-model entries.

Every call is made through the C ABI with the argument list of _hip.SIGNATURES, on one row or problem of the 3-joint chain of
chain_cases.py (two knots for iLQR and the roll-out VJP, three for TOPP-RA, one line-search candidate): all arguments good but the
ones the fault names.  The texts are written out here, not taken from the library: they are what callers have seen so far and what a
change of the entry layer must keep byte for byte.  Where an entry hands its arguments on to another one, the text carries that
entry's name and is written out in full.  Each entry also records what a call with nothing wrong answers (0) and what a call with a
zero count and every array null answers, and `floor`, the number of faults its list must hold."""
import ctypes
import functools

import numpy as np

import chain_cases as ch
from manipulapy_amd import _hip

N = 3
INVALID, UNSUPPORTED = 1, 4
BYTES = 256                               # room of an array argument: one problem fits, and so does a start 8 bytes in
SIZES = {"Y": 1024, "K": 512, "work": 65536}   # the three a problem needs more for: the regressor, the iLQR gains, the normal-form workspace
BIG = "not available for models with more than 8 joints (this one has 9)"
ALIGN = "device pointers must be 16-byte aligned"
POINTER = {"cpu": "null pointer", "host": "null host pointer", "device": "null device pointer"}
ROWS3 = "the three row outputs must all be given or all be null"

SCALARS = {"frame": 0, "task": 1, "damping": 0.1, "rows": 1, "B": 1, "A": 1, "N": 2, "dt": 0.01, "intRes": 1, "steps": 1, "runs": 1, "n": N,
           "eomg": 0.01, "ev": 0.001, "max_iterations": 1, "step_cap": 0.5, "w_o": 1.0, "w_p": 1.0, "adaptive": 0, "backtracking": 0,
           "seed": 7, "nthreads": 1}
# arrays that are host memory in every flavour, and what a good call holds in them (None: the argument is optional and left out)
HOST_ALWAYS = {"g": None, "Ftip": None, "wq": np.zeros(2 * N), "wr": np.zeros(N), "wf": np.zeros(2 * N), "vlim": np.ones(N),
               "tlim": np.tile([-1.0, 1.0], N), "alim": np.ones(N), "joint_limits": np.tile([-1.0, 1.0], N)}
LEFT_OUT = ("Ftipmat", "Amat")             # optional device / host arrays a good call leaves out
# what a fault puts in place of a good host vector
BAD = {"nan6": np.array([0, 0, 0, 0, np.nan, 0.0]), "inf3": np.array([0, np.inf, 0.0]), "zero3": np.array([1.0, 0.0, 1.0]),
       "inf_v3": np.array([1.0, 1.0, np.inf]), "crossed": np.array([-1.0, 1.0, 1.0, -1.0, -1.0, 1.0]),
       "nan_pair": np.array([-1.0, 1.0, -1.0, np.nan, -1.0, 1.0])}


def _entry(stem, flavour, tm=False):
    return f"mp_{stem}_{ {'cpu': 'cpu_', 'host': 'host_', 'device': 'tm_' if tm else ''}[flavour] }f64"


def _spec(flavour, entry, args, zero_count, floor, need=(), align=(), more=(), gate=True, zero=(0, ""), vals=None, model=True):
    """one entry: `args` the C signature's names without the context and the thread count, `need` the arrays whose absence answers
    the flavour's null-pointer text, `align` those a device entry wants 16-byte aligned, `more` its other faults, `gate` whether it
    refuses models of more than 8 joints, `zero` (code, text) of the zero-count call, `vals` the good scalars that differ from SCALARS"""
    gpu = flavour != "cpu"
    names = (["ctx"] if gpu else []) + args.split() + ([] if gpu else ["nthreads"])
    faults = []
    if model and gpu:
        faults += [(f"null {k}", {k: None}, INVALID, "null context or model") for k in ("ctx", "model")]
    elif model:
        faults.append(("null model", {"model": None}, INVALID, "null model"))
    if model and gate:
        faults.append(("a 9-joint model", {"model": "big"}, UNSUPPORTED, BIG))
    faults += list(more)
    faults += [(f"null {k}", {k: None}, INVALID, POINTER[flavour]) for k in need]
    if flavour == "device":
        faults += [(f"misaligned {k}", {k: "misaligned"}, INVALID, ALIGN) for k in align]
    return dict(entry=entry, names=names, faults=faults, zero_count=zero_count, zero=zero, vals=vals or {}, floor=floor)


def _opspace(f):
    more = [("frame 3", {"frame": 3}, INVALID, "frame must be 0 (space), 1 (body) or 2 (hybrid), got 3"),
            ("task -1", {"task": -1}, INVALID, "task must be 0 (full), 1 (linear) or 2 (angular), got -1"),
            ("damping -1", {"damping": -1.0}, INVALID, "damping must be finite and >= 0"),
            ("damping nan", {"damping": float("nan")}, INVALID, "damping must be finite and >= 0"),
            ("negative rows", {"rows": -1}, INVALID, "negative row count")]
    outs = "T J Jdqd Lambda Jbar mu p"
    none = [("no output", {k: None for k in outs.split()}, INVALID, "at least one output is required")]
    return {"opspace": _spec(f, _entry("opspace", f), "model frame task damping q qd rows g " + outs, {"rows": 0}, {"cpu": 10, "host": 11, "device": 20}[f],
                             need=("q", "qd"), align=("q", "qd") + tuple(outs.split()), more=more + none),
            "opspace_torque": _spec(f, _entry("opspace_torque", f), "model frame task damping q qd acc tau0 rows g tau", {"rows": 0},
                                    {"cpu": 11, "host": 12, "device": 17}[f], need=("q", "qd", "acc", "tau"),
                                    align=("q", "qd", "acc", "tau0", "tau"), more=more)}


def _rows(f):
    """the per-row families whose only checks are the model, the row count and the pointers"""
    neg = [("negative rows", {"rows": -1}, INVALID, "negative row count")]
    out = {}
    for stem in ("id_derivatives", "fd_derivatives"):
        out[stem] = _spec(f, _entry(stem, f), "model q qd x rows g Ftip y dq dqd mat", {"rows": 0}, {"cpu": 8, "host": 9, "device": 16}[f],
                          need=("q", "qd", "x", "dq", "dqd"), align=("q", "qd", "x", "y", "dq", "dqd", "mat"), more=neg)
    out["id_vjp"] = _spec(f, _entry("id_vjp", f), "model q qd qdd gtau rows g Ftip gq gqd gqdd", {"rows": 0}, {"cpu": 9, "host": 10, "device": 17}[f],
                          need=("q", "qd", "qdd", "gtau", "gq", "gqd"), align=("q", "qd", "qdd", "gtau", "gq", "gqd", "gqdd"), more=neg)
    out["fd_vjp"] = _spec(f, _entry("fd_vjp", f), "model q qd tau gqdd rows g Ftip qdd gq gqd gtau", {"rows": 0}, {"cpu": 9, "host": 10, "device": 18}[f],
                          need=("q", "qd", "tau", "gqdd", "gq", "gqd"), align=("q", "qd", "tau", "gqdd", "qdd", "gq", "gqd", "gtau"), more=neg)
    out["fk_jac_vjp"] = _spec(f, _entry("fk_jac_vjp", f), "model frame q gT gJ rows T J gq", {"rows": 0}, {"cpu": 6, "host": 7, "device": 13}[f],
                              need=("q",), align=("q", "gT", "gJ", "T", "J", "gq"),
                              more=neg + [("frame 2", {"frame": 2}, INVALID, "frame must be 0 (space) or 1 (body), got 2"),
                                          ("no output", {"T": None, "J": None, "gq": None}, INVALID, "at least one output is required")])
    out["id_regressor"] = _spec(f, _entry("id_regressor", f), "model q qd qdd rows g Ftip Y tau_ext", {"rows": 0}, {"cpu": 7, "host": 8, "device": 13}[f],
                                need=("q", "qd", "qdd", "Y"), align=("q", "qd", "qdd", "Y", "tau_ext"), more=neg)
    # the normal form wants b and rr at every row count, so its zero-count call with null arrays is refused
    out["id_regressor_normal"] = _spec(f, _entry("id_regressor_normal", f),
                                       "model q qd qdd rhs rows g Ftip " + ("work " if f == "device" else "") + "Amat b rr", {"rows": 0},
                                       {"cpu": 9, "host": 10, "device": 18}[f],
                                       need=("q", "qd", "qdd", "rhs", "b", "rr") + (("work",) if f == "device" else ()),
                                       align=("q", "qd", "qdd", "rhs", "work", "b", "rr"), more=neg, zero=(INVALID, POINTER[f]))
    out["mass_matrix"] = _spec(f, _entry("mass_matrix", f), "model q rows M", {"rows": 0}, {"cpu": 4, "host": 5, "device": 7}[f], need=("q", "M"),
                               align=("q", "M"), more=neg, gate=False)
    out["forward_dynamics"] = _spec(f, _entry("forward_dynamics", f), "model q qd tau rows g Ftip qdd", {"rows": 0}, {"cpu": 6, "host": 7, "device": 11}[f],
                                    need=("q", "qd", "tau", "qdd"), align=("q", "qd", "tau", "qdd"), more=neg, gate=False)
    return out


def _rollout_vjp(f):
    if f == "cpu":
        more = [("negative B", {"B": -1}, INVALID, "negative B or N"), ("negative N", {"N": -1}, INVALID, "negative B or N")]
    else:
        more = [("negative B", {"B": -1}, INVALID, "negative B (-1) or N (2)"), ("negative N", {"N": -1}, INVALID, "negative B (1) or N (-1)")]
    more.append(("intRes 0", {"intRes": 0}, INVALID, "intRes must be >= 1 (got 0)"))
    work = "work " if f == "device" else ""
    need = ("theta0", "dtheta0", "taumat", "gtheta0", "gdtheta0", "gtaumat") + (("work",) if f == "device" else ())
    return {"fd_trajectory_vjp": _spec(f, _entry("fd_trajectory_vjp", f, tm=True),
                                       "model theta0 dtheta0 taumat Ftipmat B N g dt intRes gpos gvel gacc " + work + "gtheta0 gdtheta0 gtaumat",
                                       {"B": 0}, {"cpu": 11, "host": 12, "device": 23}[f], need=need,
                                       align=("theta0", "dtheta0", "taumat", "gpos", "gvel", "gacc", "work", "gtheta0", "gdtheta0", "gtaumat"),
                                       more=more)}


def _ilqr(f):
    gpu = f != "cpu"
    weights = [(f"null {k}", {k: None}, INVALID, "null weight vector") for k in ("wq", "wr", "wf")]
    weights += [("non-finite wq", {"wq": "nan6"}, INVALID, "non-finite weight"), ("non-finite wr", {"wr": "inf3"}, INVALID, "non-finite weight"),
                ("non-finite wf", {"wf": "nan6"}, INVALID, "non-finite weight")]
    knots = [("N 1", {"N": 1}, INVALID, "N must be >= 2 (got 1)")]
    back = [("negative B", {"B": -1}, INVALID, "negative B (-1)" if gpu else "negative B")] + knots + weights
    # the weights are checked before the count by the twin and the device entry, after it by the host entries
    weights_first = (0, "") if f == "host" else (INVALID, "null weight vector")
    if f == "device":
        bargs = "model pos vel taumat dq dqd Minv xref wq wr wf reg B N dt work K k dV status"
        bneed = ("pos", "vel", "taumat", "dq", "dqd", "Minv", "xref", "reg", "K", "k", "dV", "status")
    else:
        bargs = "model pos vel taumat xref wq wr wf reg B N g dt K k dV status"
        bneed = ("pos", "vel", "taumat", "xref", "reg", "K", "k", "dV", "status")
    if gpu:
        roll = [("negative A", {"A": -1}, INVALID, "negative A (-1) or B (1)"), ("negative B", {"B": -1}, INVALID, "negative A (1) or B (-1)")]
        gains = [(f"{k} alone", {k: None}, INVALID, "K and k must both be given or both be null") for k in ("K", "k")]
        gains += [(f"gains without {k}", {k: None}, INVALID, "the gains need the nominal pos and vel") for k in ("pos", "vel")]
    else:
        roll = [("negative A", {"A": -1}, INVALID, "negative A"), ("negative B", {"B": -1}, INVALID, "negative B")]
        gains = [(f"gains without {k}", {k: None}, INVALID, "K and k must both be given, with the nominal pos and vel, or both be null")
                 for k in ("K", "k", "pos", "vel")]
    rows = [(f"no {k}", {k: None}, INVALID, ROWS3) for k in ("opos", "ovel", "otau")]
    rargs = "model theta0 dtheta0 taumat pos vel K k alpha xref wq wr wf A B N g dt cost opos ovel otau"
    return {"ilqr_backward": _spec(f, _entry("ilqr_backward", f, tm=True), bargs, {"B": 0}, {"cpu": 19, "host": 20, "device": 36}[f], need=bneed,
                                   align=bneed + ("work",), more=back, zero=weights_first),
            "ilqr_rollout": _spec(f, _entry("ilqr_rollout", f, tm=True), rargs, {"A": 0}, {"cpu": 24, "host": 25, "device": 38}[f],
                                  need=("theta0", "dtheta0", "taumat", "alpha", "xref", "cost"),
                                  align=("theta0", "dtheta0", "taumat", "pos", "vel", "K", "k", "alpha", "xref", "cost", "opos", "ovel", "otau"),
                                  more=roll + knots + weights + gains + rows, zero=weights_first)}


def _toppra(f):
    """path dynamics (twin and device entry), the sweep (twin and device entry) and the whole (twin and host entry); the whole's twin
    hands on to the other two twins, whose names its texts then carry"""
    gpu = f != "cpu"
    speed = [("null vlim", {"vlim": None}, INVALID, "null velocity limits"),
             ("zero vlim", {"vlim": "zero3"}, INVALID, "velocity limits must be finite and positive"),
             ("infinite vlim", {"vlim": "inf_v3"}, INVALID, "velocity limits must be finite and positive")]
    limits = [("crossed tlim", {"tlim": "crossed"}, INVALID, "torque limits must be ordered pairs (lo <= hi, either may be infinite)"),
              ("nan tlim", {"tlim": "nan_pair"}, INVALID, "torque limits must be ordered pairs (lo <= hi, either may be infinite)"),
              ("zero alim", {"alim": "zero3"}, INVALID, "acceleration limits must be positive")]
    knots = [("negative B", {"B": -1}, INVALID, "negative B (-1)" if gpu else "negative B"), ("N 2", {"N": 2}, INVALID, "N must be >= 3 (got 2)")]
    rows = [(f"no {k}", {k: None}, INVALID, ROWS3) for k in ("qd", "qdd", "tau")]
    deriv = [(f"no {k}", {k: None}, INVALID, "acceleration limits and the row outputs need the path derivatives dq and ddq") for k in ("dq", "ddq")]
    three = {"N": 3}
    out = {}
    if f != "host":
        arrays = ("q", "dq", "ddq", "a", "b", "c", "xbar")
        out["path_dynamics"] = _spec(f, _entry("path_dynamics", f), "model q dq ddq rows vlim g Ftip a b c xbar", {"rows": 0},
                                     {"cpu": 13, "device": 21}[f], need=arrays, align=arrays,
                                     more=[("negative rows", {"rows": -1}, INVALID, "negative row count")] + speed, zero=(INVALID, "null velocity limits"))
        need = ("a", "b", "c", "xbar", "sd_start", "sd_end", "K", "x", "u", "t", "duration", "status")
        sweep = "a b c xbar dq ddq tlim alim sd_start sd_end B N K x u t duration status qd qdd tau"
        if f == "cpu":
            size = [(f"n {k}", {"n": k}, UNSUPPORTED, "n must be 1..8") for k in (0, 9)]
            out["toppra_sweep"] = _spec(f, "mp_toppra_sweep_cpu_f64", "n " + sweep, {"B": 0}, 24, need=need, more=size + knots + limits + rows + deriv,
                                        vals=three, model=False)
        else:
            out["toppra_sweep"] = _spec(f, "mp_toppra_tm_f64", "model " + sweep, {"B": 0}, 42, need=need,
                                        align=need + ("dq", "ddq", "qd", "qdd", "tau"), more=knots + limits + rows + deriv, vals=three)
    if f != "device":
        whole = "model q dq ddq vlim tlim alim sd_start sd_end B N g Ftip K x u t duration status qd qdd tau"
        if f == "host":
            need = ("q", "dq", "ddq", "sd_start", "sd_end", "K", "x", "u", "t", "duration", "status")
            out["toppra"] = _spec(f, "mp_toppra_host_f64", whole, {"B": 0}, 25, need=need, more=knots + speed + limits + rows, vals=three,
                                  zero=(INVALID, "null velocity limits"))
        else:
            def said_by(entry, faults):
                return [(label, over, code, f"{entry}: {text}") for label, over, code, text in faults]
            path = said_by("mp_path_dynamics_cpu_f64", speed + [(f"null {k}", {k: None}, INVALID, "null pointer") for k in ("q", "dq", "ddq")])
            swept = ("sd_start", "sd_end", "K", "x", "u", "t", "duration", "status")
            sweep = said_by("mp_toppra_sweep_cpu_f64", limits + rows + [(f"null {k}", {k: None}, INVALID, "null pointer") for k in swept])
            out["toppra"] = _spec(f, "mp_toppra_cpu_f64", whole, {"B": 0}, 24, more=knots + path + sweep, vals=three,
                                  zero=(INVALID, "mp_path_dynamics_cpu_f64: null velocity limits"))
    return out


def _ik(f):
    """the host entry stages its arrays and hands on to the device entry, whose name the settings' texts then carry"""
    got = "" if f == "cpu" else " (got 0)"
    joint = "a joint has its lower limit above its upper limit" if f == "cpu" else "joint 1 has lower limit above upper limit"
    tolerances = "eomg, ev, step_cap must be positive and damping non-negative"
    settings = [("max_iterations 0", {"max_iterations": 0}, INVALID, "max_iterations must be at least 1" + got),
                ("eomg 0", {"eomg": 0.0}, INVALID, tolerances), ("ev 0", {"ev": 0.0}, INVALID, tolerances),
                ("damping -1", {"damping": -1.0}, INVALID, tolerances), ("step_cap 0", {"step_cap": 0.0}, INVALID, tolerances),
                ("crossed limits", {"joint_limits": "crossed"}, INVALID, joint)]
    if f == "host":
        settings = [(label, over, code, "mp_inverse_kinematics_f64: " + text) for label, over, code, text in settings]
    arrays = ("T_desired", "theta0", "theta", "success", "iterations", "restarts")
    return {"inverse_kinematics": _spec(f, _entry("inverse_kinematics", f),
                                        "model T_desired theta0 B joint_limits eomg ev max_iterations damping step_cap w_o w_p adaptive backtracking "
                                        "seed theta success iterations restarts", {"B": 0}, {"cpu": 14, "host": 15, "device": 18}[f],
                                        need=arrays, align=("T_desired", "theta0", "theta"), gate=False,
                                        more=[("negative B", {"B": -1}, INVALID, "negative problem count")] + settings)}


def _pd(f):
    if f == "device":
        return {}
    more = [("negative runs", {"runs": -1}, INVALID, "negative run or step count"), ("negative steps", {"steps": -1}, INVALID, "negative run or step count")]
    if f == "host":
        more.append(("dt nan", {"dt": float("nan")}, INVALID, "dt must be finite"))
    return {"pd_regulation": _spec(f, _entry("pd_regulation", f), "model theta0 theta_des Kp Kd runs g dt steps errors count", {"runs": 0},
                                   {"cpu": 9, "host": 11}[f], need=("theta0", "theta_des", "Kp", "Kd", "errors", "count"), more=more, gate=False)}


@functools.lru_cache(maxsize=None)
def entries(flavour):
    """{family: its entry of this flavour}; a family without an entry of this flavour is left out"""
    out = {}
    for family in (_opspace, _rows, _rollout_vjp, _ilqr, _toppra, _ik, _pd):
        out.update(family(flavour))
    return out


FAMILIES = {f: tuple(entries(f)) for f in ("cpu", "host", "device")}


@functools.lru_cache(maxsize=None)
def models():
    """(the chain's HipModel, a 9-joint model); made once and kept alive"""
    from test_random_robots import random_robot

    t = random_robot(np.random.default_rng(1), 9, ("general",))
    return ch.chain(N)[3], _hip.HipModel(t.S, t.Mcom, t.G, t.M_ee)


def arrays_of(spec):
    """the array arguments of an entry that are not host memory in every flavour"""
    return tuple(k for k in spec["names"] if k not in SCALARS and k not in HOST_ALWAYS and k not in ("ctx", "model"))


def host_arrays(spec):
    """{array argument: a zeroed host array with one good problem's room}; T_desired holds the identity; kept alive by the caller"""
    a = {k: np.zeros(SIZES.get(k, BYTES) // 8) for k in arrays_of(spec)}
    if "T_desired" in a:
        a["T_desired"][:16] = np.eye(4).ravel()
    return a


def good_values(spec, address, ctx=None):
    """{argument: value} of a call with nothing wrong; `address`: {array argument: its address}"""
    v = dict(SCALARS, model=models()[0].handle, ctx=None if ctx is None else ctx.handle, **HOST_ALWAYS)
    v.update(address)
    v.update(spec["vals"])
    v.update({k: None for k in LEFT_OUT})
    return v


def call(spec, values, over=()):
    """(code, text of mp_last_error) of the entry on `values` with the replacements of `over`"""
    lib = _hip.load_library()
    fn = getattr(lib, spec["entry"])
    names = spec["names"]
    assert len(names) == len(fn.argtypes), spec["entry"]
    v = dict(values)
    for k, x in dict(over).items():
        v[k] = v[k] + 8 if x == "misaligned" else models()[1].handle if x == "big" else BAD[x] if isinstance(x, str) else x
    args = []
    for name, typ in zip(names, fn.argtypes):
        x = v[name]
        if isinstance(x, np.ndarray):
            x = x.ctypes.data
        if typ in (_hip._vp, _hip._c_dp):
            x = getattr(x, "value", x)
            x = None if x is None else ctypes.cast(ctypes.c_void_p(x), typ)
        args.append(x)
    rc = fn(*args)
    return rc, (lib.mp_last_error() or b"").decode()


def said(spec, text):
    return text if text.startswith("mp_") else f"{spec['entry']}: {text}"


def check(spec, values):
    """the call with nothing wrong answers 0, the zero-count call with null arrays what the table says, and every fault of the entry
    its code and its text, byte for byte; the list is as long as the table's floor"""
    name = spec["entry"]
    assert call(spec, values)[0] == 0, f"{name}: the call with nothing wrong: {call(spec, values)}"
    nothing = dict(spec["zero_count"], **{k: None for k in arrays_of(spec) + tuple(HOST_ALWAYS)})
    rc, msg = call(spec, values, nothing)
    code, text = spec["zero"]
    assert rc == code and (code == 0 or msg == said(spec, text)), f"{name}, zero count and null arrays: code {rc}, {msg!r}"
    for label, over, code, text in spec["faults"]:
        rc, msg = call(spec, values, over)
        assert (rc, msg) == (code, said(spec, text)), f"{name}, {label}: code {rc}, {msg!r}"
    assert len(spec["faults"]) >= spec["floor"], f"{name}: {len(spec['faults'])} faults, the table's floor is {spec['floor']}"
