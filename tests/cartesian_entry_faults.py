"""Shared by test_cartesian_host.py and test_gpu_cartesian.py: the single-fault calls of the Cartesian-path entries in their three
flavours - the CPU twin (`cpu`), the host-array entry of a context (`host`) and the device-pointer entry (`device`) - with the code and
the exact text each must answer, in the style of blend_entry_faults.py (sphere_entry_faults' models, box and constants are imported,
not modified).

Every call is made through the C ABI with the argument list of _hip.SIGNATURES, on one problem of the 3-joint chain of chain_cases.py
with the position task: all arguments good but the ones the fault names.  The texts are written out here, not taken from the library."""
import ctypes

import numpy as np

import chain_cases as ch
import goal_cases as gc
import sphere_entry_faults as sf
from manipulapy_amd import _hip

N, GRID, BYTES = sf.N, 5, 1024
INVALID, UNSUPPORTED = sf.INVALID, sf.UNSUPPORTED
INPUTS, COUNT = ("q_start", "T_goal"), "B"
SETTINGS = ("lo", "hi", "N", "task", "eomg", "ev", "damping", "max_iters", "max_joint_step", "margin", "tol", "max_steps")
EXTRAS = ("workspace", "workspace_bytes", "max_blocks")
OUTPUTS = _hip.CARTESIAN_OUTPUTS
GRID_ROWS = ("q", "dq", "ddq")
GOOD = {"lo": "lo", "hi": "hi", "N": GRID, "task": 1, "eomg": 1e-6, "ev": 1e-6, "damping": 0.01, "max_iters": 20, "max_joint_step": 0.5,
        "margin": 0.01, "tol": 0.01, "max_steps": 64, "max_blocks": 0}
BAD_SETTINGS = (("margin nan", {"margin": float("nan")}, "margin must be finite"),
                ("tol 0", {"tol": 0.0}, "tol must be positive and finite"),
                ("max_steps 0", {"max_steps": 0}, "max_steps 0 outside 1..65536"),
                ("task 2", {"task": 2}, "task 2 is neither MP_TASK_FULL (0) nor MP_TASK_POSITION (1)"),
                ("N 1", {"N": 1}, "1 grid points, outside 2..65536"),
                ("N 65537", {"N": 65537}, "65537 grid points, outside 2..65536"),
                ("null box", {"lo": None}, "null joint box"),
                ("empty box", {"hi": "below"}, "joint 0: the box must be finite with lo <= hi"),
                ("eomg 0", {"eomg": 0.0}, "eomg and ev must be positive and finite"),
                ("ev inf", {"ev": float("inf")}, "eomg and ev must be positive and finite"),
                ("damping 0", {"damping": 0.0}, "damping must be positive and finite"),
                ("max_joint_step 0", {"max_joint_step": 0.0}, "max_joint_step must be positive and finite"),
                ("max_iters -1", {"max_iters": -1}, "max_iters -1 outside 0..65536"))
REQUIRED = "q, dq and ddq are what the spans are read from: all three are required"


def entry_name(flavour):
    return f"mp_cartesian_path_{'cpu_' if flavour == 'cpu' else 'host_' if flavour == 'host' else ''}f64"


def names_of(flavour):
    lead = ("model", "handle") if flavour == "cpu" else ("ctx", "model", "handle")
    return lead + INPUTS + (COUNT,) + SETTINGS + (EXTRAS if flavour == "device" else ()) + OUTPUTS + (("nthreads",) if flavour == "cpu" else ())


def host_arrays():
    """{array argument: a host array of BYTES bytes holding one good problem - a short line from the zero configuration}"""
    a = {k: np.zeros(BYTES // 8) for k in INPUTS + OUTPUTS}
    tb = ch.chain(N)[0]
    a["T_goal"][:16] = gc.fk_jacobian(np.asarray(tb.S, dtype=np.float64), np.asarray(tb.M_ee, dtype=np.float64),
                                      np.array([[0.05, 0.0, 0.05]]), np.float64)[0].reshape(16)
    return a


def good_values(address, ctx=None):
    model, handle, _, _ = sf.models()
    v = dict(GOOD, model=model.handle, handle=handle.handle, ctx=None if ctx is None else ctx.handle, nthreads=1, **address)
    v[COUNT] = 1
    v["workspace_bytes"] = _hip.cartesian_path_workspace_bytes(1, GRID)
    return v


def faults(flavour):
    """(label, {argument: replacement}, code, text behind "<entry>: ") of every single fault of the entry"""
    _, _, other, big = sf.models()
    gpu = flavour != "cpu"
    null = "null context, model or collision handle" if gpu else "null model or collision handle"
    out = [(f"null {k}", {k: None}, INVALID, null) for k in (("ctx",) if gpu else ()) + ("model", "handle")]
    out.append(("a 9-joint model", {"model": big.handle}, UNSUPPORTED, sf.BIG))
    out.append(("a handle of another joint count", {"handle": other.handle}, INVALID,
                "the collision handle was made for a model of 2 joints" + (", this one has 3" if gpu else "")))
    out += [(label, over, INVALID, text) for label, over, text in BAD_SETTINGS]
    out.append(("the full task on three joints", {"task": 0}, UNSUPPORTED, "a task of 6 rows needs at least 6 joints (this model has 3)"))
    out.append(("a negative count", {COUNT: -1}, INVALID, "negative problem count"))
    pointer = {"cpu": "null pointer", "host": "null host pointer", "device": "null device pointer"}[flavour]
    out += [(f"null {k}", {k: None}, INVALID, pointer) for k in INPUTS]
    if flavour == "device":
        out += [(f"without {k}", {k: None}, INVALID, REQUIRED) for k in GRID_ROWS]
        out += [(f"misaligned {k}", {k: "misaligned"}, INVALID, "device pointers must be 16-byte aligned")
                for k in INPUTS + OUTPUTS + ("workspace",)]
        out.append(("negative max_blocks", {"max_blocks": -1}, INVALID, "negative max_blocks"))
        need = _hip.cartesian_path_workspace_bytes(1, GRID)
        out.append(("no workspace", {"workspace": None}, INVALID,
                    f"the workspace holds 0 bytes, the call needs {need} (mp_cartesian_path_workspace_bytes)"))
        out.append(("a short workspace", {"workspace_bytes": need - 16}, INVALID,
                    f"the workspace holds {need - 16} bytes, the call needs {need} (mp_cartesian_path_workspace_bytes)"))
    else:
        out.append(("no output", {k: None for k in OUTPUTS}, INVALID, "at least one output is required"))
    return out


def call(flavour, values, over=()):
    """(code, text of mp_last_error) of the entry on `values` with the replacements of `over`"""
    lib = _hip.load_library()
    fn = getattr(lib, entry_name(flavour))
    names = names_of(flavour)
    assert len(names) == len(fn.argtypes), entry_name(flavour)
    v, bx = dict(values), sf.box()
    for k, x in dict(over).items():
        v[k] = v[k] + 8 if x == "misaligned" else x
    args = []
    for name, typ in zip(names, fn.argtypes):
        x = bx[v[name]].ctypes.data if name in ("lo", "hi") and v[name] is not None else v[name]   # (the box is always a host array)
        if typ in (_hip._vp, _hip._c_dp):
            x = getattr(x, "value", x)
            x = None if x is None else ctypes.cast(ctypes.c_void_p(x), typ)
        args.append(x)
    rc = fn(*args)
    return rc, (lib.mp_last_error() or b"").decode()


def check(flavour, values):
    """every fault of the entry answers its code and its text, byte for byte"""
    name = entry_name(flavour)
    seen = faults(flavour)
    for label, over, code, text in seen:
        rc, msg = call(flavour, values, over)
        assert (rc, msg) == (code, f"{name}: {text}"), f"{name}, {label}: code {rc}, {msg!r}"
    return len(seen)
