"""Shared by test_blend_host.py and test_gpu_blend.py: the single-fault calls of the corner-blending entries in their three flavours -
the CPU twin (`cpu`), the host-array entry of a context (`host`) and the device-pointer entry (`device`) - with the code and the exact
text each must answer, in the style of sphere_entry_faults.py (whose models, box-free helpers and constants are imported, not
modified).

Every call is made through the C ABI with the argument list of _hip.SIGNATURES, on one problem of the 3-joint chain of chain_cases.py:
all arguments good but the ones the fault names.  The texts are written out here, not taken from the library."""
import ctypes

import numpy as np

import sphere_entry_faults as sf
from manipulapy_amd import _hip

N, W_IN, GRID, BYTES = sf.N, sf.W_IN, 5, 1024
INVALID, UNSUPPORTED = sf.INVALID, sf.UNSUPPORTED
INPUTS, COUNT = ("waypoints_in", "count_in"), "B"
SETTINGS = ("W_in", "N", "blend", "max_halvings", "margin", "tol", "max_steps")
EXTRAS = ("max_blocks",)
OUTPUTS = ("status", "corner", "count", "points", "cut", "knot", "length", "halvings", "evaluations", "clearance", "q", "dq", "ddq")
TABLES = ("status", "count", "points", "cut", "knot", "length")   # what the device form's grid reads back
GOOD = {"W_in": W_IN, "N": GRID, "blend": 0.5, "max_halvings": 2, "margin": 0.01, "tol": 0.01, "max_steps": 64, "max_blocks": 0}
BAD_SETTINGS = (("margin nan", {"margin": float("nan")}, "margin must be finite"),
                ("tol 0", {"tol": 0.0}, "tol must be positive and finite"),
                ("max_steps 0", {"max_steps": 0}, "max_steps 0 outside 1..65536"),
                ("W_in 0", {"W_in": 0}, "0 input rows a path, outside 1..65536"),
                ("W_in 65537", {"W_in": 65537}, "65537 input rows a path, outside 1..65536"),
                ("N 2", {"N": 2}, "2 grid points, outside 3..65536"),
                ("N 65537", {"N": 65537}, "65537 grid points, outside 3..65536"),
                ("blend 0", {"blend": 0.0}, "blend must be positive and finite"),
                ("blend inf", {"blend": float("inf")}, "blend must be positive and finite"),
                ("max_halvings -1", {"max_halvings": -1}, "max_halvings -1 outside 0..32"),
                ("max_halvings 33", {"max_halvings": 33}, "max_halvings 33 outside 0..32"))
REQUIRED = "q, dq and ddq are sampled from status, count, points, cut, knot and length: all six are required with them"


def entry_name(flavour):
    return f"mp_path_blend_{'cpu_' if flavour == 'cpu' else 'host_' if flavour == 'host' else ''}f64"


def names_of(flavour):
    lead = ("model", "handle") if flavour == "cpu" else ("ctx", "model", "handle")
    return lead + INPUTS + (COUNT,) + SETTINGS + (EXTRAS if flavour == "device" else ()) + OUTPUTS + (("nthreads",) if flavour == "cpu" else ())


def host_arrays():
    """{array argument: a host array of BYTES bytes holding one good problem - three waypoints with a corner}; kept alive by the caller"""
    a = {k: np.zeros(BYTES // 8) for k in INPUTS + OUTPUTS}
    a["waypoints_in"][:W_IN * N] = np.array([[0.0, 0.0, 0.0], [0.05, 0.0, 0.0], [0.05, 0.05, 0.0], [0.05, 0.05, 0.0]]).reshape(-1)
    a["count_in"] = np.zeros(BYTES // 4, dtype=np.int32)
    a["count_in"][0] = 3
    return a


def good_values(address, ctx=None):
    model, handle, _, _ = sf.models()
    v = dict(GOOD, model=model.handle, handle=handle.handle, ctx=None if ctx is None else ctx.handle, nthreads=1, **address)
    v[COUNT] = 1
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
    out.append(("a negative count", {COUNT: -1}, INVALID, "negative problem count"))
    pointer = {"cpu": "null pointer", "host": "null host pointer", "device": "null device pointer"}[flavour]
    out += [(f"null {k}", {k: None}, INVALID, pointer) for k in INPUTS]
    out.append(("no output", {k: None for k in OUTPUTS}, INVALID, "at least one output is required"))
    if flavour == "device":
        out += [(f"misaligned {k}", {k: "misaligned"}, INVALID, "device pointers must be 16-byte aligned") for k in INPUTS + OUTPUTS]
        out.append(("negative max_blocks", {"max_blocks": -1}, INVALID, "negative max_blocks"))
        out += [(f"the grid without {k}", {k: None}, INVALID, REQUIRED) for k in TABLES]
    return out


def call(flavour, values, over=()):
    """(code, text of mp_last_error) of the entry on `values` with the replacements of `over`"""
    lib = _hip.load_library()
    fn = getattr(lib, entry_name(flavour))
    names = names_of(flavour)
    assert len(names) == len(fn.argtypes), entry_name(flavour)
    v = dict(values)
    for k, x in dict(over).items():
        v[k] = v[k] + 8 if x == "misaligned" else x
    args = []
    for name, typ in zip(names, fn.argtypes):
        x = v[name]
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
