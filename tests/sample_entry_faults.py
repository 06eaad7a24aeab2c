"""Shared by test_sample_host.py and test_gpu_sample.py: the single-fault calls of the trajectory-sampling entries in their three
flavours - the CPU twin (`cpu`), the host-array entry of a context (`host`) and the device-pointer entry (`device`) - with the code
and the exact text each must answer, in the style of blend_entry_faults.py (whose models and constants, sphere_entry_faults.py's, are
imported, not modified).

Every call is made through the C ABI with the argument list of _hip.SIGNATURES, on one timed path of the 3-joint chain of
chain_cases.py with N = 3 grid points, T = 1 and dt = 0.25 (five rows), in either source: all arguments good but the ones the fault
names.  The texts are written out here, not taken from the library."""
import ctypes

import numpy as np

import sphere_entry_faults as sf
from manipulapy_amd import _hip

N, W_IN, GRID, ROWS, BYTES = sf.N, 4, 3, 5, 1024
INVALID, UNSUPPORTED = sf.INVALID, sf.UNSUPPORTED
TIMING, COUNT = ("t", "x"), "B"
GRID_SOURCE = ("q", "dq", "ddq")
CURVE_SOURCE = ("blend_status", "blend_count", "points", "cut", "knot", "length")
OUTPUTS = ("status", "count", "needed", "s", "sd", "sdd", "positions", "velocities", "accelerations", "torques")
GOOD = {"N": GRID, "dt": 0.25, "M": ROWS, "g": None, "Ftip": None, "max_blocks": 0}
BAD_SETTINGS = (("N 2", {"N": 2}, "2 grid points, outside 3..2^31-1"),
                ("N 2^31", {"N": 2 ** 31}, "2147483648 grid points, outside 3..2^31-1"),
                ("dt 0", {"dt": 0.0}, "dt must be positive and finite"),
                ("dt negative", {"dt": -0.25}, "dt must be positive and finite"),
                ("dt inf", {"dt": float("inf")}, "dt must be positive and finite"),
                ("dt nan", {"dt": float("nan")}, "dt must be positive and finite"),
                ("M 0", {"M": 0}, "0 sample rows a path, outside 1..2^31-1"),
                ("M 2^31", {"M": 2 ** 31}, "2147483648 sample rows a path, outside 1..2^31-1"),
                ("rows past the address space", {"B": 2 ** 58}, "288230376151711744 paths of 5 rows and 3 grid points are not addressable"))
ALL_THREE = "the grid source needs q, dq and ddq, all three"
ALL_SIX = "the curve source needs status, count, points, cut, knot and length, all six"
ONE_SOURCE = "exactly one source of the geometry must be given, the grid or the curve"


def entry_name(flavour):
    return f"mp_trajectory_sample_{'cpu_' if flavour == 'cpu' else 'host_' if flavour == 'host' else ''}f64"


def names_of(flavour):
    lead = ("model",) if flavour == "cpu" else ("ctx", "model")
    return (lead + TIMING + (COUNT, "N") + GRID_SOURCE + CURVE_SOURCE + ("W_in", "dt", "M", "g", "Ftip") +
            (("max_blocks",) if flavour == "device" else ()) + OUTPUTS + (("nthreads",) if flavour == "cpu" else ()))


def host_arrays():
    """{array argument: a host array of BYTES bytes holding one good path in both sources}; kept alive by the caller"""
    a = {k: np.zeros(BYTES // 8) for k in TIMING + GRID_SOURCE + CURVE_SOURCE + OUTPUTS}
    a["t"][:GRID] = [0.0, 0.5, 1.0]
    a["x"][:GRID] = [0.0, 4.0, 0.0]
    a["q"][:GRID * N] = np.array([[0.0, 0.0, 0.0], [0.05, 0.02, 0.0], [0.1, 0.05, 0.0]]).reshape(-1)
    a["dq"][:GRID * N] = np.array([[0.1, 0.0, 0.0], [0.1, 0.05, 0.0], [0.1, 0.1, 0.0]]).reshape(-1)
    for k in ("blend_status", "blend_count"):
        a[k] = np.zeros(BYTES // 4, dtype=np.int32)
    a["blend_count"][0] = 3
    a["points"][:W_IN * N] = np.array([[0.0, 0.0, 0.0], [0.05, 0.0, 0.0], [0.05, 0.05, 0.0], [0.05, 0.05, 0.0]]).reshape(-1)
    a["cut"][:W_IN] = [0.0, 0.01, 0.0, 0.0]
    a["knot"][:W_IN] = [0.0, 0.04, 0.105, 0.105]
    a["length"][0] = 0.105
    return a


def good_values(address, source, ctx=None):
    """{argument: value} of a call with nothing wrong in the given source ("grid" or "curve"); `address`: {array argument: its address}"""
    model = sf.models()[0]
    v = dict(GOOD, model=model.handle, ctx=None if ctx is None else ctx.handle, nthreads=1, **address)
    v[COUNT] = 1
    v["W_in"] = W_IN if source == "curve" else 0
    for k in (GRID_SOURCE if source == "curve" else CURVE_SOURCE):
        v[k] = None
    return v


def faults(flavour, source, values):
    """(label, {argument: replacement}, code, text behind "<entry>: ") of every single fault of the entry"""
    big = sf.models()[3]
    gpu = flavour != "cpu"
    out = [(f"null {k}", {k: None}, INVALID, "null context or model" if gpu else "null model") for k in (("ctx",) if gpu else ()) + ("model",)]
    out.append(("a 9-joint model", {"model": big.handle}, UNSUPPORTED, sf.BIG))
    out += [(label, over, INVALID, text) for label, over, text in BAD_SETTINGS]
    out.append(("a negative count", {COUNT: -1}, INVALID, "negative path count"))
    mine, other = (GRID_SOURCE, CURVE_SOURCE) if source == "grid" else (CURVE_SOURCE, GRID_SOURCE)
    out += [(f"the {source} source without {k}", {k: None}, INVALID, ALL_THREE if source == "grid" else ALL_SIX) for k in mine]
    out.append(("no source", {k: None for k in mine}, INVALID, ONE_SOURCE))
    # (the other group's addresses: any readable array will do, the call is refused before it reads)
    out.append(("both sources", {k: values["t"] for k in other}, INVALID, ONE_SOURCE))
    out.append(("part of the other source", {other[0]: values["t"]}, INVALID, ALL_SIX if source == "grid" else ALL_THREE))
    if source == "curve":
        out += [("W_in 0", {"W_in": 0}, INVALID, "0 rows a path in the curve's tables, outside 1..65536"),
                ("W_in 65537", {"W_in": 65537}, INVALID, "65537 rows a path in the curve's tables, outside 1..65536")]
    pointer = {"cpu": "null pointer", "host": "null host pointer", "device": "null device pointer"}[flavour]
    out += [(f"null {k}", {k: None}, INVALID, pointer) for k in TIMING]
    out.append(("no output", {k: None for k in OUTPUTS}, INVALID, "at least one output is required"))
    if flavour == "device":
        out += [(f"misaligned {k}", {k: "misaligned"}, INVALID, "device pointers must be 16-byte aligned")
                for k in TIMING + (mine[0], mine[-1]) + OUTPUTS]
        out.append(("negative max_blocks", {"max_blocks": -1}, INVALID, "negative max_blocks"))
    return out


def call(flavour, values, over=()):
    """(code, text of mp_last_error) of the entry on `values` with the replacements of `over`"""
    lib = _hip.load_library()
    fn = getattr(lib, entry_name(flavour))
    names = names_of(flavour)
    assert len(names) == len(fn.argtypes), entry_name(flavour)
    v = dict(values)
    for k, x in dict(over).items():
        v[k] = v[k] + 8 if isinstance(x, str) and x == "misaligned" else x
    args = []
    for name, typ in zip(names, fn.argtypes):
        x = v[name]
        if typ in (_hip._vp, _hip._c_dp):
            x = getattr(x, "value", x)
            x = None if x is None else ctypes.cast(ctypes.c_void_p(x), typ)
        args.append(x)
    rc = fn(*args)
    return rc, (lib.mp_last_error() or b"").decode()


def check(flavour, values, source):
    """every fault of the entry answers its code and its text, byte for byte"""
    name = entry_name(flavour)
    seen = faults(flavour, source, values)
    for label, over, code, text in seen:
        rc, msg = call(flavour, values, over)
        assert (rc, msg) == (code, f"{name}: {text}"), f"{name}, {label}: code {rc}, {msg!r}"
    return len(seen)
