"""Shared by test_sphere_entry_faults_host.py and test_gpu_sphere_entry_faults.py: the single-fault calls of the sphere-model entries
(collision, collision edges, RRT-Connect, path shortcutting, goal configurations) in their three flavours - the CPU twins (`cpu`), the host-array entries
of a context (`host`) and the device-pointer entries (`device`) - with the code and the exact text each must answer.

Every call is made through the C ABI with the argument list of _hip.SIGNATURES, on one problem of the 3-joint chain of chain_cases.py:
all arguments good but the ones the fault names.  The texts are written out here, not taken from the library: they are what callers
have seen so far and what a change of the entries' scaffolding must keep byte for byte."""
import ctypes
import functools

import numpy as np

import chain_cases as ch
from manipulapy_amd import _hip

N = 3
INVALID, UNSUPPORTED = 1, 4
MAX_NODES = MAX_WAYPOINTS = W_IN = 4
BYTES = 256                               # room of every array argument: one problem's rows and a misaligned start fit many times

# family -> (input arrays, the count, the settings, the device form's extra arguments, the outputs), in the order of the C signature:
# [ctx,] model, handle, inputs, count, settings, [extras,] outputs [, nthreads]
FAMILIES = {
    "collision": (("q",), "rows", ("eps_world", "eps_self"), (),
                  ("dist_world", "arg_world", "dist_self", "arg_self", "grad_dist_world", "grad_dist_self", "cost", "grad")),
    "collision_edges": (("q_from", "q_to"), "edges", ("margin", "tol", "max_steps"), ("max_blocks",),
                        ("status", "t", "steps", "clearance", "witness")),
    "rrt_connect": (("q_start", "q_goal"), "B", ("lo", "hi", "seed", "step", "min_advance", "max_iters", "max_nodes", "max_waypoints",
                                                 "margin", "tol", "max_steps"), ("workspace", "workspace_bytes", "max_blocks"),
                    ("status", "count", "waypoints", "iterations", "nodes", "evaluations")),
    "path_shortcut": (("waypoints_in", "count_in"), "B", ("W_in", "seed", "max_iters", "min_gain", "max_waypoints", "margin", "tol",
                                                          "max_steps"), ("workspace", "workspace_bytes", "max_blocks"),
                      ("status", "count", "waypoints", "length_in", "length_out", "iterations", "accepted", "skipped_full", "evaluations")),
    "goal_ik": (("T_goal", "q_seed"), "B", ("lo", "hi", "seed", "eomg", "ev", "damping", "step_cap", "max_iters", "max_attempts", "margin",
                                            "tol"), ("max_blocks",),
                ("status", "q", "attempts", "iterations", "converged", "pose_error", "clearance", "witness")),
}
SETTINGS = {"eps_world": 0.05, "eps_self": 0.05, "margin": 0.01, "tol": 0.01, "max_steps": 64, "seed": 7, "step": 0.3, "min_advance": 0.04,
            "max_iters": 2, "max_nodes": MAX_NODES, "max_waypoints": MAX_WAYPOINTS, "W_in": W_IN, "min_gain": 0.0, "max_blocks": 0,
            "eomg": 0.01, "ev": 0.001, "damping": 0.01, "step_cap": 0.5, "max_attempts": 2}
COUNT_WORD = {"collision": "row", "collision_edges": "edge", "rrt_connect": "problem", "path_shortcut": "problem", "goal_ik": "problem"}
_EDGE = (("margin nan", {"margin": float("nan")}, "margin must be finite"),
         ("tol 0", {"tol": 0.0}, "tol must be positive and finite"),
         ("max_steps 0", {"max_steps": 0}, "max_steps 0 outside 1..65536"))
# one bad value per check of the settings: (label, what replaces the good arguments, the text behind "<entry>: ")
BAD_SETTINGS = {
    "collision": (("eps_world 0", {"eps_world": 0.0}, "eps_world and eps_self must be positive and finite"),
                  ("eps_self inf", {"eps_self": float("inf")}, "eps_world and eps_self must be positive and finite")),
    "collision_edges": _EDGE,
    "rrt_connect": _EDGE + (("null box", {"lo": None}, "null sampling box"),
                            ("empty box", {"hi": "below"}, "joint 0: the sampling box must be finite with lo <= hi"),
                            ("step 0", {"step": 0.0}, "step must be positive and finite"),
                            ("min_advance -1", {"min_advance": -1.0}, "min_advance must be non-negative and finite"),
                            ("max_iters -1", {"max_iters": -1}, "negative max_iters"),
                            ("max_nodes 1", {"max_nodes": 1}, "max_nodes 1 outside 2..65536"),
                            ("max_waypoints 1", {"max_waypoints": 1}, "max_waypoints 1 below 2")),
    "path_shortcut": _EDGE + (("W_in 0", {"W_in": 0}, "0 input rows a path, outside 1..65536"),
                              ("max_iters -1", {"max_iters": -1}, "negative max_iters"),
                              ("min_gain -1", {"min_gain": -1.0}, "min_gain must be non-negative and finite"),
                              ("max_waypoints 1", {"max_waypoints": 1}, "max_waypoints 1 outside 2..65536")),
    "goal_ik": _EDGE[:2] + (("null box", {"hi": None}, "null joint box"),
                            ("empty box", {"hi": "below"}, "joint 0: the box must be finite with lo <= hi"),
                            ("eomg 0", {"eomg": 0.0}, "eomg and ev must be positive and finite"),
                            ("ev inf", {"ev": float("inf")}, "eomg and ev must be positive and finite"),
                            ("damping 0", {"damping": 0.0}, "damping must be positive and finite"),
                            ("step_cap nan", {"step_cap": float("nan")}, "step_cap must be positive and finite"),
                            ("max_iters -1", {"max_iters": -1}, "negative max_iters"),
                            ("max_attempts 0", {"max_attempts": 0}, "max_attempts 0 outside 1..65536")),
}
BIG = "not available for models with more than 8 joints (this one has 9)"


def entry_name(family, flavour):
    return f"mp_{family}_{'cpu_' if flavour == 'cpu' else 'host_' if flavour == 'host' else ''}f64"


def names_of(family, flavour):
    inputs, count, settings, extras, outputs = FAMILIES[family]
    lead = ("model", "handle") if flavour == "cpu" else ("ctx", "model", "handle")
    return lead + inputs + (count,) + settings + (extras if flavour == "device" else ()) + outputs + (("nthreads",) if flavour == "cpu" else ())


def workspace_bytes(family):
    """one block's workspace at the settings above"""
    return (_hip.rrt_connect_workspace_bytes(N, MAX_NODES, 1) if family == "rrt_connect" else
            _hip.path_shortcut_workspace_bytes(N, MAX_WAYPOINTS, 1) if family == "path_shortcut" else 0)


@functools.lru_cache(maxsize=None)
def models():
    """(the chain's HipModel, its collision handle, a handle made for 2 joints, a 9-joint model); made once and kept alive"""
    from test_random_robots import random_robot

    t = random_robot(np.random.default_rng(1), 9, ("general",))
    return ch.chain(N)[3], ch.collision_model(N)[0].handle, ch.collision_model(2)[0].handle, _hip.HipModel(t.S, t.Mcom, t.G, t.M_ee)


def host_arrays(family):
    """{array argument: a host array of BYTES bytes holding one good problem}; kept alive by the caller"""
    a = {k: np.zeros(BYTES // 8) for k in FAMILIES[family][0] + FAMILIES[family][4]}
    if family == "path_shortcut":
        a["waypoints_in"][:W_IN * N] = np.linspace(0.0, 0.1, W_IN * N)
        a["count_in"] = np.zeros(BYTES // 4, dtype=np.int32)
        a["count_in"][0] = 2
    return a


def box():
    lim = ch.chain(N)[2]
    lo, hi = np.ascontiguousarray(lim[:, 0]), np.ascontiguousarray(lim[:, 1])
    return {"lo": lo, "hi": hi, "below": np.ascontiguousarray(lo - 1.0)}


def good_values(family, flavour, address, ctx=None):
    """{argument: value} of a call with nothing wrong; `address`: {array argument: its address}"""
    model, handle, _, _ = models()
    v = dict(SETTINGS, model=model.handle, handle=handle.handle, ctx=None if ctx is None else ctx.handle, nthreads=1, lo="lo", hi="hi",
             **address)
    v[FAMILIES[family][1]] = 1
    v["workspace_bytes"] = workspace_bytes(family)
    return v


def faults(family, flavour):
    """(label, {argument: replacement}, code, text behind "<entry>: ") of every single fault of the entry"""
    inputs, count, _, _, outputs = FAMILIES[family]
    _, _, other, big = models()
    gpu = flavour != "cpu"
    null = "null context, model or collision handle" if gpu else "null model or collision handle"
    out = [(f"null {k}", {k: None}, INVALID, null) for k in (("ctx",) if gpu else ()) + ("model", "handle")]
    out.append(("a 9-joint model", {"model": big.handle}, UNSUPPORTED, BIG))
    out.append(("a handle of another joint count", {"handle": other.handle}, INVALID,
                "the collision handle was made for a model of 2 joints" + (", this one has 3" if gpu else "")))
    out += [(label, over, INVALID, text) for label, over, text in BAD_SETTINGS[family]]
    out.append(("a negative count", {count: -1}, INVALID, f"negative {COUNT_WORD[family]} count"))
    pointer = {"cpu": "null pointer", "host": "null host pointer", "device": "null device pointer"}[flavour]
    out += [(f"null {k}", {k: None}, INVALID, pointer) for k in inputs]
    out.append(("no output", {k: None for k in outputs}, INVALID, "at least one output is required"))
    if flavour == "device":
        out += [(f"misaligned {k}", {k: "misaligned"}, INVALID, "device pointers must be 16-byte aligned")
                for k in inputs + outputs + (("workspace",) if family in ("rrt_connect", "path_shortcut") else ())]
        out.append(("negative max_blocks", {"max_blocks": -1}, INVALID, "negative max_blocks") if family != "collision" else None)
        one = workspace_bytes(family)
        if one:
            short = f"the workspace holds %d bytes, one block needs {one} (mp_{family}_workspace_bytes)"
            out.append(("a short workspace", {"workspace_bytes": one - 16}, INVALID, short % (one - 16)))
            out.append(("no workspace", {"workspace": None}, INVALID, short % 0))
    return [f for f in out if f is not None]


def call(family, flavour, values, over=()):
    """(code, text of mp_last_error) of the entry on `values` with the replacements of `over`"""
    lib = _hip.load_library()
    fn = getattr(lib, entry_name(family, flavour))
    names = names_of(family, flavour)
    assert len(names) == len(fn.argtypes), entry_name(family, flavour)
    v, bx = dict(values), box()
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


def check(family, flavour, values):
    """every fault of the entry answers its code and its text, byte for byte"""
    name = entry_name(family, flavour)
    seen = faults(family, flavour)
    for label, over, code, text in seen:
        rc, msg = call(family, flavour, values, over)
        assert (rc, msg) == (code, f"{name}: {text}"), f"{name}, {label}: code {rc}, {msg!r}"
    return len(seen)
