"""The CPU twins of the sphere-model entries (mp_collision_cpu_f64, mp_collision_edges_cpu_f64, mp_rrt_connect_cpu_f64,
mp_path_shortcut_cpu_f64, mp_goal_ik_cpu_f64) and the two workspace sizes: a call with exactly one thing wrong answers the code and the text recorded in
sphere_entry_faults.py, byte for byte, with the entry's own name in front - a null model or handle, a 9-joint model, a handle made for
another joint count, one bad value per check of the settings, a negative count, null inputs, no output."""
import pytest

import sphere_entry_faults as sf
from manipulapy_amd import _hip


@pytest.mark.parametrize("family", tuple(sf.FAMILIES))
def test_cpu_twin_single_faults(family):
    arrays = sf.host_arrays(family)
    values = sf.good_values(family, "cpu", {k: a.ctypes.data for k, a in arrays.items()})
    assert sf.call(family, "cpu", values)[0] == 0, "the call with nothing wrong"
    assert sf.check(family, "cpu", values) >= 8


@pytest.mark.parametrize("name,limit,word", (("mp_rrt_connect_workspace_bytes", "max_nodes", "outside 2..65536"),
                                             ("mp_path_shortcut_workspace_bytes", "max_waypoints", "outside 2..65536")))
def test_workspace_bytes_single_faults(name, limit, word):
    lib = _hip.load_library()
    fn = getattr(lib, name)
    assert fn(sf.N, 4, 1) > 0
    for args, code, text in (((0, 4, 1), sf.INVALID, "joint count 0 below 1"),
                             ((9, 4, 1), sf.UNSUPPORTED, sf.BIG),
                             ((sf.N, 1, 1), sf.INVALID, f"{limit} 1 {word}"),
                             ((sf.N, 65537, 1), sf.INVALID, f"{limit} 65537 {word}"),
                             ((sf.N, 4, 0), sf.INVALID, "block count 0 below 1")):
        got = (int(fn(*args)), lib.mp_last_error().decode())
        assert got == (-code, f"{name}: {text}"), (args, got)
