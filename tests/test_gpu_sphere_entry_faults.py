"""GPU: the ten sphere-model entries of a context (collision, collision edges, RRT-Connect, path shortcutting and goal
configurations, on device pointers and on host arrays): a call with exactly one thing wrong answers the code and the text recorded in sphere_entry_faults.py,
byte for byte, with the entry's own name in front - the faults of the CPU twins and, on device pointers, a misaligned pointer, a
short or missing workspace and a negative max_blocks.  Every call is refused before anything is launched.

And the grid rule's four terms held apart: on the 3-joint chain with 65 problems (two blocks wanted, far fewer than the device keeps
resident) the planner's and the shortcutter's outputs at max_blocks = 1 equal those on a workspace of exactly one block."""
import pytest

import chain_cases as ch
import sphere_entry_faults as sf
import test_gpu_chain_cases as gc
from manipulapy_amd import registry

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = registry.get_context()
    c.selftest()
    return c


@pytest.mark.parametrize("family", tuple(sf.FAMILIES))
def test_device_entry_single_faults(ctx, family):
    names = sf.FAMILIES[family][0] + sf.FAMILIES[family][4]
    bufs = {k: ctx.alloc(sf.BYTES) for k in names}
    one = sf.workspace_bytes(family)
    if one:
        bufs["workspace"] = ctx.alloc(one)
    try:
        values = sf.good_values(family, "device", {k: b.ptr.value for k, b in bufs.items()}, ctx)
        assert sf.check(family, "device", values) >= 12
    finally:
        for b in bufs.values():
            b.free()


@pytest.mark.parametrize("family", tuple(sf.FAMILIES))
def test_host_entry_single_faults(ctx, family):
    arrays = sf.host_arrays(family)
    values = sf.good_values(family, "host", {k: a.ctypes.data for k, a in arrays.items()}, ctx)
    assert sf.check(family, "host", values) >= 9


def test_one_block_by_max_blocks_equals_one_block_by_workspace(ctx):
    n, B = 3, 65
    case = ch.plan_case(n)
    gc._identical(gc._rrt(ctx, n, case["qs"][:B], case["qg"][:B], max_blocks=1), gc._rrt(ctx, n, case["qs"][:B], case["qg"][:B], blocks=1),
                  "rrt: max_blocks 1 against a workspace of one block")
    sc = ch.shortcut_case(n)
    wp, cnt = sc["waypoints"][:B], sc["count"][:B]
    gc._identical(gc._shortcut(ctx, n, wp, cnt, max_blocks=1), gc._shortcut(ctx, n, wp, cnt, blocks=1),
                  "shortcut: max_blocks 1 against a workspace of one block")
