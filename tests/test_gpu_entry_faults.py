"""GPU: the device-pointer and host-array entries of the float64 families that came before the sphere model (entry_faults.py lists
them): a call with nothing wrong answers 0 (one row or problem is launched), a call with a zero count and null arrays what the table
records, and a call with exactly one thing wrong the code and the text recorded there, byte for byte - the faults of the CPU twins
in the GPU entries' words and, on device pointers, each misaligned pointer."""
import pytest

import entry_faults as ef
from manipulapy_amd import registry

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = registry.get_context()
    c.selftest()
    return c


@pytest.mark.parametrize("family", ef.FAMILIES["device"])
def test_device_entry_single_faults(ctx, family):
    spec = ef.entries("device")[family]
    assert ctx.lib.mp_id_regressor_normal_workspace_bytes(ef.models()[0].handle, 1) <= ef.SIZES["work"]
    bufs = {k: ctx.to_device(a) for k, a in ef.host_arrays(spec).items()}
    try:
        ef.check(spec, ef.good_values(spec, {k: b.ptr.value for k, b in bufs.items()}, ctx))
        ctx.synchronize()
    finally:
        for b in bufs.values():
            b.free()


@pytest.mark.parametrize("family", ef.FAMILIES["host"])
def test_host_entry_single_faults(ctx, family):
    spec = ef.entries("host")[family]
    arrays = ef.host_arrays(spec)
    ef.check(spec, ef.good_values(spec, {k: a.ctypes.data for k, a in arrays.items()}, ctx))
