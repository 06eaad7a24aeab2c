"""The CPU twins of the float64 entries that came before the sphere model (entry_faults.py lists them): a call with nothing wrong
answers 0, a call with a zero count and null arrays what the table records, and a call with exactly one thing wrong the code and the
text recorded there, byte for byte - a null or 9-joint model, one bad value per check of the settings, a negative count, each
required array missing."""
import pytest

import entry_faults as ef


@pytest.mark.parametrize("family", ef.FAMILIES["cpu"])
def test_cpu_twin_single_faults(family):
    spec = ef.entries("cpu")[family]
    arrays = ef.host_arrays(spec)
    ef.check(spec, ef.good_values(spec, {k: a.ctypes.data for k, a in arrays.items()}))
