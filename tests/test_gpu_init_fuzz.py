"""A 5-second slice of tools/fuzz_init.py: randomised two-view scenes on the device against tests/init_model.py with the
parity test's comparison rules."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

pytestmark = pytest.mark.gpu


def test_fuzz_slice():
    from orb_slam2_map_amd import lib
    if lib.device_count() < 1:
        pytest.skip("no HIP device")
    pytest.importorskip("torch")
    import fuzz_init as F
    tot = F.run(5.0, 20261019)
    print("\n".join(F.report(tot)))
    assert tot["scenes"] >= 4 and tot["downstream_compared"] > 0 and not tot["mismatches"], tot["mismatches"][:10]
