"""A 5-second slice of tools/fuzz_sim3opt.py: randomised loop candidates on the device against tests/sim3opt_model.py with
the parity test's comparison rules; scenes within 1e-6 of a classification threshold are left out, at most 1 % of them."""
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
    import fuzz_sim3opt as F
    tot = F.run(5.0, 20261)
    print("\n".join(F.report(tot)))
    assert tot["compared"] > 0 and not tot["mismatches"], tot["mismatches"][:10]
    assert tot["left_out"] <= 0.01 * (tot["compared"] + tot["left_out"])
