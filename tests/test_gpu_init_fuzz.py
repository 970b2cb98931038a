"""A 5-second slice of tools/fuzz_init.py: randomised two-view scenes on the device against tests/init_model.py with the
parity test's comparison rules; a scene where those rules leave something out is held to float64 stage by stage instead
(tests/init_fp64.py, rungs 3, 4, 6 and 7 on the scene's own result)."""
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
    import init_fp64
    tot = F.run(5.0, 20261019, fp64=init_fp64)
    print("\n".join(F.report(tot)))
    assert tot["scenes"] >= 4 and tot["downstream_compared"] > 0 and not tot["mismatches"], tot["mismatches"][:10]
    assert tot["fp64_hypotheses"] == tot["hypotheses_left_out"] and (tot["fp64_scenes"] > 0) == (tot["hypotheses_left_out"] > 0)
