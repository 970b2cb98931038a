"""A fixed slice of tools/fuzz_eg.py in the suite: two rounds of drawn pose graphs (the same graphs on every machine) through
ONE batched call each, compared with the model by fuzz_lba.compare_by_rule; no mismatch, and no more than one graph in
eight left out."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

pytestmark = pytest.mark.gpu


def test_two_rounds_of_the_fuzz_tool_report_no_mismatch():
    from orb_slam2_map_amd import lib
    if lib.device_count() < 1:
        pytest.skip("no HIP device")
    pytest.importorskip("torch")
    import fuzz_eg as F
    tot = F.run(0.0, 20264, batch=6, rounds=2)
    print("eg fuzz slice: compared %d, left out %d, spread %.3e / %.3e, device %.3e / %.3e, float %d ulp" % (
        tot["compared"], tot["left_out"], tot["spread_pose"], tot["spread_point"], tot["dev_pose"], tot["dev_point"],
        tot["float_ulp"]))
    assert tot["rounds"] == 2 and not tot["mismatches"], tot["mismatches"][:10]
    assert tot["compared"] >= 8 and tot["left_out"] <= F.LEFT_OUT_CAP * (tot["compared"] + tot["left_out"])
