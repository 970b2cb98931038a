"""A bounded, seeded slice of tools/fuzz_compact.py (the rounds of the covis, cull, refresh and kfdb fuzzers with compactions
of device and model at random points; tests/compact_model.py, exact equality) inside the suite."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_fuzz_compact_slice(gpu):
    seconds, seed = 5, 20261021
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_compact.py"), str(seconds), str(seed)], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    tail = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
    assert r.returncode == 0 and tail.startswith("fuzz ok"), r.stdout[-2000:]
    rounds, compactions, dropped, queries = [int(x) for x in re.findall(r"\d+", tail.split(" in ")[0])][:4]
    assert rounds >= 4 and compactions >= 3 and dropped >= 3 and queries >= 10, "the slice ran almost nothing: %s" % tail
