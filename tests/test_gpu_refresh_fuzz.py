"""A bounded, seeded slice of tools/fuzz_refresh.py (random graphs and tables, refreshes in both forms interleaved with edits
and refused calls on the device against tests/refresh_model.py) inside the suite."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_fuzz_refresh_slice(gpu):
    seconds, seed = 5, 20261021
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_refresh.py"), str(seconds), str(seed)], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    tail = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
    assert r.returncode == 0 and tail.startswith("fuzz ok"), r.stdout[-2000:]
    rounds, refreshes, table_refreshes = [int(x) for x in re.findall(r"\d+", tail.split(" in ")[0])][:3]
    assert rounds >= 1 and refreshes + table_refreshes >= 10, "the slice ran almost nothing: %s" % tail
