"""A bounded, seeded slice of tools/fuzz_cull.py (random maps, candidate lists, observation queries and refused calls on the
device key-frame culling against tests/cull_model.py) inside the suite."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_fuzz_cull_slice(gpu):
    seconds, seed = 5, 20261020
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_cull.py"), str(seconds), str(seed)], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    tail = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
    assert r.returncode == 0 and tail.startswith("fuzz ok"), r.stdout[-2000:]
    rounds, calls = [int(x) for x in re.findall(r"\d+", tail.split(" in ")[0])][:2]
    assert rounds >= 1 and calls >= 10, "the slice ran almost nothing: %s" % tail
