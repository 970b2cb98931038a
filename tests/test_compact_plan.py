"""The host-only parts of a compaction (orb_slam2_map_amd/csrc/compact_plan.h and id_table_compact in id_table.h) without a
device: tests/compact_plan_test.cpp checks the plan on hand cases and on every keep mask of a small table, the C1 keep set
on parent chains, the capacity rule against a simulation of the doubling, and runs the transaction over malloc-backed
buffers with a failure injected at every allocation and operation in turn.  Built and run plain and under
AddressSanitizer + UBSan (a stand-alone program both times)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("compact_plan")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pthread", "-I" + os.path.join(ROOT, "include"),
            "-I" + os.path.join(ROOT, "orb_slam2_map_amd", "csrc"), os.path.join(ROOT, "tests", "compact_plan_test.cpp")]
    plain, san = str(d / "compact_plan_test"), str(d / "compact_plan_test_san")
    subprocess.run(base + ["-o", plain], check=True)
    subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", san], check=True)
    return plain, san


@pytest.mark.parametrize("which", [0, 1], ids=["plain", "sanitized"])
def test_compact_plan(exes, which):
    r = subprocess.run([exes[which]], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "compact_plan_test ok" in r.stdout, r.stdout
