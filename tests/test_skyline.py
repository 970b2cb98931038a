"""csrc/skyline.h, the envelope LL^T of the Sim3 pose graph, on the host: tests/skyline_test.cpp is compiled with g++ (no
contraction, AddressSanitizer + UBSan, warnings as errors) and run once.  It holds skyline_llt_solve to the dense
llt_solve of opt_math.h on the permuted matrix bit for bit -- x and every kept entry of L -- on a chain, a ring, a ring with
chords, two components, a single block and an empty system, each with 1, 2 and 5 cooperating threads; a pivot that is not
> 0 gives false and x = 0; the reverse Cuthill-McKee order is a permutation; and on the ring of 64 with neighbours at +-1
and +-2 the bandwidth is at most 2 x 2 + 1 blocks.

"Bandwidth" there is the largest distance |position(i) - position(j)| of a non-zero block from the diagonal, the
quantity the derivation in skyline_test.cpp bounds (it is exactly 5 on that ring); the longest block ROW, which is what
orbgpu_essential_graph_result.bandwidth reports in scalars, counts the diagonal block too and is 6 blocks there."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orb_slam2_map_amd", "csrc")
GRAPHS = ("chain", "ring", "ring_with_chords", "two_components", "single_block", "empty", "ring64_reach2")


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("skyline") / "skyline_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-pthread", "-I" + CSRC, os.path.join(ROOT, "tests", "skyline_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr  # no sanitizer report either
    return r.stdout.splitlines()


def test_every_check_passes(lines):
    assert lines[-1] == "PASSED"
    assert not [ln for ln in lines if ln.startswith("FAIL")]


@pytest.mark.parametrize("graph", GRAPHS)
def test_graph_is_covered(lines, graph):
    mine = [ln for ln in lines if ln.startswith("ok %s:" % graph)]
    assert any("is a permutation" in ln for ln in mine)
    for nt in (1, 2, 5):
        assert any("bit for bit, %d thread(s)" % nt in ln for ln in mine), (graph, nt)
    if graph != "empty":
        assert sum("non-positive pivot" in ln for ln in mine) == 2 and any("NaN pivot" in ln for ln in mine)


def test_ring_bandwidth_is_the_derived_one(lines):
    assert any(ln.startswith("ok ring64_reach2: bandwidth at most 2 x 2 + 1 blocks") for ln in lines)
    info = [ln for ln in lines if ln.startswith("info ring64_reach2:")][0].split()
    assert int(info[info.index("bandwidth_blocks") + 1]) - 1 <= 2 * 2 + 1


def test_header_is_pure_cxx():
    src = open(os.path.join(CSRC, "skyline.h")).read()
    assert "#include <hip" not in src and '#include "common.h"' not in src and "__syncthreads" not in src
