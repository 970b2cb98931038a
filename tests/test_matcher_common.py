"""csrc/matcher_common.h on the host: tests/matcher_common_test.cpp is compiled with g++ (no contraction, AddressSanitizer,
UBSan and float-cast-overflow, no recovery, warnings as errors) and run once.  It holds rot_bin and three_maxima to
literals: every angle difference at which the bin changes, the fold of 30 onto 0, and the differences that have no bin
(915 and more, -375 and less, NaN, +-inf), which must come back as -1 without a float ever being converted outside int's
range; ComputeThreeMaxima on equal counts and on both sides of its 0.1 rule."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orb_slam2_map_amd", "csrc")
ANGLES = ("0", "14.99", "15", "344.99", "345", "359.99", "-0.01", "884.9", "885", "-400", "NaN a", "NaN b", "+inf", "-inf")


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("matcher_common") / "matcher_common_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all",
                    "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "matcher_common_test.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr  # no sanitizer report either
    return r.stdout.splitlines()


def test_every_check_passes(lines):
    assert lines[-1] == "PASSED"
    assert not [ln for ln in lines if ln.startswith("FAIL")]


@pytest.mark.parametrize("angle", ANGLES)
def test_angle_is_covered(lines, angle):
    assert any(ln.startswith("ok rot_bin %s:" % angle) for ln in lines)


def test_three_maxima_is_covered(lines):
    for what in ("four equal", "100 10 9", "100 9 9", "101 10 10"):
        assert any(ln.startswith("ok three_maxima %s:" % what) for ln in lines), what


def test_grid_cell_is_covered(lines):
    """grid_cell (Frame::PosInGrid for the frame glue and orbgpu_assign_features_to_grid): half away from zero on both
    edges of both axes, and NaN, +-inf and values beyond int come back as -1 without a conversion outside int's range."""
    for what in ("(4, 100)", "(4-, 100)", "(508-, 380-)", "(508, 100)", "(100, 380)", "(-4, 100)", "(-4+, -4+)",
                 "(NaN, 100)", "(100, NaN)", "(+inf, 100)", "(100, -inf)", "(1e30, 100)", "(3.5e10, 100)"):
        assert any(ln.startswith("ok grid_cell %s:" % what) for ln in lines), what


def test_header_is_pure_cxx():
    """The header is what the host loop of orbgpu_search_for_initialization compiles too: nothing of HIP outside the
    __HIPCC__ branch."""
    src = open(os.path.join(CSRC, "matcher_common.h")).read()
    host = src.split("#else", 1)[1]
    assert "#include <hip" not in host and "__syncthreads" not in host and "atomicAdd" not in host
