"""k_orient's slot -> level mapping without a device: tests/orient_levels_test.cpp plans every size of a grid (64x64 to
1280x960, 9 to 2000 features, every level count the size allows) and checks that the levels' selection ranges tile
[0, sel_cap_total) and that slot_level() and the plan's byte table (extractor_plan.h) name for every slot the one level
whose range holds it.  Run plain and under AddressSanitizer + UBSan; a stand-alone program both times."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(64, 64), (96, 80), (176, 144), (200, 103), (640, 480), (1280, 960)]
NFEATURES = [9, 37, 200, 1000, 2000]
MAX_LEVELS = {(64, 64): 1, (96, 80): 2, (200, 103): 3}  # at scale 1.2 (the sizes tests/test_gpu_orient_levels.py runs)


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("orient_levels")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
            "-I" + os.path.join(ROOT, "orb_slam2_map_amd", "csrc"), os.path.join(ROOT, "tests", "orient_levels_test.cpp")]
    plain, san = str(d / "orient_levels_test"), str(d / "orient_levels_test_san")
    subprocess.run(base + ["-o", plain], check=True)
    subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", san], check=True)
    return [subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for exe in (plain, san)]


def test_slot_levels(outputs):
    for r in outputs:
        assert r.returncode == 0 and "orient_levels_test ok" in r.stdout and "FAILED" not in r.stdout, r.stdout[-4000:]
    assert outputs[0].stdout == outputs[1].stdout
    planned = {}
    for ln in outputs[0].stdout.splitlines():
        if ln.startswith("P "):
            _, size, n, l, _, slots = ln.split()
            w, h = (int(x) for x in size.split("x"))
            planned.setdefault((w, h, int(n[1:])), []).append(int(l[1:]))
            assert int(slots) > 0
    # the whole grid was planned, each size with level counts 1 .. its largest; the one size the plan refuses (a single
    # 64x64 level cannot hold 2000 key points' quadtree nodes in LDS) has no slots to check
    refused = [ln.split(None, 3) for ln in outputs[0].stdout.splitlines() if ln.startswith("R ")]
    assert [r[1:3] for r in refused] == [["64x64", "n2000"]] and "nfeatures too large for the quadtree kernel" in refused[0][3]
    assert sorted(planned) == sorted((w, h, n) for (w, h) in SIZES for n in NFEATURES if (w, h, n) != (64, 64, 2000))
    # (many features on few levels of a small image are refused as well: 96x80 with 2000 features is planned from two levels)
    for (w, h, n), levels in planned.items():
        assert levels == list(range(levels[0], levels[0] + len(levels))), (w, h, n, levels)
        assert levels[-1] == MAX_LEVELS.get((w, h), levels[-1]), (w, h, n, levels)
    assert all(planned[640, 480, n][-1] == 8 and planned[1280, 960, n][-1] == 8 for n in NFEATURES)
