"""The extractor's host-only plan (orb_slam2_map_amd/csrc/extractor_plan.h) without a device:
tests/extractor_plan_test.cpp plans a size, checks the plan's invariants (slot and selection layout, every lane of the
FAST column tables, the cells of every wave, exact reciprocals, the level-0 border selectors, the blur strips, the table
arena, the launch decisions) and prints the plan; this file runs it plain and under AddressSanitizer + UBSan (a
stand-alone program both times), compares constants and level sizes with the oracle, every table and scalar with the
digests recorded from the configure() this header replaced (tests/golden/extractor_plan_digests.json), and the refusals
with the messages tests/test_gpu_limits.py matches."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "extractor_plan_digests.json")

# (width, height, nfeatures, scale factor, levels, ORBGPU_DEBUG_QT_KEYS hook)
CASES = [
    (640, 480, 1000, 1.2, 8, -1),
    (1280, 960, 2000, 1.2, 8, -1),
    (752, 480, 1000, 1.2, 8, -1),
    (1241, 376, 1000, 1.2, 8, -1),   # odd width: no BorderCol table, no direct mode
    (333, 251, 1000, 1.2, 8, -1),
    (176, 144, 1000, 1.1, 8, -1),
    (1000, 200, 600, 1.2, 7, -1),    # (level 7 would be 56 px high: seven levels are what the size allows)
    (130, 98, 1000, 1.2, 2, -1),     # smallest that still has a level 1
    (640, 480, 1000, 1.2, 8, 0),     # k_quadtree<true> with no key in LDS ...
    (640, 480, 1000, 1.2, 8, 8),     # ... and with eight
]
REFUSALS = [
    ((4200, 64, 500, 1.2, 1, -1), "outside the supported range"),
    ((300, 1000, 500, 1.2, 2, -1), "aspect ratio unsupported"),
    ((640, 480, 60000, 1.2, 8, -1), "nfeatures too large for the quadtree kernel"),
]


def case_id(c):
    return "%dx%d-n%d-s%s-l%d-k%d" % c


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("extractor_plan")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
            "-I" + os.path.join(ROOT, "orb_slam2_map_amd", "csrc"), os.path.join(ROOT, "tests", "extractor_plan_test.cpp")]
    plain, san = str(d / "extractor_plan_test"), str(d / "extractor_plan_test_san")
    subprocess.run(base + ["-o", plain], check=True)
    subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", san], check=True)
    return plain, san


def run(exe, case):
    return subprocess.run([exe] + [repr(x) if isinstance(x, float) else str(x) for x in case], stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_plan(exes, oracle, case):
    w, h, nfeatures, sf, nl, _ = case
    outs = [run(exe, case) for exe in exes]
    for r in outs:
        assert r.returncode == 0 and "extractor_plan_test ok" in r.stdout, r.stdout
    assert outs[0].stdout == outs[1].stdout
    lines = [ln.split() for ln in outs[0].stdout.splitlines()]
    # constants, quotas and level sizes: the oracle's
    oe = oracle.Extractor(nfeatures, sf, nl, 20, 7)
    oe.extract(np.zeros((h, w), np.uint8))
    consts = np.array([[np.float32(x) for x in ln[2:]] for ln in lines if ln[0] == "C"], np.float32)
    assert consts.shape == (nl, 4)
    for col, ref in enumerate((oe.scale_factors(), oe.inv_scale_factors(), oe.sigma2(), oe.inv_sigma2())):
        assert np.array_equal(consts[:, col], ref), col
    levels = np.array([[int(x) for x in ln[1:]] for ln in lines if ln[0] == "L"])
    assert np.array_equal(levels[:, 0], np.arange(nl))
    assert np.array_equal(levels[:, 3], oe.quotas())
    for l in range(nl):
        op = oe.pyramid_level(l)
        assert (levels[l, 1], levels[l, 2]) == (op.shape[1] - 38, op.shape[0] - 38), l
    assert [int(x) for x in next(ln for ln in lines if ln[0] == "U")[1:]] == list(oe.umax())
    # every table and scalar: what the replaced configure() built
    with open(GOLDEN) as f:
        golden = json.load(f)[case_id(case)]
    got = {ln[1]: ln[2] for ln in lines if ln[0] == "D"}
    assert got.keys() == golden.keys()
    assert {k: v for k, v in got.items() if golden[k] != v} == {}
    if w % 4 != 0:
        assert got["border_fast"] == "0" and got["direct0_ok"] == "0" and got["bcol.d"].startswith("0:")


@pytest.mark.parametrize("case,message", REFUSALS, ids=lambda x: case_id(x) if isinstance(x, tuple) else None)
def test_refusals(exes, case, message):
    for exe in exes:
        r = run(exe, case)
        assert r.returncode == 3 and r.stdout.startswith("refused: ") and message in r.stdout, r.stdout
