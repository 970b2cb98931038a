"""The host tables of the pyramid resize chain (orb_slam2_map_amd/csrc/resize_tables.h) without a device:
tests/resize_tables_test.cpp checks every window, selector and weight of both forms of k_resize_fast slot by slot, runs
the forms on the host with the kernel's byte operations (under AddressSanitizer + UBSan: the direct source is an
allocation of exactly w x h bytes) and writes the pyramid it computed; this file compares that pyramid with the oracle's."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(176, 144), (220, 170), (333, 251), (640, 480), (752, 480), (1241, 376), (1280, 960)]
SCALES = [1.1, 1.15, 1.2, 1.5, 2.0]
MAX_LEVELS = 8


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("resize_tables") / "resize_tables_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "orb_slam2_map_amd", "csrc"),
                    os.path.join(ROOT, "tests", "resize_tables_test.cpp"), "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def frames():
    from orb_slam2_map_amd.synth import Stream
    return {s: Stream(s[0], s[1], 99).frame(0)[0] for s in SIZES}


def levels_of(w, h, sf):
    """How many levels (of at most MAX_LEVELS) the size and the scale allow: ORBextractor.cc:410-470 / :1112 in float."""
    scale, n = np.float32(1.0), 0
    for l in range(MAX_LEVELS):
        if l > 0:
            scale = np.float32(np.float64(scale) * np.float64(np.float32(sf)))
        inv = np.float32(1.0) / scale
        if min(int(np.rint(np.float32(w) * inv)), int(np.rint(np.float32(h) * inv))) < 62:
            break
        n += 1
    return n


@pytest.mark.parametrize("sf", SCALES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_tables_and_pyramid(exe, oracle, frames, tmp_path, size, sf):
    w, h = size
    img = frames[size]
    src, dst = str(tmp_path / "img.bin"), str(tmp_path / "pyr.bin")
    img.tofile(src)
    r = subprocess.run([exe, str(w), str(h), repr(sf), str(MAX_LEVELS), src, dst], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "resize_tables_test ok" in r.stdout, r.stdout
    words = r.stdout.split()
    nl = int(words[1])
    assert nl == levels_of(w, h, sf) and nl >= 2
    fast8 = [int(x) for x in words[3:words.index("direct8")]]
    direct8 = words[words.index("direct8") + 1]
    if sf <= 1.5:  # the 16-byte window holds eight pixels' taps up to scale 1.5; at 2.0 they span 17 bytes and more
        assert fast8 == list(range(1, nl)), "levels in the 8-pixel form: %s of %d" % (fast8, nl)
        if w % 8 != 0:  # (no direct mode at all)
            assert direct8 == "0"
        elif w >= 640:  # a narrow row can leave its last item's taps no window that ends with the row: 4 pixels then
            assert direct8 == "1", "level 1 from the caller's image keeps the 4-pixel form"
    else:
        assert fast8 == [] and direct8 == "0"
    oe = oracle.Extractor(500, sf, nl, 20, 7)
    oe.extract(img)
    got = np.fromfile(dst, np.uint8)
    off = 0
    for l in range(1, nl):
        op = oe.pyramid_level(l)
        inner = op[19:op.shape[0] - 19, 19:op.shape[1] - 19]
        mine = got[off:off + inner.size].reshape(inner.shape)
        off += inner.size
        assert np.array_equal(mine, inner), "level %d differs from the oracle at %d px" % (l, int((mine != inner).sum()))
    assert off == got.size
