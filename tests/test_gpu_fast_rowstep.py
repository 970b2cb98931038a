"""k_fast_detect's row step outside the score network: the running row offset with its clamp at the band's last input row,
the band mask that only runs in a wave's last steps, the record queue and its fallback.  FAST candidates of every level
(DBG_CANDIDATES) and the key-point output against the oracle, bit-exact, on images small enough that one wave holds
bands and levels of different heights."""
import numpy as np
import pytest

from conftest import corners_to_array
from test_gpu_fast_polarity import RING, assert_same_keypoints

pytestmark = pytest.mark.gpu

EDGE = 19
# (w, h) -> pyramid levels at scale 1.2 (a level needs 62 px).  64x64 and 96x70: one level, one band (96x70: 32 rows in a
# cell pitch of 38); 96x80: two levels with bands of 42 and 29 rows in one wave; 96x103 and 200x103: level 0 has two
# bands of 36 and 29 rows (the last one shorter), 200x103 three levels in three waves.
SIZES = {(64, 64): 1, (96, 80): 2, (96, 70): 1, (96, 103): 2, (200, 103): 3}
DIRECT_OK = [s for s, nl in SIZES.items() if nl >= 2 and s[0] % 8 == 0]  # what direct mode asks of a geometry
KINDS = ("textured", "boundary", "flat")
BG = 120


def band_rows(h):
    """First and last scored row of every band (row of cells) of a level-0 plane of height h: ORBextractor.cc:789-807
    with W = 30 and the 16-px border; FAST scores rows 3 .. of a cell's sub-image."""
    span = (h - EDGE + 3) - (EDGE - 3)
    n = span // 30
    hcell = -(-span // n)
    out = []
    for b in range(n):
        y0 = EDGE + b * hcell
        out.append((y0, min(y0 + hcell, h - EDGE) - 1))
    return out


def make_frame(kind, w, h, frame):
    if kind == "flat":
        return np.full((h, w), 40 + 50 * frame, np.uint8)
    if kind == "textured":
        rng = np.random.default_rng(100 * frame + w + h)
        coarse = rng.integers(0, 256, ((h + 3) // 4, (w + 3) // 4))
        img = np.kron(coarse, np.ones((4, 4), np.int64))[:h, :w] + rng.integers(-12, 13, (h, w))
        return np.clip(img, 0, 255).astype(np.uint8)
    # "boundary": corners in the first and the last row of every band and nowhere else at level 0 -- whether the last row of
    # a band survives depends on the row below counting as 0 (the band mask) and on the rows the clamped fetch delivers.
    # A corner is a centre and an arc of 9 .. 11 ring pixels, each within minThFAST = 7 of the background and 10 .. 14
    # apart from each other: no other pixel of the image has nine ring pixels that far from it.
    img = np.full((h, w), BG, np.uint8)
    for b, (first, last) in enumerate(band_rows(h)):
        for i, x in enumerate(range(22 + 4 * (b % 2), w - 22, 8)):
            p = i + 3 * b + frame
            sign = 1 if p % 2 == 0 else -1
            y = last if i % 2 == 0 else first
            img[y, x] = BG - sign * (5 + p % 3)
            for k in range(9 + p % 3):
                dx, dy = RING[(5 * p + k) % 16]
                img[y + dy, x + dx] = BG + sign * (5 + (p // 3) % 3)
    return img


def set_hooks(monkeypatch, direct, variant, poison=False):
    for v in ("ORBGPU_FAST_EARLY_OUT", "ORBGPU_DEBUG_FAST_QUEUE", "ORBGPU_DEBUG_NO_DIRECT0", "ORBGPU_DEBUG_DIRECT0_MIN",
              "ORBGPU_DEBUG_POISON_PYRAMID"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv(*(("ORBGPU_DEBUG_DIRECT0_MIN", "1") if direct else ("ORBGPU_DEBUG_NO_DIRECT0", "1")))
    if variant == "early_out":
        monkeypatch.setenv("ORBGPU_FAST_EARLY_OUT", "1")
    elif variant == "queue16":
        monkeypatch.setenv("ORBGPU_DEBUG_FAST_QUEUE", "16")
    if poison:
        monkeypatch.setenv("ORBGPU_DEBUG_POISON_PYRAMID", "1")


@pytest.fixture(scope="module")
def inputs(oracle):
    """Every input once, with what the oracle makes of each of its frames: (candidates per level, key points, descriptors)."""
    out = {}
    for (w, h), nl in SIZES.items():
        oe = oracle.Extractor(200, 1.2, nl, 20, 7)
        for kind in KINDS:
            imgs = np.stack([make_frame(kind, w, h, f) for f in range(3)])
            ref = []
            for f in range(3):
                ok, od = oe.extract(imgs[f])
                ref.append(([corners_to_array(oe.level_candidates(l)) for l in range(nl)], ok.copy(), od.copy()))
            out[kind, w, h] = (imgs, ref)
    return out


def check(gpu, inputs, kind, size, batch, what):
    w, h = size
    nl = SIZES[size]
    ge = gpu.ORBextractor(200, 1.2, nl, 20, 7, max_batch=batch)  # (the hooks are read when a handle is created)
    imgs, ref = inputs[kind, w, h]
    first = 0 if batch == 3 else 1
    gk, gd = ge.extract_batch(imgs[first:first + batch])
    for f in range(batch):
        cand, ok, od = ref[first + f]
        tag = "%s %s %dx%d batch %d frame %d" % (what, kind, w, h, batch, first + f)
        for l in range(nl):
            gc, _ = ge.debug_read(gpu.DBG_CANDIDATES, f, l)
            assert gc.shape == cand[l].shape and np.array_equal(gc, cand[l]), "%s L%d: FAST candidates differ (%d vs %d)" % (
                tag, l, len(gc), len(cand[l]))
        assert_same_keypoints(gk[f], gd[f], ok, od, tag)
    ge.close()


def test_inputs_are_what_they_are_for(inputs):
    """Read off the oracle: survivors in (nearly) every scored row of the textured image, corners in the first and last
    row of every band of the boundary image and in no other row of level 0, none on the flat one; and the geometry
    the sizes were chosen for."""
    assert band_rows(103) == [(19, 54), (55, 83)] and band_rows(80) == [(19, 60)] and band_rows(70) == [(19, 50)]
    for (w, h) in SIZES:
        for f in range(3):
            assert all(len(c) == 0 for c in inputs["flat", w, h][1][f][0]) and len(inputs["flat", w, h][1][f][1]) == 0
            rows = set(int(y) for y in inputs["textured", w, h][1][f][0][0][:, 1])
            assert len(rows) >= (h - 2 * EDGE) // 2
            got = set(int(y) + EDGE - 3 for y in inputs["boundary", w, h][1][f][0][0][:, 1])  # (relative to the 16-px border)
            want = set(y for band in band_rows(h) for y in band)
            assert got == want, "boundary %dx%d frame %d: corners in rows %r, planted in %r" % (w, h, f, sorted(got), sorted(want))


# (direct mode only where the geometry takes it: elsewhere the handle would run the padded mode again)
CASES = [(s, "padded") for s in SIZES] + [(s, "direct") for s in DIRECT_OK]


@pytest.mark.parametrize("variant", ["default", "early_out", "queue16"])
@pytest.mark.parametrize("size,mode", CASES, ids=lambda v: v if isinstance(v, str) else "%dx%d" % v)
def test_rowstep_matches_oracle(gpu, inputs, monkeypatch, size, mode, variant):
    set_hooks(monkeypatch, mode == "direct", variant)
    for kind in KINDS:
        for batch in (1, 3):
            check(gpu, inputs, kind, size, batch, "%s %s" % (mode, variant))


@pytest.mark.parametrize("mode", ["padded", "direct"])
def test_no_row_beyond_the_last_needed_one_counts(gpu, inputs, monkeypatch, mode):
    """Both plane buffers hold 0xA5 before every call: a row fetch that ran past the band's last input row (rows + 5),
    or a band mask that let a row outside the band score, would change candidates next to the poisoned rows."""
    for size in (DIRECT_OK if mode == "direct" else list(SIZES)):
        for variant in ("default", "early_out"):
            set_hooks(monkeypatch, mode == "direct", variant, poison=True)
            for kind in ("boundary", "textured"):
                check(gpu, inputs, kind, size, 3, "poisoned %s %s" % (mode, variant))
