"""k_fast_detect's single-network corner score (polarity chosen by the selector H = min_i max(v[2i], v[2i+9]), bytes
complemented where dark) against the oracle on small images built so that every branch of the selector occurs in cell
interiors: FAST candidates of every level (DBG_CANDIDATES) and the key-point output, bit-exact."""
import numpy as np
import pytest

from conftest import corners_to_array

pytestmark = pytest.mark.gpu

FIELDS = ("x", "y", "size", "angle", "response", "octave", "class_id")
# ring order of the extractor (dx, dy)
RING = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0),
        (-3, 1), (-2, 2), (-1, 3))
SIZES = {(64, 64): 1, (96, 80): 2}  # (w, h) -> pyramid levels at scale 1.2 (a level needs 62 px)
FIRST, PITCH = 22, 8                # patch centres: FAST scores the pixels 19 .. size - 20; a patch is 7 x 7


def ring_terms(img, x, y):
    """(c, H, c - A, B - c) of the pixel: the selector and the two terms of the two-network score."""
    c = int(img[y, x])
    v = [int(img[y + dy, x + dx]) for dx, dy in RING]
    H = min(max(v[2 * i], v[(2 * i + 9) & 15]) for i in range(8))
    arcs = [[v[(a + k) & 15] for k in range(9)] for a in range(16)]
    return c, H, c - min(max(a) for a in arcs), max(min(a) for a in arcs) - c


def centres(w, h):
    return [(x, y) for y in range(FIRST, h - 19 - 3, PITCH) for x in range(FIRST, w - 19 - 3, PITCH)]


def plant(img, x, y, c, ring):
    img[y - 3:y + 4, x - 3:x + 4] = c
    for (dx, dy), v in zip(RING, ring):
        img[y + dy, x + dx] = v


def arc_ring(c, start, length, delta, rest):
    """`length` contiguous ring pixels at c + delta from `start`, the others at c + rest."""
    r = [c + rest] * 16
    for k in range(length):
        r[(start + k) & 15] = c + delta
    return r


def patches_arcs(p, frame):
    """bright and dark arcs of exactly 9 (a corner) and exactly 8 (none), every start position over the patches"""
    sign = 1 if p % 2 == 0 else -1
    length = 9 if (p // 2) % 2 == 0 else 8
    c = 90 + 10 * (p % 7)
    ring = arc_ring(c, (p + 5 * frame) % 16, length, sign * (30 + p % 9), -sign * (p % 3))
    want = (lambda c_, H, dk, br: (br if sign > 0 else dk) == 30 + p % 9 and (H > c_ if sign > 0 else H < c_)) if length == 9 \
        else (lambda c_, H, dk, br: max(dk, br) <= 0)
    return c, ring, want


def patches_h_equal(p, frame):
    """H == c: one selector pair holds c and a value below it, every other pair has a pixel above c"""
    c = 60 + 20 * (p % 6)
    i0 = (p + 3 * frame) % 8
    ring = [c + 35 if (k + p) % 3 else c - 35 for k in range(16)]
    for i in range(8):  # every pair's maximum above c ...
        if max(ring[2 * i], ring[(2 * i + 9) & 15]) < c:
            ring[2 * i] = c + 35
    ring[2 * i0], ring[(2 * i0 + 9) & 15] = (c, c - 35) if p % 2 else (c - 1 - p % 4, c)  # ... except this one's: c
    return c, ring, lambda c_, H, dk, br: H == c_ and max(dk, br) <= 0


def patches_diametral(p, frame):
    """one diametral pair on one side of c, the 14 others on the other side: the selector names a polarity, no arc of 9 has it"""
    sign = 1 if p % 2 == 0 else -1
    c = 128 + 3 * (p % 5)
    k0 = (p + frame) % 8
    ring = [c - sign * 40] * 16
    ring[k0] = ring[k0 + 8] = c + sign * 40
    return c, ring, lambda c_, H, dk, br: max(dk, br) < 0 and (H < c_ if sign > 0 else H > c_)


def patches_extremes(p, frame):
    """centres 0 and 255, where the complement maps to the other end of the range"""
    start = (3 * p + frame) % 16
    kind = p % 6
    if kind == 0:
        return 0, arc_ring(0, start, 9, 255, 0), lambda c_, H, dk, br: br == 255 and dk <= 0
    if kind == 1:
        return 255, arc_ring(255, start, 9, -255, 0), lambda c_, H, dk, br: dk == 255 and br <= 0
    if kind == 2:
        return 0, arc_ring(0, start, 10, 25 + p, 1), lambda c_, H, dk, br: br == 25 + p
    if kind == 3:
        return 255, arc_ring(255, start, 11, -(25 + p), -1), lambda c_, H, dk, br: dk == 25 + p
    if kind == 4:
        return 0, arc_ring(0, start, 7, 200, 0), lambda c_, H, dk, br: H == 0 and max(dk, br) <= 0
    return 255, arc_ring(255, start, 7, -200, 0), lambda c_, H, dk, br: H == 255 and max(dk, br) <= 0


PLANTED = {"arcs": patches_arcs, "h_equal": patches_h_equal, "diametral": patches_diametral, "extremes": patches_extremes}


def make_frame(kind, w, h, frame):
    if kind == "checkerboard":  # one-pixel squares: no ring has nine contiguous pixels on one side of its centre
        yy, xx = np.mgrid[0:h, 0:w]
        return (((xx + yy + frame) % 2) * (180 - 40 * frame) + 30 + 10 * frame).astype(np.uint8)
    if kind == "textured":
        rng = np.random.default_rng(100 * frame + w)
        coarse = rng.integers(0, 256, ((h + 3) // 4, (w + 3) // 4))
        img = np.kron(coarse, np.ones((4, 4), np.int64))[:h, :w] + rng.integers(-12, 13, (h, w))
        return np.clip(img, 0, 255).astype(np.uint8)
    img = np.full((h, w), 128 if kind != "extremes" else (0 if frame % 2 == 0 else 255), np.uint8)
    for p, (x, y) in enumerate(centres(w, h)):
        c, ring, want = PLANTED[kind](p, frame)
        plant(img, x, y, c, ring)
        assert want(*ring_terms(img, x, y)), "%s patch %d of frame %d is not what it is meant to be: %r" % (
            kind, p, frame, ring_terms(img, x, y))
    return img


def assert_same_keypoints(gk, gd, ok, od, what):
    assert len(gk) == len(ok), "%s: key point count %d != oracle %d" % (what, len(gk), len(ok))
    for f in FIELDS:
        a = np.ascontiguousarray(gk[f]).view(np.uint32)
        b = np.ascontiguousarray(ok[f]).view(np.uint32)
        assert np.array_equal(a, b), "%s: field %s differs" % (what, f)
    assert gd.shape == od.shape and np.array_equal(gd, od), "%s: descriptors differ" % what


@pytest.fixture(scope="module")
def inputs(oracle):
    """Every input once, with what the oracle makes of each of its frames: (candidates per level, key points, descriptors)."""
    out = {}
    for (w, h), nl in SIZES.items():
        oe = oracle.Extractor(200, 1.2, nl, 20, 7)
        for kind in list(PLANTED) + ["checkerboard", "textured"]:
            imgs = np.stack([make_frame(kind, w, h, f) for f in range(3)])
            ref = []
            for f in range(3):
                ok, od = oe.extract(imgs[f])
                ref.append(([corners_to_array(oe.level_candidates(l)) for l in range(nl)], ok.copy(), od.copy()))
            out[kind, w, h] = (imgs, ref)
    return out


def test_inputs_cover_the_selector(inputs):
    """What the images are for, read off the oracle: corners of both kinds where arcs of 9 were planted, none on the
    checkerboard, scores at the 255 clamp on the extremes."""
    for (w, h) in SIZES:
        for f in range(3):
            assert len(inputs["arcs", w, h][1][f][0][0]) >= len(centres(w, h)) // 2
            assert len(inputs["checkerboard", w, h][1][f][0][0]) == 0
            assert len(inputs["textured", w, h][1][f][0][0]) > 0
        assert max(int(inputs["extremes", w, h][1][f][0][0][:, 2].max()) for f in range(3)) == 254  # (the response is s - 1)


@pytest.mark.parametrize("variant", ["default", "early_out", "queue16"])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("size", list(SIZES), ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", list(PLANTED) + ["checkerboard", "textured"])
def test_score_matches_oracle(gpu, inputs, monkeypatch, kind, size, batch, variant):
    w, h = size
    nl = SIZES[size]
    for v in ("ORBGPU_FAST_EARLY_OUT", "ORBGPU_DEBUG_FAST_QUEUE"):
        monkeypatch.delenv(v, raising=False)
    if variant == "early_out":
        monkeypatch.setenv("ORBGPU_FAST_EARLY_OUT", "1")
    elif variant == "queue16":
        monkeypatch.setenv("ORBGPU_DEBUG_FAST_QUEUE", "16")
    ge = gpu.ORBextractor(200, 1.2, nl, 20, 7, max_batch=batch)  # (the hooks are read when a handle is created)
    imgs, ref = inputs[kind, w, h]
    first = 0 if batch == 3 else 1
    gk, gd = ge.extract_batch(imgs[first:first + batch])
    for f in range(batch):
        cand, ok, od = ref[first + f]
        what = "%s %dx%d frame %d %s" % (kind, w, h, first + f, variant)
        for l in range(nl):
            gc, _ = ge.debug_read(gpu.DBG_CANDIDATES, f, l)
            assert gc.shape == cand[l].shape and np.array_equal(gc, cand[l]), "%s L%d: FAST candidates differ (%d vs %d)" % (
                what, l, len(gc), len(cand[l]))
        assert_same_keypoints(gk[f], gd[f], ok, od, what)
