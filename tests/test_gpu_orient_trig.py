"""Orientation, cos / sin of the angle and the descriptor as one chain: k_describe rotates the pattern by the (ca, sb) of a
key point's record, so a wrong, stale or missing pair changes the descriptor.  Key points and descriptors are compared with
the oracle bit for bit below OR_BATCH_MIN = 32 frames per call (k_orient takes one key point per half wave and workgroup
pass) and from it (four), with slots that stay empty, with frames that yield no key point, on handles that are called
twice, and in both trig modes of the library (with and without the exception table).  Whoever moves the cos / sin
evaluation (DESIGN.md 9.34 measured folding it into k_orient) has these cases to pass."""
import numpy as np
import pytest

from test_gpu_fast_polarity import assert_same_keypoints
from test_gpu_fast_rowstep import make_frame

pytestmark = pytest.mark.gpu

SIZES = {(64, 64): 1, (96, 80): 2}  # (w, h) -> pyramid levels at scale 1.2
OR_BATCH_MIN = 32
# features asked for: per-level slot counts that are no multiple of the 8 (32) slots of a workgroup, more key points than a
# small image has (slots stay empty behind the last one) and fewer (the quadtree drops some)
NFEATURES = (200, 37, 9)


def frames(w, h, n):
    """n frames: textured ones with a flat one (no key point at all) second and last"""
    out = [make_frame("textured", w, h, f) for f in range(n)]
    out[1 % n] = make_frame("flat", w, h, 1)
    out[n - 1] = make_frame("flat", w, h, 2)
    return np.stack(out)


_ref = {}


def reference(oracle, w, h, nfeat, n, mode):
    """The oracle's (key points, descriptors) of every frame, made once per configuration and trig mode."""
    key = (w, h, nfeat, n, mode)
    if key not in _ref:
        oe = oracle.Extractor(nfeat, 1.2, SIZES[w, h], 20, 7)
        imgs = frames(w, h, n)
        _ref[key] = (imgs, [tuple(a.copy() for a in oe.extract(imgs[f])) for f in range(n)])
    return _ref[key]


@pytest.fixture(params=["host_libm", "rounded_double"])
def trig_mode(request, gpu, oracle):
    """with the exception table (the default) and without it; handles pick the mode up when they are created"""
    if request.param == "rounded_double":
        gpu.set_trig_mode(gpu.TRIG_ROUNDED_DOUBLE)
        oracle.set_trig_mode(oracle.TRIG_ROUNDED_DOUBLE)
    try:
        yield request.param
    finally:
        gpu.set_trig_mode(gpu.TRIG_HOST_LIBM)
        oracle.set_trig_mode(oracle.TRIG_LIBM_FLOAT)


def run(gpu, oracle, monkeypatch, size, nfeat, n, batch_of, mode):
    for v in ("ORBGPU_FAST_EARLY_OUT", "ORBGPU_DEBUG_FAST_QUEUE", "ORBGPU_DEBUG_NO_DIRECT0", "ORBGPU_DEBUG_DIRECT0_MIN",
              "ORBGPU_DEBUG_POISON_PYRAMID"):
        monkeypatch.delenv(v, raising=False)
    w, h = size
    imgs, ref = reference(oracle, w, h, nfeat, n, mode)
    total = 0
    for first, batch in batch_of:
        ge = gpu.ORBextractor(nfeat, 1.2, SIZES[size], 20, 7, max_batch=batch)
        for call in range(2):  # the second call finds the records of the first in place: nothing stale may be used
            lo = first if call == 0 else n - batch - first
            gk, gd = ge.extract_batch(imgs[lo:lo + batch])
            for f in range(batch):
                ok, od = ref[lo + f]
                assert_same_keypoints(gk[f], gd[f], ok, od, "%dx%d %d features %s batch %d call %d frame %d" % (
                    w, h, nfeat, mode, batch, call, lo + f))
                total += len(ok)
        ge.close()
    return total


@pytest.mark.parametrize("nfeat", NFEATURES)
@pytest.mark.parametrize("size", list(SIZES), ids=lambda s: "%dx%d" % s)
def test_small_batches(gpu, oracle, monkeypatch, trig_mode, size, nfeat):
    """1 and 3 frames per call: one key point per half wave"""
    assert run(gpu, oracle, monkeypatch, size, nfeat, 4, [(0, 1), (1, 1), (0, 3)], trig_mode) > 0


@pytest.mark.parametrize("size,nfeat", [((64, 64), 200), ((96, 80), 37)], ids=["64x64_200", "96x80_37"])
def test_full_batch(gpu, oracle, monkeypatch, trig_mode, size, nfeat):
    """OR_BATCH_MIN frames per call: four key points per half wave"""
    n = OR_BATCH_MIN + 1
    assert run(gpu, oracle, monkeypatch, size, nfeat, n, [(0, OR_BATCH_MIN)], trig_mode) > 0


def test_frames_without_key_points(gpu, oracle, monkeypatch, trig_mode):
    """Every frame of the call is flat: no slot holds a key point, nothing is stored, the counts are 0."""
    imgs = np.stack([make_frame("flat", 96, 80, f) for f in range(3)])
    ge = gpu.ORBextractor(200, 1.2, 2, 20, 7, max_batch=3)
    gk, gd = ge.extract_batch(imgs)
    assert all(len(k) == 0 for k in gk) and all(len(d) == 0 for d in gd)
    ge.close()
