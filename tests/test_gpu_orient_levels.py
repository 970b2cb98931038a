"""k_orient forms a frame's level records once per workgroup, finds a slot's level through the plan's slot -> level table
and writes the (up to eight) key points of a wave in one pass behind its iteration loop.  Key points (all seven fields),
descriptors and counts are compared with the oracle bit for bit: one, two and three levels; slot ranges that stay partly
empty next to ranges that are full to the quota, so that the eight slots of an iteration straddle a level boundary and a
wave holds live and skipped slots; batches below OR_BATCH_MIN = 32 frames (one slot per half wave) and from it (four);
flat frames inside a batch and batches of flat frames only; two calls per handle; padded and direct mode; a call whose
cap is one short of a frame's total; poisoned plane buffers."""
import numpy as np
import pytest

from test_gpu_fast_polarity import assert_same_keypoints
from test_gpu_fast_rowstep import make_frame, set_hooks

pytestmark = pytest.mark.gpu

SIZES = {(64, 64): 1, (96, 80): 2, (200, 103): 3}  # (w, h) -> pyramid levels at scale 1.2
NFEATURES = (200, 37, 9)
OR_BATCH_MIN = 32
NFRAMES = OR_BATCH_MIN + 2
# "straddle" frames: texture in the left part of the image only, the fraction chosen per configuration so that the
# quadtree fills one level to exactly its quota and runs out of corners on another (reference() checks that it does).
# A single level (64x64) has no boundary to straddle: its frame only leaves the range partly empty.
STRADDLE = {(64, 64, 200): 0.5, (64, 64, 37): 0.5, (64, 64, 9): 0.4,
            (96, 80, 200): 0.70, (96, 80, 37): 0.28, (96, 80, 9): 0.24,
            (200, 103, 200): 0.30, (200, 103, 37): 0.14, (200, 103, 9): 0.12}
I_TEXTURED, I_FLAT, I_STRADDLE = 0, 1, 2  # what the first three frames of a configuration are


def straddle_frame(w, h, nfeat):
    img = np.full((h, w), 90, np.uint8)
    x1 = int(w * STRADDLE[w, h, nfeat])
    img[:, :x1] = make_frame("textured", w, h, 0)[:, :x1]
    return img


def sel_caps(oe, w, h, nl):
    """slots of every level's selection range (extractor_plan.h: level_max_keypoints() + 1)"""
    caps = []
    for l in range(nl):
        p = oe.pyramid_level(l)
        n_ini = int(np.float32(p.shape[1] - 38 - 32) / np.float32(p.shape[0] - 38 - 32) + np.float32(0.5))
        caps.append(max(4 * n_ini, int(oe.quotas()[l]) + 3) + 1)
    return caps


_ref = {}


def reference(oracle, w, h, nfeat):
    """Frames and the oracle's (key points, descriptors) of each, once per configuration; the inputs are checked to be what
    they are meant to be on the oracle's per-level counts."""
    key = (w, h, nfeat)
    if key in _ref:
        return _ref[key]
    nl = SIZES[w, h]
    oe = oracle.Extractor(nfeat, 1.2, nl, 20, 7)
    imgs = [make_frame("textured", w, h, f) for f in range(NFRAMES)]
    imgs[I_FLAT] = make_frame("flat", w, h, 1)
    imgs[I_STRADDLE] = straddle_frame(w, h, nfeat)
    imgs[NFRAMES - 1] = make_frame("flat", w, h, 2)
    imgs = np.stack(imgs)
    ref = [tuple(a.copy() for a in oe.extract(imgs[f])) for f in range(NFRAMES)]
    counts = [np.bincount(ref[f][0]["octave"], minlength=nl) for f in range(NFRAMES)]
    quotas = np.asarray(oe.quotas())
    caps = np.asarray(sel_caps(oe, w, h, nl))
    # textured: key points on every level; flat: none; no level overflows its slot range
    assert (counts[I_TEXTURED] > 0).all() and counts[I_FLAT].sum() == 0 and counts[NFRAMES - 1].sum() == 0, (key, counts[:3])
    assert all((c < caps).all() for c in counts), (key, caps)
    c = counts[I_STRADDLE]
    assert c.sum() > 0, (key, c)
    if nl > 1:
        assert (c < quotas).any(), (key, c, quotas)  # some level's range partly empty: the quadtree ran out of corners
        assert (c == quotas).any(), (key, c, quotas)  # ... and another full to the quota
        # the eight slots of some iteration belong to two levels (96x80 with 37 features: its only boundary is slot 24)
        bounds = np.cumsum(caps)[:-1]
        assert (bounds % 8 != 0).any() == (key != (96, 80, 37)) and c[0] > 0, (key, caps, c)
    # a wave (two neighbouring slots per iteration, the iterations eight slots apart) with live and skipped slots
    live = np.concatenate([np.arange(cap) < n for cap, n in zip(caps, c)])
    live = np.concatenate([live, np.zeros(-len(live) % 32, bool)]).reshape(-1, 4, 4, 2)  # (workgroup, iteration, wave, half)
    per_wave = live.transpose(0, 2, 1, 3).reshape(-1, 8).sum(1)
    assert ((per_wave > 0) & (per_wave < 8)).any(), (key, per_wave)
    _ref[key] = (imgs, ref)
    return _ref[key]


def cases():
    for (w, h), nl in SIZES.items():
        for nfeat in NFEATURES:
            for direct in ((False, True) if nl > 1 else (False,)):  # direct mode: level 0 read from the image (>= 2 levels, w % 8 == 0)
                yield pytest.param(w, h, nfeat, direct, id="%dx%d_%d_%s" % (w, h, nfeat, "direct" if direct else "padded"))


def run(gpu, imgs, ref, nfeat, nl, batch_of, what):
    total = 0
    for first, batch in batch_of:
        ge = gpu.ORBextractor(nfeat, 1.2, nl, 20, 7, max_batch=batch)
        for call in range(2):  # the second call finds the records of the first in place
            lo = first if call == 0 else NFRAMES - batch - first
            gk, gd = ge.extract_batch(imgs[lo:lo + batch])
            for f in range(batch):
                ok, od = ref[lo + f]
                assert_same_keypoints(gk[f], gd[f], ok, od, "%s batch %d call %d frame %d" % (what, batch, call, lo + f))
                total += len(ok)
        ge.close()
    return total


@pytest.mark.parametrize("w,h,nfeat,direct", cases())
def test_against_oracle(gpu, oracle, monkeypatch, w, h, nfeat, direct):
    """1 and 3 frames per call (one slot per half wave), 32 and 33 (four); textured, flat and straddling frames in them"""
    set_hooks(monkeypatch, direct, None)
    imgs, ref = reference(oracle, w, h, nfeat)
    what = "%dx%d %d features %s" % (w, h, nfeat, "direct" if direct else "padded")
    batches = [(I_TEXTURED, 1), (I_STRADDLE, 1), (0, 3), (0, OR_BATCH_MIN), (0, OR_BATCH_MIN + 1)]
    assert run(gpu, imgs, ref, nfeat, SIZES[w, h], batches, what) > 0


@pytest.mark.parametrize("size,nfeat", [((96, 80), 37), ((200, 103), 200)], ids=["96x80_37", "200x103_200"])
@pytest.mark.parametrize("direct", [False, True], ids=["padded", "direct"])
def test_poisoned_planes(gpu, oracle, monkeypatch, size, nfeat, direct):
    """0xA5 over both plane buffers before every call: nothing k_orient reads is left over from an earlier call"""
    set_hooks(monkeypatch, direct, None, poison=True)
    w, h = size
    imgs, ref = reference(oracle, w, h, nfeat)
    assert run(gpu, imgs, ref, nfeat, SIZES[size], [(I_TEXTURED, 1), (I_STRADDLE, 1), (0, 3), (0, OR_BATCH_MIN)],
               "%dx%d %d features poisoned" % (w, h, nfeat)) > 0


@pytest.mark.parametrize("batch", [3, OR_BATCH_MIN])
def test_flat_frames_only(gpu, monkeypatch, batch):
    """Every frame of the call is flat: total = 0, n_out = 0, nothing stored."""
    set_hooks(monkeypatch, False, None)
    imgs = np.stack([make_frame("flat", 200, 103, f % 4) for f in range(batch)])
    ge = gpu.ORBextractor(200, 1.2, 3, 20, 7, max_batch=batch)
    for call in range(2):
        gk, gd = ge.extract_batch(imgs)
        assert all(len(k) == 0 for k in gk) and all(len(d) == 0 for d in gd)
    ge.close()


@pytest.mark.parametrize("batch", [3, OR_BATCH_MIN + 1])
def test_cap_one_short(gpu, oracle, monkeypatch, batch):
    """cap = (key points of the textured frame) - 1: a frame with more than cap key points reports -1 - total and its rows
    keep what they held before the call; the frames that fit are extracted as ever."""
    import torch
    set_hooks(monkeypatch, False, None)
    w, h, nfeat = 96, 80, 200
    imgs, ref = reference(oracle, w, h, nfeat)
    totals = [len(ref[f][0]) for f in range(batch)]
    cap = totals[I_TEXTURED] - 1
    assert totals[I_STRADDLE] <= cap and totals[I_FLAT] == 0 and sum(t > cap for t in totals) >= 1, totals
    d_img = torch.from_numpy(imgs[:batch].copy()).cuda()
    kps = torch.full((batch, cap, 7), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    desc = torch.full((batch, cap, 32), 0xC3, dtype=torch.uint8, device="cuda")
    nout = torch.full((batch,), 12345, dtype=torch.int32, device="cuda")
    ge = gpu.ORBextractor(nfeat, 1.2, SIZES[w, h], 20, 7, max_batch=batch)
    for call in range(2):
        ge.extract_batch_device(d_img.data_ptr(), batch, w, h, w, w * h, kps.data_ptr(), desc.data_ptr(), cap, nout.data_ptr(),
                                torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        n, k, d = nout.cpu().numpy(), kps.cpu().numpy(), desc.cpu().numpy()
        for f in range(batch):
            if totals[f] > cap:
                assert n[f] == -1 - totals[f], (call, f, n[f], totals[f])
                assert (k[f] == 0x5A5A5A5A).all() and (d[f] == 0xC3).all(), (call, f)
            else:
                assert n[f] == totals[f], (call, f, n[f], totals[f])
                gk = k[f, :n[f]].copy().view(gpu.KEYPOINT_DTYPE).reshape(-1)
                assert_same_keypoints(gk, d[f, :n[f]], ref[f][0], ref[f][1], "cap %d call %d frame %d" % (cap, call, f))
                assert (k[f, n[f]:] == 0x5A5A5A5A).all() and (d[f, n[f]:] == 0xC3).all(), (call, f)
    ge.close()
