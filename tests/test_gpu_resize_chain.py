"""The pyramid resize chain on the device: k_resize_fast writes plane interiors and the 3 px of border the blur reads;
the whole 19-px border exists only once a padded plane is handed out (k_ring_fill).  Everything is compared with the CPU oracle,
bit for bit, below and above the batch size at which the launch shape changes, with level 0 read from the caller's image
(direct mode) and from the padded copy, and with the plane buffers poisoned before every call
(ORBGPU_DEBUG_POISON_PYRAMID): a stage that read a border pixel the hot path does not write would read 0xA5."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from test_gpu_extractor import assert_same_keypoints  # noqa: E402

pytestmark = pytest.mark.gpu

# (width, height, scale factor, levels, features): many small levels, an odd pitch and right edge, the shipped geometry,
# a coarse pyramid, and scale 2.0 (the widest tap windows the fast kernel takes; its taps do not fit the 8-pixel form).
# Scale 2.0 has 3 levels, not 4: level 3 of 640x480 would be 80x60, and the library accepts no level under 62 px a side
# ("pyramid level 3 too small", before this file existed as well).
CONFIGS = [(176, 144, 1.1, 8, 400), (333, 251, 1.2, 8, 600), (640, 480, 1.2, 8, 1000), (640, 480, 1.5, 5, 1000),
           (640, 480, 2.0, 3, 1000)]
MAX_BATCH = 40
_images, _oracles = {}, {}


def images(w, h):
    """MAX_BATCH + 1 frames of the seeded synthetic stream, made once per size."""
    if (w, h) not in _images:
        from orb_slam2_map_amd.synth import Stream
        st = Stream(w, h, 4242)
        _images[(w, h)] = np.stack([st.frame(t)[0] for t in range(MAX_BATCH + 1)])
    return _images[(w, h)]


def oracle_of(oracle, cfg, t):
    """The oracle's extraction of frame t (made once): (extractor holding the pyramid, key points, descriptors)."""
    key = cfg + (t,)
    if key not in _oracles:
        w, h, sf, nl, nfeat = cfg
        oe = oracle.Extractor(nfeat, sf, nl, 20, 7)
        ok, od = oe.extract(images(w, h)[t])
        _oracles[key] = (oe, ok, od)
    return _oracles[key]


def set_mode(monkeypatch, direct, poison):
    for v in ("ORBGPU_FAST_EARLY_OUT", "ORBGPU_DEBUG_NO_DIRECT0", "ORBGPU_DEBUG_DIRECT0_MIN", "ORBGPU_DEBUG_POISON_PYRAMID"):
        monkeypatch.delenv(v, raising=False)
    if direct:
        monkeypatch.setenv("ORBGPU_DEBUG_DIRECT0_MIN", "1")
    else:
        monkeypatch.setenv("ORBGPU_DEBUG_NO_DIRECT0", "1")
    if poison:
        monkeypatch.setenv("ORBGPU_DEBUG_POISON_PYRAMID", "1")


def assert_padded_planes(gpu, ge, oe, frame, nl, what):
    """Every level through both getters: the padded debug view (borders included) and mvImagePyramid[l]."""
    for l in range(nl):
        op = oe.pyramid_level(l)
        hh, ww = op.shape
        raw, pitch = ge.debug_read(gpu.DBG_PYRAMID_PADDED, frame, l)
        gp = raw.reshape(-1, pitch)[:hh, :ww]
        assert np.array_equal(gp, op), "%s L%d: padded plane differs at %d px" % (what, l, int((gp != op).sum()))
        lv, w_, h_ = ge.get_pyramid_level(frame, l)
        assert (w_, h_) == (ww - 38, hh - 38) and np.array_equal(lv, op[19:hh - 19, 19:ww - 19]), "%s L%d: getter" % (what, l)


@pytest.mark.parametrize("poison", [False, True], ids=["plain", "poison"])
@pytest.mark.parametrize("direct", [False, True], ids=["padded0", "direct0"])
@pytest.mark.parametrize("batch", [1, 9, 40])
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "%dx%d_sf%g_%dl" % c[:4])
def test_chain_against_oracle(gpu, oracle, monkeypatch, cfg, batch, direct, poison):
    """Key points and descriptors first (no getter has run: the hot path alone must be right, poisoned or not), then
    complete padded planes through the getters, then a second call on the same handle."""
    w, h, sf, nl, nfeat = cfg
    set_mode(monkeypatch, direct, poison)
    imgs = images(w, h)
    ge = gpu.ORBextractor(nfeat, sf, nl, 20, 7, max_batch=batch)
    for first in (0, 1):  # second call: the same handle, after the getters, on shifted frames
        what = "%s batch %d direct %d poison %d call %d" % (cfg, batch, direct, poison, first)
        gk, gd = ge.extract_batch(imgs[first:first + batch])
        frames = sorted({0, batch - 1})
        for f in frames:
            _, ok, od = oracle_of(oracle, cfg, first + f)
            assert_same_keypoints(gk[f], gd[f], ok, od, "%s frame %d" % (what, f))
        for f in frames:
            assert_padded_planes(gpu, ge, oracle_of(oracle, cfg, first + f)[0], f, nl, "%s frame %d" % (what, f))
    ge.close()


@pytest.mark.parametrize("poison", [False, True], ids=["plain", "poison"])
def test_borders_after_graph_replay(gpu, oracle, monkeypatch, poison):
    """The host entry point records a graph on the second call of a configuration and replays it afterwards: the border
    state is that of the replayed call, and the level-3 getter still returns a complete plane."""
    cfg = CONFIGS[2]
    set_mode(monkeypatch, False, poison)
    monkeypatch.delenv("ORBGPU_DEBUG_NO_DIRECT0")
    ge = gpu.ORBextractor(cfg[4])
    for t in range(4):
        k, d = ge(images(640, 480)[t])
        oe, ok, od = oracle_of(oracle, cfg, t)
        assert_same_keypoints(k, d, ok, od, "host call %d" % t)
        if t >= 1:  # (calls 2 and 3 come out of the graph)
            op = oe.pyramid_level(3)
            raw, pitch = ge.debug_read(gpu.DBG_PYRAMID_PADDED, 0, 3)
            assert np.array_equal(raw.reshape(-1, pitch)[:op.shape[0], :op.shape[1]], op), "call %d: level-3 borders" % t
    assert ge.graph_counts()[1] >= 1, "the graph was never replayed"
    ge.close()


def test_stereo_on_poisoned_planes(gpu, oracle, monkeypatch):
    """Frame::ComputeStereoMatches reads both handles' planes as the hot path left them (interior + 3-px ring)."""
    from orb_slam2_map_amd.synth import StereoStream
    from test_gpu_stereo import Pair, _bits
    set_mode(monkeypatch, False, True)
    monkeypatch.delenv("ORBGPU_DEBUG_NO_DIRECT0")
    P = Pair(gpu, oracle, StereoStream(640, 480, 12), 1, 1000)
    u, d, _ = P.model()
    gu, gd = P.gpu(gpu)
    assert np.array_equal(_bits(gu), _bits(u)) and np.array_equal(_bits(gd), _bits(d))


@pytest.mark.parametrize("batch", [2, 32])
def test_row_slack_is_never_read(gpu, oracle, monkeypatch, batch):
    """Device input whose rows have slack bytes (stride 648) or none (640): the bytes between the rows, and behind the last
    row of the last frame, never reach a plane -- zeros and 0xFF there give identical pyramids, equal to the oracle's.
    Two frames take the 4-pixel items from the caller's image, 32 the 8-pixel ones."""
    torch = pytest.importorskip("torch")
    cfg = CONFIGS[2]
    set_mode(monkeypatch, True, False)
    imgs = images(640, 480)[:batch]
    ends = (0, batch - 1)
    for stride in (640, 648):
        planes = []
        for fill in (0x00, 0xFF):
            ge = gpu.ORBextractor(cfg[4], max_batch=batch)
            cap = ge.max_keypoints(640, 480)
            buf = torch.full((batch * 480 * stride,), fill, dtype=torch.uint8, device="cuda")
            buf.view(batch, 480, stride)[:, :, :640] = torch.from_numpy(imgs).cuda()
            kps = torch.zeros((batch, cap, 7), dtype=torch.float32, device="cuda")
            desc = torch.zeros((batch, cap, 32), dtype=torch.uint8, device="cuda")
            n = torch.zeros(batch, dtype=torch.int32, device="cuda")
            ge.extract_batch_device(buf.data_ptr(), batch, 640, 480, stride, 480 * stride, kps.data_ptr(), desc.data_ptr(),
                                    cap, n.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            for f in ends:
                _, ok, od = oracle_of(oracle, cfg, f)
                nf = int(n[f])
                gk = np.frombuffer(kps[f, :nf].cpu().numpy().tobytes(), gpu.KEYPOINT_DTYPE)
                assert_same_keypoints(gk, desc[f, :nf].cpu().numpy(), ok, od, "stride %d fill %#x frame %d" % (stride, fill, f))
            got = []
            for f in ends:
                for l in range(cfg[3]):
                    raw, pitch = ge.debug_read(gpu.DBG_PYRAMID_PADDED, f, l)
                    hh, ww = oracle_of(oracle, cfg, f)[0].pyramid_level(l).shape
                    got.append(raw.reshape(-1, pitch)[:hh, :ww].copy())  # (the bytes past a row's end belong to no plane)
            planes.append(got)
            assert_padded_planes(gpu, ge, oracle_of(oracle, cfg, batch - 1)[0], batch - 1, cfg[3], "stride %d fill %#x" % (stride, fill))
            ge.close()
        for a, b in zip(*planes):
            assert np.array_equal(a, b), "stride %d: the pyramid depends on the slack bytes" % stride
