"""GPU parity of call SEQUENCES on one extractor handle: the state a handle keeps between calls (the recorded hipGraph of
the host entry points, the tables configure() builds for one image size, the lazy level 0 of direct mode, the cell
counters) must never leak one call into the next.  Every call of every case is compared with the oracle: key points as
u32 patterns, descriptors, and mvImagePyramid levels 0, 1 and the last of the first and last frame.  Failed calls --
ECAPACITY, and ENOMEM forced by the ORBGPU_DEBUG_FAIL_ALLOC_OVER hook -- must leave a handle that gives exact results on
the next call.  The module runs twice: as shipped, and with level 0 always copied into a padded plane."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_extractor import assert_same_keypoints, check_stages

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = ("ORBGPU_FAST_EARLY_OUT", "ORBGPU_DEBUG_NO_DIRECT0", "ORBGPU_DEBUG_DIRECT0_MIN", "ORBGPU_DEBUG_NO_GRAPH",
         "ORBGPU_DEBUG_FAIL_ALLOC_OVER")


@pytest.fixture(autouse=True, params=["shipped", "padded_level0"])
def level0_variant(request, monkeypatch):
    """Handles are created after this has set the environment (the hooks are read at creation)."""
    for v in HOOKS:
        monkeypatch.delenv(v, raising=False)
    if request.param == "padded_level0":
        monkeypatch.setenv("ORBGPU_DEBUG_NO_DIRECT0", "1")
    return request.param


_ORACLE = {}


def oracle_result(oracle, img, nfeat, nlevels):
    """(key points, descriptors, {level: mvImagePyramid[level]}) of the oracle, memoised per image."""
    key = (img.shape, nfeat, nlevels, hash(img.tobytes()))
    if key not in _ORACLE:
        oe = oracle.Extractor(nfeat, 1.2, nlevels)
        k, d = oe.extract(img)
        lv = {}
        for l in (0, 1, nlevels - 1):
            lw, lh = C.c_int(), C.c_int()
            oe.L.ora_blurred_level(oe.h, l, C.byref(lw), C.byref(lh))  # (the level's size, blurred or not)
            lv[l] = oe.pyramid_level(l)[19:19 + lh.value, 19:19 + lw.value].copy()
        _ORACLE[key] = (k, d, lv)
    return _ORACLE[key]


class Seq:
    """One handle, a sequence of calls, each checked against the oracle."""

    def __init__(self, gpu, oracle, nfeat=1000, nlevels=8, max_batch=1):
        self.gpu, self.oracle, self.nfeat, self.nlevels = gpu, oracle, nfeat, nlevels
        self.ge = gpu.ORBextractor(nfeat, 1.2, nlevels, max_batch=max_batch)
        self.keep = []  # every caller buffer stays alive until the case ends: a stale pointer then reads wrong bytes
        self.n = 0

    def host(self, imgs, cap=None):
        imgs = np.ascontiguousarray(imgs, np.uint8)
        b, h, w = imgs.shape
        cap = cap or self.ge.max_keypoints(w, h)
        kps = np.zeros((b, cap), self.gpu.KEYPOINT_DTYPE)
        desc = np.zeros((b, cap, 32), np.uint8)
        n = np.zeros(b, np.int32)
        L = self.ge.L
        self.gpu.check(L.orbgpu_extract_batch(self.ge.h, imgs.ctypes.data_as(C.c_void_p), b, w, h, imgs.strides[1],
                                              imgs.strides[0], kps.ctypes.data_as(C.c_void_p),
                                              desc.ctypes.data_as(C.c_void_p), cap, n.ctypes.data_as(C.c_void_p)))
        return self.verify(imgs, [kps[f, :n[f]] for f in range(b)], [desc[f, :n[f]] for f in range(b)], "host")

    def device(self, imgs, cap=None):
        import torch
        imgs = np.ascontiguousarray(imgs, np.uint8)
        b, h, w = imgs.shape
        cap = cap or self.ge.max_keypoints(w, h)
        buf = torch.from_numpy(imgs).cuda()
        kps = torch.zeros((b, cap, 7), dtype=torch.float32, device="cuda")
        desc = torch.zeros((b, cap, 32), dtype=torch.uint8, device="cuda")
        nout = torch.zeros(b, dtype=torch.int32, device="cuda")
        self.keep.append((buf, kps, desc, nout))
        self.ge.extract_batch_device(buf.data_ptr(), b, w, h, w, w * h, kps.data_ptr(), desc.data_ptr(), cap,
                                     nout.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        n = nout.cpu().numpy()
        assert (n >= 0).all(), "device call over cap: %s" % n
        gk = [np.frombuffer(kps[f, :n[f]].cpu().numpy().tobytes(), self.gpu.KEYPOINT_DTYPE) for f in range(b)]
        gd = [desc[f, :n[f]].cpu().numpy() for f in range(b)]
        return self.verify(imgs, gk, gd, "device")

    def verify(self, imgs, gk, gd, entry):
        self.n += 1
        b = len(imgs)
        what = "call %d (%s, batch %d, %dx%d)" % (self.n, entry, b, imgs.shape[2], imgs.shape[1])
        for f in range(b):
            ok, od, _ = oracle_result(self.oracle, imgs[f], self.nfeat, self.nlevels)
            assert_same_keypoints(gk[f], gd[f], ok, od, "%s frame %d" % (what, f))
        self.check_levels(imgs, what)
        return gk, gd

    def check_levels(self, imgs, what):
        """mvImagePyramid of the last call: levels 0, 1 and the last, first and last frame; no frame past the batch."""
        b = len(imgs)
        for f in sorted({0, b - 1}):
            lv = oracle_result(self.oracle, imgs[f], self.nfeat, self.nlevels)[2]
            for l in sorted(lv):
                g, w, h = self.ge.get_pyramid_level(f, l)
                assert np.array_equal(g, lv[l]), "%s: mvImagePyramid[%d] of frame %d differs at %d px" % (
                    what, l, f, int((g != lv[l]).sum()) if g.shape == lv[l].shape else -1)
        with pytest.raises(self.gpu.OrbGpuError) as ei:
            self.ge.get_pyramid_level(b, 0)
        assert ei.value.status == self.gpu.EINVAL, "%s: frame %d is not part of the last call" % (what, b)

    def stages(self, img, frame, what):
        """check_stages of test_gpu_extractor (padded pyramid, blurred planes, candidates, selection) for one frame."""
        oe = self.oracle.Extractor(self.nfeat, 1.2, self.nlevels)
        oe.extract(img)
        check_stages(self.gpu, self.ge, oe, frame, self.nlevels, what)

    def counts(self):
        return self.ge.graph_counts()


def frames(stream, first, n):
    return np.stack([stream.frame(first + i)[0] for i in range(n)])


def test_replay_after_device_call_restores_the_last_call(gpu, oracle, stream640):
    """Bug 1 (a graph replay kept the bookkeeping of the call before it): host batch of 8 three times (the graph is
    recorded by the second and replayed by the third), orbgpu_extract_batch_device on a caller buffer X of 8 other
    frames, host batch of 8 again -- a replay.  Before the fix the replay left last_src / last_batch of the device call in
    place: in direct mode mvImagePyramid[0] and the padded debug view were made from X's images, and the blurred level-0
    view used X's layout.  All three must show the host images."""
    s = Seq(gpu, oracle)
    host, other = frames(stream640, 0, 8), frames(stream640, 30, 8)
    for _ in range(3):
        s.host(host)
    s.device(other)
    rec, rep = s.counts()
    s.host(host)
    assert s.counts() == (rec, rep + 1), "the last host call must be a graph replay: %s -> %s" % ((rec, rep), s.counts())
    for f in (0, 7):
        s.stages(host[f], f, "host batch after a device batch, frame %d" % f)


def test_replay_after_device_call_of_another_batch_size(gpu, oracle, stream640):
    """Bug 1, the frame range: host batch of 8 three times, a device batch of 2 (not in direct mode), host batch of 8 --
    a replay; frame 5 of the last call must be readable (before the fix the range was the device call's 2 frames).
    Mirrored on a handle made with max_batch=8 (so that the device call does not reconfigure): host batch of 2 three
    times, device batch of 8, host batch of 2 (a replay): frame 5 must be rejected with EINVAL, frames 0 and 1 must be the
    host images (before the fix: the device call's 8 frames, level 0 made from its buffer in direct mode)."""
    s = Seq(gpu, oracle)
    host, other = frames(stream640, 0, 8), frames(stream640, 40, 2)
    for _ in range(3):
        s.host(host)
    s.device(other)
    rec, rep = s.counts()
    s.host(host)  # (check_levels reads frame 7 and expects EINVAL for frame 8)
    assert s.counts() == (rec, rep + 1)
    g, _, _ = s.ge.get_pyramid_level(5, 0)
    assert np.array_equal(g, host[5])

    s = Seq(gpu, oracle, max_batch=8)
    host2, other8 = frames(stream640, 50, 2), frames(stream640, 60, 8)
    cap = s.ge.max_keypoints(640, 480)
    for _ in range(3):  # host cap 4x the device call's: its per-key scratch for 8 frames fits in the host calls' (no new key)
        s.host(host2, cap=4 * cap)
    assert s.counts()[1] >= 1, "the third host call must replay"
    s.device(other8, cap=cap)
    rec, rep = s.counts()
    s.host(host2, cap=4 * cap)  # check_levels: frame 2 must be rejected
    assert s.counts() == (rec, rep + 1)
    with pytest.raises(gpu.OrbGpuError) as ei:
        s.ge.get_pyramid_level(5, 0)
    assert ei.value.status == gpu.EINVAL
    for f in (0, 1):
        s.stages(host2[f], f, "batch of 2 after a device batch of 8, frame %d" % f)


def test_graph_does_not_outlive_a_reconfigure(gpu, oracle):
    """Bug 2 (a graph replayed over freed tables): host calls at 640x480 (the graph is recorded), one device call at
    1000x200 with a cap no larger than the host calls' -- wider, so the per-column tables (d_ctab, d_bcol, d_xtab, the
    strip tables) grow and are re-allocated, but fewer pyramid bytes, so d_pyr and every buffer of the graph key stay
    where they were -- then host calls at 640x480 again.  Before the fix the key still matched and the replay used the
    freed table addresses; now configure() drops the graph, and a new one is recorded."""
    from orb_slam2_map_amd.synth import Stream
    s = Seq(gpu, oracle, nfeat=600, nlevels=4)  # (1000x200 has 4 usable levels)
    a = Stream(640, 480, 99).frame(1)[0][None]
    wide = Stream(1000, 200, 99).frame(2)[0][None]
    cap = s.ge.max_keypoints(640, 480)
    for _ in range(3):
        s.host(a, cap=cap)
    rec, rep = s.counts()
    assert rec >= 1 and rep >= 1
    s.device(wide, cap=min(cap, s.ge.max_keypoints(1000, 200)))
    for _ in range(3):
        s.host(a, cap=cap)
    rec2, rep2 = s.counts()
    assert rec2 == rec + 1 and rep2 == rep + 1, "reconfigure -> plain, record, replay: %s -> %s" % ((rec, rep), (rec2, rep2))
    s.stages(a[0], 0, "640x480 after a 1000x200 device call")


def pyramid_bytes(ge, w, h, batch):
    """Bytes of the padded pyramid of `batch` frames at w x h (d_pyr: 64-byte pitches, planes on 256-byte boundaries)."""
    total = 0
    for s in ge.GetInverseScaleFactors():
        lw, lh = int(np.rint(np.float32(w) * s)), int(np.rint(np.float32(h) * s))
        pitch = (lw + 38 + 63) // 64 * 64
        total += (pitch * (lh + 38) + 255) // 256 * 256
    return total * batch


@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("where", ["table", "pyramid"])
def test_failed_reconfigure_leaves_the_handle_unconfigured(gpu, oracle, entry, where, monkeypatch):
    """Bug 3 (a failed reconfigure left the handle half configured): a good call at A, a call at B that fails with
    ENOMEM under ORBGPU_DEBUG_FAIL_ALLOC_OVER, then A again and B again.  Before the fix configure() had written B's
    geometry into the handle, the failed reservation had freed the old buffer, and A's next call found the handle still
    "configured for A": its kernels ran with B's geometry over a null table.  where=table: threshold 0, B = 1000x200
    after A = 640x480 (no staging buffer grows: the first table reservation that allocates fails); where=pyramid: a
    threshold just under B's pyramid, B = 1280x960 (the tables fit, d_pyr fails)."""
    from orb_slam2_map_amd.synth import Stream
    if where == "table":
        s = Seq(gpu, oracle, nfeat=600, nlevels=4)
        a, b = Stream(640, 480, 7).frame(3)[0][None], Stream(1000, 200, 7).frame(4)[0][None]
        limit = 0
    else:
        s = Seq(gpu, oracle, nfeat=1000, nlevels=8)
        a, b = Stream(640, 480, 7).frame(3)[0][None], Stream(1280, 960, 7).frame(4)[0][None]
        limit = pyramid_bytes(s.ge, 1280, 960, 1) - 4096
        assert limit > pyramid_bytes(s.ge, 640, 480, 1) and limit > 1280 * 960
    cap = max(s.ge.max_keypoints(640, 480), s.ge.max_keypoints(b.shape[2], b.shape[1]))
    call = s.host if entry == "host" else s.device
    for _ in range(3):  # (host: the graph is recorded and replayed)
        call(a, cap=cap)
    monkeypatch.setenv("ORBGPU_DEBUG_FAIL_ALLOC_OVER", str(limit))
    with pytest.raises(gpu.OrbGpuError) as ei:
        call(b, cap=cap)
    monkeypatch.delenv("ORBGPU_DEBUG_FAIL_ALLOC_OVER")
    assert ei.value.status == gpu.ENOMEM, str(ei.value)
    msg = str(ei.value)
    assert "hipMalloc(" in msg, msg
    nbytes = int(msg.split("hipMalloc(")[1].split(")")[0])
    if where == "table":
        assert nbytes < (1 << 20), "expected a table reservation to fail: %s" % msg
    else:
        assert nbytes == pyramid_bytes(s.ge, 1280, 960, 1), "expected d_pyr to fail: %s" % msg
    with pytest.raises(gpu.OrbGpuError) as ei:
        s.ge.get_pyramid_level(0, 0)  # no last call to read: its planes are being replaced
    assert ei.value.status == gpu.EINVAL
    for img in (a, a, b, b, a):
        call(img, cap=cap)
    s.stages(a[0], 0, "A after a failed B")


def test_capacity_error_inside_the_graph_sequence(gpu, oracle, stream640):
    """ECAPACITY on the host entry point between replays, and on a replay itself: the next call with enough cap (same
    image) is exact, and the graph path resumes."""
    s = Seq(gpu, oracle)
    img = stream640.frame(5)[0][None]
    for _ in range(3):
        s.host(img)
    for _ in range(3):  # (the third of these is itself a replay)
        with pytest.raises(gpu.OrbGpuError) as ei:
            s.host(img, cap=50)
        assert ei.value.status == gpu.ECAPACITY
    rec, rep = s.counts()
    assert rep >= 2
    for _ in range(3):
        s.host(img)
    assert s.counts() == (rec + 1, rep + 1)
    s.stages(img[0], 0, "after ECAPACITY")


def test_option_toggles_between_replays(gpu, oracle, stream640):
    """set_fast_early_out, set_concurrent_blur and set_profiling toggled between replays of the host entry point; a
    device call with each schedule in between.  Every call exact; replays resume after each toggle."""
    s = Seq(gpu, oracle)
    imgs = [stream640.frame(10 + i)[0][None] for i in range(3)]
    batch8 = frames(stream640, 70, 8)
    steps = [("early_out", 1), ("blur", 1), ("profiling", 1), ("profiling", 0), ("early_out", 0), ("blur", 0)]
    for i in range(3):
        s.host(imgs[i % 3])
    for opt, on in steps:
        rep0 = s.counts()[1]
        {"early_out": s.ge.set_fast_early_out, "blur": s.ge.set_concurrent_blur, "profiling": s.ge.set_profiling}[opt](on)
        for i in range(3):
            s.host(imgs[i % 3])
        s.device(batch8)
        s.host(imgs[0])
        if opt == "profiling" and on:
            assert s.counts()[1] == rep0, "profiled calls launch plainly"
        else:
            assert s.counts()[1] > rep0, "%s=%d: the graph path must resume" % (opt, on)


@pytest.mark.parametrize("first", ["host", "device"])
def test_batch_size_sequence(gpu, oracle, stream640, first):
    """Batch sizes 1, 8, 3, 40, 7, 1 on one handle (max_batch 1), the entry point alternating: across the direct-mode
    threshold (8), QT_BATCH_MIN and OR_BATCH_MIN, and growth past max_batch and past the largest batch so far."""
    s = Seq(gpu, oracle)
    pool = frames(stream640, 0, 40)
    entries = [s.host, s.device] if first == "host" else [s.device, s.host]
    for i, b in enumerate((1, 8, 3, 40, 7, 1)):
        imgs = np.roll(pool, -5 * i, axis=0)[:b]
        entries[i % 2](imgs)
    s.host(pool[:8])
    s.host(pool[:8])
    s.stages(pool[7], 7, "batch of 8 after the sequence")


def _in_fresh_thread(fn):
    """fn() on a host thread of its own: its stateless calls find workspaces that own nothing yet."""
    import threading
    box = {}

    def body():
        try:
            box["value"] = fn()
        except BaseException as ex:  # noqa: BLE001 -- re-raised by the caller
            box["error"] = ex

    t = threading.Thread(target=body)
    t.start()
    t.join(120)
    assert not t.is_alive()
    if "error" in box:
        raise box["error"]
    return box["value"]


def _stateless_families(gpu, oracle):
    """(name, limit, call, check) per family of stateless entry points, on inputs of a few hundred rows: under
    ORBGPU_DEBUG_FAIL_ALLOC_OVER=limit a staging allocation of the call fails in a fresh thread; check(result) holds the
    result of the repeated call against the oracle or the model."""
    import scenario
    import pose_model
    import sim3_model
    import stereo_model
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import fuzz_pose
    import fuzz_sim3
    from orb_slam2_map_amd.synth import Stream, StereoStream
    st = Stream(640, 480, 77)
    oe = oracle.Extractor(300)
    (ka, da), (kb, db) = oe.extract(st.frame(1)[0]), oe.extract(st.frame(2)[0])
    fam = []
    # brute force: the matcher the workspace creates is refused first (the workspace is bound by then)
    want_bf = oracle.match_bf(da, ka["angle"], db, kb["angle"], nnratio=0.7)
    fam.append(("bf", 0, lambda: gpu.ORBmatcher(0.7, True).MatchBruteForce(da, ka["angle"], db, kb["angle"]),
                lambda got: got[0] == want_bf[0] and np.array_equal(got[1], want_bf[1])))
    # projection: the 4-byte frame arrays (1.2 KB) are uploaded, the descriptors (9.6 KB) refused: an error after an enqueue
    sf = np.asarray(oe.scale_factors(), np.float32)
    Tcw, rng = scenario.rigid(), np.random.default_rng(5)
    (px, py), (ox, oy) = st.offset(1), st.offset(2)
    P, _ = scenario.world_points_from_prev(ka, st.frame(1)[2], (ox - px, oy - py), st, Tcw, rng)
    mp = scenario.local_map(oracle, st, Tcw, P, da, ka["octave"], sf, rng, obs_zero_frac=0.1)
    of = scenario.make_frame(oracle, kb, db, st.frame(2)[2], st, sf)
    gf = gpu.Frame(of.kp_x, of.kp_y, of.octave, of.angle, of.u_right, of.desc, float(of.max_x), float(of.max_y), of.scale_factors)
    k0 = np.full(of.n, -1, np.int32)
    want_pj = oracle.search_by_projection(of, mp, 3.0, 0.8, k0)
    assert 4 * of.n < 5000 < 32 * of.n
    fam.append(("projection", 5000, lambda: gpu.ORBmatcher(0.8, True).SearchByProjection(gf, mp, 3.0, k0),
                lambda got: got[0] == want_pj[0] and np.array_equal(got[1], want_pj[1])))
    # pose: the first staging buffer is refused
    sc = pose_model.make_scene(300, 4243)
    n = sc["n"]
    has, wp = (sc["kp_to_mp"] >= 0).astype(np.uint8), sc["world_pos"][sc["kp_to_mp"].clip(0)]
    fr = gpu.Frame(sc["kps_xy"][:, 0], sc["kps_xy"][:, 1], sc["octave"], np.zeros(n, np.float32), sc["u_right"],
                   np.zeros((n, 32), np.uint8), 640, 480, np.ones(pose_model.NLEVELS, np.float32))
    fx, fy, cx, cy, bf = (float(k) for k in sc["K"])

    def check_pose(got):
        rep = fuzz_pose.compare([sc], [(b"", got[3], got[2])])
        return rep["compared"] == 1 and not rep["mismatches"]

    fam.append(("pose", 0, lambda: gpu.pose_optimization(fr, has, wp, sc["Tcw"], sc["inv_level_sigma2"], fx, fy, cx, cy, bf,
                                                         outlier=np.full(n, fuzz_pose.SENTINEL, np.uint8)), check_pose))
    # sim3: the two host blocks (7 KB, 8 KB) are uploaded, the device flavour's records (48 n1 = 9.6 KB) refused: an
    # error after an enqueue
    s3 = sim3_model.make_scene(120, 31, n1=200, n_hyp=50)
    models, spread = fuzz_sim3.model_pass([s3])
    m = models[0]
    keep = ~fuzz_sim3.left_out(m, fuzz_sim3.MARGIN_FACTOR * fuzz_sim3.BOUND_FACTOR * spread)
    assert keep[:m["iterations"]].all(), "the scene must leave no scanned hypothesis to the margins"

    def check_sim3(got):
        u = m["n_use"]
        return (np.array_equal(got["counts"][:u][keep], m["counts"][:u][keep]) and
                all(got[k] == int(m[k]) for k in ("accepted", "n_inliers", "no_more", "best_inliers", "best_iteration", "iterations")))

    fam.append(("sim3", 9000, lambda: gpu.sim3_solve(s3["valid"], s3["Xw1"], s3["Xw2"], s3["octave1"], s3["octave2"], s3["T1w"],
                                                     s3["T2w"], s3["K1"], s3["K2"], s3["level_sigma2"], s3["triples"],
                                                     s3["fix_scale"], s3["probability"], s3["min_inliers"], s3["max_iterations"]),
                check_sim3))
    # stereo: the first staging buffer is refused
    ss = StereoStream(320, 240, 12)
    left, right, _ = ss.frame(1)
    gl, gr, ol, orr = gpu.ORBextractor(300), gpu.ORBextractor(300), oracle.Extractor(300), oracle.Extractor(300)
    (kl, dl), (kr, dr) = gl(left), gr(right)
    ol.extract(left), orr.extract(right)
    u, d, _ = stereo_model.stereo_matches(kl, dl, kr, dr, stereo_model.oracle_planes(ol), stereo_model.oracle_planes(orr),
                                          ol.scale_factors(), ol.inv_scale_factors(), ss.bf, ss.fx)
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.int32)  # noqa: E731
    fam.append(("stereo", 0, lambda: gpu.compute_stereo_matches(gl, gr, kl, dl, kr, dr, ss.bf, ss.fx),
                lambda got: np.array_equal(bits(got[0]), bits(u)) and np.array_equal(bits(got[1]), bits(d))))
    return fam


def test_stateless_entry_points_recover_from_a_refused_staging_allocation(gpu, oracle, monkeypatch):
    """One host entry of each family of stateless entry points (brute force, projection, pose, sim3, stereo), each on a
    fresh thread, whose workspace owns nothing yet: under ORBGPU_DEBUG_FAIL_ALLOC_OVER a staging allocation is refused
    and the call returns ENOMEM -- for projection and sim3 after uploads from the caller's arrays were enqueued, which
    the entry waits for before it returns; with the hook cleared the same call on the same thread, so on the workspace
    the failure left behind, gives the oracle's (the model's) result."""
    for name, limit, call, check in _stateless_families(gpu, oracle):
        def case():
            monkeypatch.setenv("ORBGPU_DEBUG_FAIL_ALLOC_OVER", str(limit))
            with pytest.raises(gpu.OrbGpuError) as ei:
                call()
            monkeypatch.delenv("ORBGPU_DEBUG_FAIL_ALLOC_OVER")
            assert ei.value.status == gpu.ENOMEM and "hipMalloc(" in str(ei.value), "%s: %s" % (name, ei.value)
            return call()

        assert check(_in_fresh_thread(case)), "%s: the call after the refused one differs from the reference" % name


CHILD = r"""
import ctypes as C, os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from orb_slam2_map_amd import lib as G
from orb_slam2_map_amd.synth import Stream
from oracle import oracle_py as O
L = G.lib()
h = C.c_void_p()
rc = L.orbgpu_matcher_create(0, 2 ** 31 - 1, 4096, C.byref(h))
assert rc == G.ENOMEM, ("oversized matcher", rc)
print("matcher_create ENOMEM", flush=True)
os.environ["ORBGPU_DEBUG_FAIL_ALLOC_OVER"] = "0"
rc = L.orbgpu_mappoint_table_create(0, 0, C.byref(h))
assert rc == G.ENOMEM, ("table", rc)
print("mappoint_table_create ENOMEM", flush=True)
st = Stream(640, 480, 1234)
k0, d0 = O.Extractor(1000).extract(st.frame(0)[0])
k1, d1 = O.Extractor(1000).extract(st.frame(1)[0])
try:
    G.ORBmatcher(0.7, True).MatchBruteForce(d0, k0["angle"], d1, k1["angle"])
    raise SystemExit("match_bf succeeded under the hook")
except G.OrbGpuError as ex:
    assert ex.status == G.ENOMEM, ex
print("match_bf ENOMEM", flush=True)
del os.environ["ORBGPU_DEBUG_FAIL_ALLOC_OVER"]
m = C.c_void_p()
assert L.orbgpu_matcher_create(0, 4, 2048, C.byref(m)) == G.OK
t = C.c_void_p()
assert L.orbgpu_mappoint_table_create(0, 0, C.byref(t)) == G.OK
n, mb = G.ORBmatcher(0.7, True).MatchBruteForce(d0, k0["angle"], d1, k1["angle"])
no, mo = O.match_bf(d0, k0["angle"], d1, k1["angle"], nnratio=0.7)
assert n == no and np.array_equal(mb, mo), "match after the failures differs from the oracle"
assert L.orbgpu_matcher_destroy(m) == G.OK and L.orbgpu_mappoint_table_destroy(t) == G.OK
print("child ok: %d matches" % n, flush=True)
"""


def test_failed_creates_do_not_deadlock(gpu, oracle):
    """The create deadlock: orbgpu_matcher_create and orbgpu_mappoint_table_create called the public destroy on their
    error paths while holding the (non-recursive) lifecycle mutex, so an ENOMEM hung the thread and every later create
    and destroy of the process.  In a child process (a regression fails on the timeout instead of hanging the suite):
    orbgpu_matcher_create(0, 2^31-1, 4096) -> ENOMEM (hipMalloc refuses the size); under ORBGPU_DEBUG_FAIL_ALLOC_OVER=0
    orbgpu_mappoint_table_create(0, 0) -> ENOMEM and the first orbgpu_match_bf (its matcher is created on that path) ->
    ENOMEM; with the hook unset a create of each, one match (equal to the oracle) and the destroys succeed."""
    env = {k: v for k, v in os.environ.items() if k not in HOOKS}
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0, r.stdout[-3000:]
    assert lines and lines[-1].startswith("child ok"), r.stdout[-3000:]
