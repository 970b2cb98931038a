"""Frame::ComputeStereoMatches on the device (orbgpu_compute_stereo_matches / orbgpu_stereo_matches_batch_device)
against the CPU restatement in stereo_model.py, compared as bit patterns."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import stereo_model as M  # noqa: E402

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.fixture(scope="module")
def G():
    from orb_slam2_map_amd import lib
    if lib.device_count() < 1:
        pytest.skip("no HIP device")
    return lib


@pytest.fixture(scope="module")
def O():
    from oracle import oracle_py
    return oracle_py


class Pair:
    """One stereo pair extracted by two GPU handles (host entry) and by the oracle, with the model's answer."""

    def __init__(self, G, O, st, t, nfeatures):
        self.st = st
        self.left, self.right, _ = st.frame(t)
        self.gl, self.gr = G.ORBextractor(nfeatures), G.ORBextractor(nfeatures)
        self.kl, self.dl = self.gl(self.left)
        self.kr, self.dr = self.gr(self.right)
        self.ol, self.orr = O.Extractor(nfeatures), O.Extractor(nfeatures)
        okl, odl = self.ol.extract(self.left)
        okr, odr = self.orr.extract(self.right)
        assert self.kl.tobytes() == okl.tobytes() and np.array_equal(self.dl, odl), "left key points differ from the oracle"
        assert self.kr.tobytes() == okr.tobytes() and np.array_equal(self.dr, odr), "right key points differ from the oracle"
        self.pl, self.pr = M.oracle_planes(self.ol), M.oracle_planes(self.orr)
        self.scale, self.inv_scale = self.ol.scale_factors(), self.ol.inv_scale_factors()

    def model(self, kl=None, dl=None, kr=None, dr=None, mbf=None):
        kl = self.kl if kl is None else kl
        return M.stereo_matches(kl, self.dl if dl is None else dl, self.kr if kr is None else kr,
                                self.dr if dr is None else dr, self.pl, self.pr, self.scale, self.inv_scale,
                                self.st.bf if mbf is None else mbf, self.st.fx)

    def gpu(self, G, kl=None, dl=None, kr=None, dr=None, mbf=None):
        return G.compute_stereo_matches(self.gl, self.gr, self.kl if kl is None else kl, self.dl if dl is None else dl,
                                        self.kr if kr is None else kr, self.dr if dr is None else dr,
                                        self.st.bf if mbf is None else mbf, self.st.fx)


@pytest.fixture(scope="module")
def kitti(G, O):
    from orb_slam2_map_amd.synth import StereoStream
    return Pair(G, O, StereoStream(1241, 376, 11), 0, 2000)


@pytest.fixture(scope="module")
def vga(G, O):
    from orb_slam2_map_amd.synth import StereoStream
    return Pair(G, O, StereoStream(640, 480, 12), 1, 1000)


@pytest.mark.parametrize("which", ["kitti", "vga"])
def test_host_entry_equals_model(G, request, which):
    P = request.getfixturevalue(which)
    u, d, reason = P.model()
    gu, gd = P.gpu(G)
    assert np.array_equal(_bits(gu), _bits(u))
    assert np.array_equal(_bits(gd), _bits(d))
    assert M.n_stereo(reason) > len(P.kl) // 3  # a real stereo pair: most key points are matched
    assert (reason == M.R_CUT).sum() > 0


def test_crafted_lists_over_real_pyramids(G, kitti, vga):
    seen = np.zeros(len(M.REASONS), np.int64)
    for P in (kitti, vga):
        for seed in range(3):
            rng = np.random.default_rng(seed)
            kl, dl, kr, dr = M.craft_lists(P.kl, P.dl, P.kr, P.dr, rng, P.st.w, P.st.h, 8)
            for mbf in (P.st.bf, np.float32(P.st.bf / 20)):  # a small mbf: disparities >= maxD
                u, d, reason = P.model(kl, dl, kr, dr, mbf)
                gu, gd = P.gpu(G, kl, dl, kr, dr, mbf)
                assert np.array_equal(_bits(gu), _bits(u)), (seed, mbf)
                assert np.array_equal(_bits(gd), _bits(d)), (seed, mbf)
                seen += np.bincount(reason, minlength=len(M.REASONS))
    for r in ("no_candidate", "th_high", "right_bound", "edge", "disparity", "cut", "accepted", "plane"):
        assert seen[M.REASONS.index(r)] > 0, r


def test_th_high_ties_and_min_disparity(G, kitti):
    P = kitti
    rng = np.random.default_rng(5)
    u0, _, reason0 = P.model()
    i = int(np.nonzero(reason0 == M.R_OK)[0][0])
    kl, dl = P.kl[i:i + 1].copy(), P.dl[i:i + 1].copy()
    for dist, expect_th in ((99, False), (100, True)):
        kr = kl.copy()
        dr = M.flip_bits(dl[0], dist, rng)[None]
        u, d, reason = P.model(kl, dl, kr, dr)
        assert (reason[0] == M.R_THHIGH) == expect_th
        gu, gd = P.gpu(G, kl, dl, kr, dr)
        assert _bits(gu).tolist() == _bits(u).tolist() and _bits(gd).tolist() == _bits(d).tolist()
    # equal distances: the lowest right index wins (its x decides the SAD windows)
    kr = np.concatenate([kl, kl]).copy()
    kr["x"][0] = kl["x"][0] - 2.0
    kr["x"][1] = kl["x"][0] - 1.0
    dr = np.concatenate([dl, dl])
    for order in ((0, 1), (1, 0)):
        u, d, _ = P.model(kl, dl, kr[list(order)], dr[list(order)])
        gu, gd = P.gpu(G, kl, dl, kr[list(order)], dr[list(order)])
        assert _bits(gu).tolist() == _bits(u).tolist() and _bits(gd).tolist() == _bits(d).tolist()
    # minD = -3: a right key point at uL + 3 is a candidate, at uL + 3.5 it is not
    for off, cand in ((3.0, True), (3.5, False)):
        kr = kl.copy()
        kr["x"] = kl["x"] + np.float32(off)
        u, d, reason = P.model(kl, dl, kr, dl)
        assert (reason[0] != M.R_THHIGH) == cand
        gu, gd = P.gpu(G, kl, dl, kr, dl)
        assert _bits(gu).tolist() == _bits(u).tolist() and _bits(gd).tolist() == _bits(d).tolist()


def test_empty_lists_and_no_match(G, kitti):
    P = kitti
    gu, gd = P.gpu(G, P.kl[:0], P.dl[:0])
    assert len(gu) == 0 and len(gd) == 0
    gu, gd = P.gpu(G, kr=P.kr[:0], dr=P.dr[:0])
    assert (gu == -1).all() and (gd == -1).all()
    # a frame without any match: nothing is cut, nothing faults
    kl = P.kl.copy()
    kl["octave"] = 99
    gu, gd = P.gpu(G, kl)
    assert (gu == -1).all() and (gd == -1).all()


def test_zero_disparity_clamp(G, O):
    """Both images mirrored about column c (different noise): a key point at (c, y) matched at uR = c has
    d(incR = -1) = d(incR = +1), so deltaR = 0 and the disparity is exactly 0 -- the 0.01 clamp (Frame.cc:615-617)."""
    w, h, c = 640, 480, 320
    left, right = M.mirrored_pair(w, h, c, 21)
    gl, gr = G.ORBextractor(1000), G.ORBextractor(1000)
    kl, dl = gl(left)
    kr, dr = gr(right)
    ol, orr = O.Extractor(1000), O.Extractor(1000)
    ol.extract(left)
    orr.extract(right)
    kl, dl, kr, dr = M.clamp_keys(kl, dl, kr, dr, c, h)
    u, d, reason = M.stereo_matches(kl, dl, kr, dr, M.oracle_planes(ol), M.oracle_planes(orr), ol.scale_factors(),
                                    ol.inv_scale_factors(), 380.0, 700.0)
    assert (reason == M.R_CLAMP).any()
    gu, gd = G.compute_stereo_matches(gl, gr, kl, dl, kr, dr, 380.0, 700.0)
    assert np.array_equal(_bits(gu), _bits(u)) and np.array_equal(_bits(gd), _bits(d))


def _device_batch(G, torch, st, B, nfeatures, shared):
    """B pairs on the device: one handle over 2B frames (left images, then right images) or two handles over B each."""
    frames = [st.frame(t) for t in range(B)]
    L = np.stack([f[0] for f in frames])
    R = np.stack([f[1] for f in frames])
    w, h = st.w, st.h
    probe = G.ORBextractor(nfeatures)
    cap = probe.max_keypoints(w, h)
    probe.close()

    def extract(ext, imgs):
        d_img = torch.from_numpy(imgs).cuda()
        n = len(imgs)
        k = torch.zeros((n, cap, 7), dtype=torch.float32, device="cuda")
        d = torch.zeros((n, cap, 32), dtype=torch.uint8, device="cuda")
        c = torch.zeros(n, dtype=torch.int32, device="cuda")
        ext.extract_batch_device(d_img.data_ptr(), n, w, h, w, w * h, k.data_ptr(), d.data_ptr(), cap, c.data_ptr(), 0)
        return d_img, k, d, c

    if shared:
        el = er = G.ORBextractor(nfeatures, max_batch=2 * B)
        img, k, d, c = extract(el, np.concatenate([L, R]))
        kl, dl, nl, kr, dr, nr = k[:B], d[:B], c[:B], k[B:], d[B:], c[B:]
        lf0, rf0 = 0, B
        keep = (img,)
    else:
        el, er = G.ORBextractor(nfeatures, max_batch=B), G.ORBextractor(nfeatures, max_batch=B)
        imgl, kl, dl, nl = extract(el, L)
        imgr, kr, dr, nr = extract(er, R)
        lf0 = rf0 = 0
        keep = (imgl, imgr)
    u = torch.zeros((B, cap), dtype=torch.float32, device="cuda")
    z = torch.zeros((B, cap), dtype=torch.float32, device="cuda")
    ns = torch.zeros(B, dtype=torch.int32, device="cuda")
    run = lambda: G.stereo_matches_batch_device(el, lf0, er, rf0, B, cap, kl.data_ptr(), nl.data_ptr(), dl.data_ptr(),
                                                kr.data_ptr(), nr.data_ptr(), dr.data_ptr(), st.bf, st.fx, u.data_ptr(),
                                                z.data_ptr(), ns.data_ptr(), 0)
    run()
    torch.cuda.synchronize()
    return dict(el=el, er=er, keep=keep, kl=kl, dl=dl, nl=nl, kr=kr, dr=dr, nr=nr, u=u, z=z, ns=ns, run=run, L=L, R=R,
                cap=cap, lf0=lf0, rf0=rf0)


@pytest.mark.parametrize("shared", [True, False])
def test_batched_device_equals_host_entry(G, O, shared):
    torch = pytest.importorskip("torch")
    from orb_slam2_map_amd.synth import StereoStream
    st = StereoStream(640, 480, 13)
    B = 4
    D = _device_batch(G, torch, st, B, 1000, shared)
    nl, nr, ns = D["nl"].cpu().numpy(), D["nr"].cpu().numpy(), D["ns"].cpu().numpy()
    hl, hr = G.ORBextractor(1000), G.ORBextractor(1000)
    ol, orr = O.Extractor(1000), O.Extractor(1000)
    for p in range(B):
        kl = D["kl"][p, :nl[p]].cpu().numpy().view(G.KEYPOINT_DTYPE).reshape(-1)
        kr = D["kr"][p, :nr[p]].cpu().numpy().view(G.KEYPOINT_DTYPE).reshape(-1)
        dl, dr = D["dl"][p, :nl[p]].cpu().numpy(), D["dr"][p, :nr[p]].cpu().numpy()
        hl(D["L"][p])
        hr(D["R"][p])
        hu, hz = G.compute_stereo_matches(hl, hr, kl, dl, kr, dr, st.bf, st.fx)
        assert np.array_equal(_bits(D["u"][p, :nl[p]].cpu().numpy()), _bits(hu)), p
        assert np.array_equal(_bits(D["z"][p, :nl[p]].cpu().numpy()), _bits(hz)), p
        assert (D["u"][p, nl[p]:].cpu().numpy() == -1).all()
        ol.extract(D["L"][p])
        orr.extract(D["R"][p])
        _, _, reason = M.stereo_matches(kl, dl, kr, dr, M.oracle_planes(ol), M.oracle_planes(orr), ol.scale_factors(),
                                        ol.inv_scale_factors(), st.bf, st.fx)
        assert ns[p] == M.n_stereo(reason), p


def test_direct_mode_reads_the_callers_level0(G):
    """8 frames of 640 px: the extraction runs in direct mode (level 0 is never copied).  The stereo call reads the
    caller's images; it neither materialises the plane nor changes its answer once a getter has."""
    torch = pytest.importorskip("torch")
    from orb_slam2_map_amd.synth import StereoStream
    st = StereoStream(640, 480, 14)
    D = _device_batch(G, torch, st, 4, 1000, True)
    u0, z0 = D["u"].clone(), D["z"].clone()
    D["run"]()
    torch.cuda.synchronize()
    assert torch.equal(D["u"].view(torch.int32), u0.view(torch.int32))
    # the stereo calls did not materialise level 0: after the caller's buffer changes, the getter returns the new bytes
    img = D["keep"][0]
    saved = img.clone()
    img[0].fill_(77)
    torch.cuda.synchronize()
    lvl0, _, _ = D["el"].get_pyramid_level(0, 0)
    assert (lvl0 == 77).all()
    # now level 0 is materialised (from the overwritten image): restore the caller's buffer; the stereo call reads it
    img.copy_(saved)
    torch.cuda.synchronize()
    D["run"]()
    torch.cuda.synchronize()
    assert torch.equal(D["u"].view(torch.int32), u0.view(torch.int32))
    assert torch.equal(D["z"].view(torch.int32), z0.view(torch.int32))


def test_invalid_handle_combinations(G):
    from orb_slam2_map_amd.synth import StereoStream
    st = StereoStream(640, 480, 15)
    l, r, _ = st.frame(0)
    a, b = G.ORBextractor(1000), G.ORBextractor(1000)
    k, d = a(l)
    with pytest.raises(G.OrbGpuError) as ei:  # b has no last call
        G.compute_stereo_matches(a, b, k, d, k, d, st.bf, st.fx)
    assert ei.value.status == G.EINVAL
    b(r[:, :600].copy())
    with pytest.raises(G.OrbGpuError) as ei:  # image sizes differ
        G.compute_stereo_matches(a, b, k, d, k, d, st.bf, st.fx)
    assert ei.value.status == G.EINVAL
    c = G.ORBextractor(1000, nlevels=7)
    c(r)
    with pytest.raises(G.OrbGpuError) as ei:  # levels differ
        G.compute_stereo_matches(a, c, k, d, k, d, st.bf, st.fx)
    assert ei.value.status == G.EINVAL
    e = G.ORBextractor(1000, scaleFactor=1.25)
    e(r)
    with pytest.raises(G.OrbGpuError) as ei:  # scale factors differ
        G.compute_stereo_matches(a, e, k, d, k, d, st.bf, st.fx)
    assert ei.value.status == G.EINVAL
    b(r)
    dummy = np.zeros(64, np.uint8).ctypes.data
    for lf0, rf0, batch in ((1, 0, 1), (0, 0, 2), (-1, 0, 1)):  # frame ranges outside the last call (one frame each)
        with pytest.raises(G.OrbGpuError) as ei:
            G.stereo_matches_batch_device(a, lf0, b, rf0, batch, 8, dummy, dummy, dummy, dummy, dummy, dummy, st.bf, st.fx,
                                          dummy, dummy)
        assert ei.value.status == G.EINVAL


def test_fuzz_slice(G):
    import subprocess
    root = os.path.dirname(HERE)
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_stereo.py"), "5", "7"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and " mismatches 0" in r.stdout, r.stdout[-3000:]
    assert "rounds 0 " not in r.stdout


def _stereo_map(kl, dl, u, d, fx, cx, cy, sf, rng):
    """Map points of a stereo frame (Tcw = I): the left key points with a depth, back-projected and jittered, each with
    the key point's descriptor (a few bits flipped), a normal towards the camera and distance bounds whose predicted
    level is the key point's octave."""
    sel = np.nonzero(d > 0)[0]
    z = d[sel].astype(np.float64)
    x = (kl["x"][sel] - cx) * z / fx
    y = (kl["y"][sel] - cy) * z / fx
    P = np.stack([x, y, z], 1) * (1.0 + rng.uniform(-0.004, 0.004, (len(sel), 1)))
    dist = np.linalg.norm(P, axis=1)
    oct_ = kl["octave"][sel].astype(np.float64)
    desc = np.stack([M.flip_bits(dl[i], int(rng.integers(0, 12)), rng) for i in sel])
    return {"world_pos": P.astype(np.float32), "normal": (P / dist[:, None]).astype(np.float32),
            "min_dist": (0.5 * dist).astype(np.float32),
            "max_dist": (dist * float(sf[1]) ** (oct_ - 0.5)).astype(np.float32), "desc": desc,
            "skip": np.zeros(len(sel), np.uint8), "obs_pos": np.ones(len(sel), np.uint8)}


@pytest.mark.parametrize("shared", [True, False])
def test_stereo_frame_through_search_local_points(G, O, shared):
    """extract -> stereo -> frame glue without depth -> SearchLocalPoints, all on the device, with the device frame
    view's u_right = the stereo output of the pair; against the oracle's search_local_points fed the model's u_right."""
    torch = pytest.importorskip("torch")
    from orb_slam2_map_amd.synth import StereoStream
    st = StereoStream(640, 480, 17)
    B, w, h = 3, st.w, st.h
    D = _device_batch(G, torch, st, B, 1000, shared)
    cap = D["cap"]
    fx = float(st.fx)
    cx, cy = float(np.float32(w / 2)), float(np.float32(h / 2))
    cam = G.make_camera(fx, fx, cx, cy, float(st.bf), w, h)
    cs = torch.zeros((B, 64 * 48 + 1), dtype=torch.int32, device="cuda")
    items = torch.zeros((B, cap), dtype=torch.int32, device="cuda")
    G.frame_glue_batch_device(B, cap, D["kl"].data_ptr(), D["nl"].data_ptr(), None, 0, 0, cam, None, None, None,
                              cs.data_ptr(), items.data_ptr(), 0)
    torch.cuda.synchronize()
    sf = np.asarray(D["el"].GetScaleFactors(), np.float32)
    log_sf = float(np.log(np.float32(sf[1])))
    Tcw = np.eye(4, dtype=np.float32)
    nl, nr = D["nl"].cpu().numpy(), D["nr"].cpu().numpy()
    ol, orr = O.Extractor(1000), O.Extractor(1000)
    rng = np.random.default_rng(31)
    for p in range(B):
        kl = D["kl"][p, :nl[p]].cpu().numpy().view(G.KEYPOINT_DTYPE).reshape(-1)
        kr = D["kr"][p, :nr[p]].cpu().numpy().view(G.KEYPOINT_DTYPE).reshape(-1)
        dl, dr = D["dl"][p, :nl[p]].cpu().numpy(), D["dr"][p, :nr[p]].cpu().numpy()
        ol.extract(D["L"][p])
        orr.extract(D["R"][p])
        u, d, _ = M.stereo_matches(kl, dl, kr, dr, M.oracle_planes(ol), M.oracle_planes(orr), ol.scale_factors(),
                                   ol.inv_scale_factors(), st.bf, st.fx)
        assert np.array_equal(_bits(D["u"][p, :nl[p]].cpu().numpy()), _bits(u)), p
        table = _stereo_map(kl, dl, u, d, fx, cx, cy, sf, rng)
        m = len(table["min_dist"])
        of = O.Frame(kl["x"], kl["y"], kl["octave"], kl["angle"], u, dl, w, h, sf)
        no, ko, _, _ = O.search_local_points(of, Tcw, fx, fx, cx, cy, float(st.bf), table, log_sf)
        assert no > 100, no
        assert (ko >= 0).sum() > 0 and (u[ko >= 0] > 0).sum() > 50  # matches of key points that have a right coordinate
        dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in table.items()}
        tb = G.DeviceMapPointTable()
        tb.m = m
        for k in dev:
            setattr(tb, k, dev[k].data_ptr())
        fv = G.DeviceFrameView()
        fv.cap, fv.n = cap, D["nl"].data_ptr() + 4 * p
        fv.kps, fv.desc = D["kl"].data_ptr() + 28 * cap * p, D["dl"].data_ptr() + 32 * cap * p
        fv.u_right = D["u"].data_ptr() + 4 * cap * p  # the stereo output of pair p
        fv.cell_start, fv.cell_items = cs.data_ptr() + 4 * (64 * 48 + 1) * p, items.data_ptr() + 4 * cap * p
        fv.nlevels, fv.scale_factors = len(sf), sf.ctypes.data
        fv.min_x, fv.max_x, fv.min_y, fv.max_y = 0.0, float(w), 0.0, float(h)
        k2m = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
        counts = torch.zeros(2, dtype=torch.int32, device="cuda")
        G.search_local_points_device(fv, tb, Tcw, fx, fx, cx, cy, float(st.bf), log_sf, 3.0, 0.8, k2m.data_ptr(),
                                     counts.data_ptr(), None, stream=0)
        torch.cuda.synchronize()
        assert int(counts[0]) == no, p
        assert np.array_equal(k2m.cpu().numpy()[:nl[p]], ko), p


def test_ties_go_to_the_lowest_right_index(G, kitti):
    """Two right key points at the same (lowest) distance, far apart: the one with the lower index decides the SAD
    windows, so swapping the indices changes the answer."""
    P = kitti
    _, _, reason0 = P.model()
    done = 0
    for i in np.nonzero(reason0 == M.R_OK)[0][:40]:
        kl, dl = P.kl[i:i + 1].copy(), P.dl[i:i + 1].copy()
        kr = np.concatenate([kl, kl]).copy()
        kr["x"][0] = kl["x"][0] - 2.0
        kr["x"][1] = kl["x"][0] - 30.0
        dr = np.concatenate([dl, dl])
        outs = []
        for order in ((0, 1), (1, 0)):
            u, d, _ = P.model(kl, dl, kr[list(order)], dr[list(order)])
            gu, gd = P.gpu(G, kl, dl, kr[list(order)], dr[list(order)])
            assert _bits(gu).tolist() == _bits(u).tolist() and _bits(gd).tolist() == _bits(d).tolist()
            outs.append(_bits(u).tolist())
        done += outs[0] != outs[1]
    assert done >= 5  # the choice is visible in the output for these key points


def test_sad_equal_to_threshold_is_cut(G, kitti):
    """SAD == 1.5f * 1.4f * median exactly: the reference cuts it (`< thDist` keeps, :632).  A list whose median SAD is
    m has thDist = 2.1 m: a five-key list of real matches whose SADs sort as [a, b, m, m, 2.1 m], with 2.1 m an integer
    SAD that some match has."""
    P = kitti
    _, _, reason0, sad0 = M.stereo_matches(P.kl, P.dl, P.kr, P.dr, P.pl, P.pr, P.scale, P.inv_scale, P.st.bf, P.st.fx,
                                           return_sad=True)
    sads = {}
    for i in np.nonzero(reason0 == M.R_OK)[0]:
        sads.setdefault(int(sad0[i]), []).append(int(i))
    th_of = lambda med: (np.float32(1.5) * np.float32(1.4)) * np.float32(med)
    pick = None
    for med in sorted(sads):
        th = th_of(med)
        if th == np.float32(int(th)) and int(th) in sads:
            pick = (med, int(th))
            break
    assert pick is not None, "no SAD pair (median, 2.1 x median) among the matches"
    med, top = pick
    # the list: one match at the threshold, two below the median, two at the median -> sorted [a, b, med, med, top]
    below = [s for s in sorted(sads) if s < med][:2]
    idx = [sads[below[0]][0], sads[below[-1]][-1], sads[med][0], sads[med][-1], sads[top][0]]
    kl, dl = P.kl[idx], P.dl[idx]
    u, d, reason = P.model(kl, dl)
    assert reason[-1] == M.R_CUT and (reason[:-1] != M.R_CUT).all(), reason
    gu, gd = P.gpu(G, kl, dl)
    assert _bits(gu).tolist() == _bits(u).tolist() and _bits(gd).tolist() == _bits(d).tolist()
