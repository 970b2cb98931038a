"""The matcher scenes of the rotation-histogram tests (test-side helper): the scenes the other matcher tests already
use, wrapped so that only the two angle arrays vary.  Every scene offers
    oracle(angle_a, angle_b, check)  -> (count, output[, prev_matched])
    gpu_flavours(gpu)                -> {name: the same call on the device}
    pairs()                          -> every row (i, j) the matcher accepts with the check off, in no particular order
    index                            -> "b": output[j] = i;  "a": output[i] = j
angle_a is the side the reference subtracts from (key frame / last frame / first frame), angle_b the other one.

`extractor_side` is the product library, or HostSide() where there is no device: the oracle's extractor yields the
same key points and descriptors (test_gpu_extractor.py, smoke()), so both build the same scenes."""
import numpy as np

import scenario
from oracle import oracle_py as O


class _HostExtractor:
    def __init__(self, nfeatures=1000, max_batch=1):
        self.e = O.Extractor(nfeatures)

    def extract_batch(self, imgs):
        r = [self.e.extract(g) for g in imgs]
        return [k for k, _ in r], [d for _, d in r]

    def GetScaleFactors(self):
        return self.e.scale_factors()

    def GetScaleSigmaSquares(self):
        return self.e.sigma2()


class HostSide:
    """Stands in for the product library where a scene builder only extracts and builds host frames."""
    ORBextractor = _HostExtractor
    Frame = O.Frame


def _with_angle(frame, angle):
    frame.angle = np.ascontiguousarray(angle, np.float32)
    return frame


def _gframe(gpu, of):
    return gpu.Frame(of.kp_x, of.kp_y, of.octave, of.angle, of.u_right, of.desc, float(of.max_x), float(of.max_y),
                     of.scale_factors)


class Scene:
    index = "b"

    def pairs(self):
        z = np.zeros(max(self.n_a, self.n_b, 1), np.float32)
        r = self.oracle(z[:self.n_a], z[:self.n_b], False)
        return self._visible(r[1])

    def _visible(self, out):
        s = np.nonzero(out >= 0)[0]
        return np.stack([out[s], s], 1) if self.index == "b" else np.stack([s, out[s]], 1)

    def unchecked(self):
        z = np.zeros(max(self.n_a, self.n_b, 1), np.float32)
        return self.oracle(z[:self.n_a], z[:self.n_b], False)


class BFScene(Scene):
    """Self-match of n random descriptors (the oracle's own CPU test): every row matches itself."""

    def __init__(self, n, seed=3):
        self.d = np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)
        self.n_a = self.n_b = n

    def oracle(self, aa, ab, check):
        return O.match_bf(self.d, aa, self.d, ab, nnratio=0.7, check_orientation=check)

    def gpu_flavours(self, gpu):
        return {"host": lambda aa, ab, check: gpu.ORBmatcher(0.7, check).MatchBruteForce(self.d, aa, self.d, ab)}


class EmptyBFScene(BFScene):
    """No A rows against 10 B rows."""

    def __init__(self):
        BFScene.__init__(self, 10)
        self.n_a = 0

    def oracle(self, aa, ab, check):
        return O.match_bf(self.d[:0], aa, self.d, ab, nnratio=0.7, check_orientation=check)

    def gpu_flavours(self, gpu):
        return {"host": lambda aa, ab, check: gpu.ORBmatcher(0.7, check).MatchBruteForce(self.d[:0], aa, self.d, ab)}


class BowScene(Scene):
    """SearchByBoW(KF, F) on two frames of the stream (test_gpu_bow.py::test_search_by_bow_on_extracted_frames)."""

    def __init__(self, side, levelsup=4, ratio=0.7, valid_frac=0.85, empty=False):
        from orb_slam2_map_amd.synth import Stream
        rng = np.random.default_rng(levelsup)
        self.v = scenario.synthetic_vocabulary(10, 4, 5 + levelsup, stop_frac=0.02)
        st = Stream(640, 480, 1234)
        ge = side.ORBextractor(1000, max_batch=2)
        (k0, k1), (d0, d1) = ge.extract_batch(np.stack([st.frame(40)[0], st.frame(41)[0]]))
        self._finish(d0, d1, (rng.random(len(k0)) < valid_frac).astype(np.uint8), levelsup, ratio)
        if empty:
            self.valid[:] = 0

    def _finish(self, d0, d1, valid, levelsup, ratio):
        v = self.v
        self.d0, self.d1, self.valid, self.levelsup, self.ratio = d0, d1, valid, levelsup, ratio
        self.ov = O.Vocabulary(v["k"], v["L"], v["parent"], v["is_leaf"], v["desc"], v["weight"])
        self.o0, self.o1 = self.ov.transform(d0, levelsup), self.ov.transform(d1, levelsup)
        self.n_a, self.n_b = len(d0), len(d1)

    def oracle(self, aa, ab, check):
        return O.search_by_bow(self.d0, aa, self.valid, self.o0, self.d1, ab, self.o1, 50, self.ratio, check)

    def _nodes(self, gpu):
        v = self.v
        gv = gpu.ORBVocabulary(v["k"], v["L"], v["parent"], v["is_leaf"], v["desc"], v["weight"])
        nodes = gv.transform(self.d0, self.levelsup)["node_id"], gv.transform(self.d1, self.levelsup)["node_id"]
        gv.close()
        return nodes

    def gpu_flavours(self, gpu):
        n0, n1 = self._nodes(gpu)
        return {"host": lambda aa, ab, check: gpu.search_by_bow(self.d0, aa, self.valid, n0, self.d1, ab, n1, 50,
                                                                self.ratio, check)}


class BowDuplicatesScene(BowScene):
    """test_gpu_bow.py::test_search_by_bow_conflicts_within_nodes: 40 features repeated 20 times under a 4 x 2 tree."""

    def __init__(self):
        from test_gpu_bow import _features
        rng = np.random.default_rng(9)
        self.v = scenario.synthetic_vocabulary(4, 2, 1)
        base = _features(self.v, 40, 1, p=0.02)
        dk = np.repeat(base, 20, axis=0)
        dk = np.packbits(np.unpackbits(dk, axis=1) ^ (rng.random((800, 256)) < 0.01).astype(np.uint8), axis=1)
        df = np.packbits(np.unpackbits(dk[rng.permutation(800)], axis=1) ^ (rng.random((800, 256)) < 0.01).astype(np.uint8),
                         axis=1)
        self._finish(dk, df, None, 1, 0.95)


class BowKeyFramesScene(Scene):
    """SearchByBoW(KF, KF) (test_gpu_matcher_m6.py::test_search_by_bow_keyframes)."""
    index = "a"

    def __init__(self, side, levelsup=3, ratio=0.75, empty=False):
        from test_gpu_matcher_m6 import _two_keyframes
        st, ge, fr, ks, ds, g, o, shift = _two_keyframes(side, O, 60, 61)
        rng = np.random.default_rng(levelsup)
        self.v = v = scenario.synthetic_vocabulary(10, 4, 8)
        self.ov = O.Vocabulary(10, 4, v["parent"], v["is_leaf"], v["desc"], v["weight"])
        self.ds, self.levelsup, self.ratio = ds, levelsup, ratio
        self.to = [self.ov.transform(d, levelsup) for d in ds]
        self.v1 = (rng.random(len(ks[0])) < 0.8).astype(np.uint8)
        self.v2 = (rng.random(len(ks[1])) < 0.8).astype(np.uint8)
        if empty:
            self.v2[:] = 0
        self.n_a, self.n_b = len(ds[0]), len(ds[1])

    def oracle(self, aa, ab, check):
        return O.search_by_bow_keyframes(self.ds[0], aa, self.v1, self.to[0], self.ds[1], ab, self.v2, self.to[1],
                                         self.ratio, check)

    def gpu_flavours(self, gpu):
        v = self.v
        gv = gpu.ORBVocabulary(10, 4, v["parent"], v["is_leaf"], v["desc"], v["weight"])
        nd = [gv.transform(d, self.levelsup)["node_id"] for d in self.ds]
        gv.close()
        return {"host": lambda aa, ab, check: gpu.search_by_bow_keyframes(self.ds[0], aa, self.v1, nd[0], self.ds[1], ab,
                                                                           self.v2, nd[1], self.ratio, check)}


class LastFrameScene(Scene):
    """SearchByProjection(CurrentFrame, LastFrame) (test_gpu_matcher_proj.py::test_search_by_projection_last_frame,
    th = 7, 40 % of the last frame's points without observations: those do not block, so a later row may take the
    same key point, and both rows vote)."""

    def __init__(self, side, th=7.0, obs_zero=0.4, empty=False):
        from orb_slam2_map_amd.synth import Stream
        rng = np.random.default_rng(int(th) + 5)
        self.st = st = Stream(640, 480, 1234)
        ge = side.ORBextractor(1000, max_batch=2)
        self.fr = fr = [st.frame(30), st.frame(31)]
        self.ks, self.ds = ks, ds = ge.extract_batch(np.stack([f[0] for f in fr]))
        self.sf = sf = np.asarray(ge.GetScaleFactors(), np.float32)
        self.Tcw = Tcw = scenario.rigid()
        self.ocur = scenario.make_frame(O, ks[1], ds[1], fr[1][2], st, sf)
        (px, py), (ox, oy) = st.offset(30), st.offset(31)
        P, _ = scenario.world_points_from_prev(ks[0], fr[0][2], (ox - px, oy - py), st, Tcw, rng)
        n = len(ks[0])
        self.last = {"has_mp": (rng.random(n) < 0.8).astype(np.uint8), "outlier": (rng.random(n) < 0.05).astype(np.uint8),
                     "obs_pos": (rng.random(n) >= obs_zero).astype(np.uint8), "world_pos": P, "desc": ds[0],
                     "kp_octave": ks[0]["octave"], "kp_angle": ks[0]["angle"], "Tcw": Tcw.copy()}
        if empty:
            self.last["has_mp"][:] = 0
        self.th = th
        self.cam = tuple(float(v) for v in (st.fx, st.fy, st.cx, st.cy, st.bf))
        self.n_a, self.n_b = n, self.ocur.n

    def _oracle(self, last, ab, check):
        fx, fy, cx, cy, bf = self.cam
        k0 = np.full(self.n_b, -1, np.int32)
        return O.search_by_projection_last(_with_angle(self.ocur, ab), self.Tcw, fx, fy, cx, cy, bf, bf / fx, last, self.th,
                                           False, check, k0)

    def oracle(self, aa, ab, check):
        return self._oracle(dict(self.last, kp_angle=np.ascontiguousarray(aa, np.float32)), ab, check)

    def pairs(self):
        """The output shows the last row per key point only.  A row can be taken over only if its point has no
        observations; what such a row chose is what the output shows right after it, that is with the rows behind it
        left out (they cannot have influenced it)."""
        z = np.zeros(max(self.n_a, self.n_b), np.float32)
        last = dict(self.last, kp_angle=z[:self.n_a])
        _, out = self._oracle(last, z[:self.n_b], False)
        found = {int(i): int(j) for i, j in self._visible(out)}
        hidden = [i for i in range(self.n_a) if last["has_mp"][i] and not last["obs_pos"][i] and i not in found]
        for i in hidden:
            has = last["has_mp"].copy()
            has[i + 1:] = 0
            _, out = self._oracle(dict(last, has_mp=has), z[:self.n_b], False)
            j = np.nonzero(out == i)[0]
            if len(j):
                found[i] = int(j[0])
        return np.array(sorted(found.items()), np.int64).reshape(-1, 2)

    def gpu_flavours(self, gpu):
        fx, fy, cx, cy, bf = self.cam
        mb = bf / fx
        last, Tcw, th = self.last, self.Tcw, self.th
        gcur = _gframe(gpu, self.ocur)
        olast = scenario.make_frame(O, self.ks[0], self.ds[0], self.fr[0][2], self.st, self.sf)
        k0 = np.full(self.n_b, -1, np.int32)

        def host(aa, ab, check):
            l2 = dict(last, kp_angle=np.ascontiguousarray(aa, np.float32))
            return gpu.ORBmatcher(0.9, check).SearchByProjectionLast(_with_angle(gcur, ab), Tcw, fx, fy, cx, cy, bf, mb, l2,
                                                                     th, False, k0)

        has = last["has_mp"] != 0
        ids = np.arange(self.n_a, dtype=np.int64) * 7 + 11
        tbl = gpu.MapPointTable()
        if has.any():
            tbl.upsert(ids[has], world_pos=last["world_pos"][has], desc=last["desc"][has],
                       n_obs=last["obs_pos"][has].astype(np.int32))
        last_ids = np.where(has, ids, -1)

        def table(aa, ab, check):
            dl = gpu.DeviceFrame().upload(_gframe(gpu, _with_angle(olast, aa)))
            dc = gpu.DeviceFrame().upload(_gframe(gpu, _with_angle(self.ocur, ab)))
            return gpu.search_by_projection_last_table(dc, Tcw, dl, Tcw, tbl, last_ids, fx, fy, cx, cy, bf, mb, th, False,
                                                       check, last_outlier=last["outlier"])

        def device(aa, ab, check):
            """Both frames as one batch of key-point records on the device (28-byte records, the angle at offset 12),
            the current one glued there."""
            import torch
            w, h = 640, 480
            cap = max(self.n_a, self.n_b) + 37
            rec = np.zeros((2, cap), gpu.KEYPOINT_DTYPE)
            rec[0, :self.n_a], rec[1, :self.n_b] = self.ks[0], self.ks[1]
            rec["angle"][0, :self.n_a], rec["angle"][1, :self.n_b] = aa, ab
            kps = torch.from_numpy(rec.view(np.float32).reshape(2, cap, 7).copy()).cuda()
            dsc = np.zeros((2, cap, 32), np.uint8)
            dsc[0, :self.n_a], dsc[1, :self.n_b] = self.ds[0], self.ds[1]
            desc = torch.from_numpy(dsc).cuda()
            nout = torch.tensor([self.n_a, self.n_b], dtype=torch.int32, device="cuda")
            depth = torch.from_numpy(np.stack([f[2] for f in self.fr])).cuda()
            s = torch.cuda.current_stream().cuda_stream
            ur, dz = (torch.zeros((2, cap), dtype=torch.float32, device="cuda") for _ in range(2))
            cs = torch.zeros((2, 64 * 48 + 1), dtype=torch.int32, device="cuda")
            items = torch.zeros((2, cap), dtype=torch.int32, device="cuda")
            cam = gpu.make_camera(fx, fy, cx, cy, bf, w, h)
            gpu.frame_glue_batch_device(2, cap, kps.data_ptr(), nout.data_ptr(), depth.data_ptr(), w, w * h, cam, None,
                                        ur.data_ptr(), dz.data_ptr(), cs.data_ptr(), items.data_ptr(), s)

            def padded(a, shape, dtype):
                out = np.zeros(shape, dtype)
                out[:len(a)] = a
                return torch.from_numpy(out).cuda()
            d_has, d_out, d_obs = (padded(last[k], cap, np.uint8) for k in ("has_mp", "outlier", "obs_pos"))
            d_wp = padded(last["world_pos"], (cap, 3), np.float32)
            sf = self.sf
            fv = gpu.DeviceFrameView()
            fv.cap, fv.n, fv.kps, fv.desc = cap, nout.data_ptr() + 4, kps.data_ptr() + cap * 28, desc.data_ptr() + cap * 32
            fv.u_right, fv.cell_start = ur.data_ptr() + cap * 4, cs.data_ptr() + (64 * 48 + 1) * 4
            fv.cell_items = items.data_ptr() + cap * 4
            fv.nlevels, fv.scale_factors = len(sf), sf.ctypes.data
            fv.min_x, fv.max_x, fv.min_y, fv.max_y = 0.0, float(w), 0.0, float(h)
            lv = gpu.DeviceLastFrameView()
            lv.cap, lv.n, lv.kps, lv.desc = cap, nout.data_ptr(), kps.data_ptr(), desc.data_ptr()
            lv.has_mp, lv.outlier, lv.obs_pos, lv.world_pos = d_has.data_ptr(), d_out.data_ptr(), d_obs.data_ptr(), d_wp.data_ptr()
            k2m = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
            counts = torch.zeros(2, dtype=torch.int32, device="cuda")
            gpu.search_by_projection_last_device(fv, Tcw, lv, Tcw, fx, fy, cx, cy, bf, mb, th, False, check, k2m.data_ptr(),
                                                 counts.data_ptr(), stream=s)
            torch.cuda.synchronize()
            c = counts.cpu().numpy()
            assert c[1] == 0
            return int(c[0]), k2m.cpu().numpy()[:self.n_b]
        return {"host": host, "table": table, "device": device}


class KeyFrameScene(Scene):
    """SearchByProjection(CurrentFrame, KeyFrame) (test_gpu_matcher_proj.py::test_search_by_projection_keyframe, the
    relocalisation scene with th = 10, ORBdist = 100)."""

    def __init__(self, side, th=10.0, orb_dist=100, empty=False):
        from orb_slam2_map_amd.synth import Stream
        rng = np.random.default_rng(int(th))
        st = Stream(640, 480, 1234)
        ge = side.ORBextractor(1000, max_batch=2)
        fr = [st.frame(40), st.frame(42)]
        ks, ds = ge.extract_batch(np.stack([f[0] for f in fr]))
        sf = np.asarray(ge.GetScaleFactors(), np.float32)
        self.Tcw = Tcw = scenario.rigid()
        self.ocur = scenario.make_frame(O, ks[1], ds[1], fr[1][2], st, sf)
        (px, py), (ox, oy) = st.offset(40), st.offset(42)
        P, _ = scenario.world_points_from_prev(ks[0], fr[0][2], (ox - px, oy - py), st, Tcw, rng)
        n = len(ks[0])
        T = Tcw.astype(np.float64)
        Ow = -T[:3, :3].T @ T[:3, 3]
        dist = np.linalg.norm(P.astype(np.float64) - Ow, axis=1)
        maxd = (dist * sf[ks[0]["octave"]]).astype(np.float32)
        mind = (maxd / sf[-1]).astype(np.float32)
        self.kf = {"has_mp": (rng.random(n) < 0.85).astype(np.uint8), "bad": (rng.random(n) < 0.03).astype(np.uint8),
                   "already_found": np.zeros(n, np.uint8), "world_pos": P, "min_dist_inv": np.float32(0.8) * mind,
                   "max_dist_inv": np.float32(1.2) * maxd, "max_dist": maxd, "desc": ds[0], "kp_angle": ks[0]["angle"]}
        if empty:
            self.kf["has_mp"][:] = 0
        self.k0 = np.full(self.ocur.n, -1, np.int32)
        self.k0[rng.choice(self.ocur.n, 100, replace=False)] = -2
        self.args = (float(st.fx), float(st.fy), float(st.cx), float(st.cy), float(np.log(np.float32(sf[1]))))
        self.th, self.orb_dist = th, orb_dist
        self.n_a, self.n_b = n, self.ocur.n

    def oracle(self, aa, ab, check):
        kf = dict(self.kf, kp_angle=np.ascontiguousarray(aa, np.float32))
        return O.search_by_projection_keyframe(_with_angle(self.ocur, ab), self.Tcw, *self.args, kf, self.th, self.orb_dist,
                                               check, self.k0)

    def gpu_flavours(self, gpu):
        gcur = _gframe(gpu, self.ocur)

        def host(aa, ab, check):
            kf = dict(self.kf, kp_angle=np.ascontiguousarray(aa, np.float32))
            return gpu.ORBmatcher(0.9, check).SearchByProjectionKeyFrame(_with_angle(gcur, ab), self.Tcw, *self.args, kf,
                                                                         self.th, self.orb_dist, self.k0)
        return {"host": host}


class TriangulationScene(Scene):
    """SearchForTriangulation (test_gpu_matcher_m6.py::test_search_for_triangulation).  Rows are independent: two rows
    may name the same key point of key frame 2, and the output is per row."""
    index = "a"

    def __init__(self, side, only_stereo, levelsup=3, empty=False):
        from test_gpu_matcher_m6 import _two_keyframes
        st, ge, fr, ks, ds, g, o, shift = _two_keyframes(side, O, 50, 52)
        rng = np.random.default_rng(levelsup)
        self.v = v = scenario.synthetic_vocabulary(10, 4, 31)
        self.ov = O.Vocabulary(10, 4, v["parent"], v["is_leaf"], v["desc"], v["weight"])
        self.ds, self.levelsup, self.only_stereo = ds, levelsup, only_stereo
        self.to = [self.ov.transform(d, levelsup) for d in ds]
        e = np.array([shift[0], shift[1], 0.0]) / max(np.hypot(*shift), 1e-9)
        self.F12 = np.array([[0, -e[2], e[1]], [e[2], 0, -e[0]], [-e[1], e[0], 0]], np.float32)
        self.ex, self.ey = float(320 + 1e6 * e[0]), float(240 + 1e6 * e[1])
        self.sig2 = np.asarray(ge.GetScaleSigmaSquares(), np.float32)
        frac = 1.1 if empty else 0.2
        self.h1 = (rng.random(len(ks[0])) < frac).astype(np.uint8)
        self.h2 = (rng.random(len(ks[1])) < 0.2).astype(np.uint8)
        self.o = [scenario.make_frame(O, ks[i], ds[i], fr[i][2], st, ge.GetScaleFactors()) for i in range(2)]
        self.n_a, self.n_b = self.o[0].n, self.o[1].n

    def oracle(self, aa, ab, check):
        o = self.o
        return O.search_for_triangulation(_with_angle(o[0], aa), self.h1, self.to[0], _with_angle(o[1], ab), self.h2,
                                          self.to[1], self.F12, self.ex, self.ey, self.sig2, self.only_stereo, check)

    def gpu_flavours(self, gpu):
        v = self.v
        gv = gpu.ORBVocabulary(10, 4, v["parent"], v["is_leaf"], v["desc"], v["weight"])
        nd = [gv.transform(d, self.levelsup)["node_id"] for d in self.ds]
        gv.close()
        g = [_gframe(gpu, f) for f in self.o]

        def host(aa, ab, check):
            return gpu.search_for_triangulation(_with_angle(g[0], aa), self.h1, nd[0], _with_angle(g[1], ab), self.h2, nd[1],
                                                self.F12, self.ex, self.ey, self.sig2, self.only_stereo, check)
        return {"host": host}


class InitializationScene(Scene):
    """SearchForInitialization (test_gpu_matcher_m6.py::test_search_for_initialization, window 100, ratio 0.9).  A
    stolen match leaves its vote behind, so pairs() (the rows that still hold a match) is not the list of voters."""
    index = "a"

    def __init__(self, side, window=100, ratio=0.9, empty=False):
        from orb_slam2_map_amd.synth import Stream
        st = Stream(640, 480, 1234)
        ge = side.ORBextractor(2000, max_batch=2)
        fr = [st.frame(70), st.frame(71)]
        ks, ds = ge.extract_batch(np.stack([f[0] for f in fr]))
        sf = ge.GetScaleFactors()
        self.of = [scenario.make_frame(O, ks[i], ds[i], fr[i][2], st, sf) for i in range(2)]
        if empty:
            self.of[0].octave[:] = 1  # only level-0 key points of the first frame are matched (ORBmatcher.cc:421-423)
        self.pm0 = np.stack([ks[0]["x"], ks[0]["y"]], 1).astype(np.float32)
        self.window, self.ratio = window, ratio
        self.n_a, self.n_b = self.of[0].n, self.of[1].n

    def oracle(self, aa, ab, check):
        return O.search_for_initialization(_with_angle(self.of[0], aa), _with_angle(self.of[1], ab), self.pm0, self.window,
                                           self.ratio, check)

    def gpu_flavours(self, gpu):
        g = [_gframe(gpu, f) for f in self.of]

        def host(aa, ab, check):
            return gpu.search_for_initialization(_with_angle(g[0], aa), _with_angle(g[1], ab), self.pm0, self.window,
                                                 self.ratio, check)
        return {"host": host}


class StealScene(InitializationScene):
    """A crafted SearchForInitialization: 30 level-0 key points in F2, and for each of them two key points of F1 one pixel
    apart whose 10-px windows hold that key point alone.  The earlier F1 row is 10 bits away from the F2 descriptor.
    For the first `n_steal` key points the later row is 5 bits away and steals the match (ORBmatcher.cc:459-470); for
    the others it is 20 bits away and, the key point being held at a smaller distance, finds no candidate at all.
    The robbed rows keep their votes (rotHist is never cleaned, :476-483), and the filter skips them (:497-501)."""

    def __init__(self, n_steal=8):
        rng = np.random.default_rng(17)
        n2 = 30
        self.n_steal = n_steal
        x2 = (60.0 + 70.0 * (np.arange(n2) % 8)).astype(np.float32)
        y2 = (60.0 + 90.0 * (np.arange(n2) // 8)).astype(np.float32)
        d2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)

        def flipped(d, nbits):
            bits = np.unpackbits(d)
            bits[rng.choice(256, nbits, replace=False)] ^= 1
            return np.packbits(bits)
        x1, y1, d1 = [], [], []
        for j in range(n2):
            x1 += [x2[j], x2[j] + 1.0]
            y1 += [y2[j], y2[j]]
            d1 += [flipped(d2[j], 10), flipped(d2[j], 5 if j < n_steal else 20)]
        x1, y1, d1 = np.asarray(x1, np.float32), np.asarray(y1, np.float32), np.stack(d1)
        sf = (np.float32(1.2) ** np.arange(8, dtype=np.float32)).astype(np.float32)

        def frame(x, y, d):
            n = len(x)
            return O.Frame(x, y, np.zeros(n, np.int32), np.zeros(n, np.float32), np.full(n, -1, np.float32), d, 640, 480, sf)
        self.of = [frame(x1, y1, d1), frame(x2, y2, d2)]
        self.pm0 = np.stack([x1, y1], 1)
        self.window, self.ratio = 10, 0.9
        self.n_a, self.n_b = 2 * n2, n2
        self.final_pairs = np.array([(2 * j + (j < n_steal), j) for j in range(n2)], np.int64)
        self.stale_pairs = np.array([(2 * j, j) for j in range(n_steal)], np.int64)

    def angles(self):
        """Live rows: 15 in bin 2, 10 in bin 6, 5 in bin 9; the 8 robbed rows vote for bin 10, which only they make third."""
        import rot_plan as RP
        rng = np.random.default_rng(4)
        bins = np.concatenate([rng.permutation([2] * 15 + [6] * 10 + [9] * 5), [10] * len(self.stale_pairs)])
        return RP.plant(np.concatenate([self.final_pairs, self.stale_pairs]), self.n_a, self.n_b, bins, rng)


# ---- planting a case into a scene ------------------------------------------------------------------------------------
def base(scene):
    """(pairs, count, output) of the scene with the check off; the angles do not enter, so this is computed once."""
    if not hasattr(scene, "_base"):
        r = scene.unchecked()
        scene._base = (scene.pairs(), r[0], r[1])
    return scene._base


def plan(scene, case, seed=0):
    """Angles for `case` over the scene's pairs, and what rot_plan's statement of the rule expects the matcher to return."""
    import zlib
    import rot_plan as RP
    pairs, n0, out0 = base(scene)
    rng = np.random.default_rng([seed, zlib.crc32(case.encode())])
    aa, ab = RP.plant_case(case, pairs, scene.n_a, scene.n_b, rng)
    keep = RP.keep_mask(aa, ab, pairs)
    return {"aa": aa, "ab": ab, "pairs": pairs, "keep": keep, "removed": int((~keep).sum()), "count_off": n0, "out_off": out0}


def same(r, e):
    return r[0] == e[0] and all(np.array_equal(x, y) for x, y in zip(r[1:], e[1:]))
