"""The first three steps of LoopClosing::ComputeSim3 (LoopClosing.cc:266-324) chained through the library on a synthetic
key-frame pair with a planted Sim3: orbgpu_search_by_bow_keyframes -> orbgpu_sim3_solve -> orbgpu_search_by_sim3.  What
only this test shows: the solver's R12 / t12 / s12 have the orientation the matcher takes (x1 = s12 R12 x2 + t12)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import scenario  # noqa: E402
import sim3_model as M  # noqa: E402
from test_gpu_matcher_m6 import _two_keyframes  # noqa: E402

pytestmark = pytest.mark.gpu


def test_bow_matches_to_solver_to_search_by_sim3(gpu, oracle):
    """The stream is a pure image shift, so map points at one depth d in camera 2 and the similarity x1 = s x2 + t with
    t = s d shift / f (and a small rotation about the optical axis, 2 px at the image border) put every point of key
    frame 2 on its own image content in key frame 1.  Every key point of both frames holds such a map point; the solver
    sees the BoW matches, wrong ones included."""
    st, ge, fr, ks, ds, g, o, shift = _two_keyframes(gpu, oracle)
    rng = np.random.default_rng(5)
    sf = np.asarray(ge.GetScaleFactors(), np.float32)
    log_sf = float(np.log(np.float32(sf[1])))
    fx, fy, cx, cy = (float(v) for v in (st.fx, st.fy, st.cx, st.cy))
    v = scenario.synthetic_vocabulary(10, 4, 8)
    gv = gpu.ORBVocabulary(10, 4, v["parent"], v["is_leaf"], v["desc"], v["weight"])
    nd = [gv.transform(d, 2)["node_id"] for d in ds]
    gv.close()
    n_bow, m12 = gpu.search_by_bow_keyframes(ds[0], ks[0]["angle"], None, nd[0], ds[1], ks[1]["angle"], None, nd[1], 0.75, True)
    assert n_bow > 100, n_bow

    # the planted similarity and the two point sets, in camera coordinates
    d, s12 = 3.0, 1.2
    R12 = scenario.rigid(0.0, 0.0, 0.006, (0, 0, 0)).astype(np.float64)[:3, :3]
    t12 = np.array([s12 * d * shift[0] / fx, s12 * d * shift[1] / fy, 0.02])

    def back(k, dx, dy):
        return np.stack([(k["x"].astype(np.float64) - dx - cx) * d / fx, (k["y"].astype(np.float64) - dy - cy) * d / fy,
                         np.full(len(k), d)], 1)
    x2_of2 = back(ks[1], 0.0, 0.0)                               # key frame 2's points, on their own key points
    x2_of1 = back(ks[0], shift[0], shift[1])                     # where key frame 1's points are seen from camera 2
    x1_of1 = s12 * x2_of1 @ R12.T + t12
    x1_of2 = s12 * x2_of2 @ R12.T + t12
    T1w, T2w = scenario.rigid(0.02, -0.01, 0.03, (0.1, -0.05, 0.2)), scenario.rigid()
    A, B = T1w.astype(np.float64), T2w.astype(np.float64)
    P1 = ((x1_of1 - A[:3, 3]) @ A[:3, :3]).astype(np.float32)   # world = Rcw^T (x - tcw)
    P2 = ((x2_of2 - B[:3, 3]) @ B[:3, :3]).astype(np.float32)

    valid = (m12 >= 0).astype(np.uint8)
    j = m12.clip(0)
    N = int(valid.sum())
    tri = np.stack([rng.choice(N, 3, replace=False) for _ in range(300)]).astype(np.int32)
    sig2 = (sf * sf).astype(np.float32)
    K = (fx, fy, cx, cy)
    r = gpu.sim3_solve(valid, P1, P2[j], ks[0]["octave"], ks[1]["octave"][j], T1w, T2w, K, K, sig2, tri, fix_scale=False,
                       probability=0.99, min_inliers=20, max_iterations=300)
    print("chain: %d BoW matches, N %d, accepted iteration %d with %d inliers, s %.4f" % (n_bow, r["n"], r["accepted"],
                                                                                          r["n_inliers"], r["s"]))
    assert r["n"] == N == n_bow and r["accepted"] >= 0 and r["n_inliers"] > 20
    assert r["inliers"].sum() == r["n_inliers"] and not r["inliers"][valid == 0].any()
    # the model on the same inputs
    m = M.solve({"valid": valid, "Xw1": P1, "Xw2": P2[j], "octave1": ks[0]["octave"], "octave2": ks[1]["octave"][j], "T1w": T1w,
                 "T2w": T2w, "K1": K, "K2": K, "level_sigma2": sig2, "fix_scale": False, "probability": 0.99, "min_inliers": 20,
                 "max_iterations": 300, "triples": tri})
    assert m["accepted"] == r["accepted"] and m["n_inliers"] == r["n_inliers"]
    assert abs(r["s"] - s12) < 0.02 and np.abs(r["R"] - R12).max() < 0.01 and np.abs(r["t"] - t12).max() < 0.05

    # SearchBySim3 with the solver's answer: every key point's map point, its scale range around the level it is seen at
    def pts(P, cam, octv, desc):
        max_d = (np.linalg.norm(cam, axis=1) * sf[octv] * 0.9995).astype(np.float32)
        n = len(P)
        return {"bad": np.zeros(n, np.uint8), "world_pos": P, "normal": np.zeros((n, 3), np.float32),
                "min_dist": (max_d / sf[-1]).astype(np.float32), "max_dist": max_d, "desc": desc}
    oct1_seen = np.where(m12 >= 0, ks[1]["octave"][j], ks[0]["octave"])          # key frame 1's point, seen in image 2
    back12 = np.full(len(ks[1]), -1)
    back12[m12[m12 >= 0]] = np.flatnonzero(m12 >= 0)
    oct2_seen = np.where(back12 >= 0, ks[0]["octave"][back12.clip(0)], ks[1]["octave"])
    pts1, pts2 = pts(P1, x2_of1, oct1_seen, ds[0]), pts(P2, x1_of2, oct2_seen, ds[1])
    n_found, found = gpu.search_by_sim3(g[0], g[1], T1w, T2w, float(r["s"]), r["R"], r["t"], fx, fy, cx, cy, log_sf, log_sf,
                                        pts1, None, pts2, None, 7.5)
    given = int(r["n_inliers"])
    print("chain: SearchBySim3 found %d, given %d inliers" % (n_found, given))
    assert n_found >= given
    # the other orientation (the inverse similarity's parts) does worse: fewer matches, or the matcher refuses it because a
    # point's predicted level leaves the pyramid (ORBGPU_ELEVEL, an out-of-range read in the reference)
    try:
        n_wrong, _ = gpu.search_by_sim3(g[0], g[1], T1w, T2w, float(1.0 / r["s"]), r["R"].T.copy(), (-r["t"]).copy(), fx, fy, cx,
                                        cy, log_sf, log_sf, pts1, None, pts2, None, 7.5)
    except gpu.OrbGpuError as e:
        assert e.status == gpu.ELEVEL
        n_wrong = 0
    assert n_wrong < n_found
