"""Steps two to four of Tracking::Relocalization (Tracking.cc:1681-1744) chained through the library on a synthetic
key frame / frame pair with a planted pose: orbgpu_search_by_bow -> orbgpu_pnp_solve -> orbgpu_pose_optimization.  What
only this test shows: the solver's Tcw has the orientation the optimiser takes (x_cam = Rcw x_world + tcw)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import pnp_model as M  # noqa: E402
import pose_model as PM  # noqa: E402
import scenario  # noqa: E402
from test_gpu_matcher_m6 import _two_keyframes  # noqa: E402

pytestmark = pytest.mark.gpu


def test_bow_matches_to_solver_to_pose_optimization(gpu, oracle):
    """The stream is a pure image shift: the content under key point p of the key frame lies at p - shift in the frame.
    Every key point of the key frame holds a map point placed, at a depth of its own (1-8 m), on the ray of p - shift of
    a camera with the planted pose.  The solver sees the BoW matches, wrong ones included."""
    st, ge, fr, ks, ds, g, o, shift = _two_keyframes(gpu, oracle)
    rng = np.random.default_rng(11)
    sf = np.asarray(ge.GetScaleFactors(), np.float32)
    fx, fy, cx, cy = (float(v) for v in (st.fx, st.fy, st.cx, st.cy))
    v = scenario.synthetic_vocabulary(10, 4, 8)
    gv = gpu.ORBVocabulary(10, 4, v["parent"], v["is_leaf"], v["desc"], v["weight"])
    nd = [gv.transform(d, 2)["node_id"] for d in ds]
    gv.close()
    n_bow, match_f = gpu.search_by_bow(ds[0], ks[0]["angle"], None, nd[0], ds[1], ks[1]["angle"], nd[1], nnratio=0.75)
    assert n_bow >= 15, n_bow                                   # Tracking.cc:1682

    Tp = scenario.rigid(0.3, -0.2, 0.5, (1.0, -0.5, 1.5)).astype(np.float64)
    z = rng.uniform(1.0, 8.0, len(ks[0]))
    Xc = np.stack([(ks[0]["x"].astype(np.float64) - shift[0] - cx) * z / fx, (ks[0]["y"].astype(np.float64) - shift[1] - cy) * z / fy, z], 1)
    Xw_kf = ((Xc - Tp[:3, 3]) @ Tp[:3, :3]).astype(np.float32)  # world = Rcw' (x - tcw)

    n1 = len(ks[1])
    valid = (match_f >= 0).astype(np.uint8)
    Xw = Xw_kf[match_f.clip(0)]
    N = int(valid.sum())
    sets = np.stack([rng.choice(N, 4, replace=False) for _ in range(300)]).astype(np.int32)
    sig2 = (sf * sf).astype(np.float32)
    sc = {"valid": valid, "Xw": Xw, "kp": np.stack([ks[1]["x"], ks[1]["y"]], 1).astype(np.float32), "octave": ks[1]["octave"],
          "K": (fx, fy, cx, cy), "level_sigma2": sig2, "probability": 0.99, "min_inliers": 10, "max_iterations": 300, "min_set": 4,
          "epsilon": 0.5, "th2": 5.991, "sets": sets}
    r = gpu.pnp_solve(sc)
    print("chain: %d BoW matches, N %d, nMinInliers %d, max_its %d, accepted iteration %d with %d inliers" % (
        n_bow, r["n"], r["min_inliers"], r["max_its"], r["accepted"], r["n_inliers"]))
    assert r["n"] == N == n_bow and r["accepted"] >= 0 and r["n_inliers"] > r["min_inliers"]
    assert r["inliers"].sum() == r["n_inliers"] and not r["inliers"][valid == 0].any()
    # the model on the same matches: the discrete results
    m = M.solve(sc)
    for k in ("accepted", "n_inliers", "best_inliers", "best_iteration", "iterations", "min_inliers", "max_its"):
        assert r[k] == int(m[k]), k
    assert np.array_equal(r["counts"], m["counts"])
    i = np.arange(n1)
    assert np.array_equal(r["inliers"], ((m["refined_mask"][i // 64] >> (i % 64).astype(np.uint64)) & np.uint64(1)).astype(np.uint8))
    assert np.abs(r["Tcw"][:3, :3] - Tp[:3, :3]).max() < 0.01 and np.abs(r["Tcw"][:3, 3] - Tp[:3, 3]).max() < 0.05

    # Optimizer::PoseOptimization from the returned pose over the returned inliers (Tracking.cc:1727-1744)
    f = gpu.Frame(ks[1]["x"], ks[1]["y"], ks[1]["octave"], ks[1]["angle"], np.full(n1, -1, np.float32), ds[1], 640, 480, sf)
    inv_sig2 = (np.float32(1.0) / sig2).astype(np.float32)
    n_good, T, outlier, res = gpu.pose_optimization(f, r["inliers"], Xw, r["Tcw"], inv_sig2, fx, fy, cx, cy, 40.0)
    pm = PM.pose_optimization(sc["kp"], ks[1]["octave"], np.full(n1, -1, np.float32), np.where(r["inliers"] != 0, i, -1), Xw, r["Tcw"],
                              inv_sig2, (fx, fy, cx, cy, 40.0))
    print("chain: PoseOptimization keeps %d of %d (model %d)" % (n_good, r["n_inliers"], pm["n_inliers"]))
    assert n_good == pm["n_inliers"] and n_good >= 0.8 * r["n_inliers"]
    assert np.abs(T[:3, :3] - Tp[:3, :3]).max() < 0.01 and np.abs(T[:3, 3] - Tp[:3, 3]).max() < 0.05
    # the other orientation (Twc in the place of Tcw) does worse
    Twc = np.linalg.inv(r["Tcw"].astype(np.float64)).astype(np.float32)
    n_wrong = gpu.pose_optimization(f, r["inliers"], Xw, Twc, inv_sig2, fx, fy, cx, cy, 40.0)[0]
    assert n_wrong < n_good
