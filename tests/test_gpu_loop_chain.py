"""Steps two to five of LoopClosing::ComputeSim3 (LoopClosing.cc:300-357) chained through the library on a synthetic
key-frame pair with a planted Sim3: orbgpu_sim3_solve -> orbgpu_search_by_sim3 -> orbgpu_sim3_optimize (th2 = 10) ->
orbgpu_search_by_projection_sim3 with the Scw the optimiser returns.  What only this test shows: the orientation
conventions of the four entry points agree (x1 = s12 R12 x2 + t12; Scw = S12 Smw maps key frame 2's world into camera 1)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import scenario  # noqa: E402
from test_gpu_matcher_m6 import _two_keyframes  # noqa: E402

pytestmark = pytest.mark.gpu


def test_solver_to_search_by_sim3_to_optimizer_to_projection(gpu, oracle):
    """The scene of test_gpu_sim3_chain.py with a planted Sim3 that the KEY POINTS agree with: the stream is a pure image
    shift, so map points at one depth d in camera 2 and x1 = x2 + t with t = d shift / f put every point of key frame 2
    exactly on its own image content in key frame 1 (a rotation or a t_z, as that test plants them for the matchers'
    windows, would contradict the observations the optimiser fits).  The scale is fixed, as LoopClosing fixes it for an
    RGB-D sensor: with all points at one depth and t_z = 0 a reprojection error does not see the scale at all.  Every key
    point of both frames holds such a map point."""
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

    d, s12 = 3.0, 1.0
    R12 = np.eye(3)
    t12 = np.array([s12 * d * shift[0] / fx, s12 * d * shift[1] / fy, 0.0])

    def back(k, dx, dy):
        return np.stack([(k["x"].astype(np.float64) - dx - cx) * d / fx, (k["y"].astype(np.float64) - dy - cy) * d / fy,
                         np.full(len(k), d)], 1)
    x2_of2 = back(ks[1], 0.0, 0.0)
    x2_of1 = back(ks[0], shift[0], shift[1])
    x1_of1 = s12 * x2_of1 @ R12.T + t12
    x1_of2 = s12 * x2_of2 @ R12.T + t12
    T1w, T2w = scenario.rigid(0.02, -0.01, 0.03, (0.1, -0.05, 0.2)), scenario.rigid()
    A, B = T1w.astype(np.float64), T2w.astype(np.float64)
    P1 = ((x1_of1 - A[:3, 3]) @ A[:3, :3]).astype(np.float32)
    P2 = ((x2_of2 - B[:3, 3]) @ B[:3, :3]).astype(np.float32)

    valid = (m12 >= 0).astype(np.uint8)
    j = m12.clip(0)
    N = int(valid.sum())
    tri = np.stack([rng.choice(N, 3, replace=False) for _ in range(300)]).astype(np.int32)
    sig2 = (sf * sf).astype(np.float32)
    K = (fx, fy, cx, cy)
    r = gpu.sim3_solve(valid, P1, P2[j], ks[0]["octave"], ks[1]["octave"][j], T1w, T2w, K, K, sig2, tri, fix_scale=True,
                       probability=0.99, min_inliers=20, max_iterations=300)
    assert r["accepted"] >= 0 and r["n_inliers"] > 20

    def pts(P, dist, octv, desc, normal=None):
        max_d = (dist * sf[octv] * 0.9995).astype(np.float32)
        n = len(P)
        return {"bad": np.zeros(n, np.uint8), "world_pos": P, "normal": np.zeros((n, 3), np.float32) if normal is None else normal,
                "min_dist": (max_d / sf[-1]).astype(np.float32), "max_dist": max_d, "desc": desc}
    oct1_seen = np.where(m12 >= 0, ks[1]["octave"][j], ks[0]["octave"])
    back12 = np.full(len(ks[1]), -1)
    back12[m12[m12 >= 0]] = np.flatnonzero(m12 >= 0)
    oct2_seen = np.where(back12 >= 0, ks[0]["octave"][back12.clip(0)], ks[1]["octave"])
    pts1 = pts(P1, np.linalg.norm(x2_of1, axis=1), oct1_seen, ds[0])
    pts2 = pts(P2, np.linalg.norm(x1_of2, axis=1), oct2_seen, ds[1])
    n_found, found = gpu.search_by_sim3(g[0], g[1], T1w, T2w, float(r["s"]), r["R"], r["t"], fx, fy, cx, cy, log_sf, log_sf,
                                        pts1, None, pts2, None, 7.5)
    assert n_found >= r["n_inliers"]

    # vpMapPointMatches as ComputeSim3 holds them at :326: the solver's inliers and what SearchBySim3 found
    match = np.where(found >= 0, found, np.where(r["inliers"] != 0, m12, -1))
    vm = (match >= 0).astype(np.uint8)
    jm = match.clip(0)
    kp1 = np.stack([ks[0]["x"], ks[0]["y"]], 1).astype(np.float32)
    kp2 = np.stack([ks[1]["x"], ks[1]["y"]], 1).astype(np.float32)[jm]
    inv_sig2 = (np.float32(1.0) / sig2).astype(np.float32)
    n_in, inl, res = gpu.sim3_optimize(vm, P1, P2[jm], ks[0]["octave"], ks[1]["octave"][jm], kp1, kp2, T1w, T2w, K, K, inv_sig2,
                                       r["R"], r["t"], r["s"], th2=10.0, fix_scale=True)

    def off(s, R, t):
        return max(abs(float(s) - s12), float(np.abs(np.asarray(R, np.float64) - R12).max()),
                   float(np.abs(np.asarray(t, np.float64) - t12).max()))
    print("loop chain: %d matches in, %d inliers (stage-1 bad %d), off the planted Sim3: solver %.2e, refined %.2e" % (
        int(vm.sum()), n_in, res["n_bad"], off(r["s"], r["R"], r["t"]), off(res["s12_d"], res["R12_d"], res["t12_d"])))
    assert res["n_correspondences"] == int(vm.sum()) and res["stages"] == 2 and res["s12_d"] == 1.0 == r["s"]
    assert n_in >= 20 and n_in == int((inl[vm != 0] != 0).sum())  # LoopClosing.cc:330
    assert off(res["s12_d"], res["R12_d"], res["t12_d"]) <= off(r["s"], r["R"], r["t"])

    # SearchByProjection(mpCurrentKF, mScw, vpLoopMapPoints, ...) (:357): key frame 2's map points, in its world, seen from
    # camera 1 through Scw; distances are measured in that world, normals point from camera 2's centre
    Scw = res["Scw"]
    O2 = -B[:3, :3].T @ B[:3, 3]
    normal = P2.astype(np.float64) - O2
    normal /= np.linalg.norm(normal, axis=1)[:, None]
    loop_pts = pts(P2, np.linalg.norm(x1_of2, axis=1) / s12, oct2_seen, ds[1], normal.astype(np.float32))
    none = np.full(g[0].n, -1, np.int32)
    n_proj, kp_to_mp = gpu.search_by_projection_sim3(g[0], Scw, fx, fy, cx, cy, log_sf, loop_pts, 10, none)
    print("loop chain: SearchByProjection with Scw found %d, optimiser inliers %d" % (n_proj, n_in))
    assert n_proj >= n_in
    # Scw must be S12 * Smw: the same product in matrix form, to float resolution
    want = np.eye(4)
    want[:3, :3], want[:3, 3] = res["s12_d"] * res["R12_d"], res["t12_d"]
    assert np.abs(Scw - want @ B).max() < 1e-5
    # the inverse orientation does worse: fewer matches, or the matcher refuses it because a point's predicted level leaves
    # the pyramid (ORBGPU_ELEVEL)
    S21 = np.linalg.inv(want)
    try:
        n_wrong, _ = gpu.search_by_projection_sim3(g[0], (S21 @ B).astype(np.float32), fx, fy, cx, cy, log_sf, loop_pts, 10, none)
    except gpu.OrbGpuError as e:
        assert e.status == gpu.ELEVEL
        n_wrong = 0
    assert n_wrong < n_proj
