"""Self-checks of tests/pose_model.py, the float64 restatement of Optimizer::PoseOptimization that the device entry
points are compared with (g2o boundary unpinned): nothing in it rests on a recalled sign or constant that is not checked
here against the model's own error function or against a scene with a known answer."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import pose_model as M  # noqa: E402

K = tuple(np.float64(k) for k in M.CAMERA)


def _edges(seed, stereo):
    rng = np.random.default_rng(seed)
    n = 12
    Xw = rng.uniform(-1, 1, (n, 3)) + np.array([0, 0, 3.0])
    obs = np.stack([rng.uniform(50, 600, n), rng.uniform(50, 400, n), rng.uniform(30, 500, n)], 1)
    q, t = M.pose_from_Tcw(M.pose_matrix(M.quat_normalize(np.r_[rng.normal(0, 0.1, 3), 1.0]), rng.normal(0, 0.2, 3)))
    return Xw, obs, np.full(n, stereo), q, t


def _jacobian_vs_central_differences(stereo):
    Xw, obs, st, q, t = _edges(3 + int(stereo), stereo)
    e0, P = M.errors(q, t, Xw, obs, st, K)
    J = M.jacobian(P, st, K)
    h = 1e-6
    worst = 0.0
    for a in range(6):
        d = np.zeros(6)
        d[a] = h
        ep, _ = M.errors(*M.pose_update(q, t, d), Xw, obs, st, K)
        em, _ = M.errors(*M.pose_update(q, t, -d), Xw, obs, st, K)
        fd = (ep - em) / (2 * h)
        scale = np.abs(J).max()
        worst = max(worst, float(np.abs(fd - J[:, :, a]).max() / scale))
    return worst


def test_jacobian_mono_matches_central_differences():
    assert _jacobian_vs_central_differences(False) < 1e-6


def test_jacobian_stereo_matches_central_differences():
    assert _jacobian_vs_central_differences(True) < 1e-6


def test_exp_is_continuous_across_the_small_angle_branch():
    """g2o's branch for theta < 1e-5 sets R = I + W + W^2 and V = R (kept as is).  R meets Rodrigues at theta = 1e-5 to
    5e-11.  V does not meet the series I + W/2 + W^2/6: the translation jumps by (W/2 + 5 W^2/6) v, about theta |v| / 2.
    An LM step whose rotation is 1e-5 rad has a translation of the order of rotation x scene depth (<= 6 m here), so the
    check uses |v| = 6e-5, where the jump is 3e-10; the jump itself is asserted to be exactly g2o's, at any |v|."""
    for axis in (np.array([1.0, 0, 0]), np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])):
        v = np.array([0.2, -0.1, 0.3])
        v = v / np.linalg.norm(v) * 6e-5
        Ra, ta = M.se3_exp(np.r_[axis * (1e-5 * (1 - 1e-9)), v])  # g2o's small-angle branch
        Rb, tb = M.se3_exp(np.r_[axis * (1e-5 * (1 + 1e-9)), v])  # Rodrigues
        assert np.abs(Ra - Rb).max() < 1e-9 and np.abs(ta - tb).max() < 1e-9
        big = np.array([0.2, -0.1, 0.3])
        W = M.skew(axis * 1e-5)
        _, ta = M.se3_exp(np.r_[axis * (1e-5 * (1 - 1e-9)), big])
        _, tb = M.se3_exp(np.r_[axis * (1e-5 * (1 + 1e-9)), big])
        assert np.abs((ta - tb) - (W / 2 + 5 * (W @ W) / 6) @ big).max() < 1e-12


def test_exp_is_a_rotation_and_quaternions_round_trip():
    R, _ = M.se3_exp(np.array([0.4, -0.7, 0.2, 0, 0, 0]))
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(R) - 1) < 1e-14
    for m in (R, np.diag([1.0, -1.0, -1.0]), np.diag([-1.0, 1.0, -1.0]), np.diag([-1.0, -1.0, 1.0])):
        q = M.quat_normalize(M.quat_from_matrix(m))
        assert np.abs(M.quat_to_matrix(q) - m).max() < 1e-14


def test_cholesky_solves_and_refuses():
    rng = np.random.default_rng(0)
    A = rng.normal(0, 1, (6, 6))
    H = A @ A.T + np.eye(6)
    b = rng.normal(0, 1, 6)
    ok, x = M.cholesky_solve(H, 0.5, b)
    assert ok and np.abs((H + 0.5 * np.eye(6)) @ x - b).max() < 1e-12
    ok, x = M.cholesky_solve(-H, 0.0, b)
    assert not ok and not x.any()
    Hn = H.copy()
    Hn[2, 2] = np.nan
    ok, x = M.cholesky_solve(Hn, 0.0, b)
    assert not ok and not x.any()


def test_noise_free_scene_recovers_the_pose():
    sc = M.make_scene(300, 11, noise=0.0, outlier_frac=0.0)
    # the generator rounds observations and points to float32: recompute exact observations of the float32 points
    T = sc["Tcw_true"]
    X = sc["world_pos"][sc["kp_to_mp"].clip(0)].astype(np.float64)
    Pc = X @ T[:3, :3].T + T[:3, 3]
    fx, fy, cx, cy, bf = K
    u = fx * Pc[:, 0] / Pc[:, 2] + cx
    r = M.pose_optimization(np.stack([u, fy * Pc[:, 1] / Pc[:, 2] + cy], 1), sc["octave"],
                            np.where(sc["u_right"] < 0, -1.0, u - bf / Pc[:, 2]), sc["kp_to_mp"], sc["world_pos"], sc["Tcw"],
                            sc["inv_level_sigma2"], sc["K"])
    # float32 observations: a pixel is known to 3e-5 at u ~ 600, i.e. ~1e-7 rad / ~1e-6 m at these depths over 240 edges
    assert np.abs(r["Tcw_d"] - T).max() < 1e-6, np.abs(r["Tcw_d"] - T).max()
    assert r["n_inliers"] == r["n_initial"] == int(sc["has"].sum()) and not (r["outlier"] == 1).any()
    assert r["rounds"] == 4


def test_planted_outliers_are_exactly_the_flagged_ones():
    for seed, mode in ((21, "mixed"), (22, "mono"), (23, "stereo")):
        sc = M.make_scene(400, seed, mode=mode, noise=0.3, outlier_frac=0.2, outlier_px=(30.0, 60.0))
        r = M.run_model(sc)
        assert sc["bad"].sum() > 40
        assert np.array_equal(r["outlier"] == 1, sc["bad"]), (seed, int(((r["outlier"] == 1) != sc["bad"]).sum()))
        assert np.all(r["outlier"][~sc["has"]] == 255)  # not an edge: untouched
        assert r["n_inliers"] == int(sc["has"].sum()) - int(sc["bad"].sum())


def test_fewer_than_three_edges_returns_zero_and_leaves_the_pose():
    sc = M.make_scene(40, 5)
    keep = np.flatnonzero(sc["kp_to_mp"] >= 0)[:2]
    k2m = np.full(40, -1, np.int32)
    k2m[keep] = sc["kp_to_mp"][keep]
    sc["kp_to_mp"] = k2m
    r = M.run_model(sc)
    assert r["n_initial"] == 2 and r["n_inliers"] == 0 and r["rounds"] == 0 and r["trials"] == 0
    assert np.array_equal(r["Tcw"], sc["Tcw"]) and np.array_equal(r["Tcw_d"], sc["Tcw"].astype(np.float64))
    assert np.all(r["outlier"][keep] == 0) and (r["outlier"] == 255).sum() == 38


def test_fewer_than_ten_edges_in_total_runs_exactly_one_round():
    for n, rounds in ((3, 1), (9, 1), (10, 4)):
        r = M.run_model(M.make_scene(n, 30 + n, assoc_frac=1.0, outlier_frac=0.0))
        assert r["n_initial"] == n and r["rounds"] == rounds, (n, r["rounds"])


def test_round_loop_counts_total_not_active_edges():
    """12 edges of which 5 are gross outliers: 7 stay active after round 0, the loop still runs all four rounds."""
    sc = M.make_scene(12, 77, assoc_frac=1.0, outlier_frac=0.0, noise=0.2)
    sc["kps_xy"][:5] += np.float32(80.0)
    r = M.run_model(sc)
    assert r["n_initial"] == 12 and r["rounds"] == 4 and np.all(r["outlier"][:5] == 1) and r["n_inliers"] == 7


def test_out_of_range_rows_and_octaves_are_skipped_and_counted():
    sc = M.make_scene(60, 9, assoc_frac=1.0)
    base = M.run_model(sc)
    sc2 = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in sc.items()}
    sc2["kp_to_mp"][3] = len(sc["world_pos"]) + 5
    sc2["octave"][7] = M.NLEVELS
    sc2["octave"][8] = -1
    r = M.run_model(sc2)
    assert r["n_bad_index"] == 3 and r["n_initial"] == base["n_initial"] - 3
    assert np.all(r["outlier"][[3, 7, 8]] == 255)


def test_non_finite_points_follow_ieee():
    sc = M.make_scene(80, 13, assoc_frac=1.0)
    sc["world_pos"][sc["kp_to_mp"][4]] = np.nan
    r = M.run_model(sc)  # NaN chi2: every trial is rejected (one per iteration), NaN > threshold is false
    assert r["n_initial"] == 80 and r["rounds"] == 4 and r["trials"] == 40 and r["iterations"] == 40
    assert r["outlier"][4] == 0 and np.abs(r["Tcw_d"] - sc["Tcw"].astype(np.float64)).max() < 1e-6  # the pose never moved
    sc = M.make_scene(80, 14, assoc_frac=1.0)
    T = sc["Tcw_true"]
    behind = (np.array([0.1, 0.1, -2.0]) - T[:3, 3]) @ T[:3, :3]
    sc["world_pos"][sc["kp_to_mp"][4]] = behind.astype(np.float32)
    r = M.run_model(sc)
    assert r["outlier"][4] == 1 and np.isfinite(r["Tcw_d"]).all() and np.abs(r["Tcw_d"] - T).max() < 0.05


def test_summation_order_moves_the_pose_only_at_rounding_level():
    worst = 0.0
    for seed in range(6):
        sc = M.make_scene([40, 150, 400][seed % 3], 100 + seed)
        base = M.run_model(sc)
        assert base["margin"] >= 1e-6
        dev, flips = M.permutation_spread(sc, base, n_perm=4, seed=seed)
        worst = max(worst, dev)
        assert flips == 0
    assert worst < 1e-6, worst
