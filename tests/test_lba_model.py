"""tests/lba_model.py, the float64 restatement of Optimizer::LocalBundleAdjustment, against itself: it converges where the
answer is known, finds the planted outliers and only them, applies the depth test, and its analytic Jacobians are the
derivatives of its own error."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import lba_model as L  # noqa: E402
import pose_model as M  # noqa: E402


@pytest.mark.parametrize("mode", ["mono", "stereo", "mixed"])
def test_noise_free_scene_returns_to_truth(mode):
    # mono scenes need two fixed cameras to pin the scale
    sc = L.make_scene(3, 2, 40, 11, mode=mode, noise=0.0, outlier_frac=0.0)
    r = L.local_ba(sc)
    assert r["rounds"] == 2 and r["stopped"] == 0 and r["n_erased"] == 0 and r["n_bad_index"] == 0
    assert r["n_edges"] == len(sc["e_point"]) and not r["erase"].any()
    assert r["chi2_start"][0] > 100.0 and r["chi2_end"][1] < 1e-3  # key points are rounded to float: not exactly 0
    start_T = np.abs(sc["Tcw"].astype(np.float64) - sc["Tcw_true"]).max()
    start_X = np.abs(sc["world_pos"].astype(np.float64) - sc["pos_true"]).max()
    assert start_T > 1e-3 and start_X > 1e-2
    assert np.abs(r["Tcw_d"] - sc["Tcw_true"][:sc["n_local"]]).max() < 1e-4
    # chi2 < 1e-3 leaves residuals of up to 0.03 px; two cameras 0.25 m apart turn a pixel into z^2 / (f b) = 0.37 m of
    # depth at 7 m
    assert np.abs(r["pos_d"] - sc["pos_true"]).max() < 0.03 * 0.37 < start_X / 3
    assert np.array_equal(r["Tcw"], r["Tcw_d"].astype(np.float32)) and np.array_equal(r["pos"], r["pos_d"].astype(np.float32))


@pytest.mark.parametrize("mode", ["mono", "stereo", "mixed"])
def test_planted_gross_outliers_and_only_they_are_erased(mode):
    sc = L.make_scene(4, 2, 60, 12, mode=mode, noise=0.1, outlier_frac=0.08, obs_frac=1.0)  # every point seen six times
    assert 5 <= sc["bad"].sum() < 0.2 * len(sc["bad"])
    r = L.local_ba(sc)
    assert np.array_equal(r["erase"].astype(bool), sc["bad"]) and r["n_erased"] == int(sc["bad"].sum())
    assert r["chi2_end"][1] < r["chi2_end"][0] < r["chi2_start"][0]  # round 2 runs on the level-0 edges only
    assert np.abs(r["Tcw_d"] - sc["Tcw_true"][:sc["n_local"]]).max() < 5e-3


def test_a_point_behind_a_camera_is_erased_by_the_depth_test_alone():
    """One observation whose point lies behind its (fixed) camera at an image position that reprojects exactly: chi2 is
    tiny, depth is negative."""
    sc = L.make_scene(2, 2, 20, 13, mode="mono", noise=0.0, outlier_frac=0.0, rot_sigma=0.0, trans_sigma=0.0, point_sigma=0.0)
    fixed_pose = sc["n_local"]  # the first fixed camera
    T = sc["Tcw_true"][fixed_pose]
    Xc = np.array([0.3, -0.2, -4.0])
    Xw = (Xc - T[:3, 3]) @ T[:3, :3]
    sc["world_pos"] = np.vstack([sc["world_pos"], Xw.astype(np.float32)])
    p = len(sc["world_pos"]) - 1
    cam = sc["cam"][fixed_pose].astype(np.float64)
    Xc = T[:3, :3] @ sc["world_pos"][p].astype(np.float64) + T[:3, 3]
    uv = np.array([cam[0] * Xc[0] / Xc[2] + cam[2], cam[1] * Xc[1] / Xc[2] + cam[3]])
    # a second fixed camera sees it in front, so that the point itself is well determined by fixed cameras only
    for pose in (fixed_pose,):
        sc["e_point"] = np.r_[sc["e_point"], p].astype(np.int32)
        sc["e_pose"] = np.r_[sc["e_pose"], pose].astype(np.int32)
        sc["e_oct"] = np.r_[sc["e_oct"], 0].astype(np.int32)
        sc["e_xy"] = np.vstack([sc["e_xy"], uv.astype(np.float32)])
        sc["e_ur"] = np.r_[sc["e_ur"], -1.0].astype(np.float32)
    r = L.local_ba(sc)
    assert r["erase"][-1] == 1 and r["n_erased"] == 1 and not r["erase"][:-1].any()
    # its chi2 at the final state is far below the threshold: the depth test alone erased it
    q, t = M.pose_from_Tcw(sc["Tcw"][fixed_pose])
    Pc = M.quat_to_matrix(q) @ r["pos_d"][p] + t
    e = uv.astype(np.float32).astype(np.float64) - np.array([cam[0] * Pc[0] / Pc[2] + cam[2], cam[1] * Pc[1] / Pc[2] + cam[3]])
    assert Pc[2] < 0 and float(e @ e) < 1e-3


@pytest.mark.parametrize("mode", ["mono", "stereo"])
def test_analytic_jacobians_are_the_derivatives_of_the_error(mode):
    sc = L.make_scene(2, 1, 12, 14, mode=mode)
    Tcw = sc["Tcw"].astype(np.float64)
    P = len(Tcw)
    qs, ts = zip(*[M.pose_from_Tcw(sc["Tcw"][i]) for i in range(P)])
    qs, ts = np.array(qs), np.array(ts)
    X = sc["world_pos"].astype(np.float64)
    cam = sc["cam"].astype(np.float64)
    ed = {"point": sc["e_point"].astype(np.int64), "pose": sc["e_pose"].astype(np.int64), "stereo": ~(sc["e_ur"] < 0),
          "obs": np.c_[sc["e_xy"].astype(np.float64), sc["e_ur"].astype(np.float64)]}
    ed["K"] = tuple(cam[ed["pose"], k] for k in range(5))

    def err(qs_, ts_, X_):
        return L.edge_errors(np.array([M.quat_to_matrix(q) for q in qs_]), ts_, X_, ed)
    e0, Pc = err(qs, ts, X)
    Rp = np.array([M.quat_to_matrix(q) for q in qs])
    Jc = M.jacobian(Pc, ed["stereo"], ed["K"])
    Jp = L.point_jacobian(Pc, Rp[ed["pose"]], ed["stereo"], ed["K"])
    rows = 3 if mode == "stereo" else 2
    assert (ed["stereo"].all() if mode == "stereo" else not ed["stereo"].any())
    h = 1e-6
    for a in range(6):  # central differences of e under exp(h e_a) * T, every pose at once
        d = np.zeros(6)
        d[a] = h
        plus = [M.pose_update(q, t, d) for q, t in zip(qs, ts)]
        minus = [M.pose_update(q, t, -d) for q, t in zip(qs, ts)]
        ep, _ = err(np.array([p[0] for p in plus]), np.array([p[1] for p in plus]), X)
        em, _ = err(np.array([p[0] for p in minus]), np.array([p[1] for p in minus]), X)
        num = (ep - em) / (2 * h)
        scale = np.abs(Jc[:, :rows, :]).max()
        assert np.abs(num[:, :rows] - Jc[:, :rows, a]).max() <= 1e-6 * scale, a
    for c in range(3):
        d = np.zeros(3)
        d[c] = h
        ep, _ = err(qs, ts, X + d)
        em, _ = err(qs, ts, X - d)
        num = (ep - em) / (2 * h)
        scale = np.abs(Jp[:, :rows, :]).max()
        assert np.abs(num[:, :rows] - Jp[:, :rows, c]).max() <= 1e-6 * scale, c
    assert not Jc[~ed["stereo"], 2].any() and not Jp[~ed["stereo"], 2].any() and not e0[~ed["stereo"], 2].any()


def test_stop_flag_conventions():
    sc = L.make_scene(3, 2, 40, 15)
    r = L.local_ba(sc, stop_before=True)
    assert r["stopped"] == 1 and r["rounds"] == 0 and "Tcw_d" not in r and (r["erase"] == 255).all()
    full = L.local_ba(sc)
    half = L.local_ba(sc, stop_between=True)
    assert half["stopped"] == 1 and half["rounds"] == 1 and half["iterations"] == [full["iterations"][0], 0]
    assert half["chi2_end"][0] == full["chi2_end"][0] and half["n_erased"] >= full["n_erased"] > 0  # the final test still runs


def test_vertices_without_a_level0_edge_keep_their_round1_estimate():
    """Every observation of one point, and every observation made by one free pose, is a gross outlier: round 1 puts
    them all on level 1, round 2 runs without the vertex, whose estimate stays what round 1 left."""
    for which in ("point", "pose"):
        sc = L.make_scene(3, 2, 40, 16, mode="stereo", outlier_frac=0.0, noise=0.2)
        hit = sc["e_point"] == 5 if which == "point" else sc["e_pose"] == 1
        sc["e_xy"][hit] += np.float32(80.0) * np.where(np.arange(hit.sum())[:, None] % 2 == 0, 1, -1).astype(np.float32)
        one = L.local_ba(sc, stop_between=True)
        two = L.local_ba(sc)
        assert two["rounds"] == 2 and two["erase"][hit].all() and one["erase"][hit].all()
        if which == "point":
            assert np.array_equal(two["pos_d"][5], one["pos_d"][5]) and not np.array_equal(two["pos_d"][6], one["pos_d"][6])
        else:
            assert np.array_equal(two["Tcw_d"][1], one["Tcw_d"][1]) and not np.array_equal(two["Tcw_d"][0], one["Tcw_d"][0])


def test_out_of_range_rows_are_counted_and_all_fixed_is_points_only():
    sc = L.make_scene(2, 2, 20, 17)
    sc["e_point"][3] = 20
    sc["e_pose"][5] = -1
    sc["e_oct"][7] = M.NLEVELS
    r = L.local_ba(sc)
    assert r["n_bad_index"] == 3 and r["n_edges"] == len(sc["e_point"]) - 3 and (r["erase"][[3, 5, 7]] == 255).all()
    sc = L.make_scene(2, 2, 20, 18, noise=0.0, outlier_frac=0.0, rot_sigma=0.0, trans_sigma=0.0)
    sc["fixed"][:] = 1
    r = L.local_ba(sc)
    assert r["rounds"] == 2 and r["chi2_end"][1] < r["chi2_start"][0]
    for i in range(sc["n_local"]):  # untouched but for the quaternion round trip
        q, t = M.pose_from_Tcw(sc["Tcw"][i])
        assert np.array_equal(r["Tcw_d"][i], M.pose_matrix(q, t))
    assert np.abs(r["pos_d"] - sc["pos_true"]).max() < np.abs(sc["world_pos"] - sc["pos_true"]).max()


def test_the_device_tests_small_scenes_are_stable_under_permuted_summation():
    """tests/test_gpu_lba.py compares a scene only when the model's margin and accept / reject trace survive permuted
    summation orders, and may leave out one scene in eight: its seeds are fixed so that the model alone stays within
    that.  Checked here on the three small shapes (the two large ones take the model tens of seconds)."""
    import test_gpu_lba as T
    left_out = 0
    for k in range(3):
        for sc in T.shape_scenes(k):
            m = L.local_ba(sc)
            _, _, same, margin = L.permutation_spread(sc, m, n_perm=T.SHAPES[k][4], seed=len(sc["e_point"]))
            left_out += not (same and margin >= 1e-6)
    assert left_out <= (len(T.SHAPES) * len(T.MODES)) // 8
