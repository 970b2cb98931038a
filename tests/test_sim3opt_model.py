"""The float64 restatement of Optimizer::OptimizeSim3 (sim3opt_model.py, conventions O1-O9 of include/orbgpu.h) on its
own: it recovers a planted Sim3, clears exactly the planted outliers, follows the two-stage rules, and every committed
parity scene is far enough from a classification threshold to be compared exactly with the device."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import sim3opt_model as M  # noqa: E402


def _exact_problem(n, seed, fix_scale):
    """Widened records whose observations are the exact double projections under the planted Sim3: zero residual there."""
    sc = M.make_scene(n, seed, fix_scale=fix_scale, outlier_frac=0.0, noise_px=0.0)
    pb = M.prepare(sc)
    tr = sc["true"]
    truth = (M.quat_normalize(M.quat_from_matrix(tr["R"])), np.array(tr["t"], np.float64), np.float64(tr["s"]))
    e12, e21 = M.pair_errors(truth, pb["X1"], pb["X2"], np.zeros_like(pb["obs1"]), np.zeros_like(pb["obs2"]), pb["K1"], pb["K2"])
    pb["obs1"], pb["obs2"] = -e12, -e21
    return sc, pb, truth


@pytest.mark.parametrize("fix_scale", [False, True])
def test_noise_free_scene_returns_the_planted_sim3(fix_scale):
    sc, pb, truth = _exact_problem(60, 11, fix_scale)
    r = M.optimize_core(pb, M.state_from_floats(sc["R12"], sc["t12"], sc["s12"]), sc["th2"], fix_scale)
    q, t, s = r["state"]
    assert r["stages"] == 2 and r["n_bad"] == 0 and r["n_inliers"] == 60
    dev = max(np.abs(M.quat_to_matrix(q) - M.quat_to_matrix(truth[0])).max(), np.abs(t - truth[1]).max(), abs(s - truth[2]))
    print("noise-free: deviation from the planted Sim3 %.3e after %d iterations" % (dev, r["iterations"]))
    assert dev < 1e-8, dev
    if fix_scale:
        assert s == 1.0


def test_planted_outliers_are_exactly_the_cleared_rows():
    # 10 % outliers: with 30 % of them 50-200 px off, the stage-1 optimum under the Huber kernel is itself pulled far enough
    # (a few pixels at the image border) for a true match to fail th2 there -- the algorithm's property, not the model's.
    for seed, fs in ((21, False), (22, True)):
        sc = M.make_scene(150, seed, fix_scale=fs, outlier_frac=0.1, noise_px=0.1)
        r = M.optimize_sim3(sc)
        cleared = r["inlier"] == 0
        assert np.array_equal(cleared, sc["outlier"]), (seed, int(cleared.sum()), int(sc["outlier"].sum()))
        assert np.all(r["inlier"][np.asarray(sc["valid"]) == 0] == 255)
        assert r["n_inliers"] == 150 - int(sc["outlier"].sum()) and r["stages"] == 2
        # every planted outlier is already gone after stage 1
        assert r["n_bad"] == int(sc["outlier"].sum())


def test_second_stage_budget_follows_nbad():
    clean = M.optimize_sim3(M.make_scene(80, 31, outlier_frac=0.0, noise_px=0.1))
    assert clean["n_bad"] == 0 and clean["stages"] == 2 and 5 < clean["iterations"] <= 10
    dirty = M.optimize_sim3(M.make_scene(80, 32, outlier_frac=0.3))
    assert dirty["n_bad"] > 0 and dirty["stages"] == 2 and dirty["iterations"] > 10  # more than 5 + 5: the budget was 10
    assert dirty["iterations"] <= 15 and dirty["trials"] <= 150


def test_fewer_than_ten_left_returns_zero_and_keeps_the_clearing():
    sc = M.make_scene(16, 4003, outlier_frac=0.6)
    r = M.optimize_sim3(sc)
    assert r["stages"] == 1 and r["n_inliers"] == 0 and r["n_correspondences"] - r["n_bad"] < 10
    q0, t0, s0 = M.state_from_floats(sc["R12"], sc["t12"], sc["s12"])
    assert np.array_equal(r["R12_d"], M.quat_to_matrix(q0)) and np.array_equal(r["t12_d"], t0) and r["s12_d"] == s0
    assert np.array_equal(r["t12"], np.asarray(sc["t12"], np.float32)) and r["s12"] == sc["s12"]
    assert int((r["inlier"] == 0).sum()) == r["n_bad"] > 0 and int((r["inlier"] == 1).sum()) == 16 - r["n_bad"]
    assert r["iterations"] <= 5


def test_no_correspondence_and_fixed_scale():
    sc = M.make_scene(30, 41)
    sc["valid"] = np.zeros_like(sc["valid"])
    r = M.optimize_sim3(sc)
    assert r["n_correspondences"] == r["n_inliers"] == r["stages"] == r["iterations"] == 0 and np.all(r["inlier"] == 255)
    sc = M.make_scene(120, 42, fix_scale=True)
    sc["s12"] = np.float32(1.25)  # whatever the caller's scale is, it stays bit for bit
    r = M.optimize_sim3(sc)
    assert r["stages"] == 2 and r["s12_d"] == np.float64(np.float32(1.25)) and r["s12"] == np.float32(1.25)
    J = M.numeric_jacobian(M.state_from_floats(sc["R12"], sc["t12"], sc["s12"]), M.prepare(sc), True)
    assert np.all(J[:, :, 6] == 0.0) and np.abs(J[:, :, :6]).max() > 1.0


def test_out_of_range_octaves_are_no_correspondences():
    sc = dict(M.PARITY_SCENES)["bad_octaves"]
    r = M.optimize_sim3(sc)
    assert r["n_bad_index"] == 3 and r["n_correspondences"] == 87
    v = np.flatnonzero(sc["valid"])
    assert np.all(r["inlier"][v[[3, 10, 20]]] == 255)


def test_numeric_jacobian_agrees_with_a_larger_step():
    sc = M.make_scene(50, 51)
    pb, st = M.prepare(sc), M.state_from_floats(sc["R12"], sc["t12"], sc["s12"])
    J9, J5 = M.numeric_jacobian(st, pb, False), M.numeric_jacobian(st, pb, False, delta=1e-5)
    rel = np.abs(J9 - J5).max(axis=(0, 1)) / np.abs(J5).max(axis=(0, 1))  # per column, relative to its largest entry
    print("numeric Jacobian, step 1e-9 against 1e-5: relative difference per column %s" % np.array2string(rel, precision=2))
    assert rel.max() < 1e-5, rel


def test_exp_branches_agree_at_their_boundaries_and_update_composes():
    rng = np.random.default_rng(3)
    for _ in range(20):
        x = np.r_[rng.normal(0, 0.2, 3), rng.normal(0, 0.3, 3), rng.normal(0, 0.1)]
        q, t, s = M.sim3_exp(x)
        # exp(x) exp(-x) = identity (the published branch for |sigma| >= eps, theta >= eps is the exact closed form)
        q2, t2, s2 = M.sim3_update((q, t, s), -x, False)
        assert abs(s2 - 1.0) < 1e-12 and np.abs(t2).max() < 1e-12 and np.abs(M.quat_to_matrix(q2) - np.eye(3)).max() < 1e-12
    # theta just below and above eps with sigma = 0: the two rotation branches meet
    for th in (0.999e-5, 1.001e-5):
        q, t, s = M.sim3_exp(np.r_[th, 0, 0, 0.1, 0.2, 0.3, 0.0])
        assert abs(q[0] - th / 2) < 1e-15 and np.abs(t - [0.1, 0.2, 0.3]).max() < 1e-5 and s == 1.0


def test_outputs_follow_o9():
    sc = M.make_scene(100, 71)
    r = M.optimize_sim3(sc)
    assert np.array_equal(r["R12"], r["R12_d"].astype(np.float32)) and np.array_equal(r["t12"], r["t12_d"].astype(np.float32))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = r["s12_d"] * r["R12_d"], r["t12_d"]
    assert np.array_equal(r["T12"], T.astype(np.float32))
    Scw = T @ np.asarray(sc["T2w"], np.float64)   # S12 * Smw in matrix form
    assert np.abs(r["Scw"] - Scw).max() < 1e-5 and np.array_equal(r["Scw"][3], [0, 0, 0, 1])
    # the summation order and a one-ulp libm change move the state a little and no classification
    dev, flips = M.model_spread(sc, r)
    print("model spread on one scene: %.3e" % dev)
    assert 0 < dev < 1e-6 and flips == 0


def test_every_parity_scene_is_clear_of_the_thresholds():
    names = [n for n, _ in M.PARITY_SCENES]
    assert len(set(names)) == len(names) == 2 * len(M.PARITY_SIZES) + 4
    kinds = set()
    for name, sc in M.PARITY_SCENES:
        r = M.optimize_sim3(sc)
        assert r["margin"] >= 1e-6, (name, r["margin"])
        assert len(sc["valid"]) > r["n_correspondences"] and not np.asarray(sc["valid"], bool)[:len(sc["valid"])].all()
        kinds.add((r["stages"], r["n_bad"] > 0))
    assert kinds == {(1, False), (1, True), (2, False), (2, True)}
    assert M.LDS_PAIRS + 1 in M.PARITY_SIZES
