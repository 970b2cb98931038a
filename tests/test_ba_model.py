"""tests/ba_model.py (the oracle of orbgpu_bundle_adjustment*) pinned to the model we already trust: with LBA's Huber value
its single optimize(5) IS round 1 of lba_model.local_ba, bit for bit; and the properties of the definition (B1-B7 in
include/orbgpu.h) that the device tests rely on.  No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import ba_model as B  # noqa: E402
import lba_model as M  # noqa: E402

# (free, fixed cameras, points, KF 0 among the local key frames)
PINNED = [(2, 0, 8, True), (3, 0, 40, True), (17, 0, 600, True), (3, 2, 40, False), (1, 1, 6, False)]


@pytest.mark.parametrize("shape", PINNED, ids=["%d-%d-%d" % s[:3] for s in PINNED])
@pytest.mark.parametrize("mode", ("mono", "mixed"))
def test_one_round_is_local_ba_stopped_between_its_rounds(shape, mode):
    nf, nx, npts, kf0 = shape
    sc = M.make_scene(nf, nx, npts, 900 + npts, mode=mode, kf0_fixed=kf0, obs_frac=0.3 if npts == 600 else 0.7)
    want = M.local_ba(sc, stop_between=True)
    assert want["stopped"] == 1 and want["rounds"] == 1
    pr = B.from_lba_scene(sc)
    assert pr["fixed"][:sc["n_local"]].tolist() == sc["fixed"].tolist() and pr["fixed"][sc["n_local"]:].all()
    got = B.bundle_adjustment(pr, 5, robust=True, huber_chi2=(5.991, 7.815))
    nl = sc["n_local"]
    assert got["Tcw_d"][:nl].tobytes() == want["Tcw_d"].tobytes()
    assert got["pos_d"].tobytes() == want["pos_d"].tobytes()
    assert got["Tcw"][:nl].tobytes() == want["Tcw"].tobytes() and got["pos"].tobytes() == want["pos"].tobytes()
    assert (got["iterations"], got["trials"]) == (want["iterations"][0], want["trials"][0])
    assert got["trace"] == want["trace"] and len(got["trace"]) > 0
    assert got["chi2_start"] == want["chi2_start"][0] and got["chi2_end"] == want["chi2_end"][0]
    assert got["n_edges"] == want["n_edges"] and got["n_not_included"] == 0 and not got["not_included"].any()
    # fixed cameras: the quaternion round trip of their input, whatever the iterations did
    still = B.bundle_adjustment(pr, 0)
    assert got["Tcw_d"][nl:].tobytes() == still["Tcw_d"][nl:].tobytes()


def test_the_huber_value_is_part_of_the_definition():
    """5.99 (Optimizer.cc:85) against LocalBundleAdjustment's 5.991: another delta, another result on a scene whose
    outliers reach the kernel."""
    assert B.deltas()[0] == np.float64(np.float32(np.sqrt(5.99))) and B.deltas()[0] != B.deltas((5.991, 7.815))[0]
    assert B.deltas()[1] == B.deltas((5.991, 7.815))[1]
    pr = B.from_lba_scene(M.make_scene(3, 0, 40, 41, mode="mono", kf0_fixed=True, outlier_frac=0.1))
    a = B.bundle_adjustment(pr, 5)
    b = B.bundle_adjustment(pr, 5, huber_chi2=(5.991, 7.815))
    assert a["Tcw_d"].tobytes() != b["Tcw_d"].tobytes() or a["pos_d"].tobytes() != b["pos_d"].tobytes()
    assert a["chi2_start"] != b["chi2_start"]


def test_robust_off_is_another_optimisation():
    pr = B.from_lba_scene(M.make_scene(3, 0, 40, 42, mode="mixed", kf0_fixed=True, outlier_frac=0.1))
    a = B.bundle_adjustment(pr, 10, robust=True)
    b = B.bundle_adjustment(pr, 10, robust=False)
    assert b["chi2_start"] > 2 * a["chi2_start"]  # plain chi2 of gross outliers against their Huber cost
    assert np.abs(a["Tcw_d"] - b["Tcw_d"]).max() > 1e-6
    # the kernel protects the estimate: with it the poses end nearer the truth
    truth = pr["Tcw_true"]
    assert np.abs(a["Tcw_d"] - truth).max() < np.abs(b["Tcw_d"] - truth).max()


def test_no_iterations_is_the_round_trip():
    sc = M.make_scene(3, 2, 40, 43, mode="mixed")
    pr = B.from_lba_scene(sc)
    r = B.bundle_adjustment(pr, 0)
    assert (r["iterations"], r["trials"], r["trace"], r["stopped"]) == (0, 0, [], 0)
    assert r["chi2_start"] == r["chi2_end"] > 0
    assert np.array_equal(r["pos_d"], sc["world_pos"].astype(np.float64)) and np.array_equal(r["pos"], sc["world_pos"])
    assert np.abs(r["Tcw_d"] - sc["Tcw"].astype(np.float64)).max() < 1e-6  # through the unit quaternion, not bit for bit
    assert r["Tcw_d"].shape == (5, 4, 4) and not r["not_included"].any()
    s = B.bundle_adjustment(pr, 20, stop_before=True)
    assert s["stopped"] == 1 and "Tcw_d" not in s and s["n_edges"] == len(sc["e_point"])


def test_a_point_without_an_edge_is_not_included_and_untouched():
    sc = M.make_scene(3, 0, 40, 44, mode="mixed", kf0_fixed=True)
    pr = B.from_lba_scene(sc)
    hit = pr["e_point"] == 7
    pr["e_pose"] = np.where(hit, -1, pr["e_pose"]).astype(np.int32)  # its observers are in no row: skipped edges
    r = B.bundle_adjustment(pr, 5)
    assert r["not_included"].tolist() == [1 if p == 7 else 0 for p in range(40)] and r["n_not_included"] == 1
    assert r["n_bad_index"] == int(hit.sum()) and r["n_edges"] == len(hit) - int(hit.sum())
    assert np.array_equal(r["pos_d"][7], sc["world_pos"][7].astype(np.float64))
    assert (r["pos_d"][np.arange(40) != 7] != sc["world_pos"].astype(np.float64)[np.arange(40) != 7]).any(axis=1).all()


def test_no_fixed_row_leaves_the_gauge_to_lambda():
    sc = M.make_scene(3, 0, 40, 45, mode="stereo", kf0_fixed=True)
    r = B.bundle_adjustment(B.from_lba_scene(sc, all_free=True), 10)
    assert r["chi2_end"] < r["chi2_start"] and np.isfinite(r["Tcw_d"]).all() and 1 in r["trace"]


def test_gather_all_builds_the_graph_of_the_reference():
    kps = np.array([[10 * j, 5 * j, -1.0, j % 3] for j in range(4)], np.float32)
    kf = lambda i, bad=False: dict(id=i, bad=bad, cov=[], K=(500, 500, 320, 240, 40), Tcw=np.eye(4, dtype=np.float32),  # noqa: E731
                                   inv_sigma2=np.ones(8, np.float32), kps=kps, mps=[-1] * 4)
    mp = {"kfs": [kf(0), kf(1, bad=True), kf(2), kf(9)], "cur": 0,
          "mps": [dict(id=0, bad=False, pos=(0, 0, 1), obs={0: 0, 1: 1, 2: 2}), dict(id=1, bad=True, pos=(0, 0, 2), obs={0: 1}),
                  dict(id=2, bad=False, pos=(0, 0, 3), obs={1: 0, 3: 3}), dict(id=3, bad=False, pos=(0, 0, 4), obs={2: 0, 3: 1})]}
    g = B.gather_all(mp, vp_kfs=[0, 1, 2])  # key frame 3 (id 9) is not handed in: above maxKFid = 2
    assert g["kf_rows"] == [0, 2] and g["points"] == [0, 2, 3] and g["fixed"].tolist() == [1, 0] and g["max_kf_id"] == 2
    assert g["e_point"].tolist() == [0, 0, 2] and g["e_pose"].tolist() == [0, 1, 1] and g["edge_kf"] == [0, 2, 2]
    r = B.bundle_adjustment(g, 2)
    assert r["not_included"].tolist() == [0, 1, 0]
    # an observer with an id within maxKFid that is in no row keeps its edge, with pose -1
    mp["kfs"][3]["id"] = 1
    g = B.gather_all(mp, vp_kfs=[0, 1, 2])
    assert g["e_pose"].tolist() == [0, 1, -1, 1, -1] and B.bundle_adjustment(g, 1)["n_bad_index"] == 2
