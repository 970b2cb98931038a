"""The middle of LoopClosing::CorrectLoop on the device: orbgpu_essential_graph spreads a loop's correction over a
synthetic ring map (poses and points), and what it returns -- Tiw and the corrected points, as they are -- is the input
of orbgpu_bundle_adjustment, the call that follows it (RunGlobalBundleAdjustment).  The bundle adjustment accepts them,
its outputs are finite, and the chi2 it starts from is below the one it starts from on the uncorrected map."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import eg_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

CAM = np.float32([535.4, 539.2, 320.1, 247.6, 40.0])
V, PER_KF, REACH = 20, 12, 2


def ring_map(seed=7):
    """A ring of V key frames that has drifted on its way round (eg_model.make_scene, scale fixed) with PER_KF points per
    key frame, each seen from its own key frame and its neighbours on the TRUE ring -- across the seam too.  A point lies
    where its reference key frame's state puts it: on the drifted map for the rows that still carry their drift, on the
    true one for the rows LoopClosing has corrected already."""
    sc = M.make_scene(V, seed, reach=REACH, fix_scale=True, rot_drift=0.1, trans_drift=0.5, n_corrected=2, n_iterations=20,
                      compose=True)
    rng = np.random.default_rng(seed)
    G = sc["true"]
    pos, ref, e_pt, e_kf, e_xy = [], [], [], [], []
    for r in range(V):
        for _ in range(PER_KF):
            Xc = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(4, 8)])
            Xw = M.s_map(M.s_inv(G[r]), Xc)            # where the point is
            pos.append(M.s_map(M.s_inv(sc["Scw"][r]), Xc))  # where the map has it
            ref.append(r)
            for d in range(-REACH, REACH + 1):
                k = (r + d) % V
                Pc = M.s_map(G[k], Xw)
                if Pc[2] > 0.5:
                    e_pt.append(len(pos) - 1)
                    e_kf.append(k)
                    e_xy.append([CAM[0] * Pc[0] / Pc[2] + CAM[2], CAM[1] * Pc[1] / Pc[2] + CAM[3]])
    sc["world_pos"], sc["point_ref"] = np.float32(pos), np.int32(ref)
    obs = {"edge_point": np.int32(e_pt), "edge_pose": np.int32(e_kf), "edge_octave": np.zeros(len(e_pt), np.int32),
           "edge_xy": np.float32(e_xy), "edge_u_right": np.full(len(e_pt), -1, np.float32)}
    return sc, obs


def ba_problem(Tcw, pos, sc, obs):
    return dict(obs, Tcw=np.asarray(Tcw, np.float32).reshape(-1, 4, 4), fixed=sc["fixed"], cam=np.tile(CAM, (V, 1)),
                inv_level_sigma2=np.ones((V, 8), np.float32), world_pos=np.asarray(pos, np.float32), n_iterations=2, robust=False)


def test_essential_graph_output_feeds_the_global_bundle_adjustment():
    from orb_slam2_map_amd import lib as G
    if G.device_count() < 1:
        pytest.skip("no HIP device")
    import fuzz_eg as F
    sc, obs = ring_map()
    Siw, Tiw, pos, res = G.essential_graph(F.to_problem(sc), world_pos=sc["world_pos"], point_ref=sc["point_ref"])
    assert res["stopped"] == 0 and res["n_bad_ref"] == 0 and res["n_edges"] == len(sc["edge_i"]) and res["iterations"] >= 1
    assert res["chi2_end"] < res["chi2_start"] and np.isfinite(Tiw).all() and np.isfinite(pos).all()
    assert np.array_equal(Tiw.reshape(V, 16), M.tiw_of(Siw))
    before = G.bundle_adjustment(ba_problem(M.tiw_of(sc["Scw"]), sc["world_pos"], sc, obs))
    after = G.bundle_adjustment(ba_problem(Tiw, pos, sc, obs))
    for out in (before, after):
        assert out[5]["n_edges"] == len(obs["edge_point"]) and out[5]["n_bad_index"] == 0 and out[5]["n_not_included"] == 0
    assert np.isfinite(after[1]).all() and np.isfinite(after[3]).all() and np.isfinite(after[5]["chi2_end"])
    print("chain: essential graph chi2 %.3e -> %.3e; bundle adjustment starts from %.3e on the uncorrected map, %.3e on the "
          "corrected one" % (res["chi2_start"], res["chi2_end"], before[5]["chi2_start"], after[5]["chi2_start"]))
    assert after[5]["chi2_start"] < before[5]["chi2_start"]
