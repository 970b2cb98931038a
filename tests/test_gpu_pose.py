"""Optimizer::PoseOptimization on the device (orbgpu_pose_optimization*) against the float64 restatement in
pose_model.py -- vs CPU restatement; g2o boundary unpinned.  Discrete outputs are compared exactly on every scene whose
margin (least |chi2 / threshold - 1| in the model) is >= 1e-6; the pose within 16 x the model's own spread under permuted
summation order; the float pose within 1 ulp; determinism and the three flavours as bytes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import pose_model as M  # noqa: E402
import scenario  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    from orb_slam2_map_amd import lib
    if lib.device_count() < 1:
        pytest.skip("no HIP device")
    return lib


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def F(G):
    import fuzz_pose
    return fuzz_pose


def _cap(G):
    e = G.ORBextractor(2000)
    cap = e.max_keypoints(1280, 960)
    e.close()
    return cap


def test_parity_with_the_model_over_sizes_and_kinds(G, torch, F):
    cap = _cap(G)
    assert cap > 1536, cap  # more edges than fit the workgroup's LDS: the spill path
    scenes = []
    for mode in ("mono", "stereo", "mixed"):
        for k, n in enumerate((3, 9, 10, 40, 150, 400, 1000, cap)):
            scenes.append(M.make_scene(n, 1000 + 17 * k + len(mode), mode=mode, assoc_frac=1.0 if n < 40 or n == cap else 0.8))
    got = F.run_batch(torch, scenes)
    assert G.pose_last_spills() == 3  # the three cap-sized scenes
    rep = F.compare(scenes, got)
    print("pose parity: compared %d, left out %d, model spread %.3e, device deviation %.3e, float pose <= %d ulp" % (
        rep["compared"], rep["left_out"], rep["spread"], rep["device_dev"], rep["float_ulp"]))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "pose_parity.json"), "w") as f:
        json.dump({"note": "vs CPU restatement; g2o boundary unpinned", "scenes": len(scenes), "compared": rep["compared"],
                   "left_out": rep["left_out"], "model_permutation_spread": rep["spread"], "device_max_deviation": rep["device_dev"],
                   "float_pose_max_ulp": rep["float_ulp"], "mismatches": rep["mismatches"]}, f, indent=1)
    assert rep["left_out"] <= 0.01 * len(scenes), rep
    assert not rep["mismatches"], rep["mismatches"][:10]
    assert all(r["rounds"] == (0 if r["n_initial"] < 3 else 1 if r["n_initial"] < 10 else 4) for _, r, _ in got)


def test_same_bytes_alone_in_a_batch_and_through_every_flavour(G, torch, F):
    sc = M.make_scene(600, 4242)
    others = [M.make_scene(int(n), 5000 + i) for i, n in enumerate(np.random.default_rng(1).integers(3, 1200, 127))]
    alone = F.run_batch(torch, [sc])[0]
    again = F.run_batch(torch, [sc])[0]
    assert alone[0] == again[0] and np.array_equal(alone[2], again[2])
    for pos in (0, 63, 127):
        batch = others[:pos] + [sc] + others[pos:]
        got = F.run_batch(torch, batch)[pos]
        assert got[0] == alone[0] and np.array_equal(got[2], alone[2]), pos
    # single-problem device entry
    p, d = F.upload(torch, sc)
    G.pose_optimization_device(p, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    one = F.download(d, sc["n"])
    assert one[0] == alone[0] and np.array_equal(one[2], alone[2])
    # host flavour: world positions per key point
    n = sc["n"]
    has = (sc["kp_to_mp"] >= 0).astype(np.uint8)
    wp = sc["world_pos"][sc["kp_to_mp"].clip(0)]
    fr = G.Frame(sc["kps_xy"][:, 0], sc["kps_xy"][:, 1], sc["octave"], np.zeros(n, np.float32), sc["u_right"],
                 np.zeros((n, 32), np.uint8), 640, 480, np.ones(M.NLEVELS, np.float32))
    fx, fy, cx, cy, bf = (float(k) for k in sc["K"])
    ni, T, out, res = G.pose_optimization(fr, has, wp, sc["Tcw"], sc["inv_level_sigma2"], fx, fy, cx, cy, bf,
                                          outlier=np.full(n, F.SENTINEL, np.uint8))
    ref = alone[1]
    assert ni == ref["n_inliers"] and T.tobytes() == ref["Tcw"].tobytes() and np.array_equal(out, alone[2])
    assert all(np.array_equal(res[k], ref[k]) for k in ref)
    # table flavour: ids instead of rows, one unknown id
    tb = G.MapPointTable()
    rows = len(sc["world_pos"])
    ids = 1000 + 3 * np.arange(rows, dtype=np.int64)
    tb.upsert(ids, world_pos=sc["world_pos"], normal=np.zeros((rows, 3), np.float32), min_dist=np.ones(rows, np.float32),
              max_dist=np.ones(rows, np.float32), desc=np.zeros((rows, 32), np.uint8))
    df = G.DeviceFrame().upload(fr)
    kp_ids = np.where(sc["kp_to_mp"] >= 0, ids[sc["kp_to_mp"].clip(0)], -1)
    ni, T, out, res = G.pose_optimization_table(df, tb, kp_ids, sc["Tcw"], sc["inv_level_sigma2"], fx, fy, cx, cy, bf,
                                                outlier=np.full(n, F.SENTINEL, np.uint8))
    assert ni == ref["n_inliers"] and np.array_equal(out, alone[2]) and all(np.array_equal(res[k], ref[k]) for k in ref)
    assert tb.last_unknown() == (0, 0)
    free = int(np.flatnonzero(sc["kp_to_mp"] < 0)[0])
    kp_ids[free] = 5  # an id the table was never told about: not an edge, counted
    ni2, _, out2, res2 = G.pose_optimization_table(df, tb, kp_ids, sc["Tcw"], sc["inv_level_sigma2"], fx, fy, cx, cy, bf,
                                                   outlier=np.full(n, F.SENTINEL, np.uint8))
    assert ni2 == ni and np.array_equal(out2, out) and tb.last_unknown() == (0, 1)
    assert all(np.array_equal(res2[k], ref[k]) for k in ref)


def test_non_finite_points_bad_indices_and_padding(G, torch, F):
    scenes = []
    sc = M.make_scene(200, 31, assoc_frac=1.0)
    sc["world_pos"][sc["kp_to_mp"][4]] = np.nan
    scenes.append(sc)
    sc = M.make_scene(200, 32, assoc_frac=1.0)
    T = sc["Tcw_true"]
    sc["world_pos"][sc["kp_to_mp"][4]] = ((np.array([0.1, 0.1, -2.0]) - T[:3, 3]) @ T[:3, :3]).astype(np.float32)
    sc["world_pos"][sc["kp_to_mp"][9]] = (-T[:3, 3] @ T[:3, :3]).astype(np.float32)  # the camera centre: z = 0
    scenes.append(sc)
    sc = M.make_scene(200, 33, assoc_frac=0.9)
    e = np.flatnonzero(sc["kp_to_mp"] >= 0)
    sc["kp_to_mp"][e[3]] = len(sc["world_pos"])
    sc["kp_to_mp"][e[5]] = 1 << 30
    sc["octave"][e[7]] = M.NLEVELS
    sc["octave"][e[8]] = -3
    scenes.append(sc)
    scenes.append(M.make_scene(2, 34, assoc_frac=1.0))
    scenes.append(M.make_scene(50, 35, assoc_frac=0.0))
    got = F.run_batch(torch, scenes, caps=[256, 200, 777, 2, 64])  # key-point arrays longer than n: the tail is not read
    rep = F.compare(scenes, got)
    assert rep["left_out"] == 0 and not rep["mismatches"], rep["mismatches"]
    assert got[2][1]["n_bad_index"] == 4
    assert got[3][1]["n_inliers"] == 0 and got[3][1]["Tcw"].tobytes() == scenes[3]["Tcw"].tobytes()
    assert got[4][1]["n_initial"] == 0 and np.all(got[4][2] == F.SENTINEL)
    # the scene with a NaN point: the model's answer bit for bit is the input pose's quaternion round trip
    m = M.run_model(scenes[0])
    assert got[0][1]["trials"] == m["trials"] == 40 and np.array_equal(got[0][1]["Tcw_d"], m["Tcw_d"])


def test_spill_path_gives_the_same_bytes():
    """ORBGPU_DEBUG_POSE_LDS_EDGES=0 sends every problem through the global-memory spill; a fresh process each, so that
    the hook is read at its first call."""
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\n"
            "import torch, fuzz_pose as F, pose_model as M\nfrom orb_slam2_map_amd import lib as G\n"
            "sc = [M.make_scene(n, 900 + n) for n in (3, 40, 700, 1500)]\n"
            "got = F.run_batch(torch, sc)\n"
            "print('SPILLS', G.pose_last_spills())\n"
            "print('BYTES', ''.join(g[0].hex() + g[2].tobytes().hex() for g in got))\n") % (
                ROOT, HERE, os.path.join(ROOT, "tools"))
    outs = []
    for lim in (None, "0"):
        env = dict(os.environ)
        env.pop("ORBGPU_DEBUG_POSE_LDS_EDGES", None)
        if lim is not None:
            env["ORBGPU_DEBUG_POSE_LDS_EDGES"] = lim
        r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env,
                           timeout=300)
        assert r.returncode == 0, r.stdout[-3000:]
        outs.append({l.split()[0]: l.split()[1] for l in r.stdout.splitlines() if l.startswith(("SPILLS", "BYTES"))})
    assert outs[0]["SPILLS"] == "0" and outs[1]["SPILLS"] == "4"
    assert outs[0]["BYTES"] == outs[1]["BYTES"]


def test_chain_from_the_motion_model_matcher(G, torch, F):
    """extract -> frame glue -> orbgpu_search_by_projection_last_device -> pose optimisation with nothing but poses crossing
    to the host: the association array and the world positions are the matcher's own device arrays.  The model runs on
    the downloaded copies."""
    from orb_slam2_map_amd.synth import Stream
    rng = np.random.default_rng(7)
    w, h = 640, 480
    st = Stream(w, h, 1234)
    fr = [st.frame(30), st.frame(31)]
    ge = G.ORBextractor(1000, max_batch=2)
    cap = ge.max_keypoints(w, h)
    s = torch.cuda.current_stream().cuda_stream
    img = torch.from_numpy(np.stack([f[0] for f in fr])).cuda()
    depth = torch.from_numpy(np.stack([f[2] for f in fr])).cuda()
    kps = torch.zeros((2, cap, 7), dtype=torch.float32, device="cuda")
    desc = torch.zeros((2, cap, 32), dtype=torch.uint8, device="cuda")
    nout = torch.zeros(2, dtype=torch.int32, device="cuda")
    ge.extract_batch_device(img.data_ptr(), 2, w, h, w, w * h, kps.data_ptr(), desc.data_ptr(), cap, nout.data_ptr(), s)
    ur = torch.zeros((2, cap), dtype=torch.float32, device="cuda")
    dz = torch.zeros((2, cap), dtype=torch.float32, device="cuda")
    cs = torch.zeros((2, 64 * 48 + 1), dtype=torch.int32, device="cuda")
    items = torch.zeros((2, cap), dtype=torch.int32, device="cuda")
    fx, fy, cx, cy, bf = (float(v) for v in (st.fx, st.fy, st.cx, st.cy, st.bf))
    cam = G.make_camera(fx, fy, cx, cy, bf, w, h)
    G.frame_glue_batch_device(2, cap, kps.data_ptr(), nout.data_ptr(), depth.data_ptr(), w, w * h, cam, None,
                              ur.data_ptr(), dz.data_ptr(), cs.data_ptr(), items.data_ptr(), s)
    torch.cuda.synchronize()
    n0, n1 = int(nout[0]), int(nout[1])
    hk = kps.cpu().numpy().view(G.KEYPOINT_DTYPE).reshape(2, cap)
    sf = np.asarray(ge.GetScaleFactors(), np.float32)
    sg = np.asarray(ge.GetInverseScaleSigmaSquares(), np.float32)
    Tcw = scenario.rigid()
    (px, py), (ox, oy) = st.offset(30), st.offset(31)
    P, _ = scenario.world_points_from_prev(hk[0, :n0], fr[0][2], (ox - px, oy - py), st, Tcw, rng)

    def padded(a, shape, dtype):
        out = np.zeros(shape, dtype)
        out[:len(a)] = a
        return torch.from_numpy(out).cuda()
    d_has = padded((rng.random(n0) < 0.8).astype(np.uint8), cap, np.uint8)
    d_wp = padded(P, (cap, 3), np.float32)
    fv = G.DeviceFrameView()
    fv.cap, fv.n, fv.kps, fv.desc = cap, nout.data_ptr() + 4, kps.data_ptr() + cap * 28, desc.data_ptr() + cap * 32
    fv.u_right, fv.cell_start, fv.cell_items = ur.data_ptr() + cap * 4, cs.data_ptr() + (64 * 48 + 1) * 4, items.data_ptr() + cap * 4
    fv.nlevels, fv.scale_factors = len(sf), sf.ctypes.data
    fv.min_x, fv.max_x, fv.min_y, fv.max_y = 0.0, float(w), 0.0, float(h)
    lv = G.DeviceLastFrameView()
    lv.cap, lv.n, lv.kps, lv.desc = cap, nout.data_ptr(), kps.data_ptr(), desc.data_ptr()
    lv.has_mp, lv.outlier, lv.obs_pos, lv.world_pos = d_has.data_ptr(), None, None, d_wp.data_ptr()
    k2m = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
    counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    # the motion-model prediction is a little off; the matcher runs at it, the optimiser starts from it
    T0 = (scenario.rigid(0.012, -0.018, 0.016, (0.035, -0.025, 0.06))).astype(np.float32)
    G.search_by_projection_last_device(fv, T0, lv, Tcw, fx, fy, cx, cy, bf, bf / fx, 15.0, False, True, k2m.data_ptr(),
                                       counts.data_ptr(), stream=s)
    d_out = torch.full((cap,), F.SENTINEL, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(G.C.sizeof(G.PoseResult), dtype=torch.uint8, device="cuda")
    G.pose_optimization_device({"frame": fv, "d_kp_to_mp": k2m.data_ptr(), "d_world_pos": d_wp.data_ptr(), "rows": cap,
                                "Tcw": T0, "inv_level_sigma2": sg, "fx": fx, "fy": fy, "cx": cx, "cy": cy, "mbf": bf,
                                "d_outlier": d_out.data_ptr(), "d_result": d_res.data_ptr()}, stream=s)
    torch.cuda.synchronize()
    assert int(counts[0]) > 100
    res = G.PoseResult.from_buffer_copy(d_res.cpu().numpy().tobytes()).as_dict()
    hk1 = hk[1, :n1]
    sc = {"n": n1, "kps_xy": np.stack([hk1["x"], hk1["y"]], 1), "octave": hk1["octave"], "u_right": ur[1, :n1].cpu().numpy(),
          "kp_to_mp": k2m.cpu().numpy()[:n1], "world_pos": d_wp.cpu().numpy(), "Tcw": T0, "inv_level_sigma2": sg,
          "K": (st.fx, st.fy, st.cx, st.cy, st.bf)}
    rep = F.compare([sc], [(None, res, d_out.cpu().numpy()[:n1])])
    print("chain: edges %d, inliers %d, spread %.3e, device deviation %.3e" % (res["n_initial"], res["n_inliers"],
                                                                              rep["spread"], rep["device_dev"]))
    assert rep["left_out"] == 0 and not rep["mismatches"], rep["mismatches"]
    assert res["n_initial"] == int(counts[0]) and res["n_inliers"] > 50
    assert np.abs(res["Tcw_d"] - Tcw.astype(np.float64)).max() < np.abs(T0.astype(np.float64) - Tcw).max()

    # second half (Tracking::TrackLocalMap): SearchLocalPoints at the optimised pose over a table whose row i is the last
    # frame's key point i (so the associations carry over), then the optimiser again on what the matcher wrote
    T1 = res["Tcw"].copy()
    Ow = -Tcw[:3, :3].T.astype(np.float64) @ Tcw[:3, 3].astype(np.float64)
    dist = np.linalg.norm(P.astype(np.float64) - Ow, axis=1)
    normal = ((P.astype(np.float64) - Ow) / dist[:, None]).astype(np.float32)
    max_d = (dist * sf[hk[0, :n0]["octave"]]).astype(np.float32)
    tb = G.DeviceMapPointTable()
    dev = {"world_pos": d_wp, "normal": padded(normal, (cap, 3), np.float32), "max_dist": padded(max_d, cap, np.float32),
           "min_dist": padded(max_d / sf[-1], cap, np.float32), "desc": desc[0].contiguous()}
    tb.m = n0
    for k, v in dev.items():
        setattr(tb, k, v.data_ptr())
    tb.skip, tb.obs_pos = None, None
    before = k2m.clone()
    G.search_local_points_device(fv, tb, T1, fx, fy, cx, cy, bf, float(np.log(np.float32(sf[1]))), 3.0, 0.8, k2m.data_ptr(),
                                 counts.data_ptr(), stream=s)
    d_out.fill_(F.SENTINEL)
    G.pose_optimization_device({"frame": fv, "d_kp_to_mp": k2m.data_ptr(), "d_world_pos": d_wp.data_ptr(), "rows": n0,
                                "Tcw": T1, "inv_level_sigma2": sg, "fx": fx, "fy": fy, "cx": cx, "cy": cy, "mbf": bf,
                                "d_outlier": d_out.data_ptr(), "d_result": d_res.data_ptr()}, stream=s)
    torch.cuda.synchronize()
    res2 = G.PoseResult.from_buffer_copy(d_res.cpu().numpy().tobytes()).as_dict()
    sc2 = dict(sc, kp_to_mp=k2m.cpu().numpy()[:n1], Tcw=T1, world_pos=d_wp.cpu().numpy()[:n0])
    rep2 = F.compare([sc2], [(None, res2, d_out.cpu().numpy()[:n1])])
    print("chain, after SearchLocalPoints: new matches %d, edges %d, inliers %d, spread %.3e, device deviation %.3e" % (
        int(counts[0]), res2["n_initial"], res2["n_inliers"], rep2["spread"], rep2["device_dev"]))
    assert rep2["left_out"] == 0 and not rep2["mismatches"], rep2["mismatches"]
    assert res2["n_initial"] == int((k2m[:n1] >= 0).sum()) >= res["n_initial"] and bool((k2m[before >= 0] >= 0).all())


def test_fuzz_slice(G, F):
    tot = F.run(5.0, 20261)
    print("fuzz slice: %r" % {k: v for k, v in tot.items() if k != "mismatches"})
    assert tot["compared"] > 0 and not tot["mismatches"], tot["mismatches"][:10]
    assert tot["left_out"] <= 0.01 * (tot["compared"] + tot["left_out"])
