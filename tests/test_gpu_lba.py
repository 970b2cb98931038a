"""Optimizer::LocalBundleAdjustment on the device (orbgpu_local_ba*) against the float64 restatement in lba_model.py -- vs
CPU restatement; g2o boundary unpinned.  The comparison rule is test_gpu_pose.py's: discrete outputs exactly, poses and
points within 16 x the model's own spread under permuted summation order, float outputs within 1 ulp of the rounded model,
on every scene whose model is stable under those permutations (margin >= 1e-6, one accept / reject trace); determinism, the
two homes of the reduced system and the flavours as bytes."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import lba_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

# (free, fixed cameras, points, share of the cameras that see a point, permutations of the model)
SHAPES = [(1, 1, 6, 0.7, 4), (2, 0, 8, 0.7, 4), (3, 2, 40, 0.7, 4), (8, 4, 300, 0.5, 3), (17, 5, 600, 0.3, 2)]
MODES = ("mono", "stereo", "mixed")
TALLY = {"scenes": 0, "compared": 0, "left_out": 0}
RESULT_BYTES = 72  # sizeof(orbgpu_local_ba_result); its last int32 is reduced_in_lds


def shape_scenes(k):
    nf, nx, npts, obs, _ = SHAPES[k]
    return [M.make_scene(nf, nx, npts, 100 + 10 * k + j, mode=mode, kf0_fixed=(nx == 0), obs_frac=obs) for j, mode in enumerate(MODES)]


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
    import fuzz_lba
    return fuzz_lba


def _record(name, entry):
    path = os.path.join(ROOT, "profiles", "lba_parity.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    doc = {"note": "vs CPU restatement; g2o boundary unpinned", "cases": {}}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc["cases"][name] = entry
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)


def _check(F, name, scenes, got, n_perm, keys=None, may_leave_out=0):
    rep = F.compare(scenes, got, n_perm=n_perm, keys=keys)
    print("%s: compared %d, left out %d, model spread %.3e / %.3e, device deviation %.3e / %.3e (poses / points), float "
          "outputs <= %d ulp" % (name, rep["compared"], rep["left_out"], rep["spread_pose"], rep["spread_point"],
                                 rep["dev_pose"], rep["dev_point"], rep["float_ulp"]))
    _record(name, {k: rep[k] for k in ("compared", "left_out", "spread_pose", "spread_point", "dev_pose", "dev_point",
                                       "float_ulp", "mismatches")})
    assert not rep["mismatches"], rep["mismatches"][:10]
    assert rep["left_out"] <= may_leave_out, rep
    return rep


@pytest.mark.parametrize("k", range(len(SHAPES)), ids=["%d-%d-%d" % s[:3] for s in SHAPES])
def test_parity_with_the_model(G, torch, F, k):
    scenes = shape_scenes(k)
    if SHAPES[k][1] == 0:
        assert all(sc["fixed"].sum() == 1 for sc in scenes)  # KF 0 among the local key frames
    got = F.run_batch(torch, scenes)
    assert G.local_ba_last_spills() == 0 and all(r["reduced_in_lds"] == 1 for _, r, _ in got)
    rep = _check(F, "shape %d-%d-%d" % SHAPES[k][:3], scenes, got, SHAPES[k][4], keys=["shape%d-%s" % (k, m) for m in MODES],
                 may_leave_out=len(scenes))
    for key in ("compared", "left_out"):
        TALLY[key] += rep[key]
    TALLY["scenes"] += len(scenes)
    # at most one scene in eight of the whole set (15 scenes: one) may be left out
    assert TALLY["left_out"] <= (len(SHAPES) * len(MODES)) // 8, TALLY
    assert all(r["rounds"] == 2 and r["stopped"] == 0 and r["n_edges"] == len(sc["e_point"]) for sc, (_, r, _) in zip(scenes, got))


def test_reduced_system_in_lds_and_in_global_memory_give_the_same_bytes(G, torch, F):
    scenes = shape_scenes(len(SHAPES) - 1)
    in_lds = F.run_batch(torch, scenes)
    assert G.local_ba_last_spills() == 0
    os.environ["ORBGPU_DEBUG_LBA_LDS_POSES"] = "2"
    try:
        in_global = F.run_batch(torch, scenes)
        assert G.local_ba_last_spills() == len(scenes)
        small = F.run_batch(torch, shape_scenes(1))  # one free pose: still fits
        assert G.local_ba_last_spills() == 0 and all(r["reduced_in_lds"] == 1 for _, r, _ in small)
    finally:
        del os.environ["ORBGPU_DEBUG_LBA_LDS_POSES"]
    for (a, ra, _), (b, rb, _) in zip(in_lds, in_global):
        assert ra["reduced_in_lds"] == 1 and rb["reduced_in_lds"] == 0
        # everything but the member that names the path
        assert a[:RESULT_BYTES - 4] == b[:RESULT_BYTES - 4] and a[RESULT_BYTES:] == b[RESULT_BYTES:]
    _check(F, "global-memory path", scenes, in_global, SHAPES[-1][4], keys=["shape%d-%s" % (len(SHAPES) - 1, m) for m in MODES],
           may_leave_out=1)


def _stripped(which):
    sc = M.make_scene(3, 2, 40, 16, mode="stereo", outlier_frac=0.0, noise=0.2)
    hit = sc["e_point"] == 5 if which == "point" else sc["e_pose"] == 1
    sc["e_xy"][hit] += np.float32(80.0) * np.where(np.arange(hit.sum())[:, None] % 2 == 0, 1, -1).astype(np.float32)
    return sc, hit


def test_vertices_round_one_strips_keep_their_round_one_estimate(G, torch, F):
    """Every edge of one point, and every edge of one free pose, goes to level 1 after round 1: the vertex takes no part
    in round 2 (its Hll never reaches the inverse) and keeps what round 1 left, which the model computes by stopping
    between the rounds."""
    scenes, hits = zip(*[_stripped(w) for w in ("point", "pose")])
    got = F.run_batch(torch, list(scenes))
    _check(F, "stripped vertices", list(scenes), got, 3)
    for which, sc, hit, (_, r, a) in zip(("point", "pose"), scenes, hits, got):
        one = M.local_ba(sc, stop_between=True)
        full = F.reference(sc, 3)[0]
        assert a["erase"][hit].all() and r["rounds"] == 2
        if which == "point":
            assert np.array_equal(full["pos_d"][5], one["pos_d"][5])
            assert np.abs(a["pos_d"][5] - one["pos_d"][5]).max() <= 16 * F.reference(sc, 3)[2]
            assert np.isfinite(a["pos_d"]).all()
        else:
            assert np.array_equal(full["Tcw_d"][1], one["Tcw_d"][1])
            assert np.abs(a["Tcw_d"][1] - one["Tcw_d"][1]).max() <= 16 * F.reference(sc, 3)[1]


def test_all_local_poses_fixed_is_points_only(G, torch, F):
    scenes = []
    # points alone converge within a few iterations, after which rho is rounding noise: seeds whose model is stable
    for mode, seed in zip(MODES, (303, 301, 301)):
        sc = M.make_scene(2, 2, 30, seed, mode=mode, rot_sigma=0.0, trans_sigma=0.0)
        sc["fixed"][:] = 1
        scenes.append(sc)
    got = F.run_batch(torch, scenes)
    _check(F, "points only", scenes, got, 3)
    for sc, (_, r, a) in zip(scenes, got):
        assert r["rounds"] == 2 and r["reduced_in_lds"] == 1
        m = F.reference(sc, 3)[0]
        assert np.array_equal(a["Tcw_d"], m["Tcw_d"])  # the quaternion round trip of the input, bit for bit


def test_non_finite_points_bad_indices_and_padding(G, torch, F):
    scenes = []
    sc = M.make_scene(3, 2, 40, 31, mode="mixed")
    sc["world_pos"][4] = np.nan
    scenes.append(sc)
    sc = M.make_scene(3, 2, 40, 32, mode="mixed")
    T = sc["Tcw"][1].astype(np.float64)
    sc["world_pos"][9] = (-T[:3, 3] @ T[:3, :3]).astype(np.float32)  # (about) the centre of free camera 1: z = 0
    T = sc["Tcw_true"][4]
    sc["world_pos"][4] = ((np.array([0.1, 0.1, -2.0]) - T[:3, 3]) @ T[:3, :3]).astype(np.float32)  # behind a fixed camera
    scenes.append(sc)
    sc = M.make_scene(3, 2, 40, 33, mode="mixed")
    sc["e_point"][3] = 40
    sc["e_point"][5] = 1 << 30
    sc["e_point"][6] = -1
    sc["e_pose"][8] = 5
    sc["e_pose"][9] = -7
    sc["e_oct"][11] = M.NLEVELS
    sc["e_oct"][12] = -3
    scenes.append(sc)
    # arrays longer than the counts say: the tail (out-of-range rows, NaN) is not read
    sc = M.make_scene(3, 2, 40, 34, mode="mixed")
    padded = dict(sc)
    E = len(sc["e_point"])
    padded["e_point"] = np.r_[sc["e_point"], [1 << 29] * 5].astype(np.int32)
    padded["e_pose"] = np.r_[sc["e_pose"], [-1] * 5].astype(np.int32)
    padded["e_oct"] = np.r_[sc["e_oct"], [99] * 5].astype(np.int32)
    padded["e_xy"] = np.vstack([sc["e_xy"], np.full((5, 2), np.nan, np.float32)])
    padded["e_ur"] = np.r_[sc["e_ur"], [np.nan] * 5].astype(np.float32)
    padded["world_pos"] = np.vstack([sc["world_pos"], np.full((3, 3), np.nan, np.float32)])
    scenes.append(sc)
    ups = [F.upload(torch, s) for s in scenes[:3]]
    pp, pd = F.upload(torch, padded)
    pp.update(n_edges=E, n_points=40)
    G.local_ba_batch_device([u[0] for u in ups] + [pp], stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = [F.download(u[1], s) for u, s in zip(ups, scenes[:3])] + [F.download(pd, sc)]
    rep = _check(F, "non-finite, out of range, padded", scenes, got, 3, may_leave_out=1)
    assert rep["compared"] >= 3
    assert got[2][1]["n_bad_index"] == 7 and (got[2][2]["erase"][[3, 5, 6, 8, 9, 11, 12]] == F.SENTINEL).all()
    # beyond the counts nothing was written either
    assert (pd["erase"].cpu().numpy()[E:] == F.SENTINEL).all() and (pd["pos"].cpu().numpy()[40:] == F.SENTINEL).all()
    # the NaN point is erased from every key frame by the depth test and stays NaN; everything else is finite
    a = got[0][2]
    assert a["erase"][scenes[0]["e_point"] == 4].all() and np.isnan(a["pos_d"][4]).all()
    assert np.isfinite(np.delete(a["pos_d"], 4, axis=0)).all() and np.isfinite(a["Tcw_d"]).all()


def test_same_bytes_alone_in_a_batch_and_through_the_host_flavour(G, torch, F):
    sc = M.make_scene(5, 3, 120, 4242, mode="mixed", obs_frac=0.6)
    rng = np.random.default_rng(1)
    others = [M.make_scene(int(rng.integers(1, 5)), int(rng.integers(0, 3)), int(rng.integers(6, 60)), 5000 + i,
                           kf0_fixed=bool(i % 5 == 0)) for i in range(63)]
    alone = F.run_batch(torch, [sc])[0]
    again = F.run_batch(torch, [sc])[0]
    assert alone[0] == again[0]
    for pos in (0, 31, 63):
        batch = others[:pos] + [sc] + others[pos:]
        got = F.run_batch(torch, batch)[pos]
        assert got[0] == alone[0], pos
    p, d = F.upload(torch, sc)
    G.local_ba_device(p, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert F.download(d, sc)[0] == alone[0]
    # host flavour: sentinel-filled arrays in, the same bytes out
    nl, m, e = sc["n_local"], len(sc["world_pos"]), len(sc["e_point"])
    Td, T, Xd, X, er, res = G.local_ba(F.to_problem(sc), Tcw_d=np.full((nl, 4, 4), 7.0), Tcw=np.full((nl, 4, 4), 7.0),
                                       pos_d=np.full((m, 3), 7.0), pos=np.full((m, 3), 7.0), erase=np.full(e, F.SENTINEL))
    assert res == alone[1]
    assert Td.tobytes() + T.tobytes() + Xd.tobytes() + X.tobytes() + er.tobytes() == alone[0][RESULT_BYTES:]
    assert G.local_ba(F.to_problem(sc), stop=0)[5] == alone[1]


def test_stop_flag(G, torch, F):
    sc = M.make_scene(3, 2, 40, 77, mode="mixed")
    null, zero, set_ = F.run_batch(torch, [sc, sc, sc], stops=[None, 0, 1])
    assert zero[0] == null[0] and null[1]["stopped"] == 0 and null[1]["rounds"] == 2
    r, a = set_[1], set_[2]
    assert r["stopped"] == 1 and r["rounds"] == 0 and r["iterations"] == [0, 0] and r["trials"] == [0, 0] and r["n_erased"] == 0
    assert r["n_edges"] == len(sc["e_point"])
    for k in ("Tcw_d", "Tcw", "pos_d", "pos", "erase"):  # sentinel-filled outputs are intact
        assert (a[k] == F.SENTINEL).all(), k
    m = M.local_ba(sc, stop_before=True)
    assert m["stopped"] == 1 and m["rounds"] == 0
    # host flavour: the flag is sampled at the call
    nl = sc["n_local"]
    Td, T, Xd, X, er, res = G.local_ba(F.to_problem(sc), stop=1, Tcw=np.full((nl, 4, 4), 7.0), erase=np.full(len(sc["e_point"]), 7))
    assert res["stopped"] == 1 and (T == 7).all() and (er == 7).all()


def test_fuzz_slice(G, F):
    tot = F.run(5.0, 20262)
    print("fuzz slice: %r" % {k: v for k, v in tot.items() if k != "mismatches"})
    assert tot["compared"] > 0 and not tot["mismatches"], tot["mismatches"][:10]
    assert tot["left_out"] <= F.LEFT_OUT_CAP * (tot["compared"] + tot["left_out"])
