"""Optimizer::BundleAdjustment on the device (orbgpu_bundle_adjustment*) against the float64 restatement in ba_model.py -- vs
CPU restatement; g2o boundary unpinned.  The comparison rule is fuzz_lba.compare's (tools/fuzz_ba.py): discrete outputs
exactly, poses and points within 16 x the model's own spread under permuted summation order, float outputs (float) of the
double ones and within 1 ulp of the rounded model, on every scene whose model keeps one accept / reject trace under those
permutations (nothing is classified, so there is no threshold margin); determinism, the two homes of the reduced system
and the flavours as bytes."""
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

import ba_model as B  # noqa: E402
from pose_model import NLEVELS  # noqa: E402

pytestmark = pytest.mark.gpu

# (free, fixed cameras, points, share of the cameras that see a point, permutations of the model, fixed rows)
SHAPES = [(1, 1, 6, 0.7, 4, "cameras"), (2, 0, 8, 0.7, 4, "kf0"), (3, 0, 40, 0.7, 4, "none"), (8, 4, 300, 0.5, 3, "cameras"),
          (17, 0, 600, 0.3, 2, "kf0")]
MODES = ("mono", "stereo", "mixed")
# Seeds chosen with the model ALONE (no device), by running it on the CPU from 100 + 10 k + j (+ 500 without the kernel) in
# steps of 1000 and taking the first seed at which the model meets the comparison rule against ITSELF: over the shape's
# permutations of the summation order and three more, one accept / reject trace (at 20 iterations a converged scene's rho
# is rounding noise), float outputs within 1 ulp of each other, and the three further permutations -- which stand where the
# device will stand -- within 16 x the spread of the shape's own.  The last two conditions matter where the gauge is loose
# -- no fixed row at all, or mono edges with one fixed row (the scale) -- and only lambda keeps S regular: there the model's
# own permutations differ by up to 2e5 float steps, and a spread taken from two of them says little about a third.  A scene
# the model cannot pass against itself tests no device.
# profiles/ba_parity.json (model_only) records the search; with these seeds the parity list leaves out no scene.
SEEDS = {(0, 0, True): 2100, (0, 1, True): 1101, (0, 2, True): 1102, (1, 2, True): 1112, (2, 0, True): 1120, (2, 1, True): 20121,
         (2, 2, True): 7122, (4, 0, True): 15140}
CASES = [(k, True) for k in range(len(SHAPES))] + [(len(SHAPES) - 1, False)]
TALLY = {"scenes": 0, "compared": 0, "left_out": 0}
RESULT_BYTES = 48  # sizeof(orbgpu_bundle_adjustment_result); reduced_in_lds is its last int32 but one (pad_ follows)


def shape_scenes(k, robust=True, n_iterations=20):
    import fuzz_ba as F
    nf, nx, npts, obs, _, fixed = SHAPES[k]
    return [F.make_scene(nf, nx, npts, SEEDS.get((k, j, robust), 100 + 10 * k + j + (0 if robust else 500)), n_iterations=n_iterations,
                         robust=robust, all_free=(fixed == "none"), mode=mode, kf0_fixed=(fixed == "kf0"), obs_frac=obs)
            for j, mode in enumerate(MODES)]


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
    import fuzz_ba
    return fuzz_ba


def _record(name, entry):
    path = os.path.join(ROOT, "profiles", "ba_parity.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    doc = {"note": "vs CPU restatement; g2o boundary unpinned", "cases": {}}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc.setdefault("cases", {})[name] = entry
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


def _without_path(raw):
    """Every output byte but the result member that names the home of S."""
    return raw[:RESULT_BYTES - 8] + raw[RESULT_BYTES - 4:]


@pytest.mark.parametrize("k,robust", CASES, ids=["%d-%d-%d%s" % (SHAPES[k][:3] + ("" if r else "-plain",)) for k, r in CASES])
def test_parity_with_the_model(G, torch, F, k, robust):
    scenes = shape_scenes(k, robust)
    fixed = SHAPES[k][5]
    assert all(int(sc["fixed"].sum()) == {"kf0": 1, "none": 0, "cameras": SHAPES[k][1]}[fixed] for sc in scenes)
    got = F.run_batch(torch, scenes)
    assert G.bundle_adjustment_last_spills() == 0 and all(r["reduced_in_lds"] == 1 for _, r, _ in got)
    name = "shape %d-%d-%d%s" % (SHAPES[k][:3] + ("" if robust else " plain",))
    rep = _check(F, name, scenes, got, SHAPES[k][4], keys=["shape%d-%s-%d" % (k, m, robust) for m in MODES],
                 may_leave_out=len(scenes))
    for key in ("compared", "left_out"):
        TALLY[key] += rep[key]
    TALLY["scenes"] += len(scenes)
    # at most one scene in eight of the whole list (18 scenes: two) may be left out; the seeds above leave out none
    assert TALLY["left_out"] <= (len(CASES) * len(MODES)) // 8, TALLY
    for sc, (_, r, a) in zip(scenes, got):
        assert r["stopped"] == 0 and r["n_edges"] == len(sc["e_point"]) and r["n_not_included"] == 0
        assert 1 <= r["iterations"] <= 20 and r["chi2_end"] < r["chi2_start"] and not a["not_included"].any()


def big_scene():
    import fuzz_ba as F
    return F.make_scene(100, 0, 300, 7, n_iterations=3, mode="mixed", kf0_fixed=True, obs_frac=0.06)


def test_more_free_poses_than_local_ba_takes(G, torch, F):
    """100 free poses and KF 0: beyond ORBGPU_LBA_MAX_FREE, S in the global workspace."""
    sc = big_scene()
    assert len(sc["Tcw"]) == 101 and int(sc["fixed"].sum()) == 1 and G.LBA_MAX_FREE < 100 <= G.BA_MAX_FREE
    per_pose = np.bincount(sc["e_pose"], minlength=101)
    assert 1500 <= len(sc["e_point"]) <= 2200 and per_pose.min() >= 7
    got = F.run_batch(torch, [sc])
    assert G.bundle_adjustment_last_spills() == 1 and got[0][1]["reduced_in_lds"] == 0
    _check(F, "100 free poses", [sc], got, 2)
    assert got[0][1]["iterations"] == 3 and got[0][1]["chi2_end"] < got[0][1]["chi2_start"]


def test_reduced_system_in_lds_and_in_global_memory_give_the_same_bytes(G, torch, F):
    scenes = shape_scenes(len(SHAPES) - 1)
    in_lds = F.run_batch(torch, scenes)
    assert G.bundle_adjustment_last_spills() == 0
    os.environ["ORBGPU_DEBUG_LBA_LDS_POSES"] = "2"
    try:
        in_global = F.run_batch(torch, scenes)
        assert G.bundle_adjustment_last_spills() == len(scenes)
        small = F.run_batch(torch, shape_scenes(0))  # one free pose: still fits
        assert G.bundle_adjustment_last_spills() == 0 and all(r["reduced_in_lds"] == 1 for _, r, _ in small)
    finally:
        del os.environ["ORBGPU_DEBUG_LBA_LDS_POSES"]
    for (a, ra, _), (b, rb, _) in zip(in_lds, in_global):
        assert ra["reduced_in_lds"] == 1 and rb["reduced_in_lds"] == 0
        assert _without_path(a) == _without_path(b)
    _check(F, "global-memory path", scenes, in_global, SHAPES[-1][4], keys=["shape%d-%s-1" % (len(SHAPES) - 1, m) for m in MODES])


def test_same_bytes_alone_in_a_batch_and_through_the_host_flavour(G, torch, F):
    sc = F.make_scene(5, 3, 120, 4242, n_iterations=8, mode="mixed", obs_frac=0.6)
    rng = np.random.default_rng(1)
    others = [F.make_scene(int(rng.integers(1, 5)), int(rng.integers(0, 3)), int(rng.integers(6, 60)), 5000 + i,
                           n_iterations=int(rng.integers(0, 6)), robust=bool(i % 2), kf0_fixed=bool(i % 5 == 0)) for i in range(63)]
    alone = F.run_batch(torch, [sc])[0]
    again = F.run_batch(torch, [sc])[0]
    assert alone[0] == again[0]
    for pos in (0, 31, 63):
        batch = others[:pos] + [sc] + others[pos:]
        got = F.run_batch(torch, batch)[pos]
        assert got[0] == alone[0], pos
    p, d = F.upload(torch, sc)
    G.bundle_adjustment_device(p, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert F.download(d, sc)[0] == alone[0]
    # host flavour: sentinel-filled arrays in, the same bytes out
    P, m = len(sc["Tcw"]), len(sc["world_pos"])
    Td, T, Xd, X, ni, res = G.bundle_adjustment(F.to_problem(sc), Tcw_d=np.full((P, 4, 4), 7.0), Tcw=np.full((P, 4, 4), 7.0),
                                                pos_d=np.full((m, 3), 7.0), pos=np.full((m, 3), 7.0),
                                                not_included=np.full(m, F.SENTINEL))
    assert res == alone[1]
    assert Td.tobytes() + T.tobytes() + Xd.tobytes() + X.tobytes() + ni.tobytes() == alone[0][RESULT_BYTES:]
    assert G.bundle_adjustment(F.to_problem(sc), stop=0)[5] == alone[1]
    # the two optimisers keep separate workspaces: a local BA in between changes nothing
    import fuzz_lba
    import lba_model
    fuzz_lba.run_batch(torch, [lba_model.make_scene(3, 2, 40, 5)])
    assert F.run_batch(torch, [sc])[0][0] == alone[0] and G.bundle_adjustment_last_spills() == 0


def test_stop_flag(G, torch, F):
    sc = F.make_scene(3, 2, 40, 77, n_iterations=6, mode="mixed")
    null, zero, set_ = F.run_batch(torch, [sc, sc, sc], stops=[None, 0, 1])
    assert zero[0] == null[0] and null[1]["stopped"] == 0 and null[1]["iterations"] >= 1
    r, a = set_[1], set_[2]
    assert r["stopped"] == 1 and r["iterations"] == 0 and r["trials"] == 0 and r["chi2_start"] == 0 and r["chi2_end"] == 0
    assert r["n_edges"] == len(sc["e_point"]) and r["n_not_included"] == 0
    for k in F.OUTPUTS:  # sentinel-filled outputs are intact
        assert (a[k] == F.SENTINEL).all(), k
    m = B.bundle_adjustment(sc, 6, stop_before=True)
    assert all(m[k] == r[k] for k in ("stopped", "iterations", "trials", "n_edges", "n_bad_index", "n_not_included"))
    # host flavour: the flag is sampled at the call
    P, npts = len(sc["Tcw"]), len(sc["world_pos"])
    Td, T, Xd, X, ni, res = G.bundle_adjustment(F.to_problem(sc), stop=1, Tcw=np.full((P, 4, 4), 7.0), pos=np.full((npts, 3), 7.0),
                                                not_included=np.full(npts, 7))
    assert res["stopped"] == 1 and (T == 7).all() and (X == 7).all() and (ni == 7).all()


def lone_scenes():
    import fuzz_ba as F
    still = F.make_scene(3, 2, 40, 21, n_iterations=0, mode="mixed")
    lone_point = F.make_scene(3, 0, 40, 22, n_iterations=10, mode="mixed", kf0_fixed=True)
    hit = lone_point["e_point"] == 7
    for key in ("e_point", "e_pose", "e_oct", "e_xy", "e_ur"):
        lone_point[key] = lone_point[key][~hit]
    lone_pose = F.make_scene(3, 2, 40, 23, n_iterations=10, mode="mixed")
    row = int(np.flatnonzero(lone_pose["fixed"] == 0)[1])
    keep = lone_pose["e_pose"] != row
    for key in ("e_point", "e_pose", "e_oct", "e_xy", "e_ur"):
        lone_pose[key] = lone_pose[key][keep]
    return [still, lone_point, lone_pose], row


def test_no_iterations_and_vertices_without_edges(G, torch, F):
    scenes, row = lone_scenes()
    still, lone_point, lone_pose = scenes
    got = F.run_batch(torch, scenes)
    _check(F, "no iterations, lone vertices", scenes, got, 3)
    # n_iterations = 0: the round trip of every input, bit for bit the model's
    _, r, a = got[0]
    m = F.reference(still, 3)[0]
    assert (r["iterations"], r["trials"], r["stopped"]) == (0, 0, 0) and r["chi2_start"] == r["chi2_end"] > 0
    assert np.array_equal(a["Tcw_d"], m["Tcw_d"]) and np.array_equal(a["pos"], still["world_pos"])
    assert np.array_equal(a["pos_d"], still["world_pos"].astype(np.float64))
    # a point without an edge
    _, r, a = got[1]
    assert r["n_not_included"] == 1 and a["not_included"].tolist() == [1 if p == 7 else 0 for p in range(40)]
    assert np.array_equal(a["pos"][7], lone_point["world_pos"][7]) and np.isfinite(a["pos_d"]).all()
    # a free pose without an edge keeps its estimate: the quaternion round trip of its input
    _, r, a = got[2]
    zero = dict(lone_pose, n_iterations=0)
    assert np.array_equal(a["Tcw_d"][row], B.bundle_adjustment(zero, 0)["Tcw_d"][row]) and r["iterations"] >= 1
    assert not np.array_equal(a["Tcw_d"][0], B.bundle_adjustment(zero, 0)["Tcw_d"][0])


POINTS_ONLY_SEEDS = (303, 301, 301)


def points_only_scenes():
    import fuzz_ba as F
    scenes = []
    for mode, seed in zip(MODES, POINTS_ONLY_SEEDS):
        sc = F.make_scene(2, 2, 30, seed, n_iterations=4, mode=mode, rot_sigma=0.0, trans_sigma=0.0)
        sc["fixed"][:] = 1
        scenes.append(sc)
    return scenes


def test_all_rows_fixed_is_points_only(G, torch, F):
    scenes = points_only_scenes()
    got = F.run_batch(torch, scenes)
    _check(F, "points only", scenes, got, 3)
    for sc, (_, r, a) in zip(scenes, got):
        assert r["reduced_in_lds"] == 1 and r["iterations"] >= 1
        assert np.array_equal(a["Tcw_d"], F.reference(sc, 3)[0]["Tcw_d"])  # the quaternion round trip of the input, bit for bit


def odd_scenes():
    import fuzz_ba as F
    scenes = []
    sc = F.make_scene(3, 2, 40, 31, n_iterations=5, mode="mixed")
    sc["world_pos"][4] = np.nan
    scenes.append(sc)
    sc = F.make_scene(3, 2, 40, 33, n_iterations=5, mode="mixed")
    sc["e_point"][3] = 40
    sc["e_point"][5] = 1 << 30
    sc["e_point"][6] = -1
    sc["e_pose"][8] = 5
    sc["e_pose"][9] = -7
    sc["e_oct"][11] = NLEVELS
    sc["e_oct"][12] = -3
    scenes.append(sc)
    # arrays longer than the counts say: the tail (out-of-range rows, NaN) is not read
    sc = F.make_scene(3, 2, 40, 34, n_iterations=5, mode="mixed")
    padded = dict(sc)
    E = len(sc["e_point"])
    padded["e_point"] = np.r_[sc["e_point"], [1 << 29] * 5].astype(np.int32)
    padded["e_pose"] = np.r_[sc["e_pose"], [-1] * 5].astype(np.int32)
    padded["e_oct"] = np.r_[sc["e_oct"], [99] * 5].astype(np.int32)
    padded["e_xy"] = np.vstack([sc["e_xy"], np.full((5, 2), np.nan, np.float32)])
    padded["e_ur"] = np.r_[sc["e_ur"], [np.nan] * 5].astype(np.float32)
    padded["world_pos"] = np.vstack([sc["world_pos"], np.full((3, 3), np.nan, np.float32)])
    scenes.append(sc)
    return scenes, padded


def test_non_finite_points_bad_indices_and_padding(G, torch, F):
    scenes, padded = odd_scenes()
    sc, E = scenes[2], len(scenes[2]["e_point"])
    ups = [F.upload(torch, s) for s in scenes[:2]]
    pp, pd = F.upload(torch, padded)
    pp.update(n_edges=E, n_points=40)
    G.bundle_adjustment_batch_device([u[0] for u in ups] + [pp], stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = [F.download(u[1], s) for u, s in zip(ups, scenes[:2])] + [F.download(pd, sc)]
    rep = _check(F, "non-finite, out of range, padded", scenes, got, 3)
    assert rep["compared"] == 3
    assert got[1][1]["n_bad_index"] == 7 and got[1][1]["n_edges"] == len(scenes[1]["e_point"]) - 7
    # beyond the counts nothing was written
    assert (pd["not_included"].cpu().numpy()[40:] == F.SENTINEL).all() and (pd["pos"].cpu().numpy()[40:] == F.SENTINEL).all()
    # the NaN point makes chi2, and with it rho, NaN: every trial is rejected (L5) and the input comes back
    _, r, a = got[0]
    m = F.reference(scenes[0], 3)[0]
    assert r["trials"] == len(m["trace"]) >= 1 and not any(m["trace"])
    assert np.isnan(a["pos_d"][4]).all() and np.isfinite(np.delete(a["pos_d"], 4, axis=0)).all() and np.isfinite(a["Tcw_d"]).all()
    assert np.array_equal(np.delete(a["pos"], 4, axis=0), np.delete(scenes[0]["world_pos"], 4, axis=0))


def test_fuzz_slice(G, F):
    # a fixed number of rounds, about five seconds of the model: the same eight maps on every machine, whatever its load
    tot = F.run(None, 20263, batch=4, rounds=2)
    print("fuzz slice: %r" % {k: v for k, v in tot.items() if k != "mismatches"})
    assert tot["rounds"] == 2 and tot["compared"] > 0 and not tot["mismatches"], tot["mismatches"][:10]
    assert tot["left_out"] <= F.LEFT_OUT_CAP * (tot["compared"] + tot["left_out"])
