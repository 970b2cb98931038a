"""LocalMapping::CreateNewMapPoints on the device (orbgpu_create_new_map_points*) against the numpy restatement in
newpts_model.py -- vs CPU restatement; OpenCV boundary unpinned.  match12, status and the counts exactly outside the margins
the model derives from its own spread, x3d within 16 x that spread (bit for bit at spread 0), every stage on the device's own
upstream output; the chain between neighbours, the stop flag, the flavours and determinism as bytes."""
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

import newpts_model as M  # noqa: E402

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
    import fuzz_newpts
    return fuzz_newpts


_CACHE = {}


def scene_and_run(F, torch, name):
    """one device run per parity scene, shared by the tests"""
    if name not in _CACHE:
        sc = M.scene(name)
        _CACHE[name] = (sc, F.run_device(torch, sc))
    return _CACHE[name]


@pytest.mark.parametrize("name", list(M.SCENES))
def test_parity_with_the_model(G, torch, F, name):
    sc, d = scene_and_run(F, torch, name)
    _, spread, _, _ = M.model_pass(sc)
    fig = M.compare(sc, d, M.BOUND_FACTOR * spread)
    print("%s: spread %.3g, %d of %d pairs left out, x3d deviation %.3g" % (name, spread, fig["left_out"], fig["matched"],
                                                                            fig["x3d_deviation"]))
    nn, n1 = len(sc["neighbours"]), len(sc["kf1"]["kp_x"])
    assert d["match12"].shape == (nn, n1) and d["n_done"] == nn
    if name in ("mono", "stereo", "mixed"):
        assert fig["matched"] > 100 and d["n_created"].sum() > 80


def test_a_created_point_blocks_the_key_point_for_later_neighbours(G, torch, F):
    """chain 1: created at neighbour 0, so match12[1][i] == -1 although neighbour 1 holds a candidate for it"""
    sc, d = scene_and_run(F, torch, "mixed")
    kf1, nb1 = sc["kf1"], sc["neighbours"][1]
    alone, _ = M.match(kf1, kf1["has_mp"], nb1, sc["only_stereo"], False)  # neighbour 1 as if it came first
    blocked = [i for i in np.nonzero(d["status"][0] > 0)[0] if alone[i] >= 0]
    assert len(blocked) >= 10
    assert (d["match12"][1][blocked] == -1).all() and (d["status"][1][blocked] == M.NONE).all()
    assert not kf1["has_mp"][blocked].any()  # the caller's array did not say so


def test_a_rejected_key_point_is_created_at_a_later_neighbour(G, torch, F):
    """chain 2: rejected for reprojection at neighbour 0, created at neighbour 1"""
    sc, d = scene_and_run(F, torch, "stereo")
    rej = np.isin(d["status"][0], (M.REPROJ1, M.REPROJ2))
    later = rej & (d["status"][1] > 0)
    assert rej.sum() >= 3 and later.sum() >= 1
    i = int(np.nonzero(later)[0][0])
    assert d["match12"][1][i] >= 0 and d["x3d"][1][i].any() and not d["x3d"][0][i].any()


@pytest.mark.parametrize("name", ["mono", "mixed", "mixed/only_stereo"])
def test_every_neighbours_matches_are_search_for_triangulations(G, torch, F, name):
    """match12[k] is, byte for byte, orbgpu_search_for_triangulation over has_mp1 OR the statuses of neighbours < k"""
    sc, d = scene_and_run(F, torch, name)
    kf1 = sc["kf1"]

    class View:
        def __init__(self, f):
            self.f, self.n = f, len(f["kp_x"])

        def view(self):
            f, v = self.f, G.FrameView()
            v.n = self.n
            self.keep = [np.ascontiguousarray(f[k]) for k in ("kp_x", "kp_y", "kp_octave", "kp_angle", "u_right", "desc", "scale_factors")]
            v.kp_x, v.kp_y, v.kp_octave, v.kp_angle, v.u_right, v.desc, v.scale_factors = (a.ctypes.data for a in self.keep)
            v.nlevels = len(f["scale_factors"])
            return v
    has = np.array(kf1["has_mp"], np.uint8)
    for k, nb in enumerate(sc["neighbours"]):
        n, m = G.search_for_triangulation(View(kf1), has, kf1["node"], View(nb), nb["has_mp"], nb["node"], nb["F12"], float(nb["ex"]),
                                          float(nb["ey"]), nb["level_sigma2"], sc["only_stereo"], sc["check_ori"])
        assert m.tobytes() == d["match12"][k].tobytes() and n == d["n_matches"][k], k
        has = has | (d["status"][k] > 0).astype(np.uint8)


def test_flavours_and_repeated_calls_give_the_same_bytes(G, torch, F):
    for name in ("mixed", "n2=0", "n1=0"):
        sc, d = scene_and_run(F, torch, name)
        assert F.same_bytes(d, F.run_device(torch, sc)), name
        h = F.run_host(sc)
        assert F.same_bytes(d, h), name
        assert F.same_bytes(h, F.run_host(sc)), name


def test_stop_flag_set_before_the_call(G, torch, F):
    sc, d = scene_and_run(F, torch, "mixed")
    for out in (F.run_device(torch, sc, stop=1), F.run_host(sc, stop=1)):
        assert out["n_done"] == 1
        for k in F.OUT_KEYS:
            assert out[k][0].tobytes() == d[k][0].tobytes(), k
        assert (out["match12"][1:] == -1).all() and not out["status"][1:].any() and not out["x3d"][1:].any()
        assert not out["n_matches"][1:].any() and not out["n_created"][1:].any()
    assert F.same_bytes(d, F.run_device(torch, sc, stop=0)) and F.same_bytes(d, F.run_host(sc, stop=0))


def test_argument_errors_launch_nothing(G, torch, F):
    sc = M.scene("nn=1")
    torch.cuda.synchronize()
    with pytest.raises(G.OrbGpuError) as ei:
        G.create_new_map_points(sc["kf1"], [sc["neighbours"][0]] * (G.NEW_POINTS_MAX_NEIGHBOURS + 1), sc["ratio_factor"])
    assert ei.value.status == G.EINVAL
    bad = dict(sc["neighbours"][0], kp_octave=np.full(len(sc["neighbours"][0]["kp_x"]), 99, np.int32))
    with pytest.raises(G.OrbGpuError) as ei:
        G.create_new_map_points(sc["kf1"], [bad], sc["ratio_factor"])
    assert ei.value.status == G.EINVAL
    # the device flavour: outputs stay as they were
    keep = []
    out = torch.full((64,), 5, dtype=torch.int32, device="cuda")
    kf1 = F._device_frame(torch, sc["kf1"], keep)
    with pytest.raises(G.OrbGpuError) as ei:
        G.create_new_map_points_device(kf1, [F._device_frame(torch, sc["neighbours"][0], keep)], sc["ratio_factor"],
                                       n_done=out.data_ptr(), n_matches=out.data_ptr(), n_created=out.data_ptr())  # no match12
    assert ei.value.status == G.EINVAL
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 5).all()


def test_out_of_range_octaves_in_the_device_flavour_read_nothing_out_of_range(G, torch, F):
    sc = M.scene("nn=1")
    nb = dict(sc["neighbours"][0])
    nb["kp_octave"] = np.where(np.arange(len(nb["kp_x"])) % 3 == 0, 1 << 20, nb["kp_octave"]).astype(np.int32)
    kf1 = dict(sc["kf1"])
    kf1["kp_octave"] = np.where(np.arange(len(kf1["kp_x"])) % 5 == 0, -7, kf1["kp_octave"]).astype(np.int32)
    d = F.run_device(torch, dict(sc, kf1=kf1, neighbours=[nb]))
    m = d["match12"][0]
    assert not (nb["kp_octave"][m[m >= 0]] == 1 << 20).any()
    hit = (m >= 0) & (kf1["kp_octave"] == -7)
    assert hit.any() and (d["status"][0][hit] == M.BAD_OCTAVE).all()


def test_fuzz_slice(G, F):
    tot = F.run(5.0, 20271)
    print("fuzz slice: %r" % {k: v for k, v in tot.items() if k != "mismatches"})
    assert tot["scenes"] > 0 and tot["matched"] > 0 and not tot["mismatches"], tot["mismatches"][:10]
    assert tot["left_out"] <= M.LEFT_OUT_CAP * max(tot["matched"], 1)


def test_the_shim_runs_the_whole_call_once(G, tmp_path):
    """tests/newpts_shim_gpu_test.cpp: INTEGRATION.md's LocalMapping::CreateNewMapPoints over stand-ins with a MapPoint table
    attached, against the model's arrays for the neighbours the reference keeps; the table's rows are the created points"""
    import test_newpts_shim as S
    sc, nbs, kept = S.shim_scene(False)
    exe = S.build(tmp_path, "newpts_shim_gpu_test")
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.txt")
    S.write_scene(src, sc, nbs, kept, False, False, None)
    r = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:]
    out = M.run(dict(sc, neighbours=[nbs[k] for k in kept], check_ori=False, only_stereo=False))
    rec = S.parse(dst)
    points, _ = S.check_graph(rec, sc, nbs, kept, out)
    assert len(points) == int(out["n_created"].sum()) > 80
    assert {M.UNPROJECT1, M.UNPROJECT2} <= set(np.unique(out["status"]))  # the back-projections read mvKeys (N6)
    # the one batched Upsert: a row per created point with ITS position, normal, distances and descriptor
    assert int(rec["rows"][0]) == len(points) == len(rec["row"])
    for n, (row, (x, _)) in enumerate(zip(rec["row"], points)):
        assert row["id"] == n and row["pos"].tobytes() == np.float32(x).tobytes(), n
        assert row["normal"].tolist() == [0.25, -0.5, 0.75]
        assert (row["min"], row["max"]) == (np.float32(0.8), np.float32(2.4)) and row["obs"] == 1 and row["bad"] == 0
        assert row["desc"][0] == row["desc"][1]


def test_crafted_pairs_take_every_branch_on_the_device(G, torch, F):
    """the one-key-point pairs of test_newpts_model.py, every status code that can be constructed, through the device"""
    import test_newpts_model as T
    seen = set()
    for name, k1, k2, want in T.crafted_pairs():
        # the matcher must accept the pair whatever its geometry: the epipolar line x = kp_x of key frame 2, a far epipole
        k2 = dict(k2, F12=np.float32([0, 0, 0, 0, 0, 0, 1, 0, -k2["kp_x"][0]]), ex=np.float32(1e6), ey=np.float32(1e6))
        sc = {"kf1": k1, "neighbours": [k2], "ratio_factor": T.RF, "only_stereo": False, "check_ori": False}
        d = F.run_device(torch, sc)
        if want != M.BAD_OCTAVE:  # that one the host flavour refuses; the device flavour rejects the pair
            assert F.same_bytes(d, F.run_host(sc)), name
        assert d["match12"][0][0] == 0 and d["status"][0][0] == want, (name, d["status"][0][0])
        M.compare(sc, d, 0.0)  # the model's status and, where a point was created, its bytes
        seen.add(want)
    assert {M.Z1, M.Z2, M.REPROJ1, M.REPROJ2, M.NON_FINITE, M.STEREO_DEPTH, M.SCALE, M.UNPROJECT1, M.UNPROJECT2} <= seen
