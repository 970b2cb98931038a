"""OptimizerT::BundleAdjustment / GlobalBundleAdjustemnt (orb_slam2_map_amd/shim/orbgpu_shim.hpp) against tests/ba_model.py:
it compiles with -Werror against stand-ins with the reference's members (tests/integration/ba_standin.hpp), INTEGRATION.md's
block compiles, the graph over an injected map gives the rows and edge arrays of ba_model.gather_all (Optimizer.cc:68-184),
and on a device the whole call gives what the library gives on the model's arrays, written back as :190-235."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "orb_slam2_map_amd")
for p in (HERE, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ba_model as B  # noqa: E402
from test_lba_shim import Reader, make_map, write_map  # noqa: E402

STRICT = ["-std=c++17", "-Wall", "-Wextra", "-Werror"]
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "shim"), "-I" + os.path.join(HERE, "integration")]


def _build(tmp_path_factory, name):
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(PKG, "liborbgpu.so")):
        ge.build()
    out = str(tmp_path_factory.mktemp(name) / name)
    cmd = ["g++"] + STRICT + ["-O1"] + INC + [os.path.join(HERE, name + ".cpp"), "-o", out, "-L" + PKG, "-lorbgpu",
                                              "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-pthread"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory, "ba_shim_test")


@pytest.fixture(scope="module")
def gpu_exe(tmp_path_factory):
    return _build(tmp_path_factory, "ba_shim_gpu_test")


def test_ba_shim_programs_compile(exe, gpu_exe):
    for e in (exe, gpu_exe):
        r = subprocess.run([e], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 2 and "usage" in r.stderr


def test_integration_ba_block_compiles(tmp_path):
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"<!-- ba-snippet -->\s*```cpp\n(.*?)```", text, re.S)
    assert m, "INTEGRATION.md has no ba-snippet block"
    assert "GlobalBundleAdjustemnt" in m.group(1) and "Tracking.cc:963" in m.group(1) and "LoopClosing.cc:647" in m.group(1)
    src = tmp_path / "ba_block.cc"
    src.write_text('#include <cstring>\n#include "ba_standin.hpp"\n' + m.group(1))
    r = subprocess.run(["g++"] + STRICT + ["-c"] + INC + [str(src), "-o", str(tmp_path / "ba_block.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]


def make_full_map(seed, mode="mixed", kf0=True):
    """The map of test_lba_shim.make_map handed to BundleAdjustment, with what its graph has to get right: a bad key frame
    that still observes points (BAD), a bad point, an observer whose mnId is above maxKFid (the lone camera, given the largest
    id and left out of vpKFs), an observer that is not in vpKFs although its id is within maxKFid (the last fixed camera of
    the scene), and a point whose only observers are skipped (the far point, seen by a key frame whose id is raised above
    maxKFid as well).  vpKFs and vpMP arrive in a seeded order of their own.  Returns (map, vp_kfs, vp_mps, scene, names)."""
    mp, sc = make_map(seed, mode, kf0)
    rng = np.random.default_rng(seed + 1)
    kfs, mps = mp["kfs"], mp["mps"]
    npts = len(sc["world_pos"])
    bad = next(k for k, kf in enumerate(kfs) if kf["bad"])
    far_mp = npts + 1
    far = next(iter(mps[far_mp]["obs"]))
    lone = next(k for k, kf in enumerate(kfs) if not kf["bad"] and k != far and sum(1 for m in mps if k in m["obs"]) == 1)
    kfs[lone]["id"], kfs[far]["id"] = 900, 901
    inside = [k for k in range(len(kfs)) if k not in (lone, far)]
    # the scene's last fixed camera: in the map's observations, within maxKFid, but not handed in
    absent = next(k for k in inside if np.array_equal(kfs[k]["Tcw"], sc["Tcw"][len(sc["Tcw"]) - 1]) and not kfs[k]["bad"]
                  and np.array_equal(kfs[k]["K"], sc["cam"][len(sc["Tcw"]) - 1]))
    low = min((k for k in inside if kfs[k]["id"] > 0), key=lambda k: kfs[k]["id"])  # its id is within maxKFid whatever the draw
    kfs[absent]["id"], kfs[low]["id"] = kfs[low]["id"], kfs[absent]["id"]
    vp_kfs = [int(k) for k in rng.permutation([k for k in inside if k != absent])]
    vp_mps = [int(m) for m in rng.permutation(len(mps))]
    return mp, vp_kfs, vp_mps, sc, dict(bad=bad, lone=lone, far=far, far_mp=far_mp, absent=absent, bad_mp=npts)


def write_rows(vp_kfs, vp_mps, path):
    with open(path, "wb") as f:
        f.write(np.array([len(vp_kfs)] + vp_kfs + [len(vp_mps)] + vp_mps, np.int32).tobytes())


@pytest.mark.parametrize("seed,mode,kf0", [(61, "mixed", True), (62, "stereo", False)])
def test_rows_and_edge_arrays_equal_the_models_gather_all(exe, tmp_path, seed, mode, kf0):
    mp, vp_kfs, vp_mps, sc, who = make_full_map(seed, mode, kf0)
    g = B.gather_all(mp, vp_kfs, vp_mps)
    # the map has what it was built to have
    assert who["bad"] in vp_kfs and who["bad"] not in g["kf_rows"] and who["bad_mp"] not in g["points"]
    assert g["kf_rows"] == [k for k in vp_kfs if k != who["bad"]] and g["points"] == [m for m in vp_mps if m != who["bad_mp"]]
    assert g["max_kf_id"] < 900 and who["lone"] not in g["edge_kf"] and who["far"] not in g["edge_kf"] and who["bad"] not in g["edge_kf"]
    assert int(g["fixed"].sum()) == int(kf0)
    n_absent = sum(1 for k in g["edge_kf"] if k == who["absent"])
    assert n_absent >= 1 and int((g["e_pose"] == -1).sum()) == n_absent and (g["e_oct"] == -1).sum() == 1
    far_row = g["points"].index(who["far_mp"])
    assert far_row not in g["e_point"].tolist()
    inp, rows, out = tmp_path / "in.bin", tmp_path / "rows.bin", tmp_path / "out.bin"
    write_map(mp, str(inp))
    write_rows(vp_kfs, vp_mps, str(rows))
    r = subprocess.run([exe, str(inp), str(rows), str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0 and "ba shim ok" in r.stdout, r.stdout
    rd = Reader(out.read_bytes())
    P, npts, ne, nlev, max_id, n_it, robust = (int(v) for v in rd.take(np.int32, 7))
    assert (P, npts, ne, nlev, max_id) == (len(g["kf_rows"]), len(g["points"]), len(g["e_point"]), 8, g["max_kf_id"])
    assert (n_it, robust) == (20, 0)
    assert list(rd.take(np.int32, P)) == g["kf_rows"] and list(rd.take(np.int32, npts)) == g["points"]
    assert np.array_equal(rd.take(np.int32, P), g["fixed"])
    for key in ("e_point", "e_pose", "e_oct"):
        assert np.array_equal(rd.take(np.int32, ne), g[key]), key
    assert np.array_equal(rd.take(np.float32, 2 * ne).reshape(ne, 2), g["e_xy"])
    assert np.array_equal(rd.take(np.float32, ne), g["e_ur"])
    assert np.array_equal(rd.take(np.float32, 16 * P).reshape(P, 4, 4), g["Tcw"])
    assert np.array_equal(rd.take(np.float32, 5 * P).reshape(P, 5), g["cam"])
    assert np.array_equal(rd.take(np.float32, nlev * P).reshape(P, nlev), g["inv_sigma2"])
    assert np.array_equal(rd.take(np.float32, 3 * npts).reshape(npts, 3), g["world_pos"])
    assert rd.at == len(rd.buf)
    # the model optimises the gathered problem: the far point comes back not included and unwritten
    m = B.bundle_adjustment(g, 3, robust=False)
    assert m["n_bad_index"] == n_absent + 1 and m["not_included"][far_row] == 1 and m["n_not_included"] >= 1
    assert np.array_equal(m["pos"][far_row], g["world_pos"][far_row])


@pytest.mark.gpu
@pytest.mark.parametrize("seed,mode,kf0,stop,loop_kf,robust", [(71, "mixed", True, -1, 0, 1), (72, "stereo", False, 0, 17, 0),
                                                               (73, "mono", True, 1, 0, 1), (74, "mixed", True, 1, 5, 0)])
def test_shim_end_to_end_equals_the_library_on_the_models_arrays(gpu_exe, tmp_path, seed, mode, kf0, stop, loop_kf, robust):
    from orb_slam2_map_amd import lib as G
    if G.device_count() < 1:
        pytest.skip("no HIP device")
    import fuzz_ba as F
    mp, vp_kfs, vp_mps, sc, who = make_full_map(seed, mode, kf0)
    g = B.gather_all(mp, vp_kfs, vp_mps)
    g["n_iterations"], g["robust"] = 20, bool(robust)
    inp, rows, out = tmp_path / "in.bin", tmp_path / "rows.bin", tmp_path / "out.bin"
    write_map(mp, str(inp))
    write_rows(vp_kfs, vp_mps, str(rows))
    r = subprocess.run([gpu_exe, str(inp), str(rows), str(out), str(stop), str(loop_kf), str(robust)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "ba shim ok" in r.stdout, r.stdout
    rd = Reader(out.read_bytes())
    res = G.BundleAdjustmentResult.from_buffer_copy(rd.take(np.uint8, C.sizeof(G.BundleAdjustmentResult)).tobytes()).as_dict()
    kf_T, kf_gba, kf_mark = [], [], []
    for _ in mp["kfs"]:
        kf_T.append(rd.take(np.float32, 16).reshape(4, 4))
        kf_gba.append(rd.take(np.float32, 16).reshape(4, 4))
        kf_mark.append(int(rd.take(np.int32, 1)[0]))
    pos, pos_gba, mark, updates = [], [], [], []
    for _ in mp["mps"]:
        pos.append(rd.take(np.float32, 3))
        pos_gba.append(rd.take(np.float32, 3))
        mark.append(int(rd.take(np.int32, 1)[0]))
        updates.append(int(rd.take(np.int32, 1)[0]))
    table_pos = rd.take(np.float32, 3 * len(mp["mps"])).reshape(-1, 3)
    assert rd.at == len(rd.buf)
    # the library on the model's arrays
    Td, T, Xd, X, ni, ref = G.bundle_adjustment(F.to_problem(g), stop=None if stop < 0 else stop)
    assert res == ref
    rows_of, points_of = {k: i for i, k in enumerate(g["kf_rows"])}, {m: j for j, m in enumerate(g["points"])}
    far_row = points_of[who["far_mp"]]
    if stop == 1:  # nothing happened
        assert res["stopped"] == 1 and res["iterations"] == 0 and not any(updates) and not any(kf_mark) and not any(mark)
        for k, kf in enumerate(mp["kfs"]):
            assert np.array_equal(kf_T[k], kf["Tcw"]) and np.isnan(kf_gba[k]).all()
        for m, p in enumerate(mp["mps"]):
            assert np.array_equal(pos[m], np.asarray(p["pos"], np.float32)) and np.isnan(pos_gba[m]).all()
        return
    assert res["stopped"] == 0 and res["iterations"] >= 1 and ni[far_row] == 1 and res["n_not_included"] == int(ni.sum())
    for k, kf in enumerate(mp["kfs"]):
        if loop_kf == 0:  # SetPose of every row and of nothing else
            want = T[rows_of[k]] if k in rows_of else kf["Tcw"]
            assert np.array_equal(kf_T[k], want) and np.isnan(kf_gba[k]).all() and kf_mark[k] == 0, k
        else:  # mTcwGBA and mnBAGlobalForKF; the pose stays
            assert np.array_equal(kf_T[k], kf["Tcw"]), k
            if k in rows_of:
                assert np.array_equal(kf_gba[k], T[rows_of[k]]) and kf_mark[k] == loop_kf, k
            else:
                assert np.isnan(kf_gba[k]).all() and kf_mark[k] == 0, k
    for m, p in enumerate(mp["mps"]):
        included = m in points_of and not ni[points_of[m]]
        old = np.asarray(p["pos"], np.float32)
        if loop_kf == 0:  # SetWorldPos + UpdateNormalAndDepth of the included points; the table follows
            want = X[points_of[m]] if included else old
            assert np.array_equal(pos[m], want) and updates[m] == int(included) and np.isnan(pos_gba[m]).all() and mark[m] == 0, m
            assert np.array_equal(table_pos[m], want), m
        else:
            assert np.array_equal(pos[m], old) and updates[m] == 0 and np.array_equal(table_pos[m], old), m
            if included:
                assert np.array_equal(pos_gba[m], X[points_of[m]]) and mark[m] == loop_kf, m
            else:
                assert np.isnan(pos_gba[m]).all() and mark[m] == 0, m
    assert not (m_ := [m for m in (who["far_mp"], who["bad_mp"]) if updates[m] or mark[m]]), m_
