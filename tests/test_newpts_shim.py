"""orbgpu_shim::CreateNewMapPointsT (orb_slam2_map_amd/shim/orbgpu_shim.hpp) against tests/newpts_model.py without a device:
it compiles with -Werror against stand-ins with the reference's members (tests/integration/newpts_standin.hpp), INTEGRATION.md's
block compiles, the host part (baseline test, stop, epipole, cos_stereo, the problem it hands over) is the model's, and the
write-back over the model's outputs leaves the reference's object graph: observations in order, both key frames'
associations, the second point overwriting the first on a shared key point of key frame 2."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "orb_slam2_map_amd")
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import newpts_model as M  # noqa: E402

STRICT = ["-std=c++17", "-Wall", "-Wextra", "-Werror"]
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "shim"), "-I" + os.path.join(HERE, "integration")]


def snippet():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"<!-- newpts-snippet -->\s*```cpp\n(.*?)```", text, re.S)
    assert m, "INTEGRATION.md has no newpts-snippet block"
    return m.group(1)


def build(tmp, name):
    """tests/<name>.cpp with INTEGRATION.md's block as newpts_block.inc"""
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(PKG, "liborbgpu.so")):
        ge.build()
    with open(os.path.join(str(tmp), "newpts_block.inc"), "w") as f:
        f.write(snippet())
    out = os.path.join(str(tmp), name)
    cmd = ["g++"] + STRICT + ["-O1"] + INC + ["-I" + str(tmp), "-I" + HERE, os.path.join(HERE, name + ".cpp"), "-o", out, "-L" + PKG,
                                              "-lorbgpu", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-pthread"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("newpts_shim"), "newpts_shim_test")


def test_shim_programs_compile(exe, tmp_path):
    gpu_exe = build(tmp_path, "newpts_shim_gpu_test")
    for e in (exe, gpu_exe):
        r = subprocess.run([e], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 2 and "usage" in r.stderr


def test_integration_block_compiles(tmp_path):
    src = tmp_path / "newpts_block.cc"
    src.write_text('#include <cstring>\n#include "newpts_standin.hpp"\n' + snippet())
    r = subprocess.run(["g++"] + STRICT + ["-c"] + INC + [str(src), "-o", str(tmp_path / "newpts_block.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]


# ---- the scene file of tests/newpts_shim_test.cpp ------------------------------------------------------------------------
def shim_scene(mono=False):
    """The mixed parity scene with what the host part has to get right: a neighbour too close to pass :244-261 in second
    place, and two key points of key frame 1 that share a key point of key frame 2.  Returns (frames in the covisibility
    order, indices of the neighbours the reference keeps)."""
    sc = M.scene("mono" if mono else "mixed/raw")  # mixed/raw: mvKeys differ from mvKeysUn
    m = M.run(sc)
    i = int(np.nonzero(m["status"][0] > 0)[0][0])
    spare = int(np.nonzero((m["match12"] < 0).all(0) & (np.arange(m["match12"].shape[1]) != i))[0][0])
    for k in ("kp_x", "kp_y", "kp_octave", "kp_angle", "u_right", "desc", "has_mp", "node", "depth", "cos_stereo", "kp_raw"):
        if sc["kf1"][k] is not None:
            sc["kf1"][k][spare] = sc["kf1"][k][i]
    close = dict(sc["neighbours"][0])
    close["Twc"] = np.array(close["Twc"], np.float32).copy()
    close["median_depth"] = 8.0
    if mono:
        close["median_depth"] = 1e4  # baseline / median depth < 0.01
    else:
        close["Twc"][[3, 7, 11]] = np.asarray(sc["kf1"]["Twc"], np.float32)[[3, 7, 11]] + np.float32([0.01, 0.02, 0.0])
    nbs = [sc["neighbours"][0], close] + sc["neighbours"][1:]
    return sc, nbs, [0, 2, 3]


def write_scene(path, sc, nbs, kept, mono, stop, out):
    def frame(f, fh):
        n = len(f["kp_x"])
        nl = len(f["level_sigma2"])
        fx, fy, cx, cy = (np.float32(v) for v in f["K"])
        np.array([n, nl], np.int32).tofile(fh)
        np.array([M.MB, M.SCALE_FACTOR], np.float32).tofile(fh)
        np.array([fx, fy, cx, cy, np.float32(1) / fx, np.float32(1) / fy, f["mbf"]], np.float32).tofile(fh)
        np.asarray(f["Tcw"], np.float32).tofile(fh)
        np.asarray(f["Twc"], np.float32).tofile(fh)
        np.array([f.get("median_depth", 8.0)], np.float32).tofile(fh)
        np.asarray(f.get("F12", np.zeros(9)), np.float32).tofile(fh)
        np.asarray(f["level_sigma2"], np.float32).tofile(fh)
        np.asarray(f["scale_factors"], np.float32).tofile(fh)
        for k, t in (("kp_x", np.float32), ("kp_y", np.float32), ("kp_octave", np.int32), ("kp_angle", np.float32),
                     ("u_right", np.float32), ("depth", np.float32)):
            np.asarray(f[k], t).tofile(fh)
        raw = f.get("kp_raw")  # mvKeys; None: no distortion, mvKeys = mvKeysUn
        (np.column_stack([f["kp_x"], f["kp_y"]]) if raw is None else np.asarray(raw)).astype(np.float32).tofile(fh)
        np.asarray(f["node"], np.int32).tofile(fh)
        np.asarray(f["has_mp"], np.int32).tofile(fh)
        np.asarray(f["desc"], np.uint8).tofile(fh)
    with open(path, "wb") as fh:
        np.array([1 + len(nbs), int(mono), int(stop)], np.int32).tofile(fh)
        frame(sc["kf1"], fh)
        for f in nbs:
            frame(f, fh)
        if out is not None:
            np.array([len(kept)], np.int32).tofile(fh)
            for k in ("match12", "status", "x3d"):
                np.ascontiguousarray(out[k][:len(kept)]).tofile(fh)


def expected_graph(sc, nbs, kept, out):
    """the object graph :434-449 leaves, from the outputs: points in creation order, what every key frame holds"""
    holds = [np.where(np.asarray(f["has_mp"]) != 0, -2, -1).tolist() for f in [sc["kf1"]] + nbs]
    points = []
    for k in range(len(kept)):
        for i in np.nonzero(out["status"][k] > 0)[0]:
            j = int(out["match12"][k][i])
            holds[0][i] = holds[1 + kept[k]][j] = len(points)
            points.append((out["x3d"][k][i], [(0, int(i)), (1 + kept[k], j)]))
    return points, holds


def parse(path):
    rec = {"point": [], "holds": {}, "neighbour": {}, "row": []}
    for line in open(path):
        w = line.split()
        if w[0] == "point":
            o = w.index("obs")
            c = w.index("calls")
            rec["point"].append({"id": int(w[1]), "x": np.float32(w[2:5]), "ref": int(w[6]),
                                 "obs": [tuple(int(v) for v in t.split(":")) for t in w[o + 1:c]], "calls": [int(v) for v in w[c + 1:]]})
        elif w[0] == "row":
            rec["row"].append({"id": int(w[1]), "pos": np.float32(w[2:5]), "normal": np.float32(w[5:8]), "min": np.float32(w[8]),
                               "max": np.float32(w[9]), "desc": (int(w[10]), int(w[11])), "obs": int(w[12]), "bad": int(w[13])})
        elif w[0] == "holds":
            rec["holds"][int(w[1])] = [int(v) for v in w[2:]]
        elif w[0] == "neighbour":
            rec["neighbour"][int(w[1])] = {"ex": float(w[2]), "ey": float(w[3]), "n": int(w[4]), "nlevels": int(w[5]),
                                           "rows": np.array(w[6:], np.float64).reshape(-1, 4)}
        else:
            rec[w[0]] = w[1:]
    return rec


def check_graph(rec, sc, nbs, kept, out):
    points, holds = expected_graph(sc, nbs, kept, out)
    assert len(rec["point"]) == len(points) and [int(v) for v in rec["recent"]] == list(range(len(points)))
    for n, (got, (x, obs)) in enumerate(zip(rec["point"], points)):
        assert got["id"] == n and got["ref"] == 0
        assert got["x"].tobytes() == np.float32(x).tobytes()
        assert got["obs"] == obs  # the current key frame first, then the neighbour
        assert got["calls"] == [1, 1, 1]  # one ComputeDistinctiveDescriptors, after both AddMapPoint, one UpdateNormalAndDepth
    for k, h in enumerate(holds):
        assert rec["holds"][k] == h, k
    return points, holds


@pytest.mark.parametrize("mono,stop", [(False, False), (True, False), (False, True)])
def test_host_part_and_write_back_agree_with_the_model(exe, tmp_path, mono, stop):
    sc, nbs, kept = shim_scene(mono)
    if stop:
        kept = kept[:1]
    msc = dict(sc, neighbours=[nbs[k] for k in kept], check_ori=False, only_stereo=False)
    out = M.run(msc)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.txt")
    write_scene(src, sc, nbs, kept, mono, stop, out)
    r = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    rec = parse(dst)
    # the host part
    assert [int(v) for v in rec["kept"]] == [1 + k for k in kept]
    nn, only_stereo, check_ori, ratio, n1 = rec["problem"]
    assert (int(nn), int(only_stereo), int(check_ori), int(n1)) == (len(kept), 0, 0, len(sc["kf1"]["kp_x"]))
    assert np.float32(ratio) == np.float32(1.5) * np.float32(M.SCALE_FACTOR)
    for k in kept:
        f, got = nbs[k], rec["neighbour"][1 + k]
        assert got["n"] == len(f["kp_x"]) and got["nlevels"] == M.NLEVELS
        # the epipole: the shim's float expression against the scene's FP64 one
        for a, b in ((got["ex"], float(f["ex"])), (got["ey"], float(f["ey"]))):
            assert abs(a - b) <= 2e-3 * max(1.0, abs(b)), (a, b)
        rows = got["rows"]
        stereo = np.asarray(f["u_right"]) >= 0
        assert (np.abs(rows[stereo, 0] - np.asarray(f["cos_stereo"], np.float64)[stereo]) <= 2 * M.EPS32).all()  # float cos / atan2
        assert np.array_equal(rows[:, 1], np.asarray(f["has_mp"])) and np.array_equal(rows[:, 2], np.asarray(f["node"]))
        raw_x = f["kp_x"] if f.get("kp_raw") is None else np.asarray(f["kp_raw"])[:, 0]
        assert np.array_equal(np.float32(rows[:, 3]), np.asarray(raw_x, np.float32))  # kp_raw is mvKeys, not mvKeysUn
        if not mono:
            assert not np.array_equal(np.asarray(raw_x, np.float32), np.asarray(f["kp_x"], np.float32))
    # the write-back
    points, holds = check_graph(rec, sc, nbs, kept, out)
    assert int(rec["nnew"][0]) == len(points) == int(out["n_created"].sum()) > 20
    # two points of key frame 1 on one key point of key frame 2: both exist, the neighbour holds the second
    pairs = [(obs[1], n) for n, (_, obs) in enumerate(points)]
    shared = [t for t in set(p for p, _ in pairs) if sum(p == t for p, _ in pairs) > 1]
    assert shared
    kf, j = shared[0]
    assert holds[kf][j] == max(n for p, n in pairs if p == (kf, j))
