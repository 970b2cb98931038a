"""OptimizerT::LocalBundleAdjustment (orb_slam2_map_amd/shim/orbgpu_shim.hpp) against tests/lba_model.py: it compiles with
-Werror against stand-ins with the reference's members (tests/integration/lba_standin.hpp), INTEGRATION.md's block
compiles, the breadth-first gathering over an injected map gives the lists and edge arrays of lba_model.gather
(Optimizer.cc:455-504, :522-652), and on a device the whole call gives what the library gives on the model's arrays."""
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

import lba_model as M  # noqa: E402

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
    return _build(tmp_path_factory, "lba_shim_test")


@pytest.fixture(scope="module")
def gpu_exe(tmp_path_factory):
    return _build(tmp_path_factory, "lba_shim_gpu_test")


def test_lba_shim_programs_compile(exe, gpu_exe):
    for e in (exe, gpu_exe):
        r = subprocess.run([e], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 2 and "usage" in r.stderr


def test_integration_lba_block_compiles(tmp_path):
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"<!-- lba-snippet -->\s*```cpp\n(.*?)```", text, re.S)
    assert m, "INTEGRATION.md has no lba-snippet block"
    src = tmp_path / "lba_block.cc"
    src.write_text('#include <cstring>\n#include "lba_standin.hpp"\n' + m.group(1))
    r = subprocess.run(["g++"] + STRICT + ["-c"] + INC + [str(src), "-o", str(tmp_path / "lba_block.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]


def make_map(seed, mode="mixed", kf0=True):
    """A local map around a scene of lba_model.make_scene, with what the gathering has to get right: key frames stored in
    an order that is not the list order, KF 0 among the local key frames (kf0), a bad key frame among the neighbours that
    still observes local points, a bad map point in a local key frame, a fixed camera that sees one local point only, a
    key frame nobody reaches, key points without a map point and one observation at an octave outside the sigma table."""
    rng = np.random.default_rng(seed)
    sc = M.make_scene(3, 2, 40, seed, mode=mode, kf0_fixed=kf0, obs_frac=0.6)
    P, nl, npts = len(sc["Tcw"]), sc["n_local"], len(sc["world_pos"])
    n_kf = P + 3  # + a bad neighbour, a fixed camera behind one point, an unrelated key frame
    BAD, LONE, FAR = P, P + 1, P + 2
    slot = rng.permutation(n_kf)  # where key frame k lives: the pointer order of the observation maps
    kfs = [None] * n_kf
    ids = rng.permutation(np.arange(1, 200))[:n_kf]

    def key_frame(k, Tcw, K, sigma):
        return {"id": int(ids[k]), "bad": False, "cov": [], "K": np.asarray(K, np.float32), "Tcw": np.asarray(Tcw, np.float32),
                "inv_sigma2": np.asarray(sigma, np.float32), "kps": [], "mps": []}
    for k in range(P):
        kfs[slot[k]] = key_frame(k, sc["Tcw"][k], sc["cam"][k], sc["inv_sigma2"][k])
    for k in (BAD, LONE, FAR):
        kfs[slot[k]] = key_frame(k, sc["Tcw"][P - 1], sc["cam"][0], sc["inv_sigma2"][0])
    kfs[slot[BAD]]["bad"] = True
    if kf0:
        kfs[slot[int(np.flatnonzero(sc["fixed"])[0])]]["id"] = 0
    cur = 0 if not (kf0 and sc["fixed"][0]) else 1  # the current key frame is never KF 0
    others = [k for k in range(nl) if k != cur]
    kfs[slot[cur]]["cov"] = [int(slot[others[0]]), int(slot[BAD])] + [int(slot[k]) for k in others[1:]]
    mps = [{"id": 1000 + 3 * m, "bad": False, "pos": sc["world_pos"][m], "obs": {}} for m in range(npts)]
    mps.append({"id": 5000, "bad": True, "pos": np.float32([0, 0, 5]), "obs": {}})  # seen by a local key frame, bad
    mps.append({"id": 5001, "bad": False, "pos": np.float32([1, 0, 5]), "obs": {}})  # seen by the unrelated key frame only

    def observe(k, m, x, y, ur, octave):
        kf = kfs[slot[k]]
        if rng.random() < 0.3:  # a key point without a map point in between
            kf["kps"].append((rng.uniform(0, 600), rng.uniform(0, 400), -1.0, int(rng.integers(8))))
            kf["mps"].append(-1)
        kf["kps"].append((float(x), float(y), float(ur), int(octave)))
        kf["mps"].append(m)
        mps[m]["obs"][int(slot[k])] = len(kf["kps"]) - 1
    for e in rng.permutation(len(sc["e_point"])):
        observe(int(sc["e_pose"][e]), int(sc["e_point"][e]), sc["e_xy"][e, 0], sc["e_xy"][e, 1], sc["e_ur"][e], sc["e_oct"][e])
    for m in (2, 7, 11):
        observe(BAD, m, 100.0, 100.0, -1.0, 0)
    observe(LONE, 5, *_project(sc, P - 1, 5), -1.0, 1)
    observe(cur, npts, 50.0, 60.0, -1.0, 0)
    observe(FAR, npts + 1, 70.0, 80.0, -1.0, 0)
    first = kfs[slot[others[0]]]  # one observation at an octave the key frame has no sigma for
    kp = next(i for i, m in enumerate(first["mps"]) if m >= 0)
    first["kps"][kp] = first["kps"][kp][:3] + (8,)
    for kf in kfs:
        kf["kps"] = np.array(kf["kps"], np.float64).reshape(-1, 4)
    return {"cur": int(slot[cur]), "kfs": kfs, "mps": mps}, sc


def _project(sc, k, m):
    T, c = sc["Tcw"][k].astype(np.float64), sc["cam"][k].astype(np.float64)
    Pc = T[:3, :3] @ sc["world_pos"][m].astype(np.float64) + T[:3, 3]
    return c[0] * Pc[0] / Pc[2] + c[2], c[1] * Pc[1] / Pc[2] + c[3]


def write_map(mp, path):
    b = [np.array([len(mp["kfs"]), len(mp["mps"]), mp["cur"]], np.int32).tobytes()]
    for kf in mp["kfs"]:
        b.append(np.array([kf["id"], kf["bad"], len(kf["mps"])], np.int32).tobytes())
        b.append(kf["K"].tobytes() + kf["Tcw"].tobytes())
        b.append(np.int32(len(kf["inv_sigma2"])).tobytes() + kf["inv_sigma2"].tobytes())
        b.append(np.array([len(kf["cov"])] + kf["cov"], np.int32).tobytes())
        for (x, y, ur, octave), m in zip(kf["kps"], kf["mps"]):
            b.append(np.array([x, y, ur], np.float32).tobytes() + np.array([octave, m], np.int32).tobytes())
    for m in mp["mps"]:
        b.append(np.array([m["id"], m["bad"]], np.int32).tobytes() + np.asarray(m["pos"], np.float32).tobytes())
        b.append(np.array([len(m["obs"])] + [v for k in sorted(m["obs"]) for v in (k, m["obs"][k])], np.int32).tobytes())
    with open(path, "wb") as f:
        f.write(b"".join(b))


class Reader:
    def __init__(self, buf):
        self.buf, self.at = buf, 0

    def take(self, dtype, count):
        a = np.frombuffer(self.buf, dtype, count, self.at)
        self.at += a.nbytes
        return a


@pytest.mark.parametrize("seed,mode,kf0", [(61, "mixed", True), (62, "stereo", False)])
def test_lists_and_edge_arrays_equal_the_models_gather(exe, tmp_path, seed, mode, kf0):
    mp, sc = make_map(seed, mode, kf0)
    g = M.gather(mp)
    # the map has what it was built to have
    seen = np.unique(sc["e_point"][sc["e_pose"] < sc["n_local"]])  # a point no local key frame sees is not a local point
    of_local = np.isin(sc["e_point"], seen)
    assert g["n_local"] == sc["n_local"] and sorted(g["points"]) == list(seen) and int(g["fixed"].sum()) == int(kf0)
    assert len(seen) >= len(sc["world_pos"]) - 2 and 5 in seen
    # the scene's fixed cameras and the lone one
    assert len(g["fixed_list"]) == len(np.unique(sc["e_pose"][of_local & (sc["e_pose"] >= sc["n_local"])])) + 1
    lone = [k for k in g["fixed_list"] if sum(1 for m in g["points"] if k in mp["mps"][m]["obs"]) == 1]
    assert len(lone) >= 1 and (g["e_oct"] == -1).sum() == 1 and not (g["e_pose"] == -1).any()
    assert len(g["e_point"]) == int(of_local.sum()) + 1  # the bad key frame's three observations are no edges
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    write_map(mp, str(inp))
    r = subprocess.run([exe, str(inp), str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0 and "lba shim ok" in r.stdout, r.stdout
    rd = Reader(out.read_bytes())
    nl, nx, npts, ne, nlev = (int(v) for v in rd.take(np.int32, 5))
    assert (nl, nx, npts, ne, nlev) == (g["n_local"], len(g["fixed_list"]), len(g["points"]), len(g["e_point"]), 8)
    assert list(rd.take(np.int32, nl)) == g["local"] and list(rd.take(np.int32, nx)) == g["fixed_list"]
    assert list(rd.take(np.int32, npts)) == g["points"]
    assert np.array_equal(rd.take(np.int32, nl), g["fixed"])
    for key in ("e_point", "e_pose", "e_oct"):
        assert np.array_equal(rd.take(np.int32, ne), g[key]), key
    assert np.array_equal(rd.take(np.float32, 2 * ne).reshape(ne, 2), g["e_xy"])
    assert np.array_equal(rd.take(np.float32, ne), g["e_ur"])
    P = nl + nx
    assert np.array_equal(rd.take(np.float32, 16 * P).reshape(P, 4, 4), g["Tcw"])
    assert np.array_equal(rd.take(np.float32, 5 * P).reshape(P, 5), g["cam"])
    assert np.array_equal(rd.take(np.float32, nlev * P).reshape(P, nlev), g["inv_sigma2"])
    assert np.array_equal(rd.take(np.float32, 3 * npts).reshape(npts, 3), g["world_pos"])
    assert rd.at == len(rd.buf)
    # the gathered problem is the scene's, row for row up to the order of the lists: the model optimises it
    m = M.local_ba(g)
    assert m["n_bad_index"] == 1 and m["rounds"] == 2


@pytest.mark.gpu
@pytest.mark.parametrize("seed,mode,kf0,stop", [(71, "mixed", True, -1), (72, "stereo", False, 0), (73, "mono", True, 1)])
def test_shim_end_to_end_equals_the_library_on_the_models_arrays(gpu_exe, tmp_path, seed, mode, kf0, stop):
    from orb_slam2_map_amd import lib as G
    if G.device_count() < 1:
        pytest.skip("no HIP device")
    import fuzz_lba as F
    mp, sc = make_map(seed, mode, kf0)
    g = M.gather(mp)
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    write_map(mp, str(inp))
    r = subprocess.run([gpu_exe, str(inp), str(out), str(stop)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=120)
    assert r.returncode == 0 and "lba shim ok" in r.stdout, r.stdout
    rd = Reader(out.read_bytes())
    res = G.LocalBAResult.from_buffer_copy(rd.take(np.uint8, C.sizeof(G.LocalBAResult)).tobytes()).as_dict()
    kf_T, kf_mps = [], []
    for kf in mp["kfs"]:
        kf_T.append(rd.take(np.float32, 16).reshape(4, 4))
        kf_mps.append(rd.take(np.int32, len(kf["mps"])))
    pos, updates, obs = [], [], []
    for _ in mp["mps"]:
        pos.append(rd.take(np.float32, 3))
        updates.append(int(rd.take(np.int32, 1)[0]))
        obs.append(sorted(int(k) for k in rd.take(np.int32, int(rd.take(np.int32, 1)[0]))))
    table_pos = rd.take(np.float32, 3 * len(mp["mps"])).reshape(-1, 3)
    assert rd.at == len(rd.buf)
    # the library on the model's arrays
    Td, T, Xd, X, erase, ref = G.local_ba(F.to_problem(g), stop=None if stop < 0 else stop)
    assert res == ref
    local, points = set(g["local"]), set(g["points"])
    if stop == 1:  # Optimizer.cc:655: nothing happened
        assert res["stopped"] == 1 and res["rounds"] == 0 and not any(updates)
        for k, kf in enumerate(mp["kfs"]):
            assert np.array_equal(kf_T[k], kf["Tcw"]) and np.array_equal(kf_mps[k], kf["mps"])
        for m, p in enumerate(mp["mps"]):
            assert np.array_equal(pos[m], p["pos"]) and obs[m] == sorted(p["obs"])
        return
    assert res["rounds"] == 2 and res["stopped"] == 0 and res["n_bad_index"] == 1 and res["n_erased"] == int((erase == 1).sum()) > 0
    model = M.local_ba(g)
    assert np.array_equal(erase, np.where(model["erase"] == 255, 0, model["erase"]))
    for k, kf in enumerate(mp["kfs"]):  # SetPose of the local key frames and of nothing else
        want = T[g["local"].index(k)] if k in local else kf["Tcw"]
        assert np.array_equal(kf_T[k], want), k
    gone = {(g["edge_kf"][e], g["edge_mp"][e]) for e in np.flatnonzero(erase == 1)}
    for m, p in enumerate(mp["mps"]):  # SetWorldPos + UpdateNormalAndDepth of the local points; the table follows
        want = X[g["points"].index(m)] if m in points else np.asarray(p["pos"], np.float32)
        assert np.array_equal(pos[m], want) and updates[m] == int(m in points), m
        assert np.array_equal(table_pos[m], want), m
        assert obs[m] == sorted(k for k in p["obs"] if (k, m) not in gone), m  # EraseObservation
    for k, kf in enumerate(mp["kfs"]):  # EraseMapPointMatch
        want = [-1 if (k, int(m)) in gone else int(m) for m in kf["mps"]]
        assert list(kf_mps[k]) == want, k
