"""OptimizerT::OptimizeEssentialGraph (orb_slam2_map_amd/shim/orbgpu_shim.hpp): it compiles with -Werror against stand-ins with
the reference's members (tests/integration/eg_standin.hpp), INTEGRATION.md's block compiles, the graph over a hand-built
map gives the rows, states, edges and point rows that Optimizer.cc:796-983 and :1013-1032 gather -- restated here over the
same map, with the minFeat skip, the pCurKF / pLoopKF exception, sInsertedEdges, the parent / child / loop-edge exclusions and
the mnId < rule each exercised -- and on a device the whole call gives what the library gives on those arrays, written back
as :992-1043."""
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

import eg_model as M  # noqa: E402

STRICT = ["-std=c++17", "-Wall", "-Wextra", "-Werror"]
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "shim"), "-I" + os.path.join(HERE, "integration")]
MIN_FEAT = 100


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
    return _build(tmp_path_factory, "eg_shim_test")


@pytest.fixture(scope="module")
def gpu_exe(tmp_path_factory):
    return _build(tmp_path_factory, "eg_shim_gpu_test")


def test_eg_shim_programs_compile(exe, gpu_exe):
    for e in (exe, gpu_exe):
        r = subprocess.run([e], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 2 and "usage" in r.stderr


def test_integration_eg_block_compiles(tmp_path):
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"<!-- eg-snippet -->\s*```cpp\n(.*?)```", text, re.S)
    assert m, "INTEGRATION.md has no eg-snippet block"
    assert "OptimizeEssentialGraph" in m.group(1) and "LoopClosing.cc:565" in m.group(1)
    src = tmp_path / "eg_block.cc"
    src.write_text('#include <cstring>\n#include "eg_standin.hpp"\n' + m.group(1))
    r = subprocess.run(["g++"] + STRICT + ["-c"] + INC + [str(src), "-o", str(tmp_path / "eg_block.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]


# ---- the hand-built map ----------------------------------------------------------------------------------------------------
IDS = [0, 2, 3, 5, 8, 9, 11, 14, 15, 20]   # mnId of key frame idx 0..9: never the index itself
CUR, LOOP, BAD = 9, 1, 6


def make_map(fix_scale):
    sc = M.make_scene(10, 500 + fix_scale, fix_scale=fix_scale, n_corrected=2, compose=True, rot_drift=0.08, trans_drift=0.4)
    kfs = []
    for k in range(10):
        kfs.append({"id": IDS[k], "bad": k == BAD, "parent": -1 if k == 0 else (5 if k == 7 else k - 1),
                    "Tcw": M.tiw_of(sc["Snc"][k:k + 1])[0], "children": [], "loops": [], "cov": []})
    for k, kf in enumerate(kfs):
        if kf["parent"] >= 0:
            kfs[kf["parent"]]["children"].append(k)

    def cov(a, b, w):  # symmetric weights; every list is sorted by weight below
        kfs[a]["cov"].append((b, w))
        kfs[b]["cov"].append((a, w))
    for k in range(1, 10):
        cov(k, kfs[k]["parent"], 220 + k)      # the spanning tree is strongly covisible: parent and child exclusions
    cov(9, 1, 30)     # pCurKF - pLoopKF below minFeat: the loop connection is kept all the same (:868)
    cov(9, 2, 150)    # a loop connection, then a covisibility edge that sInsertedEdges has already (:953)
    cov(9, 0, 40)     # a loop connection below minFeat: skipped
    cov(8, 1, 120)    # a loop connection of a neighbour of pCurKF: kept
    cov(8, 2, 99)     # one short of minFeat: skipped
    cov(3, 1, 130)    # covisibility edge 3 -> 1 (mnId 2 < 5); from key frame 1's side the mnId < rule drops it
    cov(5, 0, 180)    # strongly covisible AND a loop edge: the loop edge is kept, the covisibility edge excluded (:945)
    cov(5, 3, 150)    # covisibility edge 5 -> 3: key frame 3 is neither parent nor child of 5
    cov(9, 7, 110)    # covisibility edge 9 -> 7
    cov(9, 6, 300)    # a bad neighbour: skipped (:947)
    cov(4, 9, 60)     # below minFeat: GetCovisiblesByWeight does not return it
    kfs[5]["loops"], kfs[0]["loops"] = [0], [5]   # an old loop: the edge belongs to the younger key frame (:919)
    for kf in kfs:
        kf["cov"].sort(key=lambda c: -c[1])
    rng = np.random.default_rng(9)
    mps = []
    for m in range(9):
        mps.append({"id": 100 + 3 * m, "bad": m == 4, "ref": [BAD, 2, 3, LOOP, 0, 7, 4, 5, 8][m], "by": 0, "cref": 0,
                    "pos": rng.normal(0, 3, 3).astype(np.float32)})
    # point 0: its reference key frame (the bad one) has no row
    mps[1].update(by=IDS[CUR], cref=IDS[8], ref=2)            # corrected by pCurKF: through mnCorrectedReference
    mps[2].update(by=IDS[CUR], cref=999, ref=3)               # ... which names no key frame of the map
    mps[3].update(by=IDS[7], cref=IDS[8], ref=LOOP)           # corrected by another key frame: through its reference key frame
    return {"kfs": kfs, "mps": mps, "cur": CUR, "loop": LOOP, "fix_scale": bool(fix_scale),
            "non_corrected": {8: sc["Snc"][8], 9: sc["Snc"][9]}, "corrected": {8: sc["Scw"][8], 9: sc["Scw"][9]},
            "connections": {9: [0, 1, 2], 8: [1, 2]}}


def write_map(mp, path):
    hexd = lambda v: float(v).hex()  # noqa: E731
    out = ["%d %d" % (len(mp["kfs"]), len(mp["mps"]))]
    for kf in mp["kfs"]:
        out.append(" ".join([str(kf["id"]), str(int(kf["bad"])), str(kf["parent"])] + [hexd(v) for v in np.ravel(kf["Tcw"])] +
                            [str(len(kf["children"]))] + [str(c) for c in kf["children"]] +
                            [str(len(kf["loops"]))] + [str(c) for c in kf["loops"]] +
                            [str(len(kf["cov"]))] + ["%d %d" % c for c in kf["cov"]]))
    for m in mp["mps"]:
        out.append(" ".join([str(m["id"]), str(int(m["bad"])), str(m["ref"]), str(m["by"]), str(m["cref"])] + [hexd(v) for v in m["pos"]]))
    out.append("%d %d %d" % (mp["cur"], mp["loop"], int(mp["fix_scale"])))
    for poses in (mp["non_corrected"], mp["corrected"]):
        out.append(" ".join([str(len(poses))] + ["%d %s" % (k, " ".join(hexd(v) for v in S)) for k, S in sorted(poses.items())]))
    out.append(" ".join([str(len(mp["connections"]))] + ["%d %d %s" % (k, len(v), " ".join(str(j) for j in v))
                                                         for k, v in sorted(mp["connections"].items())]))
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


def gather(mp):
    """Optimizer.cc:796-983 and :1013-1032 over the map dict: what the call hands to the library.  Sets of key frames are
    walked in index order (the stand-ins lie in one array, so that is their pointer order)."""
    kfs = mp["kfs"]
    rows = [k for k, kf in enumerate(kfs) if not kf["bad"]]
    row_of_id = {kfs[k]["id"]: r for r, k in enumerate(rows)}
    row = lambda k: row_of_id.get(kfs[k]["id"], -1)  # noqa: E731
    weight = lambda a, b: dict(kfs[a]["cov"]).get(b, 0)  # noqa: E731
    Scw = np.stack([mp["corrected"][k] if k in mp["corrected"] else M.state_from_pose(kfs[k]["Tcw"]) for k in rows])
    Snc = np.stack([mp["non_corrected"][k] if k in mp["non_corrected"] else Scw[r] for r, k in enumerate(rows)])
    edges, inserted = [], set()
    for k in sorted(mp["connections"]):
        for j in sorted(mp["connections"][k]):
            if (k != mp["cur"] or j != mp["loop"]) and weight(k, j) < MIN_FEAT:
                continue
            edges.append((row(k), row(j), 0))
            inserted.add((min(kfs[k]["id"], kfs[j]["id"]), max(kfs[k]["id"], kfs[j]["id"])))
    for k, kf in enumerate(kfs):
        if kf["parent"] >= 0:
            edges.append((row(k), row(kf["parent"]), 1))
        for l in sorted(kf["loops"]):
            if kfs[l]["id"] < kf["id"]:
                edges.append((row(k), row(l), 1))
        for n, w in kf["cov"]:
            if w < MIN_FEAT or n == kf["parent"] or n in kf["children"] or n in kf["loops"]:
                continue
            if kfs[n]["bad"] or not kfs[n]["id"] < kf["id"]:
                continue
            if (min(kf["id"], kfs[n]["id"]), max(kf["id"], kfs[n]["id"])) in inserted:
                continue
            edges.append((row(k), row(n), 1))
    points = [m for m, p in enumerate(mp["mps"]) if not p["bad"]]
    refs = [row_of_id.get(mp["mps"][m]["cref"], -1) if mp["mps"][m]["by"] == kfs[mp["cur"]]["id"] else row(mp["mps"][m]["ref"])
            for m in points]
    fixed = np.array([k == mp["loop"] for k in rows], np.uint8)
    return {"rows": rows, "Scw": Scw, "Snc": Snc, "fixed": fixed, "edge_i": np.int32([e[0] for e in edges]),
            "edge_j": np.int32([e[1] for e in edges]), "edge_kind": np.int32([e[2] for e in edges]), "points": points,
            "point_ref": np.int32(refs), "world_pos": np.stack([mp["mps"][m]["pos"] for m in points]),
            "fix_scale": mp["fix_scale"], "n_iterations": 20}


def test_the_hand_built_map_exercises_every_rule():
    g = gather(make_map(False))
    r = {k: i for i, k in enumerate(g["rows"])}
    e = list(zip(g["edge_i"].tolist(), g["edge_j"].tolist(), g["edge_kind"].tolist()))
    assert BAD not in g["rows"] and len(g["rows"]) == 9 and g["fixed"].tolist() == [k == LOOP for k in g["rows"]]
    assert e[:3] == [(r[8], r[1], 0), (r[9], r[1], 0), (r[9], r[2], 0)]      # 8-2, 9-0 fall to minFeat; 9-1 is the exception
    assert (r[9], r[0], 0) not in e and (r[8], r[2], 0) not in e
    assert (r[5], r[0], 1) in e and e.count((r[5], r[0], 1)) == 1 and (r[0], r[5], 1) not in e   # the loop edge, once
    assert (r[3], r[1], 1) in e and (r[1], r[3], 1) not in e                    # mnId <
    assert (r[5], r[3], 1) in e and (r[9], r[7], 1) in e
    assert (r[9], r[2], 1) not in e                                            # sInsertedEdges
    assert sum(1 for a in e if a[2] == 1 and a[:2] == (r[3], r[2])) == 1        # the parent: its tree edge, no covisibility edge
    assert (r[2], r[3], 1) not in e and (r[4], r[9], 1) not in e and (r[9], r[4], 1) not in e   # child; below minFeat
    assert (-1, r[5], 1) in e and sum(1 for a in e if -1 in a[:2]) == 1         # the bad key frame's tree edge: row -1
    assert len(e) == 3 + 9 + 1 + 3
    assert g["points"] == [0, 1, 2, 3, 5, 6, 7, 8] and g["point_ref"][:5].tolist() == [-1, r[8], -1, r[LOOP], r[7]]
    m = M.essential_graph(g)
    assert m["n_bad_index"] == 1 and m["n_bad_ref"] == 2 and m["n_free_active"] == 8 and m["chi2_end"] < m["chi2_start"]


def _read(path):
    t = open(path).read().split()
    at = [0]

    def take(n, conv):
        v = [conv(x) for x in t[at[0]:at[0] + n]]
        at[0] += n
        return v
    V, E, npts, fs, n_it = take(5, int)
    out = {"V": V, "E": E, "M": npts, "fix_scale": fs, "n_iterations": n_it, "rows": take(V, int), "fixed": take(V, int)}
    out["Scw"] = np.array(take(8 * V, float.fromhex)).reshape(V, 8)
    out["Snc"] = np.array(take(8 * V, float.fromhex)).reshape(V, 8)
    for k in ("edge_i", "edge_j", "edge_kind"):
        out[k] = take(E, int)
    out["points"], out["point_ref"] = take(npts, int), take(npts, int)
    out["world_pos"] = np.array(take(3 * npts, float.fromhex), np.float32).reshape(npts, 3)
    assert at[0] == len(t)
    return out


@pytest.mark.parametrize("fix_scale", [False, True])
def test_the_gathered_problem_equals_the_restatement(exe, tmp_path, fix_scale):
    mp = make_map(fix_scale)
    g = gather(mp)
    inp, out = tmp_path / "in.txt", tmp_path / "out.txt"
    write_map(mp, str(inp))
    r = subprocess.run([exe, str(inp), str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0 and "eg shim ok" in r.stdout, r.stdout
    o = _read(str(out))
    assert (o["V"], o["E"], o["M"], o["fix_scale"], o["n_iterations"]) == (9, len(g["edge_i"]), 8, int(fix_scale), 20)
    assert o["rows"] == g["rows"] and o["fixed"] == g["fixed"].tolist()
    assert o["Scw"].tobytes() == g["Scw"].tobytes() and o["Snc"].tobytes() == g["Snc"].tobytes()
    for k in ("edge_i", "edge_j", "edge_kind", "point_ref"):
        assert o[k] == g[k].tolist(), k
    assert o["points"] == g["points"] and o["world_pos"].tobytes() == g["world_pos"].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("fix_scale", [False, True])
def test_shim_end_to_end_equals_the_library_on_the_gathered_arrays(gpu_exe, tmp_path, fix_scale):
    from orb_slam2_map_amd import lib as G
    if G.device_count() < 1:
        pytest.skip("no HIP device")
    import fuzz_eg as F
    mp = make_map(fix_scale)
    g = gather(mp)
    inp, out = tmp_path / "in.txt", tmp_path / "out.bin"
    write_map(mp, str(inp))
    r = subprocess.run([gpu_exe, str(inp), str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "eg shim ok" in r.stdout, r.stdout
    buf = out.read_bytes()
    n = C.sizeof(G.EssentialGraphResult)
    res = G.EssentialGraphResult.from_buffer_copy(buf[:n]).as_dict()
    kf = np.frombuffer(buf[n:n + 68 * 10], np.uint8).reshape(10, 68)
    at = n + 68 * 10
    pt = np.frombuffer(buf[at:at + 16 * 9], np.uint8).reshape(9, 16)
    table = np.frombuffer(buf[at + 16 * 9:], np.float32).reshape(9, 3)
    Siw, Tiw, pos, ref = G.essential_graph(F.to_problem(g), world_pos=g["world_pos"], point_ref=g["point_ref"])
    assert res == ref and res["n_bad_index"] == 1 and res["n_bad_ref"] == 2 and res["stopped"] == 0 and res["iterations"] >= 1
    for k in range(10):  # SetPose of every row, once, and of nothing else
        T, calls = kf[k, :64].copy().view(np.float32).reshape(4, 4), int(kf[k, 64:].copy().view(np.int32)[0])
        if k in g["rows"]:
            assert calls == 1 and np.array_equal(T, Tiw[g["rows"].index(k)]), k
        else:
            assert calls == 0 and np.array_equal(T, mp["kfs"][k]["Tcw"].reshape(4, 4)), k
    for m in range(9):  # SetWorldPos + UpdateNormalAndDepth of every point with a row; the table follows
        x, calls = pt[m, :12].copy().view(np.float32), int(pt[m, 12:].copy().view(np.int32)[0])
        j = g["points"].index(m) if m in g["points"] else -1
        moved = j >= 0 and g["point_ref"][j] >= 0
        want = pos[j] if moved else mp["mps"][m]["pos"]
        assert calls == int(moved) and np.array_equal(x, want) and np.array_equal(table[m], want), m
