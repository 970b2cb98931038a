"""CovisibilityGraphT (orb_slam2_map_amd/shim/orbgpu_shim.hpp) and INTEGRATION.md's observation-graph block (2o): they
compile with -Werror against stand-ins with the reference's members (tests/integration/covis_standin.hpp); the host-only
parts (id <-> pointer maps, marshalling, the host half of UpdateConnections) run as a stand-alone program, also under
-fsanitize=address,undefined; on the GPU the block, run over one small scene, prints the lists of tests/covis_model.py."""
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

import covis_model as M  # noqa: E402

STRICT = ["-std=c++17", "-Wall", "-Wextra", "-Werror"]
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "shim"), "-I" + os.path.join(HERE, "integration")]


def integration_block():
    """the code block of INTEGRATION.md's observation-graph section (it carries no snippet marker)"""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"^### 2o\. .*?```cpp\n(.*?)```", text, re.S | re.M)
    assert m, "INTEGRATION.md has no observation-graph block"
    return m.group(1)


def _build(tmp, name, extra=(), inc=()):
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(PKG, "liborbgpu.so")):
        ge.build()
    out = str(tmp / name)
    cmd = ["g++"] + STRICT + ["-O1"] + list(extra) + INC + list(inc) + [os.path.join(HERE, name + ".cpp"), "-o", out, "-L" + PKG,
                                                                      "-lorbgpu", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-pthread"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return out


@pytest.fixture(scope="module")
def gpu_exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("covis_gpu")
    (tmp / "covis_block.inc").write_text(integration_block())
    return _build(tmp, "covis_shim_gpu_test", inc=["-I" + str(tmp)])


@pytest.mark.parametrize("sanitize", [False, True])
def test_host_only_parts_run_stand_alone(tmp_path, sanitize):
    exe = _build(tmp_path, "covis_shim_test", extra=["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else [])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
    assert r.returncode == 2 and "usage" in r.stderr
    r = subprocess.run([exe, "run"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "covis shim ok" in r.stdout, r.stdout[-3000:]


def test_integration_block_compiles_and_the_device_program_builds(gpu_exe):
    r = subprocess.run([gpu_exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 2 and "usage" in r.stderr


def scene(seed=3, n_kf=9, n_pts=120):
    """key frames of 60 slots over 120 points (ids above 2^32): neighbours share 15 or more points, far ones a few"""
    rng = np.random.default_rng(seed)
    kfs = [(5 + 4 * i, 60) for i in range(n_kf)]
    obs = []
    for i in range(n_kf):
        lo = (i * 11) % n_pts
        window = [(lo + k) % n_pts for k in range(50)]
        pts = rng.permutation(window)[:int(rng.integers(30, 46))]
        if i == n_kf - 1:  # shares fewer than 15 points with anyone: the single best connection (KeyFrame.cc:386-390)
            pts = list(pts[:8]) + list(range(n_pts + 100, n_pts + 130))
        idxs = rng.permutation(60)[:len(pts)]
        obs += [(i, int(a), int(2 ** 33 + 7 * p)) for a, p in zip(idxs, pts)]
    by_kf = lambda i: [o[2] for o in obs if o[0] == i]  # noqa: E731
    f1 = [int(x) for x in rng.choice(by_kf(2) + by_kf(3), 50)] + [-1] * 5 + [2 ** 33 + 7 * 1000]
    f2 = [int(x) for x in rng.choice(by_kf(6) + by_kf(7), 50)] + [-1] * 3
    bad_kf = 6
    return dict(kfs=kfs, obs=obs, bad_mp=f2[0], bad_kf=bad_kf, f1=f1, f2=f2)


def scene_text(sc):
    lines = [str(len(sc["kfs"]))] + ["%d %d" % k for k in sc["kfs"]] + [str(len(sc["obs"]))] + ["%d %d %d" % o for o in sc["obs"]]
    lines.append("%d %d" % (sc["bad_mp"], sc["bad_kf"]))
    for f in (sc["f1"], sc["f2"]):
        lines.append("%d %s" % (len(f), " ".join(str(x) for x in f)))
    return "\n".join(lines) + "\n"


def model_answer(sc):
    g = M.CovisGraph()
    pm = M.PointerMap(g)
    out = {"CONN": []}
    for i, (kf_id, n) in enumerate(sc["kfs"]):
        kf = pm.AddKeyFrame(kf_id, n)
        pairs = []
        for _, idx, mp_id in (o for o in sc["obs"] if o[0] == i):
            pairs.append((idx, pm.mps[mp_id] if mp_id in pm.mps else pm.NewMapPoint(mp_id)))
        pm.AddObservations(kf, pairs)
        _, ordered, weights = pm.UpdateConnections(kf, 15)
        out["CONN"].append([kf_id, kf.mpParent.mnId if kf.mpParent else -1, len(ordered)] + [x for kw in zip(ordered, weights) for x in kw])
    lm = g.local_map(sc["f1"], [])
    out["KFS"], out["PTS"], out["REF"] = lm["kf_ids"].tolist(), lm["point_ids"].tolist(), lm["ref_kf"]
    pm.SetBadFlagMapPoint(pm.mps[sc["bad_mp"]])
    bad_id = sc["kfs"][sc["bad_kf"]][0]
    parent = g.row_of[bad_id].parent
    for c in g.children(bad_id):
        if parent >= 0:
            g.set_parent(c, parent)
    g.set_bad([bad_id])
    lm2 = g.local_map([-1 if x == sc["bad_mp"] else x for x in sc["f2"]], out["KFS"])
    out["KFS2"], out["PTS2"] = lm2["kf_ids"].tolist(), lm2["point_ids"].tolist()
    out["REF2"] = lm2["ref_kf"] if lm2["ref_kf"] >= 0 else out["REF"]
    return out


def test_the_scene_has_something_to_find():
    sc = scene()
    want = model_answer(sc)
    assert len(set(o[:2] for o in sc["obs"])) == len(sc["obs"]) == len(set((o[0], o[2]) for o in sc["obs"]))
    weights = [w for c in want["CONN"] for w in c[4::2]]
    assert any(w >= 15 for w in weights) and any(w < 15 for w in weights)  # both branches of KeyFrame.cc:379-390
    assert sum(1 for c in want["CONN"] if c[1] >= 0) == len(sc["kfs"]) - 1
    assert len(want["KFS"]) >= 3 and len(want["PTS"]) > 60 and want["REF"] in want["KFS"]
    bad_id = sc["kfs"][sc["bad_kf"]][0]
    assert want["KFS2"] != want["KFS"]
    assert sc["bad_mp"] not in want["PTS2"] and want["REF2"] != bad_id


@pytest.mark.gpu
def test_integration_block_on_the_device_equals_the_model(gpu, gpu_exe, tmp_path):
    sc = scene()
    path = tmp_path / "scene.txt"
    path.write_text(scene_text(sc))
    r = subprocess.run([gpu_exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "covis shim ok" in r.stdout and "STAMP" not in r.stdout, r.stdout[-3000:]
    want = model_answer(sc)
    lines = [l.split() for l in r.stdout.splitlines() if l.strip()]
    conn = [[int(x) for x in l[1:]] for l in lines if l[0] == "CONN"]
    assert conn == want["CONN"]
    got = {l[0]: [int(x) for x in l[1:]] for l in lines if l[0] in ("KFS", "PTS", "REF", "KFS2", "PTS2", "REF2")}
    for k in ("KFS", "PTS", "KFS2", "PTS2"):
        assert got[k] == [len(want[k])] + want[k], k
    assert got["REF"] == [want["REF"]] and got["REF2"] == [want["REF2"]]
