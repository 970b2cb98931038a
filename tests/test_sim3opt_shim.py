"""OptimizerT::OptimizeSim3 (orb_slam2_map_amd/shim/orbgpu_shim.hpp) against tests/sim3opt_model.py: it compiles with
-Werror against stand-ins with the reference's members (tests/integration/sim3opt_standin.hpp), INTEGRATION.md's block
compiles, the valid[] / gather construction over injected key frames is the model's (Optimizer.cc:1099-1137), and on a
device the whole call gives what the library gives on the model's arrays."""
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
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import sim3opt_model as M  # noqa: E402

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
    return _build(tmp_path_factory, "sim3opt_shim_test")


@pytest.fixture(scope="module")
def gpu_exe(tmp_path_factory):
    return _build(tmp_path_factory, "sim3opt_shim_gpu_test")


def test_sim3opt_shim_programs_compile(exe, gpu_exe):
    for e in (exe, gpu_exe):
        r = subprocess.run([e], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 2 and "usage" in r.stderr


def test_integration_sim3opt_block_compiles(tmp_path):
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"<!-- sim3opt-snippet -->\s*```cpp\n(.*?)```", text, re.S)
    assert m, "INTEGRATION.md has no sim3opt-snippet block"
    assert "not part of the library" not in text
    src = tmp_path / "sim3opt_block.cc"
    src.write_text('#include <cstring>\n#include "sim3opt_standin.hpp"\n' + m.group(1))
    r = subprocess.run(["g++"] + STRICT + ["-c"] + INC + [str(src), "-o", str(tmp_path / "sim3opt_block.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]


def _key_frames(sc, seed):
    """The scene as two key frames: KF1's key point i is row i; KF2's key points are a shuffle with extras, the match of
    row i sits at i2[i].  Rows that are no correspondence take turns in the five ways the reference skips one."""
    rng = np.random.default_rng(seed)
    n1 = len(sc["valid"])
    n2 = n1 + 9
    i2 = rng.permutation(n2)[:n1].astype(np.int32)
    kind = np.ones(n1, np.int32)
    bad = np.flatnonzero(np.asarray(sc["valid"]) == 0)
    kind[bad] = np.array([0, 2, 3, 4, 5])[np.arange(len(bad)) % 5]
    xy2 = rng.uniform(0, 600, (n2, 2)).astype(np.float32)
    oc2 = rng.integers(0, 8, n2).astype(np.int32)
    xy2[i2], oc2[i2] = sc["kp2_xy"], sc["octave2"]
    blob = (np.array([n1, n2, int(sc["fix_scale"])], np.int32).tobytes() + np.array(sc["K1"], np.float32).tobytes() +
            sc["T1w"].tobytes() + sc["T2w"].tobytes() + sc["inv_level_sigma2"].tobytes() + sc["R12"].tobytes() +
            sc["t12"].tobytes() + np.float32(sc["s12"]).tobytes() + np.float32(sc["th2"]).tobytes() + kind.tobytes() +
            i2.tobytes() + sc["kp1_xy"].tobytes() + sc["octave1"].tobytes() + xy2.tobytes() + oc2.tobytes() +
            sc["Xw1"].tobytes() + sc["Xw2"].tobytes())
    return blob, kind


def _scene(n, seed, fix_scale):
    sc = M.make_scene(n, seed, fix_scale=fix_scale)
    v = np.flatnonzero(sc["valid"])
    sc["octave2"] = sc["octave2"].copy()
    sc["octave2"][v[2]] = M.NLEVELS  # a valid row the library will not take as a correspondence
    return sc


@pytest.mark.parametrize("n,seed,fix_scale", [(60, 81, False), (10, 82, True)])
def test_rows_and_gathers_equal_the_model(exe, tmp_path, n, seed, fix_scale):
    sc = _scene(n, seed, fix_scale)
    blob, kind = _key_frames(sc, seed)
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    inp.write_bytes(blob)
    r = subprocess.run([exe, str(inp), str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0 and "sim3opt shim ok" in r.stdout, r.stdout
    buf, n1 = out.read_bytes(), len(sc["valid"])
    at = [0]

    def take(dtype, count):
        a = np.frombuffer(buf, dtype, count, at[0])
        at[0] += a.nbytes
        return a
    valid, in_range = take(np.uint8, n1), take(np.uint8, n1)
    o1, o2 = take(np.int32, n1), take(np.int32, n1)
    x1, x2 = take(np.float32, 3 * n1).reshape(n1, 3), take(np.float32, 3 * n1).reshape(n1, 3)
    k1, k2 = take(np.float32, 2 * n1).reshape(n1, 2), take(np.float32, 2 * n1).reshape(n1, 2)
    q, t, s, R = take(np.float64, 4), take(np.float64, 3), take(np.float64, 1)[0], take(np.float64, 9).reshape(3, 3)
    assert at[0] == len(buf)
    want = np.asarray(sc["valid"]) != 0
    assert np.array_equal(valid != 0, want) and np.array_equal(kind == 1, want)
    pb = M.prepare(sc)  # the model's correspondences are the rows that are valid and in range
    assert np.array_equal(np.flatnonzero((valid != 0) & (in_range != 0)), pb["idx"]) and pb["n_bad_index"] == 1
    for got, key in ((o1, "octave1"), (o2, "octave2"), (x1, "Xw1"), (x2, "Xw2"), (k1, "kp1_xy"), (k2, "kp2_xy")):
        assert np.array_equal(got[want], np.asarray(sc[key])[want]), key
        assert not got[~want].any(), key
    q0, t0, s0 = M.state_from_floats(sc["R12"], sc["t12"], sc["s12"])
    assert np.array_equal(q, q0) and np.array_equal(t, t0) and s == s0
    assert np.abs(R - M.quat_to_matrix(q0)).max() < 1e-15


@pytest.mark.gpu
@pytest.mark.parametrize("n,seed,fix_scale", [(150, 91, False), (40, 92, True), (14, 93, False)])
def test_shim_end_to_end_equals_the_library_on_the_models_arrays(gpu_exe, tmp_path, n, seed, fix_scale):
    from orb_slam2_map_amd import lib as G
    if G.device_count() < 1:
        pytest.skip("no HIP device")
    sc = _scene(n, seed, fix_scale) if n != 14 else M.make_scene(n, seed, fix_scale=fix_scale, outlier_frac=0.6)
    blob, kind = _key_frames(sc, seed)
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    inp.write_bytes(blob)
    r = subprocess.run([gpu_exe, str(inp), str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "sim3opt shim ok" in r.stdout, r.stdout
    buf, n1 = out.read_bytes(), len(sc["valid"])
    n_inliers = int(np.frombuffer(buf, np.int32, 1)[0])
    is_null = np.frombuffer(buf, np.uint8, n1, 4) != 0
    S = np.frombuffer(buf, np.float64, 8, 4 + n1)
    res = G.Sim3OptResult.from_buffer_copy(buf[4 + n1 + 64:]).as_dict()
    assert 4 + n1 + 64 + C.sizeof(G.Sim3OptResult) == len(buf)
    ni, inl, ref = G.sim3_optimize(sc["valid"], sc["Xw1"], sc["Xw2"], sc["octave1"], sc["octave2"], sc["kp1_xy"], sc["kp2_xy"],
                                   sc["T1w"], sc["T2w"], sc["K1"], sc["K2"], sc["inv_level_sigma2"], sc["R12"], sc["t12"],
                                   sc["s12"], th2=sc["th2"], fix_scale=fix_scale, inlier=np.full(n1, 7, np.uint8))
    assert n_inliers == ni == res["n_inliers"] and all(np.array_equal(res[k], ref[k]) for k in ref)
    m = M.optimize_sim3(sc)
    assert all(res[k] == m[k] for k in M.DISCRETE)
    # the matches that are NULL afterwards: those that were NULL before and the cleared correspondences
    assert np.array_equal(is_null, (kind == 0) | (inl == 0)) and np.array_equal(inl == 0, m["inlier"] == 0)
    if res["stages"] == 2:
        assert n != 14 and np.abs(M.quat_to_matrix(S[:4]) - res["R12_d"]).max() < 1e-14
        assert np.array_equal(S[4:7], res["t12_d"]) and S[7] == res["s12_d"]
    else:  # fewer than 10 left: S12 stays as it came
        q0, t0, s0 = M.state_from_floats(sc["R12"], sc["t12"], sc["s12"])
        assert n == 14 and n_inliers == 0 and np.array_equal(S[:4], q0) and np.array_equal(S[4:7], t0) and S[7] == s0
