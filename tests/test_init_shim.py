"""InitializerT (orb_slam2_map_amd/shim/orbgpu_shim.hpp) against tests/init_model.py: it compiles with -Werror against
stand-ins with the reference's members (tests/integration/init_standin.hpp), together with the MonocularInitialization
wiring of INTEGRATION.md (restated in tests/init_shim_test.cpp: that block carries no snippet marker); without a device its
sampler and what it hands over give the model's sets; on the device it equals the model end to end."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "orb_slam2_map_amd")
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import init_model as M  # noqa: E402

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
    return _build(tmp_path_factory, "init_shim_test")


@pytest.fixture(scope="module")
def gpu_exe(tmp_path_factory):
    return _build(tmp_path_factory, "init_shim_gpu_test")


def test_init_shim_programs_compile(exe, gpu_exe):
    for e in (exe, gpu_exe):
        r = subprocess.run([e], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 2 and "usage" in r.stderr


def test_integration_block_is_the_one_compiled():
    """INTEGRATION.md's MonocularInitialization block and the function tests/init_shim_test.cpp compiles hold the same calls"""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    src = open(os.path.join(HERE, "init_shim_test.cpp")).read()
    for line in ("mpInitializer = new Initializer(mInitialFrame, 1.0, 200, RandomInt);",
                 "if (mpInitializer->Initialize(mCurrentFrame, mvIniMatches, Rcw, tcw, mvIniP3D, vbTriangulated)) {"):
        assert line in text and line in src, line


def _draws(rng, n, sets):
    return [int(rng.integers(0, n - k)) for _ in range(sets) for k in range(8)]


@pytest.mark.parametrize("n1,n2,n,iterations,success,seed", [(40, 50, 25, 200, 1, 1), (30, 20, 8, 7, 0, 2), (12, 9, 7, 5, 1, 3),
                                                             (20, 20, 20, 5000, 1, 4)])
def test_sampler_and_handover_equal_the_model(exe, tmp_path, n1, n2, n, iterations, success, seed):
    rng = np.random.default_rng(seed)
    matches = np.full(n1, -1, np.int32)
    matches[rng.permutation(n1)[:n]] = rng.permutation(n2)[:n]
    matches[np.flatnonzero(matches < 0)[:1]] = n2 + 3           # I1: not kept
    its = min(iterations, 4096)
    draws = _draws(rng, n, 2 * its) if n >= 8 else []
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    inp.write_bytes(np.array([n1, n2, iterations, len(draws), success], np.int32).tobytes() + matches.tobytes() +
                    np.array(draws, np.int32).tobytes())
    r = subprocess.run([exe, str(inp), str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0 and "init shim ok" in r.stdout, r.stdout
    got = np.frombuffer(out.read_bytes(), np.int32)
    if n < 8:
        assert got.tolist() == [0, n, -1, 0]
        return
    it = iter(draws)
    want = M.sample_sets(n, 2 * its, lambda lo, hi: next(it))
    assert got[:3].tolist() == [success, n, its]
    assert np.array_equal(got[3:3 + 8 * its].reshape(-1, 8), want[:its])
    assert got[3 + 8 * its] == success
    assert np.array_equal(got[4 + 8 * its:].reshape(-1, 8), want[its:])       # the second call goes on in the stream


def test_sampler_refuses_what_the_model_refuses():
    with pytest.raises(ValueError):
        M.sample_sets(7, 1, lambda lo, hi: 0)
    with pytest.raises(ValueError):
        M.sample_sets(9, 1, lambda lo, hi: hi + 1)


# the first seeds of the draw for which the model alone has spread 0 and leaves nothing out (as init_model.PARITY_SCENES')
DRAW_SEEDS = {"general": 9402, "planar": 13406, "few": 9404}


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["general", "planar", "few"])
def test_shim_end_to_end_equals_the_model(gpu_exe, tmp_path, key):
    """An InitializerT over stand-in frames: its answer, R21, t21, vP3D and vbTriangulated equal the model's over the sets
    the replayed sampler draws."""
    from orb_slam2_map_amd import lib as G
    if G.device_count() < 1:
        pytest.skip("no HIP device")
    n, seed, kind, _ = M.PARITY_SCENES[key]
    sc = M.make_scene(n, seed, kind, n_hyp=1)
    n1, n2, its = len(sc["kp1"]), len(sc["kp2"]), 40
    rng = np.random.default_rng(DRAW_SEEDS[key])
    draws = _draws(rng, n, its)
    it = iter(draws)
    sc["sets"] = M.sample_sets(n, its, lambda lo, hi: next(it))
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    inp.write_bytes(np.array([n1, n2, its, len(draws)], np.int32).tobytes() + np.array(sc["K"], np.float32).tobytes() +
                    sc["kp1"].tobytes() + sc["kp2"].tobytes() + sc["matches12"].tobytes() + np.array(draws, np.int32).tobytes())
    r = subprocess.run([gpu_exe, str(inp), str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "init shim ok" in r.stdout, r.stdout
    buf = out.read_bytes()
    m, spread = M.model_pass(sc)
    oh, of = M.left_out(m, M.BOUND_FACTOR * spread)
    print("%s: spread %.3e, left out %d, model success %d" % (key, spread, oh.sum() + of.sum(), m["success"]))
    assert spread == 0.0 and not oh.any() and not of.any()      # the scene is compared bit for bit
    got = np.frombuffer(buf, np.int32, 1)[0]
    res = G.InitResult.from_buffer_copy(buf[4:4 + C.sizeof(G.InitResult)]).as_dict()
    at = 4 + C.sizeof(G.InitResult)
    assert got == m["success"] == res["success"] and res["n"] == n
    for k in ("best_h", "best_f", "used_homography", "n_inliers", "best_motion", "second_best_good"):
        assert int(res[k]) == int(m[k]), k
    assert np.array_equal(res["n_good"], m["n_good"]) and res["parallax_deg"].tobytes() == m["parallax_deg"].tobytes()
    if got:
        assert buf[at:at + 36] == m["R21"].tobytes() and buf[at + 36:at + 48] == m["t21"].tobytes()
        at += 48
        assert buf[at:at + 12 * n1] == m["P3D"].tobytes()
        at += 12 * n1
        assert np.array_equal(np.frombuffer(buf, np.uint8, n1, at), m["triangulated"])
        at += n1
    assert np.frombuffer(buf, np.int32, 1, at)[0] == its
    assert np.array_equal(np.frombuffer(buf, np.int32, 8 * its, at + 4).reshape(-1, 8), sc["sets"])
    assert at + 4 + 32 * its == len(buf)
