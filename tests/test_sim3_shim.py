"""Sim3SolverT (orb_slam2_map_amd/shim/orbgpu_shim.hpp) against tests/sim3_model.py without a device: it compiles with
-Werror against stand-ins with the reference's members (tests/integration/sim3_standin.hpp); its sampler and its iterate
state machine, run over injected counts, give the model's sequence."""
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

import sim3_model as M  # noqa: E402

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
    return _build(tmp_path_factory, "sim3_shim_test")


@pytest.fixture(scope="module")
def gpu_exe(tmp_path_factory):
    return _build(tmp_path_factory, "sim3_shim_gpu_test")


def test_sim3_shim_device_program_compiles(gpu_exe):
    r = subprocess.run([gpu_exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 2 and "usage" in r.stderr


def test_sim3_shim_compiles(exe):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 2 and "usage" in r.stderr


def test_integration_sim3_block_compiles(tmp_path):
    import re
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"<!-- sim3-snippet -->\s*```cpp\n(.*?)```", text, re.S)
    assert m, "INTEGRATION.md has no sim3-snippet block"
    src = tmp_path / "sim3_block.cc"
    src.write_text('#include <cstring>\n#include "sim3_standin.hpp"\n' + m.group(1))
    r = subprocess.run(["g++"] + STRICT + ["-c"] + INC + [str(src), "-o", str(tmp_path / "sim3_block.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]


@pytest.mark.parametrize("n1,n_valid,min_inliers,max_iterations,chunk,seed", [
    (40, 25, 20, 300, 5, 1),   # max_its = 7
    (90, 70, 20, 30, 5, 2),    # capped by max_iterations
    (33, 20, 20, 300, 5, 3),   # N == min_inliers: one iteration
    (30, 19, 20, 300, 5, 4),   # N < min_inliers: bNoMore at once
    (70, 64, 6, 300, 7, 5)])
def test_sampler_and_state_machine_equal_the_model(exe, tmp_path, n1, n_valid, min_inliers, max_iterations, chunk, seed):
    rng = np.random.default_rng(seed)
    valid = np.zeros(n1, np.int32)
    valid[rng.permutation(n1)[:n_valid]] = 1
    max_its = M.ransac_iterations(n_valid, 0.99, min_inliers, max_iterations)
    draws = []
    for _ in range(max_its):
        draws += [int(rng.integers(0, n_valid - k)) for k in range(3)]
    counts = rng.integers(0, min_inliers + 3, max_its).astype(np.int32)
    counts[rng.integers(0, max_its)] = min_inliers + 1
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    inp.write_bytes(np.array([n1, min_inliers, max_iterations, chunk, len(draws)], np.int32).tobytes() + valid.tobytes() +
                    np.array(draws, np.int32).tobytes() + counts.tobytes())
    r = subprocess.run([exe, str(inp), str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0 and "sim3 shim ok" in r.stdout, r.stdout
    got = np.frombuffer(out.read_bytes(), np.int32)
    assert got[0] == n_valid and got[1] == max_its
    it = iter(draws)
    want = M.sample_triples(n_valid, max_its, lambda lo, hi: next(it))
    assert np.array_equal(got[2:2 + 3 * max_its].reshape(-1, 3), want)
    log = got[2 + 3 * max_its:].reshape(-1, 6)
    st = M.RansacState(n_valid, min_inliers, max_its)
    rows = []
    while True:
        acc, n_inl, no_more = st.iterate(chunk, counts)
        rows.append([int(acc >= 0), n_inl, int(no_more), st.iterations, n_inl, max(st.best_iteration, 0)])
        if no_more:
            break
    assert log.tolist() == rows


def test_sampler_refuses_what_the_model_refuses():
    with pytest.raises(ValueError):
        M.sample_triples(2, 1, lambda lo, hi: 0)
    with pytest.raises(ValueError):
        M.sample_triples(5, 1, lambda lo, hi: hi + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("n,seed,fix_scale,chunk", [(150, 61, False, 5), (40, 62, True, 5), (25, 63, False, 3), (19, 64, False, 5)])
def test_shim_end_to_end_equals_the_model(gpu_exe, tmp_path, n, seed, fix_scale, chunk):
    """A Sim3SolverT over stand-in key frames asks the library once and serves iterate(chunk) until bNoMore: every call's
    answer, the accepted T12 / R / t / s and vbInliers equal the model's over the triples the replayed sampler draws."""
    from orb_slam2_map_amd import lib as G
    if G.device_count() < 1:
        pytest.skip("no HIP device")
    sc = M.make_scene(n, seed, fix_scale=fix_scale)
    n1 = len(sc["valid"])
    max_its = M.ransac_iterations(n, 0.99, 20, 300)
    rng = np.random.default_rng(seed)
    draws = []
    for _ in range(max_its):
        draws += [int(rng.integers(0, n - k)) for k in range(3)]
    it = iter(draws)
    sc["triples"] = M.sample_triples(n, max_its, lambda lo, hi: next(it))
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    inp.write_bytes(np.array([n1, int(fix_scale), 20, 300, chunk, len(draws)], np.int32).tobytes() +
                    np.array(sc["K1"], np.float32).tobytes() + sc["T1w"].tobytes() + sc["T2w"].tobytes() + sc["level_sigma2"].tobytes() +
                    sc["valid"].astype(np.int32).tobytes() + sc["octave1"].tobytes() + sc["octave2"].tobytes() +
                    sc["Xw1"].tobytes() + sc["Xw2"].tobytes() + np.array(draws, np.int32).tobytes())
    r = subprocess.run([gpu_exe, str(inp), str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "sim3 shim ok" in r.stdout, r.stdout
    buf = out.read_bytes()
    head = np.frombuffer(buf, np.int32, 2)
    assert head[0] == n and head[1] == max_its
    m = M.solve(sc)
    st = M.RansacState(n, 20, max_its)
    at, first = 8, True
    while True:
        acc, n_inl, no_more = st.iterate(chunk, m["counts"])
        if first and n >= 20:
            assert np.array_equal(np.frombuffer(buf, np.int32, 3 * max_its, at).reshape(-1, 3), sc["triples"])
        if first:
            at += 12 * max_its if n >= 20 else 12 * max_its  # the program pads the block when nothing was drawn
            first = False
        assert np.frombuffer(buf, np.int32, 4, at).tolist() == [int(acc >= 0), n_inl, int(no_more), st.iterations]
        at += 16
        if acc >= 0:
            got = np.frombuffer(buf, np.float32, 29, at)
            at += 116
            assert got[:16].tobytes() == m["T12"][acc].tobytes() and got[16:25].tobytes() == m["R"][acc].tobytes()
            assert got[25:28].tobytes() == m["t"][acc].tobytes() and got[28:].tobytes() == m["s"][acc:acc + 1].tobytes()
            bits = np.unpackbits(m["masks"][acc].view(np.uint8), bitorder="little")[:n1]
            assert np.array_equal(np.frombuffer(buf, np.uint8, n1, at), bits)
            at += n1
        if no_more:
            break
    assert at == len(buf)
