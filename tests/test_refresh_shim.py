"""CovisibilityGraphT's SetScaleFactors / SetDescriptors / SetCentres / RefreshMapPoints (orb_slam2_map_amd/shim/orbgpu_shim.hpp)
and INTEGRATION.md's refresh block (2q): they compile with -Werror against stand-ins with the reference's members
(tests/integration/refresh_standin.hpp); the host-only parts run as a stand-alone program, also under
-fsanitize=address,undefined; the device program (tests/refresh_shim_gpu_test.cpp) refreshes a small map with and without a
MapPoint table."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "orb_slam2_map_amd")

STRICT = ["-std=c++17", "-Wall", "-Wextra", "-Werror"]
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "shim"), "-I" + os.path.join(HERE, "integration")]


def integration_block():
    """the code block of INTEGRATION.md's refresh section"""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"^### 2q\. .*?```cpp\n(.*?)```", text, re.S | re.M)
    assert m, "INTEGRATION.md has no refresh block"
    return m.group(1)


def build(tmp_path, name, extra=()):
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(PKG, "liborbgpu.so")):
        ge.build()
    (tmp_path / "refresh_block.inc").write_text(integration_block())
    exe = str(tmp_path / name)
    cmd = ["g++"] + STRICT + ["-O1"] + list(extra) + INC + ["-I" + str(tmp_path), os.path.join(HERE, name + ".cpp"), "-o", exe,
                                                           "-L" + PKG, "-lorbgpu", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-pthread"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return exe


def test_the_block_names_the_hooks():
    block = integration_block()
    for name in ("SetScaleFactors(pKF->mvScaleFactors)", "->SetDescriptors(pKF,", "->SetCentres({this}, CameraCentre)",
                 "void MapPoint::SetRefreshed(", "->RefreshMapPoints(vpMapPointMatches,"):
        assert name in block


@pytest.mark.parametrize("sanitize", [False, True])
def test_shim_and_block_compile_and_the_host_only_parts_run(tmp_path, sanitize):
    exe = build(tmp_path, "refresh_shim_test", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else [])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
    assert r.returncode == 2 and "usage" in r.stderr
    r = subprocess.run([exe, "run"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "refresh shim ok" in r.stdout, r.stdout[-3000:]


def test_the_device_program_builds(tmp_path):
    exe = build(tmp_path, "refresh_shim_gpu_test")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 2 and "usage" in r.stderr


@pytest.mark.gpu
def test_refresh_map_points_with_and_without_a_table(gpu, tmp_path):
    exe = build(tmp_path, "refresh_shim_gpu_test")
    r = subprocess.run([exe, "run"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "refresh shim gpu ok" in r.stdout, r.stdout[-3000:]
