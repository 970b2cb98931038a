"""CovisibilityGraphT::Compact / KeyFrameDatabaseT::Compact (orb_slam2_map_amd/shim/orbgpu_shim.hpp) and INTEGRATION.md's
compaction block (2p, its second block): they compile with -Werror against stand-ins with the reference's members
(tests/integration/compact_standin.hpp); what needs no device runs as a stand-alone program, also under
-fsanitize=address,undefined; on the GPU the block compacts a graph and a database once its example policy says so."""
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
    """the code block of INTEGRATION.md that defines CompactAfterCulling"""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blocks = [b for b in re.findall(r"```cpp\n(.*?)```", text, re.S) if "void CompactAfterCulling(" in b]
    assert len(blocks) == 1, "INTEGRATION.md has no compaction block"
    return blocks[0]


def build(tmp, sanitize=False):
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(PKG, "liborbgpu.so")):
        ge.build()
    (tmp / "compact_block.inc").write_text(integration_block())
    exe = str(tmp / "compact_shim_test")
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    cmd = ["g++"] + STRICT + ["-O1"] + extra + INC + ["-I" + str(tmp), os.path.join(HERE, "compact_shim_test.cpp"), "-o", exe,
                                                     "-L" + PKG, "-lorbgpu", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-pthread"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return exe


def test_the_documents_say_where_the_call_goes():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = integration_block()
    for name in ("pCovisibilityGraph->Compact()", "pKeyFrameDB->Compact()", "orbgpu_covis_graph_size"):
        assert name in block
    for section in ("2h", "2o", "2p"):
        body = re.search(r"^### %s\. .*?(?=^### |^## )" % section, text, re.S | re.M).group(0)
        assert "Compact()" in body, section


@pytest.mark.parametrize("sanitize", [False, True])
def test_shim_and_block_compile_and_the_host_only_parts_run(tmp_path, sanitize):
    exe = build(tmp_path, sanitize)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
    assert r.returncode == 2 and "usage" in r.stderr
    r = subprocess.run([exe, "run"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "compact shim ok" in r.stdout, r.stdout[-3000:]


@pytest.mark.gpu
def test_block_on_the_device(gpu, tmp_path):
    exe = build(tmp_path)
    r = subprocess.run([exe, "gpu"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "compact shim ok" in r.stdout, r.stdout[-3000:]
