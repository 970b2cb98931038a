"""Host-only headers of the library ((thread, device) workspace lookup, id hash, the id tables' growth transaction, the
projection matchers' host boundary): compiled with plain g++ and run on the CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_workspace_lookup_is_per_thread_and_device(tmp_path):
    exe = str(tmp_path / "workspace_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-pthread", "-fsanitize=address,undefined",
                    "-I" + os.path.join(ROOT, "orb_slam2_map_amd", "csrc"), os.path.join(ROOT, "tests", "workspace_test.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "workspace_test ok" in r.stdout, r.stdout


def test_stateless_entry_points_use_the_lookup():
    """No entry point keeps a bare thread_local workspace object any more, and none keeps a release of its own: the stream,
    the buffers and their teardown are staging.h's."""
    import re
    csrc = os.path.join(ROOT, "orb_slam2_map_amd", "csrc")
    for name in ("matcher_bf.hip", "matcher_proj.hip", "pose_opt.hip", "sim3.hip", "stereo.hip"):
        src = open(os.path.join(csrc, name)).read()
        assert "per_device_workspace<" in src, name
        assert "static thread_local Ws ws" not in src and "static thread_local ProjWorkspace ws" not in src
        assert "static thread_local bool attr_set" not in src  # function attributes are per device as well
        assert "hipStreamCreateWithFlags" not in src and "hipStreamDestroy" not in src, name
        assert not re.search(r"DevBuf\s*\*\s*\w+\s*\[\s*\]", src), name       # DevBuf *bufs[] = {...}
        assert not re.search(r"\{\s*&\w+\s*,\s*&\w+", src), name             # for (DevBuf *b : {&a, &b, ...})
    staging = open(os.path.join(csrc, "staging.h")).read()
    assert "hipStreamCreateWithFlags" in staging and "hipStreamDestroy" in staging and "release_workspace(" in staging
    lookup = open(os.path.join(csrc, "workspace.h")).read()
    assert "#include <hip" not in lookup and '#include "common.h"' not in lookup and "staging.h" in lookup


def test_id_hash_and_pointer_index(tmp_path):
    """The id tables' id -> row hash (insert, find and the lookup the kernels run, slot_for, the capacity rule, growth,
    clear, the rollback of a refused call) and the shim's pointer index against std::map / a linear search, under
    AddressSanitizer + UBSan."""
    exe = str(tmp_path / "id_hash_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-I" + os.path.join(ROOT, "orb_slam2_map_amd", "csrc"), "-I" + os.path.join(ROOT, "orb_slam2_map_amd", "shim"),
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "id_hash_test.cpp"), "-o", exe, "-pthread"],
                   check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "id_hash ok" in r.stdout and "ptr_index ok" in r.stdout, r.stdout


def test_id_table_growth_transaction(tmp_path):
    """id_table.h over malloc-backed buffers and recording operations, under AddressSanitizer + UBSan: growth and a
    retain-style compaction of a small table with every allocation and every operation failed once -- the code returned,
    the table bit for bit what it was, a sync before the first new buffer is freed, no leak -- and then unfailed: contents
    carried over, every id found by id_hash_lookup over the uploaded copy, the old buffers freed exactly once."""
    exe = str(tmp_path / "id_table_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pthread", "-fsanitize=address,undefined",
                    "-I" + os.path.join(ROOT, "orb_slam2_map_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "id_table_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "id_table_test ok" in r.stdout, r.stdout


def test_id_tables_share_one_core():
    """map_table.hip and kfdb.hip keep no lookup, no carve-out, no capacity loop and no growth of their own: the hash is
    id_hash.h's, the transaction id_table.h's, which stays compilable without HIP."""
    import re
    csrc = os.path.join(ROOT, "orb_slam2_map_amd", "csrc")
    for name in ("map_table.hip", "kfdb.hip"):
        src = open(os.path.join(csrc, name)).read()
        assert "id_hash_lookup(" in src and '#include "id_table.h"' in src, name
        assert not re.search(r"\b\w+_lookup\s*\([^;{]*\)\s*\{", src), name      # a function definition named *_lookup
        assert not re.search(r"struct\s+Carve", src), name
        assert not re.search(r"while\s*\(\s*\(.*<<\s*l2\s*\)\s*<", src) and "l2++" not in src, name  # the capacity loop
        assert "hash_slot_for" not in src, name
        assert "id_table_grow(" in src, name
    table = open(os.path.join(csrc, "map_table.hip")).read()
    assert "id_table_replace(" in table and table.count("&world_pos") == 1 and table.count("&t->world_pos") == 0
    core = open(os.path.join(csrc, "id_table.h")).read()
    assert "#include <hip" not in core and '#include "common.h"' not in core and "struct Carver" in core
    assert "l2++" in open(os.path.join(csrc, "id_hash.h")).read()


def test_projection_boundary_on_the_host(tmp_path):
    """The host half of the projection matchers (proj_boundary.h: projections, gates, levels and flags per flavour, claim
    tables, the Sim3 decomposition against the oracle's, bit for bit) and the rotation check's host build, on hand-derived
    values under AddressSanitizer + UBSan."""
    san = ["-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined"]
    inc = ["-I" + os.path.join(ROOT, d) for d in (os.path.join("orb_slam2_map_amd", "csrc"), "include", "oracle")]
    obj, exe = str(tmp_path / "orb_oracle_match.o"), str(tmp_path / "proj_boundary_test")
    subprocess.run(["gcc", "-std=c11", "-Wno-unused-parameter"] + san + inc +
                   ["-c", os.path.join(ROOT, "oracle", "orb_oracle_match.c"), "-o", obj], check=True)
    subprocess.run(["g++", "-std=c++17"] + san + inc + [os.path.join(ROOT, "tests", "proj_boundary_test.cpp"), obj, "-o", exe],
                   check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "proj_boundary_test ok" in r.stdout, r.stdout


def test_projection_float_conventions_live_in_the_boundary_header():
    """Every `volatile` temporary that pins a float convention of the projection matchers' host side is in proj_boundary.h,
    which stays compilable without HIP."""
    csrc = os.path.join(ROOT, "orb_slam2_map_amd", "csrc")
    assert "volatile" not in open(os.path.join(csrc, "matcher_proj.hip")).read()
    boundary = open(os.path.join(csrc, "proj_boundary.h")).read()
    assert "volatile" in boundary and "#include <hip" not in boundary and '#include "common.h"' not in boundary
