"""orbgpu_compact_result and the two compaction entry points at the C boundary: the structure's size and field offsets are
the same in include/orbgpu.h (measured by a C99 program) and in lib.py, both symbols are exported and declared, the ABI
version is still 1, and what needs no device -- a handle that holds nothing, a null handle -- answers without one."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "orb_slam2_map_amd")
FIELDS = ("compacted", "rows_before", "rows_after", "rows_bad_kept", "row_capacity", "slots_before", "slots_after", "slot_capacity")


@pytest.fixture(scope="module")
def glib():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(PKG, "liborbgpu.so")):
        ge.build()
    from orb_slam2_map_amd import lib
    return lib


def test_struct_layout_matches_the_header(glib, tmp_path):
    src = tmp_path / "compact_abi.c"
    src.write_text('#include "orbgpu.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n'
                   '    printf("%d", (int)sizeof(orbgpu_compact_result));\n' +
                   "".join('    printf(" %%d", (int)offsetof(orbgpu_compact_result, %s));\n' % f for f in FIELDS) +
                   '    printf(" %d\\n", ORBGPU_ABI_VERSION);\n    return 0;\n}\n')
    exe = str(tmp_path / "compact_abi")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-o", exe], check=True)
    got = [int(x) for x in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    R = glib.CompactResult
    assert [name for name, _ in R._fields_] == list(FIELDS)
    assert got == [C.sizeof(R)] + [getattr(R, f).offset for f in FIELDS] + [1]
    assert C.sizeof(R) == 48 and R.slots_before.offset == 24


def test_symbols_and_version(glib):
    L = glib.lib()
    for name in ("orbgpu_covis_graph_compact", "orbgpu_keyframe_db_compact"):
        assert hasattr(L, name) and name in glib.ABI_SYMBOLS
    assert L.orbgpu_abi_version() == 1
    header = open(os.path.join(ROOT, "include", "orbgpu.h")).read()
    assert "int orbgpu_covis_graph_compact(orbgpu_covis_graph *g, orbgpu_compact_result *res);" in header
    assert "int orbgpu_keyframe_db_compact(orbgpu_keyframe_db *db, orbgpu_compact_result *res);" in header
    assert "no compaction yet" not in header and "#define ORBGPU_ABI_VERSION 1" in header


def test_nothing_to_do_needs_no_device(glib):
    zeros = dict.fromkeys(FIELDS, 0)
    g = glib.CovisibilityGraph(initial_rows=2, initial_slots=8)
    db = glib.KeyFrameDatabase(100, initial_rows=2)
    try:
        assert g.compact() == zeros and db.compact() == zeros  # C6 / D4 on handles that were never bound
        assert g.size() == (0, 0) and db.size() == 0
        L = glib.lib()
        assert L.orbgpu_covis_graph_compact(g.h, None) == glib.OK and L.orbgpu_keyframe_db_compact(db.h, None) == glib.OK
        assert L.orbgpu_covis_graph_compact(None, None) == glib.EINVAL and L.orbgpu_keyframe_db_compact(None, None) == glib.EINVAL
    finally:
        g.close()
        db.close()
