"""The key-frame database's entry points (include/orbgpu.h) without a GPU: the symbols are exported and listed, the header
compiles as C99 and C++11, every refusal of K8 is answered with EINVAL before the device is touched, and without a device
the calls that compute or store fail with EHIP -- never a CPU fallback."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)

SYMBOLS = ("orbgpu_keyframe_db_create", "orbgpu_keyframe_db_destroy", "orbgpu_keyframe_db_clear", "orbgpu_keyframe_db_size",
           "orbgpu_keyframe_db_add", "orbgpu_keyframe_db_erase", "orbgpu_keyframe_db_set_covisibles", "orbgpu_keyframe_db_score",
           "orbgpu_keyframe_db_detect_loop", "orbgpu_keyframe_db_detect_reloc", "orbgpu_keyframe_db_last_query",
           "orbgpu_keyframe_db_debug_global_queries")

PROBE = """#include <stddef.h>
#include <stdio.h>
#include "orbgpu.h"
int main(void)
{
    orbgpu_keyframe_db *db = NULL;
    int32_t ids[2] = {1, 1}, n = -1;
    double vals[2] = {0.5, 0.5};
    int64_t cand[4];
    if (orbgpu_keyframe_db_create(100, 1, 0, 0, &db) != ORBGPU_EINVAL || db)
        return 1;
    if (orbgpu_keyframe_db_create(100, 0, 0, 2, &db) != ORBGPU_OK || !db)
        return 2;
    if (orbgpu_keyframe_db_add(db, 7, 2, ids, vals) != ORBGPU_EINVAL)
        return 3;
    if (orbgpu_keyframe_db_detect_reloc(db, 2, ids, vals, 4, cand, &n) != ORBGPU_EINVAL || n != -1)
        return 4;
    if (orbgpu_keyframe_db_size(db, &n) != ORBGPU_OK || n != 0)
        return 5;
    printf("%d\\n", ORBGPU_ABI_VERSION);
    return orbgpu_keyframe_db_destroy(db) == ORBGPU_OK ? 0 : 6;
}
"""


@pytest.fixture(scope="module")
def glib():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(ROOT, "orb_slam2_map_amd", "liborbgpu.so")):
        ge.build()
    from orb_slam2_map_amd import lib
    return lib


def test_symbols_are_exported_and_listed(glib):
    L = glib.lib()
    for s in SYMBOLS:
        assert hasattr(L, s) and s in glib.ABI_SYMBOLS, s
    assert L.orbgpu_abi_version() == 1  # symbols were added, nothing changed


@pytest.mark.parametrize("cc,ext,std", [("gcc", "c", "-std=c99"), ("g++", "cc", "-std=c++11")])
def test_header_compiles_and_a_c_program_is_refused_without_a_device(glib, tmp_path, cc, ext, std):
    src = tmp_path / ("probe." + ext)
    src.write_text(PROBE)
    exe = str(tmp_path / "probe")
    pkg = os.path.join(ROOT, "orb_slam2_map_amd")
    r = subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe, "-L" + pkg,
                        "-lorbgpu", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["1"], (r.returncode, r.stdout)


def _arr(a, dt):
    a = np.ascontiguousarray(a, dt)
    return a, a.ctypes.data_as(C.c_void_p)


def test_every_refusal_is_einval_before_the_device_is_touched(glib):
    L = glib.lib()
    h = C.c_void_p()
    for args in ((0, 0, 0, 0), (-5, 0, 0, 0), (100, 0, -1, 0), (100, 0, 0, -1)) + tuple((100, s, 0, 0) for s in range(1, 6)):
        assert L.orbgpu_keyframe_db_create(*args, C.byref(h)) == glib.EINVAL and not h, args  # scoring: L1_NORM only
    assert b"L1_NORM" in L.orbgpu_last_error_string()
    assert L.orbgpu_keyframe_db_create(100, 0, 0, 0, None) == glib.EINVAL
    assert L.orbgpu_keyframe_db_create(100, glib.L1_NORM, 0, 2, C.byref(h)) == glib.OK and h
    n, known = C.c_int32(-7), C.c_int32(-7)
    cand, pc = _arr(np.zeros(8), np.int64)
    out, po = _arr(np.zeros(8), np.float32)
    one, p1 = _arr([3], np.int64)
    good_i, pgi = _arr([1, 2], np.int32)
    good_v, pgv = _arr([0.5, 0.5], np.float64)
    bad = [([1, 1], [0.5, 0.5]), ([2, 1], [0.5, 0.5]), ([1, 100], [0.5, 0.5]), ([-1, 1], [0.5, 0.5]), ([1, 2], [0.5, np.inf]),
           ([1, 2], [-np.inf, 0.5]), ([1, 2], [np.nan, 0.5])]
    for ids, vals in bad:
        keep_i, pi = _arr(ids, np.int32)
        keep_v, pv = _arr(vals, np.float64)
        assert L.orbgpu_keyframe_db_add(h, 3, 2, pi, pv) == glib.EINVAL, (ids, vals)
        assert L.orbgpu_keyframe_db_score(h, 2, pi, pv, 1, p1, po) == glib.EINVAL
        assert L.orbgpu_keyframe_db_detect_loop(h, 2, pi, pv, 0, None, 0.1, 8, pc, C.byref(n)) == glib.EINVAL
        assert L.orbgpu_keyframe_db_detect_reloc(h, 2, pi, pv, 8, pc, C.byref(n)) == glib.EINVAL
    assert n.value == -7
    assert L.orbgpu_keyframe_db_add(h, -1, 2, pgi, pgv) == glib.EINVAL
    assert L.orbgpu_keyframe_db_add(h, 3, -1, pgi, pgv) == glib.EINVAL
    assert L.orbgpu_keyframe_db_add(h, 3, 2, None, pgv) == glib.EINVAL and L.orbgpu_keyframe_db_add(h, 3, 2, pgi, None) == glib.EINVAL
    assert L.orbgpu_keyframe_db_add(None, 3, 2, pgi, pgv) == glib.EINVAL
    eleven, p11 = _arr(np.arange(11), np.int64)
    assert L.orbgpu_keyframe_db_set_covisibles(h, 3, 11, p11) == glib.EINVAL
    assert b"neighbours" in L.orbgpu_last_error_string()
    assert L.orbgpu_keyframe_db_set_covisibles(h, 3, -1, p11) == glib.EINVAL
    assert L.orbgpu_keyframe_db_set_covisibles(h, -3, 2, p11) == glib.EINVAL
    assert L.orbgpu_keyframe_db_set_covisibles(h, 3, 2, None) == glib.EINVAL
    neg, pneg = _arr([4, -4], np.int64)
    assert L.orbgpu_keyframe_db_set_covisibles(h, 3, 2, pneg) == glib.EINVAL
    assert L.orbgpu_keyframe_db_detect_loop(h, 2, pgi, pgv, 0, None, float("nan"), 8, pc, C.byref(n)) == glib.EINVAL
    assert L.orbgpu_keyframe_db_detect_loop(h, 2, pgi, pgv, 1, None, 0.1, 8, pc, C.byref(n)) == glib.EINVAL
    assert L.orbgpu_keyframe_db_detect_loop(h, 2, pgi, pgv, 0, None, 0.1, -1, pc, C.byref(n)) == glib.EINVAL
    assert L.orbgpu_keyframe_db_detect_loop(h, 2, pgi, pgv, 0, None, 0.1, 8, None, C.byref(n)) == glib.EINVAL
    assert L.orbgpu_keyframe_db_detect_reloc(h, 2, pgi, pgv, 8, pc, None) == glib.EINVAL
    assert L.orbgpu_keyframe_db_score(h, 2, pgi, pgv, 1, None, po) == glib.EINVAL
    assert L.orbgpu_keyframe_db_erase(h, -1, p1, C.byref(known)) == glib.EINVAL and known.value == -7
    assert L.orbgpu_keyframe_db_erase(h, 1, None, C.byref(known)) == glib.EINVAL
    assert L.orbgpu_keyframe_db_last_query(h, 0, None, None, None, None, None, None, None) == glib.EINVAL
    # what needs no device works without one: a neighbour list for an id that is not in the database, an erase of an
    # unknown id (ignored, not counted), size, the empty last query, clear
    assert L.orbgpu_keyframe_db_set_covisibles(h, 3, 2, p11) == glib.OK
    assert L.orbgpu_keyframe_db_erase(h, 1, p1, C.byref(known)) == glib.OK and known.value == 0
    assert L.orbgpu_keyframe_db_size(h, C.byref(n)) == glib.OK and n.value == 0
    assert L.orbgpu_keyframe_db_last_query(h, 0, None, None, None, None, None, None, C.byref(n)) == glib.OK and n.value == 0
    g = C.c_int64(-1)
    assert L.orbgpu_keyframe_db_debug_global_queries(h, C.byref(g)) == glib.OK and g.value == 0
    assert L.orbgpu_keyframe_db_debug_global_queries(h, None) == glib.EINVAL
    assert L.orbgpu_keyframe_db_clear(h) == glib.OK
    assert L.orbgpu_keyframe_db_destroy(h) == glib.OK and L.orbgpu_keyframe_db_destroy(None) == glib.OK


def test_no_device_means_ehip_not_a_fallback(glib):
    if glib.device_count() > 0:
        pytest.skip("a GPU is visible")
    db = glib.KeyFrameDatabase(100, initial_rows=2)
    v = (np.array([1, 2], np.int32), np.array([0.5, 0.5]))
    for call in (lambda: db.add(3, *v), lambda: db.score(v[0], v[1], [3]), lambda: db.DetectLoopCandidates(v[0], v[1], [], 0.1),
                 lambda: db.DetectRelocalizationCandidates(*v)):
        with pytest.raises(glib.OrbGpuError) as ei:
            call()
        assert ei.value.status == glib.EHIP and "no CPU fallback" in str(ei.value)
    assert db.size() == 0
    with pytest.raises(glib.OrbGpuError) as ei:
        glib.KeyFrameDatabase(100, scoring=glib.L2_NORM)
    assert ei.value.status == glib.EINVAL
    db.close()
