"""orbgpu_covis_graph_set_scale_factors / _set_descriptors / _set_centres, orbgpu_covis_refresh_points and
orbgpu_mappoint_table_refresh: the symbols, constants and the result struct through lib.py, the header as C, and every refusal
answered with ORBGPU_EINVAL and its message before any device is touched, the graph being what it was.  No GPU: a graph that
has stored nothing is host memory only.  (Refusals that need a row or a table -- set_descriptors with a wrong n_slots or a
null array, a bad row ignoring the call, every refusal of the table form behind a real table -- are answered as early, but
rows and tables need a device to exist: they are asserted in tests/test_gpu_refresh_refusals.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("orbgpu_covis_graph_set_scale_factors", "orbgpu_covis_graph_set_descriptors", "orbgpu_covis_graph_set_centres",
       "orbgpu_covis_refresh_points", "orbgpu_mappoint_table_refresh")


@pytest.fixture(scope="module")
def G():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(ROOT, "orb_slam2_map_amd", "liborbgpu.so")):
        ge.build()
    from orb_slam2_map_amd import lib
    return lib


def refused(G, call, text):
    with pytest.raises(G.OrbGpuError) as ei:
        call()
    assert ei.value.status == G.EINVAL and text in str(ei.value), str(ei.value)


def test_symbols_constants_and_struct_layout(G):
    L = G.lib()
    for name in NEW:
        assert name in G.ABI_SYMBOLS and hasattr(L, name) and getattr(L, name).argtypes is not None, name
    assert L.orbgpu_abi_version() == 1
    header = open(os.path.join(ROOT, "include", "orbgpu.h")).read()
    assert re.search(r"#define ORBGPU_ABI_VERSION 1\b", header)
    m = re.search(r"typedef struct orbgpu_covis_refresh_result \{(.*?)\} orbgpu_covis_refresh_result;", header, re.S)
    assert m, "the header does not declare the result struct"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [(f.strip(), "int64_t" in decl) for decl in body.split(";") if decl.strip()
              for f in decl.replace("int32_t", "").replace("int64_t", "").split(",")]
    assert fields == [(name, t is C.c_int64) for name, t in G.CovisRefreshResult._fields_]
    assert C.sizeof(G.CovisRefreshResult) == 48
    for name, value in (("COVIS_REFRESH_MAX_OBS", 1024), ("REFRESH_DESCRIPTOR", 1), ("REFRESH_NORMAL_DEPTH", 2), ("REFRESH_NO_OBS", 1),
                        ("REFRESH_OVERFLOW", 2), ("REFRESH_NO_DESC", 4), ("REFRESH_NO_CENTRE", 8), ("REFRESH_NO_REF", 16),
                        ("REFRESH_UNKNOWN", 32), ("REFRESH_BAD", 64)):
        assert int(re.search(r"#define ORBGPU_%s (\S+)" % name, header).group(1), 0) == value == getattr(G, name)
    for method in ("set_scale_factors", "set_descriptors", "set_centres", "refresh_points"):
        assert callable(getattr(G.CovisibilityGraph, method))
    assert callable(G.MapPointTable.refresh)


def test_header_compiles_as_c_with_the_new_declarations(tmp_path):
    src = tmp_path / "refresh_c99.c"
    src.write_text('#include "orbgpu.h"\n'
                   'int main(void) {\n'
                   '    orbgpu_covis_refresh_result r = {0};\n'
                   '    int (*f)(orbgpu_covis_graph *, int32_t, const int64_t *, const int64_t *, const float *, uint32_t, float *, float *,\n'
                   '             float *, uint8_t *, int64_t *, int32_t *, int32_t *, uint8_t *, orbgpu_covis_refresh_result *) =\n'
                   '        orbgpu_covis_refresh_points;\n'
                   '    return (f != 0 && sizeof r == 48 && ORBGPU_COVIS_REFRESH_MAX_OBS == 1024 &&\n'
                   '            (ORBGPU_REFRESH_DESCRIPTOR | ORBGPU_REFRESH_NORMAL_DEPTH) == 3) ? 0 : 1;\n}\n')
    pkg = os.path.join(ROOT, "orb_slam2_map_amd")
    exe = str(tmp_path / "refresh_c99")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-o", exe, "-L" + pkg, "-lorbgpu", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert subprocess.run([exe]).returncode == 0


def test_refusals_need_no_device_and_change_nothing(G):
    g = G.CovisibilityGraph(initial_rows=2, initial_slots=8)
    L = G.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    try:
        # set_scale_factors
        refused(G, lambda: g.set_scale_factors([]), "n_levels = 0 (1 to 16)")
        refused(G, lambda: g.set_scale_factors(np.ones(17)), "n_levels = 17 (1 to 16)")
        refused(G, lambda: g.set_scale_factors([1.0, 0.0]), "scale factor 0 at level 1")
        refused(G, lambda: g.set_scale_factors([1.0, -1.2]), "at level 1")
        refused(G, lambda: g.set_scale_factors([np.nan]), "at level 0")
        refused(G, lambda: g.set_scale_factors([1.0, 1.2, np.inf]), "at level 2")
        assert L.orbgpu_covis_graph_set_scale_factors(g.h, 2, None) == G.EINVAL
        assert L.orbgpu_covis_graph_set_scale_factors(None, 1, p(np.ones(1, np.float32))) == G.EINVAL
        g.set_scale_factors([1.0, 1.2])  # host only: no device needed; and again
        g.set_scale_factors(1.2 ** np.arange(16))
        # set_descriptors: an unknown id (nothing is a row yet), with and without an array
        refused(G, lambda: g.set_descriptors(3, np.zeros((2, 32), np.uint8)), "key frame 3 is not in the graph")
        refused(G, lambda: g.set_descriptors(3, None), "key frame 3 is not in the graph")
        assert L.orbgpu_covis_graph_set_descriptors(None, 3, 0, None) == G.EINVAL
        # set_centres: unknown ids are ignored without a device; null arrays and bad counts are refused
        assert g.set_centres([4, 5], np.zeros((2, 3))) == 0 and g.set_centres([], np.zeros((0, 3))) == 0
        ids, c3 = np.array([1, 2], np.int64), np.zeros((2, 3), np.float32)
        assert L.orbgpu_covis_graph_set_centres(g.h, 2, None, p(c3), None) == G.EINVAL
        assert L.orbgpu_covis_graph_set_centres(g.h, 2, p(ids), None, None) == G.EINVAL
        assert L.orbgpu_covis_graph_set_centres(g.h, -1, p(ids), p(c3), None) == G.EINVAL
        assert L.orbgpu_covis_graph_set_centres(g.h, (1 << 20) + 1, p(ids), p(c3), None) == G.EINVAL
        assert L.orbgpu_covis_graph_set_centres(None, 0, None, None, None) == G.EINVAL
        # refresh_points
        pos = np.ones((2, 3), np.float32)
        refused(G, lambda: g.refresh_points([4, 4], [1, 1], pos), "map point id 4 appears twice in one refresh call")
        refused(G, lambda: g.refresh_points([4, -1], [1, 1], pos), "map point id -1 (entry 1)")
        refused(G, lambda: g.refresh_points([4, 5], [1, 1], pos, what=0), "what = 0x0")
        refused(G, lambda: g.refresh_points([4, 5], [1, 1], pos, what=4), "what = 0x4")
        refused(G, lambda: g.refresh_points([4, 5], [1, 1], pos, what=7), "what = 0x7")
        res = G.CovisRefreshResult()
        ns, st = np.zeros(2, np.int32), np.zeros(2, np.uint8)
        args = lambda **kw: [kw.get("g", g.h), kw.get("n", 2), kw.get("ids", p(ids)), kw.get("ref", p(ids)), kw.get("pos", p(pos)), 3,  # noqa: E731
                             None, None, None, None, None, None, kw.get("ns", p(ns)), kw.get("st", p(st)), kw.get("res", C.byref(res))]
        for bad_args in (dict(g=None), dict(n=-1), dict(n=(1 << 20) + 1), dict(ids=None), dict(ref=None), dict(pos=None), dict(ns=None),
                         dict(st=None), dict(res=None)):
            assert L.orbgpu_covis_refresh_points(*args(**bad_args)) == G.EINVAL, bad_args
        # the table form: without a device there is no table; the refusals that come first
        targs = lambda **kw: [kw.get("t", None), kw.get("g", g.h), 2, p(ids), p(ids), 3, None, None, None, None, None, None, p(ns), p(st),  # noqa: E731
                              C.byref(res)]
        assert L.orbgpu_mappoint_table_refresh(*targs()) == G.EINVAL
        assert L.orbgpu_mappoint_table_refresh(*targs(g=None)) == G.EINVAL
        assert g.size() == (0, 0) and g.debug_global_queries() == 0
        # what a graph without rows answers without a device: every point NO_OBS, nothing written
        init = dict(normal=np.full((2, 3), 7.0), min_dist=[1, 2], max_dist=[3, 4], desc=np.full((2, 32), 9))
        out = g.refresh_points([9, 4], [1, 2], pos, initial=init)
        assert out["status"].tolist() == [G.REFRESH_NO_OBS] * 2 and out["n_slots"].tolist() == [0, 0]
        assert out["desc_kf"].tolist() == [-1, -1] and out["desc_idx"].tolist() == [-1, -1]
        assert out["normal"].tolist() == [[7.0] * 3] * 2 and out["min_dist"].tolist() == [1, 2] and out["desc"].tolist() == [[9] * 32] * 2
        assert (out["n_no_obs"], out["n_descriptors"], out["n_normals"], out["n_entries"], out["max_obs"]) == (2, 0, 0, 0, 0)
        assert g.refresh_points([], [], np.zeros((0, 3)))["n_no_obs"] == 0
        g.clear()
        assert g.size() == (0, 0)
    finally:
        g.close()
