"""orbgpu_covis_graph_set_keypoints, orbgpu_covis_observations, orbgpu_covis_keyframe_culling: the symbols and the result
struct through lib.py, and every refusal answered with ORBGPU_EINVAL and its message before any device is touched, the graph
being what it was.  No GPU: a graph that has stored nothing is host memory only.  (set_keypoints' refusals that need a row
-- a wrong n_slots, a reserved bit, a null array -- are answered as early, but a row needs a device to exist: they are in
tests/test_gpu_cull.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    for name in ("orbgpu_covis_graph_set_keypoints", "orbgpu_covis_observations", "orbgpu_covis_keyframe_culling"):
        assert name in G.ABI_SYMBOLS and hasattr(L, name)
    header = open(os.path.join(ROOT, "include", "orbgpu.h")).read()
    m = re.search(r"typedef struct orbgpu_covis_culling_result \{(.*?)\} orbgpu_covis_culling_result;", header, re.S)
    assert m, "the header does not declare the result struct"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.replace("int32_t", "").split(",")]
    assert fields == [name for name, _ in G.CovisCullingResult._fields_]
    assert all(t is C.c_int32 for _, t in G.CovisCullingResult._fields_) and C.sizeof(G.CovisCullingResult) == 20
    for name, value in (("MAX_LEVELS", 16), ("KP_STEREO", 0x40), ("KP_FAR", 0x80)):
        assert re.search(r"#define ORBGPU_COVIS_%s (\S+)" % name, header).group(1) in (str(value), hex(value))
        assert getattr(G.CovisibilityGraph, name) == value


def test_refusals_need_no_device_and_change_nothing(G):
    g = G.CovisibilityGraph(initial_rows=2, initial_slots=8)
    L = G.lib()
    try:
        # set_keypoints: an unknown id (nothing is a row yet), with and without an array
        refused(G, lambda: g.set_keypoints(3, [0, 0]), "key frame 3 is not in the graph")
        refused(G, lambda: g.set_keypoints(3, None), "key frame 3 is not in the graph")
        assert L.orbgpu_covis_graph_set_keypoints(None, 3, 0, None) == G.EINVAL
        # observations
        refused(G, lambda: g.observations([4, -2, 5]), "map point id -2 (entry 1)")
        out = np.zeros(4, np.int32)
        ids = np.array([1, 2], np.int64)
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        assert L.orbgpu_covis_observations(g.h, -1, p(ids), p(out), p(out)) == G.EINVAL
        assert L.orbgpu_covis_observations(g.h, (1 << 20) + 1, p(ids), p(out), p(out)) == G.EINVAL
        assert L.orbgpu_covis_observations(g.h, 2, None, p(out), p(out)) == G.EINVAL
        assert L.orbgpu_covis_observations(g.h, 2, p(ids), None, p(out)) == G.EINVAL
        assert L.orbgpu_covis_observations(g.h, 2, p(ids), p(out), None) == G.EINVAL
        assert L.orbgpu_covis_observations(None, 0, None, None, None) == G.EINVAL
        # keyframe_culling
        refused(G, lambda: g.keyframe_culling([1, -1]), "key frame id -1 (entry 1)")
        refused(G, lambda: g.keyframe_culling([1], th_obs=0), "th_obs = 0 (1 to 255)")
        refused(G, lambda: g.keyframe_culling([1], th_obs=256), "th_obs = 256 (1 to 255)")
        refused(G, lambda: g.keyframe_culling(np.ones((1 << 16) + 1, np.int64)), "n = 65537 (at most 65536)")
        res = G.CovisCullingResult()
        v, a, b, bad = np.zeros(2, np.int8), np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(2, np.int64)
        args = lambda **kw: [kw.get("g", g.h), kw.get("n", 2), kw.get("ids", p(ids)), None, 3, kw.get("v", p(v)), kw.get("a", p(a)),  # noqa: E731
                             kw.get("b", p(b)), kw.get("cap", 2), kw.get("bad", p(bad)), kw.get("res", C.byref(res))]
        for bad_args in (dict(g=None), dict(n=-1), dict(ids=None), dict(v=None), dict(a=None), dict(b=None), dict(bad=None),
                         dict(cap=-1), dict(res=None)):
            assert L.orbgpu_covis_keyframe_culling(*args(**bad_args)) == G.EINVAL, bad_args
        assert L.orbgpu_covis_keyframe_culling(*args(cap=0, bad=None)) == 0  # no room asked for: no array needed
        assert g.size() == (0, 0) and g.debug_global_queries() == 0
        # what a graph without rows answers without a device: zeros, every candidate skipped
        obs, cnt = g.observations([5, -1, 5])
        assert obs.tolist() == [0, 0, 0] and cnt.tolist() == [0, 0, 0]
        out = g.keyframe_culling([4, 0, 4], [1, 0, 0])
        assert out["verdict"].tolist() == [-1, -1, -1] and out["n_mps"].tolist() == [0, 0, 0] and out["n_redundant"].tolist() == [0, 0, 0]
        assert (out["n_culled"], out["n_to_be_erased"], out["n_skipped"], out["n_points_bad"], out["n_query_points"]) == (0, 0, 3, 0, 0)
        assert g.keyframe_culling([])["n_skipped"] == 0
        g.clear()
        assert g.size() == (0, 0)
    finally:
        g.close()
