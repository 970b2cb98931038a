"""orbgpu_covis_*: every refusal returns ORBGPU_EINVAL with its message before any device is touched, and the state is
what it was.  No GPU: a graph that has stored nothing is host memory only."""
import ctypes as C
import os

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


def test_create_refuses_bad_arguments(G):
    L, h = G.lib(), C.c_void_p()
    assert L.orbgpu_covis_graph_create(0, 0, 0, None) == G.EINVAL
    assert L.orbgpu_covis_graph_create(-1, 0, 0, C.byref(h)) == G.EINVAL and b"device_id" in L.orbgpu_last_error_string()
    assert L.orbgpu_covis_graph_create(0, (1 << 20) + 1, 0, C.byref(h)) == G.EINVAL and b"initial_rows" in L.orbgpu_last_error_string()
    assert L.orbgpu_covis_graph_create(0, 0, (1 << 30) + 1, C.byref(h)) == G.EINVAL and b"initial_slots" in L.orbgpu_last_error_string()
    assert L.orbgpu_covis_graph_create(0, -1, 0, C.byref(h)) == G.EINVAL and not h.value


def test_refusals_need_no_device_and_change_nothing(G):
    g = G.CovisibilityGraph(initial_rows=2, initial_slots=8)
    try:
        assert g.size() == (0, 0)
        refused(G, lambda: g.add_keyframe(-1, 4), "key frame id -1")
        refused(G, lambda: g.add_keyframe(3, -1), "n_slots = -1")
        refused(G, lambda: g.add_keyframe(3, G.CovisibilityGraph.MAX_SLOTS + 1), "n_slots = 65537 (at most 65536)")
        refused(G, lambda: g.add_keyframe(3, 2, [5, -2]), "map point id -2 at slot 1")
        refused(G, lambda: g.set_covisibles(3, list(range(11))), "11 covisibles (at most 10)")
        refused(G, lambda: g.set_covisibles(3, [4, -1]), "covisible id -1")
        refused(G, lambda: g.set_covisibles(-3, [4]), "key frame id -3")
        refused(G, lambda: g.set_parent(-1, 2), "key frame -1, parent 2")
        refused(G, lambda: g.set_parent(1, -2), "key frame 1, parent -2")
        refused(G, lambda: g.set_slots([1], [0], [-2]), "map point id -2 (entry 0)")
        refused(G, lambda: g.local_map(np.zeros(G.CovisibilityGraph.MAX_SLOTS + 1, np.int64), [], 0, 0), "n_kp = 65537")
        L = G.lib()
        res = G.CovisLocalMapResult()
        assert L.orbgpu_covis_local_map(g.h, 1, None, 0, None, 0, None, 0, None, C.byref(res)) == G.EINVAL
        assert L.orbgpu_covis_local_map(g.h, 0, None, 0, None, 1, None, 0, None, C.byref(res)) == G.EINVAL
        assert b"capacity" in L.orbgpu_last_error_string()
        assert L.orbgpu_covis_local_map(g.h, 0, None, 0, None, 0, None, 0, None, None) == G.EINVAL
        n = C.c_int32()
        assert L.orbgpu_covis_connections(g.h, 1, 15, 1, None, None, C.byref(n), 0, None, None, C.byref(n)) == G.EINVAL
        assert L.orbgpu_covis_graph_set_slots(g.h, -1, None, None, None, None) == G.EINVAL
        assert L.orbgpu_covis_graph_set_bad(g.h, 1, None, None) == G.EINVAL
        assert L.orbgpu_covis_graph_size(g.h, None, None) == G.EINVAL
        assert g.size() == (0, 0)
        # what an empty graph answers without a device: unknown key frames are ignored, queries are empty
        assert g.set_slots([1, 2], [0, 99], [5, 6]) == 0 and g.set_bad([1, 2]) == 0
        g.set_parent(7, 3)
        g.set_covisibles(7, [1, 2, 3])  # kept for when key frame 7 is added
        out = g.local_map([5, -1, 5], [4, 9])
        assert out["kept_previous"] == 1 and out["n_unknown_previous"] == 2 and out["n_kfs"] == 0 and out["n_points"] == 0
        assert out["ref_kf"] == -1 and out["kf_ids"].size == 0 and out["point_ids"].size == 0
        c = g.connections(7, 15)
        assert c["n"] == 0 and c["n_ordered"] == 0
        assert g.debug_global_queries() == 0
        g.clear()
        assert g.size() == (0, 0)
    finally:
        g.close()

