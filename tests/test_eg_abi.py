"""The essential-graph entry points (Optimizer::OptimizeEssentialGraph, include/orbgpu.h) without a GPU: they exist, the
ctypes mirrors have the header's layout, G1-G12 are written down, bad arguments, problems beyond the named capacities and an
envelope above its cap are refused before the device is touched, and without a device the calls fail with EHIP -- never a
CPU fallback."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
SYMBOLS = ("orbgpu_essential_graph", "orbgpu_essential_graph_device", "orbgpu_essential_graph_batch_device",
           "orbgpu_essential_graph_correct_points_device", "orbgpu_sim3_from_pose")
POINTS_ARGS = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
HOST_ARGS = [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 4 + [C.c_int32]


@pytest.fixture(scope="module")
def glib():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(ROOT, "orb_slam2_map_amd", "liborbgpu.so")):
        ge.build()
    from orb_slam2_map_amd import lib
    return lib


def test_essential_graph_symbols_are_exported(glib):
    L = glib.lib()
    for s in SYMBOLS:
        assert hasattr(L, s) and s in glib.ABI_SYMBOLS, s
    assert L.orbgpu_abi_version() == 1  # symbols were only added
    for f in ("essential_graph", "essential_graph_device", "essential_graph_batch_device", "essential_graph_problem",
              "essential_graph_correct_points_device", "sim3_from_pose"):
        assert callable(getattr(glib, f))


def test_struct_layouts_and_capacities_match_the_header(glib, tmp_path):
    """sizeof / offsetof and the capacity constants as a C compiler sees the header against the ctypes mirrors."""
    members = {"orbgpu_essential_graph_result": glib.EssentialGraphResult,
               "orbgpu_essential_graph_problem": glib.EssentialGraphProblem}
    caps = ("VERTICES", "EDGES", "POINTS", "ENVELOPE", "ITERATIONS")
    lines = []
    for name, cls in members.items():
        lines.append('printf("%s %%d\\n", (int)sizeof(%s));' % (name, name))
        for f, _ in cls._fields_:
            lines.append('printf("%s.%s %%d\\n", (int)offsetof(%s, %s));' % (name, f, name, f))
    for c in caps:
        lines.append('printf("%s %%d\\n", (int)ORBGPU_EG_MAX_%s);' % (c, c))
    src = tmp_path / "layout.c"
    src.write_text('#include "orbgpu.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n' + "\n".join(lines) +
                   "\nreturn 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-o", exe], check=True)
    out = dict(l.split() for l in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines())
    for name, cls in members.items():
        assert int(out[name]) == C.sizeof(cls), name
        for f, _ in cls._fields_:
            assert int(out["%s.%s" % (name, f)]) == getattr(cls, f).offset, (name, f)
    assert C.sizeof(glib.EssentialGraphResult) == 2 * 8 + 10 * 4 and C.sizeof(glib.EssentialGraphResult) % 8 == 0
    assert C.sizeof(glib.EssentialGraphProblem) == 16 + 10 * 8
    assert tuple(int(out[c]) for c in caps) == (glib.EG_MAX_VERTICES, glib.EG_MAX_EDGES, glib.EG_MAX_POINTS, glib.EG_MAX_ENVELOPE,
                                                glib.EG_MAX_ITERATIONS) == (8192, 1 << 18, 1 << 22, 1 << 26, 100)
    import eg_model
    assert (eg_model.MAX_VERTICES, eg_model.MAX_EDGES, eg_model.MAX_POINTS, eg_model.MAX_ENVELOPE, eg_model.MAX_ITERATIONS) == (
        glib.EG_MAX_VERTICES, glib.EG_MAX_EDGES, glib.EG_MAX_POINTS, glib.EG_MAX_ENVELOPE, glib.EG_MAX_ITERATIONS)
    # the result holds what the issue names
    assert [f for f, _ in glib.EssentialGraphResult._fields_][:11] == [
        "chi2_start", "chi2_end", "iterations", "trials", "stopped", "n_edges", "n_bad_index", "n_free_active", "envelope",
        "bandwidth", "n_bad_ref"]
    # the header documents the conventions it is the definition of
    txt = open(os.path.join(ROOT, "include", "orbgpu.h")).read()
    for k in range(1, 13):
        assert re.search(r"\bG%d " % k, txt), "convention G%d missing from the header" % k
    src = open(os.path.join(ROOT, "orb_slam2_map_amd", "csrc", "essential_graph.hip")).read()
    assert "EG_THREADS = %d" % eg_model.THREADS in src


def test_sim3_from_pose_is_the_models(glib):
    import eg_model
    rng = np.random.default_rng(3)
    for _ in range(5):
        q, _ = np.linalg.qr(rng.normal(0, 1, (3, 3)))
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = (q * np.sign(np.linalg.det(q))).astype(np.float32)
        T[:3, 3] = rng.normal(0, 2, 3).astype(np.float32)
        assert glib.sim3_from_pose(T).tobytes() == eg_model.state_from_pose(T).tobytes()
    L = glib.lib()
    L.orbgpu_sim3_from_pose.argtypes = [C.c_void_p, C.c_void_p]
    buf = np.zeros(16, np.float64)
    assert L.orbgpu_sim3_from_pose(None, buf.ctypes.data) == glib.EINVAL
    assert L.orbgpu_sim3_from_pose(buf.ctypes.data, None) == glib.EINVAL


def _problem(glib, keep, V=4, E=5, **over):
    """A well-formed problem whose "device" pointers are host buffers: every call below is refused before they are read,
    or stops at the device selection."""
    buf = np.zeros(1 << 16, np.uint8)
    S = np.tile(np.float64([0, 0, 0, 1, 0, 0, 0, 1]), (max(V, 1), 1))
    fixed = np.zeros(max(V, 1), np.uint8)
    fixed[0] = 1
    d = {"Scw": S, "Snc": S.copy(), "fixed": fixed, "edge_i": np.arange(E, dtype=np.int32) % max(V, 1),
         "edge_j": (np.arange(E, dtype=np.int32) + 1) % max(V, 1), "edge_kind": np.ones(E, np.int32),
         "n_vertices": V, "n_edges": E, "n_iterations": 20, "fix_scale": False}
    for k in ("d_Siw_d", "d_Tiw", "d_result"):
        d[k] = buf.ctypes.data
    p = glib.essential_graph_problem(d, keep)
    keep.append(buf)
    for k, v in over.items():
        setattr(p, k, v)
    return p


NULLS = tuple({k: None} for k in ("Scw", "Snc", "fixed", "edge_i", "edge_j", "edge_kind"))
COUNTS = ({"n_vertices": -1}, {"n_edges": -1}, {"n_iterations": -1}, {"n_iterations": 101})


def test_device_entry_points_refuse_bad_arguments(glib):
    L = glib.lib()
    one, batch = L.orbgpu_essential_graph_device, L.orbgpu_essential_graph_batch_device
    one.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    batch.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    keep = []
    assert one(None, 0, None) == glib.EINVAL
    assert batch(-1, C.byref(_problem(glib, keep)), 0, None) == glib.EINVAL
    assert batch(65536, C.byref(_problem(glib, keep)), 0, None) == glib.EINVAL
    assert batch(1, None, 0, None) == glib.EINVAL
    outputs = tuple({k: None} for k in ("d_Siw_d", "d_Tiw", "d_result"))
    for over in NULLS + COUNTS + outputs:
        p = _problem(glib, keep, **over)
        assert one(C.byref(p), 0, None) == glib.EINVAL, over
        assert batch(1, C.byref(p), 0, None) == glib.EINVAL, over
    assert one(C.byref(_problem(glib, keep, n_iterations=101)), 0, None) == glib.EINVAL
    assert b"n_iterations" in L.orbgpu_last_error_string()
    arr = (glib.EssentialGraphProblem * 2)(_problem(glib, keep), _problem(glib, keep, n_edges=-5))
    assert batch(2, arr, 0, None) == glib.EINVAL
    assert b"problem 1" in L.orbgpu_last_error_string()


def test_capacities_and_the_envelope_cap_are_limits_not_fallbacks(glib):
    """One more than each named capacity is EINVAL (the counts are checked before any array is read), and so is a graph
    whose envelope does not fit -- found on the host, from the ordering alone."""
    L = glib.lib()
    one = L.orbgpu_essential_graph_device
    one.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    keep = []
    for over, what in (({"n_vertices": glib.EG_MAX_VERTICES + 1}, b"vertices"), ({"n_edges": glib.EG_MAX_EDGES + 1}, b"edges")):
        assert one(C.byref(_problem(glib, keep, **over)), 0, None) == glib.EINVAL, over
        assert what in L.orbgpu_last_error_string(), over
    # 8192 vertices joined at random: no ordering keeps 60 000 edges near the diagonal
    rng = np.random.default_rng(7)
    V, E = glib.EG_MAX_VERTICES, 60000
    p = _problem(glib, keep, V=V, E=E)
    ei, ej = rng.integers(0, V, E).astype(np.int32), rng.integers(0, V, E).astype(np.int32)
    keep += [ei, ej]
    p.edge_i, p.edge_j = ei.ctypes.data, ej.ctypes.data
    assert one(C.byref(p), 0, None) == glib.EINVAL
    msg = L.orbgpu_last_error_string()
    assert b"envelope" in msg and str(glib.EG_MAX_ENVELOPE).encode() in msg
    # the same rows as a chain have an envelope of 14 rows per key frame: accepted by the checks, so the call gets as far
    # as the device (the outputs here are no device memory)
    if glib.device_count() == 0:
        assert one(C.byref(_problem(glib, keep, V=V, E=V - 1)), 0, None) == glib.EHIP
        for over in ({"n_iterations": 0}, {"n_iterations": 100}, {"n_vertices": 0, "n_edges": 0}):
            assert one(C.byref(_problem(glib, keep, **over)), 0, None) == glib.EHIP, over
    # the points call
    f = L.orbgpu_essential_graph_correct_points_device
    f.argtypes = POINTS_ARGS
    o = np.zeros(1 << 12, np.uint8).ctypes.data
    for nv, npts in ((-1, 4), (4, -1), (glib.EG_MAX_VERTICES + 1, 4), (4, glib.EG_MAX_POINTS + 1)):
        assert f(nv, o, o, npts, o, o, o, None, 0, None) == glib.EINVAL, (nv, npts)
    for k in range(5):
        args = [o] * 5
        args[k] = None
        assert f(4, args[0], args[1], 4, args[2], args[3], args[4], None, 0, None) == glib.EINVAL, k
    if glib.device_count() == 0:
        assert f(4, o, o, 4, o, o, o, None, 0, None) == glib.EHIP


def test_host_entry_point_refuses_bad_arguments(glib):
    L = glib.lib()
    f = L.orbgpu_essential_graph
    f.argtypes = HOST_ARGS
    keep, out = [], np.zeros(1 << 16, np.uint8)
    o = out.ctypes.data
    assert f(None, None, o, o, 0, None, None, None, None, 0) == glib.EINVAL
    pr = _problem(glib, keep)
    assert f(C.byref(pr), None, o, None, 0, None, None, None, None, 0) == glib.EINVAL  # Tiw
    assert f(C.byref(pr), None, o, o, -1, o, o, o, None, 0) == glib.EINVAL
    assert f(C.byref(pr), None, o, o, glib.EG_MAX_POINTS + 1, o, o, o, None, 0) == glib.EINVAL
    for k in range(3):  # world_pos, point_ref, pos_out
        args = [o, o, o]
        args[k] = None
        assert f(C.byref(pr), None, o, o, 3, args[0], args[1], args[2], None, 0) == glib.EINVAL, k
    for over in NULLS + COUNTS + ({"n_edges": glib.EG_MAX_EDGES + 1}, {"n_vertices": glib.EG_MAX_VERTICES + 1}):
        assert f(C.byref(_problem(glib, keep, **over)), None, o, o, 0, None, None, None, None, 0) == glib.EINVAL, over


def test_no_device_means_ehip_not_a_fallback(glib):
    if glib.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = glib.lib()
    keep = []
    L.orbgpu_essential_graph_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    L.orbgpu_essential_graph_batch_device.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    pr = _problem(glib, keep)
    assert L.orbgpu_essential_graph_device(C.byref(pr), 0, None) == glib.EHIP
    assert L.orbgpu_essential_graph_batch_device(1, C.byref(pr), 0, None) == glib.EHIP
    S = np.tile(np.float64([0, 0, 0, 1, 0, 0, 0, 1]), (3, 1))
    d = {"Scw": S, "Snc": S, "fixed": [1, 0, 0], "edge_i": [0, 1], "edge_j": [1, 2], "edge_kind": [1, 1]}
    with pytest.raises(glib.OrbGpuError) as ei:
        glib.essential_graph(d, world_pos=np.ones((2, 3), np.float32), point_ref=[0, 1])
    assert ei.value.status == glib.EHIP
