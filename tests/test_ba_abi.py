"""The bundle-adjustment entry points (Optimizer::BundleAdjustment, include/orbgpu.h) without a GPU: they exist, the ctypes
mirrors have the header's layout, bad arguments and problems beyond the named capacities are refused before the device is
touched, and without a device the calls fail with EHIP -- never a CPU fallback."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("orbgpu_bundle_adjustment", "orbgpu_bundle_adjustment_device", "orbgpu_bundle_adjustment_batch_device",
           "orbgpu_bundle_adjustment_last_spills")


@pytest.fixture(scope="module")
def glib():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(ROOT, "orb_slam2_map_amd", "liborbgpu.so")):
        ge.build()
    from orb_slam2_map_amd import lib
    return lib


def test_bundle_adjustment_symbols_are_exported(glib):
    L = glib.lib()
    for s in SYMBOLS:
        assert hasattr(L, s) and s in glib.ABI_SYMBOLS, s
    assert L.orbgpu_abi_version() == 1  # symbols were only added
    for f in ("bundle_adjustment", "bundle_adjustment_device", "bundle_adjustment_batch_device", "bundle_adjustment_last_spills",
              "bundle_adjustment_problem"):
        assert callable(getattr(glib, f))


def test_struct_layouts_and_capacities_match_the_header(glib, tmp_path):
    """sizeof / offsetof and the capacity constants as a C compiler sees the header against the ctypes mirrors."""
    members = {"orbgpu_bundle_adjustment_result": glib.BundleAdjustmentResult,
               "orbgpu_bundle_adjustment_problem": glib.BundleAdjustmentProblem}
    lines = []
    for name, cls in members.items():
        lines.append('printf("%s %%d\\n", (int)sizeof(%s));' % (name, name))
        for f, _ in cls._fields_:
            lines.append('printf("%s.%s %%d\\n", (int)offsetof(%s, %s));' % (name, f, name, f))
    for c in ("POSES", "FREE", "POINTS", "EDGES", "ITERATIONS"):
        lines.append('printf("%s %%d\\n", (int)ORBGPU_BA_MAX_%s);' % (c, c))
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
    assert C.sizeof(glib.BundleAdjustmentResult) == 2 * 8 + 8 * 4 and C.sizeof(glib.BundleAdjustmentResult) % 8 == 0
    assert C.sizeof(glib.BundleAdjustmentProblem) == 24 + 17 * 8
    assert tuple(int(out[c]) for c in ("POSES", "FREE", "POINTS", "EDGES", "ITERATIONS")) == (
        glib.BA_MAX_POSES, glib.BA_MAX_FREE, glib.BA_MAX_POINTS, glib.BA_MAX_EDGES, glib.BA_MAX_ITERATIONS) == (
        1024, 256, 65536, 1 << 20, 100)
    # a whole map is not smaller than a local one
    assert glib.BA_MAX_FREE > glib.LBA_MAX_FREE and glib.BA_MAX_POINTS > glib.LBA_MAX_POINTS and glib.BA_MAX_EDGES > glib.LBA_MAX_EDGES
    # the header documents the conventions it is the definition of
    txt = open(os.path.join(ROOT, "include", "orbgpu.h")).read()
    for k in range(1, 8):
        assert re.search(r"\bB%d " % k, txt), "convention B%d missing from the header" % k


def _problem(glib, keep, P=3, M=4, E=6, **over):
    """A well-formed problem whose "device" pointers are host buffers: every call below is refused before they are read,
    or stops at the device selection."""
    levels = 8
    buf = np.zeros(1 << 16, np.uint8)
    d = {"Tcw": np.tile(np.eye(4, dtype=np.float32), (P, 1, 1)), "fixed": np.zeros(max(P, 1), np.uint8),
         "cam": np.tile(np.float32([500, 500, 320, 240, 40]), (P, 1)), "inv_level_sigma2": np.ones((P, levels), np.float32),
         "world_pos": np.ones((M, 3), np.float32), "edge_point": np.arange(E, dtype=np.int32) % max(M, 1),
         "edge_pose": np.arange(E, dtype=np.int32) % max(P, 1), "edge_octave": np.zeros(E, np.int32),
         "edge_xy": np.zeros((E, 2), np.float32), "edge_u_right": np.full(E, -1, np.float32),
         "n_poses": P, "n_points": M, "n_edges": E, "nlevels": levels, "n_iterations": 20, "robust": True}
    for k in ("d_Tcw_d", "d_Tcw", "d_pos_d", "d_pos", "d_not_included", "d_result"):
        d[k] = buf.ctypes.data
    p = glib.bundle_adjustment_problem(d, keep)
    keep.append(buf)
    for k, v in over.items():
        setattr(p, k, v)
    return p


NULLS = tuple({k: None} for k in ("Tcw", "fixed", "cam", "inv_level_sigma2", "world_pos", "edge_point", "edge_pose",
                                  "edge_octave", "edge_xy", "edge_u_right"))
COUNTS = ({"n_poses": -1}, {"n_points": -1}, {"n_edges": -1}, {"nlevels": 0}, {"nlevels": -3}, {"n_iterations": -1},
          {"n_iterations": 101})


def test_device_entry_points_refuse_bad_arguments(glib):
    L = glib.lib()
    one, batch = L.orbgpu_bundle_adjustment_device, L.orbgpu_bundle_adjustment_batch_device
    one.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    batch.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    keep = []
    assert one(None, 0, None) == glib.EINVAL
    assert batch(-1, C.byref(_problem(glib, keep)), 0, None) == glib.EINVAL
    assert batch(65536, C.byref(_problem(glib, keep)), 0, None) == glib.EINVAL
    assert batch(1, None, 0, None) == glib.EINVAL
    outputs = tuple({k: None} for k in ("d_Tcw_d", "d_Tcw", "d_pos_d", "d_pos", "d_not_included", "d_result"))
    for over in NULLS + COUNTS + outputs + ({"nlevels": glib.MAX_LEVELS + 1},):
        p = _problem(glib, keep, **over)
        assert one(C.byref(p), 0, None) == glib.EINVAL, over
        assert batch(1, C.byref(p), 0, None) == glib.EINVAL, over
    assert one(C.byref(_problem(glib, keep, n_iterations=101)), 0, None) == glib.EINVAL
    assert b"n_iterations" in L.orbgpu_last_error_string()
    arr = (glib.BundleAdjustmentProblem * 2)(_problem(glib, keep), _problem(glib, keep, n_edges=-5))
    assert batch(2, arr, 0, None) == glib.EINVAL
    assert b"problem 1" in L.orbgpu_last_error_string()
    L.orbgpu_bundle_adjustment_last_spills.argtypes = [C.c_int32, C.c_void_p]
    assert L.orbgpu_bundle_adjustment_last_spills(0, None) == glib.EINVAL


def test_capacities_are_limits_not_fallbacks(glib):
    """One more than each named capacity is EINVAL (the counts are checked before any array is read); what LBA's capacities
    refuse and these allow passes the argument checks and goes on to the device."""
    L = glib.lib()
    one = L.orbgpu_bundle_adjustment_device
    one.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    keep = []
    for over, what in (({"n_poses": glib.BA_MAX_POSES + 1}, b"pose rows"), ({"n_points": glib.BA_MAX_POINTS + 1}, b"points"),
                       ({"n_edges": glib.BA_MAX_EDGES + 1}, b"edges")):
        assert one(C.byref(_problem(glib, keep, **over)), 0, None) == glib.EINVAL, over
        assert what in L.orbgpu_last_error_string(), over
    # 257 free poses among 258 rows
    p = _problem(glib, keep, P=258, M=4, E=6)
    fixed = np.zeros(258, np.uint8)
    fixed[40] = 1
    keep.append(fixed)
    p.fixed = fixed.ctypes.data
    assert one(C.byref(p), 0, None) == glib.EINVAL and b"257 free poses" in L.orbgpu_last_error_string()
    fixed[41] = 1  # 256: accepted by the checks, so the call gets as far as the device (the outputs here are no device memory)
    if glib.device_count() == 0:
        assert one(C.byref(p), 0, None) == glib.EHIP
        # beyond every LBA capacity, within these
        for over in ({"n_points": glib.LBA_MAX_POINTS + 1}, {"n_edges": glib.LBA_MAX_EDGES + 1}, {"n_iterations": 0},
                     {"n_iterations": 100}):
            # 101 free poses; the device is selected, and found missing, before any array is read
            assert one(C.byref(_problem(glib, keep, P=101, M=4, E=6, **over)), 0, None) == glib.EHIP, over


def test_host_entry_point_refuses_bad_arguments(glib):
    L = glib.lib()
    f = L.orbgpu_bundle_adjustment
    f.argtypes = [C.c_void_p] * 8 + [C.c_int32]
    keep, out = [], np.zeros(1 << 16, np.uint8)
    o = out.ctypes.data
    assert f(None, None, o, o, o, o, o, None, 0) == glib.EINVAL
    pr = _problem(glib, keep)
    assert f(C.byref(pr), None, o, None, o, o, o, None, 0) == glib.EINVAL  # Tcw
    assert f(C.byref(pr), None, o, o, o, None, o, None, 0) == glib.EINVAL  # pos
    assert f(C.byref(pr), None, o, o, o, o, None, None, 0) == glib.EINVAL  # not_included
    for over in NULLS + COUNTS + ({"nlevels": glib.MAX_LEVELS + 1}, {"n_edges": glib.BA_MAX_EDGES + 1}):
        assert f(C.byref(_problem(glib, keep, **over)), None, o, o, o, o, o, None, 0) == glib.EINVAL, over


def test_no_device_means_ehip_not_a_fallback(glib):
    if glib.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = glib.lib()
    keep = []
    L.orbgpu_bundle_adjustment_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    L.orbgpu_bundle_adjustment_batch_device.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    pr = _problem(glib, keep)
    assert L.orbgpu_bundle_adjustment_device(C.byref(pr), 0, None) == glib.EHIP
    assert L.orbgpu_bundle_adjustment_batch_device(1, C.byref(pr), 0, None) == glib.EHIP
    v = C.c_int32()
    L.orbgpu_bundle_adjustment_last_spills.argtypes = [C.c_int32, C.c_void_p]
    assert L.orbgpu_bundle_adjustment_last_spills(0, C.byref(v)) == glib.EHIP
    d = {"Tcw": np.tile(np.eye(4, dtype=np.float32), (2, 1, 1)), "fixed": [1, 0], "cam": np.ones((2, 5), np.float32),
         "inv_level_sigma2": np.ones((2, 8), np.float32), "world_pos": np.ones((3, 3), np.float32), "edge_point": [0, 1, 2],
         "edge_pose": [0, 1, 0], "edge_octave": [0, 0, 0], "edge_xy": np.zeros((3, 2)), "edge_u_right": [-1, -1, -1]}
    with pytest.raises(glib.OrbGpuError) as ei:
        glib.bundle_adjustment(d)
    assert ei.value.status == glib.EHIP
    with pytest.raises(glib.OrbGpuError):
        glib.bundle_adjustment_last_spills()
