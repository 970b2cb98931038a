"""The CreateNewMapPoints entry points (include/orbgpu.h) without a GPU: they exist, the ctypes mirrors have the header's
layout, bad arguments and problems beyond the limits are refused before the device is touched, and without a device the
calls fail with EHIP -- never a CPU fallback."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import newpts_model as M  # noqa: E402

SYMBOLS = ("orbgpu_create_new_map_points", "orbgpu_create_new_map_points_device")


@pytest.fixture(scope="module")
def glib():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(ROOT, "orb_slam2_map_amd", "liborbgpu.so")):
        ge.build()
    from orb_slam2_map_amd import lib
    return lib


def test_symbols_are_exported(glib):
    L = glib.lib()
    for s in SYMBOLS:
        assert hasattr(L, s) and s in glib.ABI_SYMBOLS, s
    assert L.orbgpu_abi_version() == 1  # symbols were only added
    for f in ("create_new_map_points", "create_new_map_points_device", "new_points_problem", "new_points_frame"):
        assert callable(getattr(glib, f))


def test_struct_layouts_limits_and_codes_match_the_header(glib, tmp_path):
    members = {"orbgpu_new_points_frame": glib.NewPointsFrame, "orbgpu_new_points_problem": glib.NewPointsProblem}
    codes = {"NONE": glib.NP_NONE, "TRIANGULATED": glib.NP_TRIANGULATED, "UNPROJECT1": glib.NP_UNPROJECT1,
             "UNPROJECT2": glib.NP_UNPROJECT2, "LOW_PARALLAX": glib.NP_LOW_PARALLAX, "W_ZERO": glib.NP_W_ZERO, "Z1": glib.NP_Z1,
             "Z2": glib.NP_Z2, "REPROJ1": glib.NP_REPROJ1, "REPROJ2": glib.NP_REPROJ2, "ZERO_DIST": glib.NP_ZERO_DIST,
             "SCALE": glib.NP_SCALE, "NON_FINITE": glib.NP_NON_FINITE, "STEREO_DEPTH": glib.NP_STEREO_DEPTH,
             "BAD_OCTAVE": glib.NP_BAD_OCTAVE}
    lines = []
    for name, cls in members.items():
        lines.append('printf("%s %%d\\n", (int)sizeof(%s));' % (name, name))
        for f, _ in cls._fields_:
            lines.append('printf("%s.%s %%d\\n", (int)offsetof(%s, %s));' % (name, f, name, f))
    lines.append('printf("MAXN %d\\n", (int)ORBGPU_NEW_POINTS_MAX_NEIGHBOURS);')
    for c in codes:
        lines.append('printf("%s %%d\\n", (int)ORBGPU_NP_%s);' % (c, c))
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
    assert C.sizeof(glib.NewPointsFrame) == 8 + 11 * 8 + 4 * (32 + 7 + 2 * glib.MAX_LEVELS + 11)
    assert C.sizeof(glib.NewPointsProblem) == C.sizeof(glib.NewPointsFrame) + 8 + 16 + 7 * 8
    assert int(out["MAXN"]) == glib.NEW_POINTS_MAX_NEIGHBOURS == 32
    for c, v in codes.items():
        assert int(out[c]) == v, c
    # the model's codes are the header's, and the ten rejections and three creations are distinct
    assert (M.NONE, M.TRIANGULATED, M.UNPROJECT1, M.UNPROJECT2, M.LOW_PARALLAX, M.W_ZERO, M.Z1, M.Z2, M.REPROJ1, M.REPROJ2,
            M.ZERO_DIST, M.SCALE, M.NON_FINITE, M.STEREO_DEPTH, M.BAD_OCTAVE) == tuple(codes.values())
    assert len(set(codes.values())) == len(codes)
    txt = open(os.path.join(ROOT, "include", "orbgpu.h")).read()
    for k in range(1, 14):
        assert re.search(r"\bN%d " % k, txt), "convention N%d missing from the header" % k
    assert "vs CPU restatement; OpenCV boundary unpinned" in txt


def _problem(glib, keep, sc=None, device_outputs=True, **over):
    """A well-formed problem over host buffers: every call below is refused before they are read, or stops at the device
    selection."""
    sc = sc or M.scene("nn=1")
    buf = np.zeros(1 << 16, np.uint8)
    keep.append(buf)
    ptrs = {k: buf.ctypes.data for k in ("match12", "status", "x3d", "n_matches", "n_created", "n_done")}
    q = glib.new_points_problem(sc["kf1"], sc["neighbours"], sc["ratio_factor"], False, True, keep, False, **ptrs)
    for k, v in over.items():
        obj, _, field = k.rpartition(".")
        setattr(getattr(q, obj) if obj else q, field, v)
    return q


BAD = ({"nn": -1}, {"nn": 33}, {"neighbours": None}, {"n_done": None}, {"n_matches": None}, {"n_created": None},
       {"match12": None}, {"status": None}, {"x3d": None}, {"kf1.n": -1}, {"kf1.n": 65536}, {"kf1.nlevels": 0},
       {"kf1.nlevels": 17}, {"kf1.kp_x": None}, {"kf1.kp_octave": None}, {"kf1.desc": None}, {"kf1.has_mp": None},
       {"kf1.node": None}, {"kf1.depth": None}, {"kf1.cos_stereo": None}, {"kf1.u_right": None}, {"kf1.kp_angle": None})


def test_both_entry_points_refuse_bad_arguments(glib):
    L = glib.lib()
    dev, host = L.orbgpu_create_new_map_points_device, L.orbgpu_create_new_map_points
    dev.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    host.argtypes = [C.c_void_p, C.c_int32]
    keep = []
    assert dev(None, 0, None) == glib.EINVAL and host(None, 0) == glib.EINVAL
    for over in BAD:
        q = _problem(glib, keep, **over)
        assert dev(C.byref(q), 0, None) == glib.EINVAL, over
        assert host(C.byref(q), 0) == glib.EINVAL, over
    # a neighbour is checked like key frame 1, and named
    sc = M.scene("mixed")
    q = _problem(glib, keep, sc)
    arr = C.cast(q.neighbours, C.POINTER(glib.NewPointsFrame))
    arr[2].n = 70000
    assert dev(C.byref(q), 0, None) == glib.EINVAL and b"neighbour 2" in L.orbgpu_last_error_string()
    # the host flavour sees the octaves
    sc = M.scene("nn=1")
    sc["neighbours"][0]["kp_octave"][5] = 8
    assert host(C.byref(_problem(glib, keep, sc)), 0) == glib.EINVAL and b"octave" in L.orbgpu_last_error_string()
    # angles are only needed for the orientation check
    q = _problem(glib, keep, **{"kf1.kp_angle": None, "check_orientation": 0})
    if glib.device_count() == 0:
        assert dev(C.byref(q), 0, None) == glib.EHIP


def test_the_limits_themselves_are_accepted(glib):
    """32 neighbours pass the argument checks and go on to the device"""
    if glib.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = glib.lib()
    sc = M.scene("nn=1")
    sc["neighbours"] = sc["neighbours"] * 32
    keep = []
    L.orbgpu_create_new_map_points.argtypes = [C.c_void_p, C.c_int32]
    assert L.orbgpu_create_new_map_points(C.byref(_problem(glib, keep, sc)), 0) == glib.EHIP


def test_no_device_means_ehip_not_a_fallback(glib):
    if glib.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = glib.lib()
    keep = []
    L.orbgpu_create_new_map_points_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    assert L.orbgpu_create_new_map_points_device(C.byref(_problem(glib, keep)), 0, None) == glib.EHIP
    sc = M.scene("nn=1")
    with pytest.raises(glib.OrbGpuError) as ei:
        glib.create_new_map_points(sc["kf1"], sc["neighbours"], sc["ratio_factor"])
    assert ei.value.status == glib.EHIP
