"""The Sim3-optimisation entry points (Optimizer::OptimizeSim3, include/orbgpu.h) without a GPU: they exist, the ctypes
mirrors have the header's layout, bad arguments are refused before the device is touched, and without a device the calls
fail with EHIP -- never a CPU fallback."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("orbgpu_sim3_optimize", "orbgpu_sim3_optimize_device", "orbgpu_sim3_optimize_batch_device",
           "orbgpu_sim3_opt_last_spills")


@pytest.fixture(scope="module")
def glib():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(ROOT, "orb_slam2_map_amd", "liborbgpu.so")):
        ge.build()
    from orb_slam2_map_amd import lib
    return lib


def test_sim3opt_symbols_are_exported(glib):
    L = glib.lib()
    for s in SYMBOLS:
        assert hasattr(L, s) and s in glib.ABI_SYMBOLS, s
    assert L.orbgpu_abi_version() == 1  # symbols were only added
    for f in ("sim3_optimize", "sim3_optimize_device", "sim3_optimize_batch_device", "sim3_opt_last_spills"):
        assert callable(getattr(glib, f))


def test_struct_layouts_match_the_header(glib, tmp_path):
    """sizeof / offsetof as a C compiler sees the header against the ctypes mirrors, every member."""
    members = {"orbgpu_sim3_opt_result": glib.Sim3OptResult, "orbgpu_sim3_opt_problem": glib.Sim3OptProblem}
    lines = []
    for name, cls in members.items():
        lines.append('printf("%s %%d\\n", (int)sizeof(%s));' % (name, name))
        for f, _ in cls._fields_:
            lines.append('printf("%s.%s %%d\\n", (int)offsetof(%s, %s));' % (name, f, name, f))
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
    assert C.sizeof(glib.Sim3OptResult) == 13 * 8 + 13 * 4 + 32 * 4 + 7 * 4 and C.sizeof(glib.Sim3OptResult) % 8 == 0
    assert glib.Sim3OptProblem.T1w.offset == 64 and glib.Sim3OptProblem.inlier.offset == 288 + 64
    # the header documents the conventions it is the definition of
    txt = open(os.path.join(ROOT, "include", "orbgpu.h")).read()
    for k in range(1, 10):
        assert re.search(r"\bO%d " % k, txt), "convention O%d missing from the header" % k


def _problem(glib, keep, **over):
    """A well-formed problem whose "device" pointers are host buffers: every call below is refused before they are read,
    or stops at the device selection."""
    buf = np.zeros(4096, np.uint8)
    p = glib.sim3_opt_problem({"n1": 16, "T1w": np.eye(4), "T2w": np.eye(4), "K1": (500, 500, 320, 240), "K2": (500, 500, 320, 240),
                               "inv_level_sigma2": np.ones(8, np.float32), "R12": np.eye(3), "t12": np.zeros(3), "s12": 1.0,
                               "th2": 10.0, "fix_scale": False})
    for k in ("valid", "Xw1", "Xw2", "octave1", "octave2", "kp1_xy", "kp2_xy", "inlier", "result"):
        setattr(p, k, buf.ctypes.data)
    keep.append(buf)
    for k, v in over.items():
        setattr(p, k, v)
    return p


BAD = ({"valid": None}, {"Xw1": None}, {"Xw2": None}, {"octave1": None}, {"octave2": None}, {"kp1_xy": None}, {"kp2_xy": None},
       {"n1": -1}, {"n1": 65537}, {"nlevels": 0}, {"nlevels": -3})


def test_device_entry_points_refuse_bad_arguments(glib):
    L = glib.lib()
    one, batch = L.orbgpu_sim3_optimize_device, L.orbgpu_sim3_optimize_batch_device
    one.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    batch.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    keep = []
    assert one(None, 0, None) == glib.EINVAL
    assert batch(-1, C.byref(_problem(glib, keep)), 0, None) == glib.EINVAL
    assert batch(1, None, 0, None) == glib.EINVAL
    for over in BAD + ({"inlier": None}, {"result": None}, {"nlevels": glib.MAX_LEVELS + 1}):
        p = _problem(glib, keep, **over)
        assert one(C.byref(p), 0, None) == glib.EINVAL, over
        assert batch(1, C.byref(p), 0, None) == glib.EINVAL, over
    # the second problem of a batch is checked too
    arr = (glib.Sim3OptProblem * 2)(_problem(glib, keep), _problem(glib, keep, n1=1 << 20))
    assert batch(2, arr, 0, None) == glib.EINVAL
    assert b"problem 1" in L.orbgpu_last_error_string()
    L.orbgpu_sim3_opt_last_spills.argtypes = [C.c_int32, C.c_void_p]
    assert L.orbgpu_sim3_opt_last_spills(0, None) == glib.EINVAL


def test_host_entry_point_refuses_bad_arguments(glib):
    L = glib.lib()
    f = L.orbgpu_sim3_optimize
    f.argtypes = [C.c_void_p] * 4 + [C.c_int32]
    keep, ni, inl = [], C.c_int32(), np.zeros(4096, np.uint8)
    assert f(None, inl.ctypes.data, C.addressof(ni), None, 0) == glib.EINVAL
    assert f(C.byref(_problem(glib, keep)), inl.ctypes.data, None, None, 0) == glib.EINVAL
    assert f(C.byref(_problem(glib, keep)), None, C.addressof(ni), None, 0) == glib.EINVAL
    for over in BAD + ({"nlevels": glib.MAX_LEVELS + 1},):
        assert f(C.byref(_problem(glib, keep, **over)), inl.ctypes.data, C.addressof(ni), None, 0) == glib.EINVAL, over
    with pytest.raises(ValueError):
        glib.sim3_optimize(np.ones(4, np.uint8), np.zeros((3, 3)), np.zeros((4, 3)), np.zeros(4), np.zeros(4), np.zeros((4, 2)),
                           np.zeros((4, 2)), np.eye(4), np.eye(4), (1, 1, 0, 0), (1, 1, 0, 0), np.ones(8), np.eye(3), np.zeros(3), 1.0)


def test_no_device_means_ehip_not_a_fallback(glib):
    if glib.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = glib.lib()
    keep = []
    L.orbgpu_sim3_optimize_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    L.orbgpu_sim3_optimize_batch_device.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    pr = _problem(glib, keep)
    assert L.orbgpu_sim3_optimize_device(C.byref(pr), 0, None) == glib.EHIP
    assert L.orbgpu_sim3_optimize_batch_device(1, C.byref(pr), 0, None) == glib.EHIP
    v = C.c_int32()
    L.orbgpu_sim3_opt_last_spills.argtypes = [C.c_int32, C.c_void_p]
    assert L.orbgpu_sim3_opt_last_spills(0, C.byref(v)) == glib.EHIP
    n = 12
    with pytest.raises(glib.OrbGpuError) as ei:
        glib.sim3_optimize(np.ones(n, np.uint8), np.ones((n, 3), np.float32), np.ones((n, 3), np.float32), np.zeros(n, np.int32),
                           np.zeros(n, np.int32), np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32), np.eye(4), np.eye(4),
                           (500, 500, 320, 240), (500, 500, 320, 240), np.ones(8, np.float32), np.eye(3), np.zeros(3), 1.0)
    assert ei.value.status == glib.EHIP
    with pytest.raises(glib.OrbGpuError):
        glib.sim3_opt_last_spills()
