"""The PnP solver's entry points (include/orbgpu.h) without a GPU: the header compiles as C and C++, the ctypes mirror
has its layout, the host formula equals the model's, bad arguments are refused before the device is touched and without
a device the calls fail with EHIP -- never a CPU fallback."""
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

import pnp_model as M  # noqa: E402

SYMBOLS = ("orbgpu_pnp_ransac_parameters", "orbgpu_pnp_solve_device", "orbgpu_pnp_solve_batch_device", "orbgpu_pnp_solve",
           "orbgpu_pnp_solve_all", "orbgpu_pnp_solve_table")


def probe_source(glib):
    """a C / C++ program that prints the size of both structs and the offset of EVERY field the mirror has"""
    lines = []
    for ctype, cls in (("orbgpu_pnp_problem", glib.PnpProblem), ("orbgpu_pnp_result", glib.PnpResult)):
        lines.append('    printf("%%zu\\n", sizeof(%s));' % ctype)
        lines += ['    printf("%%zu\\n", offsetof(%s, %s));' % (ctype, name) for name, _ in cls._fields_]
    return '#include <stddef.h>\n#include <stdio.h>\n#include "orbgpu.h"\nint main(void)\n{\n' + "\n".join(lines) + "\n    return 0;\n}\n"


@pytest.fixture(scope="module")
def glib():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(ROOT, "orb_slam2_map_amd", "liborbgpu.so")):
        ge.build()
    from orb_slam2_map_amd import lib
    return lib


def test_pnp_symbols_are_exported(glib):
    L = glib.lib()
    for s in SYMBOLS:
        assert hasattr(L, s) and s in glib.ABI_SYMBOLS, s


@pytest.mark.parametrize("cc,ext,std", [("gcc", "c", "-std=c99"), ("g++", "cc", "-std=c++11")])
def test_header_compiles_and_the_mirror_has_its_layout(glib, tmp_path, cc, ext, std):
    src = tmp_path / ("probe." + ext)
    src.write_text(probe_source(glib))
    exe = str(tmp_path / "probe")
    r = subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    got = [int(x) for x in subprocess.run([exe], stdout=subprocess.PIPE, text=True).stdout.split()]
    want = []
    for cls in (glib.PnpProblem, glib.PnpResult):
        want += [C.sizeof(cls)] + [getattr(cls, name).offset for name, _ in cls._fields_]
    assert got == want
    assert len(glib.PnpProblem._fields_) == 29 and len(glib.PnpResult._fields_) == 13  # the header's field counts
    assert C.sizeof(glib.PnpResult) == 112


def test_ransac_parameters_equal_the_model(glib):
    table = [(n, p, mi, mx, ms, eps) for n in (0, 1, 3, 9, 10, 11, 25, 64, 100, 300, 1200, 10 ** 6) for p in (0.99, 0.5, 1.0, 0.0, 1.5)
             for mi in (0, 1, 10, 50) for mx in (0, 1, 300) for ms in (4, 6) for eps in (0.5, 0.4, 0.0, 1.0, 2.5, -1.0, float("nan"), 1e30)]
    for a in table:
        assert glib.pnp_ransac_parameters(*a) == M.ransac_parameters(*a), a
    assert glib.pnp_ransac_parameters(300, 0.99, 10, 300, 4, 0.5) == (150, 35)
    assert glib.pnp_ransac_parameters(11, 0.99, 10, 300, 4, 0.5) == (10, 4)
    L = glib.lib()
    L.orbgpu_pnp_ransac_parameters.argtypes = [C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p]
    a, b = C.c_int32(), C.c_int32()
    assert L.orbgpu_pnp_ransac_parameters(10, 0.99, 6, 300, 4, 0.5, None, C.byref(b)) == glib.EINVAL
    assert L.orbgpu_pnp_ransac_parameters(10, 0.99, 6, 300, 4, 0.5, C.byref(a), None) == glib.EINVAL
    for bad in ((-1, 6, 300, 4), (10, -1, 300, 4), (10, 6, -1, 4), (10, 6, 300, -1)):
        assert L.orbgpu_pnp_ransac_parameters(bad[0], 0.99, bad[1], bad[2], bad[3], 0.5, C.byref(a), C.byref(b)) == glib.EINVAL


def _problem(glib, keep, **over):
    """host buffers in the place of device pointers: every call below is refused before they are read"""
    buf = np.zeros(1 << 16, np.uint8)
    keep.append(buf)
    p = {k: buf.ctypes.data for k in ("valid", "Xw", "kp", "octave", "sets", "counts", "Tcw", "masks", "refined_mask", "result")}
    p.update(n1=16, n_hyp=4, K=(500, 500, 320, 240), level_sigma2=M.SIGMA2, probability=0.99, min_inliers=10, max_iterations=300,
             min_set=4, epsilon=0.5, th2=5.991)
    p.update(over)
    return glib.pnp_problem(p)


def test_entry_points_refuse_bad_arguments(glib):
    L = glib.lib()
    one, batch, host, every = L.orbgpu_pnp_solve_device, L.orbgpu_pnp_solve_batch_device, L.orbgpu_pnp_solve, L.orbgpu_pnp_solve_all
    one.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    batch.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    host.argtypes = [C.c_void_p] * 5 + [C.c_int32]
    every.argtypes = [C.c_void_p] * 6 + [C.c_int32]
    keep = []
    assert one(None, 0, None) == glib.EINVAL and batch(1, None, 0, None) == glib.EINVAL
    assert batch(-1, C.byref(_problem(glib, keep)), 0, None) == glib.EINVAL
    res = glib.PnpResult()
    for over in ({"valid": 0}, {"Xw": 0}, {"kp": 0}, {"octave": 0}, {"sets": 0}, {"n1": -1}, {"n_hyp": -1}, {"n1": M.MAX_N1 + 1},
                 {"n_hyp": M.MAX_HYP + 1}, {"min_set": 3}, {"min_set": 65}, {"nlevels": 0}, {"nlevels": glib.MAX_LEVELS + 1},
                 {"min_inliers": -1}, {"max_iterations": -1}, {"start_iteration": -1}, {"best_so_far": -1}, {"n_iterations": -1}):
        p = _problem(glib, keep, **over)
        assert one(C.byref(p), 0, None) == glib.EINVAL, over
        assert batch(1, C.byref(p), 0, None) == glib.EINVAL, over
        assert host(C.byref(p), None, None, None, C.byref(res), 0) == glib.EINVAL, over
        assert every(C.byref(p), None, None, None, None, C.byref(res), 0) == glib.EINVAL, over
    for over in ({"counts": 0}, {"Tcw": 0}, {"masks": 0}, {"refined_mask": 0}, {"result": 0}):
        assert one(C.byref(_problem(glib, keep, **over)), 0, None) == glib.EINVAL, over
    assert host(None, None, None, None, C.byref(res), 0) == glib.EINVAL
    assert host(C.byref(_problem(glib, keep)), None, None, None, None, 0) == glib.EINVAL
    assert every(None, None, None, None, None, C.byref(res), 0) == glib.EINVAL
    # a set index outside [0, N) is refused by the host flavours before the device is looked for
    sc = M.make_scene(30, 1, n_hyp=4)
    sc["sets"][2, 3] = 30
    for f in (glib.pnp_solve, glib.pnp_solve_all):
        with pytest.raises(glib.OrbGpuError) as ei:
            f(sc)
        assert ei.value.status == glib.EINVAL


def test_no_device_means_ehip_not_a_fallback(glib):
    if glib.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = glib.lib()
    L.orbgpu_pnp_solve_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    keep = []
    assert L.orbgpu_pnp_solve_device(C.byref(_problem(glib, keep)), 0, None) == glib.EHIP
    sc = M.make_scene(30, 1, n_hyp=4)
    for f in (glib.pnp_solve, glib.pnp_solve_all):
        with pytest.raises(glib.OrbGpuError) as ei:
            f(sc)
        assert ei.value.status == glib.EHIP
