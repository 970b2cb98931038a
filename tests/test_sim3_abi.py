"""The Sim3 solver's entry points (include/orbgpu.h) without a GPU: the header compiles as C and C++, the ctypes mirror
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

import sim3_model as M  # noqa: E402

SYMBOLS = ("orbgpu_sim3_ransac_iterations", "orbgpu_sim3_solve_device", "orbgpu_sim3_solve_batch_device", "orbgpu_sim3_solve",
           "orbgpu_sim3_solve_all")


def probe_source(glib):
    """a C / C++ program that prints the size of both structs and the offset of EVERY field the mirror has"""
    lines = []
    for ctype, cls in (("orbgpu_sim3_problem", glib.Sim3Problem), ("orbgpu_sim3_result", glib.Sim3Result)):
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


def test_sim3_symbols_are_exported(glib):
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
    for cls in (glib.Sim3Problem, glib.Sim3Result):
        want += [C.sizeof(cls)] + [getattr(cls, name).offset for name, _ in cls._fields_]
    assert got == want
    assert len(glib.Sim3Problem._fields_) == 34 and len(glib.Sim3Result._fields_) == 10  # the header's field counts
    assert C.sizeof(glib.Sim3Problem) == 376 and C.sizeof(glib.Sim3Result) == 40


def test_ransac_iterations_equal_the_model(glib):
    table = [(n, p, mi, mx) for n in (0, 1, 3, 19, 20, 21, 25, 64, 100, 300, 2816, 10 ** 6) for p in (0.99, 0.5, 0.999, 1.0, 0.0, 1.5)
             for mi in (0, 1, 6, 20, 21) for mx in (0, 1, 5, 300)]
    for a in table:
        assert glib.sim3_ransac_iterations(*a) == M.ransac_iterations(*a), a
    assert glib.sim3_ransac_iterations(100, 0.99, 20, 300) == 300 and glib.sim3_ransac_iterations(25, 0.99, 20, 300) == 7
    L = glib.lib()
    L.orbgpu_sim3_ransac_iterations.argtypes = [C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_void_p]
    v = C.c_int32()
    assert L.orbgpu_sim3_ransac_iterations(10, 0.99, 6, 300, None) == glib.EINVAL
    for bad in ((-1, 6, 300), (10, -1, 300), (10, 6, -1)):
        assert L.orbgpu_sim3_ransac_iterations(bad[0], 0.99, bad[1], bad[2], C.byref(v)) == glib.EINVAL


def _problem(glib, keep, **over):
    """host buffers in the place of device pointers: every call below is refused before they are read"""
    buf = np.zeros(1 << 16, np.uint8)
    keep.append(buf)
    p = {k: buf.ctypes.data for k in ("valid", "Xw1", "Xw2", "octave1", "octave2", "triples", "counts", "R", "t", "s", "T12",
                                      "masks", "result")}
    p.update(n1=16, n_hyp=4, T1w=np.eye(4), T2w=np.eye(4), K1=(500, 500, 320, 240), K2=(500, 500, 320, 240),
             level_sigma2=M.SIGMA2, fix_scale=0, probability=0.99, min_inliers=6, max_iterations=300)
    p.update(over)
    return glib.sim3_problem(p)


def test_entry_points_refuse_bad_arguments(glib):
    L = glib.lib()
    one, batch, host = L.orbgpu_sim3_solve_device, L.orbgpu_sim3_solve_batch_device, L.orbgpu_sim3_solve
    one.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    batch.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    host.argtypes = [C.c_void_p] * 8 + [C.c_int32]
    L.orbgpu_sim3_solve_all.argtypes = [C.c_void_p] * 8 + [C.c_int32]
    keep = []
    assert one(None, 0, None) == glib.EINVAL and batch(1, None, 0, None) == glib.EINVAL
    assert batch(-1, C.byref(_problem(glib, keep)), 0, None) == glib.EINVAL
    res = glib.Sim3Result()
    for over in ({"valid": 0}, {"Xw1": 0}, {"Xw2": 0}, {"octave1": 0}, {"octave2": 0}, {"triples": 0}, {"n1": -1}, {"n_hyp": -1},
                 {"n1": 1 << 20}, {"n_hyp": 1 << 20}, {"nlevels": 0}, {"nlevels": glib.MAX_LEVELS + 1}, {"min_inliers": -1},
                 {"max_iterations": -1}, {"start_iteration": -1}, {"best_so_far": -1}):
        p = _problem(glib, keep, **over)
        assert one(C.byref(p), 0, None) == glib.EINVAL, over
        assert batch(1, C.byref(p), 0, None) == glib.EINVAL, over
        assert host(C.byref(p), None, None, None, None, None, None, C.byref(res), 0) == glib.EINVAL, over
        assert L.orbgpu_sim3_solve_all(C.byref(p), None, None, None, None, None, None, C.byref(res), 0) == glib.EINVAL, over
    for over in ({"counts": 0}, {"R": 0}, {"t": 0}, {"s": 0}, {"T12": 0}, {"masks": 0}, {"result": 0}):
        assert one(C.byref(_problem(glib, keep, **over)), 0, None) == glib.EINVAL, over
    assert host(None, None, None, None, None, None, None, C.byref(res), 0) == glib.EINVAL
    assert host(C.byref(_problem(glib, keep)), None, None, None, None, None, None, None, 0) == glib.EINVAL
    # a triple index outside [0, N) is refused by the host flavour before the device is looked for
    sc = M.make_scene(30, 1, n_hyp=4)
    sc["triples"][2, 2] = 30
    with pytest.raises(glib.OrbGpuError) as ei:
        glib.sim3_solve(sc["valid"], sc["Xw1"], sc["Xw2"], sc["octave1"], sc["octave2"], sc["T1w"], sc["T2w"], sc["K1"], sc["K2"],
                        sc["level_sigma2"], sc["triples"], min_inliers=6)
    assert ei.value.status == glib.EINVAL


def test_no_device_means_ehip_not_a_fallback(glib):
    if glib.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = glib.lib()
    L.orbgpu_sim3_solve_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    keep = []
    assert L.orbgpu_sim3_solve_device(C.byref(_problem(glib, keep)), 0, None) == glib.EHIP
    sc = M.make_scene(30, 1, n_hyp=4)
    with pytest.raises(glib.OrbGpuError) as ei:
        glib.sim3_solve(sc["valid"], sc["Xw1"], sc["Xw2"], sc["octave1"], sc["octave2"], sc["T1w"], sc["T2w"], sc["K1"], sc["K2"],
                        sc["level_sigma2"], sc["triples"], min_inliers=6)
    assert ei.value.status == glib.EHIP
