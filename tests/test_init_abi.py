"""The Initializer's C ABI without a device: the layouts of orbgpu_init_problem / orbgpu_init_result as lib.py mirrors them
against the header (through a C program), every EINVAL path (nothing is launched, so none needs a GPU), and I10's cosine
limits as the library computes them against tests/init_model.py."""
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

import init_model as M  # noqa: E402


@pytest.fixture(scope="module")
def G():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(ROOT, "orb_slam2_map_amd", "liborbgpu.so")):
        ge.build()
    from orb_slam2_map_amd import lib
    return lib


def test_struct_layouts_match_the_header(G, tmp_path):
    fields = {"orbgpu_init_result": [k for k, _ in G.InitResult._fields_], "orbgpu_init_problem": [k for k, _ in G.InitProblem._fields_]}
    lines = ['#include "orbgpu.h"', "#include <stddef.h>", "#include <stdio.h>", "int main(void) {"]
    for st, names in fields.items():
        lines.append('    printf("%%d\\n", (int)sizeof(%s));' % st)
        lines += ['    printf("%%d\\n", (int)offsetof(%s, %s));' % (st, k) for k in names]
    lines += ["    return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe],
                   check=True)
    got = [int(v) for v in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    want = []
    for cls in (G.InitResult, G.InitProblem):
        want += [C.sizeof(cls)] + [getattr(cls, k).offset for k, _ in cls._fields_]
    assert got == want
    assert C.sizeof(G.InitResult) == 240 and C.sizeof(G.InitProblem) == 144


def test_cos_limits_equal_the_model(G):
    for mp in (1.0, 0.5, 0.0, -1.0, 3.0, 90.0, 180.0, 181.0, float("nan")):
        lf, lh = G.initializer_cos_limits(mp)
        assert lf.tobytes() == np.float32(M.cos_limit(mp, True)).tobytes(), mp
        assert lh.tobytes() == np.float32(M.cos_limit(mp, False)).tobytes(), mp
    assert G.lib().orbgpu_initializer_cos_limits(C.c_float(1.0), None, None) == G.EINVAL


def test_every_einval_path_needs_no_device(G):
    L = G.lib()
    L.orbgpu_initializer_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    L.orbgpu_initializer_batch_device.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    L.orbgpu_initializer.argtypes = [C.c_void_p] * 4 + [C.c_int32]
    L.orbgpu_initializer_all.argtypes = [C.c_void_p] * 8 + [C.c_int32]
    sc = M.make_scene(20, 1, n_hyp=4)
    keep = []
    some = np.zeros(4096, np.uint8)
    ptrs = {k: some.ctypes.data for k in ("scores_h", "scores_f", "masks_h", "masks_f", "P3D", "triangulated", "result")}
    q0 = G._init_host_problem(sc, keep, **ptrs)
    base = {k: getattr(q0, k) for k, _ in G.InitProblem._fields_}
    base["K"] = (base["fx"], base["fy"], base["cx"], base["cy"])
    res = G.InitResult()
    assert L.orbgpu_initializer_device(None, 0, None) == G.EINVAL
    assert L.orbgpu_initializer_batch_device(-1, C.byref(q0), 0, None) == G.EINVAL
    assert L.orbgpu_initializer_batch_device(1, None, 0, None) == G.EINVAL
    assert L.orbgpu_initializer_batch_device(65536, C.byref(q0), 0, None) == G.EINVAL
    assert L.orbgpu_initializer(None, None, None, C.byref(res), 0) == G.EINVAL
    assert L.orbgpu_initializer(C.byref(q0), None, None, None, 0) == G.EINVAL
    assert L.orbgpu_initializer_all(C.byref(q0), None, None, None, None, None, None, None, 0) == G.EINVAL
    common = [{"kp1": 0}, {"kp2": 0}, {"matches12": 0}, {"sets": 0}, {"n1": -1}, {"n2": -1}, {"n_hyp": -1}, {"n1": 16385},
              {"n2": 16385}, {"n_hyp": 4097}, {"sigma": 0.0}, {"sigma": -1.0}, {"sigma": float("nan")}, {"min_triangulated": -1}]
    device_only = [{"scores_h": 0}, {"scores_f": 0}, {"masks_h": 0}, {"masks_f": 0}, {"P3D": 0}, {"triangulated": 0}, {"result": 0}]
    for over in common + device_only:
        q = G.init_problem(dict(base, **over))
        assert L.orbgpu_initializer_device(C.byref(q), 0, None) == G.EINVAL, over
        assert L.orbgpu_initializer_batch_device(1, C.byref(q), 0, None) == G.EINVAL, over
        assert L.orbgpu_last_error_string()
    for over in common:
        q = G.init_problem(dict(base, **over))
        assert L.orbgpu_initializer(C.byref(q), None, None, C.byref(res), 0) == G.EINVAL, over
        assert L.orbgpu_initializer_all(C.byref(q), None, None, None, None, None, None, C.byref(res), 0) == G.EINVAL, over
    # I2 in the host flavours: a set index outside [0, N) is refused before anything is launched (N = 20 >= 8)
    for v in (20, -1):
        bad = dict(sc, sets=sc["sets"].copy())
        bad["sets"][2, 5] = v
        for fn in (G.initializer, G.initializer_all):
            with pytest.raises(G.OrbGpuError) as ei:
                fn(bad)
            assert ei.value.status == G.EINVAL and "outside [0, 20)" in str(ei.value)
    with pytest.raises(ValueError):
        G.initializer(dict(sc, matches12=sc["matches12"][:-1]))
