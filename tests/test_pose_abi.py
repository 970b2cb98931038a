"""The pose-optimisation entry points (Optimizer::PoseOptimization, include/orbgpu.h) without a GPU: they exist, refuse
bad arguments before the device is touched, and without a device fail with EHIP -- never a CPU fallback."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("orbgpu_pose_optimization", "orbgpu_pose_optimization_device", "orbgpu_pose_optimization_batch_device",
           "orbgpu_pose_optimization_table", "orbgpu_pose_last_spills")


@pytest.fixture(scope="module")
def glib():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(ROOT, "orb_slam2_map_amd", "liborbgpu.so")):
        ge.build()
    from orb_slam2_map_amd import lib
    return lib


def test_pose_symbols_are_exported(glib):
    L = glib.lib()
    for s in SYMBOLS:
        assert hasattr(L, s) and s in glib.ABI_SYMBOLS, s


def test_struct_layouts_match_the_header(glib):
    assert C.sizeof(glib.PoseResult) == 16 * 8 + 16 * 4 + 6 * 4
    assert glib.PoseResult.Tcw.offset == 128 and glib.PoseResult.n_initial.offset == 192
    assert glib.PoseProblem.rows.offset == 24 and glib.PoseProblem.Tcw.offset == 32
    assert glib.PoseProblem.fx.offset == 48 and glib.PoseProblem.d_outlier.offset == 72 and C.sizeof(glib.PoseProblem) == 88


def _problem(glib, keep, **over):
    """A well-formed problem whose "device" pointers are host buffers: every call below is refused before they are read,
    or stops at the device selection."""
    buf = np.zeros(4096, np.uint8)
    T = np.eye(4, dtype=np.float32)
    sg = np.ones(8, np.float32)
    fv = glib.DeviceFrameView()
    fv.cap, fv.n, fv.kps, fv.u_right, fv.nlevels = 16, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, 8
    p = glib.PoseProblem()
    p.frame = C.addressof(fv)
    p.d_kp_to_mp = p.d_world_pos = p.d_outlier = p.d_result = buf.ctypes.data
    p.rows, p.Tcw, p.inv_level_sigma2 = 16, T.ctypes.data, sg.ctypes.data
    p.fx, p.fy, p.cx, p.cy, p.mbf = 500.0, 500.0, 320.0, 240.0, 40.0
    keep += [buf, T, sg, fv]
    for k, v in over.items():
        if k in ("cap", "nlevels", "n", "kps", "u_right"):
            setattr(fv, k, v)
        else:
            setattr(p, k, v)
    return p


def test_device_entry_points_refuse_bad_arguments(glib):
    L = glib.lib()
    one, batch = L.orbgpu_pose_optimization_device, L.orbgpu_pose_optimization_batch_device
    one.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    batch.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    keep = []
    assert one(None, 0, None) == glib.EINVAL
    assert batch(-1, C.byref(_problem(glib, keep)), 0, None) == glib.EINVAL
    assert batch(1, None, 0, None) == glib.EINVAL
    for over in ({"frame": None}, {"d_kp_to_mp": None}, {"Tcw": None}, {"inv_level_sigma2": None}, {"d_outlier": None},
                 {"d_result": None}, {"d_world_pos": None}, {"rows": -1}, {"nlevels": 0}, {"nlevels": glib.MAX_LEVELS + 1},
                 {"cap": -1}, {"cap": 1 << 20}, {"n": None}, {"kps": None}, {"u_right": None}):
        p = _problem(glib, keep, **over)
        assert one(C.byref(p), 0, None) == glib.EINVAL, over
        assert batch(1, C.byref(p), 0, None) == glib.EINVAL, over
    assert L.orbgpu_pose_last_spills(0, None) == glib.EINVAL


def test_host_and_table_entry_points_refuse_bad_arguments(glib):
    L = glib.lib()
    f = L.orbgpu_pose_optimization
    f.argtypes = [C.c_void_p] * 5 + [C.c_float] * 5 + [C.c_void_p] * 3 + [C.c_int32]
    n = 8
    fr = glib.Frame(np.full(n, 100, np.float32), np.full(n, 100, np.float32), np.zeros(n, np.int32), np.zeros(n, np.float32),
                    np.full(n, -1, np.float32), np.zeros((n, 32), np.uint8), 640, 480, np.ones(8, np.float32))
    has, wp, out = np.ones(n, np.uint8), np.zeros((n, 3), np.float32), np.zeros(n, np.uint8)
    T, sg, ni = np.eye(4, dtype=np.float32), np.ones(8, np.float32), C.c_int32()
    p = lambda a: a.ctypes.data  # noqa: E731

    def call(view=None, has_=p(has), wp_=p(wp), T_=p(T), sg_=p(sg), out_=p(out), ni_=C.addressof(ni)):
        v = fr.view() if view is None else view
        return f(C.byref(v) if v is not False else None, has_, wp_, T_, sg_, 500.0, 500.0, 320.0, 240.0, 40.0, out_, ni_,
                 None, 0)
    assert call(view=False) == glib.EINVAL
    assert call(has_=None) == glib.EINVAL and call(wp_=None) == glib.EINVAL and call(T_=None) == glib.EINVAL
    assert call(sg_=None) == glib.EINVAL and call(out_=None) == glib.EINVAL and call(ni_=None) == glib.EINVAL
    for bad in ({"n": -1}, {"nlevels": 0}, {"nlevels": glib.MAX_LEVELS + 1}, {"kp_octave": None}):
        v = fr.view()
        for k, val in bad.items():
            setattr(v, k, val)
        assert call(view=v) == glib.EINVAL, bad
    g = L.orbgpu_pose_optimization_table
    g.argtypes = [C.c_void_p] * 5 + [C.c_float] * 5 + [C.c_void_p] * 3
    assert g(None, None, None, p(T), p(sg), 500.0, 500.0, 320.0, 240.0, 40.0, p(out), C.addressof(ni), None) == glib.EINVAL


def test_no_device_means_ehip_not_a_fallback(glib):
    if glib.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = glib.lib()
    keep = []
    L.orbgpu_pose_optimization_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    L.orbgpu_pose_optimization_batch_device.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    pr = _problem(glib, keep)
    assert L.orbgpu_pose_optimization_device(C.byref(pr), 0, None) == glib.EHIP
    assert L.orbgpu_pose_optimization_batch_device(1, C.byref(pr), 0, None) == glib.EHIP
    v = C.c_int32()
    assert L.orbgpu_pose_last_spills(0, C.byref(v)) == glib.EHIP
    n = 8
    fr = glib.Frame(np.full(n, 100, np.float32), np.full(n, 100, np.float32), np.zeros(n, np.int32), np.zeros(n, np.float32),
                    np.full(n, -1, np.float32), np.zeros((n, 32), np.uint8), 640, 480, np.ones(8, np.float32))
    with pytest.raises(glib.OrbGpuError) as ei:
        glib.pose_optimization(fr, np.ones(n, np.uint8), np.ones((n, 3), np.float32), np.eye(4), np.ones(8, np.float32),
                               500.0, 500.0, 320.0, 240.0, 40.0)
    assert ei.value.status == glib.EHIP
