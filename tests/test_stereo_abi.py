"""Argument validation of the stereo entry points (Frame::ComputeStereoMatches, include/orbgpu.h): every refusal below
happens before the handles are read or the device is touched, so no GPU is needed."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def glib():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(ROOT, "orb_slam2_map_amd", "liborbgpu.so")):
        ge.build()
    from orb_slam2_map_amd import lib
    return lib


def test_stereo_symbols_are_exported(glib):
    L = glib.lib()
    for s in ("orbgpu_stereo_matches_batch_device", "orbgpu_compute_stereo_matches"):
        assert hasattr(L, s) and s in glib.ABI_SYMBOLS


def test_batch_device_refuses_bad_arguments(glib):
    L = glib.lib()
    # stands in for a handle: never dereferenced, every call below is refused by an earlier check
    fake = np.zeros(64, np.uint8)
    h = fake.ctypes.data
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data
    f = L.orbgpu_stereo_matches_batch_device

    def call(left=h, right=h, batch=1, cap=8, kl=p, nl=p, dl=p, kr=p, nr=p, dr=p, ur=p, dz=p):
        return f(left, 0, right, 0, batch, cap, kl, nl, dl, kr, nr, dr, 100.0, 500.0, ur, dz, None, None)

    assert call(left=None) == glib.EINVAL
    assert call(right=None) == glib.EINVAL
    assert call(batch=-1) == glib.EINVAL
    assert call(cap=-1) == glib.EINVAL
    assert call(ur=None) == glib.EINVAL
    assert call(dz=None) == glib.EINVAL
    assert call(kl=None) == glib.EINVAL
    assert call(nr=None) == glib.EINVAL
    assert call(dr=None) == glib.EINVAL
    assert b"null" in L.orbgpu_last_error_string()


def test_host_entry_refuses_bad_arguments(glib):
    L = glib.lib()
    fake = np.zeros(64, np.uint8)
    h = fake.ctypes.data
    kps = np.zeros(4, glib.KEYPOINT_DTYPE)
    desc = np.zeros((4, 32), np.uint8)
    out = np.zeros(4, np.float32)
    kp, dp, op = kps.ctypes.data, desc.ctypes.data, out.ctypes.data
    f = L.orbgpu_compute_stereo_matches
    assert f(None, h, 4, kp, dp, 4, kp, dp, 100.0, 500.0, op, op) == glib.EINVAL
    assert f(h, None, 4, kp, dp, 4, kp, dp, 100.0, 500.0, op, op) == glib.EINVAL
    assert f(h, h, -1, kp, dp, 4, kp, dp, 100.0, 500.0, op, op) == glib.EINVAL
    assert f(h, h, 4, kp, dp, -1, kp, dp, 100.0, 500.0, op, op) == glib.EINVAL
    assert f(h, h, 4, kp, dp, 4, kp, dp, 100.0, 500.0, None, op) == glib.EINVAL
    assert f(h, h, 4, kp, dp, 4, kp, dp, 100.0, 500.0, op, None) == glib.EINVAL
    assert f(h, h, 4, None, dp, 4, kp, dp, 100.0, 500.0, op, op) == glib.EINVAL
    assert f(h, h, 4, kp, dp, 4, kp, None, 100.0, 500.0, op, op) == glib.EINVAL
