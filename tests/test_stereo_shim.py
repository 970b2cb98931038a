"""ComputeStereoMatchesT (orb_slam2_map_amd/shim/orbgpu_shim.hpp) and INTEGRATION.md's "Stereo frames" block: both
compile with -Werror (and the shim under AddressSanitizer / UBSan) against stand-ins with the stereo Frame members; on
the GPU the shim's answer equals the host entry point's."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "orb_slam2_map_amd")
STRICT = ["-std=c++17", "-Wall", "-Wextra", "-Werror"]


def _lib():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(PKG, "liborbgpu.so")):
        ge.build()


def build(tmp_path, sanitize=False):
    _lib()
    exe = str(tmp_path / ("stereo_shim_test" + ("_san" if sanitize else "")))
    cmd = ["g++"] + STRICT + ["-O1"] + (["-fsanitize=address,undefined"] if sanitize else []) + [
        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "shim"), os.path.join(ROOT, "tests", "stereo_shim_test.cpp"),
        "-o", exe, "-L" + PKG, "-lorbgpu", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-pthread"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return exe


@pytest.mark.parametrize("sanitize", [False, True])
def test_stereo_shim_compiles(tmp_path, sanitize):
    exe = build(tmp_path, sanitize)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
    assert r.returncode == 2 and "usage" in r.stderr


STANDIN = r'''
#include <cstdint>
#include <vector>
#include "orbgpu_shim.hpp"
namespace cv {
struct Point2f { float x, y; };
struct KeyPoint { Point2f pt; float size, angle, response; int octave, class_id; };
struct Mat { unsigned char *data = nullptr; int rows = 0; };
}
namespace ORB_SLAM2 {
class ORBextractor {  // with the Impl member INTEGRATION.md section 1 adds
  public:
    struct Impl { orbgpu_shim::ORBextractorT<cv::KeyPoint> gpu; };
    Impl *impl;
};
class Frame {  // include/Frame.h:100-190, the members the stereo constructor touches
  public:
    void ComputeStereoMatches();
    ORBextractor *mpORBextractorLeft, *mpORBextractorRight;
    int N;
    std::vector<cv::KeyPoint> mvKeys, mvKeysRight;
    std::vector<float> mvuRight, mvDepth;
    cv::Mat mDescriptors, mDescriptorsRight;
    float mbf, mb;
    static float fx;
};
}
'''


def stereo_block():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"<!-- stereo-snippet -->\s*```cpp\n(.*?)```", text, re.S)
    assert m, "INTEGRATION.md has no stereo block"
    return m.group(1)


DEVICE_CHAIN = r'''
#include <cstddef>
#include <vector>
#include "orbgpu.h"
void stereo_chain(orbgpu_extractor *ext, const uint8_t *d_gray, int B, int w, int h, orbgpu_keypoint *d_kps,
                  uint8_t *d_desc, int cap, int32_t *d_n, void *stream, float mbf, float fx, float *d_u_right,
                  float *d_kp_depth, int32_t *d_n_stereo, int dev, orbgpu_camera cam, orbgpu_keypoint *d_kps_un,
                  int32_t *d_cell_start, int32_t *d_cell_items, int nlevels, const std::vector<float> &mvScaleFactors)
{
'''


def test_integration_stereo_device_chain_compiles(tmp_path):
    """INTEGRATION.md's batched chain (extract 2B frames -> stereo -> frame glue -> device frame view), wrapped in a
    function that declares the names it uses."""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"<!-- stereo-device-snippet -->\s*```cpp\n(.*?)```", text, re.S)
    assert m, "INTEGRATION.md has no batched stereo block"
    src = tmp_path / "chain.cc"
    src.write_text(DEVICE_CHAIN + m.group(1) + "    (void)fv;\n}\n")
    r = subprocess.run(["g++"] + STRICT + ["-c", "-I" + os.path.join(ROOT, "include"), str(src), "-o",
                                           str(tmp_path / "chain.o")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True)
    assert r.returncode == 0, r.stdout[-4000:]


def test_integration_stereo_block_compiles(tmp_path):
    src = tmp_path / "stereo.cc"
    src.write_text(STANDIN + stereo_block())
    r = subprocess.run(["g++"] + STRICT + ["-Wno-unused-parameter", "-c", "-I" + os.path.join(ROOT, "include"),
                                           "-I" + os.path.join(PKG, "shim"), str(src), "-o", str(tmp_path / "stereo.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]


@pytest.mark.gpu
def test_stereo_shim_equals_host_entry(tmp_path):
    from orb_slam2_map_amd import lib as G
    from orb_slam2_map_amd.synth import StereoStream
    if G.device_count() < 1:
        pytest.skip("no HIP device")
    exe = build(tmp_path)
    st = StereoStream(1241, 376, 16)
    left, right, _ = st.frame(2)
    lp, rp, out = tmp_path / "l.raw", tmp_path / "r.raw", tmp_path / "out.bin"
    lp.write_bytes(left.tobytes())
    rp.write_bytes(right.tobytes())
    r = subprocess.run([exe, str(lp), str(rp), str(st.w), str(st.h), "2000", repr(float(st.bf)), repr(float(st.fx)), str(out)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "stereo shim ok" in r.stdout, r.stdout
    buf = out.read_bytes()
    n = int(np.frombuffer(buf, np.int32, 1)[0])
    su = np.frombuffer(buf, np.float32, n, 4)
    sd = np.frombuffer(buf, np.float32, n, 4 + 4 * n)
    el, er = G.ORBextractor(2000), G.ORBextractor(2000)
    kl, dl = el(left)
    kr, dr = er(right)
    u, d = G.compute_stereo_matches(el, er, kl, dl, kr, dr, st.bf, st.fx)
    assert n == len(kl) and np.array_equal(su.view(np.int32), u.view(np.int32)) and np.array_equal(sd.view(np.int32), d.view(np.int32))
