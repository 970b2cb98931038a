"""The arithmetic of k_fast_detect's corner score without a device: orb_slam2_map_amd/csrc/fast_polarity.h holds the
scalar form of the two-network score and of the single-network form with the polarity selector (what fast_score_pk
runs on packed pixel pairs); tests/fast_polarity_test.cpp compares them on every ring over {c-1, c+1} with c at up to
4 positions for the centres 0, 1, 128, 254, 255 and on 4 M random rings with planted arcs.  (`fast_polarity_test full`
runs all 3^16 rings over {c-1, c, c+1} per centre instead: 20 s of CPU time, too long for the suite.)"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# rings the reduced run visits: sum over k <= 4 of C(16, k) 2^(16-k) for the centres 1, 128, 254; at 0 and 255 only one of
# c-1 / c+1 is a byte (sum of C(16, k)); 4 M random ones
RINGS = 3 * 14598144 + 2 * 2517 + 8 * 500000


def test_single_network_score_equals_two_networks(tmp_path):
    exe = str(tmp_path / "fast_polarity_test")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-pthread",
                    "-I" + os.path.join(ROOT, "orb_slam2_map_amd", "csrc"),
                    os.path.join(ROOT, "tests", "fast_polarity_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["fast_polarity_test", "ok", str(RINGS)], r.stdout
