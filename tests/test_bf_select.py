"""The candidate selection of k_bf_topk without a device: orb_slam2_map_amd/csrc/bf_select.h holds, in scalar form for
one lane and one row block, the blanking loop the kernel ran before and the order walk it runs now ("the next value
below the one just taken", the bar compared on the tagged value); tests/bf_select_test.cpp compares lists, bars and
trip counts on all 3^16 blocks over {bar-1, bar, bar+1}, on crafted blocks (ties, 16 equal distances, rows past jlast,
negative dot, a list that fills inside a block) and on about six million random blocks in sequences, and shows that one
bar for the two lanes of an A row (not in the kernel) would leave the merged list as it is."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_order_walk_equals_blanking_loop(tmp_path):
    exe = str(tmp_path / "bf_select_test")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-pthread",
                    "-I" + os.path.join(ROOT, "orb_slam2_map_amd", "csrc"),
                    os.path.join(ROOT, "tests", "bf_select_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    out = r.stdout.split()
    assert r.returncode == 0 and out[:2] == ["bf_select_test", "ok"], r.stdout
    assert int(out[2]) > 3 ** 16 + 3000000, r.stdout  # the exhaustive set and a few million random blocks
