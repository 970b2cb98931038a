"""carve.h's WorkPlan, the planner that names each workspace buffer of local_ba.hip and essential_graph.hip once:
tests/work_plan_test.cpp is built for the host with g++ (AddressSanitizer + UBSan) and checks, for segment lists with counts
of 0, counts that end exactly on 256 bytes, one problem and three problems, and element sizes 1, 4, 8 and 16, that the
offsets, upload_bytes() and total() are those of a plain Carver(256) in which every uploaded take precedes every scratch
take; that the blob holds each source at its offset and zeros in the gaps; that the measuring pass reads no source; and that
a segment filled in place is handed out at blob + offset."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_work_plan_on_the_host(tmp_path):
    exe = str(tmp_path / "work_plan_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-I" + os.path.join(ROOT, "orb_slam2_map_amd", "csrc"), os.path.join(ROOT, "tests", "work_plan_test.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout == "work_plan_test ok\n", r.stdout  # no sanitizer report either
