"""The shared parts of the device optimisers are written once: the Sim3 exponential and algebra in
sim3_math.h, the barrier, the stop flag, the workgroup reductions and the decision on a Levenberg-Marquardt trial in
opt_math.h, and each workspace buffer of the two graph optimisers named once through carve.h's WorkPlan; and each staging
segment of the host flavours is declared once on carve.h's HostPlan."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orb_slam2_map_amd", "csrc")
NAMES = sorted(n for n in os.listdir(CSRC) if n.endswith((".hip", ".h")))
SRC = {n: open(os.path.join(CSRC, n)).read() for n in NAMES}
OPTIMISERS = ("pose_opt.hip", "sim3_opt.hip", "local_ba.hip", "essential_graph.hip")


def _holders(pattern):
    return [n for n in NAMES if re.search(pattern, SRC[n])]


def test_the_copies_and_their_notes_are_gone():
    for word in ("second text", "WorkgroupBarrier {", "the move was not tried"):
        assert [n for n in NAMES if n.endswith(".hip") and word in SRC[n]] == [], word
    assert _holders(r"struct WorkgroupBarrier\b") == ["opt_math.h"]
    assert _holders(r"bool stop_requested\(") == ["opt_math.h"]
    assert _holders(r"double block_max\(") == ["opt_math.h"]
    assert _holders(r"void wave_sum\(double \(&v\)\[K\]\)") == ["opt_math.h"]


def test_the_trial_decision_is_in_opt_math_for_the_kernels_that_kept_it():
    # 1 - (2 rho - 1)^3, whatever the variable is called: in opt_math.h for k_pose_opt, k_local_ba and k_bundle_adjustment,
    # which call lm_trial, and written out in k_sim3_opt and k_essential_graph, where calling it failed a row of their bench
    # tools against the parent's spread
    cube = r"1\.0 - \((\w+) \* \1\) \* \1"
    kept_out = ["essential_graph.hip", "sim3_opt.hip"]
    assert _holders(cube) == sorted(kept_out + ["opt_math.h"])
    assert all(len(re.findall(cube, SRC[n])) == 1 for n in kept_out + ["opt_math.h"])
    assert _holders(r"lam \* nu;") == sorted(kept_out + ["opt_math.h"])
    for n in ("pose_opt.hip", "local_ba.hip"):
        assert SRC[n].count("lm_trial(cur, tmp, scale, lam, nu, rho, stop)") == 1, n
    for n in kept_out:
        assert "lm_trial(" not in SRC[n].split("#include", 1)[1], n
    for n in OPTIMISERS:
        assert "while (!stop && rho < 0 && trial < 10);" in SRC[n], n  # the loop conditions stay in the kernels


def test_the_sim3_exponential_is_in_sim3_math_alone():
    # the branch table of O5: the large-angle, large-sigma A and the published small-angle B
    for expr in ("(a * sigma + (1.0 - b) * th) / (th * c)", "(((0.5 * sigma2 - sigma) + 1.0) * sx) / (sigma2 * sigma)",
                 "small_th = th < eps"):
        assert [n for n in NAMES if expr in SRC[n]] == ["sim3_math.h"], expr
    assert _holders(r"void sim3_update\(") == ["sim3_math.h"] and len(re.findall(r"void sim3_update\(", SRC["sim3_math.h"])) == 2
    for fn in ("sim3_mul", "sim3_inv", "sim3_map", "lu_solve3", "sim3_log", "sim3_edge_error", "chi2_of", "load8"):
        assert _holders(r"\b(void|double) %s\(" % fn) == ["sim3_math.h"], fn
    for n in ("sim3_opt.hip", "essential_graph.hip"):
        assert '#include "sim3_math.h"' in SRC[n], n
    # host + device, no HIP header: the header stays compilable by g++
    assert "#include <hip" not in SRC["sim3_math.h"] and '#include "common.h"' not in SRC["sim3_math.h"]
    assert "__device__" not in SRC["sim3_math.h"] and "__syncthreads" not in SRC["sim3_math.h"]


def test_each_workspace_buffer_is_named_once():
    for n in ("local_ba.hip", "essential_graph.hip"):
        src = SRC[n]
        assert "struct Layout" not in src and "copy_in(" not in src and "carve.take(" not in src, n
        assert not re.search(r"reinterpret_cast<[^>]*>\s*\(\s*dev\b", src), n
        assert "WorkPlan measured;" in src and "WorkPlan plan(measured, dev, blob.data());" in src, n
        assert "void **" not in src, n
    assert "struct WorkPlan" in SRC["carve.h"] and "#include <hip" not in SRC["carve.h"]
    assert "EG_THREADS = 512" in SRC["essential_graph.hip"]


HOST_FLAVOURS = ("sim3.hip", "sim3_opt.hip", "pnp.hip", "initializer.hip", "local_ba.hip", "essential_graph.hip")


def test_the_host_flavours_declare_each_staging_segment_once():
    """the seven host flavours keep no take() list and no copy with a byte count of its own -- a segment's
    reservation, copies and device pointer all come from its one declaration on carve.h's HostPlan -- except the rows
    orbgpu_sim3_solve fetches after it has read the result, whose offsets are the handles'."""
    for n in HOST_FLAVOURS:
        src = SRC[n]
        assert "Carver in(16)" not in src and "Carver out(16)" not in src and "out.take(" not in src and "in.take(" not in src, n
        assert "HostPlan<N_BUF> plan;" in src and "host_begin(device_id, plan, wsp)" in src, n
        assert "plan.upload(ws);" in src and "plan.download(ws);" in src, n
        assert "ws.upload(" not in src, n
        assert ("ws.download(" in src) == (n == "sim3.hip"), n
    second_phase = re.findall(r"ws\.download\((\w+(?:\.data\(\))?), H_OUT, ([^,]+), (\w+)\.off \+ ", SRC["sim3.hip"])
    assert [(host, seg) for host, _, seg in second_phase] == [("R", "o_R"), ("t", "o_t"), ("s", "o_s"), ("T12", "o_T"),
                                                              ("mask.data()", "o_m")]
    assert SRC["sim3.hip"].count("ws.download(") == len(second_phase)
    # one body above the two bundle adjustment kernels
    assert SRC["local_ba.hip"].count("HostPlan<N_BUF> plan;") == 1 and SRC["local_ba.hip"].count("return ba_host<") == 2
    assert "struct HostPlan" in SRC["carve.h"] and "#include <hip" not in SRC["carve.h"] and '#include "common.h"' not in SRC["carve.h"]
    assert "void **" not in SRC["carve.h"]
