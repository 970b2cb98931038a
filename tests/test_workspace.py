"""Host-only headers of the library ((thread, device) workspace lookup, id hash, the id tables' growth transaction, the
projection matchers' host boundary): compiled with plain g++ and run on the CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_workspace_lookup_is_per_thread_and_device(tmp_path):
    exe = str(tmp_path / "workspace_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-pthread", "-fsanitize=address,undefined",
                    "-I" + os.path.join(ROOT, "orb_slam2_map_amd", "csrc"), os.path.join(ROOT, "tests", "workspace_test.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "workspace_test ok" in r.stdout, r.stdout


def test_stateless_entry_points_use_the_lookup():
    """No entry point keeps a bare thread_local workspace object any more, and none keeps a release of its own: the stream,
    the buffers and their teardown are staging.h's."""
    import re
    csrc = os.path.join(ROOT, "orb_slam2_map_amd", "csrc")
    for name in ("matcher_bf.hip", "matcher_proj.hip", "pose_opt.hip", "sim3.hip", "stereo.hip"):
        src = open(os.path.join(csrc, name)).read()
        # the lookup itself, or staging.h's beginning of a solver / optimiser entry, which makes it
        assert "per_device_workspace<" in src or "batch_begin(" in src, name
        assert "static thread_local Ws ws" not in src and "static thread_local ProjWorkspace ws" not in src
        assert "static thread_local bool attr_set" not in src  # function attributes are per device as well
        assert "hipStreamCreateWithFlags" not in src and "hipStreamDestroy" not in src, name
        assert not re.search(r"DevBuf\s*\*\s*\w+\s*\[\s*\]", src), name       # DevBuf *bufs[] = {...}
        assert not re.search(r"\{\s*&\w+\s*,\s*&\w+", src), name             # for (DevBuf *b : {&a, &b, ...})
    staging = open(os.path.join(csrc, "staging.h")).read()
    assert "hipStreamCreateWithFlags" in staging and "hipStreamDestroy" in staging and "release_workspace(" in staging
    assert staging.count("per_device_workspace<Ws>(device_id)") == 3  # batch_begin, host_begin, last_spills
    lookup = open(os.path.join(csrc, "workspace.h")).read()
    assert "#include <hip" not in lookup and '#include "common.h"' not in lookup and "staging.h" in lookup


def test_id_hash_and_pointer_index(tmp_path):
    """The id tables' id -> row hash (insert, find and the lookup the kernels run, slot_for, the capacity rule, growth,
    clear, the rollback of a refused call) and the shim's pointer index against std::map / a linear search, under
    AddressSanitizer + UBSan."""
    exe = str(tmp_path / "id_hash_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-I" + os.path.join(ROOT, "orb_slam2_map_amd", "csrc"), "-I" + os.path.join(ROOT, "orb_slam2_map_amd", "shim"),
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "id_hash_test.cpp"), "-o", exe, "-pthread"],
                   check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "id_hash ok" in r.stdout and "ptr_index ok" in r.stdout, r.stdout


def test_id_table_growth_transaction(tmp_path):
    """id_table.h over malloc-backed buffers and recording operations, under AddressSanitizer + UBSan: growth and a
    retain-style compaction of a small table with every allocation and every operation failed once -- the code returned,
    the table bit for bit what it was, a sync before the first new buffer is freed, no leak -- and then unfailed: contents
    carried over, every id found by id_hash_lookup over the uploaded copy, the old buffers freed exactly once."""
    exe = str(tmp_path / "id_table_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pthread", "-fsanitize=address,undefined",
                    "-I" + os.path.join(ROOT, "orb_slam2_map_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "id_table_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "id_table_test ok" in r.stdout, r.stdout


def test_id_tables_share_one_core():
    """map_table.hip and kfdb.hip keep no lookup, no carve-out, no capacity loop and no growth of their own: the hash is
    id_hash.h's, the transaction id_table.h's, which stays compilable without HIP."""
    import re
    csrc = os.path.join(ROOT, "orb_slam2_map_amd", "csrc")
    for name in ("map_table.hip", "kfdb.hip"):
        src = open(os.path.join(csrc, name)).read()
        assert "id_hash_lookup(" in src and '#include "id_table.h"' in src, name
        assert not re.search(r"\b\w+_lookup\s*\([^;{]*\)\s*\{", src), name      # a function definition named *_lookup
        assert not re.search(r"struct\s+Carve", src), name
        assert not re.search(r"while\s*\(\s*\(.*<<\s*l2\s*\)\s*<", src) and "l2++" not in src, name  # the capacity loop
        assert "hash_slot_for" not in src, name
        assert "id_table_grow(" in src, name
    table = open(os.path.join(csrc, "map_table.hip")).read()
    assert "id_table_replace(" in table and table.count("&world_pos") == 1 and table.count("&t->world_pos") == 0
    core = open(os.path.join(csrc, "id_table.h")).read()
    assert "#include <hip" not in core and '#include "common.h"' not in core and '#include "carve.h"' in core
    assert "struct Carver" in open(os.path.join(csrc, "carve.h")).read()
    assert "l2++" in open(os.path.join(csrc, "id_hash.h")).read()


def _host_program(tmp_path, name, *flags):
    """tests/<name>.cpp built for the CPU under AddressSanitizer + UBSan; returns the program's path"""
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined"] + list(flags) +
                   ["-I" + os.path.join(ROOT, "orb_slam2_map_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", name + ".cpp"), "-o", exe], check=True)
    return exe


def test_carver_offsets_and_the_host_flavours_layouts(tmp_path):
    """carve.h at alignments 16 and 256 over the sizes 0, 1, 15, 16, 17, 255, 256, 257 in sequence (aligned, no overlap,
    each offset (prev + bytes + A - 1) & ~(A - 1)), and HostPlan through a recording workspace whose blocks and caller
    arrays are heap blocks of exactly the reserved and the documented lengths: the segment lists of the seven host
    flavours at n1 in {0, 1, 15, 16, 17, 64, 65} x H in {0, 1, 3} x min_set in {4, 5} x n2 in {0, 1, 17}, n_local / n_poses
    in {0, 1, 3} x M in {0, 1, 5} x E in {0, 1, 7}, V in {0, 1, 3}, optional outputs given and null -- offsets and block
    sizes against the hand-summed formulas the entry points held before, the copies (direction, buffer, offset, bytes,
    host address) against the guards they held, none for a null pointer, rows == 0 or words == 0; and one copy more than
    the plan holds."""
    r = subprocess.run([_host_program(tmp_path, "carve_test")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "carve_test ok" in r.stdout, r.stdout


def test_mask_to_bytes(tmp_path):
    """ransac_host.h's mask_to_bytes at n in {0, 1, 63, 64, 65, 130} over heap arrays of exactly (n + 63) / 64 words and n
    bytes against a per-bit loop."""
    r = subprocess.run([_host_program(tmp_path, "ransac_host_test", "-ffp-contract=off"), "masks"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "mask_to_bytes ok" in r.stdout, r.stdout


def test_ransac_max_iterations_equals_both_models(tmp_path):
    """ransac_host.h's ransac_max_iterations, fed as sim3.hip and pnp.hip feed it, equals sim3_model.ransac_iterations and
    the second value of pnp_model.ransac_parameters on the argument tables of test_sim3_abi.py and test_pnp_abi.py and on
    the hostile tuples of test_sim3_model.py::test_ransac_iterations."""
    import struct
    import sys
    import numpy as np
    if os.path.join(ROOT, "tests") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pnp_model
    import sim3_model
    f32 = np.float32
    lines, want = [], []

    def feed(n, nmin, eps, p, mx, expected):
        lines.append("%d %d %x %x %d" % (n, nmin, struct.unpack("<I", struct.pack("<f", eps))[0],
                                         struct.unpack("<Q", struct.pack("<d", p))[0], mx))
        want.append(expected)

    sim3 = [(n, p, mi, mx) for n in (0, 1, 3, 19, 20, 21, 25, 64, 100, 300, 2816, 10 ** 6) for p in (0.99, 0.5, 0.999, 1.0, 0.0, 1.5)
            for mi in (0, 1, 6, 20, 21) for mx in (0, 1, 5, 300)]
    sim3 += [(50, 1.0, 6, 300), (7, 1.5, 3, 10), (10 ** 6, 0.99, 1, 300), (30, 0.5, 29, 0)]
    pnp = [(n, p, mi, mx, ms, eps) for n in (0, 1, 3, 9, 10, 11, 25, 64, 100, 300, 1200, 10 ** 6) for p in (0.99, 0.5, 1.0, 0.0, 1.5)
           for mi in (0, 1, 10, 50) for mx in (0, 1, 300) for ms in (4, 6) for eps in (0.5, 0.4, 0.0, 1.0, 2.5, -1.0, float("nan"), 1e30)]
    with np.errstate(all="ignore"):
        for n, p, mi, mx in sim3:  # sim3.hip: eps = (float)min_inliers / (float)n
            feed(n, mi, f32(mi) / f32(n), p, mx, sim3_model.ransac_iterations(n, p, mi, mx))
        for n, p, mi, mx, ms, eps in pnp:  # pnp.hip: the adjusted nmin, eps raised to nmin / n
            nmin, its = pnp_model.ransac_parameters(n, p, mi, mx, ms, eps)
            ratio = f32(nmin) / f32(n)
            feed(n, nmin, ratio if f32(eps) < ratio else f32(eps), p, mx, its)
    exe = _host_program(tmp_path, "ransac_host_test", "-ffp-contract=off")
    r = subprocess.run([exe, "table"], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    got = [int(x) for x in r.stdout.split()]
    assert len(got) == len(want) == len(sim3) + len(pnp)
    assert got == want, [(a, g, w) for a, g, w in zip(lines, got, want) if g != w][:10]


def test_solver_entry_points_share_one_host_scaffold():
    """The solver / optimiser units keep no layout arithmetic, no entry prologue and no iteration-cap expression of
    their own: the offsets are carve.h's, the typed pointers and the two beginnings staging.h's, the cap ransac_host.h's --
    and the two new headers stay compilable without HIP."""
    import re
    csrc = os.path.join(ROOT, "orb_slam2_map_amd", "csrc")
    read = lambda name: open(os.path.join(csrc, name)).read()  # noqa: E731
    for name in ("pose_opt.hip", "sim3.hip", "sim3_opt.hip", "pnp.hip", "local_ba.hip", "essential_graph.hip"):
        src = read(name)
        assert "auto pad =" not in src, name
        assert not re.search(r"reinterpret_cast<[^>]*>\s*\(\s*d(in|out)\b", src), name
        assert "batch_begin(" in src and "n <= 65535" not in src, name
    for name in ("sim3.hip", "sim3_opt.hip", "pnp.hip"):
        src = read(name)
        assert "hipDeviceSynchronize" not in src and "host_begin(" in src and "HostPlan<N_BUF> plan;" in src, name
    for name in ("local_ba.hip", "essential_graph.hip"):  # one staging block for the outputs (local_ba) or each way
        assert "hipDeviceSynchronize" not in read(name) and "host_begin(" in read(name), name
    for name in ("sim3.hip", "pnp.hip"):
        assert "std::pow(" not in read(name) and "ransac_max_iterations(" in read(name), name
    for name in ("sim3.hip", "pnp.hip", "map_table.hip"):
        assert "mask_to_bytes(" in read(name) and ">> (i & 63)" not in read(name), name
    staging = read("staging.h")
    assert "hipDeviceSynchronize" in staging and "int host_begin(" in staging and "int batch_begin(" in staging
    assert "n <= 65535" in staging and '"bad arguments"' in staging
    assert "std::pow(" in read("ransac_host.h")
    for name in ("carve.h", "ransac_host.h"):
        assert "#include <hip" not in read(name) and '#include "common.h"' not in read(name), name


def test_projection_boundary_on_the_host(tmp_path):
    """The host half of the projection matchers (proj_boundary.h: projections, gates, levels and flags per flavour, claim
    tables, the Sim3 decomposition against the oracle's, bit for bit) and the rotation check's host build, on hand-derived
    values under AddressSanitizer + UBSan."""
    # float-cast-overflow is not part of `undefined`: with it, and no recovery, a conversion of NaN or of a float no int
    # holds ends the program, so the non-finite level rows also show that no builder converts before it tests
    san = ["-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined,float-cast-overflow",
           "-fno-sanitize-recover=float-cast-overflow"]
    inc = ["-I" + os.path.join(ROOT, d) for d in (os.path.join("orb_slam2_map_amd", "csrc"), "include", "oracle")]
    obj, exe = str(tmp_path / "orb_oracle_match.o"), str(tmp_path / "proj_boundary_test")
    subprocess.run(["gcc", "-std=c11", "-Wno-unused-parameter"] + san + inc +
                   ["-c", os.path.join(ROOT, "oracle", "orb_oracle_match.c"), "-o", obj], check=True)
    subprocess.run(["g++", "-std=c++17"] + san + inc + [os.path.join(ROOT, "tests", "proj_boundary_test.cpp"), obj, "-o", exe],
                   check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "proj_boundary_test ok" in r.stdout, r.stdout


def test_projection_float_conventions_live_in_the_boundary_header():
    """Every `volatile` temporary that pins a float convention of the projection matchers' host side is in proj_boundary.h,
    which stays compilable without HIP."""
    csrc = os.path.join(ROOT, "orb_slam2_map_amd", "csrc")
    assert "volatile" not in open(os.path.join(csrc, "matcher_proj.hip")).read()
    boundary = open(os.path.join(csrc, "proj_boundary.h")).read()
    assert "volatile" in boundary and "#include <hip" not in boundary and '#include "common.h"' not in boundary
