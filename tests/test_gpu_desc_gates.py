"""The descriptor-driven matchers' accept rules and gates on the hand-worked cases of desc_gate_cases.py: every entry point
that can express a case has to give the case's literal expectation exactly (test_desc_gates.py holds the oracle to the
same literals).

Table A runs through MatchBruteForce, search_by_bow and search_by_bow_keyframes at every shape of a case (as it is, and
padded with far fillers to na 33 / 70 and nb 63 / 65), and through BatchMatcher.match / .search_by_bow at cap 96 in
batches of 9, 3 and 1 pairs, which are one, four and sixteen B row ranges (nsplit) in k_bf_topk.  Table B runs through
search_for_triangulation and the match step of create_new_map_points and create_new_map_points_device.  The last test
asserts that every flavour and every nsplit was reached; it needs the module to have run."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(os.path.dirname(HERE), "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import desc_gate_cases as D  # noqa: E402
import proj_gate_cases as G  # noqa: E402
from bf_batch_pack import run as run_batch  # noqa: E402

pytestmark = pytest.mark.gpu

SEEN = set()    # flavours that gave a literal
NSPLIT = set()  # nsplit of every batched call
A_FLAVOURS = ("MatchBruteForce", "BatchMatcher.match", "search_by_bow", "BatchMatcher.search_by_bow", "search_by_bow_keyframes")
B_FLAVOURS = ("search_for_triangulation", "create_new_map_points", "create_new_map_points_device")


def same(tag, got, want, n=None):
    """Prints the differing rows, then says whether there are none (and the count is the literal's)."""
    bad = np.nonzero(np.asarray(got) != np.asarray(want))[0]
    n_want = int((np.asarray(want) >= 0).sum())
    if len(bad) or (n is not None and n != n_want):
        print(tag, "differs at rows", bad[:8], "got", np.asarray(got)[bad[:8]], "expected", np.asarray(want)[bad[:8]],
              "count", n, "expected", n_want)
    return len(bad) == 0 and (n is None or n == n_want)


@pytest.mark.parametrize("case", D.BF_CASES, ids=repr)
def test_table_a_through_the_host_entry_points(gpu, case):
    flavours = D.bf_flavours(case)
    ok = True
    for na, nb in D.bf_shapes(case):
        tag = "%s %dx%d" % (case, na, nb)
        if "MatchBruteForce" in flavours:
            pr = D.bf_problem(case, na, nb)
            n, mb = gpu.ORBmatcher(pr.ratio, pr.ori).MatchBruteForce(pr.a, pr.aa, pr.b, pr.ab, valid_a=pr.valid, th_low=pr.th)
            ok &= same(tag + " MatchBruteForce", mb, pr.want, n)
            SEEN.add("MatchBruteForce")
        pr = D.bf_problem(case, na, nb, nodes=True)
        if "search_by_bow" in flavours:
            n, mb = gpu.search_by_bow(pr.a, pr.aa, pr.valid, pr.node_a, pr.b, pr.ab, pr.node_b, pr.th, pr.ratio, pr.ori)
            ok &= same(tag + " search_by_bow", mb, pr.want, n)
            SEEN.add("search_by_bow")
        if "search_by_bow_keyframes" in flavours:
            n, m12 = gpu.search_by_bow_keyframes(pr.a, pr.aa, pr.valid, pr.node_a, pr.b, pr.ab, pr.valid_b, pr.node_b, pr.ratio,
                                                 pr.ori)
            ok &= same(tag + " search_by_bow_keyframes", m12, D.match12_of(pr.want, na), n)
            SEEN.add("search_by_bow_keyframes")
    assert ok


def batch_problems(flavour, pairs):
    """Every case the flavour can express, once, at a shape that moves on with the case and with the batch size, so that
    over the three batch sizes a case meets three of its shapes; sorted by call parameters so that a batch needs few calls."""
    prs = []
    for k, case in enumerate(D.BF_CASES):
        if flavour not in D.bf_flavours(case):
            continue
        shapes = D.bf_shapes(case)
        na, nb = shapes[(k + pairs) % len(shapes)]
        prs.append(D.bf_problem(case, na, nb, nodes=flavour == "BatchMatcher.search_by_bow"))
    return sorted(prs, key=lambda q: (q.th, q.ratio, q.ori, q.valid is not None))


@pytest.mark.parametrize("flavour", ["BatchMatcher.match", "BatchMatcher.search_by_bow"])
@pytest.mark.parametrize("pairs", [9, 3, 1])
def test_table_a_through_the_batched_entry_points(gpu, flavour, pairs):
    pytest.importorskip("torch")
    prs = batch_problems(flavour, pairs)
    assert len(prs) >= 30
    want_nsplit = {9: 1, 3: 4, 1: 16}[pairs]
    bm = gpu.BatchMatcher(pairs, D.CAP)
    ok = True
    try:
        for first in range(0, len(prs), pairs):
            group = prs[first:first + pairs]
            if len(group) < pairs:
                group = (group + prs)[:pairs]  # the last batch is filled up from the front: nsplit depends on the pair count
            out, launches = run_batch(bm, group, D.CAP)
            NSPLIT.update(l["nsplit"] for l in launches)
            assert all(l["nsplit"] == want_nsplit for l in launches), launches
            for pr, (n, mb, behind, _sweeps) in zip(group, out):
                ok &= same("%s %dx%d %s, %d pairs" % (pr.case, len(pr.a), len(pr.b), flavour, pairs), mb, pr.want, n)
                ok &= bool(np.all(behind == -1))
    finally:
        bm.close()
    assert ok
    SEEN.add(flavour)


# ---- Table B ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def newpts():
    import fuzz_newpts
    return fuzz_newpts


@pytest.mark.parametrize("case", D.TRI_CASES, ids=repr)
def test_table_b_on_the_device(gpu, newpts, case):
    torch = pytest.importorskip("torch")
    flavours = D.tri_flavours(case)
    ok = True
    if "search_for_triangulation" in flavours:
        f1, f2 = case.side(1), case.side(2)
        n, m12 = gpu.search_for_triangulation(D.TriView(gpu, f1), f1["has_mp"], f1["node"], D.TriView(gpu, f2), f2["has_mp"],
                                              f2["node"], case.F, float(case.epipole[0]), float(case.epipole[1]), D.SIGMA2,
                                              case.only_stereo, case.ori)
        ok &= same("%s search_for_triangulation" % case, m12, case.expect, n)
        SEEN.add("search_for_triangulation")
    sc = D.new_points_scene(case)
    if "create_new_map_points" in flavours:
        h = newpts.run_host(sc)
        ok &= h["n_done"] == 1 and same("%s create_new_map_points" % case, h["match12"][0], case.expect, int(h["n_matches"][0]))
        SEEN.add("create_new_map_points")
    d = newpts.run_device(torch, sc)
    ok &= d["n_done"] == 1 and same("%s create_new_map_points_device" % case, d["match12"][0], case.expect, int(d["n_matches"][0]))
    SEEN.add("create_new_map_points_device")
    assert ok


def test_octave_outside_the_levels_is_refused_where_the_host_can_see_it(gpu, newpts):
    """The guard case through the flavours that take host arrays: an error that names the key point, not a result."""
    case = [c for c in D.TRI_CASES if c.guard_only][0]
    f1, f2 = case.side(1), case.side(2)
    with pytest.raises(gpu.OrbGpuError) as ei:
        gpu.search_for_triangulation(D.TriView(gpu, f1), f1["has_mp"], f1["node"], D.TriView(gpu, f2), f2["has_mp"], f2["node"],
                                     case.F, float(case.epipole[0]), float(case.epipole[1]), D.SIGMA2, False, False)
    assert "key point 0: octave out of range" in str(ei.value)
    with pytest.raises(gpu.OrbGpuError) as ei:
        newpts.run_host(D.new_points_scene(case))
    assert "octave out of range" in str(ei.value)


# ---- the rotation bin at the sites that Tables A and B do not reach -----------------------------------------------------
@pytest.mark.parametrize("odd", [None, 1000.0, -1000.0, float("nan"), float("inf")], ids=str)
def test_initialization_drops_a_pair_without_a_bin(gpu, odd):
    """The host loop of orbgpu_search_for_initialization on proj_gate_cases.init_case() with the rotation check on: all
    angles 0 is one bin and keeps the four matches; row 4's angle 1000 degrees off, or no number, takes that pair alone."""
    f1, f2, prev, m12 = G.init_case()
    fr1, fr2 = G.make_frame(gpu, f1), G.make_frame(gpu, f2)
    want = m12.copy()
    if odd is not None:
        fr1.angle[4] = odd
        want[4] = -1
    n, out, _pm = gpu.search_for_initialization(fr1, fr2, prev, G.INIT_WINDOW, G.INIT_NNRATIO, True)
    assert same("search_for_initialization %s" % odd, out, want, n)


@pytest.mark.parametrize("odd", [None, 1000.0, float("nan")], ids=str)
def test_projection_finish_drops_a_pair_without_a_bin(gpu, odd):
    """k_proj_resolve's finish through SearchByProjection(CurrentFrame, LastFrame) with the rotation check on: row 10 of
    proj_gate_cases.last_case takes key point 7; with its angle 1000 degrees off, or no number, that key point alone is freed."""
    kps, last, expect = G.last_case("neither")
    want = expect.copy()
    if odd is not None:
        last["kp_angle"][10] = odd
        want[7] = -1
    n, k2m = gpu.ORBmatcher(0.9, True).SearchByProjectionLast(G.make_frame(gpu, kps), G.TCW, G.FX, G.FY, G.CX, G.CY, G.MBF, G.MB,
                                                              last, G.LAST_TH, False, np.full(len(kps), -1, np.int32))
    assert same("SearchByProjectionLast %s" % odd, k2m, want, n)


def test_zz_every_flavour_and_every_split_was_reached():
    print("flavours", sorted(SEEN), "nsplit", sorted(NSPLIT))
    assert SEEN == set(A_FLAVOURS) | set(B_FLAVOURS), sorted(set(A_FLAVOURS) | set(B_FLAVOURS) - SEEN)
    assert NSPLIT == {1, 4, 16}, sorted(NSPLIT)
