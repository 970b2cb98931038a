"""The hand-worked cases of the descriptor-driven matchers (desc_gate_cases.py) against the oracle, on the host: the oracle
has to give the literal expectation of every case, through each of its entry points that can express the case and at
every shape the device runs it at.  This is the half that tells a wrong kernel from a wrong oracle:
test_gpu_desc_gates.py holds the device to the same literals."""
import numpy as np
import pytest

import desc_gate_cases as D
import proj_gate_cases as G
from bf_batch_scenes import feature_vector


def oracle_bf(oracle, pr, flavour):
    """(nmatches, match_b) of a problem through one entry point of the oracle."""
    if flavour == "match_bf":
        return oracle.match_bf(pr.a, pr.aa, pr.b, pr.ab, valid_a=pr.valid, th_low=pr.th, nnratio=pr.ratio,
                               check_orientation=pr.ori)
    if flavour == "search_by_bow":
        return oracle.search_by_bow(pr.a, pr.aa, pr.valid, feature_vector(pr.node_a), pr.b, pr.ab, feature_vector(pr.node_b),
                                    pr.th, pr.ratio, pr.ori)
    n, m12 = oracle.search_by_bow_keyframes(pr.a, pr.aa, pr.valid, feature_vector(pr.node_a), pr.b, pr.ab, pr.valid_b,
                                            feature_vector(pr.node_b), pr.ratio, pr.ori)
    return n, m12


@pytest.mark.parametrize("case", D.BF_CASES, ids=repr)
def test_table_a_literal_is_the_oracles_answer(oracle, case):
    flavours = D.bf_flavours(case)
    seen = 0
    for na, nb in D.bf_shapes(case):
        if "MatchBruteForce" in flavours:
            pr = D.bf_problem(case, na, nb)
            n, mb = oracle_bf(oracle, pr, "match_bf")
            assert np.array_equal(mb, pr.want) and n == int((pr.want >= 0).sum()), (na, nb, mb[:8], np.nonzero(mb != pr.want)[0][:8])
            seen += 1
        pr = D.bf_problem(case, na, nb, nodes=True)
        if "search_by_bow" in flavours:
            n, mb = oracle_bf(oracle, pr, "search_by_bow")
            assert np.array_equal(mb, pr.want) and n == int((pr.want >= 0).sum()), (na, nb, mb[:8], np.nonzero(mb != pr.want)[0][:8])
            seen += 1
        if "search_by_bow_keyframes" in flavours:
            n, m12 = oracle_bf(oracle, pr, "search_by_bow_keyframes")
            want = D.match12_of(pr.want, na)
            assert np.array_equal(m12, want) and n == int((want >= 0).sum()), (na, nb, m12[:8])
            seen += 1
    assert seen >= len(D.bf_shapes(case))


def test_fillers_are_far_from_every_case_row_and_from_each_other():
    """What lets a literal stand at every shape: no filler is within 102 bits (D + 2 of the deepest setting, beyond every
    th_low) of a case row or of a filler of the other side.  The issue's bound of 90 is implied."""
    fa, fb = D.fillers()
    rows = D._case_rows()
    assert (len(fa), len(fb)) == (69, 64)
    assert D.hamming_matrix(fa, rows).min() >= 102 > 90 and D.hamming_matrix(fb, rows).min() >= 102
    assert D.hamming_matrix(fa, fb).min() >= 102
    assert max(D.list_depth(r, th) for r, th, _ in D.LIST_SETTINGS) == D.MAX_LISTED


def test_table_a_distances_are_what_the_comments_say():
    """low bits and bit ranges: |d1 - d2| between two prefixes; the tie rows are 20 from zero and 20 apart."""
    r = D.desc_rows([0, 20, (10, 30), (20, 40), 50, (1, 101)])
    m = D.hamming_matrix(r, r)
    assert m[0].tolist() == [0, 20, 20, 20, 50, 100] and m[1, 2] == 20 and m[1, 4] == 30 and m[2, 3] == 20


def test_every_shape_and_flavour_of_table_a_occurs():
    shapes = {s for c in D.BF_CASES for s in D.bf_shapes(c)}
    assert {x for x, _ in shapes} >= set(D.NA_SHAPES) and {y for _, y in shapes} >= set(D.NB_SHAPES)
    assert {f for c in D.BF_CASES for f in D.bf_flavours(c)} == {"MatchBruteForce", "BatchMatcher.match", "search_by_bow",
                                                                 "BatchMatcher.search_by_bow", "search_by_bow_keyframes"}


@pytest.mark.parametrize("case", [c for c in D.TRI_CASES if not c.guard_only], ids=repr)
def test_table_b_literal_is_the_oracles_answer(oracle, case):
    f1, f2 = case.side(1), case.side(2)
    n, m12 = oracle.search_for_triangulation(D.TriView(oracle, f1), f1["has_mp"], feature_vector(f1["node"]),
                                             D.TriView(oracle, f2), f2["has_mp"], feature_vector(f2["node"]), case.F,
                                             float(case.epipole[0]), float(case.epipole[1]), D.SIGMA2, case.only_stereo,
                                             case.ori)
    assert np.array_equal(m12, case.expect) and n == int((case.expect >= 0).sum()), m12


def test_the_guard_case_is_one_only_the_device_arrays_flavour_can_meet():
    """Every other Table B case keeps its octaves inside the levels, so the oracle (which has no guard) may read them."""
    for c in D.TRI_CASES:
        octv = c.side(2)["kp_octave"]
        assert c.guard_only == bool(((octv < 0) | (octv >= D.NLEVELS)).any()), c


def test_initialization_drops_a_pair_without_a_bin_in_the_oracle(oracle):
    """SearchForInitialization on proj_gate_cases.init_case() with the rotation check on: all angles 0 keeps the four
    matches (one bin); with row 4's angle 1000 degrees off, or no number, that pair alone goes."""
    f1, f2, prev, m12 = G.init_case()
    for odd in (None, 1000.0, G.NAN):
        fr1, fr2 = G.make_frame(oracle, f1), G.make_frame(oracle, f2)
        want = m12.copy()
        if odd is not None:
            fr1.angle[4] = odd
            want[4] = -1
        n, out, _pm = oracle.search_for_initialization(fr1, fr2, prev, G.INIT_WINDOW, G.INIT_NNRATIO, True)
        assert np.array_equal(out, want) and n == int((want >= 0).sum()), (odd, out)


@pytest.mark.parametrize("odd", [None, 1000.0, float("nan")], ids=str)
def test_projection_last_drops_a_pair_without_a_bin_in_the_oracle(oracle, odd):
    """SearchByProjection(CurrentFrame, LastFrame) on proj_gate_cases.last_case with the rotation check on: row 10 takes key
    point 7; with its angle 1000 degrees off, or no number, that key point alone is freed."""
    kps, last, expect = G.last_case("neither")
    want = expect.copy()
    if odd is not None:
        last["kp_angle"][10] = odd
        want[7] = -1
    n, k2m = oracle.search_by_projection_last(G.make_frame(oracle, kps), G.TCW, G.FX, G.FY, G.CX, G.CY, G.MBF, G.MB, last,
                                              G.LAST_TH, False, True, np.full(len(kps), -1, np.int32))
    assert np.array_equal(k2m, want) and n == int((want >= 0).sum()), (odd, k2m)
