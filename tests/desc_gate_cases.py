"""Hand-worked cases for the accept rules and gates of the descriptor-driven matchers (test-side helper, shared by
test_desc_gates.py on the host and test_gpu_desc_gates.py on the device), in the style of proj_gate_cases.py: every case
is a few rows built directly, and carries its expected result as a literal that is worked out in the comment beside it
from the reference lines the kernels cite -- never from the code under test.  Where a float32 product decides, it is
computed here with np.float32 and asserted against the literal.

Table A (BF_CASES): ORBmatcher::SearchByBoW(KeyFrame*, Frame&) :159-288, lines :201-249, and the key-frame flavour
:522-655, lines :566-618.  A descriptor is given as d (the low d bits set) or (lo, hi) (bits lo..hi-1 set), so two rows d1
and d2 are |d1 - d2| apart: rows are places on a line.  expect[j] is the A row that takes B row j (match_b).

Table B (TRI_CASES): ORBmatcher::SearchForTriangulation :657-823 with CheckDistEpipolarLine :140-157.  With
F12 = [[0, 0, 0], [0, 0, -1], [0, 1, 0]] the line of key point (kx, ky) is a = 0, b = 1, c = -ky, so den = 1 and
dsqr = (py - ky)^2; every row of key frame 1 lies on y = 0, so num is the candidate's y itself, exactly.
expect[i] is the key point of key frame 2 that row i takes (match12)."""
from types import SimpleNamespace

import numpy as np

from proj_gate_cases import F32, NAN, NLEVELS, SF, TH_LOW, low_bits, up

INF = F32(np.inf)


def desc_row(spec):
    """d: the low d bits; (lo, hi): bits lo..hi-1."""
    if isinstance(spec, tuple):
        lo, hi = spec
        return low_bits(hi) ^ low_bits(lo)
    return low_bits(int(spec))


def desc_rows(specs):
    return np.stack([desc_row(s) for s in specs]) if len(specs) else np.zeros((0, 32), np.uint8)


_POP = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1).astype(np.int64)


def hamming_matrix(a, b):
    return _POP[a[:, None, :] ^ b[None, :, :]].sum(-1)


# ======================================================================================================================
# Table A
# ======================================================================================================================
def list_depth(nnratio, th_low):
    """D: the smallest second distance >= th_low whose successor can no longer fail the ratio test for any best <= th_low,
    i.e. the smallest D >= th_low with nnratio * (D + 1) > th_low in float32.  A second at D + 1 or beyond need not be
    listed for a row: whatever it is, the row is kept."""
    d = int(th_low)
    while not F32(nnratio) * F32(d + 1) > F32(th_low):
        d += 1
    return d


def ratio_keeps(best, second, nnratio):
    """(float)bestDist1 < mfNNratio * (float)bestDist2 (:230), in float32."""
    return bool(F32(best) < F32(nnratio) * F32(second))


class BfCase:
    """One (A, B) pair.  a, b: descriptor specs; valid_b only exists in the key-frame flavour (a key point of key frame 2
    without a good map point, :574-580).  th_low 49 is the key-frame flavour's `bestDist1 < TH_LOW` (:598) on integers: a
    case of th_low 49 is one that the key-frame flavour can express, and the other flavours run it with th_low = 49.
    angle_a / angle_b and ori: the rotation check (:238-243, :262-281)."""

    def __init__(self, name, a, b, expect, nnratio=0.7, th_low=TH_LOW, valid_a=None, valid_b=None, node_a=None, node_b=None,
                 angle_a=None, angle_b=None, ori=False):
        self.name, self.nnratio, self.th_low, self.ori = name, float(nnratio), int(th_low), bool(ori)
        self.a, self.b = desc_rows(a), desc_rows(b)
        self.expect = np.array(expect, np.int32)
        self.valid_a = None if valid_a is None else np.array(valid_a, np.uint8)
        self.valid_b = None if valid_b is None else np.array(valid_b, np.uint8)
        self.node_a = None if node_a is None else np.array(node_a, np.int32)
        self.node_b = None if node_b is None else np.array(node_b, np.int32)
        self.angle_a = np.zeros(len(a), F32) if angle_a is None else np.array(angle_a, F32)
        self.angle_b = np.zeros(len(b), F32) if angle_b is None else np.array(angle_b, F32)
        assert len(self.expect) == len(b) and (node_a is None) == (node_b is None)
        assert len(self.angle_a) == len(a) and len(self.angle_b) == len(b)
        # the (10, 256) setting lists every row there is: it runs without fillers
        self.fillers = not (self.th_low >= 256)

    def __repr__(self):
        return self.name


# ---- the float32 products that decide ---------------------------------------------------------------------------------
# 0.7f * 50.f = 34.9999994 rounds to the float 35; 0.5f * 50.f = 25 exactly; 0.9f * 50.f = 44.9999988 rounds to 45: in all
# three the integer ON the product is not below it (strict `<`), the one under it is
assert F32(0.7) * F32(50) == F32(35) and F32(0.5) * F32(50) == F32(25) and F32(0.9) * F32(50) == F32(45)
assert not ratio_keeps(35, 50, 0.7) and ratio_keeps(34, 50, 0.7)
assert not ratio_keeps(25, 50, 0.5) and ratio_keeps(24, 50, 0.5)
assert not ratio_keeps(45, 50, 0.9) and ratio_keeps(44, 50, 0.9)
assert F32(0.6) * F32(40) == F32(24) and float(F32(0.6)) * 40 > 24 and not ratio_keeps(24, 40, 0.6) and ratio_keeps(23, 40, 0.6)
# 0.7f * 72 = 50.4 > 50 and 0.7f * 71 = 49.7; 0.6f * 84 = 50.4 and 0.6f * 83 = 49.8; 2 * 101 > 100 at once
LIST_SETTINGS = [(0.7, 50, 71), (0.6, 50, 83), (2.0, 100, 100)]  # (nnratio, th_low, D)
for _r, _th, _d in LIST_SETTINGS:
    assert list_depth(_r, _th) == _d
MAX_LISTED = 100  # the largest D: fillers stay beyond D + 1 of every setting


def _list_cases():
    """best = th_low against second = D is decided by the ratio in float32; a second at D + 1 is never listed and the row
    must be kept all the same; then the same two seconds under best = th_low - 1."""
    #            best th, second D         th, D + 1   th - 1, D   th - 1, D + 1
    kept = {(0.7, 50): (False,             True,       True,       True),   # 50 < 49.7 no; 50 < 50.4; 49 < 49.7; 49 < 50.4
            (0.6, 50): (False,             True,       True,       True),   # 50 < 49.8 no; 50 < 50.4; 49 < 49.8; 49 < 50.4
            (2.0, 100): (True,             True,       True,       True)}   # 100 < 200; 100 < 202; 99 < 200; 99 < 202
    out = []
    for r, th, d in LIST_SETTINGS:
        pairs = [(th, d), (th, d + 1), (th - 1, d), (th - 1, d + 1)]
        for (best, second), k in zip(pairs, kept[(r, th)]):
            assert ratio_keeps(best, second, r) == k, (r, best, second)
            # best == second (the (2.0, 100) setting, D = th_low): two rows at one distance, the lower index is the best
            b = [best, (1, second + 1)] if best == second else [best, second]
            out.append(BfCase("list_r%g_th%d_best%d_second%d" % (r, th, best, second), [0], b, [0 if k else -1, -1],
                              nnratio=r, th_low=th))
    return out


BF_CASES = [
    # ---- bestDist1 <= TH_LOW (:228): 50 is kept, 51 is not; a sole candidate leaves bestDist2 = 256 (:203): 50 < 179.2
    BfCase("th_low_50_sole", [0], [50], [0]),
    BfCase("th_low_51_sole", [0], [51], [-1]),
    # ---- key-frame flavour, bestDist1 < TH_LOW (:598): 49 is kept, 50 is not
    BfCase("kf_49_sole", [0], [49], [0], th_low=49),
    BfCase("kf_50_sole", [0], [50], [-1], th_low=49),
    # ---- the ratio is strict and in float (:230)
    BfCase("ratio_07_35_50", [0], [35, 50], [-1, -1], nnratio=0.7),
    BfCase("ratio_07_34_50", [0], [34, 50], [0, -1], nnratio=0.7),
    BfCase("ratio_05_25_50", [0], [25, 50], [-1, -1], nnratio=0.5),
    BfCase("ratio_05_24_50", [0], [24, 50], [0, -1], nnratio=0.5),
    BfCase("ratio_09_45_50", [0], [45, 50], [-1, -1], nnratio=0.9),
    BfCase("ratio_09_44_50", [0], [44, 50], [0, -1], nnratio=0.9),
    # 0.6f * 40.f is 24.00000095..., exactly half way between 24 and the next float: it rounds to even, 24.0, and 24 < 24 cuts;
    # a product kept in double (or a fused one) would keep the row
    BfCase("ratio_06_24_40_product_rounds_to_24", [0], [24, 40], [-1, -1], nnratio=0.6),
    BfCase("ratio_06_23_40", [0], [23, 40], [0, -1], nnratio=0.6),
    # the same pairs with the second listed first: best and second do not depend on the order of unequal rows (:216-225)
    BfCase("ratio_07_50_35", [0], [50, 35], [-1, -1], nnratio=0.7),
    BfCase("ratio_07_50_34", [0], [50, 34], [-1, 0], nnratio=0.7),
    # ---- ties: `dist < bestDist1` (:216) keeps the first of two rows at the least distance, and `else if (dist < bestDist2)`
    # (:222) makes the other the second: 20 < r * 20 fails for every nnratio <= 1; nnratio 10 keeps the lower index.
    # Bits 0..19 and bits 10..29 are both 20 from the all-zero row (and 20 from each other).
    BfCase("tie_nnratio_07", [0], [20, (10, 30)], [-1, -1], nnratio=0.7),
    BfCase("tie_nnratio_1", [0], [20, (10, 30)], [-1, -1], nnratio=1.0),
    BfCase("tie_nnratio_10", [0], [20, (10, 30)], [0, -1], nnratio=10.0, th_low=256),
    BfCase("tie_nnratio_10_three", [0], [30, (5, 25), 20], [-1, 0, -1], nnratio=10.0, th_low=256),  # 30, 20, 20: the first 20
    # ---- claimed rows are skipped before the distance (:209-210).  Row 0 (the zero row) sees j0 at 10 and j1 at 50:
    # 10 < 35, it takes j0.  Row 1 (30) sees j0 at 20 and j1 at 20: j0 is skipped, so j1 is the best with bestDist2 = 256
    # and is taken; were j0 still counted, 20 < 0.7 * 20 would cut the row.
    BfCase("claimed_row_is_skipped", [0, 30], [10, 50], [0, 1]),
    # Rows 0..3 are copies of j0..j3 (0 against a second 10 away: 0 < 7) and take them in turn; row 3 (40) has j4 (60) as
    # its second: 0 < 14.  Row 4 (25) sees j1 and j2 at 5, j0 and j3 at 15, all claimed, and j4 at 35: its only free
    # candidate is the fifth nearest, with bestDist2 = 256: taken.
    BfCase("only_the_fifth_nearest_is_free", [10, 20, 30, 40, 25], [10, 20, 30, 40, 60], [0, 1, 2, 3, 4]),
    # ---- a cut row claims nothing: row 0 sees j0 at 20 and j1 at 25: 20 < 17.5 fails.  Row 1 (18) sees j0 at 2 and j1 at 7:
    # 2 < 4.9, it takes j0; had row 0 claimed j0, row 1 would have taken j1 (7, alone)
    BfCase("cut_row_claims_nothing", [0, 18], [20, 25], [1, -1]),
    # ---- valid_a = 0 (:195-199): row 0 is a copy of j0 and is no row.  Row 1 (12) sees j0 at 2 and j1 at 18: 2 < 12.6
    BfCase("invalid_a_neither_matches_nor_claims", [10, 12], [10, 30], [1, -1], valid_a=[0, 1]),
    # ---- key-frame flavour, valid2 = 0 (:574-580): j0 at 5 would be the best, j2 at 35 would be the second that cuts
    # (30 < 24.5 fails); both are no candidates, so j1 at 30 is alone
    BfCase("kf_invalid_b_is_neither_best_nor_second", [0], [5, 30, 35], [-1, 0, -1], th_low=49, valid_b=[0, 1, 0],
           node_a=[7], node_b=[7, 7, 7]),
    # ---- nodes (:180-190: only the rows of one node meet).  Row 0 (node 7) has j2 at 30 under its node; j0 at 5 (node 8)
    # and j1 at 6 (no node) would be nearer, j3 at 35 (node 8) would cut as the second.  Row 1 (no node) is a copy of j2
    # and never matches.  Row 2 (node 8) is a copy of j0: 0 against j3 at 30.  Rows of different nodes do not interact.
    BfCase("nodes", [0, 30, 5], [5, 6, 30, 35], [2, -1, 0, -1], node_a=[7, -1, 8], node_b=[8, -1, 7, 8]),
    # a claim holds inside a node only in so far as B rows are of one node: rows 0 and 1 (node 7) both want j0, row 1
    # gets j1; row 2 (node 8) is a copy of j0 too but j0 is not of its node: it takes j2 at 40 (alone)
    BfCase("nodes_claims", [10, 10, 10], [10, 14, 50], [0, 1, 2], node_a=[7, 7, 8], node_b=[7, 7, 8]),
    # ---- rotation (:238-243, :262-281).  Six rows, each a copy of its B row (0 against 10: kept); differences 0, 0, 0 are
    # bin 0, 90 is bin 3: the maxima are bin 0 with 3 and bin 3 with 1 (1 < 0.1f * 3 fails: kept), there is no third.
    # Row 4 is 1000 degrees off (quotient 33) and row 5 has no angle at all: neither has a bin, neither votes, both go.
    BfCase("rotation_pairs_without_a_bin", [10, 20, 30, 40, 50, 60], [10, 20, 30, 40, 50, 60], [0, 1, 2, 3, -1, -1],
           angle_a=[0, 0, 0, 90, 1000, NAN], ori=True),
    # the same with the odd angles on the B side and the difference negative: -1000 + 360 = -640, quotient -21; -inf
    BfCase("rotation_pairs_without_a_bin_b_side", [10, 20, 30, 40, 50, 60], [10, 20, 30, 40, 50, 60], [0, 1, 2, 3, -1, -1],
           angle_a=[10, 10, 10, 100, 0, 0], angle_b=[10, 10, 10, 10, 1000, INF], ori=True),
    # the check itself: bins 0, 0, 0, 1, 1, 2, 2, 3: the three maxima are 0, 1, 2 and the pair in bin 3 goes
    BfCase("rotation_fourth_bin", [10, 20, 30, 40, 50, 60, 70, 80], [10, 20, 30, 40, 50, 60, 70, 80],
           [0, 1, 2, 3, 4, 5, 6, -1], angle_a=[0, 0, 0, 30, 30, 60, 60, 90], ori=True),
] + _list_cases()

NA_SHAPES, NB_SHAPES, CAP = (1, 33, 70), (1, 63, 65), 96
FILLER_SEED, FILLER_MIN = 41, MAX_LISTED + 2


def _case_rows():
    return np.concatenate([np.concatenate([c.a, c.b]) for c in BF_CASES])


_fillers = {}


def fillers():
    """(A fillers [69][32], B fillers [64][32]): random descriptors, each drawn again until it is at least FILLER_MIN = 102
    bits from every case row of this file and from every filler of the other side.  That is beyond D + 1 of every setting
    (no filler is ever a best or a second that matters, nor listed) and beyond every th_low (no filler row matches)."""
    if not _fillers:
        rng = np.random.default_rng(FILLER_SEED)
        rows = _case_rows()
        fa, fb = np.zeros((0, 32), np.uint8), np.zeros((0, 32), np.uint8)

        def draw(others):
            for _ in range(1000):
                r = rng.integers(0, 256, (1, 32), dtype=np.uint8)
                if hamming_matrix(r, rows).min() >= FILLER_MIN and (len(others) == 0 or hamming_matrix(r, others).min() >= FILLER_MIN):
                    return r
            raise AssertionError("no filler row found: choose another seed")
        while len(fa) < max(NA_SHAPES) - 1 or len(fb) < max(NB_SHAPES) - 1:
            if len(fa) < max(NA_SHAPES) - 1:
                fa = np.concatenate([fa, draw(fb)])
            if len(fb) < max(NB_SHAPES) - 1:
                fb = np.concatenate([fb, draw(fa)])
        # what the issue asks to hold on the CPU: every filler is at least 90 from every case row (here 102)
        assert hamming_matrix(fa, rows).min() >= 90 and hamming_matrix(fb, rows).min() >= 90
        assert hamming_matrix(fa, fb).min() >= FILLER_MIN
        _fillers["a"], _fillers["b"] = fa, fb
    return _fillers["a"], _fillers["b"]


def bf_shapes(case):
    """The (na, nb) a case runs at: as it is, and padded with fillers to every larger shape of NA_SHAPES x NB_SHAPES (1 only
    for a case that has one row on that side)."""
    na, nb = len(case.a), len(case.b)
    out = [(na, nb)]
    if case.fillers:
        out += [(x, y) for x in NA_SHAPES for y in NB_SHAPES
                if (x, y) != (na, nb) and (x > na or x == na == 1) and (y > nb or y == nb == 1) and x >= na and y >= nb]
    return out


def bf_problem(case, na=None, nb=None, nodes=False):
    """The case at shape (na, nb) as a problem of tools/bf_batch_pack.py: case rows first, then fillers (angle 0, valid, and
    under `nodes` spread over the case's node ids and -1).  `want`: the literal, -1 on the filler rows.  nodes=True gives a
    case without nodes one node for all its rows, which is how the node-wise entry points express it."""
    na, nb = na or len(case.a), nb or len(case.b)
    ka, kb = len(case.a), len(case.b)
    assert na >= ka and nb >= kb and (case.fillers or (na, nb) == (ka, kb))
    fa, fb = fillers() if (na, nb) != (ka, kb) else (None, None)
    pad = lambda rows, f, n, k: rows if n == k else np.concatenate([rows, f[:n - k]])  # noqa: E731
    ext = lambda v, n, fill: np.concatenate([v, np.full(n - len(v), fill, v.dtype)])  # noqa: E731
    pr = SimpleNamespace(a=pad(case.a, fa, na, ka), b=pad(case.b, fb, nb, kb), aa=ext(case.angle_a, na, 0),
                         ab=ext(case.angle_b, nb, 0), valid=None if case.valid_a is None else ext(case.valid_a, na, 1),
                         valid_b=None if case.valid_b is None else ext(case.valid_b, nb, 1), node_a=None, node_b=None,
                         ratio=case.nnratio, th=case.th_low, ori=case.ori, case=case,
                         want=ext(case.expect, nb, -1))
    if nodes or case.node_a is not None:
        la = np.full(ka, 7, np.int32) if case.node_a is None else case.node_a
        lb = np.full(kb, 7, np.int32) if case.node_b is None else case.node_b
        ids = sorted(set(la.tolist()) | set(lb.tolist()) | {-1})
        pr.node_a = np.concatenate([la, np.array([ids[k % len(ids)] for k in range(na - ka)], np.int32)])
        pr.node_b = np.concatenate([lb, np.array([ids[(k + 1) % len(ids)] for k in range(nb - kb)], np.int32)])
    pr.want.setflags(write=False)
    return pr


def match12_of(match_b, na):
    """The key-frame flavour's table, indexed by key frame 1 (matches are one to one, vbMatched2 :576, :603)."""
    out = np.full(na, -1, np.int32)
    for j, i in enumerate(match_b):
        if i >= 0:
            out[i] = j
    return out


def bf_flavours(case):
    """Which entry points can express a case: valid_b exists in the key-frame flavour alone, which in turn has th_low fixed
    at `< 50` and no brute-force form; a case with nodes needs a node-wise entry."""
    if case.valid_b is not None:
        return ("search_by_bow_keyframes",)
    out = ("search_by_bow", "BatchMatcher.search_by_bow")
    if case.node_a is None:
        out = ("MatchBruteForce", "BatchMatcher.match") + out
    if case.th_low == 49:
        out = out + ("search_by_bow_keyframes",)
    return out


# ======================================================================================================================
# Table B
# ======================================================================================================================
F12 = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], F32)
SIGMA2 = SF * SF  # mvLevelSigma2[i] = mvScaleFactor[i] * mvScaleFactor[i] in float (ORBextractor.cc:423)
FAR = (5000.0, 5000.0)  # an epipole far from every key point: the gate of :743-749 passes
CHI2 = 3.84


def line_passes(dy, octave):
    """CheckDistEpipolarLine (:140-157) for num = dy, den = 1: dsqr = num * num / den is a float, 3.84 * sigma2 a double."""
    dsqr = F32(F32(dy) * F32(dy))
    return bool(float(dsqr) < CHI2 * float(SIGMA2[octave]))


def epipole_skips(dist, octave):
    """:743-749 for a candidate `dist` left of the epipole on its row: distex * distex + 0 < 100 * scale, in float."""
    d = F32(dist)
    return bool(F32(d * d) < F32(100) * SF[octave])


# octave 0: 1.959^2 = 3.8377 < 3.84 <= 1.96^2 = 3.8416; octave 1, sigma2 = 1.44000006: 2.351^2 = 5.5272 < 5.5296 <= 2.352^2
assert line_passes(1.959, 0) and not line_passes(1.96, 0) and line_passes(2.351, 1) and not line_passes(2.352, 1)
DY_384F = F32(1.9595917)
assert F32(DY_384F * DY_384F) == F32(3.84) and line_passes(DY_384F, 0) and not F32(DY_384F * DY_384F) < F32(3.84) * SIGMA2[0]
assert not line_passes(up(DY_384F), 0)
# the epipole at x = 300: 300 - 290 = 10 exactly, 100 is not < 100; 300 - 290.01f = 9.98999, 99.8; octave 1: 100 * 1.2f = 120.0000048
# rounds to the float above 120: 11^2 = 121; 300 - 289.05f = 10.950012, 119.9
EPI_X = 300.0
for _x, _o, _skip in ((290.0, 0, False), (290.01, 0, True), (289.0, 1, False), (289.05, 1, True)):
    assert epipole_skips(F32(EPI_X) - F32(_x), _o) == _skip, _x
assert F32(100) * SF[1] == up(120)


def k1(x, ur=-1.0, node=10, has=0, bits=0, angle=0.0):
    """A key point of key frame 1: always on y = 0."""
    return (x, 0.0, 0, ur, node, has, bits, angle)


def k2(x, y=0.0, octave=0, ur=-1.0, node=10, has=0, bits=0, angle=0.0):
    return (x, y, octave, ur, node, has, bits, angle)


class TriCase:
    def __init__(self, name, rows1, rows2, expect, F=F12, epipole=FAR, only_stereo=False, ori=False, guard_only=False):
        self.name, self.rows1, self.rows2, self.F, self.epipole = name, rows1, rows2, np.array(F, F32), epipole
        self.only_stereo, self.ori, self.guard_only = bool(only_stereo), bool(ori), bool(guard_only)
        self.expect = np.array(expect, np.int32)
        assert len(self.expect) == len(rows1)

    def __repr__(self):
        return self.name

    def side(self, which):
        """The arrays of one key frame: x, y, octave, u_right, node, has_mp, desc, angle."""
        a = list(zip(*(self.rows1 if which == 1 else self.rows2)))
        return {"kp_x": np.array(a[0], F32), "kp_y": np.array(a[1], F32), "kp_octave": np.array(a[2], np.int32),
                "u_right": np.array(a[3], F32), "node": np.array(a[4], np.int32), "has_mp": np.array(a[5], np.uint8),
                "desc": desc_rows(a[6]), "kp_angle": np.array(a[7], F32)}


def _each_own_node(rows1, rows2):
    """Row i and candidate i under node 10 + i: the pairs do not meet."""
    return ([r[:4] + (10 + i,) + r[5:] for i, r in enumerate(rows1)], [r[:4] + (10 + i,) + r[5:] for i, r in enumerate(rows2)])


_EPI_ROWS2 = [k2(290.0), k2(290.01), k2(289.0, octave=1), k2(289.05, octave=1)]

TRI_CASES = [
    # ---- dsqr < 3.84 * sigma2 in double (:156): key point i of key frame 2 lies dy below the line y = 0 of row i
    TriCase("line_gate", *_each_own_node([k1(100), k1(110), k1(120), k1(130)],
                                         [k2(50, 1.959), k2(50, 1.96), k2(50, 2.351, 1), k2(50, 2.352, 1)]), [0, -1, 2, -1]),
    # 1.9595917f squared is the float 3.84f = 3.8399999142 itself: below 3.84 in double, not below 3.84f in float
    TriCase("line_gate_is_compared_in_double", *_each_own_node([k1(100), k1(110)], [k2(50, DY_384F), k2(50, up(DY_384F))]), [0, -1]),
    TriCase("line_gate_above", *_each_own_node([k1(100), k1(110)], [k2(50, -1.959), k2(50, -1.96)]), [0, -1]),
    # ---- den == 0 (:151-152): F12 = 0 makes every line (0, 0, 0)
    TriCase("den_zero", *_each_own_node([k1(100), k1(110)], [k2(50), k2(60)]), [-1, -1], F=np.zeros((3, 3), F32)),
    # ---- the epipole gate, for mono against mono only (:743-749): distex^2 + distey^2 < 100 * scale[octave] skips
    TriCase("epipole_gate", *_each_own_node([k1(10), k1(20), k1(30), k1(40)], _EPI_ROWS2), [0, -1, 2, -1], epipole=(EPI_X, 0.0)),
    # u_right 0.0 and -0.0 are stereo (`>= 0`, :705, :728): the gate is not asked
    TriCase("epipole_gate_row_is_stereo", *_each_own_node([k1(10, ur=0.0), k1(20, ur=-0.0), k1(30, ur=0.0), k1(40, ur=-0.0)],
                                                          _EPI_ROWS2), [0, 1, 2, 3], epipole=(EPI_X, 0.0)),
    TriCase("epipole_gate_candidate_is_stereo",
            *_each_own_node([k1(10), k1(20), k1(30), k1(40)],
                            [r[:3] + (u,) + r[4:] for r, u in zip(_EPI_ROWS2, (0.0, -0.0, -0.0, 0.0))]), [0, 1, 2, 3],
            epipole=(EPI_X, 0.0)),
    # ---- bOnlyStereo (:707-709, :730-732): a mono row, a mono candidate, and a stereo pair
    TriCase("only_stereo", *_each_own_node([k1(100), k1(110, ur=5.0), k1(120, ur=0.0)],
                                           [k2(50, ur=5.0), k2(60), k2(70, ur=-0.0)]), [-1, -1, 2], only_stereo=True),
    TriCase("not_only_stereo", *_each_own_node([k1(100), k1(110, ur=5.0), k1(120, ur=0.0)],
                                               [k2(50, ur=5.0), k2(60), k2(70, ur=-0.0)]), [0, 1, 2]),
    # ---- dist > TH_LOW (:738): 50 stays, 51 goes
    TriCase("th_low", *_each_own_node([k1(100), k1(110)], [k2(50, bits=50), k2(60, bits=51)]), [0, -1]),
    # ---- `dist > bestDist` is the skip (:738), so of equal distances the LAST of the node's list wins: bits 0..19, 10..29 and
    # 20..39 are all 20 from the zero row
    TriCase("tie_takes_the_last", [k1(100)], [k2(50, bits=20), k2(60, bits=(10, 30)), k2(70, bits=(20, 40))], [2]),
    # ---- bestDist is lowered by a candidate that PASSES the line test only (:751-755): y = 5 fails it (25 > 3.84).
    # row 0: 10 failing, then 30: the 30;  row 1: 30, then 10 failing: the 30;  row 2: 10, then 30: the 10;  row 3: 30, then 10
    TriCase("failing_candidate_does_not_lower_the_bar",
            [k1(100, node=10), k1(110, node=11), k1(120, node=12), k1(130, node=13)],
            [k2(50, 5.0, node=10, bits=10), k2(51, node=10, bits=30), k2(52, node=11, bits=30), k2(53, 5.0, node=11, bits=10),
             k2(54, node=12, bits=10), k2(55, node=12, bits=30), k2(56, node=13, bits=30), k2(57, node=13, bits=10)],
            [1, 2, 4, 7]),
    # ---- skips: row 0 has a map point (:699-703); candidate 1 has one (:722-726); row 2 and candidate 2 are in no node (-1
    # is not a node they share); candidate 3 is under another node; row 4 is the control
    TriCase("skips", [k1(100, node=10, has=1), k1(110, node=11), k1(120, node=-1), k1(130, node=13), k1(140, node=15)],
            [k2(50, node=10), k2(60, node=11, has=1), k2(70, node=-1), k2(80, node=14), k2(90, node=15)], [-1, -1, -1, -1, 4]),
    # ---- vbMatched2 is never set (:677 declares it, :725 reads it): two rows take the same key point
    TriCase("no_matched2", [k1(100), k1(110)], [k2(50)], [0, 0]),
    # ---- a candidate's coordinate that is no number fails the line test (and the epipole gate does not skip it: NaN < x)
    TriCase("nan_candidate", *_each_own_node([k1(100), k1(110), k1(120)], [k2(NAN), k2(50, NAN), k2(60)]), [-1, -1, 2]),
    # ---- the rotation check (:772-795) on three pairs in bin 0 and one in bin 3 (all stay: 1 < 0.1f * 3 fails), and the two
    # pairs without a bin of BF_CASES' rotation case
    TriCase("rotation_three_and_one", *_each_own_node([k1(100), k1(110), k1(120), k1(130, angle=90)],
                                                      [k2(50), k2(60), k2(70), k2(80)]), [0, 1, 2, 3], ori=True),
    TriCase("rotation_pairs_without_a_bin",
            *_each_own_node([k1(100), k1(110), k1(120), k1(130, angle=90), k1(140, angle=1000), k1(150, angle=NAN)],
                            [k2(50), k2(60), k2(70), k2(80), k2(90), k2(95)]), [0, 1, 2, 3, -1, -1], ori=True),
    TriCase("rotation_pairs_without_a_bin_2nd_frame",
            *_each_own_node([k1(100), k1(110), k1(120), k1(130, angle=90), k1(140), k1(150)],
                            [k2(50), k2(60), k2(70), k2(80), k2(90, angle=1000), k2(95, angle=-INF)]), [0, 1, 2, 3, -1, -1],
            ori=True),
    TriCase("rotation_fourth_bin",
            *_each_own_node([k1(100 + 5 * i, angle=a) for i, a in enumerate((0, 0, 0, 30, 30, 60, 60, 90))],
                            [k2(50 + 5 * i) for i in range(8)]), [0, 1, 2, 3, 4, 5, 6, -1], ori=True),
    # ---- the flavour over device arrays cannot refuse an octave outside [0, ORBGPU_MAX_LEVELS) on the host as the others
    # do, and skips such a candidate before anything is indexed with it; octave 8 of 8 levels has sigma2 = 0 and fails the
    # line test.  Each candidate is a copy of its row and would win otherwise; octave 7 is the control.  The reference and
    # the oracle have no such guard: this case is for that flavour alone.
    TriCase("octave_guard", *_each_own_node([k1(100), k1(110), k1(120), k1(130)],
                                            [k2(50, octave=-1), k2(60, octave=8), k2(70, octave=16), k2(80, octave=7)]),
            [-1, -1, -1, 3], guard_only=True),
]


class TriView:
    """A key frame as a FrameView of `side` (the oracle's module or the library): only the members that
    SearchForTriangulation reads, so that coordinates that are no numbers never meet a grid."""

    def __init__(self, side, f):
        self.side, self.f, self.n = side, f, len(f["kp_x"])

    def view(self):
        v = self.side.FrameView()
        v.n = self.n
        self.keep = [np.ascontiguousarray(self.f[k]) for k in ("kp_x", "kp_y", "kp_octave", "kp_angle", "u_right", "desc")] + \
                    [np.ascontiguousarray(SF)]
        v.kp_x, v.kp_y, v.kp_octave, v.kp_angle, v.u_right, v.desc, v.scale_factors = (a.ctypes.data for a in self.keep)
        v.nlevels = NLEVELS
        return v


def tri_flavours(case):
    if case.guard_only:
        return ("create_new_map_points_device",)
    return ("search_for_triangulation", "create_new_map_points", "create_new_map_points_device")


FX, FY, CX, CY, MB = 512.0, 512.0, 320.0, 240.0, 40.0 / 512.0  # the camera of proj_gate_cases.py


def new_points_scene(case):
    """The case as a CreateNewMapPoints problem with one neighbour (tests/newpts_model.py's layout): both key frames at
    the identity pose, a stereo key point at depth 2.  Only the match step (match12[0], n_matches[0]) is read: what the
    later stages make of pairs without parallax is not this file's business."""
    eye = np.eye(4, dtype=F32).reshape(16)

    def frame(which):
        f = case.side(which)
        stereo = f["u_right"] >= 0
        depth = np.where(stereo, F32(2), F32(-1)).astype(F32)
        with np.errstate(all="ignore"):
            cs = np.cos(F32(2) * np.arctan2(F32(MB) / F32(2), depth)).astype(F32)
        f.update({"depth": depth, "cos_stereo": cs, "kp_raw": None, "Tcw": eye, "Twc": eye, "K": (FX, FY, CX, CY),
                  "mbf": FX * MB, "level_sigma2": SIGMA2, "scale_factors": SF})
        return f
    nb = frame(2)
    nb.update({"F12": case.F.reshape(9), "ex": F32(case.epipole[0]), "ey": F32(case.epipole[1])})
    return {"kf1": frame(1), "neighbours": [nb], "ratio_factor": F32(1.5) * F32(1.2), "only_stereo": case.only_stereo,
            "check_ori": case.ori}
