"""GPU parity of k_bf_topk's candidate selection (the order walk of bf_select.h, the bar compared on the tagged value)
against the oracle on crafted descriptor sets, through the batched entry points.  The two `other_half` scenes were
written for one bar per A row (bf_select.h: built, measured, left out) and hold whether the halves share a bar or not.

With one B row range (nsplit == 1) the lane (A row & 31, half h) of a wave holds, per row block of 32 B rows starting
at j0 (a multiple of 32), the 16 rows j0 + 4 h + (reg & 3) + 8 (reg >> 2); the scenes put their near rows there so that
they meet in one lane.  Everything else is random rows (distance 128 +- 8 from anything, far beyond any bar here).  Each
scene states what the oracle must decide on it, and the test reads that off the oracle's result first.

Shapes: cap 96 and 200 (the row stride: the scenes of 130 B rows run at 200 only); na 33, 70, 96; nb 63, 64, 65, 130; the
scenes as one batch of nine pairs (nsplit 1), in batches of three (nsplit 4) and alone (nsplit 16): with more than one
range the near rows fall into other lanes, and the result must not change.  The last test asserts that both kinds of launch were seen; it needs the module to have run."""
from types import SimpleNamespace

import numpy as np
import pytest

import bf_batch_scenes as S

pytestmark = pytest.mark.gpu

SEEN = []  # last_launch() of every call of this module


def lane_rows(j0, h, regs):
    return [j0 + 4 * h + (reg & 3) + 8 * (reg >> 2) for reg in regs]


def at_distance(rng, row, d):
    """A copy of `row` with d bits flipped."""
    bits = np.unpackbits(row)
    bits[rng.permutation(256)[:d]] ^= 1
    return np.packbits(bits)


def scene(seed, na, nb, ratio, th, ori=False):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (na, 32), dtype=np.uint8)
    b = rng.integers(0, 256, (nb, 32), dtype=np.uint8)
    aa, ab = (rng.random(na) * 360).astype(np.float32), (rng.random(nb) * 360).astype(np.float32)
    pr = SimpleNamespace(a=a, b=b, aa=aa, ab=ab, valid=None, node_a=None, node_b=None, ratio=float(ratio), th=int(th),
                         ori=bool(ori), seed=seed, must={}, rng=rng)
    return pr


def place(pr, i, rows, dists):
    """B rows `rows` at the distances `dists` from A row i."""
    for j, d in zip(rows, dists):
        pr.b[j] = at_distance(pr.rng, pr.a[i], d)


def six_in_a_lane():
    """Six B rows of one lane within dmax of A row 32 (the second wave), two pairs of equal distances; A rows 0..2 are
    copies of the three nearest and claim them, so row 32 is decided by its 4th and 5th candidate: 20 at the HIGHER of
    two equal rows against 25."""
    pr = scene(1, 33, 63, 0.9, 50)
    rows = lane_rows(0, 1, [2, 5, 7, 8, 13, 14])  # 6, 13, 15, 20, 29, 30
    place(pr, 32, rows, [20, 12, 20, 7, 25, 25])
    pr.a[0], pr.a[1], pr.a[2] = pr.b[rows[3]], pr.b[rows[1]], pr.b[rows[0]]
    pr.must = {rows[3]: 0, rows[1]: 1, rows[0]: 2, rows[2]: 32}
    return pr


def sixteen_identical():
    """All 16 rows of a lane equal A row 37: 16 trips; best and second are both 0, so nothing matches the row."""
    pr = scene(2, 70, 64, 0.7, 50, ori=True)
    rows = lane_rows(32, 0, range(16))
    place(pr, 37, rows, [0] * 16)
    pr.must = {j: -1 for j in rows}
    return pr


def other_half(inside):
    """The h = 0 lane of A row 5 fills its list in the first tile (5, 6, 7, 8: bar 8); the h = 1 lane meets its only
    candidates in the second tile.  A rows 0 and 1 claim the rows at 5 and 6.  Beyond the bar (20, 30) the candidates
    must not count: row 5 takes the row at 7 against 8.  Inside it (6, 7) they must: row 5 takes the new row at 6
    against 7."""
    pr = scene(3 + inside, 33 if inside else 96, 130, 0.9, 50)
    h0 = lane_rows(0, 0, [1, 6, 11, 12])
    h1 = lane_rows(64 + 32, 1, [3, 9])
    place(pr, 5, h0, [5, 6, 7, 8])
    place(pr, 5, h1, [6, 7] if inside else [20, 30])
    pr.a[0], pr.a[1] = pr.b[h0[0]], pr.b[h0[1]]
    pr.must = {h0[0]: 0, h0[1]: 1}
    pr.must.update({h1[0]: 5, h0[2]: -1} if inside else {h0[2]: 5, h1[0]: -1, h1[1]: -1})
    return pr


def at_the_bar():
    """th_low 50, nnratio 0.7: a second best at 71 still fails the ratio test for a best of 50 (49.7 < 50), one at 72
    cannot (50.4): 71 is the last distance listed.  Row 3 (50, 71) stays unmatched, row 40 (50, 72) matches."""
    pr = scene(5, 70, 65, 0.7, 50)
    r3, r40 = lane_rows(0, 0, [4, 10]), lane_rows(32, 1, [0, 15])
    place(pr, 3, r3, [50, 71])
    place(pr, 40, r40, [50, 72])
    pr.must = {r3[0]: -1, r3[1]: -1, r40[0]: 40, r40[1]: -1}
    return pr


def repeated_last_row(seed, na, nb):
    """The last B row is the nearest of A row 9 (3 against 10).  The staging repeats it to the end of the last tile: every
    lane of the wave meets copies past the last row, which are skipped one by one and must not be listed."""
    pr = scene(seed, na, nb, 0.7, 50)
    place(pr, 9, [nb - 1, 17], [3, 10])
    pr.must = {nb - 1: 9, 17: -1}
    return pr


def chain():
    """A rows 10..15 are one descriptor, six B rows of one lane lie at 2, 4, .. 12 from it: row 10 + k takes the k-th,
    the 2nd, 3rd and 4th from the list entry of that rank, the last two after the list is used up."""
    pr = scene(9, 96, 64, 0.9, 50)
    rows = lane_rows(32, 1, [0, 3, 6, 9, 12, 15])
    for i in range(11, 16):
        pr.a[i] = pr.a[10]
    place(pr, 10, rows, [2, 4, 6, 8, 10, 12])
    pr.must = {j: 10 + k for k, j in enumerate(rows)}
    return pr


def chain_with_nodes():
    """The chain under the node-wise entry: every second near row sits under another node and is passed over (it must
    still advance the lane), so rows 10, 11, 12 take the rows at 2, 6, 10 and the others nothing."""
    pr = chain()
    rng = np.random.default_rng(10)
    pr.node_a = np.asarray([7, 8, -1], np.int32)[rng.integers(0, 3, len(pr.a))]
    pr.node_b = np.asarray([7, 8, -1], np.int32)[rng.integers(0, 3, len(pr.b))]
    rows = sorted(pr.must)
    pr.node_a[10:16] = 7
    pr.node_b[rows] = [7, 8, 7, 8, 7, 8]
    pr.must = {rows[0]: 10, rows[2]: 11, rows[4]: 12}
    return pr


def randomly_labelled(pr, ids):
    """A scene under random node labels (a tenth of the rows outside the feature vector): what the oracle decides is no
    longer what the scene states."""
    pr.must = {}
    return S.with_nodes(pr, ids=ids)


_scenes = {}


def scenes(name):
    if name not in _scenes:
        _scenes[name] = {
            "bf": lambda: [six_in_a_lane(), sixteen_identical(), other_half(0), other_half(1), at_the_bar(),
                           repeated_last_row(6, 96, 65), repeated_last_row(7, 33, 63), repeated_last_row(8, 70, 130), chain()],
            "nodes": lambda: [chain_with_nodes(), randomly_labelled(six_in_a_lane(), (7, 7, 8)), randomly_labelled(chain(), (7,))],
        }[name]()
    return _scenes[name]


def run_and_check(gpu, oracle, prs, cap):
    pytest.importorskip("torch")
    bm = gpu.BatchMatcher(len(prs), cap)
    try:
        out, launches = S.run(bm, prs, cap)
    finally:
        bm.close()
    SEEN.extend(launches)
    for p, (pr, (n, mb, behind, sweeps)) in enumerate(zip(prs, out)):
        want_n, want = S.expected(oracle, pr)
        for j, i in pr.must.items():
            assert want[j] == i, "scene %d is not what it is meant to be: B row %d -> %d, not %d" % (p, j, want[j], i)
        print("pair %d (%d x %d): %d matches, oracle %d, %d sweeps" % (p, len(pr.a), len(pr.b), n, want_n, sweeps))
        assert n == want_n and np.array_equal(mb, want), (p, n, want_n, np.nonzero(mb != want)[0][:8])
        assert np.all(behind == -1), p
    return launches


@pytest.mark.parametrize("cap", [96, 200])
@pytest.mark.parametrize("pairs", [9, 3, 1])
def test_crafted_scenes(gpu, oracle, cap, pairs):
    prs = scenes("bf")
    assert {len(q.a) for q in prs} == {33, 70, 96} and {len(q.b) for q in prs} == {63, 64, 65, 130}
    prs = [q for q in prs if len(q.b) <= cap]  # cap is the row stride: the three scenes of 130 B rows need cap 200
    assert len(prs) == (6 if cap == 96 else 9)
    if pairs == 9:
        prs = (prs * 2)[:9]  # nine pairs in the call is what gives one range
    for first in range(0, len(prs), pairs):
        launches = run_and_check(gpu, oracle, prs[first:first + pairs], cap)
        assert all(l["nsplit"] == 1 for l in launches) == (pairs == 9), launches


@pytest.mark.parametrize("cap", [96, 200])
@pytest.mark.parametrize("pairs", [3, 1])
def test_crafted_scenes_node_wise(gpu, oracle, cap, pairs):
    """k_bf_topk<true>: a near row under another node is passed over and still advances the lane."""
    prs = scenes("nodes")
    for first in range(0, len(prs), pairs):
        run_and_check(gpu, oracle, prs[first:first + pairs], cap)


def test_node_wise_single_range(gpu, oracle):
    """Nine pairs in a call: one B row range, so the near rows of the node-wise chain do meet in one lane."""
    prs = scenes("nodes") * 3
    launches = run_and_check(gpu, oracle, prs, 96)
    assert all(l["nsplit"] == 1 for l in launches)


def test_zz_both_kinds_of_launch_were_seen():
    splits = {l["nsplit"] for l in SEEN}
    print("splits", sorted(splits))
    assert 1 in splits and any(s > 1 for s in splits), sorted(splits)
