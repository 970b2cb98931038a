"""GPU parity of the batched brute-force and node-wise matchers (orbgpu_match_bf_batch_device,
orbgpu_search_by_bow_batch_device) against the oracle on every launch shape match_batch_device() picks: the number of
B row ranges with a candidate list of their own (nsplit 1 .. 16), the full scan from LDS or from global memory
(stage_b), and a resolve workgroup with fewer threads than rows (ORBGPU_DEBUG_BF_RESOLVE_THREADS).  The data are the
conflict scenes of bf_batch_scenes.py (test_bf_batch_scenes.py shows on the CPU that they reach the full scan), packed
with random bytes behind every row count.  Integer code against an integer oracle: every comparison is exact.

The last test asserts on the launch shapes the others SAW (orbgpu_matcher_last_launch), not on the heuristic: if the
heuristic changes, it names the shape that needs a new parameter.  It needs the rest of the module to have run."""
import ctypes as C

import numpy as np
import pytest

import bf_batch_scenes as S

pytestmark = pytest.mark.gpu

CAP = 320  # no multiple of the 64-row B tile or of the 256 A rows of a workgroup: two A row blocks
SEEN = []  # last_launch() of every call of this module
_default_threads = {}


def run(gpu, max_pairs, prs, cap):
    pytest.importorskip("torch")
    bm = gpu.BatchMatcher(max_pairs, cap)
    try:
        out, launches = S.run(bm, prs, cap)
    finally:
        bm.close()
    SEEN.extend(launches)
    return out, launches


def check(oracle, prs, out, sweeps_above_2=True):
    for p, (pr, (n, mb, behind, sweeps)) in enumerate(zip(prs, out)):
        want_n, want = S.expected(oracle, pr)
        print("pair %d (%d x %d, ratio %.2f, th %d): %d matches, oracle %d, %d sweeps" %
              (p, len(pr.a), len(pr.b), pr.ratio, pr.th, n, want_n, sweeps))
        assert n == want_n, (p, n, want_n)
        assert np.array_equal(mb, want), (p, int((mb != want).sum()))
        assert np.all(behind == -1), p
        assert sweeps >= 1
        if sweeps_above_2 and pr.ratio == 10.0:
            assert sweeps > 2, (p, sweeps)  # claims moved twice at least: the scene did conflict on the device


@pytest.mark.parametrize("pairs,max_pairs", [(1, 1), (2, 2), (3, 3), (5, 5), (9, 9), (2, 64), (9, 64)])
def test_every_split(gpu, oracle, pairs, max_pairs):
    """The same conflict scenes under every number of B row ranges (16, 8, 4, 2, 1, 16, 4 with the heuristic this test
    was written against): k_bf_resolve must merge the partial lists into the same four candidates."""
    prs = S.problems("split")[:pairs]
    out, launches = run(gpu, max_pairs, prs, CAP)
    print("nsplit", sorted({l["nsplit"] for l in launches}))
    assert len({l["nsplit"] for l in launches}) == 1 and all(l["stage_b"] == 1 for l in launches)
    check(oracle, prs, out)


def test_batch_equals_host_entry(gpu, oracle):
    """One list per row (nine pairs, stride 320) and sixteen (the host entry: one pair, stride 1024): same bytes."""
    prs = S.problems("split")
    out, launches = run(gpu, 9, prs, CAP)
    for p, (pr, (n, mb, _, _)) in enumerate(zip(prs, out)):
        hn, hmb = gpu.ORBmatcher(pr.ratio, pr.ori).MatchBruteForce(pr.a, pr.aa, pr.b, pr.ab, valid_a=pr.valid, th_low=pr.th)
        assert hn == n and hmb.tobytes() == mb.tobytes(), p
    check(oracle, prs, out)


@pytest.mark.parametrize("max_pairs", [9, 64])
def test_ragged_counts(gpu, oracle, max_pairs):
    """Empty sides, single rows and counts at the edges of the 64-row B tile and the 256-row A block in one batch; with
    max_pairs = 64 the 5 (or 1) B rows of a pair are spread over more ranges than there are rows."""
    prs = S.problems("ragged")
    out, launches = run(gpu, max_pairs, prs, CAP)
    print("nsplit", sorted({l["nsplit"] for l in launches}))
    check(oracle, prs, out, sweeps_above_2=False)
    for p in (0, 1):
        assert out[p][0] == 0 and np.all(out[p][1] == -1)


def test_unstaged_full_scan(gpu, oracle):
    """A row stride above 3200 leaves no room for the B descriptors in LDS: the full scan reads global memory.  The
    300 live rows are the same in both strides, and so must the result be."""
    prs = S.problems("unstaged")
    far, launches = run(gpu, 2, prs, 3264)
    assert all(l["stage_b"] == 0 for l in launches)
    near, launches = run(gpu, 2, prs, CAP)
    assert all(l["stage_b"] == 1 for l in launches)
    check(oracle, prs, far)
    check(oracle, prs, near)
    for a, b in zip(far, near):
        assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("threads", [256, 512])
def test_fewer_resolve_threads_than_rows(gpu, oracle, monkeypatch, threads):
    """700 rows on 256 or 512 threads: a thread decides rows i != tid too, whose lists it reloads every sweep."""
    prs = S.problems("threads")
    if not _default_threads:
        out, launches = run(gpu, 3, prs, 704)
        assert all(l["resolve_threads"] == 1024 for l in launches)
        _default_threads["out"] = out
    monkeypatch.setenv("ORBGPU_DEBUG_BF_RESOLVE_THREADS", str(threads))
    out, launches = run(gpu, 3, prs, 704)
    assert all(l["resolve_threads"] == threads for l in launches)
    check(oracle, prs, out)
    check(oracle, prs, _default_threads["out"])
    for a, b in zip(out, _default_threads["out"]):
        assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("setting", [0, 1], ids=["ratio0.95_th50", "ratio10_th256"])
def test_node_wise_batch(gpu, oracle, setting):
    """k_bf_topk<true> on three pairs: node arrays at [pair][cap] offsets, six crowded nodes, a tenth of the rows
    outside the feature vector on both sides, a validity mask.  Against the oracle's SearchByBoW on the feature vector
    built from the labels, and against the host entry pair by pair."""
    prs = S.problems("nodes")[setting::2]
    assert len(prs) == 3
    out, launches = run(gpu, 3, prs, CAP)
    check(oracle, prs, out, sweeps_above_2=False)
    for p, (pr, (n, mb, _, _)) in enumerate(zip(prs, out)):
        hn, hmb = gpu.search_by_bow(pr.a, pr.aa, pr.valid, pr.node_a, pr.b, pr.ab, pr.node_b, pr.th, pr.ratio, pr.ori)
        assert hn == n and hmb.tobytes() == mb.tobytes(), p


def test_node_wise_batch_with_empty_pairs(gpu, oracle):
    prs = S.problems("nodes_empty")
    out, _ = run(gpu, 3, prs, CAP)
    check(oracle, prs, out, sweeps_above_2=False)
    for p in (0, 2):
        assert out[p][0] == 0 and np.all(out[p][1] == -1)


def test_argument_checks(gpu):
    """EINVAL, no launch, no crash."""
    torch = pytest.importorskip("torch")
    L = gpu.lib()
    bm = gpu.BatchMatcher(2, CAP)
    v = [C.c_int32() for _ in range(3)]
    refs = [C.byref(x) for x in v]
    assert L.orbgpu_matcher_last_launch(bm.h, *refs) == gpu.EINVAL  # nothing recorded yet
    assert L.orbgpu_matcher_last_launch(bm.h, None, refs[1], refs[2]) == gpu.EINVAL
    with pytest.raises(gpu.OrbGpuError):
        bm.last_launch()
    d = S.pack(S.problems("nodes_empty")[:2], CAP)
    bf = lambda pairs, cap: L.orbgpu_match_bf_batch_device(
        bm.h, pairs, cap, d.desc_a.data_ptr(), d.ang_a.data_ptr(), None, d.na.data_ptr(), d.desc_b.data_ptr(),
        d.ang_b.data_ptr(), d.nb.data_ptr(), 4, 50, 0.7, 1, d.match_b.data_ptr(), d.nm.data_ptr(), None)
    bow = lambda pairs, cap, node_a, node_b: L.orbgpu_search_by_bow_batch_device(
        bm.h, pairs, cap, d.desc_a.data_ptr(), d.ang_a.data_ptr(), None, node_a, d.na.data_ptr(), d.desc_b.data_ptr(),
        d.ang_b.data_ptr(), node_b, d.nb.data_ptr(), 4, 50, 0.7, 1, d.match_b.data_ptr(), d.nm.data_ptr(), None)
    na, nb = d.node_a.data_ptr(), d.node_b.data_ptr()
    assert bow(2, CAP, None, nb) == gpu.EINVAL and bow(2, CAP, na, None) == gpu.EINVAL
    assert b"node" in L.orbgpu_last_error_string()
    assert bf(3, CAP) == gpu.EINVAL and bow(3, CAP, na, nb) == gpu.EINVAL          # pairs > max_pairs
    assert bf(2, CAP + 1) == gpu.EINVAL and bow(2, CAP + 1, na, nb) == gpu.EINVAL  # cap above the matcher's
    assert bf(0, CAP) == gpu.EINVAL
    assert L.orbgpu_matcher_last_launch(bm.h, *refs) == gpu.EINVAL  # still nothing launched
    torch.cuda.synchronize()
    bm.close()


def test_zz_every_launch_shape_was_seen():
    splits = {l["nsplit"] for l in SEEN}
    print("splits", sorted(splits), "stage_b", sorted({l["stage_b"] for l in SEEN}), "resolve threads",
          sorted({l["resolve_threads"] for l in SEEN}))
    assert splits >= {1, 2, 4, 8, 16}, "no parameter of this module reaches nsplit %s any more" % sorted({1, 2, 4, 8, 16} - splits)
    assert {l["stage_b"] for l in SEEN} == {0, 1}
    assert {l["resolve_threads"] for l in SEEN} >= {256, 512, 1024}
