"""The scenes of test_gpu_matcher_batch.py bite: read off the oracle alone (no device), the committed seeds send enough
rows through the exact full scan of k_bf_resolve, and the pruned-list settings still accept something.  The decisions
are counted before the rotation check (it removes matches afterwards, it does not undo how they were decided)."""
import numpy as np

import bf_batch_scenes as S

BF_SETS = ["split", "ragged", "unstaged", "threads"]


def test_feature_vector_layout():
    fv = S.feature_vector(np.array([7, -1, 3, 7, 3, -1, 40], np.int32))
    assert fv["fv_nodes"].tolist() == [3, 7, 40] and fv["fv_start"].tolist() == [0, 2, 4, 5]
    assert fv["fv_items"].tolist() == [2, 4, 0, 3, 6]
    empty = S.feature_vector(np.zeros(0, np.int32))
    assert len(empty["fv_nodes"]) == 0 and empty["fv_start"].tolist() == [0]


def test_outside_four_nearest_counts_by_key():
    """Row 0 is nearest to B rows 0..4 in that order (distances 0, 1, 1, 2, 2): B row 3 is its fourth key, row 4 is not."""
    b = np.zeros((6, 32), np.uint8)
    b[1, 0], b[2, 0], b[3, 0], b[4, 0], b[5] = 1, 2, 3, 5, 255
    pr = S.SimpleNamespace(a=np.zeros((1, 32), np.uint8), b=b, node_a=None, node_b=None)
    for j, want in ((3, 0), (4, 1)):
        mb = np.full(6, -1, np.int32)
        mb[j] = 0
        assert S.outside_four_nearest(pr, mb) == want
    pr.node_a, pr.node_b = np.array([9], np.int32), np.array([9, 1, 1, 9, 9, 9], np.int32)  # rows 1, 2 leave the node
    assert S.outside_four_nearest(pr, mb) == 0


def test_conflict_scenes_reach_the_full_scan(oracle):
    seen = {s: 0 for s in S.SETTINGS}
    for name in BF_SETS:
        for p, pr in enumerate(S.problems(name)):
            n, claimed = S.expected(oracle, pr)[0], S.expected(oracle, pr, claims=True)
            out = S.outside_four_nearest(pr, claimed[1])
            print("%s[%d] %dx%d ratio %.1f th %d: %d matches (%d before the rotation check), %d outside the four "
                  "nearest" % (name, p, len(pr.a), len(pr.b), pr.ratio, pr.th, n, claimed[0], out))
            seen[(pr.ratio, pr.th)] += 1
            if name == "ragged":
                continue  # counts of 0, 1, 5 rows cannot conflict; the set is about the edges
            if pr.ratio >= 2:
                assert out >= 20, (name, p, out)
            else:
                assert claimed[0] >= 1, (name, p)  # accepted by the ratio test
    assert min(seen.values()) >= 4
    ragged = S.problems("ragged")
    assert sum(S.outside_four_nearest(pr, S.expected(oracle, pr, claims=True)[1]) for pr in ragged) >= 20
    assert [S.expected(oracle, pr)[0] for pr in ragged[:2]] == [0, 0]


def test_node_scenes_reach_the_full_scan(oracle):
    for name in ("nodes", "nodes_empty"):
        for p, pr in enumerate(S.problems(name)):
            (n, mb), claimed = S.expected(oracle, pr), S.expected(oracle, pr, claims=True)
            out = S.outside_four_nearest(pr, claimed[1])
            print("%s[%d] %dx%d ratio %.2f th %d: %d matches, %d outside the four nearest of their node" %
                  (name, p, len(pr.a), len(pr.b), pr.ratio, pr.th, n, out))
            live = np.nonzero(mb >= 0)[0]
            assert np.all(pr.node_a[mb[live]] == pr.node_b[live]) and np.all(pr.node_b[live] >= 0)
            if len(pr.a) and len(pr.b):
                assert (pr.node_a < 0).sum() >= 10 and (pr.node_b < 0).sum() >= 10
                if pr.ratio >= 2:
                    assert out >= 10, (name, p, out)
                else:
                    assert n >= 1, (name, p)
            else:
                assert n == 0
