"""tests/kfdb_model.py, the restatement of KeyFrameDatabase.cc:33-309 and L1Scoring::score that the device database is
compared with: K1's two formulations agree, K2 on a hand-computed example, K3 at the truncation's edges, K5's stale
score.  No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import kfdb_model as M  # noqa: E402


def test_k1_inverted_file_walk_equals_the_sort_by_first_word_and_sequence():
    """lKFsSharingWords from the literal per-word lists == rows sorted by (first common word, add sequence number), over
    random add / erase / re-add / query sequences"""
    checked = 0
    for seed in range(240):
        rng = np.random.default_rng(seed)
        n_words = int(rng.choice([6, 12, 40]))
        db = M.KeyFrameDatabase(n_words)
        ids_in = []
        for step in range(int(rng.integers(5, 40))):
            op = rng.random()
            if op < 0.55 or not ids_in:
                kf_id = int(rng.integers(0, 30))
                v = M.random_vector(rng, n_words, int(rng.integers(1, min(n_words, 8) + 1)))
                if kf_id in ids_in:
                    with pytest.raises(M.Refused):
                        db.add(kf_id, *v)
                else:
                    db.add(kf_id, *v)
                    ids_in.append(kf_id)
            elif op < 0.75:
                victim = int(rng.choice(ids_in))  # may come back later with a new sequence number
                assert db.erase([victim, 1000]) == 1
                ids_in.remove(victim)
            else:
                q = M.random_vector(rng, n_words, int(rng.integers(1, min(n_words, 8) + 1)))
                conn = [int(c) for c in rng.choice(30, size=int(rng.integers(0, 4)), replace=False)]
                if rng.random() < 0.5:
                    db.detect_loop(q[0], q[1], conn, 0.0)
                else:
                    conn = []
                    db.detect_reloc(*q)
                lq = db.last_query()
                want = db.sharing_by_sort(q[0], conn)
                assert [(int(a), int(b), int(c)) for a, b, c in zip(lq["id"], lq["words"], lq["first_word"])] == want
                checked += 1
    assert checked >= 200


def test_k2_score_by_hand_and_its_properties():
    # common words 3 and 7:  (|0.5-0.25| - 0.5 - 0.25) + (|0.125-0.5| - 0.125 - 0.5) = -0.5 + -0.25 = -0.75 -> 0.375
    a = (np.array([1, 3, 7]), np.array([0.375, 0.5, 0.125]))
    b = (np.array([3, 5, 7, 9]), np.array([0.25, 0.125, 0.5, 0.125]))
    assert M.l1_score(a[0], a[1], b[0], b[1]) == 0.375 == M.l1_score(b[0], b[1], a[0], a[1])
    v = (np.array([0, 2, 4, 8]), np.array([0.5, 0.25, 0.125, 0.125]))  # L1-normalised, exact in binary
    assert M.l1_score(v[0], v[1], v[0], v[1]) == 1.0
    rng = np.random.default_rng(1)
    ids, vals = M.random_vector(rng, 1000, 200)
    assert np.float32(M.l1_score(ids, vals, ids, vals)) == np.float32(1.0)
    assert M.l1_score(np.array([1, 3]), np.array([0.5, 0.5]), np.array([0, 2, 4]), np.array([0.25, 0.25, 0.5])) == 0.0
    assert M.l1_score(np.array([], int), np.array([]), ids, vals) == 0.0
    # the sum is sequential in ascending word id: the same terms in another order give other bits
    ids2, vals2 = M.vector_from(rng, ids, vals, 150, 1000, 30)
    common = np.intersect1d(ids, ids2)
    s = 0.0
    for w in common:
        vi, wi = vals[np.searchsorted(ids, w)], vals2[np.searchsorted(ids2, w)]
        s += abs(vi - wi) - abs(vi) - abs(wi)
    assert M.l1_score(ids, vals, ids2, vals2) == -s / 2.0


@pytest.mark.parametrize("max_common,want", [(1, 0), (4, 3), (5, 4), (10, 8), (11, 8)])
def test_k3_threshold_is_a_float_product_truncated(max_common, want):
    assert M.min_common_words(max_common) == want
    # and the query uses it with a strict '>': a row sharing `want` words is not scored, one sharing want + 1 is
    n_words = 64
    q = (np.arange(max_common, dtype=np.int32), np.full(max_common, 1.0 / max_common))
    db = M.KeyFrameDatabase(n_words)
    db.add(0, q[0], q[1])  # shares max_common words
    if want >= 1:
        db.add(1, np.arange(want, dtype=np.int32), np.full(want, 1.0 / want))
    if want + 1 < max_common:
        db.add(2, np.arange(want + 1, dtype=np.int32), np.full(want + 1, 1.0 / (want + 1)))
    db.detect_reloc(*q)
    lq = db.last_query()
    scored = {int(i): not np.isnan(s) for i, s in zip(lq["id"], lq["score"])}
    assert scored[0]
    if want >= 1:
        assert not scored[1]
    if want + 1 < max_common:
        assert scored[2]


def stale_scene():
    """K5: row 1 names row 0 as a neighbour; query A scores both, query B shares one word with row 0 (below the threshold)
    and ten with row 1"""
    words_r = np.arange(0, 10, dtype=np.int32)
    words_s = np.arange(20, 30, dtype=np.int32)
    r = (words_r, np.full(10, 0.1))
    s = (words_s, np.full(10, 0.1))
    qa = (np.concatenate([words_r, words_s]).astype(np.int32), np.full(20, 0.05))
    qb = (np.concatenate([words_r[:1], words_s]).astype(np.int32), np.full(11, 1.0 / 11))
    return r, s, qa, qb


def test_k5_a_neighbour_that_is_not_scored_adds_the_score_of_an_earlier_query():
    r, s, qa, qb = stale_scene()
    db = M.KeyFrameDatabase(64)
    db.add(0, *r)
    db.add(1, *s)
    db.add(2, np.array([29, 40], np.int32), np.array([0.5, 0.5]))  # shares one word with B: in the list, never scored
    db.set_covisibles(1, [0, 2, 77])
    first = M.KeyFrameDatabase(64)  # the same without query A
    first.add(0, *r)
    first.add(1, *s)
    first.add(2, np.array([29, 40], np.int32), np.array([0.5, 0.5]))
    first.set_covisibles(1, [0, 2, 77])
    # A: rows 0 and 1 score 0.5 each; row 1 sums 0.5 + 0.5 (row 0) + 0 (row 2) = 1.0 and keeps itself as best (K6: strict >);
    # row 0's 0.5 is not above 0.75 * 1.0
    assert db.detect_reloc(*qa) == [1]
    score_r_from_a = db.kfs[0].reloc_score
    assert score_r_from_a > 0
    db.detect_reloc(*qb)
    first.detect_reloc(*qb)
    a_with = dict(zip(db.last_query()["id"].tolist(), db.last_query()["acc"].tolist()))
    a_without = dict(zip(first.last_query()["id"].tolist(), first.last_query()["acc"].tolist()))
    s_b = np.float32(M.l1_score(qb[0], qb[1], s[0], s[1]))
    assert np.isnan(db.last_query()["score"][list(db.last_query()["id"]).index(0)])  # B does not score row 0
    assert np.float32(a_with[1]) == np.float32(s_b + score_r_from_a)  # ... but adds what A left; never-scored row 2 adds 0
    assert np.float32(a_without[1]) == s_b
    # a refused call in between changes nothing
    with pytest.raises(M.Refused):
        db.detect_reloc(np.array([3, 3], np.int32), np.array([0.5, 0.5]))
    db.detect_reloc(*qb)
    assert dict(zip(db.last_query()["id"].tolist(), db.last_query()["acc"].tolist()))[1] == a_with[1]


def test_loop_query_rules_and_refusals():
    db = M.KeyFrameDatabase(100)
    v = (np.arange(10, dtype=np.int32), np.full(10, 0.1))
    for k in range(4):
        db.add(k, *v)
    db.set_covisibles(1, [0, 2])
    s = np.float32(1.0)
    # connected row 0 is out; si >= minScore passes at equality; row 1 sums itself and row 2, the others stay below 0.75 * 2
    assert db.detect_loop(v[0], v[1], [0], float(s)) == [1]
    lq = db.last_query()
    assert lq["id"].tolist() == [1, 2, 3] and lq["acc"].tolist() == [2.0, 1.0, 1.0]  # row 0 adds nothing as a neighbour
    assert db.detect_loop(v[0], v[1], [], float(np.nextafter(s, np.float32(2)))) == []
    for bad in ((np.array([1, 1]), np.array([0.5, 0.5])), (np.array([2, 1]), np.array([0.5, 0.5])),
                (np.array([1, 100]), np.array([0.5, 0.5])), (np.array([-1, 1]), np.array([0.5, 0.5])),
                (np.array([1, 2]), np.array([0.5, np.inf])), (np.array([1, 2]), np.array([np.nan, 0.5]))):
        with pytest.raises(M.Refused):
            db.add(9, *bad)
        with pytest.raises(M.Refused):
            db.detect_reloc(*bad)
    with pytest.raises(M.Refused):
        db.add(1, *v)
    with pytest.raises(M.Refused):
        db.set_covisibles(1, list(range(11)))
    assert db.size() == 4 and db.detect_reloc(np.array([], np.int32), np.array([])) == [] and db.last_query()["id"].size == 0
    assert db.erase([1]) == 1 and 1 not in db.covis  # K7: erase forgets the erased key frame's list
    db.clear()
    assert db.size() == 0 and db.detect_reloc(*v) == []
