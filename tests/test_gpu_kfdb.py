"""The device KeyFrameDatabase against tests/kfdb_model.py (vs CPU restatement; DBoW2 boundary unpinned): candidate id
lists equal and in order, the records of the sharing list equal with scores and sums bit-equal.  Every
database starts with initial_rows = 2, so rows, pool and hash grow in every test that adds more."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import kfdb_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
LENGTHS = (1, 5, 63, 64, 65, 200, 1500)


@pytest.fixture(scope="module")
def F(gpu):
    import fuzz_kfdb
    return fuzz_kfdb


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def uniform(words, total=1.0):
    words = np.asarray(words, np.int32)
    return words, np.full(len(words), total / max(len(words), 1))


def planted(seed, n_words, n_kf, q_len):
    """a query and n_kf key frames sharing 1 .. all of its words, lengths from LENGTHS, ids not in add order, neighbour lists
    inside and across the groups (and naming ids that do not exist)"""
    rng = np.random.default_rng(seed)
    q = M.random_vector(rng, n_words, q_len)
    ids = (7 * rng.permutation(n_kf) + 1000).tolist()
    kfs = []
    for i, kf_id in enumerate(ids):
        length = min(int(LENGTHS[i % len(LENGTHS)] if i % 3 else rng.choice(LENGTHS)), n_words - len(q[0]))
        group = i % 4  # group g shares about g/3 of what it can
        keep = max(1, min(len(q[0]), length) * group // 3) if rng.random() < 0.9 else 0
        v = M.vector_from(rng, q[0], q[1], keep, n_words, max(length - keep, 0 if keep else 1))
        nb = [int(x) for x in rng.choice(ids + [5, 6], size=min(int(rng.integers(0, 11)), len(ids)), replace=False)]
        kfs.append((kf_id, v, nb))
    return q, kfs


def fill(pair, kfs, covis_first=False):
    for kf_id, v, nb in kfs:
        if covis_first:
            assert pair.set_covisibles(kf_id, nb) == ""
        assert pair.add(kf_id, *v) == ""
        if not covis_first:
            assert pair.set_covisibles(kf_id, nb) == ""


SCENES = [(1000, 0, 64, None), (1000, 1, 1, None), (1000, 3, 5, None), (100000, 64, 63, None), (100000, 65, 65, None),
          (1000, 300, 200, None), (100000, 300, 1500, None), (100000, 65, 200, "64"), (1000, 64, 64, "0")]


@pytest.mark.parametrize("n_words,n_kf,q_len,lds", SCENES)
def test_score_reloc_and_loop_on_planted_scenes(F, monkeypatch, n_words, n_kf, q_len, lds):
    """cases 1 and 2; `lds` forces the query through the global-memory path (staging limit below the query's length)"""
    if lds is None:
        monkeypatch.delenv("ORBGPU_DEBUG_KFDB_LDS_WORDS", raising=False)
    else:
        monkeypatch.setenv("ORBGPU_DEBUG_KFDB_LDS_WORDS", lds)
    q, kfs = planted(100 + n_kf + q_len, n_words, n_kf, q_len)
    pair = F.Pair(n_words, initial_rows=2)
    try:
        fill(pair, kfs, covis_first=(n_kf % 2 == 1))
        all_ids = [k[0] for k in kfs]
        assert pair.score(q[0], q[1], all_ids + [3, 999999]) == ""
        if kfs:
            got = pair.dev.score(q[0], q[1], all_ids + [3, 999999])
            assert np.isnan(got[-2:]).all() and not np.isnan(got[:-2]).any()
        assert pair.reloc(*q) == ""
        n_first = len(pair.model.last_query()["id"])
        assert n_first == sum(1 for k in kfs if np.intersect1d(k[1][0], q[0]).size)
        sc = pair.model.last_query()["score"]
        sc = sc[~np.isnan(sc)]
        for min_score in ([0.0] if not len(sc) else [0.0, float(np.median(sc)), float(sc.max())]):
            for conn in ([], all_ids[::3] + [4]):
                assert pair.loop(q[0], q[1], conn, min_score) == "", (min_score, len(conn))
        q2 = M.vector_from(np.random.default_rng(5), q[0], q[1], max(len(q[0]) // 3, 1), n_words, 7)
        assert pair.reloc(*q2) == ""  # rows q2 does not score add what the first reloc query left (K5)
        assert pair.reloc(*q) == ""
        # which instantiation ran is observable: every score launch of a forced scene read the query from global memory
        assert (pair.dev.debug_global_queries() > 0) == (lds is not None and n_kf > 0)
        if lds is not None:
            assert pair.dev.debug_global_queries() == 2 + 3 + 6  # 2 score calls, 3 reloc and 6 loop queries
    finally:
        pair.close()


def test_identical_row_scores_one_and_a_disjoint_row_zero(F):
    pair = F.Pair(1000, initial_rows=2)
    try:
        v = (np.array([0, 2, 4, 8, 900], np.int32), np.array([0.5, 0.25, 0.125, 0.0625, 0.0625]))
        assert pair.add(11, *v) == "" and pair.add(5, *uniform([1, 3, 5])) == "" and pair.add(8, *uniform([])) == ""
        got = pair.dev.score(v[0], v[1], [5, 11, 8, 12])
        # -s / 2.0 of an empty sum is -0.0, in the reference as well: a disjoint row scores (minus) zero
        assert got[0] == 0.0 and got[2] == 0.0 and bits(got[1]) == bits(1.0) and np.isnan(got[3])
        assert pair.score(v[0], v[1], [5, 11, 8, 12]) == ""
        rng = np.random.default_rng(3)
        for n in LENGTHS[:-1]:
            w = M.random_vector(rng, 1000, n)
            assert pair.add(100 + n, *w) == ""
            assert pair.dev.score(w[0], w[1], [100 + n])[0] == np.float32(M.l1_score(w[0], w[1], w[0], w[1])) == np.float32(1.0)
    finally:
        pair.close()


def test_k1_add_order_breaks_a_tie_on_the_first_common_word(F):
    pair = F.Pair(1000, initial_rows=2)
    try:
        q = uniform([10, 20, 30, 40])
        assert pair.add(9, *uniform([10, 20, 30])) == "" and pair.add(4, *uniform([10, 20, 40])) == ""
        assert pair.add(6, *uniform([5, 20, 30, 40])) == ""  # first common word 20: behind both
        assert pair.reloc(*q) == "" and pair.dev.last_query()["id"].tolist() == [9, 4, 6]
        assert pair.loop(q[0], q[1], [], 0.0) == "" and pair.dev.last_query()["first_word"].tolist() == [10, 10, 20]
        assert pair.erase([9]) == "" and pair.add(9, *uniform([10, 20, 30])) == ""  # a new sequence number
        assert pair.reloc(*q) == "" and pair.dev.last_query()["id"].tolist() == [4, 9, 6]
        assert pair.dev.DetectRelocalizationCandidates(*q).tolist() == pair.model.detect_reloc(*q)
    finally:
        pair.close()


@pytest.mark.parametrize("max_common", [1, 4, 5, 10, 11])
def test_k3_rows_at_the_threshold_and_one_above(F, max_common):
    min_common = M.min_common_words(max_common)
    assert min_common == {1: 0, 4: 3, 5: 4, 10: 8, 11: 8}[max_common]
    pair = F.Pair(1000, initial_rows=2)
    try:
        q = uniform(np.arange(100, 100 + max_common))
        assert pair.add(1, *uniform(np.arange(100, 100 + max_common))) == ""
        if min_common >= 1:
            assert pair.add(2, *uniform(list(range(100, 100 + min_common)) + [500])) == ""
        if min_common + 1 < max_common:
            assert pair.add(3, *uniform(list(range(100, 100 + min_common + 1)) + [600])) == ""
        assert pair.set_covisibles(1, [2, 3]) == ""
        for call in (lambda: pair.reloc(*q), lambda: pair.loop(q[0], q[1], [], 0.0)):
            assert call() == ""
            lq = pair.dev.last_query()
            scored = dict(zip(lq["id"].tolist(), (~np.isnan(lq["score"])).tolist()))
            assert scored[1] and not scored.get(2, False) and scored.get(3, True)
            assert dict(zip(lq["id"].tolist(), lq["words"].tolist()))[1] == max_common
    finally:
        pair.close()


def test_k4_connected_rows_the_equal_score_and_weak_neighbours(F):
    pair = F.Pair(1000, initial_rows=2)
    try:
        q = M.random_vector(np.random.default_rng(7), 1000, 40)
        rng = np.random.default_rng(8)
        assert pair.add(1, q[0], q[1]) == ""  # the best score there is: 1.0
        rows = {k: M.vector_from(rng, q[0], q[1], keep, 1000, 5) for k, keep in ((2, 38), (3, 36), (4, 35), (5, 2))}
        for k, v in rows.items():
            assert pair.add(k, *v) == ""
        assert pair.set_covisibles(2, [1, 5, 3]) == "" and pair.set_covisibles(3, [1]) == ""
        assert pair.loop(q[0], q[1], [1], 0.0) == ""  # connected: not in the list, adds nothing to rows 2 and 3
        lq = pair.dev.last_query()
        assert 1 not in lq["id"].tolist() and lq["id"].tolist() == pair.model.last_query()["id"].tolist()
        s = dict(zip(lq["id"].tolist(), lq["score"].tolist()))
        acc = dict(zip(lq["id"].tolist(), lq["acc"].tolist()))
        assert np.isnan(s[5])  # 2 words <= minCommonWords: in the list, not scored, and as a neighbour of row 2 ignored
        assert bits(acc[2]) == bits(np.float32(s[2]) + np.float32(s[3])) and bits(acc[3]) == bits(s[3])
        # min_score = the bits of row 3's own score: it passes (>=); one ulp more and it does not
        assert pair.loop(q[0], q[1], [1], s[3]) == ""
        assert not np.isnan(dict(zip(*[pair.dev.last_query()[k].tolist() for k in ("id", "acc")]))[3])
        assert pair.loop(q[0], q[1], [1], float(np.nextafter(np.float32(s[3]), np.float32(2)))) == ""
        assert np.isnan(dict(zip(*[pair.dev.last_query()[k].tolist() for k in ("id", "acc")]))[3])
        assert pair.loop(q[0], q[1], [], 0.0) == "" and pair.dev.DetectLoopCandidates(q[0], q[1], [], 0.0).tolist()[0] == 1
    finally:
        pair.close()


def test_k5_a_stale_score_is_added_and_a_refused_call_changes_nothing(F, gpu):
    words_r, words_s = np.arange(0, 10), np.arange(20, 30)
    r, s = uniform(words_r), uniform(words_s)
    qa = uniform(np.concatenate([words_r, words_s]))
    qb = uniform(np.concatenate([words_r[:1], words_s]))
    pair, fresh = F.Pair(64, initial_rows=2), F.Pair(64, initial_rows=2)
    try:
        for p in (pair, fresh):
            assert p.add(0, *r) == "" and p.add(1, *s) == "" and p.add(2, *uniform([29, 40])) == ""
            assert p.set_covisibles(1, [0, 2, 77]) == ""
        assert pair.reloc(*qa) == ""  # A scores rows 0 and 1
        score_r = dict(zip(*[pair.dev.last_query()[k].tolist() for k in ("id", "score")]))[0]
        assert score_r > 0
        assert pair.reloc(*qb) == "" and fresh.reloc(*qb) == ""
        with_a = {k: pair.dev.last_query()[k].copy() for k in ("id", "score", "acc")}
        without = dict(zip(*[fresh.dev.last_query()[k].tolist() for k in ("id", "acc")]))
        at = with_a["id"].tolist()
        s_b = with_a["score"][at.index(1)]
        assert np.isnan(with_a["score"][at.index(0)]) and np.isnan(with_a["score"][at.index(2)])
        assert bits(with_a["acc"][at.index(1)]) == bits(np.float32(s_b) + np.float32(score_r))  # row 0: from A; row 2: 0
        assert bits(without[1]) == bits(s_b)
        # a refused call between A and B leaves B's result unchanged
        again = F.Pair(64, initial_rows=2)
        try:
            assert again.add(0, *r) == "" and again.add(1, *s) == "" and again.add(2, *uniform([29, 40])) == ""
            assert again.set_covisibles(1, [0, 2, 77]) == ""
            assert again.reloc(*qa) == ""
            assert again.reloc(np.array([3, 3], np.int32), np.array([0.5, 0.5])) == ""  # refused by both
            with pytest.raises(gpu.OrbGpuError):
                again.dev.add(1, *s)  # a duplicate: refused
            assert again.reloc(*qb) == ""
            lq = again.dev.last_query()
            assert lq["id"].tolist() == at and bits(lq["acc"]).tolist() == bits(with_a["acc"]).tolist()
        finally:
            again.close()
    finally:
        pair.close()
        fresh.close()


def test_k6_one_entry_for_a_shared_best_neighbour_and_no_replacement_on_equal_scores(F):
    pair = F.Pair(1000, initial_rows=2)
    try:
        q = M.random_vector(np.random.default_rng(11), 1000, 30)
        rng = np.random.default_rng(12)
        best = (q[0], q[1])
        twin = M.vector_from(rng, q[0], q[1], 28, 1000, 3)
        assert pair.add(50, *M.vector_from(rng, q[0], q[1], 27, 1000, 4)) == ""
        assert pair.add(40, *twin) == "" and pair.add(41, *twin) == ""  # equal scores
        assert pair.add(30, *best) == ""
        assert pair.add(60, *M.vector_from(rng, q[0], q[1], 26, 1000, 4)) == ""
        assert pair.set_covisibles(50, [30]) == "" and pair.set_covisibles(60, [40, 30]) == ""
        assert pair.set_covisibles(40, [41]) == "" and pair.set_covisibles(41, [40]) == ""
        for call in (lambda: pair.reloc(*q), lambda: pair.loop(q[0], q[1], [], 0.01)):
            assert call() == ""
            lq = pair.dev.last_query()
            best_of = dict(zip(lq["id"].tolist(), lq["best_id"].tolist()))
            assert best_of[50] == 30 and best_of[60] == 30 and best_of[40] == 40 and best_of[41] == 41
        got = pair.dev.DetectRelocalizationCandidates(*q).tolist()
        assert got == pair.model.detect_reloc(*q) and got.count(30) == 1
    finally:
        pair.close()


def test_k7_neighbours_are_ids_resolved_when_the_query_runs(F):
    pair = F.Pair(1000, initial_rows=2)
    try:
        q = M.random_vector(np.random.default_rng(21), 1000, 20)
        assert pair.set_covisibles(1, [2]) == ""  # neither is in the database yet
        assert pair.add(1, q[0], q[1]) == ""
        assert pair.reloc(*q) == ""
        alone = pair.dev.last_query()["acc"][0]
        assert pair.add(2, q[0], q[1]) == ""
        assert pair.reloc(*q) == ""
        lq = pair.dev.last_query()
        assert lq["id"].tolist() == [1, 2] and bits(lq["acc"][0]) == bits(np.float32(alone) + np.float32(alone))
        assert pair.erase([2]) == "" and pair.reloc(*q) == ""
        assert bits(pair.dev.last_query()["acc"]).tolist() == bits(alone).tolist()
        assert pair.add(2, q[0], q[1]) == "" and pair.loop(q[0], q[1], [], 0.0) == ""
        assert bits(pair.dev.last_query()["acc"][0]) == bits(np.float32(alone) + np.float32(alone))
        # erase forgets the erased key frame's own list: row 1 comes back without neighbours, behind row 2
        assert pair.erase([1]) == "" and pair.add(1, q[0], q[1]) == "" and pair.reloc(*q) == ""
        lq = pair.dev.last_query()
        assert lq["id"].tolist() == [2, 1] and bits(lq["acc"]).tolist() == [bits(alone)[0], bits(alone)[0]]
    finally:
        pair.close()


def test_edits_erase_clear_and_a_refused_duplicate(F, gpu):
    q, kfs = planted(77, 1000, 40, 64)
    pair = F.Pair(1000, initial_rows=2)
    try:
        fill(pair, kfs)
        ids = [k[0] for k in kfs]
        assert pair.reloc(*q) == ""
        before = pair.dev.DetectRelocalizationCandidates(*q).tolist()
        pair.model.detect_reloc(*q)
        with pytest.raises(gpu.OrbGpuError) as ei:
            pair.dev.add(ids[3], *kfs[5][1])  # present: refused ...
        assert ei.value.status == gpu.EINVAL and pair.dev.size() == 40
        assert pair.add(ids[3], *kfs[5][1]) == ""  # ... by the model as well
        assert pair.dev.DetectRelocalizationCandidates(*q).tolist() == before  # ... and the next query is unchanged
        pair.model.detect_reloc(*q)
        assert pair.dev.erase([ids[0], 123456, ids[1], ids[0]]) == 2 and pair.model.erase([ids[0], 123456, ids[1], ids[0]]) == 2
        assert pair.dev.erase([123456]) == 0 and pair.dev.size() == 38
        assert pair.reloc(*q) == "" and pair.loop(q[0], q[1], ids[5:9], 0.0) == ""
        assert not set(pair.dev.last_query()["id"].tolist()) & {ids[0], ids[1]}
        assert pair.clear() == "" and pair.dev.size() == 0
        assert pair.reloc(*q) == "" and pair.dev.last_query()["id"].size == 0
        fill(pair, kfs[:10])  # the ids, rows and pool space are free again
        assert pair.reloc(*q) == "" and pair.loop(q[0], q[1], [], 0.0) == ""
    finally:
        pair.close()


def test_k9_empty_cases(F):
    pair = F.Pair(1000, initial_rows=2)
    try:
        q = uniform([1, 2, 3])
        assert pair.reloc(*q) == "" and pair.loop(q[0], q[1], [], 0.0) == ""  # empty database
        assert pair.dev.DetectRelocalizationCandidates(*q).size == 0
        assert pair.add(1, *uniform([7, 8])) == "" and pair.add(2, *uniform([])) == ""
        assert pair.reloc(*q) == "" and pair.dev.last_query()["id"].size == 0  # no sharing row
        assert pair.reloc(*uniform([])) == "" and pair.loop(*uniform([]), [1], 0.0) == ""  # empty query
        assert pair.score(*uniform([]), [1, 2, 3]) == ""
    finally:
        pair.close()


def test_the_same_calls_on_fresh_handles_give_the_same_bytes(F):
    q, kfs = planted(31, 100000, 65, 200)
    outs = []
    for _ in range(2):
        pair = F.Pair(100000, initial_rows=2)
        try:
            fill(pair, kfs)
            parts = []
            for call in (lambda: pair.dev.DetectRelocalizationCandidates(*q), lambda: pair.dev.DetectLoopCandidates(q[0], q[1], [], 0.01),
                         lambda: pair.dev.DetectRelocalizationCandidates(*q)):
                parts.append(call().tobytes())
                parts += [v.tobytes() for v in pair.dev.last_query().values()]
            parts.append(pair.dev.score(q[0], q[1], [k[0] for k in kfs]).tobytes())
            outs.append(b"".join(parts))
        finally:
            pair.close()
    assert outs[0] == outs[1] and len(outs[0]) > 1000


def test_a_small_capacity_still_reports_the_full_count(F):
    pair = F.Pair(1000, initial_rows=2)
    try:
        q = M.random_vector(np.random.default_rng(41), 1000, 30)
        for k in range(6):
            assert pair.add(10 - k, q[0], q[1]) == ""
        full = pair.dev.DetectRelocalizationCandidates(*q)
        assert full.tolist() == pair.model.detect_reloc(*q) == [10, 9, 8, 7, 6, 5]
        for call in (lambda cap: pair.dev.DetectRelocalizationCandidates(q[0], q[1], capacity=cap),
                     lambda cap: pair.dev.DetectLoopCandidates(q[0], q[1], [], 0.5, capacity=cap)):
            for cap in (0, 2, 6, 9):
                got, n = call(cap)
                assert n == 6 and got.tolist() == full.tolist()[:cap]
    finally:
        pair.close()


class KfRowMirror(C.Structure):
    """the device row of kfdb.hip (KfRow), for its size"""
    _fields_ = [("id", C.c_int64), ("off", C.c_int32), ("len", C.c_int32), ("alive", C.c_int32), ("reg", C.c_float),
                ("nn", C.c_int32), ("pad", C.c_int32), ("nb", C.c_int64 * 10)]


@pytest.mark.parametrize("what", ["rows", "pool"])
def test_a_refused_growth_leaves_the_database_as_it_was(gpu, monkeypatch, what):
    """The growth transaction of id_table.h (rows and hash) and grow_pool under ORBGPU_DEBUG_FAIL_ALLOC_OVER, on a database
    created with initial_rows = 2 (2 rows, a pool of 1024 entries).  rows: the third key frame needs 4 rows; the limit is one
    byte under the 4-row KfRow column, the largest allocation of that growth and its first.  pool: one key frame holds 1000
    entries, the next needs 100 more, so the pool doubles: the limit lets its id array (4 * 2048 bytes) through and refuses
    the value array (8 * 2048).  The add returns ENOMEM; size, relocalisation and loop candidates and the sharing list's
    scores and sums are what they were, bit for bit; then the add succeeds and the new key frame scores."""
    hook = "ORBGPU_DEBUG_FAIL_ALLOC_OVER"
    monkeypatch.delenv(hook, raising=False)
    rng = np.random.default_rng(9)
    n_words = 100000
    q = M.random_vector(rng, n_words, 60)
    if what == "rows":
        first = [(11, M.vector_from(rng, q[0], q[1], 40, n_words, 30)), (5, M.vector_from(rng, q[0], q[1], 20, n_words, 100))]
        new = (8, M.vector_from(rng, q[0], q[1], 30, n_words, 10))
        nbytes = 4 * C.sizeof(KfRowMirror)  # (a mirror that drifts from KfRow misses the hipMalloc size asserted below)
        limit = nbytes - 1
    else:
        first = [(11, M.vector_from(rng, q[0], q[1], 40, n_words, 960))]
        new = (8, M.vector_from(rng, q[0], q[1], 30, n_words, 70))
        assert len(first[0][1][0]) == 1000 and len(new[1][0]) == 100
        nbytes = 8 * 2048
        limit = 4 * 2048
    db = gpu.KeyFrameDatabase(n_words, initial_rows=2)
    for kf_id, v in first:
        db.add(kf_id, *v)
    db.set_covisibles(11, [5, 8, 77])
    db.set_covisibles(5, [11])
    db.set_covisibles(8, [11, 5])  # kept for the id until it is added

    def state():
        reloc = db.DetectRelocalizationCandidates(*q)
        reloc_list = db.last_query()
        loop = db.DetectLoopCandidates(q[0], q[1], [], 0.0)
        return [reloc, loop] + [reloc_list[k] for k in sorted(reloc_list)] + [v for _, v in sorted(db.last_query().items())]

    def same(a, b):
        return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))

    state()  # (the first relocalisation query writes the score registers the next ones read: K5)
    before = state()
    assert len(before[0]) >= 1 and len(before[1]) >= 1 and same(before, state())
    monkeypatch.setenv(hook, str(limit))
    with pytest.raises(gpu.OrbGpuError) as ei:
        db.add(new[0], *new[1])
    monkeypatch.delenv(hook)
    assert ei.value.status == gpu.ENOMEM and "hipMalloc(%d)" % nbytes in str(ei.value), str(ei.value)
    assert db.size() == len(first)
    assert np.isnan(db.score(q[0], q[1], [new[0]])[0])
    assert same(state(), before)
    db.add(new[0], *new[1])
    assert db.size() == len(first) + 1
    got = db.score(q[0], q[1], [new[0], 11])
    want = np.array([M.l1_score(q[0], q[1], *new[1]), M.l1_score(q[0], q[1], *first[0][1])], np.float32)
    assert np.array_equal(bits(got), bits(want))
    assert new[0] in db.DetectRelocalizationCandidates(*q).tolist() + db.last_query()["id"].tolist()
    db.close()
