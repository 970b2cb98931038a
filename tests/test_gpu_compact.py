"""orbgpu_covis_graph_compact and orbgpu_keyframe_db_compact on the device against tests/compact_model.py and
tests/kfdb_model.py: the result structure field for field and every query afterwards, exact equality (C1-C7, D1-D4 of
include/orbgpu.h).  Every graph starts with initial_rows = 2 and a pool of 8 slots, every database with initial_rows = 2.
The base map is 13 key frames -- twice covis_model.SLOT_SIZES (0, 1, 63, 64, 65, 130 slots) and one row of 4097 -- added in
descending id with descriptors from 8 patterns, attribute bytes and centres; refresh_points, compared bit for bit in both
halves, is what shows that descriptor and attribute bytes arrived at the right slots."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import compact_model as XM  # noqa: E402
import covis_model as M  # noqa: E402
import kfdb_model as KM  # noqa: E402
import refresh_model as RM  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = M.SLOT_SIZES + M.SLOT_SIZES + (4097,)
N_PTS = 90
UNKNOWN = 10 ** 9


@pytest.fixture(scope="module")
def F(gpu):
    import fuzz_compact
    fuzz_compact.Points.p = 0.0  # the tests say where the compactions fall
    return fuzz_compact


def base(F, seed=1, descriptors=True, sizes=SIZES):
    """the base map on a pair (device and model in step); returns (pair, rng, kf ids in add order, points, positions, refs)"""
    pair = F.CompactRefreshPair(initial_rows=2, initial_slots=8)
    rng = np.random.default_rng(seed)
    n = len(sizes)
    kf_ids = [2 ** 33 + 7 * (n - i) for i in range(n)]  # descending: rows are not in id order
    for k, s in zip(kf_ids, sizes):
        slots = rng.integers(0, N_PTS, s)
        slots[rng.random(s) < 0.2] = -1
        pair.add_keyframe(k, s, slots)
        pair.set_keypoints(k, (rng.integers(0, 3, s) | (rng.random(s) < 0.3) * 0x40 | (rng.random(s) < 0.1) * 0x80).astype(np.uint8))
        if descriptors:
            pair.set_descriptors(k, RM.PATTERNS[rng.integers(0, 8, s)] ^ (rng.random((s, 32)) < 0.02).astype(np.uint8))
    pair.set_centres(kf_ids, rng.random((n, 3)).astype(np.float32))
    pair.set_scale_factors(np.float32(1.2) ** np.arange(3, dtype=np.float32))
    for i, k in enumerate(kf_ids):  # a spanning tree over the rows and covisible lists that name rows and one id that is none
        if i:
            pair.set_parent(k, kf_ids[int(rng.integers(0, i))])
        pair.set_covisibles(k, [kf_ids[int(j)] for j in rng.permutation(n)[:4] if kf_ids[int(j)] != k] + [UNKNOWN])
    pts = list(range(N_PTS))
    v = rng.normal(size=(N_PTS, 3))
    pos = (0.5 + v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(2.0, 6.0, (N_PTS, 1))).astype(np.float32)
    ref = [kf_ids[int(rng.integers(n))] for _ in pts]
    return pair, rng, kf_ids, pts, pos, ref


def check_all(pair, rng, ids, pts, pos, ref):
    """every query of the graph on device and model; '' or the first difference.  ids: key frame ids to ask about, dropped
    and unknown ones among them"""
    errs = [pair.size()]
    errs.append(pair.local_map([int(p) for p in rng.integers(-1, N_PTS, 50)], []))
    errs.append(pair.local_map([pts[3], pts[3], pts[17]], list(ids)))
    errs.append(pair.local_map([-1, 10 ** 12], list(ids) + [UNKNOWN]))  # no vote: the previous list, unknown ids counted
    for k in list(ids) + [UNKNOWN]:
        errs.append(pair.connections(k, 1))
    errs.append(pair.connections(ids[-1], 15))
    for th in (1, 3):
        errs.append(pair.keyframe_culling(list(ids) + [UNKNOWN], None, th))
    errs.append(pair.observations(pts + [-1, 10 ** 12]))
    for what in (RM.DESCRIPTOR, RM.NORMAL_DEPTH, RM.DESCRIPTOR | RM.NORMAL_DEPTH):
        errs.append(pair.refresh(pts, ref, pos, what, RM.junk(rng, len(pts))))
    return next((e for e in errs if e), "")


def answers(dev, ids, pts, pos, ref):
    """what a device graph answers, as plain lists (floats as bit patterns): for comparing two device graphs"""
    def flat(d):
        out = {}
        for k, v in d.items():
            v = np.asarray(v)
            out[k] = (v.view(np.uint32) if v.dtype == np.float32 else v).tolist()
        return out
    out = [dev.size(), flat(dev.local_map(pts[:50], [])), flat(dev.local_map([-1], list(ids)))]
    out += [flat(dev.connections(k, 1)) for k in ids]
    out.append(flat(dev.keyframe_culling(list(ids), None, 1)))
    out.append([a.tolist() for a in dev.observations(pts)])
    out.append(flat(dev.refresh_points(pts, ref, pos, 3)))
    return out


def twin_of(gpu, model):
    """a fresh device graph that holds only what the model holds, in the same add order"""
    g = gpu.CovisibilityGraph(initial_rows=2, initial_slots=8)
    for r in model.rows:
        g.add_keyframe(r.id, len(r.slots), None if r.bad else r.slots)
        if not r.bad:
            g.set_keypoints(r.id, model.kp[r.id])
            if r.id in model.desc:
                g.set_descriptors(r.id, model.desc[r.id])
            if r.id in model.centre:
                g.set_centres([r.id], [model.centre[r.id]])
            g.set_covisibles(r.id, r.nb)
        g.set_parent(r.id, r.parent)
        if r.bad:
            g.set_bad([r.id])
    if model.scale is not None:
        g.set_scale_factors(model.scale)
    return g


BAD_SETS = {"none": [], "first": [0], "last": [len(SIZES) - 1], "alternating": list(range(0, len(SIZES), 2)),
            "all": list(range(len(SIZES)))}


@pytest.mark.parametrize("which", list(BAD_SETS))
def test_graph_bad_sets(F, gpu, which):
    pair, rng, kf_ids, pts, pos, ref = base(F)
    twin = None
    try:
        bad = [kf_ids[i] for i in BAD_SETS[which]]
        for k in kf_ids:  # the hooks of SetBadFlag leave no live row with a bad parent
            if pair.model.row_of[k].parent in bad:
                pair.set_parent(k, -1)
        if bad:
            pair.set_bad(bad)
        slots_before = sum(SIZES)
        want = dict(compacted=int(bool(bad)), rows_before=13, rows_after=13 - len(bad), rows_bad_kept=0,
                    row_capacity=XM.fresh_capacity(1, 2, 13 - len(bad)), slots_before=slots_before,
                    slots_after=slots_before - sum(SIZES[i] for i in BAD_SETS[which]))
        want["slot_capacity"] = XM.fresh_capacity(1024, 8, want["slots_after"])
        got = pair.dev.compact()
        assert got == want and pair.model.compact() == want
        assert check_all(pair, rng, kf_ids, pts, pos, ref) == ""
        assert pair.dev.compact()["compacted"] == 0 and pair.model.compact()["compacted"] == 0  # twice in a row
        assert pair.dev.compact() == dict(want, compacted=0, rows_before=want["rows_after"], slots_before=want["slots_after"])
        # a fresh graph built from the surviving content answers every query identically
        twin = twin_of(gpu, pair.model)
        assert answers(pair.dev, kf_ids, pts, pos, ref) == answers(twin, kf_ids, pts, pos, ref)
        assert twin.compact()["compacted"] == 0 and twin.size() == pair.dev.size()
    finally:
        pair.close()
        if twin is not None:
            twin.close()


def test_bad_parent_survives_until_its_child_is_reparented(F, gpu):
    pair, rng, kf_ids, pts, pos, ref = base(F, 2)
    try:
        parent, child = kf_ids[5], kf_ids[9]  # 130 and 64 slots
        assert len(pair.model.row_of[parent].slots) == 130
        pair.set_parent(child, parent)
        for k in kf_ids:
            if k != child and pair.model.row_of[k].parent == parent:
                pair.set_parent(k, -1)
        gone = kf_ids[2]
        for k in kf_ids:
            if pair.model.row_of[k].parent == gone:
                pair.set_parent(k, -1)
        pair.set_slots([child] * 3, [0, 1, 2], [5000, 5001, 5002])  # points that only the child holds
        pair.set_bad([parent, gone])
        assert pair.compact() == ""
        assert [r.id for r in pair.model.rows if r.bad] == [parent] and gone not in pair.model.row_of and pair.dev.size() == (11, 1)
        # V6(c) still appends the bad parent: a query that only the child's points vote for
        own = [5000, 5001, 5002]
        res = pair.model.local_map(own, [])
        assert parent in res["kf_ids"].tolist()
        assert pair.local_map(own, []) == "" and check_all(pair, rng, kf_ids, pts, pos, ref) == ""
        # the kept bad row: known to set_bad / set_slots, which change nothing; its n_slots is still what the refusals read
        assert pair._edit("set_bad", [parent, gone]) == "" and pair.model.set_bad([parent, gone]) == 1
        assert pair._edit("set_slots", [parent, gone], [129, 10 ** 6], [5, 5]) == ""
        assert pair._edit("set_slots", [parent], [130], [5]) == ""  # refused by both: outside the row
        assert pair._edit("set_keypoints", parent, [0] * 129) == "" and pair._edit("set_keypoints", parent, [0] * 130) == ""
        assert pair._edit("set_descriptors", parent, np.zeros((130, 32), np.uint8)) == ""
        assert pair._edit("set_keypoints", gone, []) == "" and pair._edit("set_descriptors", gone, None) == ""  # refused: no row
        assert pair.compact() == "" and pair.model.rows[0].id == kf_ids[0]
        assert check_all(pair, rng, kf_ids, pts, pos, ref) == ""
        twin = twin_of(gpu, pair.model)
        try:
            assert answers(pair.dev, kf_ids, pts, pos, ref) == answers(twin, kf_ids, pts, pos, ref)
        finally:
            twin.close()
        # C2's deviation: a parent set to the dropped id is an unknown parent
        pair.set_parent(kf_ids[0], gone)
        assert check_all(pair, rng, kf_ids, pts, pos, ref) == ""
        # once the child is re-parented the next compaction drops the row
        pair.set_parent(child, kf_ids[0])
        got = pair.dev.compact()
        assert (got["compacted"], got["rows_before"], got["rows_after"], got["rows_bad_kept"], got["slots_before"], got["slots_after"]) == (
            1, 12, 11, 0, got["slots_after"], got["slots_after"])
        assert pair.model.compact()["rows_after"] == 11 and check_all(pair, rng, kf_ids, pts, pos, ref) == ""
    finally:
        pair.close()


def test_pending_values_readding_and_growth(F):
    pair, rng, kf_ids, pts, pos, ref = base(F, 3)
    try:
        drop = [kf_ids[1], kf_ids[6], kf_ids[12]]
        for k in kf_ids:
            if pair.model.row_of[k].parent in drop:
                pair.set_parent(k, -1)
        pair.set_bad(drop)
        new = 2 ** 33 + 1000
        pair.set_parent(new, kf_ids[0])  # pending values of an id that is no row yet (C4) ...
        pair.set_covisibles(new, [kf_ids[2], kf_ids[3]])
        assert pair.compact() == ""
        pair.set_parent(drop[0], kf_ids[3])  # ... and of a dropped id (C2)
        pair.set_covisibles(drop[0], [kf_ids[4]])
        assert pair.model.parents == {new: kf_ids[0], drop[0]: kf_ids[3]}
        rows, slots = pair.dev.compact()["row_capacity"], pair.dev.compact()["slot_capacity"]
        assert (rows, slots) == (16, 1024)
        pair.add_keyframe(new, 65, rng.integers(0, N_PTS, 65))
        pair.add_keyframe(drop[0], 7, [pts[3], -1, pts[17], 5, 6, 7, 8])  # a dropped id again: a new row at the end
        assert pair.model.rows[-1].id == drop[0] and pair.model.rows[-1].parent == kf_ids[3] and pair.model.parents == {}
        pair.set_keypoints(drop[0], [1, 2, 0, 0x41, 0x82, 0, 1])
        pair.set_descriptors(drop[0], RM.PATTERNS[:7])
        pair.set_centres([drop[0], new], [[0.1, 0.2, 0.3], [0.3, 0.2, 0.1]])
        assert check_all(pair, rng, kf_ids + [new], pts, pos, ref) == ""
        # growth of rows, pool (the three columns) and hash after the compaction
        more = []
        for i in range(24):
            k = 2 ** 34 + 3 * i
            pair.add_keyframe(k, 130, rng.integers(-1, N_PTS, 130))
            pair.set_keypoints(k, rng.integers(0, 3, 130).astype(np.uint8))
            pair.set_descriptors(k, RM.PATTERNS[rng.integers(0, 8, 130)])
            pair.set_centres([k], rng.random((1, 3)).astype(np.float32))
            pair.set_parent(k, kf_ids[0] if not more else more[-1])
            more.append(k)
        assert pair.model.row_cap == 64 and pair.model.pool_cap == 4096
        assert check_all(pair, rng, kf_ids + [new] + more[::5], pts, pos, ref) == ""
        pair.set_bad(more[1::2])  # every second of a parent chain: the hooks re-parent first
        for a, b in zip(more[2::2], more[0::2]):
            pair.set_parent(a, b)
        assert pair.compact() == "" and pair.model.compact()["compacted"] == 0
        assert check_all(pair, rng, kf_ids + more, pts, pos, ref) == ""
    finally:
        pair.close()


def test_descriptor_column_before_and_after(F):
    """a compaction before the first set_descriptors: the column comes afterwards, at the new capacity"""
    pair, rng, kf_ids, pts, pos, ref = base(F, 4, descriptors=False)
    try:
        for k in kf_ids:
            pair.set_parent(k, -1)
        pair.set_bad(kf_ids[4:])  # 4097 + ... slots go; 0 + 1 + 63 + 64 stay
        assert pair.compact() == "" and pair.model.pool_cap == 1024
        assert pair.model.refresh(pts, ref, pos)["n_descriptors"] == 0
        assert check_all(pair, rng, kf_ids, pts, pos, ref) == ""
        for k in kf_ids[1:4]:
            pair.set_descriptors(k, RM.PATTERNS[rng.integers(0, 8, len(pair.model.row_of[k].slots))])
        assert pair.model.refresh(pts, ref, pos)["n_descriptors"] > 20
        assert check_all(pair, rng, kf_ids, pts, pos, ref) == ""
        k = 77
        pair.add_keyframe(k, 4097, rng.integers(0, N_PTS, 4097))  # the three columns grow together
        pair.set_descriptors(k, RM.PATTERNS[rng.integers(0, 8, 4097)])
        pair.set_bad([kf_ids[2]])
        assert pair.compact() == ""  # ... and move together
        assert check_all(pair, rng, kf_ids + [k], pts, pos, ref) == ""
    finally:
        pair.close()


def test_clear_unbound_and_empty(F, gpu):
    g = gpu.CovisibilityGraph(initial_rows=2, initial_slots=8)
    try:
        zeros = dict.fromkeys(XM.RESULT_FIELDS, 0)
        assert g.compact() == zeros and g.compact() == zeros  # C6: a handle that was never bound
        g.add_keyframe(5, 3, [1, 2, 3])
        g.set_bad([5])
        g.clear()
        assert g.compact() == dict(zeros, row_capacity=2, slot_capacity=1024)  # nothing to drop after clear
        g.add_keyframe(5, 2, [1, 2])
        g.set_bad([5])
        assert g.compact() == dict(compacted=1, rows_before=1, rows_after=0, rows_bad_kept=0, row_capacity=2, slots_before=2,
                                   slots_after=0, slot_capacity=1024)
        assert g.size() == (0, 0) and g.local_map([1, 2], [5])["n_unknown_previous"] == 1
        g.add_keyframe(5, 2, [1, 2])
        assert g.size() == (1, 0) and g.local_map([1, 2], [])["kf_ids"].tolist() == [5]
    finally:
        g.close()


def test_culling_loop_and_table_refresh(F, gpu):
    """keyframe_culling -> the hooks of SetBadFlag -> compact -> keyframe_culling again; then the table form of the refresh"""
    pair, rng, kf_ids, pts, pos, ref = base(F, 5, sizes=(64,) * 10 + (130, 1, 0))
    table = None
    try:
        # six rows that hold the same points as row 0 at the same octave: redundant under th_obs = 3
        same = pair.model.row_of[kf_ids[0]].slots
        for k in kf_ids[1:7]:
            pair.set_slots([k] * 64, list(range(64)), same)
            pair.set_keypoints(k, [0] * 64)
        pair.set_keypoints(kf_ids[0], [0] * 64)
        cand = kf_ids[:10]
        assert pair.keyframe_culling(cand, None, 3) == ""
        res = pair.model.keyframe_culling(cand, None, 3)
        culled = [k for k, v in zip(cand, res["verdict"]) if v == 1]
        assert 1 <= len(culled) < 7
        want = pair.model.predicted(cand, res)
        for k in culled:  # KeyFrame::SetBadFlag's hooks: the children to the parent, the slots, the flag
            row = pair.model.row_of[k]
            for c in pair.model.children(k):
                pair.set_parent(c, row.parent if row.parent not in culled else -1)
            pair.set_bad([k])
        dead = [int(p) for p in res["bad_point_ids"]]
        for r in list(pair.model.rows):
            idx = [i for i, p in enumerate(r.slots) if p in dead]
            if idx:
                pair.set_slots([r.id] * len(idx), idx, [-1] * len(idx))
        assert pair.model.state() == want
        assert pair.compact() == "" and pair.dev.size() == (13 - len(culled), 0)
        assert pair.keyframe_culling(cand, None, 3) == "" and pair.model.keyframe_culling(cand, None, 3)["n_skipped"] == len(culled)
        assert check_all(pair, rng, kf_ids, pts, pos, ref) == ""
        # orbgpu_mappoint_table_refresh over the compacted graph
        table = gpu.MapPointTable(initial_rows=8)
        mirror = F.fuzz_refresh.fill_table(rng, table, pts[:80], pos[:80], n_bad=3)
        ids = [int(i) for i in rng.permutation(N_PTS)] + [10 ** 12]
        refs = [ref[p] for p in ids[:-1]] + [kf_ids[0]]
        assert pair.refresh_table(table, mirror, ids, refs, 3, RM.junk(rng, len(ids))) == ""
    finally:
        if table is not None:
            table.close()
        pair.close()


def test_failed_compaction_changes_nothing(F, gpu, monkeypatch):
    """C7: an allocation refused before the first pool column and between two of them"""
    pair, rng, kf_ids, pts, pos, ref = base(F, 6)
    try:
        for k in kf_ids:
            pair.set_parent(k, -1)
        pair.set_bad(kf_ids[1::3])  # (the row of 4097 slots stays)
        before = answers(pair.dev, kf_ids, pts, pos, ref)
        # afterwards the pool is 8192 slots: 64 KiB of ids, 8 KiB of attribute bytes, 256 KiB of descriptors
        for limit in (0, 100000):
            monkeypatch.setenv("ORBGPU_DEBUG_FAIL_ALLOC_OVER", str(limit))
            with pytest.raises(gpu.OrbGpuError) as e:
                pair.dev.compact()
            monkeypatch.delenv("ORBGPU_DEBUG_FAIL_ALLOC_OVER")
            assert e.value.status == gpu.ENOMEM
            assert answers(pair.dev, kf_ids, pts, pos, ref) == before
            assert check_all(pair, rng, kf_ids, pts, pos, ref) == ""
        assert pair.compact() == "" and pair.model.pool_cap == 8192
        assert check_all(pair, rng, kf_ids, pts, pos, ref) == ""
    finally:
        pair.close()


# ---- the key-frame database -------------------------------------------------------------------------------------------
N_WORDS = 1000
VEC_LENS = (0, 1, 63, 64, 65, 300)


def db_base(F, seed=11):
    """twelve key frames, two of every vector length, that share words with a base vector; neighbour lists set"""
    rng = np.random.default_rng(seed)
    pair = F.CompactKfdbPair(N_WORDS, initial_rows=2)
    basev = KM.random_vector(rng, N_WORDS, 300)
    ids = [50 - 3 * i for i in range(12)]
    for i, k in enumerate(ids):
        n = VEC_LENS[i % 6]
        v = KM.vector_from(rng, basev[0], basev[1], min(n, int(0.8 * n)), N_WORDS, n - min(n, int(0.8 * n)))
        assert len(v[0]) == n
        assert pair.add(k, *v) == ""
    for k in ids:
        assert pair.set_covisibles(k, [int(x) for x in rng.choice(ids, 4, replace=False)] + [999]) == ""
    return pair, rng, ids, basev


def db_check(pair, rng, ids, basev):
    errs = [pair.size()]
    for keep in (300, 150, 20):
        q = KM.vector_from(rng, basev[0], basev[1], keep, N_WORDS, 10)
        errs.append(pair.score(q[0], q[1], list(ids) + [999]))
        errs.append(pair.loop(q[0], q[1], [ids[1], ids[4], 999], 0.0))
        errs.append(pair.loop(q[0], q[1], [], 0.01))
        errs.append(pair.reloc(*q))
    return next((e for e in errs if e), "")


DB_SETS = {"none": [], "first": [0], "last": [11], "alternating": list(range(0, 12, 2)), "all": list(range(12))}


@pytest.mark.parametrize("which", list(DB_SETS))
def test_database_erased_sets(F, which):
    pair, rng, ids, basev = db_base(F)
    try:
        lens = {k: len(pair.model.kfs[k].ids) for k in ids}
        assert db_check(pair, rng, ids, basev) == ""  # leaves non-zero registers behind (K5)
        assert any(kf.reloc_score != 0 for kf in pair.model.kfs.values())
        gone = [ids[i] for i in DB_SETS[which]]
        if gone:
            assert pair.erase(gone) == ""
        got = pair.dev.compact()
        pair.model.compact()
        rows = 12 - len(gone)
        slots = sum(lens[k] for k in ids if k not in gone)
        assert got == dict(compacted=int(bool(gone)), rows_before=12, rows_after=rows, rows_bad_kept=0,
                           row_capacity=XM.fresh_capacity(1, 2, rows), slots_before=sum(lens.values()), slots_after=slots,
                           slot_capacity=XM.fresh_capacity(1024, 1024, slots))  # (nothing erased: the capacities only grew)
        assert len(pair.dev.last_query()["id"]) == 0  # D2, as after clear
        assert db_check(pair, rng, ids, basev) == ""
        assert pair.compact() == "" and pair.dev.compact()["compacted"] == 0
    finally:
        pair.close()


def test_database_register_survives(F):
    """K5 after a compaction: a reloc query reads the register of a neighbour it does not score itself"""
    rng = np.random.default_rng(12)
    pair = F.CompactKfdbPair(N_WORDS, initial_rows=2)
    try:
        a, b = KM.random_vector(rng, 500, 64), KM.random_vector(rng, 500, 65)
        b = (b[0] + 500, b[1])  # no word in common with a
        assert pair.add(9, *a) == "" and pair.add(8, *KM.random_vector(rng, 500, 63)) == "" and pair.add(7, *b) == ""
        assert pair.add(6, *KM.random_vector(rng, 500, 1)) == ""
        assert pair.set_covisibles(7, [9]) == "" and pair.set_covisibles(9, [7, 8]) == ""
        assert pair.reloc(*a) == ""  # scores 9 (and whoever shares words): its register is written
        assert pair.model.kfs[9].reloc_score > 0
        assert pair.erase([8, 6]) == "" and pair.compact() == ""
        assert pair.dev.compact()["compacted"] == 0 and pair.dev.size() == 2
        # a query that shares every word with 7 and one with 9: 9 is met but not scored, and 7 adds what the earlier query
        # left in 9's register
        q = np.sort(np.concatenate([b[0], a[0][:1]])).astype(np.int32)
        qv = np.full(len(q), 1.0 / len(q))
        assert pair.reloc(q, qv) == ""
        rec = pair.model.last_query()
        i7, i9 = rec["id"].tolist().index(7), rec["id"].tolist().index(9)
        assert np.isnan(rec["score"][i9]) and rec["acc"][i7] > rec["score"][i7] > 0
        assert pair.reloc(*a) == "" and pair.loop(a[0], a[1], [], 0.0) == ""
    finally:
        pair.close()


def test_database_readd_growth_and_global_path(F, monkeypatch):
    monkeypatch.setenv("ORBGPU_DEBUG_KFDB_LDS_WORDS", "8")
    pair, rng, ids, basev = db_base(F, 13)
    try:
        assert pair.erase([ids[3]]) == "" and pair.add(ids[3], *KM.random_vector(rng, N_WORDS, 64)) == ""  # erased and re-added before
        assert pair.erase([ids[5], ids[7]]) == ""
        got = pair.dev.compact()
        pair.model.compact()
        assert (got["rows_before"], got["rows_after"]) == (13, 10)
        assert pair.add(ids[5], *KM.vector_from(rng, basev[0], basev[1], 100, N_WORDS, 5)) == ""  # ... and after
        assert pair.set_covisibles(ids[5], [ids[0], ids[3]]) == ""
        assert db_check(pair, rng, ids, basev) == ""
        n0 = pair.dev.debug_global_queries()
        assert n0 > 0
        for i in range(40):  # growth of rows, pool and hash after the compaction
            assert pair.add(1000 + i, *KM.vector_from(rng, basev[0], basev[1], 30, N_WORDS, 30)) == ""
        assert db_check(pair, rng, ids + [1000, 1039], basev) == ""
        assert pair.erase([1000 + i for i in range(0, 40, 2)]) == "" and pair.compact() == ""
        assert db_check(pair, rng, ids + [1000, 1039], basev) == "" and pair.dev.debug_global_queries() > n0
    finally:
        pair.close()


def test_database_unbound_and_clear(F, gpu):
    db = gpu.KeyFrameDatabase(N_WORDS, initial_rows=2)
    try:
        zeros = dict.fromkeys(XM.RESULT_FIELDS, 0)
        assert db.compact() == zeros  # D4: a handle that was never bound
        db.add(1, [1, 2], [0.5, 0.5])
        db.erase([1])
        db.clear()
        assert db.compact() == dict(zeros, row_capacity=2, slot_capacity=1024)
        db.add(1, [1, 2], [0.5, 0.5])
        db.erase([1])
        assert db.compact() == dict(compacted=1, rows_before=1, rows_after=0, rows_bad_kept=0, row_capacity=2, slots_before=2,
                                    slots_after=0, slot_capacity=1024)
        assert db.size() == 0 and list(db.DetectRelocalizationCandidates([1, 2], [0.5, 0.5])) == []
        db.add(1, [1, 2], [0.5, 0.5])
        assert list(db.DetectRelocalizationCandidates([1, 2], [0.5, 0.5])) == [1]
    finally:
        db.close()
