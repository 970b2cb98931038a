"""tests/compact_model.py without a device: C1-C4 on hand cases, and the property that makes compaction safe to call at any
time -- on random PointerMap histories a model compacted at random points and one that never is agree on every query that
names no dropped id, and where they differ they differ only as C2 says."""
import numpy as np
import pytest

import compact_model as XM
import covis_model as M
import cull_model as CM
import kfdb_model as KM
import refresh_model as RM


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (k, a[k], b[k])


def small_graph(cls=XM.CompactGraph, **kw):
    """rows 10, 11, 12, 13 (3, 0, 2, 4 slots); 11's parent is 10, 13's parent is 12, 12's parent is 10"""
    g = cls(**kw)
    g.add_keyframe(10, 3, [1, 2, 3])
    g.add_keyframe(11, 0)
    g.add_keyframe(12, 2, [2, -1])
    g.add_keyframe(13, 4, [3, 3, 7, 1])
    g.set_parent(11, 10)
    g.set_parent(12, 10)
    g.set_parent(13, 12)
    g.set_covisibles(13, [10, 12, 99])
    return g


def test_nothing_to_do():
    g = XM.CompactGraph(initial_rows=2, initial_slots=8)
    assert g.compact() == dict(compacted=0, rows_before=0, rows_after=0, rows_bad_kept=0, row_capacity=0, slots_before=0,
                               slots_after=0, slot_capacity=0)  # C6 on a handle that was never bound
    g = small_graph(initial_rows=2, initial_slots=8)
    r = g.compact()
    assert r == dict(compacted=0, rows_before=4, rows_after=4, rows_bad_kept=0, row_capacity=4, slots_before=9, slots_after=9,
                     slot_capacity=1024)
    assert [x.id for x in g.rows] == [10, 11, 12, 13]


def test_c1_kept_rows():
    g = small_graph(initial_rows=2, initial_slots=8)
    g.set_bad([10, 12])
    # 10 is named by 11 (live); 12 by 13 (live): both stay, and own nothing afterwards
    r = g.compact()
    assert (r["compacted"], r["rows_after"], r["rows_bad_kept"], r["slots_before"], r["slots_after"]) == (1, 4, 2, 9, 4)
    assert [x.id for x in g.rows] == [10, 11, 12, 13] and g.size() == (2, 2)
    assert g.compact()["compacted"] == 0  # twice in a row
    # a bad parent of a bad row is not kept: 13 goes bad, 12 is named by nobody live; 10 is still named by 11
    g.set_bad([13])
    r = g.compact()
    assert (r["rows_before"], r["rows_after"], r["rows_bad_kept"], r["slots_before"], r["slots_after"]) == (4, 2, 1, 4, 0)
    assert [x.id for x in g.rows] == [10, 11] and g.size() == (1, 1)
    # once the child is re-parented, the next compaction drops 10; a parent id that is no row keeps nothing
    g.set_parent(11, 4242)
    r = g.compact()
    assert (r["rows_after"], r["rows_bad_kept"]) == (1, 0) and [x.id for x in g.rows] == [11]
    assert r["row_capacity"] == 2 and r["slot_capacity"] == 1024  # C5: what a fresh handle created for (2, 8) has
    # everything bad: an empty graph
    g.set_bad([11])
    r = g.compact()
    assert (r["rows_after"], r["slots_after"], r["row_capacity"]) == (0, 0, 2) and g.rows == [] and g.size() == (0, 0)


def test_c2_dropped_id_is_unknown():
    g = small_graph()
    g.set_bad([13])
    assert g.set_bad([13]) == 1 and g.set_slots([13], [0], [5]) == 1  # a bad row is a known row
    g.compact()
    assert 13 not in g.row_of
    assert g.set_bad([13]) == 0 and g.set_slots([13], [99], [5]) == 0  # not counted, not even range-checked
    assert g.local_map([1], [13, 10])["n_unknown_previous"] == 1  # (counted also when a row has a vote and the list is not used)
    res = g.local_map([555], [13, 10])
    assert res["kept_previous"] == 1 and res["n_unknown_previous"] == 1 and list(res["kf_ids"]) == [10]
    # pending maps, as for any id that is no row
    g.set_parent(13, 11)
    g.set_covisibles(13, [10])
    assert g.parents == {13: 11} and g.covis == {13: [10]}
    g.add_keyframe(13, 2)  # accepted again: a new empty row at the end
    row = g.rows[-1]
    assert (row.id, row.slots, row.parent, row.nb, row.bad) == (13, [-1, -1], 11, [10], False)
    assert g.parents == {} and g.covis == {}
    # the deviation: a parent set to a dropped id is an unknown parent, which V6(c) does not append
    a, b = small_graph(), small_graph(cls=M.CovisGraph)
    for x in (a, b):
        x.set_bad([11])
    a.compact()
    for x in (a, b):
        x.set_parent(10, 11)
    assert list(b.local_map([1])["kf_ids"]) == [10, 13, 12, 11]  # 12: 10's first live child; 11: 10's parent, bad, and the end
    assert list(a.local_map([1])["kf_ids"]) == [10, 13, 12]


def test_c3_kept_row_is_what_it_was():
    g = small_graph(cls=XM.CompactRefreshGraph)
    g.set_keypoints(13, [1, 2, 0x41, 0x80])
    g.set_descriptors(13, np.arange(128, dtype=np.uint8).reshape(4, 32))
    g.set_centres([13, 10], [[1, 2, 3], [4, 5, 6]])
    g.local_map([7])  # stamps 13
    stamp13 = g.row_of[13].stamp
    g.set_bad([10, 11])
    before = {k: (list(r.slots), r.parent, list(r.nb), r.bad, r.stamp) for k, r in g.row_of.items()}
    r = g.compact()
    assert r["rows_after"] == 3 and [x.id for x in g.rows] == [10, 12, 13]  # 10 is named by 12
    for k, row in g.row_of.items():
        assert (row.slots, row.parent, row.nb, row.bad, row.stamp) == before[k]
    assert g.row_of[13].stamp == stamp13 != 0
    assert g.kp[13] == [1, 2, 0x41, 0x80] and g.desc[13][3, 5] == 101 and list(g.centre[13]) == [1, 2, 3]
    assert 11 not in g.kp and len(g.row_of[10].slots) == 3  # n_slots of a kept bad row stays
    with pytest.raises(M.Refused):
        g.set_keypoints(10, [0, 0])  # ... because the refusals read it
    with pytest.raises(M.Refused):
        g.set_keypoints(11, [])  # a dropped id is no row
    # a re-added id starts without descriptors and centre
    g.set_bad([13])
    g.compact()
    g.add_keyframe(13, 4, [3, 3, 7, 1])
    assert 13 not in g.desc and 13 not in g.centre and g.kp[13] == [0, 0, 0, 0]


def test_c4_untouched():
    g = small_graph(cls=XM.CompactRefreshGraph)
    g.set_scale_factors([1.0, 1.2])
    g.set_parent(77, 10)
    g.set_covisibles(78, [10, 11])
    g.local_map([1])
    stamp = g.stamp
    g.set_bad([13])
    g.compact()
    assert g.parents == {77: 10} and g.covis == {78: [10, 11]} and g.stamp == stamp and list(g.scale) == [np.float32(1.0), np.float32(1.2)]


def test_c5_capacities():
    g = XM.CompactGraph(initial_rows=2, initial_slots=8)
    for k in range(9):
        g.add_keyframe(k, 300)
    assert (g.row_cap, g.pool_cap) == (16, 4096)
    g.set_bad(list(range(1, 9)))
    r = g.compact()
    assert (r["rows_after"], r["slots_after"], r["row_capacity"], r["slot_capacity"]) == (1, 300, 2, 1024)
    g.clear()  # capacities outlive clear
    assert g.compact() == dict(compacted=0, rows_before=0, rows_after=0, rows_bad_kept=0, row_capacity=2, slots_before=0,
                               slots_after=0, slot_capacity=1024)
    assert XM.fresh_capacity(1, 1024, 3) == 1024 and XM.fresh_capacity(1, 3, 5) == 8 and XM.fresh_capacity(1024, 8, 4420) == 8192
    assert XM.graph_initial(0, 0) == (1024, 1 << 20) and XM.graph_initial(8192, 0) == (8192, 1 << 22)


def test_database_model():
    db = XM.CompactKeyFrameDatabase(100)
    ids, vals = np.array([1, 5, 9]), np.array([0.5, 0.25, 0.25])
    db.add(3, ids, vals)
    db.add(4, ids, vals)
    db.detect_reloc(ids, vals)
    assert len(db.last_query()["id"]) == 2
    db.erase([3])
    db.compact()
    assert len(db.last_query()["id"]) == 0 and db.size() == 1 and db.pool_used() == 3
    assert list(db.detect_reloc(ids, vals)) == [4] and len(db.last_query()["id"]) == 1


# ---- the property -----------------------------------------------------------------------------------------------------
class Both:
    """hooks to model A (compacted at random points, after any hook) and model B (never compacted)"""

    def __init__(self, rng, p):
        self.a, self.b, self.rng, self.p = XM.CompactCullGraph(initial_rows=2, initial_slots=8), CM.CullGraph(), rng, p
        self.dropped = set()
        self.compactions = self.rows_dropped = 0

    def maybe_compact(self):
        if self.rng.random() >= self.p:
            return
        ids = {r.id for r in self.a.rows}
        res = self.a.compact()
        gone = ids - {r.id for r in self.a.rows}
        assert res["compacted"] == int(bool(gone) or res["slots_after"] != res["slots_before"])
        assert res["rows_before"] - res["rows_after"] == len(gone)
        self.dropped |= gone
        self.compactions += res["compacted"]
        self.rows_dropped += len(gone)

    def __getattr__(self, name):
        def call(*args):
            ra, rb = getattr(self.a, name)(*args), getattr(self.b, name)(*args)
            if name == "add_keyframe":
                self.dropped.discard(int(args[0]))
            elif name in ("set_bad", "set_slots"):  # C2: *known leaves the dropped ids out
                assert ra == rb - sum(1 for k in args[0] if int(k) in self.dropped)
            self.maybe_compact()
        return call


def compare_queries(rng, both, pm):
    a, b, dropped = both.a, both.b, both.dropped
    assert a.size()[0] == b.size()[0] and sum(b.size()) - sum(a.size()) == len(dropped)
    assert {r.id for r in b.rows} - {r.id for r in a.rows} == dropped and all(b.row_of[k].bad for k in dropped)
    assert [r.id for r in a.rows] == [r.id for r in b.rows if r.id not in dropped]  # add order
    frame = M.random_frame(rng, pm)
    kp = pm.frame_kp_ids(frame)
    prev = [int(k) for k in rng.choice([r.id for r in b.rows] + [10 ** 9], size=int(rng.integers(0, 6)))]
    # (the stamp counters move together: both models answer every query)
    for q, p in ((kp, prev), ([-1], prev)):  # the second has no vote: the previous list is kept
        ra, rb = a.local_map(q, p), b.local_map(q, p)
        n_dropped = sum(1 for k in p if k in dropped)
        if rb["kept_previous"]:
            rb = dict(rb, n_unknown_previous=rb["n_unknown_previous"] + n_dropped,
                      kf_ids=np.array([k for k in rb["kf_ids"] if k not in dropped], np.int64))
            rb["n_kfs"] = len(rb["kf_ids"])  # (bad rows hold no points: the point list is the same)
        else:
            rb = dict(rb, n_unknown_previous=rb["n_unknown_previous"] + n_dropped)
        same(ra, rb)
    for k in [r.id for r in b.rows] + [10 ** 9]:
        same(a.connections(k, 1), b.connections(k, 1))
    cand = [int(k) for k in rng.choice([r.id for r in b.rows], size=int(rng.integers(0, 8)))]
    same(a.keyframe_culling(cand), b.keyframe_culling(cand))
    pts = list(pm.mps)[:50] + [-1]
    same(dict(zip("ab", a.observations(pts))), dict(zip("ab", b.observations(pts))))
    return 4 + len(b.rows)


@pytest.mark.parametrize("seed", range(6))
def test_compacted_and_never_compacted_agree(seed):
    rng = np.random.default_rng(9100 + seed)
    both = Both(rng, p=0.08)
    pm = M.PointerMap(both)
    next_ids = [int(rng.integers(0, 3)), 0]
    queries = 0
    for step in range(220):
        u = rng.random()
        if u < 0.70 or len(pm.kfs) < 3:
            M.random_edit(rng, pm, next_ids)
        elif u < 0.78:
            # a parent the reference's ChangeParent never hands out: a bad row that is still a row, or an id that is none
            live = [r.id for r in both.a.rows if not r.bad]
            bad = [r.id for r in both.a.rows if r.bad] + [10 ** 9]
            if live:
                both.set_parent(live[int(rng.integers(len(live)))], bad[int(rng.integers(len(bad)))])
        else:
            queries += compare_queries(rng, both, pm)
    queries += compare_queries(rng, both, pm)
    assert both.compactions >= 3 and both.rows_dropped >= 3 and queries > 100
