"""The device observation graph (orbgpu_covis_*) against tests/covis_model.py: exact equality of every output of
orbgpu_covis_local_map and orbgpu_covis_connections on planted maps of at most about 120 key frames.
Every graph starts with initial_rows = 2 and a pool of 8 slots, so rows, pool and hash grow in every test that adds more."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import covis_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
LDS_IDS = 4096  # CV_LDS_IDS of covis.hip
BIG = 2 ** 33


@pytest.fixture(scope="module")
def F(gpu):
    import fuzz_covis
    return fuzz_covis


def make(F, **kw):
    pair = F.Pair(initial_rows=kw.pop("initial_rows", 2), initial_slots=kw.pop("initial_slots", 8))
    return pair, M.PointerMap(pair, **kw)


def planted(pm, seed, n_kf, n_pts, first_kf=1, first_mp=BIG, descending=False):
    """n_kf key frames of 0, 1, 63, 64, 65 and 130 slots over n_pts shared points (ids above 2^32), parents and covisibles
    through UpdateConnections; ids added in descending order if asked"""
    rng = np.random.default_rng(seed)
    pts = [pm.NewMapPoint(first_mp + 3 * i) for i in range(n_pts)]
    ids = [first_kf + 2 * i for i in range(n_kf)]
    for i, kf_id in enumerate(reversed(ids) if descending else ids):
        n = M.SLOT_SIZES[i % len(M.SLOT_SIZES)]
        kf = pm.AddKeyFrame(kf_id, n)
        take = rng.permutation(n)[:int(rng.integers(0, n + 1))]
        chosen = rng.choice(n_pts, size=len(take), replace=False) if len(take) <= n_pts else rng.integers(0, n_pts, size=len(take))
        pm.AddObservations(kf, [(int(a), pts[int(b)]) for a, b in zip(take, chosen)])
        pm.UpdateConnections(kf, th=int(rng.choice([1, 3, 15])))
    return pts


def all_queries(pair, pm, rng, n_frames=6):
    for _ in range(n_frames):
        frame = M.random_frame(rng, pm, n=int(rng.integers(1, 90)))
        prev = [k.mnId for k in pm.mvpLocalKeyFrames]
        assert pair.local_map(pm.frame_kp_ids(frame), prev) == ""
        pm.UpdateLocalMap(frame)
    for kf_id in list(pm.kfs) + [10 ** 9]:
        for th in (1, 15):
            assert pair.connections(kf_id, th) == "", (kf_id, th)


@pytest.mark.parametrize("seed,n_kf,n_pts,descending", [(1, 12, 40, False), (2, 60, 300, True), (3, 120, 150, False)])
def test_planted_maps_with_growth_bad_rows_and_interleaved_edits(F, seed, n_kf, n_pts, descending):
    pair, pm = make(F)
    try:
        rng = np.random.default_rng(seed)
        pts = planted(pm, seed, n_kf, n_pts, descending=descending)
        all_queries(pair, pm, rng)
        # edits between queries: bad points, replaced points, bad key frames (bad parents, bad covisibles), new key frames
        next_ids = [10 ** 6, 10 ** 12]
        for step in range(60):
            M.random_edit(rng, pm, next_ids)
            if step % 6 == 5:
                frame = M.random_frame(rng, pm, n=int(rng.integers(1, 90)))
                assert pair.local_map(pm.frame_kp_ids(frame), [k.mnId for k in pm.mvpLocalKeyFrames]) == ""
                pm.UpdateLocalMap(frame)
        assert pair.model.size()[1] > 0 and pair.size() == ""
        pair.set_covisibles(1, [10 ** 9, 3, 5])  # an id that is no row
        all_queries(pair, pm, rng, n_frames=3)
        assert len(pts) == n_pts
    finally:
        pair.close()


def big_frame_graph(pair, n_ids):
    """two key frames whose slots hold ids 0 .. n_ids - 1 between them; the query names them all"""
    half = n_ids // 2
    pair.add_keyframe(5, half, list(range(half)))
    pair.add_keyframe(3, n_ids - half, list(range(half, n_ids)))
    pair.add_keyframe(9, 2, [n_ids + 5, 0])
    return list(range(n_ids))


@pytest.mark.parametrize("n_ids", [0, 1, LDS_IDS - 1, LDS_IDS, LDS_IDS + 1])
def test_query_lengths_around_the_lds_limit(F, monkeypatch, n_ids):
    monkeypatch.delenv("ORBGPU_DEBUG_COVIS_LDS_IDS", raising=False)
    pair, _ = make(F)
    try:
        q = big_frame_graph(pair, max(n_ids, 2))[:n_ids]
        assert pair.local_map(q + [-1] + q[:3], []) == ""
        assert pair.local_map(q, [3, 77]) == ""
        assert (pair.dev.debug_global_queries() > 0) == (n_ids > LDS_IDS)
    finally:
        pair.close()


@pytest.mark.parametrize("limit", [0, 4, 5, 6])
def test_the_debug_variable_sends_small_queries_through_global_memory(F, monkeypatch, limit):
    monkeypatch.setenv("ORBGPU_DEBUG_COVIS_LDS_IDS", str(limit))
    pair, pm = make(F)  # (the variable is read when the handle is created)
    monkeypatch.delenv("ORBGPU_DEBUG_COVIS_LDS_IDS")
    try:
        planted(pm, 11, 20, 30)
        q5 = [BIG, BIG + 3, BIG + 6, BIG + 9, BIG + 12]
        assert pair.model.local_map(q5, [])["n_voted"] > 0
        before = pair.dev.debug_global_queries()
        assert pair.local_map(q5 + q5[:2], [], 3, 7) == ""  # five distinct ids, one launch
        assert pair.dev.debug_global_queries() - before == (1 if limit < 5 else 0)
        all_queries(pair, pm, np.random.default_rng(4), n_frames=3)
        assert pair.dev.debug_global_queries() > 0  # connection queries of more than six ids among them
    finally:
        pair.close()


@pytest.mark.parametrize("n_voted,extended", [(80, True), (81, False)])
def test_eighty_voted_rows_extend_and_eighty_one_do_not(F, n_voted, extended):
    pair, pm = make(F)
    try:
        for k in range(1, 101):
            pm.AddObservations(pm.AddKeyFrame(k, 2), [(0, pm.NewMapPoint(BIG + k))])
        pair.set_covisibles(1, [100])
        pair.set_parent(100, 2)
        frame = [pm.mps[BIG + k] for k in range(1, n_voted + 1)]
        assert pair.local_map(pm.frame_kp_ids(frame), []) == ""
        got = pair.dev.local_map(pm.frame_kp_ids(frame), [])
        assert got["n_voted"] == n_voted and got["kf_ids"].tolist() == list(range(1, n_voted + 1)) + ([100] if extended else [])
    finally:
        pair.close()


def test_the_parent_break_a_bad_parent_and_unknown_or_bad_covisibles(F):
    pair, pm = make(F)
    try:
        for k in range(1, 10):
            pm.AddObservations(pm.AddKeyFrame(k, 3), [(1, pm.NewMapPoint(BIG + k))])
        pair.set_parent(2, 5)
        pair.set_parent(3, 6)
        pair.set_parent(7, 3)
        pair.set_covisibles(3, [8])
        q = [BIG + 2, BIG + 3, BIG + 3]
        assert pair.local_map(q, []) == "" and pair.dev.local_map(q, [])["kf_ids"].tolist() == [2, 3, 5]
        assert pair.local_map(q + [BIG + 5], []) == "" and pair.dev.local_map(q + [BIG + 5], [])["kf_ids"].tolist() == [2, 3, 5, 8, 7, 6]
        pair.set_bad([5, 8])  # a bad parent is appended (no bad test) and holds no point; a bad covisible is passed over
        pair.set_covisibles(3, [8, 12345, 9])
        assert pair.local_map(q, []) == ""
        got = pair.dev.local_map(q, [])
        assert got["kf_ids"].tolist() == [2, 3, 5] and got["point_ids"].tolist() == [BIG + 2, BIG + 3]
        pair.set_parent(2, -1)
        assert pair.local_map(q, []) == "" and pair.dev.local_map(q, [])["kf_ids"].tolist() == [2, 3, 9, 7, 6]
        assert pair.local_map([BIG + 5], [2, 5, 999]) == ""  # only a bad row holds... nothing: no vote, the previous list
        got = pair.dev.local_map([BIG + 5], [2, 5, 999])
        assert got["kept_previous"] == 1 and got["n_unknown_previous"] == 1 and got["kf_ids"].tolist() == [2, 5]
    finally:
        pair.close()


def test_small_capacities_still_report_the_full_counts(F):
    pair, pm = make(F)
    try:
        planted(pm, 21, 30, 60)
        rng = np.random.default_rng(5)
        frame = M.random_frame(rng, pm, n=60)
        kp = pm.frame_kp_ids(frame)
        full = pair.model.local_map(kp, [])
        assert full["n_kfs"] > 3 and full["n_points"] > 10
        for caps in ((0, 0), (1, 1), (3, 10), (full["n_kfs"], full["n_points"]), (full["n_kfs"] + 5, full["n_points"] + 5)):
            assert pair.local_map(kp, [], *caps) == "", caps
        kf = max(pm.kfs.values(), key=lambda k: len(pair.model.connections(k.mnId, 1)["ids"]))
        assert pair.model.connections(kf.mnId, 1)["n"] >= 3
        for caps in ((0, 0), (1, 2), (2, 1), (100, 100)):
            assert pair.connections(kf.mnId, 1, *caps) == "", caps
    finally:
        pair.close()


def test_growth_carries_the_state_and_clear_frees_ids_rows_and_pool(F):
    pair, pm = make(F, initial_rows=2, initial_slots=8)
    try:
        pts = planted(pm, 31, 3, 20)
        rng = np.random.default_rng(6)
        all_queries(pair, pm, rng, n_frames=2)
        planted(pm, 32, 40, 50, first_kf=1000, first_mp=BIG + 10 ** 6)  # rows 2 -> 64, the pool far past 8 slots
        pm.AddObservations(pm.kfs[1000 + 2 * 3], [(0, pts[0]), (5, pts[1])])  # old points in new rows
        all_queries(pair, pm, rng, n_frames=3)
        assert pair.clear() == ""
        pm = M.PointerMap(pair)
        assert pair.local_map([BIG], [1, 3]) == "" and pair.connections(1, 1) == ""
        planted(pm, 33, 10, 20)  # the same ids again
        all_queries(pair, pm, rng, n_frames=2)
    finally:
        pair.close()


def test_refusals_on_a_filled_graph_change_nothing(F, gpu):
    g = gpu.CovisibilityGraph(initial_rows=2, initial_slots=8)
    try:
        g.add_keyframe(1, 3, [10, 11, -1])
        g.add_keyframe(2, 3, [10, -1, 12])
        g.set_bad([2])
        before = g.local_map([10, 11], [])
        for call, text in ((lambda: g.add_keyframe(1, 3), "key frame 1 is in the graph"),
                           (lambda: g.add_keyframe(2, 3), "key frame 2 is in the graph"),
                           (lambda: g.set_slots([1, 1], [0, 3], [20, 21]), "slot 3 outside key frame 1 (3 slots, entry 1)"),
                           (lambda: g.set_slots([1, 2], [0, -1], [20, 21]), "slot -1 outside key frame 2")):
            with pytest.raises(gpu.OrbGpuError) as ei:
                call()
            assert ei.value.status == gpu.EINVAL and text in str(ei.value), str(ei.value)
        after = g.local_map([10, 11], [])
        assert g.size() == (1, 1) and all(np.array_equal(before[k], after[k]) for k in before)
        assert after["kf_ids"].tolist() == [1] and after["point_ids"].tolist() == [10, 11]
        assert g.set_slots([2, 1, 1], [0, 2, 2], [50, 51, 52]) == 3  # the bad row keeps no slot; the later entry wins
        assert g.local_map([50, 51, 52], [])["kf_ids"].tolist() == [1] and g.local_map([50, 51], [], 9, 9)["n_voted"] == 0
    finally:
        g.close()


def test_the_same_calls_on_fresh_handles_give_the_same_bytes(F):
    outs = []
    for _ in range(2):
        pair, pm = make(F)
        try:
            planted(pm, 41, 50, 400)
            rng = np.random.default_rng(7)
            parts = []
            for _ in range(4):
                got = pair.dev.local_map(pm.frame_kp_ids(M.random_frame(rng, pm, n=80)), [])
                parts += [got["kf_ids"].tobytes(), got["point_ids"].tobytes()]
            outs.append(b"".join(parts))
        finally:
            pair.close()
    assert outs[0] == outs[1] and len(outs[0]) > 1000
