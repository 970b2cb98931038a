"""orbgpu_covis_keyframe_culling, orbgpu_covis_observations and orbgpu_covis_graph_set_keypoints on the device against
tests/cull_model.py: exact equality of every output.  Every graph starts with initial_rows = 2 and a pool of
8 slots, so rows, both pool columns and the hash grow in every test; maps hold at most 60 key frames and 300 points."""
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
import cull_model as CM  # noqa: E402

pytestmark = pytest.mark.gpu
BIG = 2 ** 33


@pytest.fixture(scope="module")
def F(gpu):
    import fuzz_cull
    return fuzz_cull


def make(F, mono=False):
    pair = F.CullPair(initial_rows=2, initial_slots=8)
    return pair, CM.CullPointerMap(pair, mbMonocular=mono)


def planted(pm, seed, n_kf=30, n_pts=150, first_kf=BIG + 1, keypoints=True):
    """key frames of 0, 1, 63, 64, 65 and 130 slots (ids above 2^32) over shared points (ids above 2^32), octaves 0-7 and 15,
    mixed STEREO and FAR flags; the rows of `keypoints=False` never get set_keypoints"""
    rng = np.random.default_rng(seed)
    pts = [pm.NewMapPoint(BIG + 3 * i) for i in range(n_pts)]
    kfs = []
    for i in range(n_kf):
        n = M.SLOT_SIZES[i % len(M.SLOT_SIZES)]
        if keypoints:
            octave = rng.choice(CM.OCTAVES[:3] if i % 3 else CM.OCTAVES, size=n)
            stereo = rng.random(n) < (0.0, 0.5, 1.0, 1.0, 0.5)[i % 5]
            depth = np.where(stereo, rng.uniform(0.5, 55.0, n), -1.0)
            kf = pm.AddKeyFrame(first_kf + 2 * i, n, octave, np.where(stereo, 100.0, -1.0), depth, 40.0)
        else:
            kf = M.PointerMap.AddKeyFrame(pm, first_kf + 2 * i, n)  # no constructor hook: the column keeps its default
            kf.octave, kf.mvuRight, kf.mvDepth, kf.mThDepth, kf.mbNotErase = [0] * n, [-1.0] * n, [1.0] * n, 40.0, False
        # four slots in five hold one of the first third of the points (seen by many: redundant), the others one of the
        # rest (seen by few: the points a culled key frame takes with it)
        take = rng.permutation(n)[:int(n * rng.uniform(0.5, 1.0))]
        n_common = min(int(0.8 * len(take)), n_pts // 3)
        chosen = list(rng.permutation(n_pts // 3)[:n_common]) + list(n_pts // 3 + rng.permutation(n_pts - n_pts // 3)[:len(take) - n_common])
        pm.AddObservations(kf, [(int(a), pts[int(b)]) for a, b in zip(take, chosen)])
        kfs.append(kf)
    return kfs, pts


def snapshot(pair, pm):
    """what the queries of V6 / V7 answer, for "the call leaves the graph unchanged" """
    probe = [p.mnId for p in list(pm.mps.values())[:40]]
    lm = pair.dev.local_map(probe, [])
    con = [pair.dev.connections(k, 1) for k in list(pm.kfs)[:6]]
    flat = lambda d: {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in d.items()}  # noqa: E731
    return pair.dev.size(), flat(lm), [flat(c) for c in con]


@pytest.mark.parametrize("n_cand", [0, 1, 30])
def test_candidate_counts_and_an_unchanged_graph(F, n_cand):
    pair, pm = make(F)
    try:
        kfs, pts = planted(pm, 11 + n_cand)
        rng = np.random.default_rng(n_cand)
        ids = [kfs[int(i)].mnId for i in rng.permutation(len(kfs))[:n_cand]]
        before = snapshot(pair, pm)
        for th in (3, 1):
            assert pair.keyframe_culling(ids, None, th) == ""
        assert pair.keyframe_culling(ids, [int(i % 3 == 0) for i in range(len(ids))]) == ""
        assert snapshot(pair, pm) == before and pair.size() == ""
        if n_cand == 30:
            res = pair.model.keyframe_culling(ids)
            assert res["n_culled"] > 0 and res["n_points_bad"] > 2 and res["n_query_points"] > 100, "the map has nothing to cull"
            for cap in (0, 2):  # point_capacity 0 and smaller than the count
                assert pair.keyframe_culling(ids, None, 3, cap) == ""
                assert pair.dev.keyframe_culling(ids, None, 3, cap)["n_points_bad"] == res["n_points_bad"]
    finally:
        pair.close()


def test_skipped_candidates_and_not_erase(F):
    pair, pm = make(F)
    try:
        kfs, _ = planted(pm, 5, n_kf=24)
        pm.AddKeyFrame(0, 64, [0] * 64, [100.0] * 64, [1.0] * 64)  # id 0 holds what key frame 5 holds, and is skipped all the same
        pm.AddObservations(pm.kfs[0], list(enumerate([mp for mp in kfs[5].mvpMapPoints if mp is not None][:64])))
        pm.SetBadFlagKeyFrame(kfs[3])
        live = [k.mnId for k in kfs if not k.mbBad]
        ids = [0, live[0], 10 ** 12, kfs[3].mnId, live[1], live[0], live[2], live[1]] + live[3:]
        ne = [0, 0, 0, 0, 1, 0, 0, 1] + [int(i % 4 == 1) for i in range(len(live) - 3)]
        culled = [k for k, v in zip(ids, pair.model.keyframe_culling(ids, ne)["verdict"]) if v == 1]
        assert len(culled) >= 2, "the map has nothing to cull"
        ne = [1 if k == culled[1] else f for k, f in zip(ids, ne)]  # mbNotErase on one that would go
        assert pair.keyframe_culling(ids, ne) == ""
        res = pair.dev.keyframe_culling(ids, ne)
        assert res["verdict"][[0, 2, 3]].tolist() == [-1, -1, -1] and res["n_skipped"] >= 3
        assert set(res["verdict"].tolist()) == {-1, 0, 1, 2}, "the list does not reach every verdict"
        assert res["verdict"][5] == (-1 if res["verdict"][1] == 1 else res["verdict"][1])  # a culled id that occurs again is skipped
    finally:
        pair.close()


def test_rows_without_keypoints_and_the_global_memory_query(F, monkeypatch):
    monkeypatch.setenv("ORBGPU_DEBUG_COVIS_LDS_IDS", "8")
    pair, pm = make(F, mono=True)
    try:
        kfs, pts = planted(pm, 8, n_kf=18, n_pts=90, keypoints=False)
        ids = [k.mnId for k in kfs]
        before = pair.dev.debug_global_queries()
        assert pair.keyframe_culling(ids, None, 3, len(pts)) == ""  # (a given capacity: one call)
        assert pair.observations([p.mnId for p in pts[:20]]) == ""
        assert pair.dev.debug_global_queries() == before + 2
        assert pair.observations([pts[0].mnId]) == "" and pair.dev.debug_global_queries() == before + 2  # 1 id: through LDS
        assert pair.model.keyframe_culling(ids)["n_culled"] > 0
    finally:
        pair.close()


def test_refusals_that_need_a_row_change_nothing(F):
    import ctypes as C
    from orb_slam2_map_amd import lib as G
    pair, pm = make(F)
    try:
        kfs, pts = planted(pm, 51, n_kf=12)
        kf = kfs[2]  # 63 slots
        ids = [k.mnId for k in kfs]
        for kp, text in (([0] * 62, "n_slots = 62"), ([0] * 64, "n_slots = 64"), ([0] * 62 + [0x10], "0x10 at slot 62"),
                         ([0x20] + [0] * 62, "0x20 at slot 0"), ([0xB5] + [0] * 62, "0xb5 at slot 0")):
            with pytest.raises(G.OrbGpuError) as ei:
                pair.dev.set_keypoints(kf.mnId, kp)
            assert ei.value.status == G.EINVAL and text in str(ei.value), str(ei.value)
            with pytest.raises(CM.Refused):
                pair.model.set_keypoints(kf.mnId, kp)
        assert G.lib().orbgpu_covis_graph_set_keypoints(pair.dev.h, C.c_int64(kf.mnId), 63, None) == G.EINVAL
        assert pair.keyframe_culling(ids) == "" and pair.observations([p.mnId for p in pts]) == ""  # the column is what it was
        pair.set_keypoints(kfs[0].mnId, [])  # a row of no slots
        pm.SetBadFlagKeyFrame(kf)
        pair.set_keypoints(kf.mnId, [CM.KP_FAR] * 63)  # a bad row ignores the call ...
        with pytest.raises(G.OrbGpuError):
            pair.dev.set_keypoints(kf.mnId, [0] * 5)  # ... but not a wrong length
        assert pair.keyframe_culling(ids) == ""
    finally:
        pair.close()


def test_observations(F):
    pair, pm = make(F)
    try:
        assert pair.observations([]) == "" and pair.observations([-1, 7]) == ""  # an empty graph
        kfs, pts = planted(pm, 21, n_kf=20, n_pts=80)
        ask = [pts[3].mnId, -1, pts[3].mnId, 10 ** 15, 5] + [p.mnId for p in pts]
        assert pair.observations(ask) == ""
        obs, cnt = pair.dev.observations(ask)
        assert obs[0] == obs[2] == pts[3].nObs and cnt[0] == len(pts[3].mObservations) and obs[0] > cnt[0] > 0  # stereo weighs 2
        assert obs[[1, 3, 4]].tolist() == [0, 0, 0] and cnt[[1, 3, 4]].tolist() == [0, 0, 0]
        assert obs[5:].tolist() == [p.nObs for p in pts]
        pm.SetBadFlagKeyFrame(kfs[4])
        assert pair.observations(ask) == ""
    finally:
        pair.close()


def test_after_set_bad_clear_and_re_adding(F):
    pair, pm = make(F)
    try:
        kfs, _ = planted(pm, 31, n_kf=20)
        for k in (kfs[2], kfs[9]):
            pm.SetBadFlagKeyFrame(k)
        ids = [k.mnId for k in kfs]
        assert pair.keyframe_culling(ids) == "" and pair.model.size()[1] == 2
        assert pair.clear() == ""
        assert pair.keyframe_culling(ids) == "" and pair.observations([BIG, BIG + 3]) == ""  # nothing is a row: all skipped
        pm = CM.CullPointerMap(pair, mbMonocular=False)
        kfs, _ = planted(pm, 32, n_kf=20)  # the same ids again, other slots and attributes
        assert pair.keyframe_culling([k.mnId for k in kfs], [int(i % 5 == 0) for i in range(20)]) == ""
    finally:
        pair.close()


def test_hand_case_a_sequence_matters(F):
    pair, pm = make(F, mono=True)
    try:
        pts = [pm.NewMapPoint(100 + i) for i in range(10)]
        for k in (1, 2, 3, 4):
            pm.AddObservations(pm.AddKeyFrame(k, 10), list(enumerate(pts)))
        assert pair.keyframe_culling([1, 2, 3]) == ""
        res = pair.dev.keyframe_culling([1, 2, 3])
        assert res["verdict"].tolist() == [1, 0, 0] and res["n_mps"].tolist() == [10] * 3 and res["n_redundant"].tolist() == [10, 0, 0]
        assert pair.model.keyframe_culling([1, 2, 3], order_free=True)["verdict"].tolist() == [1, 1, 1]
    finally:
        pair.close()


def test_hand_case_d_cascade(F):
    pair, pm = make(F, mono=True)
    try:
        X, a, b = 999, list(range(100, 110)), list(range(200, 209))
        for p in [X] + a + b:
            pm.NewMapPoint(p)
        for k, held in ((1, [X] + a), (2, [X] + b), (8, [X]), (5, a + b), (6, a + b), (7, a + b)):
            pm.AddObservations(pm.AddKeyFrame(k, len(held)), [(i, pm.mps[p]) for i, p in enumerate(held)])
        assert pair.keyframe_culling([1, 2]) == "" and pair.keyframe_culling([1, 2], [1, 0]) == ""
        res = pair.dev.keyframe_culling([1, 2])
        assert res["verdict"].tolist() == [1, 1] and res["n_mps"].tolist() == [11, 9] and res["bad_point_ids"].tolist() == [X]
        assert pair.dev.keyframe_culling([1, 2], [1, 0])["verdict"].tolist() == [2, 0]
    finally:
        pair.close()


def test_chain_culling_hooks_and_a_second_culling(F):
    """the culling, then KeyFrame::SetBadFlag on every verdict 1 through the hooks into the device graph, then a second
    culling and a local map on the device: all equal the model, and the points the pointer map turned bad are the reported
    bad_point_ids"""
    pair, pm = make(F)
    try:
        kfs, pts = planted(pm, 41, n_kf=36, n_pts=200)
        ids = [k.mnId for k in kfs[::-1]]
        assert pair.keyframe_culling(ids) == ""
        res = pair.dev.keyframe_culling(ids)
        assert res["n_culled"] >= 2 and res["n_points_bad"] >= 1
        want = pair.model.predicted(ids, res)
        bad_before = {p.mnId for p in pts if p.mbBad}
        for k, v in zip(ids, res["verdict"]):
            if v == 1:
                pm.SetBadFlagKeyFrame(pm.kfs[k])
        assert sorted({p.mnId for p in pts if p.mbBad} - bad_before) == res["bad_point_ids"].tolist()
        assert pair.model.state() == want and pair.size() == ""
        assert pair.keyframe_culling(ids) == "" and pair.keyframe_culling(ids[::-1], None, 2) == ""
        assert pair.local_map([p.mnId for p in pts if not p.mbBad][:60], []) == ""
        assert pair.observations([p.mnId for p in pts]) == ""
    finally:
        pair.close()
