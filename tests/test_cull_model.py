"""tests/cull_model.py: convention V8 (CullGraph) against LocalMapping::KeyFrameCulling restated over the reference's
pointer graph (CullPointerMap) on random maps, the state V8 predicts against the state the reference's hooks produce, and
hand cases with exact numbers.  No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import cull_model as CM  # noqa: E402


def build(mono=True):
    g = CM.CullGraph()
    return g, CM.CullPointerMap(g, mbMonocular=mono)


def plant(pm, kf_id, points, octaves=None, stereo=None, depth=None, n=None):
    """a key frame that holds points[i] at slot i"""
    n = len(points) if n is None else n
    octaves = [0] * n if octaves is None else octaves
    stereo = [False] * n if stereo is None else stereo
    depth = [1.0 if s else -1.0 for s in stereo] if depth is None else depth
    kf = pm.AddKeyFrame(kf_id, n, octaves, [100.0 if s else -1.0 for s in stereo], depth, 40.0)
    pm.AddObservations(kf, [(i, pm.mps[p] if p in pm.mps else pm.NewMapPoint(p)) for i, p in enumerate(points) if p >= 0])
    return kf


def cull_both(g, pm, ids, not_erase=None, th=3):
    """V8 on the table, then the reference's loop on the pointer graph (which edits the table through its hooks)"""
    res = g.keyframe_culling(ids, not_erase, th)
    want_state = g.predicted(ids, res)
    for k, keep in zip(ids, not_erase or [0] * len(ids)):
        if k in pm.kfs:
            pm.kfs[k].mbNotErase = bool(keep)
    out, bad = pm.KeyFrameCulling([pm.kfs.get(k) for k in ids], th)
    assert [o[0] for o in out] == res["verdict"].tolist()
    assert [o[1] for o in out] == res["n_mps"].tolist()
    assert [o[2] for o in out] == res["n_redundant"].tolist()
    assert bad == res["bad_point_ids"].tolist() and res["n_points_bad"] == len(bad)
    assert g.state() == want_state  # the hooks brought the graph to the state the call predicted
    return res


@pytest.mark.parametrize("seed", range(12))
def test_v8_equals_the_reference_loop_on_random_maps(seed):
    rng = np.random.default_rng(seed)
    culled = 0
    for mono in (True, False):
        g, pm = build(mono)
        kfs = CM.random_map(rng, pm, n_kf=int(rng.integers(4, 16)), n_pts=int(rng.integers(20, 90)))
        for _ in range(3):  # the second and third call run on a map the first one has culled
            ids, ne = CM.random_candidates(rng, kfs)
            before = g.state()
            res = g.keyframe_culling(ids, ne, int(rng.choice([1, 2, 3, 3, 5])))
            assert g.state() == before  # V8 does not modify the graph
            culled += res["n_culled"]
            cull_both(g, pm, ids, ne, 3)
            obs, cnt = g.observations([p.mnId for p in pm.mps.values()] + [-1, 10 ** 15])
            assert obs.tolist() == [p.nObs if not p.mbBad else 0 for p in pm.mps.values()] + [0, 0]
            assert cnt.tolist() == [len(p.mObservations) for p in pm.mps.values()] + [0, 0]
    assert culled >= 0


def test_random_maps_cull_something():
    """the comparison above is not vacuous: over the seeds it sees every verdict and some bad points"""
    seen, bad = set(), 0
    for seed in range(12):
        rng = np.random.default_rng(seed)
        g, pm = build(seed % 2 == 0)
        kfs = CM.random_map(rng, pm, n_kf=12, n_pts=40)
        ids, ne = CM.random_candidates(rng, kfs, n=10)
        res = g.keyframe_culling(ids, ne)
        seen |= set(res["verdict"].tolist())
        bad += res["n_points_bad"]
    assert seen == {-1, 0, 1, 2} and bad > 0


def test_a_sequence_matters():
    g, pm = build()
    pts = list(range(100, 110))
    for k in (1, 2, 3, 4):
        plant(pm, k, pts)
    free = g.keyframe_culling([1, 2, 3], order_free=True)
    assert free["verdict"].tolist() == [1, 1, 1]  # an order-free evaluation would cull all three
    res = cull_both(g, pm, [1, 2, 3])
    assert res["verdict"].tolist() == [1, 0, 0]  # 1: Obs 4 > 3, others 3; then Obs is 3
    assert res["n_mps"].tolist() == [10, 10, 10] and res["n_redundant"].tolist() == [10, 0, 0]
    assert (res["n_culled"], res["n_to_be_erased"], res["n_skipped"], res["n_points_bad"], res["n_query_points"]) == (1, 0, 0, 0, 10)


def test_b_scale_rule():
    for others_octave, verdict, red in ((4, 0, 0), (3, 1, 10)):  # s + 2 does not count, s + 1 does
        g, pm = build()
        pts = list(range(10))
        plant(pm, 1, pts, octaves=[2] * 10)
        for k in (2, 3, 4):
            plant(pm, k, pts, octaves=[others_octave] * 10)
        res = cull_both(g, pm, [1])
        assert (res["verdict"].tolist(), res["n_mps"].tolist(), res["n_redundant"].tolist()) == ([verdict], [10], [red])
    g, pm = build()  # octave 15: the window ends at the last level
    plant(pm, 1, [5], octaves=[15])
    for k in (2, 3, 4):
        plant(pm, k, [5], octaves=[15])
    assert cull_both(g, pm, [1])["verdict"].tolist() == [1]


def test_c_stereo_weights():
    g, pm = build(mono=False)
    pts = list(range(10))
    plant(pm, 1, pts, stereo=[True] * 10)
    plant(pm, 2, pts, stereo=[True] * 10)
    obs, cnt = g.observations(pts)
    assert obs.tolist() == [4] * 10 and cnt.tolist() == [2] * 10  # Obs 4 > 3 ...
    res = cull_both(g, pm, [1])
    assert (res["verdict"].tolist(), res["n_mps"].tolist(), res["n_redundant"].tolist()) == ([0], [10], [0])  # ... but others 1


def cascade_map():
    """Point X is held by key frames 1, 2 and 8 (Obs 3, so it is redundant nowhere).  Key frame 1 also holds ten points
    that 5, 6, 7 hold: 10 of 11, culled.  Key frame 2 also holds nine points that 5, 6, 7 hold: 9 of 10 is not culled, but
    once 1 has gone X has Obs 2 and is bad, and 9 of 9 is."""
    g, pm = build()
    X = 999
    a, b = list(range(100, 110)), list(range(200, 209))
    plant(pm, 1, [X] + a)
    plant(pm, 2, [X] + b)
    plant(pm, 8, [X])
    for k in (5, 6, 7):
        plant(pm, k, a + b)
    return g, pm, X


def test_d_cascade():
    g, pm, X = cascade_map()
    assert g.observations([X])[0].tolist() == [3]
    alone = g.keyframe_culling([2])
    assert (alone["verdict"].tolist(), alone["n_mps"].tolist(), alone["n_redundant"].tolist()) == ([0], [10], [9])
    kept = g.keyframe_culling([1, 2], not_erase=[1, 0])  # 1 is only marked: X lives, 2 stays
    assert kept["verdict"].tolist() == [2, 0] and kept["n_mps"].tolist() == [11, 10] and kept["n_points_bad"] == 0
    res = cull_both(g, pm, [1, 2])  # 1 goes, X drops to Obs 2 and dies, 2 is left with 9 of 9
    assert res["verdict"].tolist() == [1, 1] and res["n_mps"].tolist() == [11, 9] and res["n_redundant"].tolist() == [10, 9]
    assert res["bad_point_ids"].tolist() == [X]
    g, pm, X = cascade_map()
    assert cull_both(g, pm, [1, 2], not_erase=[1, 0])["verdict"].tolist() == [2, 0]


def test_e_far_slots_id_zero_and_no_points():
    g, pm = build(mono=False)
    pts = list(range(10))
    # slots 0-4 close stereo, 5-7 stereo beyond mThDepth, 8-9 monocular (mvDepth < 0): FAR
    stereo = [True] * 8 + [False] * 2
    depth = [1.0] * 5 + [50.0] * 3 + [-1.0] * 2
    plant(pm, 0, pts, stereo=stereo, depth=depth)
    plant(pm, 1, pts, stereo=stereo, depth=depth)
    for k in (2, 3, 4):
        plant(pm, k, pts[5:], stereo=[True] * 5)  # only the FAR points are seen elsewhere
    plant(pm, 9, [-1, -1], n=2)
    assert [b & CM.KP_FAR for b in g.kp[1]] == [0] * 5 + [CM.KP_FAR] * 5
    res = cull_both(g, pm, [0, 1, 9, 77])
    assert res["verdict"].tolist() == [-1, 0, 0, -1]  # id 0; 5 close points, none redundant; n_mps == 0 is never culled; no row
    assert res["n_mps"].tolist() == [0, 5, 0, 0] and res["n_redundant"].tolist() == [0, 0, 0, 0]
    assert res["n_skipped"] == 2 and res["n_query_points"] == 10
    # the same key frame in monocular mode counts all ten slots
    g, pm = build(mono=True)
    plant(pm, 1, pts, stereo=stereo, depth=depth)
    assert g.keyframe_culling([1])["n_mps"].tolist() == [10]


@pytest.mark.parametrize("n_red,n_all,verdict", [(9, 10, 0), (10, 11, 1)])
def test_e_boundary_of_ninety_percent(n_red, n_all, verdict):
    g, pm = build()
    red, rest = list(range(n_red)), list(range(500, 500 + n_all - n_red))
    plant(pm, 1, red + rest)
    for k in (2, 3, 4):
        plant(pm, k, red)
    res = cull_both(g, pm, [1])
    assert (res["verdict"].tolist(), res["n_mps"].tolist(), res["n_redundant"].tolist()) == ([verdict], [n_all], [n_red])


def test_e_a_point_twice_in_one_row():
    """V2's deviation: the table can hold what MapPoint::AddObservation's guard excludes; every slot counts"""
    g = CM.CullGraph()
    g.add_keyframe(1, 3, [7, 7, -1])
    g.add_keyframe(2, 2, [7, 7])
    g.add_keyframe(3, 1, [7])
    assert [x.tolist() for x in g.observations([7, 7])] == [[5, 5], [5, 5]]
    res = g.keyframe_culling([1, 2, 3])
    # 1: both slots see 3 slots on other rows -> 2 of 2, culled; Obs 5 -> 3: not above th, nobody else goes
    assert res["verdict"].tolist() == [1, 0, 0] and res["n_mps"].tolist() == [2, 2, 1] and res["n_redundant"].tolist() == [2, 0, 0]
    g.set_keypoints(1, [CM.KP_STEREO, 0, 0])
    g.set_keypoints(3, [CM.KP_STEREO | 3])
    assert g.observations([7])[0].tolist() == [7]
    res = g.keyframe_culling([3, 2])  # 3 at octave 3 sees four slots at octave 0; 2 then has Obs 5, others 2
    assert res["verdict"].tolist() == [1, 0] and res["n_redundant"].tolist() == [1, 0]
    res = g.keyframe_culling([2, 1], th_obs=2)  # 2 leaves with both slots: Obs 7 -> 5; 1 then sees one other slot
    assert res["verdict"].tolist() == [1, 0] and res["bad_point_ids"].size == 0
    res = g.keyframe_culling([1, 3], th_obs=1)  # 1 leaves: Obs 7 - 3 = 4; 3 leaves: Obs 2, the point is bad
    assert res["verdict"].tolist() == [1, 1] and res["bad_point_ids"].tolist() == [7]


def test_refusals_of_the_model():
    g = CM.CullGraph()
    g.add_keyframe(1, 2, [4, 5])
    for call in (lambda: g.set_keypoints(2, [0, 0]), lambda: g.set_keypoints(1, [0]), lambda: g.set_keypoints(1, [0x10, 0]),
                 lambda: g.set_keypoints(1, [0, 0x20]), lambda: g.observations([4, -2]), lambda: g.keyframe_culling([-1]),
                 lambda: g.keyframe_culling([1], th_obs=0), lambda: g.keyframe_culling([1], th_obs=256),
                 lambda: g.keyframe_culling([1] * (2 ** 16 + 1))):
        with pytest.raises(CM.Refused):
            call()
    g.set_bad([1])
    g.set_keypoints(1, [CM.KP_FAR, 0])  # a bad row ignores the call
    assert g.kp[1] == [0, 0]
