"""tests/covis_model.py: the table model of the observation graph (V1-V7) against the literal pointer-graph restatement of
Tracking::UpdateLocalKeyFrames / UpdateLocalPoints and KeyFrame::UpdateConnections in the same file, on random consistent
maps driven through the hooks and on crafted cases.  No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import covis_model as M  # noqa: E402


def pair(**kw):
    g = M.CovisGraph()
    return g, M.PointerMap(g, **kw)


def same_local_map(g, pm, frame, prev_ids):
    kp = pm.frame_kp_ids(frame)
    got = g.local_map(kp, prev_ids)
    want = pm.UpdateLocalMap(frame)
    assert got["kf_ids"].tolist() == want["kf_ids"], (got["kf_ids"], want["kf_ids"])
    assert got["point_ids"].tolist() == want["point_ids"]
    for k in ("ref_kf", "max_votes", "n_voted", "kept_previous"):
        assert got[k] == want[k], k
    return got


def same_connections(g, pm, kf, th):
    got = g.connections(kf.mnId, th)
    counter, ordered, weights = pm.UpdateConnections(kf, th)
    assert list(zip(got["ids"].tolist(), got["counts"].tolist())) == counter
    assert got["ordered_ids"].tolist() == ordered and got["ordered_weights"].tolist() == weights
    return got


@pytest.mark.parametrize("seed", range(12))
def test_random_maps_through_the_hooks(seed):
    rng = np.random.default_rng(seed)
    g, pm = pair()
    next_ids = [int(rng.integers(0, 3)), int(rng.choice([0, 2 ** 33]))]
    ops, voted, kept = {}, 0, 0
    for step in range(260):
        op = M.random_edit(rng, pm, next_ids)
        ops[op] = ops.get(op, 0) + 1
        if step % 4 == 3:
            prev = [k.mnId for k in pm.mvpLocalKeyFrames]
            got = same_local_map(g, pm, M.random_frame(rng, pm), prev)
            voted += got["n_voted"] > 0
            kept += got["kept_previous"]
        if step % 7 == 6:
            alive = [k for k in pm.kfs.values() if not k.mbBad]
            same_connections(g, pm, alive[int(rng.integers(len(alive)))], int(rng.choice([1, 3, 15])))
    assert g.size() == (sum(1 for k in pm.kfs.values() if not k.mbBad), sum(1 for k in pm.kfs.values() if k.mbBad))
    for kf in pm.kfs.values():  # V2: one relation
        want = [-1] * kf.N if kf.mbBad else [-1 if m is None else m.mnId for m in kf.mvpMapPoints]
        assert g.row_of[kf.mnId].slots == want
        # V3 (a bad child keeps its parent value where the reference erases it from the set: no query lists a bad child)
        assert [c for c in g.children(kf.mnId) if not g.row_of[c].bad] == [c.mnId for c in kf.GetChilds()]
    assert voted >= 20 and len(ops) >= 6


def chain(n_kf, shared=True):
    """key frames 1..n_kf of 4 slots; point 100 + k in slot 0 of key frame k; point 99 in slot 1 of every one if `shared`"""
    g, pm = pair()
    common = pm.NewMapPoint(99)
    for k in range(1, n_kf + 1):
        kf = pm.AddKeyFrame(k, 4)
        pm.AddObservations(kf, [(0, pm.NewMapPoint(100 + k))] + ([(1, common)] if shared else []))
    return g, pm


def test_the_parent_break_leaves_the_outer_loop():
    """K1 = [A, B], A's parent P is not included: P is appended and B contributes nothing, although B has a covisible, a
    child and a parent of its own to offer."""
    g, pm = chain(8, shared=False)
    A, B, P = pm.kfs[2], pm.kfs[3], pm.kfs[5]
    A.mpParent = P
    P.mspChildrens.add(A)
    g.set_parent(2, 5)
    B.mpParent = pm.kfs[6]
    pm.kfs[6].mspChildrens.add(B)
    g.set_parent(3, 6)
    pm.kfs[7].mpParent = B
    B.mspChildrens.add(pm.kfs[7])
    g.set_parent(7, 3)
    B.mvpOrderedConnectedKeyFrames = [pm.kfs[8]]
    g.set_covisibles(3, [8])
    frame = [pm.mps[102], pm.mps[103], pm.mps[103]]
    got = same_local_map(g, pm, frame, [])
    assert got["kf_ids"].tolist() == [2, 3, 5] and got["ref_kf"] == 3 and got["max_votes"] == 2
    # with A's parent included beforehand (voted), B's turn comes: covisible 8, child 7, then parent 6
    got = same_local_map(g, pm, frame + [pm.mps[105]], [])
    assert got["kf_ids"].tolist() == [2, 3, 5, 8, 7, 6]


@pytest.mark.parametrize("n_voted,extended", [(80, True), (81, False)])
def test_eighty_voted_rows_extend_and_eighty_one_do_not(n_voted, extended):
    g, pm = chain(100)
    pm.kfs[1].mvpOrderedConnectedKeyFrames = [pm.kfs[100]]
    g.set_covisibles(1, [100])
    frame = [pm.mps[100 + k] for k in range(1, n_voted + 1)]
    got = same_local_map(g, pm, frame, [])
    assert got["n_voted"] == n_voted
    assert got["kf_ids"].tolist() == list(range(1, n_voted + 1)) + ([100] if extended else [])


def test_a_tie_for_the_reference_key_frame_goes_to_the_smaller_id():
    g, pm = chain(6, shared=False)
    got = same_local_map(g, pm, [pm.mps[104], pm.mps[102], pm.mps[104], pm.mps[102], pm.mps[105]], [])
    assert got["ref_kf"] == 2 and got["max_votes"] == 2 and got["kf_ids"].tolist() == [2, 4, 5]


def test_no_votes_keeps_the_previous_list_without_the_ids_that_are_gone():
    g, pm = chain(5)
    lonely = pm.NewMapPoint(7)
    got = g.local_map(pm.frame_kp_ids([lonely, None]), [4, 777, 2, 4])
    assert got["kept_previous"] == 1 and got["n_unknown_previous"] == 1 and got["kf_ids"].tolist() == [4, 2, 4]
    assert got["ref_kf"] == -1 and got["n_voted"] == 0 and got["point_ids"].tolist() == [104, 99, 102]
    pm.mvpLocalKeyFrames = [pm.kfs[4], pm.kfs[2]]
    got = same_local_map(g, pm, [lonely, None], [4, 2])
    assert got["kf_ids"].tolist() == [4, 2]
    g.clear()
    got = g.local_map([7], [4, 2])
    assert got["kept_previous"] == 1 and got["n_unknown_previous"] == 2 and got["n_kfs"] == 0 and got["n_points"] == 0


def test_no_row_at_the_threshold_gives_the_single_maximum_and_weight_ties_order_by_id():
    g, pm = pair()
    shared = [pm.NewMapPoint(i) for i in range(6)]
    for k, idxs in ((3, range(6)), (9, (0, 1)), (4, (2, 3)), (7, (4,)), (5, ())):
        kf = pm.AddKeyFrame(k, 8)
        pm.AddObservations(kf, [(i, shared[i]) for i in idxs])
    got = g.connections(3, th=15)
    assert got["ids"].tolist() == [4, 7, 9] and got["counts"].tolist() == [2, 1, 2]
    assert got["ordered_ids"].tolist() == [4] and got["ordered_weights"].tolist() == [2]  # first strictly greatest
    got = same_connections(g, pm, pm.kfs[3], 1)
    assert got["ordered_ids"].tolist() == [9, 4, 7] and got["ordered_weights"].tolist() == [2, 2, 1]  # descending (weight, id)
    assert g.connections(5, 1)["n"] == 0 and g.connections(12345, 1)["n"] == 0
    pm.SetBadFlagKeyFrame(pm.kfs[9])
    assert g.connections(9, 1)["n"] == 0 and g.connections(3, 1)["ids"].tolist() == [4, 7]


def test_one_point_at_two_key_points_votes_twice():
    g, pm = chain(3, shared=False)
    got = same_local_map(g, pm, [pm.mps[101], pm.mps[102], pm.mps[101], None], [])
    assert got["max_votes"] == 2 and got["ref_kf"] == 1 and got["kf_ids"].tolist() == [1, 2]
    # (V2) the same point in two slots of one ROW counts twice as well: only the hook can write that
    g.set_slots([2], [3], [102])
    assert g.local_map([102], [])["max_votes"] == 2


def test_a_bad_parent_is_appended_and_lists_no_points_where_the_reference_lists_its_stale_ones():
    for clear in (True, False):
        g, pm = pair(clear_bad_keyframe_slots=clear)
        pts = [pm.NewMapPoint(i) for i in range(10)]
        for k in (0, 1, 2, 3, 4):  # every point has five observers: erasing one leaves it good
            pm.AddObservations(pm.AddKeyFrame(k, 10), [(i, pts[i]) for i in range(10) if k != 4 or i < 2])
        pm.SetBadFlagKeyFrame(pm.kfs[3])
        # (the reference never points at a bad parent after SetBadFlag's re-parenting; a caller's hook order can)
        pm.kfs[4].mpParent = pm.kfs[3]
        g.set_parent(4, 3)
        only4 = pm.NewMapPoint(60)
        pm.AddObservations(pm.kfs[4], [(7, only4)])
        got = g.local_map([60], [])
        want = pm.UpdateLocalMap([only4])
        assert got["kf_ids"].tolist() == want["kf_ids"] == [4, 3]
        assert got["point_ids"].tolist() == [0, 1, 60]
        assert want["point_ids"] == ([0, 1, 60] if clear else [0, 1, 60, 2, 3, 4, 5, 6, 7, 8, 9])


def test_refusals_change_nothing():
    g, pm = chain(3)
    before = (g.local_map([99], [])["point_ids"].tolist(), g.size())
    for call in (lambda: g.add_keyframe(2, 4), lambda: g.add_keyframe(-1, 4), lambda: g.add_keyframe(9, M.MAX_SLOTS + 1),
                 lambda: g.add_keyframe(9, 2, [5, -2]), lambda: g.set_slots([1, 2], [0, 4], [5, 6]), lambda: g.set_slots([1], [0], [-2]),
                 lambda: g.set_covisibles(1, list(range(11))), lambda: g.set_covisibles(1, [-1]), lambda: g.set_parent(-1, 2),
                 lambda: g.set_parent(1, -2)):
        with pytest.raises(M.Refused):
            call()
    assert (g.local_map([99], [])["point_ids"].tolist(), g.size()) == before
    assert g.set_slots([1, 555], [0, 99], [5, 6]) == 1  # an unknown key frame: ignored, idx not looked at
