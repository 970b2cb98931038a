"""tests/refresh_model.py, the definition of conventions R1-R8, against the CPU oracle's descriptor choice and against hand
cases whose answers are worked out here.  No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import refresh_model as RM  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32).tolist()


def desc_of(*ones):
    """one descriptor per argument, with that many leading one bits: the distance of two is the difference of their counts"""
    out = np.zeros((len(ones), 32), np.uint8)
    for r, k in enumerate(ones):
        b = np.zeros(256, np.uint8)
        b[:k] = 1
        out[r] = np.packbits(b)
    return out


def test_descriptor_choice_equals_the_oracle(oracle):
    rng = np.random.default_rng(5)
    g = RM.RefreshGraph()
    kf_ids, pts, pos, ref = RM.base_scene(rng, g)
    n_checked = 0
    for p in pts:
        obs = g.observations_of(p)
        group = np.stack([g.desc[k][j] for k, j in obs])
        assert RM.median_choice(group) == oracle.distinctive_descriptor(group), p
        n_checked += len(obs) > 2
    assert n_checked > 50
    for n in (1, 2, 3, 4, 7, 64, 65):  # random bits too: no ties
        group = rng.integers(0, 256, (n, 32)).astype(np.uint8)
        assert RM.median_choice(group) == oracle.distinctive_descriptor(group), n


def small(n_obs, kf_ids=(30, 20, 10), octaves=(0, 0, 0), n_levels=3):
    """point 7 at slot 1 of the first n_obs key frames of kf_ids (added in that order), each key frame with two slots"""
    g = RM.RefreshGraph()
    for i, k in enumerate(kf_ids):
        g.add_keyframe(k, 2, [-1, 7 if i < n_obs else -1])
        g.set_keypoints(k, [0, octaves[i]])
    g.set_scale_factors(np.float32(1.2) ** np.arange(n_levels, dtype=np.float32))
    return g


def test_one_two_and_three_observations():
    d = desc_of(0, 8, 24)  # distances: 0-1: 8, 1-2: 16, 0-2: 24
    for n_obs, want_kf in ((1, 30), (2, 20), (3, 20)):
        g = small(n_obs)
        for i, k in enumerate((30, 20, 10)):
            g.set_descriptors(k, np.stack([d[2], d[i]]))
        g.set_centres([30, 20, 10], [[0, 0, 0], [1, 0, 0], [0, 1, 0]])
        out = g.refresh([7], [30], [[0, 0, 2]])
        # N = 1: itself.  N = 2: rows (20, 30) in id order, the median index is 0, both medians are 0, the first (20) wins.
        # N = 3: order (10, 20, 30) = (d2, d1, d0); medians 16 (d2), 8 (d1), 8... d0: {0, 8, 24} -> 8; the first minimum is 20.
        assert out["status"].tolist() == [0] and out["n_slots"].tolist() == [n_obs]
        assert out["desc_kf"].tolist() == [want_kf] and out["desc_idx"].tolist() == [1]
        assert out["desc"][0].tolist() == d[(30, 20, 10).index(want_kf)].tolist()
        assert (out["n_descriptors"], out["n_normals"], out["n_entries"], out["max_obs"]) == (1, 1, n_obs, n_obs)
    # the normal of N = 1 from the centre (0, 0, 0) to (0, 0, 2) is (0, 0, 1) exactly; depth 2 at octave 0 of 3 levels
    g = small(1)
    g.set_centres([30], [[0, 0, 0]])
    out = g.refresh([7], [30], [[0, 0, 2]], RM.NORMAL_DEPTH)
    assert out["normal"].tolist() == [[0.0, 0.0, 1.0]] and out["status"].tolist() == [0]
    sf = np.float32(1.2) ** np.arange(3, dtype=np.float32)
    assert bits(out["max_dist"]) == bits([2.0]) and bits(out["min_dist"]) == bits([np.float32(np.float32(2.0) / sf[2])])
    assert out["desc_kf"].tolist() == [-1] and not out["desc"].any()


def test_two_equal_medians_the_first_in_id_then_index_order_wins():
    # four observations, two in one row (V2's deviation): order (10, 0), (10, 1), (20, 1), (30, 1) whatever the add order
    g = RM.RefreshGraph()
    g.add_keyframe(30, 2, [-1, 7])
    g.add_keyframe(10, 2, [7, 7])
    g.add_keyframe(20, 2, [-1, 7])
    a, b = desc_of(0, 8)
    g.set_descriptors(30, np.stack([a, a]))
    g.set_descriptors(10, np.stack([b, a]))
    g.set_descriptors(20, np.stack([b, b]))
    assert g.observations_of(7) == [(10, 0), (10, 1), (20, 1), (30, 1)]
    # group (b, a, b, a): every distance row sorts to (0, 0, 8, 8), median index 1 -> all medians 0: the first entry wins
    out = g.refresh([7], [10], [[1, 2, 3]], RM.DESCRIPTOR)
    assert (out["desc_kf"].tolist(), out["desc_idx"].tolist(), out["n_slots"].tolist()) == ([10], [0], [4])
    assert out["desc"][0].tolist() == b.tolist()


def test_rows_added_in_descending_id_are_observed_in_ascending_id():
    g = small(3)
    assert [r.id for r in g.rows] == [30, 20, 10] and g.observations_of(7) == [(10, 1), (20, 1), (30, 1)]
    # R5's sum goes by id, not by row: the point at the origin, one centre at (-1, 0, 0) -- its term is (1, 0, 0) -- and two at
    # (-2^-23, -2, 0) and (-2^-23, 0, -2): d = (2^-23, 2, 0), nrm = 2 (1 + 2^-49) in FP64, inv rounds to 0.5, so their x terms are
    # 2^-24 each.  1 + 2^-24 is a tie that rounds to even, 1, and again; 2^-24 + 2^-24 + 1 is 1 + 2^-23 exactly.
    big, small1, small2 = [-1.0, 0.0, 0.0], [-2.0 ** -23, -2.0, 0.0], [-2.0 ** -23, 0.0, -2.0]
    third = np.float32(np.float64(1.0) / np.float64(3.0))
    got = {}
    for name, centres in (("the large term first", {10: big, 20: small1, 30: small2}), ("the large term last", {10: small1, 20: small2, 30: big})):
        g = small(3)  # rows 30, 20, 10 in both: only the ids' order decides
        g.set_centres(list(centres), list(centres.values()))
        out = g.refresh([7], [30], [[0, 0, 0]], RM.NORMAL_DEPTH)
        assert out["status"].tolist() == [0], name
        got[name] = out["normal"][0]
    assert bits(got["the large term first"]) == bits([np.float32(1.0) * third, np.float32(1.0) * third, np.float32(1.0) * third])
    last = np.float32(np.float32(1.0 + 2.0 ** -23) * third)
    assert bits(got["the large term last"]) == bits([last, np.float32(1.0) * third, np.float32(1.0) * third])
    assert bits(got["the large term first"])[0] != bits(got["the large term last"])[0]


def test_reference_octave_zero_and_top_level_and_beyond():
    for octave, n_levels, ok in ((0, 3, True), (2, 3, True), (3, 3, False), (15, 16, True)):
        g = small(3, octaves=(octave, 1, 1), n_levels=n_levels)
        g.set_centres([30, 20, 10], [[0, 0, 0], [1, 0, 0], [0, 1, 0]])
        out = g.refresh([7], [30], [[0, 3, 4]], RM.NORMAL_DEPTH, initial=dict(min_dist=[9.0], max_dist=[8.0], normal=[[1, 2, 3]]))
        if not ok:
            assert out["status"].tolist() == [RM.NO_REF] and out["n_no_ref"] == 1 and out["n_normals"] == 0
            assert (out["min_dist"].tolist(), out["max_dist"].tolist(), out["normal"].tolist()) == ([9.0], [8.0], [[1, 2, 3]])
            continue
        sf = np.float32(1.2) ** np.arange(n_levels, dtype=np.float32)
        mx = np.float32(np.float32(5.0) * sf[octave])  # |(0, 3, 4)| = 5 exactly
        assert out["status"].tolist() == [0]
        assert bits(out["max_dist"]) == bits([mx]) and bits(out["min_dist"]) == bits([np.float32(mx / sf[n_levels - 1])])


def test_status_bits_are_independent_and_untouched_means_untouched():
    g = small(2)
    g.set_descriptors(30, np.full((2, 32), 3, np.uint8))
    g.set_centres([30, 20], [[0, 0, 0], [1, 1, 1]])
    init = dict(desc=np.full((3, 32), 0xAB, np.uint8), normal=np.full((3, 3), 7.0), min_dist=[1, 2, 3], max_dist=[4, 5, 6])
    out = g.refresh([7, 8, 9], [30, 30, 30], np.ones((3, 3)) * 4, initial=init)
    assert out["status"].tolist() == [RM.NO_DESC, RM.NO_OBS, RM.NO_OBS]  # key frame 20 has no descriptors; the normal runs
    assert out["desc"].tolist() == init["desc"].tolist() and out["normal"][1:].tolist() == [[7.0] * 3] * 2
    assert out["normal"][0].tolist() != [7.0] * 3 and (out["n_normals"], out["n_descriptors"], out["n_no_obs"]) == (1, 0, 2)
    g.set_descriptors(20, np.full((2, 32), 5, np.uint8))
    g.add_keyframe(40, 1, [7])  # no centre, no descriptors
    g.set_descriptors(40, np.full((1, 32), 5, np.uint8))
    out = g.refresh([7], [77], [[4, 4, 4]], initial=dict(normal=[[7, 7, 7]]))
    assert out["status"].tolist() == [RM.NO_CENTRE | RM.NO_REF] and out["normal"].tolist() == [[7.0] * 3]
    assert out["desc_kf"].tolist() == [20] and out["n_descriptors"] == 1  # medians (3: 2|.., 5: 0, 5: 0): the first 5 is key frame 20
    g.set_bad([20])
    assert g.observations_of(7) == [(30, 1), (40, 0)]
    for bad_call in (lambda: g.refresh([7, 7], [1, 1], np.zeros((2, 3))), lambda: g.refresh([-1], [1], np.zeros((1, 3))),
                     lambda: g.refresh([7], [1], np.zeros((1, 3)), 0), lambda: g.refresh([7], [1], np.zeros((1, 3)), 4)):
        with pytest.raises(RM.Refused):
            bad_call()


def test_the_models_constants_are_the_headers():
    import re
    header = open(os.path.join(os.path.dirname(HERE), "include", "orbgpu.h")).read()
    for name, value in (("REFRESH_DESCRIPTOR", RM.DESCRIPTOR), ("REFRESH_NORMAL_DEPTH", RM.NORMAL_DEPTH), ("REFRESH_NO_OBS", RM.NO_OBS),
                        ("REFRESH_OVERFLOW", RM.OVERFLOW), ("REFRESH_NO_DESC", RM.NO_DESC), ("REFRESH_NO_CENTRE", RM.NO_CENTRE),
                        ("REFRESH_NO_REF", RM.NO_REF), ("REFRESH_UNKNOWN", RM.UNKNOWN), ("REFRESH_BAD", RM.BAD),
                        ("COVIS_REFRESH_MAX_OBS", RM.MAX_OBS)):
        m = re.search(r"#define ORBGPU_%s (\S+)" % name, header)
        assert m and int(m.group(1), 0) == value, name


def test_overflow_keeps_the_count_exact():
    g = RM.RefreshGraph()
    for k in range(17):
        g.add_keyframe(k, 64, [7] * (64 if k < 16 else 1) + [-1] * (0 if k < 16 else 63))
    out = g.refresh([7], [0], [[1, 1, 1]])
    assert out["status"].tolist() == [RM.OVERFLOW] and out["n_slots"].tolist() == [1025] and out["max_obs"] == 1025 and out["n_entries"] == 0
