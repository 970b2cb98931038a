"""The oracle's rotation-consistency check against a second statement of the rule (rot_plan.py, written from
ORBmatcher.cc:238-243 and :1601-1642), on histograms planted into the scenes the GPU tests use: for every matcher with
the check and every named case, the oracle with the check on must equal rot_plan.keep_mask applied to what it
accepts with the check off.  Also shows that no case is vacuous: each one that should remove pairs does."""
import numpy as np
import pytest

import rot_plan as RP
import rot_scenes as S

SCENES = {"bf": lambda e: S.EmptyBFScene() if e else S.BFScene(400),
          "bow": lambda e: S.BowScene(S.HostSide(), empty=e),
          "bow_keyframes": lambda e: S.BowKeyFramesScene(S.HostSide(), empty=e),
          "last_frame": lambda e: S.LastFrameScene(S.HostSide(), empty=e),
          "keyframe": lambda e: S.KeyFrameScene(S.HostSide(), empty=e),
          "triangulation": lambda e: S.TriangulationScene(S.HostSide(), False, empty=e),
          "triangulation_stereo": lambda e: S.TriangulationScene(S.HostSide(), True, empty=e),
          "initialization": lambda e: S.InitializationScene(S.HostSide(), empty=e)}
_cache = {}


def scene(name, empty=False):
    if (name, empty) not in _cache:
        _cache[name, empty] = SCENES[name](empty)
    return _cache[name, empty]


# ---- the helper itself -----------------------------------------------------------------------------------------------
def test_rot_bin_edges():
    z = np.zeros(1, np.float32)
    b = lambda rot: int(RP.rot_bin(np.array([rot], np.float32), z)[0])
    assert [b(r) for r in (0.0, 14.75, 15.0, 44.75, 45.0, 344.75, 345.0, 359.75)] == [0, 0, 1, 1, 2, 11, 12, 12]
    assert int(RP.rot_bin(np.array([10.0], np.float32), np.array([350.0], np.float32))[0]) == 1   # -340 + 360 = 20
    assert int(RP.rot_bin(np.array([0.0], np.float32), np.array([0.25], np.float32))[0]) == 12    # 359.75
    # 15 / 30 is 0.5 in float32 (the one exact half-way value a 0.25-degree grid reaches): round() and rint() part here
    assert np.float32(15.0) * (np.float32(1.0) / np.float32(30)) == np.float32(0.5)


def test_three_maxima_rules():
    h = np.zeros(30, int)
    h[[9, 2, 5, 11]] = 7
    assert RP.three_maxima(h) == (2, 5, 9)                  # strict >: the lower index wins a tie
    h[:] = 0
    h[0], h[5], h[9] = 100, 10, 9
    assert RP.three_maxima(h) == (0, 5, -1)                 # 10 < 0.1f * 100 is false, 9 < 10 is true
    h[5] = 9
    assert RP.three_maxima(h) == (0, -1, -1)                # the second falls: the third goes with it
    assert RP.three_maxima(np.zeros(30, int)) == (-1, -1, -1)


@pytest.mark.parametrize("case", sorted(RP.CASES))
@pytest.mark.parametrize("M", [119, 120, 130, 400, 1031])
def test_cases_do_what_they_say(case, M):
    rng = np.random.default_rng(M)
    pairs = np.stack([rng.permutation(M), rng.permutation(M)], 1)
    bins, exact = RP.case_bins(case, pairs, rng)
    aa, ab = RP.plant(pairs, M, M, bins, rng, exact)
    assert aa.dtype == ab.dtype == np.float32 and aa.min() >= 0 and aa.max() < 360 and ab.min() >= 0 and ab.max() < 360
    wrapped = float(np.mean(aa[pairs[:, 0]] < ab[pairs[:, 1]]))
    assert 0.25 < wrapped < 0.75 or case == "single_bin" and wrapped > 0.25, wrapped   # the +360 branch runs
    h = RP.histogram(aa, ab, pairs)
    kept = set(b for b in RP.three_maxima(h) if b >= 0)
    removed = set(np.nonzero(h)[0]) - kept
    want = {"three_clear": ({3, 7, 11}, {1}), "second_below": ({4}, {8}), "four_way_tie": ({2, 5, 9}, None),
            "tie_for_third": ({6, 1, 3}, {10}), "wrap_and_top_bin": ({12, 0, 6}, set()), "top_bin_split": ({12, 0, 6}, {9}),
            "half_way": ({1, 2, 0}, {3}), "half_way_split": ({1, 0, 5}, {8}), "single_bin": ({12}, set()),
            "ten_percent_edge": ({0, 5}, None)}[case]
    assert kept == want[0] and (want[1] is None or removed == want[1]), (kept, removed)
    if case == "four_way_tie":
        assert 11 in removed and h[11] == h[2] == h[5] == h[9]
    if case == "ten_percent_edge":
        assert h[5] * 10 == h[0] and h[9] == h[5] - 1 and 9 in removed
    assert bool(removed) == RP.CASES[case][2]
    # what each companion case is for: fold bin 12 into 0 / send rot = 15 to bin 0 and the kept set changes
    if case in ("top_bin_split", "half_way_split"):
        g = h.copy()
        src = 12 if case == "top_bin_split" else 1
        g[0] += g[src]
        g[src] = 0
        third = 6 if case == "top_bin_split" else 5
        assert third in kept and third not in RP.three_maxima(g)


def test_shared_key_points_are_split():
    rng = np.random.default_rng(0)
    pairs = np.stack([np.arange(200), np.r_[np.arange(190), np.arange(10)]], 1)  # rows 190.. share j with rows 0..9
    bins, exact = RP.case_bins("three_clear", pairs, rng)
    aa, ab = RP.plant(pairs, 200, 190, bins, rng, exact)
    keep = RP.keep_mask(aa, ab, pairs)
    for t in range(10):
        assert keep[t] != keep[190 + t]


# ---- the oracle against the plan ----------------------------------------------------------------------------------------
PLAIN = [n for n in SCENES if n != "initialization"]


@pytest.mark.parametrize("case", sorted(RP.CASES))
@pytest.mark.parametrize("name", PLAIN)
def test_oracle_matches_the_plan(oracle, name, case):
    sc = scene(name)
    p = S.plan(sc, case)
    M = len(p["pairs"])
    print("%s / %s: %d pairs, %d removed" % (name, case, M, p["removed"]))
    assert M >= RP.CASES[case][1]
    want = RP.expect(p["out_off"], p["count_off"], p["pairs"], p["keep"], sc.index)
    got = sc.oracle(p["aa"], p["ab"], True)
    assert S.same(got, want), "%d vs %d, %d entries differ" % (got[0], want[0], int((got[1] != want[1]).sum()))
    if RP.CASES[case][2]:
        assert p["removed"] >= 1 and got[0] < p["count_off"]
    else:
        assert p["removed"] == 0 and S.same(got, (p["count_off"], p["out_off"]))


def test_last_frame_scene_has_rows_under_other_rows(oracle):
    """Two rows on one key point, both counted, both voting; planted so that exactly one of them is removed, which
    leaves the key point unassigned whichever of the two it was (ORBmatcher.cc:1456-1467)."""
    sc = scene("last_frame")
    pairs, n0, out0 = S.base(sc)
    js, cnt = np.unique(pairs[:, 1], return_counts=True)
    shared = js[cnt > 1]
    assert len(shared) >= 5 and len(pairs) == n0 > int((out0 >= 0).sum())
    p = S.plan(sc, "three_clear")
    _, out = sc.oracle(p["aa"], p["ab"], True)
    split = 0
    for j in shared:
        k = p["keep"][pairs[:, 1] == j]
        if k.any() and not k.all():
            split += 1
            assert out[j] == -1
    assert split >= 5
    later_kept = [j for j in shared if p["keep"][(pairs[:, 1] == j) & (pairs[:, 0] == out0[j])].all()
                  and not p["keep"][pairs[:, 1] == j].all()]
    assert later_kept, "some key point must lose its surviving later row to the removed earlier one"


def test_bow_frame_version_never_shares_a_key_point(oracle):
    """ORBmatcher.cc:209-210 skips a frame key point that already has a match, so in SearchByBoW(KF, F) no two rows
    vote with the same key point, even in the near-duplicate scene: count == assigned entries."""
    sc = S.BowDuplicatesScene()
    pairs, n0, out0 = S.base(sc)
    assert n0 == len(pairs) == int((out0 >= 0).sum()) > 100 and len(np.unique(pairs[:, 1])) == n0


@pytest.mark.parametrize("case", [c for c in sorted(RP.CASES) if RP.CASES[c][2]])
def test_initialization_differs_in_planted_rows(oracle, case):
    """Stale votes of stolen matches (random angles here) break the simple rule; the check must still bite."""
    sc = scene("initialization")
    p = S.plan(sc, case)
    assert len(p["pairs"]) >= RP.CASES[case][1]
    n, out, pm = sc.oracle(p["aa"], p["ab"], True)
    rows = p["pairs"][:, 0]
    assert n < p["count_off"] and np.any(out[rows] != p["out_off"][rows])
    assert np.all((out == p["out_off"]) | (out == -1))


def test_steal_scene_bites(oracle):
    """The crafted scene: the stale votes make bin 10 third, which pushes bin 9 (held by live rows) out."""
    sc = S.StealScene()
    n0, out0, _ = sc.unchecked()
    assert n0 == 30 and np.array_equal(np.nonzero(out0 >= 0)[0], sc.final_pairs[:, 0])
    aa, ab = sc.angles()
    voters = np.concatenate([sc.final_pairs, sc.stale_pairs])
    with_stale = RP.three_maxima(RP.histogram(aa, ab, voters))
    without = RP.three_maxima(RP.histogram(aa, ab, sc.final_pairs))
    assert with_stale == (2, 6, 10) and without == (2, 6, 9)
    keep = RP.keep_mask(aa, ab, sc.final_pairs, voters=voters)
    n, out, pm = sc.oracle(aa, ab, True)
    want = out0.copy()
    want[sc.final_pairs[~keep, 0]] = -1
    assert n == 30 - int((~keep).sum()) == 25 and np.array_equal(out, want)
    wrong = out0.copy()
    wrong[sc.final_pairs[~RP.keep_mask(aa, ab, sc.final_pairs), 0]] = -1
    assert not np.array_equal(out, wrong), "without the stale votes the kept bins differ: the scene must show that"


@pytest.mark.parametrize("name", sorted(SCENES))
def test_no_pairs(oracle, name):
    """Nothing to match: count 0 and every output entry as it was (-1, or the caller's -2 marks)."""
    sc = scene(name, True)
    rng = np.random.default_rng(1)
    aa, ab = (rng.uniform(0, 360, n).astype(np.float32) for n in (sc.n_a, sc.n_b))
    for check in (True, False):
        r = sc.oracle(aa, ab, check)
        assert r[0] == 0
        if name == "keyframe":
            assert np.array_equal(r[1], sc.k0) and (sc.k0 == -2).sum() == 100
        else:
            assert np.all(r[1] == -1)
