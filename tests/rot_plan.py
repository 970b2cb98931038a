"""Plants rotation histograms into matcher inputs (test-side helper, plain numpy; used by test_rot_plan.py and
test_gpu_matcher_rotation.py).

Every matcher with mbCheckOrientation ends the same way (ORBmatcher.cc:236-246 / :267-285 and its six siblings): an
accepted pair (i, j) votes into bin round((angle_a[i] - angle_b[j], +360 if negative) / 30) of a 30-slot histogram,
ComputeThreeMaxima (:1601-1642) keeps at most three bins, and the pairs of every other bin are removed and uncounted.
The angles are read by nothing else, so a test may take any scene, look at the pairs the matcher accepts without the
check, and choose angles that put those pairs into whatever histogram it wants.

rot_bin / three_maxima below are written from ORBmatcher.cc, in np.float32, and are the second statement of the rule
the oracle (and through it the device) is pinned to."""
import numpy as np

HISTO_LENGTH = 30
f32 = np.float32


def rot_bin(a, b):
    """ORBmatcher.cc:238-243: float rot = a - b; if (rot < 0.0) rot += 360.0f; bin = round(rot * factor);
    if (bin == HISTO_LENGTH) bin = 0.  factor = 1.0f / HISTO_LENGTH, so bin = rot / 30: the bins in use are 0..12,
    [345, 360) lands in 12 and the fold to 0 never happens for angles in [0, 360).  round() is half away from zero."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    factor = f32(1.0) / f32(HISTO_LENGTH)
    rot = (a - b).astype(f32)
    rot = np.where(rot < 0.0, (rot + f32(360.0)).astype(f32), rot).astype(f32)
    x = (rot * factor).astype(f32)
    bins = np.floor(x.astype(np.float64) + 0.5).astype(np.int64)  # x >= 0: half away from zero == floor(x + 0.5), exact in double
    return np.where(bins == HISTO_LENGTH, 0, bins)


def three_maxima(h):
    """ORBmatcher.cc:1601-1642 on the bin sizes: (ind1, ind2, ind3), -1 where there is none."""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i in range(len(h)):
        s = int(h[i])
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if f32(max2) < f32(0.1) * f32(max1):      # int < float: the int converts to float (:1633)
        ind2 = ind3 = -1
    elif f32(max3) < f32(0.1) * f32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def histogram(angle_a, angle_b, pairs):
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    return np.bincount(rot_bin(angle_a[pairs[:, 0]], angle_b[pairs[:, 1]]), minlength=HISTO_LENGTH)


def keep_mask(angle_a, angle_b, pairs, voters=None):
    """Which of `pairs` (rows (i, j): angle_a[i] against angle_b[j]) survive the check.  voters: the pairs that vote,
    if they are not the same list (SearchForInitialization's stale votes); default: `pairs` themselves."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    h = histogram(angle_a, angle_b, pairs if voters is None else voters)
    kept = [b for b in three_maxima(h) if b >= 0]
    return np.isin(rot_bin(angle_a[pairs[:, 0]], angle_b[pairs[:, 1]]), kept)


EXACT_ROTS = {"15": 15.0, "45": 45.0, "345": 345.0, "below360": 359.75}


def _bin_range(b):
    """[lo, hi) of rot (degrees) that round(rot / 30) sends to bin b, for rot in [0, 360)."""
    lo = 0.0 if b == 0 else 30.0 * b - 15.0
    hi = 360.0 if b == 12 else 30.0 * b + 15.0
    return lo, hi


def plant(pairs, n_a, n_b, bins_per_pair, rng, exact=None):
    """angle_a [n_a], angle_b [n_b], float32 in [0, 360), such that pair k = (i, j) falls into bins_per_pair[k].
    Everything lives on a 0.25-degree grid, so angle_b + rot, the wrap and the difference the matcher forms are exact
    in float32.  angle_b is random per key point; angle_a[i] = angle_b[j] + rot (mod 360) with rot drawn inside the bin
    or, where exact[k] names one, EXACT_ROTS[exact[k]].  About half of the pairs get angle_a < angle_b (the +360 branch):
    the first pair to use a key point j draws angle_b[j] on the side of 360 - rot that wraps or does not wrap; later
    pairs on the same j get their bin through angle_a alone.  An index i may appear only once."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    bins_per_pair = np.asarray(bins_per_pair, np.int64)
    assert len(bins_per_pair) == len(pairs)
    assert len(np.unique(pairs[:, 0])) == len(pairs), "an A row carries one angle: it can sit in one pair only"
    assert np.all((bins_per_pair >= 0) & (bins_per_pair <= 12)), "rot / 30 reaches bins 0..12 only"
    q = 4  # grid steps per degree
    angle_a = rng.integers(0, 360 * q, n_a).astype(np.int64)
    angle_b = rng.integers(0, 360 * q, n_b).astype(np.int64)
    seen = np.zeros(n_b, bool)
    for k, (i, j) in enumerate(pairs):
        name = None if exact is None else exact[k]
        if name:
            rot = int(round(EXACT_ROTS[name] * q))
        else:
            lo, hi = _bin_range(int(bins_per_pair[k]))
            rot = int(rng.integers(int(lo * q) + 1, int(hi * q) - 1))  # strictly inside: the edges belong to `exact`
        if not seen[j]:
            seen[j] = True
            wrap = rot > 0 and rng.random() < 0.5
            # a = b + rot wraps past 360 (and then a < b) iff b >= 360 - rot
            angle_b[j] = rng.integers(360 * q - rot, 360 * q) if wrap else rng.integers(0, 360 * q - rot)
        angle_a[i] = (angle_b[j] + rot) % (360 * q)
    angle_a = (angle_a.astype(np.float64) / q).astype(f32)
    angle_b = (angle_b.astype(np.float64) / q).astype(f32)
    assert angle_a.min(initial=0) >= 0 and angle_a.max(initial=0) < 360 and angle_b.max(initial=0) < 360
    got = rot_bin(angle_a[pairs[:, 0]], angle_b[pairs[:, 1]])
    assert np.array_equal(got, bins_per_pair), "planting failed for pairs %s" % np.nonzero(got != bins_per_pair)[0][:8]
    return angle_a, angle_b


# ---- the named histograms ------------------------------------------------------------------------------------------
# Each case: counts(M) -> list of (bin, n, exact-name or None) with sum n == M, stated for any M >= its minimum; the
# fixed numbers of the table (100 / 10 / 9 ...) are what the formulas give at the M they add up to.

def _three_clear(M):
    n3, n7, n11 = M // 2, M // 4, (15 * M) // 100
    return [(3, n3, None), (7, n7, None), (11, n11, None), (1, M - n3 - n7 - n11, None)]


def _ten_percent_edge(M):
    # bin 5 sits exactly on the cut: n5 * 10 == n0, and (float)n5 < 0.1f * (float)n0 is false, so it stays; bin 9 has
    # one pair less and goes.  M = 119 gives 100 / 10 / 9; a larger M scales the three (the equality must hold, so
    # the remainder cannot go to bin 0) and the up to 11 pairs left over go one each to bins that are removed anyway.
    k = (M + 1) // 12
    out = [(0, 10 * k, None), (5, k, None), (9, k - 1, None)]
    rest = M - (12 * k - 1)
    spare = [1, 2, 3, 4, 6, 7, 8, 10, 11, 12]
    assert rest <= 11
    for t in range(rest):
        out.append((spare[t % len(spare)], 1, None))
    return _merge(out)


def _second_below(M):
    n8 = -(-M // 11) - 1  # the largest n8 with 10 * n8 < M - n8: one pair below the cut (M = 109: 100 / 9)
    return [(4, M - n8, None), (8, n8, None)]


def _four_way_tie(M):
    n = M // 4
    out = [(9, n, None), (2, n, None), (5, n, None), (11, n, None)]
    for t in range(M - 4 * n):
        out.append(((0, 7, 12)[t], 1, None))
    return out


def _tie_for_third(M):
    t = (8 * M) // 76
    n1 = (20 * M) // 76
    return [(6, M - 2 * t - n1, None), (1, n1, None), (10, t, None), (3, t, None)]


def _wrap_and_top_bin(M):
    n0, n6 = (30 * M) // 100, M // 10
    return [(12, M - n0 - n6, None), (0, n0, None), (6, n6, None)]


def _top_bin_split(M):
    # bins 12 and 0 hold 44 % each: bin 6 (7 %) is third while they are two bins and falls under the 10 % cut if a
    # matcher folds [345, 360) into bin 0; bin 9 (5 %) is fourth and goes.  Half of bin 12 sits just under 360 or on 345.
    n6, n9 = (7 * M) // 100, (5 * M) // 100
    n = (M - n6 - n9) // 2
    n12, q = M - n6 - n9 - n, n // 4
    return [(12, n12 - 2 * q, None), (12, q, "345"), (12, q, "below360"), (0, n, None), (6, n6, None), (9, n9, None)]


def _half_way(M):
    n1, n2, n0 = M // 2, (30 * M) // 100, (15 * M) // 100
    return [(1, n1, "15"), (2, n2, "45"), (0, n0, None), (3, M - n1 - n2 - n0, None)]


def _half_way_split(M):
    # rot = 15 exactly is bin 1 under round() and bin 0 under rint(): as two bins of 44 % they leave bin 5 (7 %) third
    # and kept; merged into one of 88 % they push it under the 10 % cut.  Bin 8 is fourth and goes either way.
    n5, n8 = (7 * M) // 100, (5 * M) // 100
    n = (M - n5 - n8) // 2
    return [(1, n, "15"), (0, M - n5 - n8 - n, None), (5, n5, None), (8, n8, None)]


def _single_bin(M):
    return [(12, M, None)]


def _merge(items):
    out = {}
    for b, n, e in items:
        out[(b, e)] = out.get((b, e), 0) + n
    return [(b, n, e) for (b, e), n in out.items() if n > 0]


#        name               counts            min M  removes at least one pair
CASES = {"three_clear": (_three_clear, 20, True),
         "ten_percent_edge": (_ten_percent_edge, 119, True),
         "second_below": (_second_below, 12, True),
         "four_way_tie": (_four_way_tie, 8, True),
         "tie_for_third": (_tie_for_third, 20, True),
         # 60 / 30 / 10 % in three bins: by ComputeThreeMaxima's own rule all three stay, so this case removes nothing;
         # what it pins is that bins 12 and 0 are counted apart.  top_bin_split is its companion that does remove.
         "wrap_and_top_bin": (_wrap_and_top_bin, 10, False),
         "top_bin_split": (_top_bin_split, 100, True),
         "half_way": (_half_way, 20, True),
         "half_way_split": (_half_way_split, 100, True),
         "single_bin": (_single_bin, 1, False)}


def case_counts(name, M):
    fn, min_m, _ = CASES[name]
    assert M >= min_m, "case %s needs %d pairs, the scene gives %d" % (name, min_m, M)
    items = _merge(fn(M))
    assert sum(n for _, n, _ in items) == M
    return items


def case_bins(name, pairs, rng, split_shared=True):
    """bins_per_pair and exact for `pairs` under case `name`, shuffled over the pairs.  split_shared: where two pairs
    share a key point j, the first gets a bin that is kept and the second one that is removed (or the other way round,
    alternating), if the case has both kinds."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    M = len(pairs)
    bins, exact = [], []
    for b, n, e in case_counts(name, M):
        bins += [b] * n
        exact += [e] * n
    order = rng.permutation(M)
    bins, exact = np.asarray(bins, np.int64)[order], [exact[t] for t in order]
    kept = [b for b in three_maxima(np.bincount(bins, minlength=HISTO_LENGTH)) if b >= 0]
    is_kept = np.isin(bins, kept)
    if split_shared and is_kept.any() and not is_kept.all():
        by_j = {}
        for k, j in enumerate(pairs[:, 1]):
            by_j.setdefault(int(j), []).append(k)
        groups = [g for g in by_j.values() if len(g) > 1]
        fixed = np.zeros(M, bool)
        for g in groups:
            fixed[g] = True
        free = [k for k in range(M) if not fixed[k]]
        for t, g in enumerate(groups):
            want = [t % 2 == 0, t % 2 != 0] + [True] * (len(g) - 2)
            for k, w in zip(g, want):
                if is_kept[k] == w:
                    continue
                s = next((x for x in free if is_kept[x] == w), None)
                if s is None:
                    continue
                bins[k], bins[s] = bins[s], bins[k]
                exact[k], exact[s] = exact[s], exact[k]
                is_kept[k], is_kept[s] = is_kept[s], is_kept[k]
    return bins, exact


def plant_case(name, pairs, n_a, n_b, rng):
    """(angle_a, angle_b) for the named case over `pairs`."""
    bins, exact = case_bins(name, pairs, rng)
    return plant(pairs, n_a, n_b, bins, rng, exact)


def expect(out_unchecked, n_unchecked, pairs, keep, index):
    """What the matcher must return with the check on, from its result with the check off.  pairs: every accepted
    row (i, j) of the unchecked run, the ones whose key point a later row took over included; index: "b" if the
    output is indexed by j and holds i, "a" if it is indexed by i and holds j.  Every removed row is uncounted; an
    output entry goes back to -1 if ANY row that voted with it is removed (ORBmatcher.cc:1456-1467 clears
    mvpMapPoints[rotHist[i][j]] whoever holds it by then)."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    assert len(pairs) == n_unchecked, "the pair list must account for every counted row"
    out = np.array(out_unchecked, np.int32)
    slot = pairs[:, 1] if index == "b" else pairs[:, 0]
    out[slot[~keep]] = -1
    return n_unchecked - int((~keep).sum()), out
