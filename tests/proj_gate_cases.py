"""Hand-worked cases for the gates of the projection matchers (test-side helper, shared by test_proj_gates.py on the
host and test_gpu_proj_gates.py on the device).  Every case is a handful of key points built directly, and carries its
expected result as a literal that is worked out in the comment beside it from the reference lines the kernels cite --
never from the code under test.  test_proj_gates.py holds the oracle to the same literals.

One camera throughout, the one of tests/proj_boundary_test.cpp: identity Tcw, fx = fy = 512, cx = 320, cy = 240,
mbf = 40, a 640 x 480 image (grid cells of 10 x 10 pixels), eight levels of 1.2.  All coordinates are exact in float.

Descriptors have exact Hamming distances: a row is all zeros unless said otherwise, and `bits` = d sets the low d bits."""
import numpy as np

F32 = np.float32
W, H = 640, 480
FX, FY, CX, CY, MBF = 512.0, 512.0, 320.0, 240.0, 40.0
TCW = np.eye(4, dtype=F32)
NLEVELS = 8
TH_HIGH, TH_LOW = 100, 50


def scale_factors(factor=1.2, nlevels=NLEVELS):
    """mvScaleFactor as ORBextractor.cc:421 builds it: a running float product."""
    sf = np.ones(nlevels, F32)
    for l in range(1, nlevels):
        sf[l] = sf[l - 1] * F32(factor)
    return sf


SF = scale_factors()
LOG_SF = float(np.log(F32(1.2)))  # mfLogScaleFactor = log(mfScaleFactor), a float
NAN, INF = F32(np.nan), F32(np.inf)


def up(x):
    """The next float above x."""
    return np.nextafter(F32(x), F32(np.inf))


def down(x):
    """The next float below x."""
    return np.nextafter(F32(x), F32(-np.inf))


def low_bits(d):
    """A 256-bit descriptor with its low d bits set: distance d from the all-zero descriptor, |d1 - d2| from another."""
    out = np.zeros(32, np.uint8)
    out[:d // 8] = 255
    if d % 8:
        out[d // 8] = (1 << (d % 8)) - 1
    return out


def descriptors(bits):
    return np.stack([low_bits(int(b)) for b in bits]) if len(bits) else np.zeros((0, 32), np.uint8)


# ---- key points and rows --------------------------------------------------------------------------------------------
def kp(x, y, octave=0, ur=-1.0, bits=0):
    return (x, y, octave, ur, bits)


def row(x, y, level=0, cos=0.9, xr=0.0, bits=0, in_view=1, bad=0, obs=1):
    return (x, y, level, cos, xr, bits, in_view, bad, obs)


def make_frame(side, kps, sf=SF):
    """side: the oracle's Python module or the product library; both offer Frame(x, y, octave, angle, u_right, desc, ...)."""
    a = list(zip(*kps))
    n = len(kps)
    return side.Frame(np.array(a[0], F32), np.array(a[1], F32), np.array(a[2], np.int32), np.zeros(n, F32),
                      np.array(a[3], F32), descriptors(a[4]), W, H, sf)


def make_mp(rows):
    """The `mp` dict of SearchByProjection(Frame&, vpMapPoints, th): the query of every row, set directly."""
    a = list(zip(*rows))
    return {"proj_x": np.array(a[0], F32), "proj_y": np.array(a[1], F32), "level": np.array(a[2], np.int32),
            "view_cos": np.array(a[3], F32), "proj_xr": np.array(a[4], F32), "desc": descriptors(a[5]),
            "in_view": np.array(a[6], np.uint8), "bad": np.array(a[7], np.uint8), "obs_pos": np.array(a[8], np.uint8)}


class LocalCase:
    """One call of the local-map flavour: expect[j] is the row that ends up holding key point j (kp_to_mp)."""

    def __init__(self, name, kps, rows, expect, th=1.0, nnratio=0.8, k0=None, rewalk=None):
        self.name, self.kps, self.rows, self.th, self.nnratio = name, kps, rows, th, nnratio
        self.expect = np.array(expect, np.int32)
        self.k0 = np.full(len(kps), -1, np.int32) if k0 is None else np.array(k0, np.int32)
        self.rewalk = rewalk  # None: not asserted; else whether pass 2 has to walk some row again
        assert len(self.expect) == len(kps) == len(self.k0)

    def __repr__(self):
        return self.name


# ---- e. candidate gates (ORBmatcher.cc:82-97, Frame.cc:327-380) ----------------------------------------------------
# Level 0 with th = 1 and cos 0.9 is a window of r = 4.0 * 1 = 4; level 1 one of 4.0f * 1.2f = 4.8; level 2 one of 5.76.
GATE_CASES = [
    # RadiusByViewingCos (:131-137) compares in double: (double)0.998f = 0.99800002574920654 > 0.998, so r = 2.5 and the
    # key point 3 px away is outside; the next float below, 0.99799996614456177, gives r = 4 and it is inside
    LocalCase("cos_0998_is_above", [kp(103, 100)], [row(100, 100, cos=F32(0.998))], [-1]),
    LocalCase("cos_next_below_0998", [kp(103, 100)], [row(100, 100, cos=down(0.998))], [0]),
    # GetFeaturesInArea keeps |dx| < r && |dy| < r (Frame.cc:372): 4 away is outside, 3.5 inside, on every side
    LocalCase("strict_window",
              [kp(104, 100), kp(203.5, 100), kp(100, 204), kp(200, 203.5), kp(96, 300), kp(96.5, 400), kp(300, 296),
               kp(400, 296.5)],
              [row(100, 100), row(200, 100), row(100, 200), row(200, 200), row(100, 300), row(100, 400), row(300, 300),
               row(400, 300)],
              [-1, 1, -1, 3, -1, 5, -1, 7]),
    # rows of level 2 take octaves [l-1, l] = [1, 2] (:82): octave 1 and 2 match, 3 and 0 do not
    LocalCase("level_window", [kp(100, 100, 1), kp(200, 100, 2), kp(300, 100, 3), kp(400, 100, 0)],
              [row(100, 100, 2), row(200, 100, 2), row(300, 100, 2), row(400, 100, 2)], [0, 1, -1, -1]),
    # th = 3 multiplies the radius (:73-74): r = 12, so 12 away is outside and 11.5 inside; with th = 1.0 (every other
    # case here) the radius stays 4.0 as strict_window shows
    LocalCase("th_multiplies", [kp(112, 100), kp(211.5, 100)], [row(100, 100), row(200, 100)], [-1, 1], th=3.0),
    # AssignFeaturesToGrid rounds (Frame.cc:382-392): x = 636 is cell round(63.6) = 64 of 64 and y = 476 cell 48 of 48, so
    # the key point is in no cell and no window finds it, 1 px from the row.  x = 634 is cell 63 and is found.
    LocalCase("grid_edge", [kp(636, 100), kp(634, 300), kp(100, 476)], [row(637, 100), row(636, 300), row(100, 477)],
              [-1, 1, -1]),
    # mvuRight gate (:91-96) applies to u_right > 0 only and cuts er > r: u_right 0.0 is not gated (the row predicts 500);
    # 0.5 against 4.5 is er = 4 = r and passes; against the next float above 4.5 er = 4.0000005 fails; -1 is never gated
    LocalCase("u_right_gate",
              [kp(100, 100, ur=0.0), kp(200, 100, ur=0.5), kp(300, 100, ur=0.5), kp(400, 100, ur=-1.0)],
              [row(100, 100, xr=500.0), row(200, 100, xr=4.5), row(300, 100, xr=up(4.5)), row(400, 100, xr=500.0)],
              [0, 1, -1, 3]),
    # mbTrackInView false (:54) and isBad() (:57) rows are skipped
    LocalCase("inactive_rows", [kp(100, 100), kp(200, 100)], [row(100, 100, in_view=0), row(200, 100, bad=1)], [-1, -1]),
    # :87-89: a key point is hidden when its map point has observations.  Key point 0 is held from outside (-2) and stays;
    # key point 1 is held by row 2, which has none, so row 1 takes it; key point 2 is free; key point 3 is held by row 0,
    # which has observations, so row 4 leaves it
    LocalCase("held_key_points", [kp(100, 100), kp(200, 100), kp(300, 100), kp(500, 100)],
              [row(100, 100), row(200, 100), row(400, 400, obs=0), row(300, 100), row(500, 100)], [-2, 1, 3, 0],
              k0=[-2, 2, -1, 0]),
]

# ---- g. accept rules (ORBmatcher.cc:99-125) ------------------------------------------------------------------------
ACCEPT_CASES = [
    # bestDist <= TH_HIGH (:114): 100 is accepted, 101 is not; a single candidate has bestLevel2 = -1: no ratio test
    LocalCase("th_high", [kp(100, 100, bits=100), kp(200, 100, bits=101)], [row(100, 100), row(200, 100)], [0, -1]),
    # :116 tests the ratio only when best and second share their level.  nnratio 0.5, rows of level 1 (octaves 0 and 1):
    # 40 (octave 0) against 41 (octave 1): no test, accepted; 40 against 41, both octave 1: 40 > 20.5, rejected;
    # 40 against 80, both octave 1: 40 > 0.5 * 80 is false, accepted
    LocalCase("ratio_same_level_only",
              [kp(100, 100, 0, bits=40), kp(101, 100, 1, bits=41), kp(300, 100, 1, bits=40), kp(301, 100, 1, bits=41),
               kp(500, 100, 1, bits=40), kp(501, 100, 1, bits=80)],
              [row(100, 100, 1), row(300, 100, 1), row(500, 100, 1)], [0, -1, -1, -1, 2, -1], nnratio=0.5),
    # equal distances: `dist < bestDist` (:101) keeps the candidate visited first, and GetFeaturesInArea visits cells ix
    # outer, iy inner, and a cell's key points in their order (Frame.cc:352-376).  Octaves 0 / 1, so no ratio test.
    # th = 3, level 1: r = 14.4.  Site by site, (cell x, cell y) of the two key points:
    #   (11, 10) and (10, 10): the second wins;  (30, 11) and (30, 10): the second wins;  both in (50, 10): the first wins;
    #   (10, 31) and (11, 30): ix decides, the first wins;  (31, 30) and (30, 31): the second wins
    LocalCase("tie_takes_first_visited",
              [kp(106, 100, 0, bits=10), kp(96, 100, 1, bits=10), kp(300, 106, 0, bits=10), kp(300, 96, 1, bits=10),
               kp(500, 100, 0, bits=10), kp(501, 100, 1, bits=10), kp(96, 306, 0, bits=10), kp(106, 296, 1, bits=10),
               kp(306, 296, 0, bits=10), kp(296, 306, 1, bits=10)],
              [row(101, 100, 1), row(300, 101, 1), row(500, 100, 1), row(101, 301, 1), row(301, 301, 1)],
              [-1, 0, -1, 1, 2, -1, 3, -1, -1, 4], th=3.0),
]


# ---- h. decision depth of the cached candidate list ---------------------------------------------------------------
DEPTH_N = (15, 16, 17, 64, 65)


def depth_ks(n):
    return sorted({k for k in (0, 3, 4, 15, 16, 17, n - 1, n) if 0 <= k <= n})


def depth_case(n, k, nnratio=1.0):
    """n key points at one spot, key point j with its low j+1 bits set, octaves alternating 0 / 1.  Row j < k carries key
    point j's descriptor: distance 0 to it, and 1 to its neighbours, which have the other octave (no ratio test), so row j
    takes key point j.  The last row is all zeros, level 1, th = 3: key point j is j + 1 away and 0..k-1 are held, so it
    takes key point k, k + 1 <= 66 <= TH_HIGH away, with the second (k + 2 away) on the other octave.  k = n: nothing left.

    What the device has to do for it (nnratio 1.0): the last row's cached list is the 16 nearest, key points 0..15.  Up to
    k = 14 it finds its best and second among them; at k = 15 only the best, 16 away, whose unseen second is at least the
    16 of the last word: not rejected at nnratio 1.0 whatever its level; from k = 16 on every cached candidate is held and
    the window is walked again.  More than 64 candidates are not ranked at all: every row is walked again."""
    kps = [kp(100, 100, j % 2, bits=j + 1) for j in range(n)]
    rows = [row(100, 100, 1, bits=j + 1) for j in range(k)] + [row(100, 100, 1)]
    expect = [j if j < k else -1 for j in range(n)]
    if k < n:
        expect[k] = k  # the last row is row k
    rewalk = (k >= 16 or n > 64) if nnratio == 1.0 else None
    return LocalCase("depth_n%d_k%d_r%g" % (n, k, nnratio), kps, rows, expect, th=3.0, nnratio=nnratio, rewalk=rewalk)


def depth_cases():
    return [depth_case(n, k, r) for n in DEPTH_N for k in depth_ks(n) for r in (1.0, 0.8)]


# ---- i. width of the preference key's fields ---------------------------------------------------------------------
def key_width_case(swapped):
    """4097 key points of octave 0 in one grid cell and one of octave 1 in the cell visited next; the row at (103, 103),
    level 1, th = 1 (r = 4.8) sees cells 9..11 both ways, so cell (10, 10) is number (10 - 9) * 3 + (10 - 9) = 4 of its
    window, an even number, and (10, 11) number 5.  Every descriptor is 200 away except the last of the crowded cell
    (position 4096 in it) and the lone key point, both 10 away on different octaves: whichever is visited first is the best
    (:101 is strict) and is accepted without a ratio test.
      plain:   crowded cell (10, 10), lone key point 0 in (10, 11): key point 4097 is visited first and wins.
      swapped: crowded cell (10, 11), lone key point 0 in (10, 10): key point 0 is visited first and wins."""
    crowd_y, lone_y = (106, 100) if swapped else (100, 106)
    kps = [kp(100, lone_y, 1, bits=10)] + [kp(100, crowd_y, 0, bits=200) for _ in range(4096)] + [kp(100, crowd_y, 0, bits=10)]
    expect = [-1] * 4098
    expect[0 if swapped else 4097] = 0
    return LocalCase("key_width_swapped" if swapped else "key_width", kps, [row(103, 103, 1)], expect, rewalk=True)


def window_cell_number(x, y, r, kx, ky):
    """The number of key point (kx, ky)'s cell in the visiting order of the window (x, y, r): Frame.cc:334-352."""
    inv = F32(64) / F32(640)
    c0 = max(0, int(np.floor((F32(x) - F32(r)) * inv)))
    r0 = max(0, int(np.floor((F32(y) - F32(r)) * inv)))
    r1 = min(47, int(np.ceil((F32(y) + F32(r)) * inv)))
    return (int(np.round(F32(kx) * inv)) - c0) * (r1 - r0 + 1) + int(np.round(F32(ky) * inv)) - r0


def local_cases():
    return GATE_CASES + ACCEPT_CASES + depth_cases() + [key_width_case(False), key_width_case(True)]


# ---- a. Frame::isInFrustum + MapPoint::PredictScale (Frame.cc:269-325, MapPoint.cc:385-394) -------------------------
A, B, C, D = (0, 0, 2), (1.25, 0, 2), (-1.25, 0, 2), (0, 0, -2)
TOWARDS = (0, 0, 1)
# |B| = |C| = sqrt(1.5625 + 4) in double, rounded to float (cv::norm); PO.n = 2, divided in double, rounded to float
COS_B = F32(2.0 / float(F32(np.sqrt(5.5625))))
# 1.2f * 2.5f is 3.0000001192..., exactly half way between 3 and the next float: it rounds to even, 3.0
assert F32(1.2) * F32(2.5) == F32(3.0) and F32(0.8) * F32(2.5) == F32(2.0)
XR_3 = F32(320) - F32(40) * (F32(1) / F32(3))  # u - mbf * invz for z = 3, in float as Frame.cc:293 computes it

OUT, BAD = "out", "bad"  # not in view / predicted level out of range: counted, and not in view
# dist_on_max: logf(0.8333333f) = -0.18232158 against logf(1.2f) = 0.18232161: the quotient is -0.9999998, ceil -0,
# level 0.  Two floats more in the numerator's magnitude and the row would be level -1 and counted.
DIST_ON_MAX = (320.0, 240.0, XR_3, 0, 1.0)


def frustum_rows():
    """(name, position, normal, min_dist, max_dist, skip, obs_pos, expected).  expected: OUT, BAD, or the track scratch
    (proj_x, proj_y, proj_xr, level, view_cos).  min_dist 0.5 and max_dist 3 unless the row is about them: |A| = 2 gives
    ratio 1.5 and log(1.5) / log(1.2) = 2.22: level 3; B and C give ratio 1.272: 1.32, level 2."""
    a3 = (320.0, 240.0, 300.0, 3, 1.0)  # A: u = 512 * 0 * 0.5 + 320, ur = 320 - 40 * 0.5
    return [
        ("A_unobserved", A, TOWARDS, 0.5, 3.0, 0, 0, a3),  # Observations() == 0: in view all the same, does not block
        ("A", A, TOWARDS, 0.5, 3.0, 0, 1, a3),
        ("B_on_max_x", B, TOWARDS, 0.5, 3.0, 0, 1, (640.0, 240.0, 620.0, 2, COS_B)),  # 512 * 1.25 * 0.5 + 320 = 640 <= max_x
        # 256 * 1.2501f + 320 = 640.0256 > 640 (one ulp of 1.25 more would round back to 640)
        ("beyond_B", (F32(1.2501), 0, 2), TOWARDS, 0.5, 3.0, 0, 1, OUT),
        ("C_on_min_x", C, TOWARDS, 0.5, 3.0, 0, 1, (0.0, 240.0, -20.0, 2, COS_B)),
        ("D_behind", D, TOWARDS, 0.5, 3.0, 0, 1, OUT),
        # dist = 3 = 1.2f * 2.5f: `dist > maxDistance` is false.  The ratio 2.5f / 3 = 0.83333331 is within a float of
        # 1 / 1.2f = 0.83333330, so log(ratio) / log(1.2f) is -1 to within a float: the level is 0 or -1, and only the
        # correctly rounded float logarithms say which (DIST_ON_MAX below)
        ("dist_on_max", (0, 0, 3), TOWARDS, 0.5, 2.5, 0, 1, DIST_ON_MAX),
        ("dist_above_max", (0, 0, up(3)), TOWARDS, 0.5, 2.5, 0, 1, OUT),
        ("dist_on_min", A, TOWARDS, 2.5, 3.0, 0, 1, a3),  # 0.8f * 2.5f = 2.0: `dist < minDistance` is false
        ("dist_below_min", (0, 0, down(2)), TOWARDS, 2.5, 3.0, 0, 1, OUT),
        ("cos_on_limit", A, (0, 0, 0.5), 0.5, 3.0, 0, 1, (320.0, 240.0, 300.0, 3, 0.5)),  # 2 * 0.5 / 2: `viewCos < 0.5` false
        ("cos_below_limit", A, (0, 0, down(0.5)), 0.5, 3.0, 0, 1, OUT),
        ("level_8_of_8", A, TOWARDS, 0.5, 8.0, 0, 1, BAD),       # ratio 4: 7.60, level 8 = nlevels
        # z = +0: invz = inf, u = 512 * 0 * inf + 320 = NaN passes the bounds, dist 0 is not below 0.8f * 0, viewCos 0 / 0
        # passes, ratio 3 / 0 = inf: the level is no number
        ("depth_zero", (0, 0, 0), TOWARDS, 0.0, 3.0, 0, 1, BAD),
        # max_dist 0: maxDistance = 0 < dist, the point leaves at Frame.cc:308 before PredictScale and is not counted
        ("max_dist_zero", A, TOWARDS, 0.5, 0.0, 0, 1, OUT),
        # NaN passes every comparison of isInFrustum (they are all `<` / `>` that reject); the level is NaN
        ("nan_position", (NAN, 0, 2), TOWARDS, 0.5, 3.0, 0, 1, BAD),
        # inf: the identity pose multiplies it by 0 in the other two rows, so z, u and v are NaN and pass, but the distance
        # from the camera centre is inf > maxDistance: out at Frame.cc:308, before PredictScale, and not counted
        ("inf_position", (INF, 0, 2), TOWARDS, 0.5, 3.0, 0, 1, OUT),
        ("nan_max_dist", A, TOWARDS, 0.5, NAN, 0, 1, BAD),
        ("skipped", A, TOWARDS, 0.5, 3.0, 1, 1, OUT),            # isBad() / already seen: isInFrustum is never asked
    ]


# key points for the rows above: 0 under A (level 3 takes octaves 2..3), 1 by B (level 2: 1..2), 2 by C
FRUSTUM_KPS = [kp(320, 240, 3), kp(634.5, 240, 2), kp(1, 240, 1)]  # 634.5 is the last cell, 63; from 635 on there is none
FRUSTUM_TH, FRUSTUM_NNRATIO = 1.0, 0.8
# Row 0 has no observations: it takes key point 0 and does not hide it, so row 1 takes it too and is what remains; the
# later rows at (320, 240) find it held.  Rows 2 and 4 take key points 1 and 2 (5.5 px and 1 px away, r = 4 * 1.44).
FRUSTUM_KP_TO_MP = [1, 2, 4]
FRUSTUM_NMATCHES = 4  # the reference counts every assignment (:121), row 0's included


def frustum_table():
    rows = frustum_rows()
    return {"world_pos": np.array([r[1] for r in rows], F32), "normal": np.array([r[2] for r in rows], F32),
            "min_dist": np.array([r[3] for r in rows], F32), "max_dist": np.array([r[4] for r in rows], F32),
            "skip": np.array([r[5] for r in rows], np.uint8), "obs_pos": np.array([r[6] for r in rows], np.uint8),
            "desc": np.zeros((len(rows), 32), np.uint8)}


def frustum_expected():
    """(in_view, n_bad_levels, track): track[name] holds the expected value on the in-view rows, 0 elsewhere."""
    rows = frustum_rows()
    m = len(rows)
    in_view = np.zeros(m, np.uint8)
    trk = {"proj_x": np.zeros(m, F32), "proj_y": np.zeros(m, F32), "proj_xr": np.zeros(m, F32),
           "level": np.zeros(m, np.int32), "view_cos": np.zeros(m, F32)}
    nbad = 0
    for i, r in enumerate(rows):
        e = r[7]
        if e == BAD:
            nbad += 1
        elif e != OUT:
            in_view[i] = 1
            trk["proj_x"][i], trk["proj_y"][i], trk["proj_xr"][i], trk["level"][i], trk["view_cos"][i] = e
    return in_view, nbad, trk


# the same rows as three problems of different m for the batched entry point: (rows, kp_to_mp, nmatches, levels out of
# range).  Rows 0..6 hold every match of the whole list; of 7..12 row 8 (A again, position 1 of the slice) takes key
# point 0 and row 10 finds it held, and row 12 is the level 8; 13..18 are the three rows that are no number
FRUSTUM_BATCH = [(slice(0, 7), [1, 2, 4], 4, 0), (slice(7, 13), [1, -1, -1], 1, 1), (slice(13, 19), [-1, -1, -1], 0, 3)]


# ---- b. PredictScale sweep ------------------------------------------------------------------------------------------
SWEEP_KPS = [kp(600, 440, 0)]  # away from the optical axis: the sweep is about the builder, not the matching


def sweep_table(factor, n_axis=1 << 17, n_random=1 << 16, seed=5):
    """n_axis points (0, 0, z) with max_dist d floats from z * factor^k, d = -8..8, k = 0..7, so that max_dist / dist
    straddles every level's threshold; then n_random positions that are exact in float (multiples of 1/64) with any
    max_dist.  min_dist 0 and a normal along the axis keep every row past the range and angle tests."""
    rng = np.random.default_rng(seed)
    nb = n_axis // (17 * 8) + 1
    z = rng.uniform(1.0, 4.0, nb).astype(F32)
    k = np.arange(8, dtype=np.float64)[None, :, None]
    d = np.arange(-8, 9, dtype=np.int32)[None, None, :]
    target = (z.astype(np.float64)[:, None, None] * float(F32(factor)) ** k).astype(F32)
    max_axis = (np.broadcast_to(target, (nb, 8, 17)).copy().view(np.int32) + d).view(F32).reshape(-1)[:n_axis]
    z_axis = np.broadcast_to(z[:, None, None], (nb, 8, 17)).reshape(-1)[:n_axis]
    pos = np.zeros((n_axis + n_random, 3), F32)
    pos[:n_axis, 2] = z_axis
    pos[n_axis:, :2] = rng.integers(-128, 129, (n_random, 2)).astype(F32) / F32(64)
    pos[n_axis:, 2] = rng.integers(32, 385, n_random).astype(F32) / F32(64)
    m = n_axis + n_random
    normal = np.zeros((m, 3), F32)
    normal[:, 2] = 1
    max_dist = np.concatenate([max_axis, rng.uniform(1.0, 30.0, n_random).astype(F32)])
    return {"world_pos": pos, "normal": normal, "min_dist": np.zeros(m, F32), "max_dist": max_dist,
            "skip": np.zeros(m, np.uint8), "obs_pos": np.ones(m, np.uint8), "desc": np.zeros((m, 32), np.uint8)}


# The row of the key-width case as a map point, for the device builders: u = 512 * -0.84765625 * 0.5 + 320 = 103 and
# v = 512 * -0.53515625 * 0.5 + 240 = 103 exactly; dist = 2.237 and max_dist 2.5 give ratio 1.1175, 0.61: level 1;
# cos = 2 / 2.237 = 0.894: r = 4.0f * 1.2f
KEY_WIDTH_POINT = {"world_pos": np.array([[-0.84765625, -0.53515625, 2.0]], F32), "normal": np.array([TOWARDS], F32),
                   "min_dist": np.array([0.5], F32), "max_dist": np.array([2.5], F32), "skip": np.zeros(1, np.uint8),
                   "obs_pos": np.ones(1, np.uint8), "desc": np.zeros((1, 32), np.uint8)}


# ---- c. last-frame builder (ORBmatcher.cc:1328-1470) ---------------------------------------------------------------
def point_at(u, v, z=2.0):
    """The world point that the identity pose projects onto pixel (u, v): exact for integer u, v and z = 2."""
    return ((u - CX) * z / FX, (v - CY) * z / FY, z)


MB = MBF / FX  # the baseline: 0.078125
LAST_TH = 4.0  # window th * scale[octave]: 4, 4.8, 5.76
LAST_MOTIONS = {"neither": 0.0, "forward": 1.0, "backward": -1.0}  # z of tlw = tlc for an identity current pose (:1339-1349)


def last_case(motion):
    """Rows 0..3 are last-frame key points of octave 1 over current key points of octave 0, 1, 2, 3; rows 4..6 of octave 0
    over octaves 0, 1, 2.  The level window is [o-1, o+1], [o, no upper end) moving forward and [0, o] moving backward
    (:1385-1390); GetFeaturesInArea checks levels only when min > 0 or max >= 0 (Frame.cc:347), so octave 0 moving
    forward, (0, -1), checks nothing at all, and octave 0 standing still, (-1, 1), still refuses octave 2.
    Rows 7..9 lie at depth -2, -0.0 and +0 over key point 7: 1.0 / z is negative for the first two (:1367), and +0 gives
    u = 512 * 0 * inf = NaN, which passes the bounds (:1373) and finds nothing; row 10 at depth 2 takes key point 7.
    Rows 11 and 12 project onto u = 640 = max_x and u = 0 = min_x, both inside (:1373), octave 2 (r = 5.76), over key
    points 5.5 and 1 px away.  Row 13 is a NaN position: it stays a row, finds nothing and is no error.
    Returns (current key points, last dict, expected kp_to_mp)."""
    kps = [kp(100, 100, 0), kp(200, 100, 1), kp(300, 100, 2), kp(400, 100, 3), kp(100, 300, 0), kp(200, 300, 1),
           kp(300, 300, 2), kp(320, 240, 0), kp(634.5, 240, 2), kp(1, 240, 2)]
    pos = [point_at(100, 100), point_at(200, 100), point_at(300, 100), point_at(400, 100), point_at(100, 300),
           point_at(200, 300), point_at(300, 300), (0, 0, -2), (0, 0, -0.0), (0, 0, 0.0), (0, 0, 2), B, C, (NAN, 0, 2)]
    octave = [1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 2, 2, 0]
    m = len(pos)
    Tlast = np.eye(4, dtype=F32)
    Tlast[2, 3] = LAST_MOTIONS[motion]
    last = {"has_mp": np.ones(m, np.uint8), "outlier": np.zeros(m, np.uint8), "obs_pos": np.ones(m, np.uint8),
            "world_pos": np.array(pos, F32), "desc": np.zeros((m, 32), np.uint8), "kp_octave": np.array(octave, np.int32),
            "kp_angle": np.zeros(m, F32), "Tcw": Tlast}
    first7 = {"neither": [0, 1, 2, -1, 4, 5, -1], "forward": [-1, 1, 2, 3, 4, 5, 6], "backward": [0, 1, -1, -1, 4, -1, -1]}
    return kps, last, np.array(first7[motion] + [10, 11, 12], np.int32)


# ---- f. Fuse's gates (ORBmatcher.cc:825-975) and the flavours that have none ------------------------------------------
def fuse_case():
    """Six points at depth 2 with max_dist = their distance: ratio 1, level 0, r = th = 3, octave 0 only.  Fuse predicts
    ur = u - 40 * 0.5 = u - 20 and, with inv_level_sigma2[0] = 1, cuts e2 > 5.99 (mono, u_right < 0) or > 7.8 (:908-933):
      0: key point (-2, -1) away, mono: e2 = 5, kept            1: (-2, -1.5) away, mono: 6.25, cut
      2: the point projects onto u = 22, so ur = 2; key point (-2, -1) away with u_right = 0.0, which is stereo (>= 0):
         e2 = 4 + 1 + 4 = 9, cut (as mono it would have been 5 and kept)
      3: (-2, -1.5) away with u_right one short of the predicted 380: 4 + 2.25 + 1 = 7.25, kept
      4: distance 50 = TH_LOW, accepted (:950)                  5: distance 51, not
    Returns (key points, points dict, best_idx of Fuse, best_idx of the flavours without the gates)."""
    sites = [(100, 100), (200, 100), (22, 100), (400, 100), (100, 300), (200, 300)]
    kps = [kp(98, 99), kp(198, 98.5), kp(20, 99, ur=0.0), kp(398, 98.5, ur=379.0), kp(100, 300, bits=50),
           kp(200, 300, bits=51)]
    pos = np.array([point_at(u, v) for u, v in sites], F32)
    dist = np.sqrt((pos.astype(np.float64) ** 2).sum(1)).astype(F32)  # cv::norm: double, rounded
    m = len(sites)
    pts = {"bad": np.zeros(m, np.uint8), "world_pos": pos, "normal": np.tile(np.array(TOWARDS, F32), (m, 1)),
           "min_dist": dist / F32(2), "max_dist": dist, "desc": np.zeros((m, 32), np.uint8)}
    return kps, pts, np.array([0, -1, -1, 3, 4, -1], np.int32), np.array([0, 1, 2, 3, 4, -1], np.int32)


FUSE_TH = 3.0
INV_SIGMA2 = np.ones(NLEVELS, F32)


# ---- g, key-frame flavour: bestDist <= ORBdist (ORBmatcher.cc:1554) ---------------------------------------------------
ORB_DIST = 64


def keyframe_case():
    """Two points at depth 2 with max_dist = their distance (level 0, window th = 3) over key points 64 and 65 away:
    64 = ORBdist is accepted, 65 is not.  Returns (key points, kf dict, expected kp_to_mp)."""
    sites = [(100, 100), (200, 100)]
    pos = np.array([point_at(u, v) for u, v in sites], F32)
    dist = np.sqrt((pos.astype(np.float64) ** 2).sum(1)).astype(F32)
    kf = {"has_mp": np.ones(2, np.uint8), "bad": np.zeros(2, np.uint8), "already_found": np.zeros(2, np.uint8),
          "world_pos": pos, "min_dist_inv": dist / F32(2), "max_dist_inv": dist * F32(2), "max_dist": dist,
          "desc": np.zeros((2, 32), np.uint8), "kp_angle": np.zeros(2, F32)}
    return [kp(100, 100, bits=64), kp(200, 100, bits=65)], kf, np.array([0, -1], np.int32)


# ---- j. SearchForInitialization's windows (ORBmatcher.cc:405-520) ------------------------------------------------
INIT_WINDOW, INIT_NNRATIO = 15, 1.5


def init_case():
    """Rows are the level-0 key points of F1, each a window of 15 around its previous match on level 0 alone (:419-424).
      0: the only candidate is 15 away: outside (strict)        1: 14.5 away: matched
      2: a level-1 key point of F1 with the same window as 1: not a row (:420-421)
      3: the candidate under it has octave 1: refused (GetFeaturesInArea(.., 0, 0))
      4, 5, 6: two candidates 10 bits away each; `dist < bestDist` (:441) keeps the first visited, and with nnratio 1.5
         `bestDist < bestDist2 * nnratio` (:455) accepts it: cells (11, 30) after (10, 30): the second listed wins; (40, 31)
         after (40, 30): the second wins; both in cell (50, 30): the first wins.
    Returns (F1 key points, F2 key points, prev_matched, expected matches12)."""
    prev = [(100, 100), (200, 100), (200, 100), (300, 100), (101, 300), (400, 301), (500, 300)]
    f1 = [kp(x, y, 1 if i == 2 else 0) for i, (x, y) in enumerate(prev)]
    f2 = [kp(115, 100), kp(214.5, 100), kp(300, 100, 1), kp(106, 300, bits=10), kp(96, 300, bits=10),
          kp(400, 306, bits=10), kp(400, 296, bits=10), kp(500, 300, bits=10), kp(501, 300, bits=10)]
    return f1, f2, np.array(prev, F32), np.array([-1, 1, -1, -1, 4, 6, 7], np.int32)


def init_key_width_case(swapped):
    """The key-width case for SearchForInitialization, whose candidate keys are ordered on the host: all key points on
    level 0, one row at (103, 103) with a window of 5 (cells 9..11 again).  The two key points 10 away tie, the first
    visited is the best, and nnratio 1.5 accepts it against the equal second (:455)."""
    c = key_width_case(swapped)
    f2 = [kp(k[0], k[1], 0, bits=k[4]) for k in c.kps]
    return [kp(103, 103, 0)], f2, np.array([[103, 103]], F32), np.array([0 if swapped else 4097], np.int32)


def sim3_pair_case():
    """SearchBySim3 (ORBmatcher.cc:1102-1326) over the Fuse case taken as both key frames, point i being key point i's
    map point, under the identity Sim3: each direction finds key point i for point i within r = 3 with none of Fuse's
    gates, and accepts up to TH_HIGH (50 and 51 alike); both directions agree, so match12[i] = i.  With point 1 of key
    frame 1 already matched (:1129-1141) its row is skipped in direction 1 and the pair is not formed.
    Returns (key points, points, already1, expected match12 without / with already1)."""
    kps, pts, _gated, _ungated = fuse_case()
    return kps, pts, np.array([0, 1, 0, 0, 0, 0], np.uint8), np.arange(6, dtype=np.int32), np.array([0, -1, 2, 3, 4, 5], np.int32)
