"""LocalMapping::CreateNewMapPoints (LocalMapping.cc:207-452) restated in numpy under conventions N1-N13 of include/orbgpu.h
("vs CPU restatement; OpenCV boundary unpinned"), with the synthetic scenes of the tests.

Every float step is an np.float32 operation in the reference's order; the FP64 sums are Python floats.  The triangulation
has two eigen-paths, the convention's cyclic Jacobi (jacobi4: jacobi_model.jacobi_sym, the statement-for-statement twin of jacobi4_lane) and
numpy.linalg.eigh; their distance over the created points is the model's *spread*.
"""
import math

import numpy as np

from jacobi_model import JACOBI_STOP, jacobi_sym  # noqa: F401  (the one Jacobi of the models)

f32, f64 = np.float32, np.float64

(NONE, TRIANGULATED, UNPROJECT1, UNPROJECT2, LOW_PARALLAX, W_ZERO, Z1, Z2, REPROJ1, REPROJ2, ZERO_DIST, SCALE, NON_FINITE,
 STEREO_DEPTH, BAD_OCTAVE) = (0, 1, 2, 3, -1, -2, -3, -4, -5, -6, -7, -8, -9, -10, -11)
TH_LOW, HISTO_LENGTH = 50, 30
JACOBI_SWEEPS = 30
EPS32 = float(np.finfo(f32).eps)

# ---- what is compared ------------------------------------------------------------------------------------------------------
BOUND_FACTOR = 16.0   # the project's factor: x3d agrees within BOUND_FACTOR x spread (bit for bit at spread 0)
LEFT_OUT_CAP = 0.10   # the project's cap on the share of matched pairs that is not compared
# From the bound B = BOUND_FACTOR x spread (on |a - b| / max(1, |a|) of a created point's coordinates) to the gate
# quantities, in make_scene()'s geometry: world coordinates within 12.5 of the origin except the far points, which can only
# meet the parallax gate (below); depth in both cameras >= 2; fx = fy = 500; level_sigma2 >= 1; rotations orthonormal.
#   * a world coordinate moves by at most 12.5 B, a camera-frame coordinate by sqrt(3) x that < 22 B (a row of R has
#     1-norm <= sqrt 3): Z_MARGIN = 22 B absolute on z1 and z2 (their own rounding, 6e-8 x 12.5, is below B for any B > 0
#     the scenes give, and for B = 0 the device and the model do the same IEEE operations);
#   * a pixel moves by at most fx / z (1 + |x / z|) x 22 B <= 500 / 2 x 2 x 22 B = 1.1e4 B, u_r by mbf / z^2 x 22 B = 220 B more;
#     err2 = d'd moves by 2 |d| times that, so err2 / (k sigma2) at the threshold (|d| = sqrt(k sigma2) >= sqrt 5.991 = 2.44)
#     by 2 x 1.13e4 B / 2.44 < 1e4 B: REPROJ_MARGIN_FACTOR on |err2 / (k sigma2) - 1|;
#   * a distance moves by at most 22 B and is >= 2, a quotient of two of them relatively by 22 B, and the four float
#     roundings of the test add 4 eps: RATIO_MARGIN = 22 B + 4 eps on |lhs / rhs - 1| of either side of :430;
#   * the parallax cosine does not depend on the point at all: it is IEEE arithmetic on the inputs, the same on the device
#     and here (FP64 sums, sqrt and quotient, one rounding to float).  COS_MARGIN = 4 eps, a guard of a few float steps
#     against 0, 0.9998 and cosParallaxStereo, is all it gets.
Z_MARGIN_FACTOR = 22.0
REPROJ_MARGIN_FACTOR = 1.0e4
RATIO_MARGIN_FACTOR = 22.0
COS_MARGIN = 4 * EPS32


def dev(a, b):
    """largest |a - b| / max(1, |a|)"""
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    if a.size == 0:
        return 0.0
    with np.errstate(all="ignore"):
        d = np.abs(a - b) / np.maximum(1.0, np.abs(a))
    return float(np.nan_to_num(d, nan=np.inf).max())


# ---- N1: ORBmatcher::SearchForTriangulation as k_tri_match / k_tri_finish compute it ------------------------------------
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def three_maxima(histo):
    max1 = max2 = max3 = 0
    i1 = i2 = i3 = -1
    for i, s in enumerate(histo):
        if s > max1:
            max3, max2, max1, i3, i2, i1 = max2, max1, s, i2, i1, i
        elif s > max2:
            max3, max2, i3, i2 = max2, s, i2, i
        elif s > max3:
            max3, i3 = s, i
    if f32(max2) < f32(0.1) * f32(max1):
        i2 = i3 = -1
    elif f32(max3) < f32(0.1) * f32(max1):
        i3 = -1
    return i1, i2, i3


def rot_bin(a, b):
    rot = f32(a) - f32(b)
    if rot < 0:
        rot = rot + f32(360.0)
    v = float(rot * (f32(1.0) / f32(HISTO_LENGTH)))
    b = int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)  # roundf: half away from zero
    return 0 if b == HISTO_LENGTH else b


def match(kf1, has1, kf2, only_stereo, check_ori):
    """(match12 [n1], nmatches) of key frame 1 against neighbour kf2 with has1 as key frame 1's has_mp"""
    n1, n2 = len(kf1["kp_x"]), len(kf2["kp_x"])
    out = np.full(n1, -1, np.int32)
    if n1 == 0 or n2 == 0:
        return out, 0
    F = np.asarray(kf2["F12"], f32).reshape(9)
    ex, ey = f32(kf2["ex"]), f32(kf2["ey"])
    sg, sc = np.asarray(kf2["level_sigma2"], f32), np.asarray(kf2["scale_factors"], f32)
    x2, y2, o2 = kf2["kp_x"], kf2["kp_y"], kf2["kp_octave"]
    st2 = kf2["u_right"] >= 0
    free2 = (kf2["has_mp"] == 0) & (st2 if only_stereo else True)
    with np.errstate(all="ignore"):
        for i in range(n1):
            nd = kf1["node"][i]
            s1 = kf1["u_right"][i] >= 0
            if nd < 0 or has1[i] or (only_stereo and not s1):
                continue
            cand = np.nonzero((kf2["node"] == nd) & free2)[0]
            if cand.size == 0:
                continue
            dist = _POP[kf1["desc"][i][None, :] ^ kf2["desc"][cand]].sum(1)
            kx, ky = kf1["kp_x"][i], kf1["kp_y"][i]
            la = kx * F[0] + ky * F[3] + F[6]
            lb = kx * F[1] + ky * F[4] + F[7]
            lc = kx * F[2] + ky * F[5] + F[8]
            den = la * la + lb * lb
            best, bd = -1, None
            for j, d in zip(cand, dist):
                if d > TH_LOW:
                    continue
                px, py, o = x2[j], y2[j], o2[j]
                if not s1 and not st2[j]:
                    dex, dey = ex - px, ey - py
                    if dex * dex + dey * dey < f32(100) * sc[o]:
                        continue
                num = la * px + lb * py + lc
                if den == 0:
                    continue
                dsqr = num * num / den
                if not (float(dsqr) < 3.84 * float(sg[o])):
                    continue
                if bd is None or d <= bd:  # least distance, the largest index among equals
                    best, bd = j, d
            out[i] = best
    if check_ori:
        histo = [0] * HISTO_LENGTH
        bins = {}
        for i in np.nonzero(out >= 0)[0]:
            bins[i] = rot_bin(kf1["kp_angle"][i], kf2["kp_angle"][out[i]])
            histo[bins[i]] += 1
        keep = three_maxima(histo)
        for i, b in bins.items():
            if b not in keep:
                out[i] = -1
    return out, int((out >= 0).sum())


# ---- N5: the 4 x 4 null vector ------------------------------------------------------------------------------------------------
def jacobi4(A):
    """jacobi4_lane at null_vector4's sweep count; A (list of lists of Python floats) is overwritten; returns V"""
    return jacobi_sym(A, JACOBI_SWEEPS)


def null_vector4(Af, eig="jacobi"):
    """the float null vector of the float 4 x 4 Af as null_vector4 (jacobi.h) forms it"""
    A = [[0.0] * 4 for _ in range(4)]
    for a in range(4):
        for b in range(4):
            s = 0.0
            for r in range(4):
                s = s + float(Af[r][a]) * float(Af[r][b])
            A[a][b] = s
    if eig == "eigh":
        w, U = np.linalg.eigh(np.array(A, f64))
        v = [float(x) for x in U[:, 0]]
    else:
        V = jacobi4(A)
        v = [0.0] * 4
        for i in range(4):
            rank = 0
            for j in range(4):
                if j < i:
                    rank += not (A[j][j] < A[i][i])
                elif j > i:
                    rank += A[j][j] > A[i][i]
            if rank >= 3:
                v = [V[0][i], V[1][i], V[2][i], V[3][i]]
    big, lead = abs(v[0]), v[0]
    for r in range(1, 4):
        if abs(v[r]) > big:
            big, lead = abs(v[r]), v[r]
    if lead < 0.0:
        v = [-x for x in v]
    return [f32(x) for x in v]


# ---- N2-N10: one matched pair -----------------------------------------------------------------------------------------------------
def _fdiv(a, b):
    with np.errstate(all="ignore"):
        return f32(f64(a) / f64(b))


def _row(T, o, X):
    """(float)(Mat::dot(T's row, X) + (double)t)"""
    return f32(((float(T[o]) * float(X[0]) + float(T[o + 1]) * float(X[1])) + float(T[o + 2]) * float(X[2])) + float(T[o + 3]))


def _norm3(v):
    return f32(math.sqrt((float(v[0]) * float(v[0]) + float(v[1]) * float(v[1])) + float(v[2]) * float(v[2])))


def _unproject(K, i):
    z = K["depth"][i]
    if not (z > 0):
        return None
    raw = K.get("kp_raw")
    u, v = (K["kp_x"][i], K["kp_y"][i]) if raw is None else (raw[i][0], raw[i][1])
    cam = K["cam"]
    x, y = ((u - cam["cx"]) * z) * cam["invfx"], ((v - cam["cy"]) * z) * cam["invfy"]
    T = K["Twc"]
    return [((T[4 * r] * x + T[4 * r + 1] * y) + T[4 * r + 2] * z) + T[4 * r + 3] for r in range(3)]


def _prep(K):
    """float32 views of a frame dict's scalars, cached"""
    if "cam" not in K:
        fx, fy, cx, cy = (f32(v) for v in K["K"])
        K["cam"] = {"fx": fx, "fy": fy, "cx": cx, "cy": cy, "invfx": f32(K.get("invfx", f32(1.0) / fx)),
                    "invfy": f32(K.get("invfy", f32(1.0) / fy)), "mbf": f32(K.get("mbf", 0.0))}
        K["Tcw"] = np.asarray(K["Tcw"], f32).reshape(16)
        K["Twc"] = np.asarray(K["Twc"], f32).reshape(16)
        K["level_sigma2"] = np.asarray(K["level_sigma2"], f32)
        K["scale_factors"] = np.asarray(K["scale_factors"], f32)
    return K


def pair(K1, K2, ratio_factor, i, j, eig="jacobi", mut=None):
    """(status, x3d [3] float32 (zeros unless status > 0), gates): gates maps each gate quantity the pair reached to
    (value, kind), the distance measures near() reads.  mut: one of the mutations tests/test_newpts_model.py catches."""
    _prep(K1), _prep(K2)
    with np.errstate(all="ignore"):
        return _pair(K1, K2, f32(ratio_factor), i, j, eig, mut)


def _pair(K1, K2, rf, i, j, eig, mut):
    zero = np.zeros(3, f32)
    g = {}
    o1, o2 = int(K1["kp_octave"][i]), int(K2["kp_octave"][j])
    if not (0 <= o1 < len(K1["level_sigma2"]) and 0 <= o2 < len(K2["level_sigma2"])):
        return BAD_OCTAVE, zero, g
    c1, c2 = K1["cam"], K2["cam"]
    px1, py1, ur1 = K1["kp_x"][i], K1["kp_y"][i], K1["u_right"][i]
    px2, py2, ur2 = K2["kp_x"][j], K2["kp_y"][j], K2["u_right"][j]
    s1, s2 = bool(ur1 >= 0), bool(ur2 >= 0)
    T1, T2 = K1["Tcw"], K2["Tcw"]
    one = f32(1.0)
    xn1 = [(px1 - c1["cx"]) * c1["invfx"], (py1 - c1["cy"]) * c1["invfy"], one]
    xn2 = [(px2 - c2["cx"]) * c2["invfx"], (py2 - c2["cy"]) * c2["invfy"], one]
    r1 = [(T1[r] * xn1[0] + T1[4 + r] * xn1[1]) + T1[8 + r] * xn1[2] for r in range(3)]
    r2 = [(T2[r] * xn2[0] + T2[4 + r] * xn2[1]) + T2[8 + r] * xn2[2] for r in range(3)]
    dot = (float(r1[0]) * float(r2[0]) + float(r1[1]) * float(r2[1])) + float(r1[2]) * float(r2[2])
    n1 = math.sqrt((float(r1[0]) ** 2 + float(r1[1]) ** 2) + float(r1[2]) ** 2)
    n2 = math.sqrt((float(r2[0]) ** 2 + float(r2[1]) ** 2) + float(r2[2]) ** 2)
    cos_rays = f32(dot / (n1 * n2)) if n1 * n2 != 0 else f32(np.nan)
    cs = cos_rays + one
    cs1 = cs2 = cs
    if s1:
        cs1 = K1["cos_stereo"][i]
    elif s2:
        cs2 = K2["cos_stereo"][j]
    if mut == "cos2_always" and s2:
        cs2 = K2["cos_stereo"][j]
    cs_min = cs2 if cs2 < cs1 else cs1
    g["cos_stereo"] = (float(cos_rays) - float(cs_min), "abs")
    g["cos_zero"] = (float(cos_rays), "abs")
    if not (s1 or s2):
        g["cos_9998"] = (float(cos_rays) - 0.9998, "abs")
    if s1 or s2:
        g["cos_12"] = (float(cs1) - float(cs2), "abs")
    if cos_rays < cs_min and cos_rays > 0 and (s1 or s2 or float(cos_rays) < 0.9998):
        Af = [[xn1[0] * T1[8 + c] - T1[c] for c in range(4)], [xn1[1] * T1[8 + c] - T1[4 + c] for c in range(4)],
              [xn2[0] * T2[8 + c] - T2[c] for c in range(4)], [xn2[1] * T2[8 + c] - T2[4 + c] for c in range(4)]]
        x4 = null_vector4(Af, eig)
        if x4[3] == 0:
            return W_ZERO, zero, g
        X = [_fdiv(x4[0], x4[3]), _fdiv(x4[1], x4[3]), _fdiv(x4[2], x4[3])]
        made = TRIANGULATED
    elif s1 and cs1 < cs2:
        X = _unproject(K1, i)
        made = UNPROJECT1
    elif s2 and cs2 < cs1:
        X = _unproject(K2, j)
        made = UNPROJECT2
    else:
        return LOW_PARALLAX, zero, g
    if X is None:
        return STEREO_DEPTH, zero, g
    if not all(np.isfinite(X)):
        return NON_FINITE, zero, g
    z1 = _row(T1, 8, X)
    g["z1"] = (float(z1), "z")
    if z1 <= 0:
        return Z1, zero, g
    z2 = _row(T2, 8, X)
    g["z2"] = (float(z2), "z")
    if z2 <= 0:
        return Z2, zero, g
    mono_th, stereo_th = (7.8, 5.991) if mut == "thresholds_swapped" else (5.991, 7.8)
    for which, K, T, cam, z, px, py, ur, st, o, code in (("e1", K1, T1, c1, z1, px1, py1, ur1, s1, o1, REPROJ1),
                                                         ("e2", K2, T2, c2, z2, px2, py2, ur2, s2, o2, REPROJ2)):
        sg = float(K["level_sigma2"][o])
        xc, yc = _row(T, 0, X), _row(T, 4, X)
        invz = f32(1.0 / float(z))
        u, v = (cam["fx"] * xc) * invz + cam["cx"], (cam["fy"] * yc) * invz + cam["cy"]
        ex, ey = u - px, v - py
        if not st:
            e2, th = ex * ex + ey * ey, mono_th * sg
        else:
            mbf = c2["mbf"] if (mut == "own_mbf" and which == "e2") else c1["mbf"]
            er = (u - mbf * invz) - ur
            e2, th = (ex * ex + ey * ey) + er * er, stereo_th * sg
        g[which] = (float(e2) / th - 1.0 if th > 0 else np.inf, "reproj")
        if float(e2) > th:
            return code, zero, g
    Tw1, Tw2 = K1["Twc"], K2["Twc"]
    d1 = _norm3([X[0] - Tw1[3], X[1] - Tw1[7], X[2] - Tw1[11]])
    d2 = _norm3([X[0] - Tw2[3], X[1] - Tw2[7], X[2] - Tw2[11]])
    if d1 == 0 or d2 == 0:
        return ZERO_DIST, zero, g
    ratio_dist = _fdiv(d2, d1)
    ratio_octave = _fdiv(K1["scale_factors"][o1], K2["scale_factors"][o2])
    lo, hi = ratio_dist * rf, ratio_octave * rf
    g["ratio_lo"] = (float(lo) / float(ratio_octave) - 1.0, "ratio")
    g["ratio_hi"] = (float(ratio_dist) / float(hi) - 1.0, "ratio")
    if (lo < ratio_octave and mut != "ratio_one_sided") or ratio_dist > hi:
        return SCALE, zero, g
    return made, np.array(X, f32), g


def near(gates, bound):
    """a gate quantity of the pair lies within its margin (derived from bound = BOUND_FACTOR x spread, see the constants)"""
    m = {"abs": COS_MARGIN, "z": Z_MARGIN_FACTOR * bound, "reproj": REPROJ_MARGIN_FACTOR * bound,
         "ratio": RATIO_MARGIN_FACTOR * bound + 4 * EPS32}
    return any(abs(v) <= m[kind] for v, kind in gates.values())


# ---- the chain -----------------------------------------------------------------------------------------------------------
def run(scene, eig="jacobi", mut=None, stop=0):
    """The whole neighbour loop on the model's own upstream: dict of match12, status, x3d, n_matches, n_created, n_done and
    gates[k][i]."""
    kf1, nbs = scene["kf1"], scene["neighbours"]
    nn, n1 = len(nbs), len(kf1["kp_x"])
    out = {"match12": np.full((nn, n1), -1, np.int32), "status": np.zeros((nn, n1), np.int32), "x3d": np.zeros((nn, n1, 3), f32),
           "n_matches": np.zeros(nn, np.int32), "n_created": np.zeros(nn, np.int32), "n_done": 0, "gates": [dict() for _ in range(nn)]}
    has = np.array(kf1["has_mp"], np.uint8).copy()
    for k, K2 in enumerate(nbs):
        if k > 0 and stop:
            break
        out["n_done"] = k + 1
        m, nm = match(kf1, has, K2, scene["only_stereo"], scene["check_ori"])
        out["match12"][k], out["n_matches"][k] = m, nm
        for i in np.nonzero(m >= 0)[0]:
            st, X, g = pair(kf1, K2, scene["ratio_factor"], i, m[i], eig, mut)
            out["status"][k, i], out["x3d"][k, i], out["gates"][k][i] = st, X, g
            if st > 0 and mut != "no_has_mp_update":
                has[i] = 1
        out["n_created"][k] = int((out["status"][k] > 0).sum())
    return out


def model_pass(scene):
    """(model, spread, near mask [nn][n1], matched pairs): the model with its Jacobi, its distance from itself with eigh on
    the same matches over the points both created, and the pairs that lie near a threshold at BOUND_FACTOR x spread"""
    m = run(scene)
    spread = 0.0
    for k, K2 in enumerate(scene["neighbours"]):
        for i in np.nonzero(m["status"][k] == TRIANGULATED)[0]:
            st, X, _ = pair(scene["kf1"], K2, scene["ratio_factor"], i, m["match12"][k, i], "eigh")
            if st == TRIANGULATED:
                spread = max(spread, dev(m["x3d"][k, i], X))
    bound = BOUND_FACTOR * spread
    nr = np.zeros(m["status"].shape, bool)
    for k in range(len(scene["neighbours"])):
        for i, g in m["gates"][k].items():
            nr[k, i] = near(g, bound)
    return m, spread, nr, int((m["match12"] >= 0).sum())


def compare(scene, d, bound):
    """The device's outputs d against the model, every stage on the device's own upstream output (the method of
    tests/init_fp64.py): neighbour k's matches from has_mp1 OR the device's statuses of neighbours < k (so a left-out pair's
    device status is taken as given), neighbour k's pairs from the device's matches.  Returns the figures; raises
    AssertionError on a difference outside the margins."""
    kf1, nbs = scene["kf1"], scene["neighbours"]
    nn, n1 = len(nbs), len(kf1["kp_x"])
    has = np.array(kf1["has_mp"], np.uint8).copy()
    left = matched = 0
    x_dev = 0.0
    assert d["n_done"] == nn
    for k, K2 in enumerate(nbs):
        m, nm = match(kf1, has, K2, scene["only_stereo"], scene["check_ori"])
        assert np.array_equal(m, d["match12"][k]), "neighbour %d: match12 differs at %s" % (k, np.nonzero(m != d["match12"][k])[0][:8])
        assert nm == d["n_matches"][k]
        assert d["n_created"][k] == int((d["status"][k] > 0).sum())
        for i in range(n1):
            if m[i] < 0:
                assert d["status"][k, i] == NONE and not d["x3d"][k, i].any()
                continue
            matched += 1
            st, X, g = pair(kf1, K2, scene["ratio_factor"], i, m[i])
            if near(g, bound):
                left += 1
            else:
                assert st == d["status"][k, i], "neighbour %d key point %d: status %d, model %d" % (k, i, d["status"][k, i], st)
                if bound == 0:
                    assert X.tobytes() == d["x3d"][k, i].tobytes()
                else:
                    assert dev(X, d["x3d"][k, i]) <= bound
                x_dev = max(x_dev, dev(X, d["x3d"][k, i]))
            if d["status"][k, i] <= 0:
                assert not d["x3d"][k, i].any()
        has |= (d["status"][k] > 0).astype(np.uint8)
    assert left <= LEFT_OUT_CAP * max(matched, 1), "%d of %d pairs left out" % (left, matched)
    return {"left_out": left, "matched": matched, "x3d_deviation": x_dev}


# ---- scenes ----------------------------------------------------------------------------------------------------------------
FX, FY, CX, CY, MB = 500.0, 500.0, 320.0, 240.0, 0.08
NLEVELS, SCALE_FACTOR = 8, 1.2


def levels():
    sf = [f32(1.0)]
    for _ in range(1, NLEVELS):
        sf.append(sf[-1] * f32(SCALE_FACTOR))
    sf = np.array(sf, f32)
    return sf, sf * sf


def _rot(rx, ry, rz):
    cx_, sx, cy_, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx_, -sx], [0, sx, cx_]])
    Ry = np.array([[cy_, 0, sy], [0, 1, 0], [-sy, 0, cy_]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def _pose(R, C):
    """Tcw and Twc in float32 as KeyFrame::SetPose leaves them: Twc from the float Tcw, Ow = -Rwc tcw in float"""
    T = np.eye(4, dtype=f32)
    T[:3, :3] = R.astype(f32)
    T[:3, 3] = (-R @ C).astype(f32)
    Twc = np.eye(4, dtype=f32)
    Rwc = T[:3, :3].T
    Twc[:3, :3] = Rwc
    t = T[:3, 3]
    for r in range(3):
        Twc[r, 3] = -((Rwc[r, 0] * t[0] + Rwc[r, 1] * t[1]) + Rwc[r, 2] * t[2])
    return T, Twc


def _frame(rng, pts, descs, angles, R, C, n, mix, noise, order_seed, has_frac, spoil_ur=0.0, wrong_octave=0.0, raw_offset=None):
    """n observations of the points (a random subset in a random order); mix: 'mono', 'stereo' or 'mixed'"""
    T, Twc = _pose(R, C)
    sel = np.random.default_rng(order_seed).permutation(len(pts))[:n]
    n = len(sel)  # at most one observation per point
    Xc = (R @ (pts[sel] - C).T).T
    z = Xc[:, 2]
    u = FX * Xc[:, 0] / z + CX + noise * rng.standard_normal(n)
    v = FY * Xc[:, 1] / z + CY + noise * rng.standard_normal(n)
    octv = np.clip(np.round(np.log(np.maximum(z, 1e-3) / 4.0) / math.log(SCALE_FACTOR)), 0, NLEVELS - 1).astype(np.int32)
    bad = rng.random(n) < wrong_octave
    octv = np.where(bad, (octv + 4) % NLEVELS, octv).astype(np.int32)
    stereo = {"mono": np.zeros(n, bool), "stereo": np.ones(n, bool), "mixed": rng.random(n) < 0.5}[mix] & (z < 40)
    stereo &= u - FX * MB / z > 8  # the right image sees it
    depth = np.where(stereo, z * (1 + 0.002 * noise * rng.standard_normal(n)), -1.0).astype(f32)
    ur = np.where(stereo, u - FX * MB / z + noise * rng.standard_normal(n), -1.0)
    ur = np.where(stereo & (rng.random(n) < spoil_ur), ur - 6.0, ur).astype(f32)
    ur = np.where(stereo, np.maximum(ur, 0), -1).astype(f32)
    desc = descs[sel].copy()
    for r in range(n):  # a few flipped bits per view
        for b in rng.integers(0, 256, rng.integers(0, 9)):
            desc[r, b >> 3] ^= np.uint8(1 << (b & 7))
    sf, sg = levels()
    with np.errstate(all="ignore"):
        cs = np.cos(f32(2) * np.arctan2(f32(MB) / f32(2), depth)).astype(f32)
    ang = (angles[sel] + 2.0 * rng.standard_normal(n)) % 360.0
    odd = rng.random(n) < 0.05
    ang = np.where(odd, (ang + 170.0) % 360.0, ang)
    return {"kp_x": u.astype(f32), "kp_y": v.astype(f32), "kp_octave": octv, "kp_angle": ang.astype(f32), "u_right": ur,
            "desc": np.ascontiguousarray(desc), "has_mp": (rng.random(n) < has_frac).astype(np.uint8),
            "node": (sel // 4).astype(np.int32), "depth": depth, "cos_stereo": cs,
            # mvKeys: the distorted key points KeyFrame::UnprojectStereo reads, here a fixed shift of mvKeysUn
            "kp_raw": None if raw_offset is None else (np.column_stack([u, v]) + np.asarray(raw_offset)).astype(f32),
            "Tcw": T.reshape(16), "Twc": Twc.reshape(16), "K": (FX, FY, CX, CY), "mbf": FX * MB, "level_sigma2": sg,
            "scale_factors": sf, "point": sel, "R": R, "C": C}


def _skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def _epipolar(K1, K2):
    """LocalMapping::ComputeF12 and the epipole of ORBmatcher.cc:664-670 (the caller's work: FP64 here, rounded to float)"""
    R1, C1, R2, C2 = K1["R"], K1["C"], K2["R"], K2["C"]
    t1, t2 = -R1 @ C1, -R2 @ C2
    R12 = R1 @ R2.T
    t12 = -R12 @ t2 + t1
    Km = np.array([[FX, 0, CX], [0, FY, CY], [0, 0, 1.0]])
    F12 = np.linalg.inv(Km).T @ _skew(t12) @ R12 @ np.linalg.inv(Km)
    c2 = R2 @ C1 + t2
    with np.errstate(all="ignore"):
        K2["F12"] = (F12 / np.abs(F12).max()).astype(f32).reshape(9)
        K2["ex"], K2["ey"] = f32(FX * c2[0] / c2[2] + CX), f32(FY * c2[1] / c2[2] + CY)


def make_scene(seed, mix="mono", n1=150, n2=(97, 130, 130), noise=0.5, n_points=160, has_frac=0.15, far=12, spoil_ur=0.08,
               wrong_octave=0.03, only_stereo=False, check_ori=True, all_has=False, strangers=(), raw_offset=None):
    """nn + 1 cameras with real baselines over n_points 3D points (the last `far` of them too far for mono parallax).
    strangers: neighbours whose descriptors are unrelated (no match)."""
    rng = np.random.default_rng(seed)
    pts = np.column_stack([rng.uniform(-4, 4, n_points), rng.uniform(-3, 3, n_points), rng.uniform(4.5, 11.5, n_points)])
    if far:
        pts[-far:, 2] = rng.uniform(60, 90, far)
    descs = rng.integers(0, 256, (n_points, 32), dtype=np.uint8)
    angles = rng.uniform(0, 360, n_points)
    kf1 = _frame(rng, pts, descs, angles, _rot(0.01, -0.02, 0.005), np.array([0.05, -0.02, 0.1]), n1, mix, noise, seed * 7 + 1,
                 1.0 if all_has else has_frac, spoil_ur=spoil_ur / 2, wrong_octave=wrong_octave, raw_offset=raw_offset)
    nbs = []
    for k, n in enumerate(n2):
        a = 2.1 * k + 0.4
        C = np.array([0.7 * math.cos(a), 0.45 * math.sin(a), 0.25 + 0.1 * k])
        if k == 2:  # barely beyond the stereo baseline: the stereo branches of :340-347 and an epipole inside the image
            C = kf1["C"] + np.array([0.06, 0.03, 0.07])
        d = rng.integers(0, 256, (n_points, 32), dtype=np.uint8) if k in strangers else descs
        nb = _frame(rng, pts, d, angles, _rot(0.02 * math.sin(a), 0.03 * math.cos(a), 0.01 * k), C, n, mix, noise,
                    seed * 7 + 2 + k, has_frac, spoil_ur=spoil_ur if k == 0 else 0.0, wrong_octave=wrong_octave, raw_offset=raw_offset)
        _epipolar(kf1, nb)
        nbs.append(nb)
    return {"kf1": kf1, "neighbours": nbs, "ratio_factor": f32(1.5) * f32(SCALE_FACTOR), "only_stereo": only_stereo,
            "check_ori": check_ori, "points": pts}


# the scenes of the parity tests: name -> make_scene's arguments
SCENES = {
    "mono": dict(seed=11, mix="mono"),
    "stereo": dict(seed=12, mix="stereo"),
    "mixed": dict(seed=13, mix="mixed"),
    "mixed/only_stereo": dict(seed=14, mix="mixed", only_stereo=True, check_ori=False),
    "nn=1": dict(seed=15, mix="mixed", n2=(130,)),
    "n1=0": dict(seed=16, mix="mono", n1=0),
    "n2=0": dict(seed=17, mix="mixed", n2=(97, 0, 130)),
    "no match": dict(seed=18, mix="mixed", strangers=(1,)),
    "all has_mp1": dict(seed=19, mix="stereo", all_has=True),
    "mixed/raw": dict(seed=20, mix="mixed", raw_offset=(1.5, -0.75)),  # mvKeys differ from mvKeysUn (N6)
}


def scene(name):
    return make_scene(**SCENES[name])
