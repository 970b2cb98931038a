"""A ladder of float64 checks of the Initializer (include/orbgpu.h I1-I10), one stage at a time: every rung takes a result
as tools/fuzz_init.download gives it and checks one stage on the result's OWN output of the stage before, so the
sensitivity of an ill-conditioned null vector never enters and nothing is left out but single pairs within float rounding
of a threshold.  Plain numpy / numpy.linalg in float64, written from the operations' definitions (Initializer.cc and the
header), not from tests/init_model.py: of that file only the scene makers and prepare() (the compaction of I1, and T1 / T2
as data) are used.  DESIGN.md section 9.23 has the reasoning and the table of figures.

Every rung returns (violations: list of strings, figures: dict of the largest values it measured).  The tolerances TOL_*
are 16 x (the project's BOUND_FACTOR) the largest figure tests/test_init_fp64.py measures with the restatement standing
where the device stands, rounded up to one digit: the restatement shows what the specified float rounding costs against
float64, the factor leaves room for a different but legal summation inside the device's Jacobi.  The margins and the caps
are conditions, derived here and not tuned."""
import math

import numpy as np

from init_model import make_scene, ngood_scene, parity_scene, prepare

f64 = np.float64
TH_H, TH_F, TH_SCORE = 5.991, 3.841, 5.991
COS_GOOD = 0.99998
BOUND_FACTOR = 16.0

# A transferred coordinate carries about 1e-4 px of float rounding and |d| = 2.4 px at the threshold, so chiSquare moves by
# about 1e-4 relative: ten times that.  The same margin serves the reprojection test of CheckRT.
MARGIN_CHI = 1e-3
MARGIN_COS = 1e-7          # of cosParallax / 0.99998: a float cosine's rounding
MARGIN_Z = 1e-6            # a depth this close to 0 has no sign to speak of
CAP_SKIPPED = 0.005        # of a scene's (hypothesis, pair) cells
CAP_MATRIXLESS = 0.10      # of a scene's 2 H hypotheses: a score of 0 exports no matrix, at the scene's sigma or WIDE_SIGMA

# 16 x the restatement's largest figure, one digit, rounded up (tests/test_init_fp64.py asserts that they are)
TOL_RAY = 8e-13            # rungs 1, 2: Rayleigh quotient above lambda_min, relative to lambda_max
TOL_RANK = 2e-5            # rung 2: sigma_3 / sigma_1 of Fn
TOL_SCORE = 3e-2           # rung 3: |score - score64| / max(1, score64)
TOL_SCORE_PX = 6e-3        # rung 3: the same difference over the sum of 2 sqrt(chiSquare) / sigma of the inliers' terms: pixels
TOL_ORTH = 6e-6            # rung 5: R'R - I, | |t| - 1 |
TOL_RT = 8e-7              # rung 5 (F): R21 against U W V' / U W' V', t21 against +-u3
TOL_RANK1 = 9e-6           # rung 5 (H): sigma_2 / sigma_1 of s A / d2 - R21
TOL_ALIGN = 7e-12          # rung 5 (H): 1 - |cos| between t21 and the first left singular vector of that matrix
TOL_PT = 2e-5              # rung 6: |P3D - X64| gap / |X|
TOL_COS = 2e-6             # rung 6: the selected cosine
TOLERANCES = {"ray": "TOL_RAY", "rank": "TOL_RANK", "score": "TOL_SCORE", "score_px": "TOL_SCORE_PX", "orth": "TOL_ORTH", "rt": "TOL_RT",
              "rank1": "TOL_RANK1", "align": "TOL_ALIGN", "pt": "TOL_PT", "cos": "TOL_COS"}   # figure -> its constant


def round_up_one_digit(x):
    """the smallest d x 10^e (d = 1..9) that is >= x"""
    if not x > 0.0:
        return 0.0
    e = math.floor(math.log10(x))
    d = math.ceil(x / 10.0 ** e - 1e-9)
    return float("%de%d" % (d, e)) if d < 10 else float("1e%d" % (e + 1))


# ---- scenes ------------------------------------------------------------------------------------------------------------
TABLE = (("general", 300, 101), ("general", 300, 104), ("planar", 300, 103), ("planar", 300, 107), ("rotation", 300, 105),
         ("rotation", 65, 103), ("general", 65, 100), ("planar", 65, 107))
KINDS = ("general", "planar", "rotation", "few")
DEGENERATE = "general-300-101-repeated"


def scenes():
    """name -> scene: N <= 300, 24 hypotheses, the seeds as written (none is searched for)"""
    out = {}
    for kind, n, seed in TABLE:
        out["%s-%d-%d" % (kind, n, seed)] = make_scene(n, seed, kind, n_hyp=24)
    for i, n in enumerate((8, 9, 63, 64, 65, 129)):     # the minimal set, both sides of a mask word, two words and one
        out["edge-%d-%s" % (n, KINDS[i % 4])] = make_scene(n, 555 + i, KINDS[i % 4], n_hyp=24, noise_px=(0.3, 1.0)[i % 2],
                                                          outlier_frac=(0.1, 0.3)[i % 2])
    out["parity-planar"] = parity_scene("planar")       # an H-branch success
    out["ngood-51"] = ngood_scene(51)                   # the rank clamp min(50, nGood - 1)
    rep = make_scene(300, 101, "general", n_hyp=24)
    rep["sets"][2] = 8                                  # one pair eight times
    out[DEGENERATE] = rep
    out["general-300-101-sigma2"] = dict(make_scene(300, 101, "general", n_hyp=24), sigma=2.0)
    return out


WIDE_SIGMA = 1024.0   # every transfer inside the image is an inlier's: a finite hypothesis wins alone and shows its matrix


def with_copies(sc):
    """the scene, then one copy per hypothesis that holds that hypothesis alone (copy h's result carries hypothesis h's
    matrices, which the ABI exports for the winners only), then the same copies with WIDE_SIGMA: a matrix does not depend
    on sigma (I3, I4), and with the scene's own a hypothesis that fits no pair scores 0 and exports none"""
    sets = np.asarray(sc["sets"], np.int32).reshape(-1, 8)
    alone = [dict(sc, sets=sets[h:h + 1].copy()) for h in range(len(sets))]
    return [sc] + alone + [dict(c, sigma=WIDE_SIGMA) for c in alone]


def split_copies(results):
    """(the scene's result, copies, wide copies) of with_copies' batch"""
    H = (len(results) - 1) // 2
    return results[0], results[1:1 + H], results[1 + H:]


# ---- helpers -----------------------------------------------------------------------------------------------------------
def unpack(words, n):
    bits = np.unpackbits(np.ascontiguousarray(words, np.uint64).view(np.uint8), bitorder="little")
    return bits[:n].astype(bool), bool(bits[n:].any())


def _kmat(sc):
    fx, fy, cx, cy = (float(np.float32(k)) for k in sc["K"])
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], f64)


def _sigma(sc):
    return float(np.float32(sc.get("sigma", 1.0)))


def _tmat(T):
    sx, sy, tx, ty = (float(v) for v in T)
    return np.array([[sx, 0, tx], [0, sy, ty], [0, 0, 1]], f64)


def _normalised(prep, idx):
    """the set's pairs under T1, T2 (I3's matrices, taken as data) in float64: u1, v1, u2, v2"""
    p = prep["pts"][np.asarray(idx, np.int64)].astype(f64)
    T1, T2 = prep["T1"].astype(f64), prep["T2"].astype(f64)
    return p[:, 0] * T1[0] + T1[2], p[:, 1] * T1[1] + T1[3], p[:, 2] * T2[0] + T2[2], p[:, 3] * T2[1] + T2[3]


def _up(fig, key, value):
    fig[key] = max(fig.get(key, 0.0), float(value))


def hypotheses(r, copies, wide=None):
    """what is known of every hypothesis: from the single-hypothesis copies when given ([H] results; wide: the same copies
    run with WIDE_SIGMA, whose matrix stands in where the scene's own sigma leaves a score of 0 and so exports none),
    otherwise the two winners only.  A list of (model 'h' / 'f', index, 3x3 matrix, score, mask row); a hypothesis without
    a matrix is left out (rung_copies counts them)."""
    out = []
    if copies is not None:
        for h, c in enumerate(copies):
            for model, k, mk in (("h", "scores_h", "H21"), ("f", "scores_f", "F21")):
                src = c if c[k][0] > 0 else wide[h] if wide is not None and wide[h][k][0] > 0 else None
                if src is not None:
                    out.append((model, h, src[mk].astype(f64), c[k][0], c["masks_" + model][0]))
        return out
    if r["best_h"] >= 0:
        out.append(("h", r["best_h"], r["H21"].astype(f64), r["scores_h"][r["best_h"]], r["masks_h"][r["best_h"]]))
    if r["best_f"] >= 0:
        out.append(("f", r["best_f"], r["F21"].astype(f64), r["scores_f"][r["best_f"]], r["masks_f"][r["best_f"]]))
    return out


# ---- rung 0: a hypothesis does not depend on its neighbours --------------------------------------------------------------
def rung_copies(r, copies, wide=None, expected_matrixless=()):
    """copy h's scores and mask rows have the bytes of row h of the whole scene; a matrix does not depend on sigma (the
    wide copy's has the same bytes); the hypotheses without a matrix in either copy are counted (expected_matrixless: set
    indices that are not counted, the crafted degenerate set)"""
    bad, fig = [], {"matrixless": 0}
    H = len(r["scores_h"])
    if len(copies) != H or (wide is not None and len(wide) != H):
        return ["%d copies for %d hypotheses" % (len(copies), H)], fig
    for h, c in enumerate(copies):
        for k in ("scores_h", "scores_f", "masks_h", "masks_f"):
            if np.ascontiguousarray(c[k][0]).tobytes() != np.ascontiguousarray(r[k][h]).tobytes():
                bad.append("hypothesis %d: %s alone differs from its row in the scene" % (h, k))
        if "n_inliers" in c:      # a whole result: its SH, SF, RH, branch and inlier count follow from its one row (rung 4)
            bad += ["hypothesis %d alone: %s" % (h, v) for v in rung4(c)[0]]
        for k, b, mk in (("scores_h", "best_h", "H21"), ("scores_f", "best_f", "F21")):
            w = wide[h] if wide is not None else None
            if not c[k][0] > 0:
                if h not in expected_matrixless and not (w is not None and w[k][0] > 0):
                    fig["matrixless"] += 1
                if c[b] != -1 or c[mk].any():
                    bad.append("hypothesis %d: %s is not > 0 and yet it won alone" % (h, k))
            elif c[b] != 0:
                bad.append("hypothesis %d: %s > 0 and it did not win alone" % (h, k))
            elif w is not None and w[k][0] > 0 and w[mk].tobytes() != c[mk].tobytes():
                bad.append("hypothesis %d: %s depends on sigma" % (h, mk))
    if fig["matrixless"] > CAP_MATRIXLESS * 2 * H:
        bad.append("%d of %d hypotheses export no matrix" % (fig["matrixless"], 2 * H))
    return bad, fig


# ---- rungs 1, 2: the DLT ---------------------------------------------------------------------------------------------------
def _dlt(prep, idx, model):
    u1, v1, u2, v2 = _normalised(prep, idx)
    z, o = np.zeros_like(u1), np.ones_like(u1)
    if model == "h":
        A = np.concatenate([np.stack([z, z, z, -u1, -v1, -o, v2 * u1, v2 * v1, v2], 1),
                            np.stack([u1, v1, o, z, z, z, -u2 * u1, -u2 * v1, -u2], 1)])
    else:
        A = np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, o], 1)
    return A.T @ A


def rung1(sc, prep, hyps):
    """H: hn = T2 H21 inv(T1) is a minimiser of the 16x9 DLT matrix of the set: its Rayleigh quotient exceeds lambda_min by
    at most TOL_RAY lambda_max, whatever the eigenvalue gap (a repeated index has lambda_min = 0 several times)"""
    bad, fig = [], {}
    sets = np.asarray(sc["sets"], np.int64).reshape(-1, 8)
    T1i, T2 = np.linalg.inv(_tmat(prep["T1"])), _tmat(prep["T2"])
    for model, h, mat, _, _ in hyps:
        if model != "h":
            continue
        S = _dlt(prep, sets[h], "h")
        lam = np.linalg.eigvalsh(S)
        hn = (T2 @ mat @ T1i).reshape(9)
        excess = (hn @ S @ hn / (hn @ hn) - lam[0]) / lam[-1]
        if not np.isfinite(excess):
            bad.append("H %d: the matrix is not finite" % h)
            continue
        _up(fig, "ray", excess)
        if not excess <= TOL_RAY:
            bad.append("H %d: Rayleigh quotient %.3e lambda_max above lambda_min, allowed %.1e" % (h, excess, TOL_RAY))
    return bad, fig


def rung2(sc, prep, hyps):
    """F: Fn = inv(T2)' F21 inv(T1) has rank 2, and its Eckart-Young pre-image (Fn plus a multiple of u3 v3') is a
    minimiser of the 8x9 DLT matrix"""
    bad, fig = [], {}
    sets = np.asarray(sc["sets"], np.int64).reshape(-1, 8)
    T1i, T2it = np.linalg.inv(_tmat(prep["T1"])), np.linalg.inv(_tmat(prep["T2"])).T
    for model, h, mat, _, _ in hyps:
        if model != "f":
            continue
        Fn = T2it @ mat @ T1i
        if not np.isfinite(Fn).all():
            bad.append("F %d: the matrix is not finite" % h)
            continue
        U, s, Vt = np.linalg.svd(Fn)
        _up(fig, "rank", s[2] / s[0])
        if not s[2] / s[0] <= TOL_RANK:
            bad.append("F %d: sigma_3 / sigma_1 = %.3e, allowed %.1e" % (h, s[2] / s[0], TOL_RANK))
        S = _dlt(prep, sets[h], "f")
        lam = np.linalg.eigvalsh(S)
        Q, _ = np.linalg.qr(np.stack([Fn.reshape(9), np.outer(U[:, 2], Vt[2]).reshape(9)], 1))
        excess = (np.linalg.eigvalsh(Q.T @ S @ Q)[0] - lam[0]) / lam[-1]
        _up(fig, "ray", excess)
        if not excess <= TOL_RAY:
            bad.append("F %d: the pre-image's Rayleigh quotient %.3e lambda_max above lambda_min, allowed %.1e" % (h, excess, TOL_RAY))
    return bad, fig


# ---- rung 3: CheckHomography, CheckFundamental -----------------------------------------------------------------------------
def chi_squares(prep, model, mat, sigma):
    """both chi-square terms of every kept pair in float64 (:305-468)"""
    u1, v1, u2, v2 = (prep["pts"][:, k].astype(f64) for k in range(4))
    inv_s2 = 1.0 / (sigma * sigma)
    with np.errstate(all="ignore"):
        if model == "h":
            h, g = mat, np.linalg.inv(mat) if abs(np.linalg.det(mat)) > 0 else np.full((3, 3), np.nan)
            w = g[2, 0] * u2 + g[2, 1] * v2 + g[2, 2]
            a, b = (g[0, 0] * u2 + g[0, 1] * v2 + g[0, 2]) / w, (g[1, 0] * u2 + g[1, 1] * v2 + g[1, 2]) / w
            chi1 = ((u1 - a) ** 2 + (v1 - b) ** 2) * inv_s2
            w = h[2, 0] * u1 + h[2, 1] * v1 + h[2, 2]
            a, b = (h[0, 0] * u1 + h[0, 1] * v1 + h[0, 2]) / w, (h[1, 0] * u1 + h[1, 1] * v1 + h[1, 2]) / w
            chi2 = ((u2 - a) ** 2 + (v2 - b) ** 2) * inv_s2
        else:
            f = mat
            a, b, c = (f[k, 0] * u1 + f[k, 1] * v1 + f[k, 2] for k in range(3))       # the line of pair.first in image 2
            chi1 = (a * u2 + b * v2 + c) ** 2 / (a * a + b * b) * inv_s2
            a, b, c = (f[0, k] * u2 + f[1, k] * v2 + f[2, k] for k in range(3))       # the line of pair.second in image 1
            chi2 = (a * u1 + b * v1 + c) ** 2 / (a * a + b * b) * inv_s2
    return chi1, chi2


def rung3(sc, prep, hyps, n_hyp, cap=True):
    """mask bit = chi1 <= th && chi2 <= th outside the margin; the score (both models subtract from 5.991, each term on its
    own) within TOL_SCORE max(1, score64) plus 5.991 per skipped pair; skipped cells inside the cap (a condition on the
    committed scenes, where every hypothesis is seen; a drawn scene's two winners are not held to it)"""
    bad, fig = [], {"skipped": 0, "cells": 2 * n_hyp * prep["N"]}
    N, sigma = prep["N"], _sigma(sc)
    for model, h, mat, score, row in hyps:
        th = TH_H if model == "h" else TH_F
        tag = "%s %d: " % (model.upper(), h)
        chi1, chi2 = chi_squares(prep, model, mat, sigma)
        with np.errstate(all="ignore"):
            in1, in2 = chi1 <= th, chi2 <= th
            near = (np.abs(chi1 / th - 1.0) < MARGIN_CHI) | (np.abs(chi2 / th - 1.0) < MARGIN_CHI)
            score64 = float(np.where(in1, TH_SCORE - chi1, 0.0).sum() + np.where(in2, TH_SCORE - chi2, 0.0).sum())
        bits, beyond = unpack(row, N)
        if beyond:
            bad.append(tag + "mask bits beyond the %d kept pairs" % N)
        wrong = (bits != (in1 & in2)) & ~near
        if wrong.any():
            e = int(np.flatnonzero(wrong)[0])
            bad.append(tag + "%d mask bits wrong, first pair %d: bit %d, chi-squares %.6g %.6g, threshold %.3f" % (
                wrong.sum(), e, bits[e], chi1[e], chi2[e], th))
        skipped = int(near.sum())
        fig["skipped"] += skipped
        excess = max(0.0, abs(float(score) - score64) - TH_SCORE * skipped)
        dev = excess / max(1.0, score64)
        _up(fig, "score", dev)
        if not dev <= TOL_SCORE or not np.isfinite(float(score)):
            bad.append(tag + "score %.9g, float64 %.9g, %d pairs skipped, allowed %.1e relative" % (score, score64, skipped, TOL_SCORE))
        # the same difference as a distance: chiSquare = d^2 / sigma^2 moves by 2 sqrt(chiSquare) / sigma per pixel that
        # the transferred point (or the epipolar line) moves, so the sum over the inliers' terms turns it into pixels
        with np.errstate(all="ignore"):
            lever = float(np.where(in1, 2.0 * np.sqrt(chi1), 0.0).sum() + np.where(in2, 2.0 * np.sqrt(chi2), 0.0).sum()) / sigma
        px = excess / max(1.0, lever)
        _up(fig, "score_px", px)
        if not px <= TOL_SCORE_PX:
            bad.append(tag + "score %.9g, float64 %.9g: %.3e px per inlier term, allowed %.1e" % (score, score64, px, TOL_SCORE_PX))
    if cap and fig["skipped"] > CAP_SKIPPED * fig["cells"]:
        bad.append("%d of %d (hypothesis, pair) cells within the margin of a threshold" % (fig["skipped"], fig["cells"]))
    return bad, fig


# ---- rung 4: the scans, the branch, the inlier count -----------------------------------------------------------------------
def _scan(scores):
    best, top = -1, np.float32(0)
    for h, s in enumerate(scores):
        if s > top:                       # false for a NaN
            best, top = h, s
    return best, top


def selected_row(r):
    sel = r["best_h"] if r["used_homography"] else r["best_f"]
    return None if sel < 0 else r["masks_h" if r["used_homography"] else "masks_f"][sel]


def rung4(r, copies=None):
    """exact, from the result's own arrays (I6, I7)"""
    bad = []
    bh, SH = _scan(r["scores_h"])
    bf, SF = _scan(r["scores_f"])
    with np.errstate(all="ignore"):
        RH = np.float32(SH) / (np.float32(SH) + np.float32(SF))
    use_h = int(bool(f64(RH) > 0.40))
    for k, want in (("best_h", bh), ("best_f", bf), ("used_homography", use_h)):
        if int(r[k]) != want:
            bad.append("%s %d, from the scores %d" % (k, int(r[k]), want))
    for k, want in (("SH", SH), ("SF", SF), ("RH", RH)):
        if np.float32(r[k]).tobytes() != np.float32(want).tobytes() and not (np.isnan(r[k]) and np.isnan(want)):
            bad.append("%s %.9g, from the scores %.9g" % (k, r[k], want))
    row = selected_row(r)
    count = 0 if row is None else int(np.unpackbits(np.ascontiguousarray(row, np.uint64).view(np.uint8)).sum())
    if int(r["n_inliers"]) != count:
        bad.append("n_inliers %d, the selected row holds %d" % (int(r["n_inliers"]), count))
    for k, b in (("H21", r["best_h"]), ("F21", r["best_f"])):
        if b < 0:
            if r[k].any():
                bad.append("%s is not zero though nothing won" % k)
        elif copies is not None and 0 <= b < len(copies) and r[k].tobytes() != copies[b][k].tobytes():
            bad.append("%s differs from hypothesis %d's alone" % (k, b))
    return bad, {}


# ---- rung 6's machinery: Triangulate and CheckRT in float64 ------------------------------------------------------------------
def check_rt64(sc, prep, R, t, inl):
    """CheckRT (:798-907) for one motion over the pairs of inl [N] in float64.  Arrays over those pairs: e (compacted pair),
    X [.][3], ok (passes every test), low (cosParallax < 0.99998), near (within a margin of one of the tests), cos, gap
    ((sigma_3 - sigma_4) / sigma_1 of the 4x4), e1, e2."""
    K, sigma = _kmat(sc), _sigma(sc)
    e = np.flatnonzero(inl)
    q = prep["pts"][e].astype(f64)
    th2 = 4.0 * sigma * sigma
    P1 = K @ np.eye(3, 4)
    P2 = K @ np.concatenate([R, t[:, None]], 1)
    A = np.stack([q[:, 0, None] * P1[2] - P1[0], q[:, 1, None] * P1[2] - P1[1], q[:, 2, None] * P2[2] - P2[0], q[:, 3, None] * P2[2] - P2[1]], 1)
    out = {"e": e}
    if not len(e):
        z = np.zeros(0)
        out.update(X=np.zeros((0, 3)), ok=z.astype(bool), low=z.astype(bool), near=z.astype(bool), cos=z, gap=z, e1=z, e2=z)
        return out
    _, s, Vt = np.linalg.svd(A)
    with np.errstate(all="ignore"):
        x = Vt[:, 3]
        X = x[:, :3] / x[:, 3, None]
        finite = np.isfinite(X).all(1)
        O2 = -R.T @ t
        n1, n2 = X, X - O2
        cos = (n1 * n2).sum(1) / (np.linalg.norm(n1, axis=1) * np.linalg.norm(n2, axis=1))
        low = cos < COS_GOOD
        X2 = X @ R.T + t
        e1 = (K[0, 0] * X[:, 0] / X[:, 2] + K[0, 2] - q[:, 0]) ** 2 + (K[1, 1] * X[:, 1] / X[:, 2] + K[1, 2] - q[:, 1]) ** 2
        e2 = (K[0, 0] * X2[:, 0] / X2[:, 2] + K[0, 2] - q[:, 2]) ** 2 + (K[1, 1] * X2[:, 1] / X2[:, 2] + K[1, 2] - q[:, 3]) ** 2
        ok = finite & ~((X[:, 2] <= 0) & low) & ~((X2[:, 2] <= 0) & low) & ~(e1 > th2) & ~(e2 > th2)
        near = (np.abs(e1 / th2 - 1.0) < MARGIN_CHI) | (np.abs(e2 / th2 - 1.0) < MARGIN_CHI) | (np.abs(cos / COS_GOOD - 1.0) < MARGIN_COS) | \
            (np.abs(X[:, 2]) < MARGIN_Z) | (np.abs(X2[:, 2]) < MARGIN_Z)
        gap = (s[:, 2] - s[:, 3]) / s[:, 0]
    out.update(X=X, ok=ok, low=low, near=near & finite, cos=cos, gap=gap, e1=e1, e2=e2)
    return out


# ---- rung 5: the motion ----------------------------------------------------------------------------------------------------
def _sign_rule(v):
    """the component of largest magnitude is positive (I4); also whether another component is as large within 1e-6"""
    a = np.abs(v)
    k = int(np.argmax(a))
    return (-v if v[k] < 0 else v), bool((np.delete(a, k) > a[k] * (1.0 - 1e-6)).any())


def motions_f64(sc, F21):
    """DecomposeE in float64, I8's order (R1, t) (R2, t) (R1, -t) (R2, -t) with I4's sign rule on u3 and v3; and whether
    that rule's choice for u3 is within rounding of the other one"""
    K = _kmat(sc)
    U, _, Vt = np.linalg.svd(K.T @ F21 @ K)
    U, Vt = U.copy(), Vt.copy()
    U[:, 2], amb_u = _sign_rule(U[:, 2])
    Vt[2], _ = _sign_rule(Vt[2])
    W = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    R1, R2 = U @ W @ Vt, U @ W.T @ Vt
    R1, R2 = (R1 if np.linalg.det(R1) > 0 else -R1), (R2 if np.linalg.det(R2) > 0 else -R2)
    t = U[:, 2] / np.linalg.norm(U[:, 2])
    return [(R1, t), (R2, t), (R1, -t), (R2, -t)], amb_u


def rung5(sc, prep, r):
    """when success: R21 is a rotation, t21 a unit vector; F: they are one of DecomposeE's motions of K' F21 K, and the four
    float64 motions give n_good[0..3] up to their near-threshold pairs; H: s A / d2 - R21 has rank 1 with t21 spanning its
    column space, A = inv(K) H21 K (a plane-induced homography is proportional to R + t n' / d)"""
    bad, fig = [], {}
    if not r["success"]:
        return bad, fig
    R, t = r["R21"].astype(f64), r["t21"].astype(f64)
    orth = max(np.abs(R.T @ R - np.eye(3)).max(), abs(np.linalg.norm(t) - 1.0))
    _up(fig, "orth", orth)
    if not orth <= TOL_ORTH or not np.linalg.det(R) > 0:
        bad.append("R21 / t21 are no rotation and unit vector: %.3e, allowed %.1e, det %.3f" % (orth, TOL_ORTH, np.linalg.det(R)))
    row = selected_row(r)
    inl = unpack(row, prep["N"])[0]
    if not r["used_homography"]:
        mot, ambiguous = motions_f64(sc, r["F21"].astype(f64))
        dR = min(np.abs(R - mot[0][0]).max(), np.abs(R - mot[1][0]).max())
        dt = min(np.abs(t - mot[0][1]).max(), np.abs(t + mot[0][1]).max())
        _up(fig, "rt", max(dR, dt))
        if not max(dR, dt) <= TOL_RT:
            bad.append("R21 / t21 are %.3e / %.3e from the nearest motion of DecomposeE, allowed %.1e" % (dR, dt, TOL_RT))
        cs = [check_rt64(sc, prep, Ri, ti, inl) for Ri, ti in mot]
        want, slack = [int(c["ok"].sum()) for c in cs], [int(c["near"].sum()) for c in cs]
        # Which of the twin rotations is called R1 is not observable: it is the handedness of (v0, v1), the vectors of
        # an essential matrix's double singular value, that I4's sign rule leaves them with.  The sign of t is u3's rule;
        # where its choice is within rounding of the other one, that labelling is as good.
        orders = [[i ^ x for i in range(4)] for x in ((0, 1, 2, 3) if ambiguous else (0, 1))]
        if not any(all(abs(int(r["n_good"][i]) - want[o[i]]) <= slack[o[i]] for i in range(4)) for o in orders):
            bad.append("n_good[0..3] %s, float64 %s in I8's order (R1, R2 either way), %s pairs near a threshold" % (r["n_good"][:4].tolist(), want, slack))
        if r["n_good"][4:].any():
            bad.append("n_good[4..7] are not zero in the F branch")
    else:
        K = _kmat(sc)
        A = np.linalg.inv(K) @ r["H21"].astype(f64) @ K
        d2 = np.linalg.svd(A, compute_uv=False)[1]
        best = None
        for s in (1.0, -1.0):
            U, sv, _ = np.linalg.svd(s * A / d2 - R)
            s2 = float(np.sum(np.cross(U[:, 0], t) ** 2) / (t @ t))
            cand = (sv[1] / sv[0], s2 / (1.0 + math.sqrt(max(1.0 - s2, 0.0))))     # 1 - |cos| without the cancellation
            best = cand if best is None or cand[0] < best[0] else best
        _up(fig, "rank1", best[0])
        _up(fig, "align", best[1])
        if not best[0] <= TOL_RANK1:
            bad.append("s A / d2 - R21 has sigma_2 / sigma_1 = %.3e, allowed %.1e" % (best[0], TOL_RANK1))
        if not best[1] <= TOL_ALIGN:
            bad.append("t21 is off the column space of s A / d2 - R21: 1 - |cos| = %.3e, allowed %.1e" % (best[1], TOL_ALIGN))
    return bad, fig


# ---- rung 6: CheckRT and the triangulation of the winning motion -----------------------------------------------------------
def rung6(sc, prep, r):
    bad, fig = [], {"rt_skipped": 0}
    P, tri = r["P3D"], r["triangulated"]
    if not r["success"]:
        for k in ("P3D", "triangulated", "R21", "t21") + tuple(k for k in ("R21_out", "t21_out") if k in r):
            if np.asarray(r[k]).any():
                bad.append("%s is not zero after a failure" % k)
        return bad, fig
    for k in ("R21", "t21"):
        if k + "_out" in r and r[k + "_out"].tobytes() != r[k].tobytes():
            bad.append("the %s array differs from the result's" % k)
    R, t, b = r["R21"].astype(f64), r["t21"].astype(f64), int(r["best_motion"])
    inl = unpack(selected_row(r), prep["N"])[0]
    c = check_rt64(sc, prep, R, t, inl)
    rows = prep["first"][c["e"]]
    other = np.ones(len(P), bool)
    other[rows] = False
    if P[other].any() or tri[other].any():
        bad.append("P3D / triangulated are written outside the selected mask")
    Pd = P[rows].astype(f64)
    written = (P[rows] != 0).any(1)
    firm = ~c["near"]
    fig["rt_skipped"] = int(c["near"].sum())
    wrong = (written != c["ok"]) & firm
    if wrong.any():
        i = int(np.flatnonzero(wrong)[0])
        bad.append("%d pairs written / not written against float64 CheckRT, first pair %d: written %d, errors %.4g %.4g, cos %.8f, z %.4g" % (
            wrong.sum(), c["e"][i], written[i], c["e1"][i], c["e2"][i], c["cos"][i], c["X"][i, 2]))
    wrong = ((tri[rows] != 0) != (c["ok"] & c["low"])) & firm
    if wrong.any():
        i = int(np.flatnonzero(wrong)[0])
        bad.append("%d triangulated flags wrong, first pair %d: flag %d, passes %d, cos %.8f" % (wrong.sum(), c["e"][i], tri[rows][i], c["ok"][i], c["cos"][i]))
    if (tri[rows] > 1).any():
        bad.append("triangulated holds values other than 0 / 1")
    if int(r["n_good"][b]) != int(written.sum()):
        bad.append("n_good[%d] %d, P3D holds %d points" % (b, int(r["n_good"][b]), int(written.sum())))
    both = written & c["ok"]
    if both.any():
        with np.errstate(all="ignore"):
            dev = np.linalg.norm(Pd[both] - c["X"][both], axis=1) * c["gap"][both] / np.linalg.norm(c["X"][both], axis=1)
        _up(fig, "pt", dev.max())
        if not dev.max() <= TOL_PT:
            i = int(np.argmax(dev))
            bad.append("a point is %.3e |X| / gap from float64's, allowed %.1e (pair %d)" % (dev.max(), TOL_PT, c["e"][both][i]))
    if written.any():
        K, sigma = _kmat(sc), _sigma(sc)
        q, X1 = prep["pts"][c["e"]].astype(f64)[written], Pd[written]
        X2 = X1 @ R.T + t
        with np.errstate(all="ignore"):
            e1 = (K[0, 0] * X1[:, 0] / X1[:, 2] + K[0, 2] - q[:, 0]) ** 2 + (K[1, 1] * X1[:, 1] / X1[:, 2] + K[1, 2] - q[:, 1]) ** 2
            e2 = (K[0, 0] * X2[:, 0] / X2[:, 2] + K[0, 2] - q[:, 2]) ** 2 + (K[1, 1] * X2[:, 1] / X2[:, 2] + K[1, 2] - q[:, 3]) ** 2
            worst = np.maximum(e1, e2)
            O2 = -R.T @ t
            cosd = np.sort((X1 * (X1 - O2)).sum(1) / (np.linalg.norm(X1, axis=1) * np.linalg.norm(X1 - O2, axis=1)))
        if not (worst <= 4.0 * sigma * sigma * (1.0 + MARGIN_CHI)).all():
            bad.append("a written point reprojects %.6g px^2 off, th2 = %.3f" % (np.nanmax(worst), 4.0 * sigma * sigma))
        cos64 = np.sort(c["cos"][written])
        sel = cos64[min(50, len(cos64) - 1)]
        dev = abs(float(r["cos_parallax"][b]) - sel)
        _up(fig, "cos", dev)
        if not dev <= TOL_COS:
            bad.append("cos_parallax[%d] %.9f, the float64 cosine of rank %d is %.9f, allowed %.1e" % (
                b, r["cos_parallax"][b], min(50, len(cos64) - 1), sel, TOL_COS))
    return bad, fig


# ---- rung 7: the accept rule -------------------------------------------------------------------------------------------------
def rung7(sc, r, limits):
    """best_motion, second_best_good and success exactly as ReconstructF's (:499-569) and ReconstructH's (:688-731) if
    chains are written, from the result's own n_good, cos_parallax and n_inliers; limits = (limit_f, limit_h) of
    orbgpu_initializer_cos_limits(min_parallax): parallax > (>=) min_parallax is cosine <= limit (I10)"""
    bad = []
    ng, cosines, N = [int(v) for v in r["n_good"]], r["cos_parallax"], int(r["n_inliers"])
    min_tri = int(sc.get("min_triangulated", 50))
    lim_f, lim_h = limits
    if selected_row(r) is None:
        best, second, success = -1, 0, False
    elif r["used_homography"]:
        best, best_good, second = -1, 0, 0
        for i in range(8):
            if ng[i] > best_good:
                second, best_good, best = best_good, ng[i], i
            elif ng[i] > second:
                second = ng[i]
        success = best >= 0 and second < 0.75 * best_good and bool(cosines[best] <= lim_h) and best_good > min_tri and best_good > 0.9 * N
    else:
        max_good = max(ng[:4])
        n_min_good = max(int(0.9 * N), min_tri)
        second = sum(1 for i in range(4) if ng[i] > 0.7 * max_good)
        best = ng[:4].index(max_good)
        success = not (max_good < n_min_good or second > 1) and bool(cosines[best] <= lim_f)
    for k, want in (("best_motion", best), ("second_best_good", second), ("success", int(success))):
        if int(r[k]) != want:
            bad.append("%s %d, the if chain gives %d from n_good %s" % (k, int(r[k]), want, ng))
    return bad, {}


# ---- the ladder ------------------------------------------------------------------------------------------------------------
RUNGS = ("copies", "rung1", "rung2", "rung3", "rung4", "rung5", "rung6", "rung7")


def ladder(sc, r, copies, limits, name=None, only=RUNGS, wide=None):
    """every rung in `only` on one result: {rung: (violations, figures)}.  copies, wide: the [H] single-hypothesis results
    of with_copies, or None (then rungs 1-3 see the two winners only and there is no rung 0)."""
    prep = prepare(sc)
    hyps = hypotheses(r, copies, wide)
    H = len(np.asarray(sc["sets"]).reshape(-1, 8))
    out = {}
    if "copies" in only and copies is not None:
        out["copies"] = rung_copies(r, copies, wide, (2,) if name == DEGENERATE else ())
    if prep["N"] < 8:
        hyps = []
    for k, fn in (("rung1", lambda: rung1(sc, prep, hyps)), ("rung2", lambda: rung2(sc, prep, hyps)),
                  ("rung3", lambda: rung3(sc, prep, hyps, H, cap=copies is not None)), ("rung4", lambda: rung4(r, copies)),
                  ("rung5", lambda: rung5(sc, prep, r)), ("rung6", lambda: rung6(sc, prep, r)), ("rung7", lambda: rung7(sc, r, limits))):
        if k in only:
            out[k] = fn()
    return out


def figures(rungs):
    """one flat dict of a ladder's figures"""
    fig = {}
    for _, f in rungs.values():
        for k, v in f.items():
            fig[k] = max(fig[k], v) if k in fig and k in TOLERANCES else v
    for k in TOLERANCES:
        fig.setdefault(k, 0.0)
    if "cells" in fig:
        fig["skipped_share"] = fig["skipped"] / max(fig["cells"], 1)
    return fig


def violations(rungs):
    return ["%s: %s" % (k, v) for k in RUNGS if k in rungs for v in rungs[k][0]]


def record(path, column, by_scene):
    """profiles/init_fp64.json: per scene the figures of `column` ("restatement" or "device") beside the other's"""
    import json
    import os
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc["note"] = "each stage against float64 on the stage before's own output (tests/init_fp64.py); tolerances are 16 x the " \
                  "restatement's largest figure, one digit, rounded up"
    doc["tolerances"] = {k: globals()[v] for k, v in TOLERANCES.items()}
    doc["margins"] = {"chi": MARGIN_CHI, "cos": MARGIN_COS, "z": MARGIN_Z, "cap_skipped": CAP_SKIPPED, "cap_matrixless": CAP_MATRIXLESS}
    scenes_doc = doc.setdefault("by_scene", {})
    for name, fig in by_scene.items():
        scenes_doc.setdefault(name, {})[column] = {k: (float(v) if isinstance(v, float) else int(v)) for k, v in sorted(fig.items())}
    doc["largest"] = {col: {k: max([s[col].get(k, 0.0) for s in scenes_doc.values() if col in s] + [0.0]) for k in TOLERANCES}
                      for col in ("restatement", "device")}
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
