"""Initializer (Initializer.cc: H / F RANSAC and the two-view reconstruction of the monocular bootstrap) restated in
numpy: the definition the device entry points (orbgpu_initializer*, include/orbgpu.h I1-I10) are compared with -- vs CPU
restatement; OpenCV boundary unpinned.

Float where the reference computes in float, float64 where OpenCV's SVD stood, one rounding per operation in the order
written here.  eig="eigh" swaps the Jacobi for numpy.linalg.eigh / the same downstream steps: the second eigen-path, whose
distance from the first is the "spread" (pnp_model.py's rule)."""
import ctypes
import ctypes.util
import math

import numpy as np

from pnp_model import BOUND_FACTOR, GAP, LEFT_OUT_CAP, dev, sorted_eig  # noqa: F401  (the rules are shared; the Jacobi: jacobi_model.py)
from sim3_model import reference_random_int  # noqa: F401

f32, f64 = np.float32, np.float64
MAX_N, MAX_HYP = 16384, 4096
JACOBI_SWEEPS = 30
TH_H, TH_F = f32(5.991), f32(3.841)
K_DEFAULT = (500.0, 500.0, 320.0, 240.0)

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.acosf.restype = ctypes.c_float
_libm.acosf.argtypes = [ctypes.c_float]


# ---- I10 ---------------------------------------------------------------------------------------------------------------
def parallax_of(c):
    """(float)(acosf(c) * 180 / CV_PI): the float product, the double division, rounded to float"""
    a = f32(_libm.acosf(float(f32(c))))
    with np.errstate(all="ignore"):
        return f32(f64(a * f32(180.0)) / f64(3.1415926535897932384626433832795))


def cos_key(c):
    u = int(np.asarray(c, f32).view(np.uint32))
    return (~u) & 0xffffffff if u & 0x80000000 else u | 0x80000000


def key_cos(k):
    u = (k & 0x7fffffff) if k & 0x80000000 else (~k) & 0xffffffff
    return np.array(u, np.uint32).view(f32)[()]


def cos_limit(min_parallax, strict):
    """the largest float c in [-1, 1] for which parallax_of(c) > (strict) or >= min_parallax; NaN if none"""
    mp = f32(min_parallax)

    def holds(c):
        p = parallax_of(c)
        return bool(p > mp) if strict else bool(p >= mp)
    if not holds(f32(-1.0)):
        return f32(np.nan)
    if holds(f32(1.0)):
        return f32(1.0)
    lo, hi = cos_key(f32(-1.0)), cos_key(f32(1.0))
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        if holds(key_cos(mid)):
            lo = mid
        else:
            hi = mid
    return key_cos(lo)


# ---- I2 ----------------------------------------------------------------------------------------------------------------
def sample_sets(n, iterations, random_int):
    """The draw of Initializer::Initialize (:82-97) replayed: WITHOUT replacement, the back element moves into position
    randi.  random_int(lo, hi) is called 8 times per iteration.  n < 8 and a random_int outside [lo, hi] are refused."""
    if n < 8:
        raise ValueError("fewer matches than the minimal set")
    out = np.zeros((iterations, 8), np.int32)
    for it in range(iterations):
        avail = list(range(n))
        for j in range(8):
            randi = random_int(0, len(avail) - 1)
            if not 0 <= randi < len(avail):
                raise ValueError("RandomInt outside [min, max]")
            out[it, j] = avail[randi]
            avail[randi] = avail[-1]
            avail.pop()
    return out


# ---- small dense steps -------------------------------------------------------------------------------------------------
def mul3(A, B):
    """[..., 3, 3] x [..., 3, 3] in the arrays' type, (a b + c d) + e f per entry"""
    return (A[..., :, 0, None] * B[..., None, 0, :] + A[..., :, 1, None] * B[..., None, 1, :]) + A[..., :, 2, None] * B[..., None, 2, :]


def triple3(A, Bf, C):
    """float((A B) C) over float64 A, C and float B"""
    with np.errstate(all="ignore"):
        return mul3(mul3(A, Bf.astype(f64)), C).astype(f32)


def det3d(m):
    m = m.astype(f64)
    a, b, c, d, e, f, g, h, i = (m[..., r, s] for r in range(3) for s in range(3))
    return (a * (e * i - f * h) - b * (d * i - f * g)) + c * (d * h - e * g)


def tmat(T):
    sx, sy, tx, ty = (f64(v) for v in T)
    return np.array([[sx, 0, tx], [0, sy, ty], [0, 0, 1]], f64)


def sign_rule(v):
    k = np.argmax(np.abs(v), axis=-1)
    lead = np.take_along_axis(v, k[..., None], -1)
    return np.where(lead < 0.0, -v, v)


def svd3(Af, eig, proper):
    """I4's 3x3 SVD over a batch [B][3][3] of float entries.  Returns (U [B][3][3] with u_k in column k, d [B][3],
    Vt [B][3][3] with v_k in row k, w: the eigenvalues of A'A, descending)."""
    A = Af.astype(f64)
    with np.errstate(all="ignore"):
        S = np.zeros(A.shape)
        for j in range(3):
            S = S + A[:, j, :, None] * A[:, j, None, :]
        w, Vt = sorted_eig(S, eig, JACOBI_SWEEPS)
        av = np.stack([(A[:, :, 0] * Vt[:, k, 0, None] + A[:, :, 1] * Vt[:, k, 1, None]) + A[:, :, 2] * Vt[:, k, 2, None]
                       for k in range(3)], 1)                     # [B][k][i]
        d = np.sqrt((av[:, :, 0] * av[:, :, 0] + av[:, :, 1] * av[:, :, 1]) + av[:, :, 2] * av[:, :, 2])
        u0, u1 = av[:, 0] / d[:, 0, None], av[:, 1] / d[:, 1, None]
        c = np.stack([u0[:, 1] * u1[:, 2] - u0[:, 2] * u1[:, 1], u0[:, 2] * u1[:, 0] - u0[:, 0] * u1[:, 2],
                      u0[:, 0] * u1[:, 1] - u0[:, 1] * u1[:, 0]], 1)
        c = c / np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])[:, None]
        if proper:
            flip = (c[:, 0] * av[:, 2, 0] + c[:, 1] * av[:, 2, 1]) + c[:, 2] * av[:, 2, 2] < 0.0
            u2 = np.where(flip[:, None], -c, c)
        else:
            u2 = sign_rule(c)
        U = np.stack([u0, u1, u2], 2)
    return U, d, Vt, w


# ---- I1, I3 ------------------------------------------------------------------------------------------------------------
def normalize(kp):
    """Normalize (:749-795) over all key points: (T = (sX, sY, -meanX*sX, -meanY*sY), meanX, meanY), float"""
    kp = np.asarray(kp, f32).reshape(-1, 2)
    n = len(kp)
    with np.errstate(all="ignore"):
        s = np.add.accumulate(kp, axis=0, dtype=f32)[-1] if n else np.zeros(2, f32)
        mean = s / f32(n)
        dv = np.abs(kp - mean)
        d = np.add.accumulate(dv, axis=0, dtype=f32)[-1] if n else np.zeros(2, f32)
        d = d / f32(n)
        sc = (1.0 / d.astype(f64)).astype(f32)
        T = np.array([sc[0], sc[1], -mean[0] * sc[0], -mean[1] * sc[1]], f32)
    return T, mean, sc


def prepare(pr):
    k1, k2 = np.asarray(pr["kp1"], f32).reshape(-1, 2), np.asarray(pr["kp2"], f32).reshape(-1, 2)
    m = np.asarray(pr["matches12"], np.int64)
    n1, n2 = len(k1), len(k2)
    kept = (m >= 0) & (m < n2)
    first = np.flatnonzero(kept)
    second = m[first]
    T1, mean1, s1 = normalize(k1)
    T2, mean2, s2 = normalize(k2)
    pts = np.concatenate([k1[first], k2[second]], 1).astype(f32) if len(first) else np.zeros((0, 4), f32)
    with np.errstate(all="ignore"):
        pn = np.concatenate([(k1[first] - mean1) * s1, (k2[second] - mean2) * s2], 1).astype(f32) if len(first) else np.zeros((0, 4), f32)
    return {"n1": n1, "n2": n2, "N": len(first), "first": first.astype(np.int32), "second": second.astype(np.int32),
            "n_bad_index": int((m >= n2).sum()), "pts": pts, "pn": pn, "T1": T1, "T2": T2}


# ---- I4, I5 ------------------------------------------------------------------------------------------------------------
def dlt_rows(pn, model):
    """pn [B][8][4] normalised (u1 v1 u2 v2) -> A [B][rows][9] float"""
    u1, v1, u2, v2 = (pn[:, :, k] for k in range(4))
    z, o = np.zeros_like(u1), np.ones_like(u1)
    with np.errstate(all="ignore"):
        if model == "H":
            r0 = np.stack([z, z, z, -u1, -v1, -o, v2 * u1, v2 * v1, v2], 2)
            r1 = np.stack([u1, v1, o, z, z, z, -u2 * u1, -u2 * v1, -u2], 2)
            return np.stack([r0, r1], 2).reshape(len(pn), 16, 9)
        return np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, o], 2)


def null_vector(A, eig):
    """float null vector [B][9] of float A [B][rows][9], and the relative gap between the two smallest eigenvalues"""
    A = A.astype(f64)
    with np.errstate(all="ignore"):
        S = np.zeros((len(A), 9, 9))
        for r in range(A.shape[1]):
            S = S + A[:, r, :, None] * A[:, r, None, :]
        w, Vt = sorted_eig(S, eig, JACOBI_SWEEPS)
        gap = (w[:, 7] - w[:, 8]) / np.abs(w[:, 0])
        return Vt[:, 8].astype(f32), np.where(np.isfinite(gap), gap, 0.0)


def inv3(M):
    """adj / det in float64 over float entries, rounded to float"""
    m = M.astype(f64)
    a, b, c, d, e, f, g, h, i = (m[:, r, s] for r in range(3) for s in range(3))
    with np.errstate(all="ignore"):
        det = (a * (e * i - f * h) - b * (d * i - f * g)) + c * (d * h - e * g)
        adj = [e * i - f * h, c * h - b * i, b * f - c * e, f * g - d * i, a * i - c * g, c * d - a * f,
               d * h - e * g, b * g - a * h, a * e - b * d]
        return np.stack([x / det for x in adj], 1).reshape(-1, 3, 3).astype(f32)


def hypotheses_h(prep, sets, eig):
    pn = prep["pn"][sets]
    hn, gap = null_vector(dlt_rows(pn, "H"), eig)
    T1, T2 = tmat(prep["T1"]), tmat(prep["T2"])
    with np.errstate(all="ignore"):
        T2i = np.array([[1.0 / T2[0, 0], 0, -T2[0, 2] / T2[0, 0]], [0, 1.0 / T2[1, 1], -T2[1, 2] / T2[1, 1]], [0, 0, 1]], f64)
    H21 = triple3(T2i[None], hn.reshape(-1, 3, 3), T1[None])
    return H21, inv3(H21), gap


def hypotheses_f(prep, sets, eig):
    pn = prep["pn"][sets]
    fpre, gap = null_vector(dlt_rows(pn, "F"), eig)
    U, d, Vt, w = svd3(fpre.reshape(-1, 3, 3), eig, False)
    with np.errstate(all="ignore"):
        Fn = ((d[:, 0, None] * U[:, :, 0])[:, :, None] * Vt[:, None, 0, :] + (d[:, 1, None] * U[:, :, 1])[:, :, None] * Vt[:, None, 1, :]).astype(f32)
        g3 = np.minimum(w[:, 0] - w[:, 1], w[:, 1] - w[:, 2]) / np.abs(w[:, 0])
    T1, T2 = tmat(prep["T1"]), tmat(prep["T2"])
    F21 = triple3(T2.T[None].copy(), Fn, T1[None])
    return F21, np.minimum(gap, np.where(np.isfinite(g3), g3, 0.0))


def _running_sum(t1, t2):
    """[B][N] float terms -> the running float sum in index order, term 1 before term 2"""
    B, N = t1.shape
    if N == 0:
        return np.zeros(B, f32)
    terms = np.stack([t1, t2], 2).reshape(B, 2 * N).astype(f32)
    return np.add.accumulate(terms, axis=1, dtype=f32)[:, -1]


def _finv(x):
    return (1.0 / x.astype(f64)).astype(f32)


def check_homography(prep, H21, H12, sigma):
    """CheckHomography for B hypotheses: (score [B] float, inlier [B][N], least |chi / th - 1| [B])"""
    u1, v1, u2, v2 = (prep["pts"][None, :, k] for k in range(4))
    h, hi = H21.reshape(-1, 9, 1), H12.reshape(-1, 9, 1)
    with np.errstate(all="ignore"):
        inv_s2 = _finv(np.asarray(f32(sigma) * f32(sigma)))
        w2 = _finv((hi[:, 6] * u2 + hi[:, 7] * v2) + hi[:, 8])
        a = ((hi[:, 0] * u2 + hi[:, 1] * v2) + hi[:, 2]) * w2
        b = ((hi[:, 3] * u2 + hi[:, 4] * v2) + hi[:, 5]) * w2
        chi1 = ((u1 - a) * (u1 - a) + (v1 - b) * (v1 - b)) * inv_s2
        w1 = _finv((h[:, 6] * u1 + h[:, 7] * v1) + h[:, 8])
        a = ((h[:, 0] * u1 + h[:, 1] * v1) + h[:, 2]) * w1
        b = ((h[:, 3] * u1 + h[:, 4] * v1) + h[:, 5]) * w1
        chi2 = ((u2 - a) * (u2 - a) + (v2 - b) * (v2 - b)) * inv_s2
        in1, in2 = chi1 <= TH_H, chi2 <= TH_H
        score = _running_sum(np.where(in1, TH_H - chi1, f32(0)), np.where(in2, TH_H - chi2, f32(0)))
        near = np.minimum(np.abs(chi1.astype(f64) / f64(TH_H) - 1.0), np.abs(chi2.astype(f64) / f64(TH_H) - 1.0))
        near = np.where(np.isfinite(near), near, np.inf)
    return score, in1 & in2, near.min(1) if near.shape[1] else np.full(len(near), np.inf)


def check_fundamental(prep, F21, sigma):
    u1, v1, u2, v2 = (prep["pts"][None, :, k] for k in range(4))
    f = F21.reshape(-1, 9, 1)
    with np.errstate(all="ignore"):
        inv_s2 = _finv(np.asarray(f32(sigma) * f32(sigma)))
        a2 = (f[:, 0] * u1 + f[:, 1] * v1) + f[:, 2]
        b2 = (f[:, 3] * u1 + f[:, 4] * v1) + f[:, 5]
        c2 = (f[:, 6] * u1 + f[:, 7] * v1) + f[:, 8]
        num2 = (a2 * u2 + b2 * v2) + c2
        chi1 = ((num2 * num2) / (a2 * a2 + b2 * b2)) * inv_s2
        a1 = (f[:, 0] * u2 + f[:, 3] * v2) + f[:, 6]
        b1 = (f[:, 1] * u2 + f[:, 4] * v2) + f[:, 7]
        c1 = (f[:, 2] * u2 + f[:, 5] * v2) + f[:, 8]
        num1 = (a1 * u1 + b1 * v1) + c1
        chi2 = ((num1 * num1) / (a1 * a1 + b1 * b1)) * inv_s2
        in1, in2 = chi1 <= TH_F, chi2 <= TH_F
        score = _running_sum(np.where(in1, TH_H - chi1, f32(0)), np.where(in2, TH_H - chi2, f32(0)))
        near = np.minimum(np.abs(chi1.astype(f64) / f64(TH_F) - 1.0), np.abs(chi2.astype(f64) / f64(TH_F) - 1.0))
        near = np.where(np.isfinite(near), near, np.inf)
    return score, in1 & in2, near.min(1) if near.shape[1] else np.full(len(near), np.inf)


def mask_words(inl, n1):
    """bit e of the row = compacted pair e; (n1 + 63) / 64 words"""
    words = (n1 + 63) // 64
    bits = np.zeros(words * 64, np.uint8)
    bits[:len(inl)] = inl
    return np.packbits(bits.reshape(-1, 8), axis=1, bitorder="little").reshape(-1).view(np.uint64).copy() if words else np.zeros(0, np.uint64)


# ---- I8 ----------------------------------------------------------------------------------------------------------------
def _fsqrt(x):
    return np.sqrt(f64(x)).astype(f32)


def _fnorm3(t):
    t = t.astype(f64)
    return f32(np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]))


def motions_h(H21, K, eig):
    """ReconstructH's eight motions: (R [8][3][3], t [8][3]) float, or None when a ratio test fails; also the SVD's
    relative eigenvalue gap"""
    fx, fy, cx, cy = (f64(f32(k)) for k in K)
    Kd = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], f64)
    with np.errstate(all="ignore"):
        Ki = np.array([[1.0 / fx, 0, -cx / fx], [0, 1.0 / fy, -cy / fy], [0, 0, 1]], f64)
        A = triple3(Ki[None], H21[None], Kd[None])
        Ud, dd, Vd, w = svd3(A, eig, True)
        gap = float(np.minimum(w[0, 0] - w[0, 1], w[0, 1] - w[0, 2]) / np.abs(w[0, 0]))
        U, Vt = Ud[0].astype(f32), Vd[0].astype(f32)
        s = f32(det3d(U) * det3d(Vt))
        d1, d2, d3 = (f32(x) for x in dd[0])
        if f64(d1 / d2) < 1.00001 or f64(d2 / d3) < 1.00001:
            return None, gap
        q1, q2, q3 = d1 * d1, d2 * d2, d3 * d3
        aux1, aux3 = _fsqrt((q1 - q2) / (q1 - q3)), _fsqrt((q2 - q3) / (q1 - q3))
        x1, x3 = [aux1, aux1, -aux1, -aux1], [aux3, -aux3, aux3, -aux3]
        root = _fsqrt((q1 - q2) * (q2 - q3))
        aux_st, ctheta = root / ((d1 + d3) * d2), (q2 + d1 * d3) / ((d1 + d3) * d2)
        aux_sp, cphi = root / ((d1 - d3) * d2), (d1 * d3 - q2) / ((d1 - d3) * d2)
        sgn = [1, -1, -1, 1]
        sU = s * U
        R, t = np.zeros((8, 3, 3), f32), np.zeros((8, 3), f32)
        for m in range(8):
            i, second = m & 3, m >= 4
            base = aux_sp if second else aux_st
            sn = base if sgn[i] > 0 else -base
            Rp = np.zeros((3, 3), f32)
            if not second:
                Rp[0, 0], Rp[0, 2], Rp[1, 1], Rp[2, 0], Rp[2, 2] = ctheta, -sn, 1, sn, ctheta
            else:
                Rp[0, 0], Rp[0, 2], Rp[1, 1], Rp[2, 0], Rp[2, 2] = cphi, sn, -1, sn, -cphi
            R[m] = mul3(mul3(sU, Rp), Vt)
            scale = d1 + d3 if second else d1 - d3
            tp = np.array([x1[i] * scale, f32(0) * scale, (x3[i] if second else -x3[i]) * scale], f32)
            tv = (U[:, 0] * tp[0] + U[:, 1] * tp[1]) + U[:, 2] * tp[2]
            t[m] = tv / _fnorm3(tv)
    return (R, t), gap


def motions_f(F21, K, eig):
    """DecomposeE's four motions in ReconstructF's order"""
    fx, fy, cx, cy = (f64(f32(k)) for k in K)
    Kd = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], f64)
    with np.errstate(all="ignore"):
        E = triple3(Kd.T[None].copy(), F21[None], Kd[None])
        Ud, _, Vd, w = svd3(E, eig, False)
        U, Vt = Ud[0].astype(f32), Vd[0].astype(f32)
        tv = U[:, 2].copy()
        tn = tv / _fnorm3(tv)
        W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], f32)
        R1, R2 = mul3(mul3(U, W), Vt), mul3(mul3(U, W.T.copy()), Vt)
        if det3d(R1) < 0.0:
            R1 = -R1
        if det3d(R2) < 0.0:
            R2 = -R2
    return np.stack([R1, R2, R1, R2]).astype(f32), np.stack([tn, tn, -tn, -tn]).astype(f32)


# ---- I9 ----------------------------------------------------------------------------------------------------------------
def check_rt(prep, R, t, inl, K, sigma, eig):
    """CheckRT for one motion over the inlier pairs.  Returns a dict: n_good, cos (the selected cosine), P3D [n1][3],
    good [n1], cosines (of the good pairs, in pair order), gap (least relative gap below the third eigenvalue)."""
    n1 = prep["n1"]
    fx, fy, cx, cy = (f32(k) for k in K)
    out = {"n_good": 0, "cos": f32(1.0), "P3D": np.zeros((n1, 3), f32), "good": np.zeros(n1, np.uint8), "cosines": np.zeros(0, f32),
           "gap": np.inf}
    idx = np.flatnonzero(inl)
    if len(idx) == 0:
        return out
    q = prep["pts"][idx]
    with np.errstate(all="ignore"):
        Kf = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], f32)
        P1 = np.array([[fx, 0, cx, 0], [0, fy, cy, 0], [0, 0, 1, 0]], f32)
        M = np.concatenate([R, t[:, None]], 1).astype(f32)
        P2 = ((Kf[:, 0, None] * M[None, 0] + Kf[:, 1, None] * M[None, 1]) + Kf[:, 2, None] * M[None, 2]).astype(f32)
        O2 = (((-R[0]) * t[0] + (-R[1]) * t[1]) + (-R[2]) * t[2]).astype(f32)
        th2 = f32(4.0 * f64(f32(sigma) * f32(sigma)))
        A = np.stack([q[:, 0, None] * P1[None, 2] - P1[None, 0], q[:, 1, None] * P1[None, 2] - P1[None, 1],
                      q[:, 2, None] * P2[None, 2] - P2[None, 0], q[:, 3, None] * P2[None, 2] - P2[None, 1]], 1).astype(f64)
        S = np.zeros((len(idx), 4, 4))
        for r in range(4):
            S = S + A[:, r, :, None] * A[:, r, None, :]
        w, Vt = sorted_eig(S, eig, JACOBI_SWEEPS)
        gap = (w[:, 2] - w[:, 3]) / np.abs(w[:, 0])
        out["gap"] = float(np.where(np.isfinite(gap), gap, 0.0).min())
        x4 = Vt[:, 3].astype(f32)
        p = x4[:, :3] / x4[:, 3, None]
        finite = np.isfinite(p).all(1)
        pd = p.astype(f64)
        dist1 = np.sqrt((pd[:, 0] * pd[:, 0] + pd[:, 1] * pd[:, 1]) + pd[:, 2] * pd[:, 2]).astype(f32)
        nrm = (p - O2[None]).astype(f32)
        nd = nrm.astype(f64)
        dist2 = np.sqrt((nd[:, 0] * nd[:, 0] + nd[:, 1] * nd[:, 1]) + nd[:, 2] * nd[:, 2]).astype(f32)
        dot = (pd[:, 0] * nd[:, 0] + pd[:, 1] * nd[:, 1]) + pd[:, 2] * nd[:, 2]
        cosp = (dot / (dist1 * dist2).astype(f64)).astype(f32)
        low = cosp.astype(f64) < 0.99998
        p2 = np.stack([((R[i, 0] * p[:, 0] + R[i, 1] * p[:, 1]) + R[i, 2] * p[:, 2]) + t[i] for i in range(3)], 1).astype(f32)
        ok = finite & ~((p[:, 2] <= 0) & low) & ~((p2[:, 2] <= 0) & low)
        iz1 = _finv(p[:, 2])
        im1x, im1y = (fx * p[:, 0]) * iz1 + cx, (fy * p[:, 1]) * iz1 + cy
        e1 = (im1x - q[:, 0]) * (im1x - q[:, 0]) + (im1y - q[:, 1]) * (im1y - q[:, 1])
        iz2 = _finv(p2[:, 2])
        im2x, im2y = (fx * p2[:, 0]) * iz2 + cx, (fy * p2[:, 1]) * iz2 + cy
        e2 = (im2x - q[:, 2]) * (im2x - q[:, 2]) + (im2y - q[:, 3]) * (im2y - q[:, 3])
        ok = ok & ~(e1 > th2) & ~(e2 > th2)
        near = np.minimum(np.abs(e1.astype(f64) / f64(th2) - 1.0), np.abs(e2.astype(f64) / f64(th2) - 1.0))
        near = np.minimum(near, np.abs(cosp.astype(f64) / 0.99998 - 1.0))
        out["near"] = float(np.where(np.isfinite(near) & finite, near, np.inf).min())
    first = prep["first"][idx[ok]]
    out["P3D"][first] = p[ok]
    out["good"][first] = low[ok]
    out["cosines"] = cosp[ok]
    out["n_good"] = int(ok.sum())
    if out["n_good"] > 0:
        keys = sorted(cos_key(c) for c in out["cosines"])
        out["cos"] = key_cos(keys[min(50, out["n_good"] - 1)])
    return out


# ---- the whole of Initialize ---------------------------------------------------------------------------------------------
def initialize(pr, eig="jacobi"):
    """The whole Initializer over pr["sets"] [H][8].  pr: kp1, kp2, matches12, sets, K and optionally sigma (1.0),
    min_parallax (1.0), min_triangulated (50)."""
    prep = prepare(pr)
    N, n1 = prep["N"], prep["n1"]
    K = pr.get("K", K_DEFAULT)
    sigma, min_par, min_tri = pr.get("sigma", 1.0), pr.get("min_parallax", 1.0), int(pr.get("min_triangulated", 50))
    sets = np.asarray(pr["sets"], np.int64).reshape(-1, 8)
    H = len(sets)
    words = (n1 + 63) // 64
    z33 = np.zeros((3, 3), f32)
    out = {"N": N, "n_bad_index": prep["n_bad_index"], "n_bad_set": 0, "prep": prep,
           "scores_h": np.zeros(H, f32), "scores_f": np.zeros(H, f32), "masks_h": np.zeros((H, words), np.uint64),
           "masks_f": np.zeros((H, words), np.uint64), "mats_h": np.zeros((H, 3, 3), f32), "mats_f": np.zeros((H, 3, 3), f32),
           "gap_h": np.full(H, np.inf), "gap_f": np.full(H, np.inf), "near_h": np.full(H, np.inf), "near_f": np.full(H, np.inf),
           "repeated": np.zeros(H, bool), "best_h": -1, "best_f": -1, "SH": f32(0), "SF": f32(0), "used_homography": 0,
           "n_inliers": 0, "n_good": np.zeros(8, np.int32), "cos_parallax": np.zeros(8, f32), "best_motion": -1,
           "second_best_good": 0, "success": 0, "parallax_deg": f32(0), "H21": z33.copy(), "F21": z33.copy(), "R21": z33.copy(),
           "t21": np.zeros(3, f32), "P3D": np.zeros((n1, 3), f32), "triangulated": np.zeros(n1, np.uint8), "n_motions": 0,
           "svd_gap": np.inf, "rt_gap": np.inf, "rt_near": np.inf, "motions": None}
    with np.errstate(all="ignore"):
        out["RH"] = f32(0) / f32(0)
    if N < 8:
        return out
    good = np.array([s.min() >= 0 and s.max() < N for s in sets], bool) if H else np.zeros(0, bool)
    out["n_bad_set"] = int((~good).sum())
    inl_h, inl_f = np.zeros((H, N), bool), np.zeros((H, N), bool)
    if good.any():
        g = np.flatnonzero(good)
        sel = sets[g]
        H21, H12, gh = hypotheses_h(prep, sel, eig)
        sh, ih, nh = check_homography(prep, H21, H12, sigma)
        F21, gf = hypotheses_f(prep, sel, eig)
        sf, jf, nf = check_fundamental(prep, F21, sigma)
        out["scores_h"][g], out["scores_f"][g], out["mats_h"][g], out["mats_f"][g] = sh, sf, H21, F21
        out["gap_h"][g], out["gap_f"][g], out["near_h"][g], out["near_f"][g] = gh, gf, nh, nf
        inl_h[g], inl_f[g] = ih, jf
        out["repeated"][g] = np.array([len(set(s.tolist())) < 8 for s in sel])
        for j, h in enumerate(g):
            out["masks_h"][h], out["masks_f"][h] = mask_words(ih[j], n1), mask_words(jf[j], n1)
    # I6
    SH, SF, bh, bf = f32(0), f32(0), -1, -1
    for h in range(H):
        if out["scores_h"][h] > SH:
            SH, bh = out["scores_h"][h], h
        if out["scores_f"][h] > SF:
            SF, bf = out["scores_f"][h], h
    with np.errstate(all="ignore"):
        RH = f32(SH / (SH + SF))
    use_h = bool(f64(RH) > 0.40)
    out.update(best_h=bh, best_f=bf, SH=SH, SF=SF, RH=RH, used_homography=int(use_h))
    if bh >= 0:
        out["H21"] = out["mats_h"][bh].copy()
    if bf >= 0:
        out["F21"] = out["mats_f"][bf].copy()
    sel = bh if use_h else bf
    if sel < 0:
        return out
    inl = inl_h[sel] if use_h else inl_f[sel]
    Ni = int(inl.sum())
    out["n_inliers"] = Ni
    if use_h:
        mo, out["svd_gap"] = motions_h(out["H21"], K, eig)
        if mo is None:
            return out
        Rs, ts = mo
    else:
        Rs, ts = motions_f(out["F21"], K, eig)
    out["n_motions"] = len(Rs)
    out["motions"] = (Rs, ts)
    rts = [check_rt(prep, Rs[m], ts[m], inl, K, sigma, eig) for m in range(len(Rs))]
    for m, r in enumerate(rts):
        out["n_good"][m], out["cos_parallax"][m] = r["n_good"], r["cos"]
        out["rt_gap"], out["rt_near"] = min(out["rt_gap"], r["gap"]), min(out["rt_near"], r.get("near", np.inf))
    ng = [int(x) for x in out["n_good"]]
    lim_f, lim_h = cos_limit(min_par, True), cos_limit(min_par, False)
    best, second, success = -1, 0, False
    if use_h:
        best_good = 0
        for i in range(8):
            if ng[i] > best_good:
                second, best_good, best = best_good, ng[i], i
            elif ng[i] > second:
                second = ng[i]
        success = best >= 0 and second < 0.75 * best_good and bool(out["cos_parallax"][best] <= lim_h) and \
            best_good > min_tri and best_good > 0.9 * Ni
    else:
        max_good = max(ng[:4])
        n_min_good = max(int(0.9 * Ni), min_tri)
        second = sum(1 for i in range(4) if ng[i] > 0.7 * max_good)
        best = [i for i in range(4) if ng[i] == max_good][0]
        success = (not (max_good < n_min_good or second > 1)) and bool(out["cos_parallax"][best] <= lim_f)
    out.update(best_motion=best, second_best_good=second, success=int(success))
    if best >= 0 and ng[best] > 0:
        out["parallax_deg"] = parallax_of(out["cos_parallax"][best])
    if success:
        out.update(R21=Rs[best].copy(), t21=ts[best].copy(), P3D=rts[best]["P3D"], triangulated=rts[best]["good"])
    return out


# ---- scenes ------------------------------------------------------------------------------------------------------------
def _rot(axis_angle):
    w = np.asarray(axis_angle, f64)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx


def make_scene(n, seed, kind="general", n_hyp=24, n1=None, n2=None, noise_px=None, outlier_frac=0.1, K=K_DEFAULT,
               n_inliers_planted=None):
    """A seeded two-view scene of a 640x480 camera: n matched pairs scattered over n1 rows of frame 1 (the others -1) and a
    permutation of n2 key points of frame 2; sets drawn without replacement.  kind:
      general   points at depths 2-10 m, baseline 0.5 m and a small rotation: the F branch succeeds
      planar    points on a tilted plane about 5 m away, 0.7 px noise: the H branch succeeds
      rotation  no baseline: whatever branch is taken, reconstruction is rejected
      few       general, but only n_inliers_planted (default 30 < min_triangulated = 50) pairs follow the motion
    Returns the problem dict with "true": the planted R21, t21."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = K
    n1 = n + n // 3 + 2 if n1 is None else n1
    n2 = n + n // 4 + 5 if n2 is None else n2
    if noise_px is None:
        noise_px = 0.7 if kind == "planar" else 0.3
    R = _rot(rng.normal(0, 0.03, 3))
    t = np.array([0.5, 0.05, 0.02]) + rng.normal(0, 0.02, 3)
    if kind == "rotation":
        R, t = _rot(rng.normal(0, 0.05, 3)), np.zeros(3)
    u, v = rng.uniform(20, 620, n), rng.uniform(20, 460, n)
    x, y = (u - cx) / fx, (v - cy) / fy
    if kind == "planar":
        nrm, d = np.array([0.15, -0.1, 1.0]), 5.0          # plane n . X = d
        z = d / (nrm[0] * x + nrm[1] * y + nrm[2])
    else:
        z = rng.uniform(2.0, 10.0, n)
    X1 = np.stack([x * z, y * z, z], 1)
    X2 = X1 @ R.T + t
    uv1 = np.stack([u, v], 1)
    uv2 = np.stack([fx * X2[:, 0] / X2[:, 2] + cx, fy * X2[:, 1] / X2[:, 2] + cy], 1)
    uv1, uv2 = uv1 + rng.normal(0, noise_px, (n, 2)), uv2 + rng.normal(0, noise_px, (n, 2))
    outl = rng.random(n) < outlier_frac
    if kind == "few":
        keep = int(30 if n_inliers_planted is None else n_inliers_planted)
        outl = np.ones(n, bool)
        outl[rng.permutation(n)[:keep]] = False
    uv2[outl] = np.stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)], 1)[outl]
    rows1, rows2 = np.sort(rng.permutation(n1)[:n]), rng.permutation(n2)[:n]
    kp1 = np.stack([rng.uniform(0, 640, n1), rng.uniform(0, 480, n1)], 1)
    kp2 = np.stack([rng.uniform(0, 640, n2), rng.uniform(0, 480, n2)], 1)
    kp1[rows1], kp2[rows2] = uv1, uv2
    m = np.full(n1, -1, np.int32)
    m[rows1] = rows2
    sets = np.zeros((n_hyp, 8), np.int32)
    for h in range(n_hyp):
        if n >= 8:
            sets[h] = rng.choice(n, 8, replace=False)
    return {"kp1": kp1.astype(f32), "kp2": kp2.astype(f32), "matches12": m, "sets": sets, "K": K, "sigma": 1.0,
            "min_parallax": 1.0, "min_triangulated": 50, "true": {"R": R, "t": t}, "outlier": outl, "kind": kind}


# key -> (N, seed, kind, n_hyp): 8 / 9 around the minimal set, 63 / 64 / 65 around a mask word, 300 with the reference's
# 200 hypotheses, 1200; the four kinds at N = 300
PARITY_SCENES = {"8": (8, 9008, "general", 24), "9": (9, 9009, "general", 24), "63": (63, 9063, "general", 24),
                 "64": (64, 9064, "general", 24), "65": (65, 10065, "general", 24), "300": (300, 9300, "general", 24),
                 "300x200": (300, 10301, "general", 200), "1200": (1200, 10120, "general", 24),
                 "general": (300, 9401, "general", 24), "planar": (300, 13402, "planar", 24),
                 "rotation": (300, 20403, "rotation", 24), "few": (300, 9404, "few", 24)}
# The seeds are the first of seed0 + 1000 k for which the model alone (model_pass) has spread 0 -- its Jacobi and eigh paths
# agree in every float, so the device is compared bit for bit -- leaves out at most LEFT_OUT_CAP of the hypotheses and
# gives the verdict of the scene's kind.  Without a baseline the fundamental matrix is not determined: the rotation scene
# leaves out 3 of its 48 hypotheses.
# what each kind's name says: (used_homography or None for either, success)
VERDICTS = {"general": (0, 1), "planar": (1, 1), "rotation": (None, 0), "few": (None, 0)}


def parity_scene(key):
    n, seed, kind, n_hyp = PARITY_SCENES[key]
    return make_scene(n, seed, kind, n_hyp=n_hyp)


NGOOD_SEEDS = {50: 17550, 51: 20551, 52: 10552}   # chosen as PARITY_SCENES' seeds are


def ngood_scene(n_good):
    """A noise-free general scene whose best motion has exactly n_good good pairs (50, 51, 52: the rank min(50, nGood - 1)
    on both sides of the clamp); min_triangulated is lowered so that it is accepted."""
    sc = make_scene(n_good, NGOOD_SEEDS[n_good], "general", n_hyp=24, noise_px=0.0, outlier_frac=0.0)
    sc["min_triangulated"] = 20
    return sc


# ---- what is compared --------------------------------------------------------------------------------------------------
# A hypothesis is not well-conditioned when the gap between the two smallest eigenvalues of its A'A (and, for F, a gap of
# the rank-2 projection's 3x3), relative to the largest, is below GAP (pnp_model.py: an eigenvector moves by about
# 2^-53 / gap under a change of algorithm, 1e-8 at 1e-8, below the 6e-8 resolution of the float it is rounded to), or when
# an index repeats in its set.
# From the bound B (on |a - b| / max(1, |a|) of a matrix's entries) to chiSquare / th: a transferred point or an epipolar
# line's coefficients move by about B x (|u| + |v| + 1) <= 1121 B for pixels inside 640x480 -- relative to a matrix whose
# entries are O(1) after the normalisation is undone only up to the image's scale, so a further factor 640 is allowed for
# it; squareDist = d'd moves by 2 |d| times that, and at the threshold |d| = sqrt(5.991) sigma, so chiSquare / th moves by
# at most 2 x 1121 x 640 B / sqrt(5.991) < 5.9e5 B.  A (hypothesis, pair) with |chiSquare / th - 1| below MARGIN_FACTOR x B
# is not compared, nor is a hypothesis that holds one.
MARGIN_FACTOR = 5.9e5


def well_conditioned(m):
    ok = ~m["repeated"]
    return ok & (m["gap_h"] >= GAP), ok & (m["gap_f"] >= GAP)


def model_pass(scene):
    """(model, spread): the model with its Jacobi, and its distance from itself with eigh over the hypotheses both call
    well-conditioned (scores and matrices), and over the final motion and points when both passes made the same discrete
    choices."""
    m, e = initialize(scene), initialize(scene, eig="eigh")
    wh, wf = well_conditioned(m)
    eh, ef = well_conditioned(e)
    m["well_h"], m["well_f"] = wh, wf
    oh, of = wh & eh, wf & ef
    spread = max(dev(m["mats_h"][oh], e["mats_h"][oh]), dev(m["mats_f"][of], e["mats_f"][of]),
                 dev(m["scores_h"][oh], e["scores_h"][oh]), dev(m["scores_f"][of], e["scores_f"][of]))
    same = all(m[k] == e[k] for k in ("best_h", "best_f", "used_homography", "best_motion", "success")) and \
        np.array_equal(m["triangulated"], e["triangulated"])
    if same:
        spread = max(spread, dev(m["R21"], e["R21"]), dev(m["t21"], e["t21"]), dev(m["P3D"], e["P3D"]))
    return m, spread


def left_out(m, bound):
    """masks over the hypotheses (H, F): not well-conditioned, or a near-threshold pair"""
    return (~m["well_h"] | (m["near_h"] < MARGIN_FACTOR * bound)), (~m["well_f"] | (m["near_f"] < MARGIN_FACTOR * bound))
