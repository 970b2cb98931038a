"""PnPsolver (PnPsolver.cc: EPnP + RANSAC for relocalisation) restated in numpy: the definition the device entry points
(orbgpu_pnp_*, include/orbgpu.h P1-P10) are compared with -- vs CPU restatement; OpenCV boundary unpinned.

Everything from the correspondences to R, t runs in float64 with one rounding per operation, in the order written here;
every function works on a batch of B independent problems at once (leading axis), which changes no bit.  A sum over the
points of a set is a WAVE SUM: lane l of 64 adds the terms l, l + 64, ... in that order starting from +0.0, then the 64
partial sums are folded by halves (lane l += lane l + 32, then + 16, ... + 1).  eig="eigh" swaps the Jacobi for
numpy.linalg.eigh / the same downstream steps: the second eigen-path, whose distance from the first is the "spread"."""
import math

import numpy as np

from jacobi_model import JACOBI_STOP, jacobi_sym_batch  # noqa: F401  (the one Jacobi of the models)
from sim3_model import _log, iteration_cap, reference_random_int  # noqa: F401  (what the two solvers' models share)

f32, f64 = np.float32, np.float64
NLEVELS = 8
SIGMA2 = (f32(1.2) ** np.arange(NLEVELS, dtype=f32)) ** 2
INT_MAX = 2 ** 31 - 1
LANES = 64
JACOBI_SWEEPS = 30
CC_REL = 1e-6      # P5: 1 / k_i = 0 when k_i <= CC_REL * k_0 (the set has no extent along axis i: coplanar, collinear)
LS_REL = 1e-12     # P5: eigenvalues of L'L at or below LS_REL x the largest are dropped from the least-squares solve
MAX_N1, MAX_HYP, MIN_SET_LO, MIN_SET_HI = 16384, 4096, 4, 64
PAIRS6 = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


# ---- P3 ----------------------------------------------------------------------------------------------------------------
def ransac_parameters(n, probability, min_inliers, max_iterations, min_set, epsilon):
    """SetRansacParameters (:121-152).  Returns (adjusted min_inliers, max_its)."""
    with np.errstate(all="ignore"):
        v = f32(n) * f32(epsilon)                      # int nMinInliers = N * mRansacEpsilon
        nmin = int(v) if np.isfinite(v) and -2 ** 31 <= v <= INT_MAX else INT_MAX
    nmin = max(nmin, min_inliers, min_set)
    if n == 0:
        return nmin, 1
    eps = f32(epsilon)
    ratio = f32(nmin) / f32(n)
    if eps < ratio:
        eps = ratio
    nit = 1 if nmin == n else iteration_cap(probability, eps)
    return nmin, max(1, min(nit, max_iterations))


# ---- P4 (reference_random_int: sim3_model.py) --------------------------------------------------------------------------
def sample_sets(n, iterations, min_set, random_int):
    """The draw of PnPsolver::iterate (:188-201) replayed: position idx, not randi, is overwritten with the last entry,
    so an index can come twice.  random_int(lo, hi) is called min_set times per iteration.  n < min_set and a random_int
    outside [lo, hi] are refused, as orbgpu_shim::PnPSampleSets refuses them."""
    if n < min_set:
        raise ValueError("fewer correspondences than the minimal set")
    out = np.zeros((iterations, min_set), np.int32)
    for it in range(iterations):
        avail = list(range(n))
        size = n
        for i in range(min_set):
            randi = random_int(0, size - 1)
            if not 0 <= randi < size:
                raise ValueError("RandomInt outside [min, max]")
            idx = avail[randi]
            out[it, i] = idx
            avail[idx] = avail[size - 1]
            size -= 1
    return out


# ---- P8 ----------------------------------------------------------------------------------------------------------------
class RansacState:
    """mnIterations / mnBestInliers between calls of iterate.  counts[h]: inliers of hypothesis h; refine(h) -> refined
    count of the inlier set of hypothesis h (called for records only: Refine reads mvbBestInliers, which only a record
    changes, and an unsuccessful Refine of the same set stays unsuccessful)."""

    def __init__(self, n, min_inliers, max_its):
        self.n, self.min_inliers, self.max_its = n, min_inliers, max_its
        self.iterations, self.best, self.best_iteration = 0, 0, -1

    def iterate(self, n_iterations, counts, refine):
        """Returns (accepted iteration or -1, refined count, no_more, ran_out).  ran_out: the scan needs hypothesis
        len(counts), which is not there -- draw more and call again."""
        if self.n < self.min_inliers:
            return -1, 0, True, False
        cur = 0
        while self.iterations < self.max_its or cur < n_iterations:   # the reference's ||
            if self.iterations >= len(counts):
                return -1, 0, False, True
            cur += 1
            it = self.iterations
            self.iterations += 1
            c = int(counts[it])
            if c >= self.min_inliers and c > self.best:
                self.best, self.best_iteration = c, it
                rc = int(refine(it))
                if rc > self.min_inliers:
                    return it, rc, False, False
        return -1, 0, self.iterations >= self.max_its, False


# ---- P5 ----------------------------------------------------------------------------------------------------------------
def wave_sum(C):
    """C [B][n][...] -> [B][...], the wave sum of the module docstring."""
    C = np.asarray(C, f64)
    B, n = C.shape[:2]
    rows = max((n + LANES - 1) // LANES, 1)
    pad = np.zeros((B, rows * LANES) + C.shape[2:], f64)
    pad[:, :n] = C
    pad = pad.reshape((B, rows, LANES) + C.shape[2:])
    with np.errstate(all="ignore"):
        acc = np.zeros((B, LANES) + C.shape[2:], f64)
        for r in range(rows):
            acc = acc + pad[:, r]
        s = LANES // 2
        while s >= 1:
            acc[:, :s] = acc[:, :s] + acc[:, s:2 * s]
            s //= 2
    return acc[:, 0].copy()


def jacobi(A):
    """Cyclic Jacobi on symmetric [B][m][m]: pairs row by row, at most 30 sweeps, H6's stopping rule and rotation.
    Returns (eigenvalues [B][m] = the diagonal, V [B][m][m] with eigenvectors in columns), unsorted."""
    return jacobi_sym_batch(A, JACOBI_SWEEPS)


def sym_eig(A, eig, sweeps=JACOBI_SWEEPS):
    """(w, V) unsorted for the Jacobi, ascending for eigh; a matrix with a NaN or inf gives NaN in both."""
    if eig == "jacobi":
        return jacobi_sym_batch(A, sweeps)
    A = np.array(A, f64)
    B, m = A.shape[:2]
    w, V = np.full((B, m), np.nan), np.full((B, m, m), np.nan)
    ok = np.isfinite(A).all((1, 2))
    if ok.any():
        w[ok], V[ok] = np.linalg.eigh(A[ok])
    return w, V


def sign_rule(v):
    """[..., m] vectors: flipped so that the component of largest magnitude (lowest index on ties) is positive"""
    k = np.argmax(np.abs(v), axis=-1)
    lead = np.take_along_axis(v, k[..., None], -1)
    return np.where(lead < 0.0, -v, v)


def sorted_eig(A, eig, sweeps=JACOBI_SWEEPS):
    """Eigenvalues descending (stable), eigenvectors as ROWS with the sign rule: what the SVD of a symmetric positive
    semi-definite matrix with CV_SVD_U_T hands the reference, made definite."""
    w, V = sym_eig(A, eig, sweeps)
    order = np.argsort(-w, axis=1, kind="stable")
    w = np.take_along_axis(w, order, 1)
    Vt = np.take_along_axis(np.swapaxes(V, 1, 2), order[:, :, None], 1)
    return w, sign_rule(Vt)


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def canonical_basis(vs, k):
    """vs [B][k][12]: an orthonormal basis of the structurally singular subspace, smallest eigenvalue first.  Returns the
    canonical basis of the same subspace: the projector's columns orthonormalised by pivoted Gram-Schmidt (largest
    remaining column, lowest index on ties), each vector with the sign rule."""
    B = vs.shape[0]
    with np.errstate(all="ignore"):
        Q = np.zeros((B, 12, 12))
        for j in range(k):
            Q = Q + vs[:, j, :, None] * vs[:, j, None, :]
        out = np.zeros((B, k, 12))
        for s in range(k):
            n2 = np.zeros((B, 12))
            for r in range(12):
                n2 = n2 + Q[:, r, :] * Q[:, r, :]
            piv = np.argmax(n2, axis=1)
            nrm = np.sqrt(np.take_along_axis(n2, piv[:, None], 1))
            b = np.take_along_axis(Q, piv[:, None, None].repeat(12, 1), 2)[:, :, 0] / nrm
            b = sign_rule(b)
            out[:, s] = b
            d = np.zeros((B, 12))
            for r in range(12):
                d = d + b[:, r, None] * Q[:, r, :]
            Q = Q - d[:, None, :] * b[:, :, None]
    return out


def lstsq_min_norm(L, rho, eig):
    """x [B][k] minimising |L x - rho| with the least norm: eigen-decomposition of L'L (sums over the six rows in
    order), x = sum_i v_i (v_i . L'rho) / w_i over the eigenvalues above LS_REL x the largest, in the solver's order.
    Also returns how close an eigenvalue came to that threshold (least |log10(w_i / threshold)|)."""
    B, _, k = L.shape
    with np.errstate(all="ignore"):
        Nm, g = np.zeros((B, k, k)), np.zeros((B, k))
        for i in range(6):
            Nm = Nm + L[:, i, :, None] * L[:, i, None, :]
            g = g + L[:, i, :] * rho[:, i, None]
        w, V = sym_eig(Nm, eig)
        wmax = w[:, 0].copy()
        for i in range(1, k):
            wmax = np.where(w[:, i] > wmax, w[:, i], wmax)
        thr = LS_REL * wmax
        x = np.zeros((B, k))
        for i in range(k):
            pr = np.zeros(B)
            for a in range(k):
                pr = pr + V[:, a, i] * g[:, a]
            coef = np.where(w[:, i] <= thr, 0.0, pr / w[:, i])
            x = x + coef[:, None] * V[:, :, i]
        near = np.abs(np.log10(np.abs(w) / thr[:, None]))
        near = np.where(np.isfinite(near), near, np.inf).min(1)
    return x, near


def qr_solve(A, b):
    """Householder QR of [B][6][4], x [B][4]; a zero pivot column gives x = 0."""
    A, b = np.array(A, f64), np.array(b, f64)
    B = A.shape[0]
    A1, A2 = np.zeros((B, 4)), np.zeros((B, 4))
    sing = np.zeros(B, bool)
    with np.errstate(all="ignore"):
        for k in range(4):
            eta = np.abs(A[:, k, k])
            for i in range(k + 1, 6):
                elt = np.abs(A[:, i, k])
                eta = np.where(eta < elt, elt, eta)
            sing |= eta == 0.0
            inv_eta = 1.0 / eta
            ssum = np.zeros(B)
            for i in range(k, 6):
                A[:, i, k] = A[:, i, k] * inv_eta
                ssum = ssum + A[:, i, k] * A[:, i, k]
            sigma = np.sqrt(ssum)
            sigma = np.where(A[:, k, k] < 0.0, -sigma, sigma)
            A[:, k, k] = A[:, k, k] + sigma
            A1[:, k] = sigma * A[:, k, k]
            A2[:, k] = -eta * sigma
            for j in range(k + 1, 4):
                ssum = np.zeros(B)
                for i in range(k, 6):
                    ssum = ssum + A[:, i, k] * A[:, i, j]
                tau = ssum / A1[:, k]
                for i in range(k, 6):
                    A[:, i, j] = A[:, i, j] - tau * A[:, i, k]
        for j in range(4):
            tau = np.zeros(B)
            for i in range(j, 6):
                tau = tau + A[:, i, j] * b[:, i]
            tau = tau / A1[:, j]
            for i in range(j, 6):
                b[:, i] = b[:, i] - tau * A[:, i, j]
        x = np.zeros((B, 4))
        x[:, 3] = b[:, 3] / A2[:, 3]
        for i in (2, 1, 0):
            ssum = np.zeros(B)
            for j in range(i + 1, 4):
                ssum = ssum + A[:, i, j] * x[:, j]
            x[:, i] = (b[:, i] - ssum) / A2[:, i]
    return np.where(sing[:, None], 0.0, x)


def gauss_newton(L, rho, betas):
    b = betas.copy()
    B = L.shape[0]
    with np.errstate(all="ignore"):
        for _ in range(5):
            A, r = np.zeros((B, 6, 4)), np.zeros((B, 6))
            for i in range(6):
                l = [L[:, i, c] for c in range(10)]
                A[:, i, 0] = (((2.0 * l[0]) * b[:, 0] + l[1] * b[:, 1]) + l[3] * b[:, 2]) + l[6] * b[:, 3]
                A[:, i, 1] = ((l[1] * b[:, 0] + (2.0 * l[2]) * b[:, 1]) + l[4] * b[:, 2]) + l[7] * b[:, 3]
                A[:, i, 2] = ((l[3] * b[:, 0] + l[4] * b[:, 1]) + (2.0 * l[5]) * b[:, 2]) + l[8] * b[:, 3]
                A[:, i, 3] = ((l[6] * b[:, 0] + l[7] * b[:, 1]) + l[8] * b[:, 2]) + (2.0 * l[9]) * b[:, 3]
                s = (l[0] * b[:, 0]) * b[:, 0]
                s = s + (l[1] * b[:, 0]) * b[:, 1]
                s = s + (l[2] * b[:, 1]) * b[:, 1]
                s = s + (l[3] * b[:, 0]) * b[:, 2]
                s = s + (l[4] * b[:, 1]) * b[:, 2]
                s = s + (l[5] * b[:, 2]) * b[:, 2]
                s = s + (l[6] * b[:, 0]) * b[:, 3]
                s = s + (l[7] * b[:, 1]) * b[:, 3]
                s = s + (l[8] * b[:, 2]) * b[:, 3]
                s = s + (l[9] * b[:, 3]) * b[:, 3]
                r[:, i] = rho[:, i] - s
            b = b + qr_solve(A, r)
    return b


def betas_from(x, kind):
    """The three approximations' beta vectors from the least-squares solution x (columns 0136 / 012 / 01234 of L)."""
    B = x.shape[0]
    b = np.zeros((B, 4))
    with np.errstate(all="ignore"):
        neg = x[:, 0] < 0.0
        b0 = np.where(neg, np.sqrt(-x[:, 0]), np.sqrt(x[:, 0]))
        if kind == 1:
            b[:, 0] = b0
            for i in (1, 2, 3):
                b[:, i] = np.where(neg, -x[:, i], x[:, i]) / b0
            return b
        b1 = np.where(neg, np.where(x[:, 2] < 0.0, np.sqrt(-x[:, 2]), 0.0), np.where(x[:, 2] > 0.0, np.sqrt(x[:, 2]), 0.0))
        b0 = np.where(x[:, 1] < 0.0, -b0, b0)
        b[:, 0], b[:, 1] = b0, b1
        if kind == 3:
            b[:, 2] = x[:, 3] / b0
    return b


def pose_from_betas(betas, vs, al, pw, uv, c0, K, n, eig):
    """compute_R_and_t: control points in the camera frame, sign, the absolute orientation, the mean reprojection error."""
    fu, fv, uc, vc = K
    B = betas.shape[0]
    with np.errstate(all="ignore"):
        ccs = np.zeros((B, 12))
        for i in range(4):
            ccs = ccs + betas[:, i, None] * vs[:, i, :]
        ccs = ccs.reshape(B, 4, 3)

        def pcs_of(a):
            return ((a[..., 0, None] * ccs[:, None, 0] + a[..., 1, None] * ccs[:, None, 1]) + a[..., 2, None] * ccs[:, None, 2]) + \
                a[..., 3, None] * ccs[:, None, 3]
        first = pcs_of(al[:, :1])
        ccs = np.where((first[:, 0, 2] < 0.0)[:, None, None], -ccs, ccs)
        pcs = pcs_of(al)
        pc0 = wave_sum(pcs) / float(n)
        dc, dw = pcs - pc0[:, None], pw - c0[:, None]
        abt = wave_sum(dc[:, :, :, None] * dw[:, :, None, :])          # [B][j][m]
        S = np.zeros((B, 3, 3))
        for j in range(3):
            S = S + abt[:, j, :, None] * abt[:, j, None, :]
        _, V = sym_eig(S, eig)
        R = np.zeros((B, 3, 3))
        for k in range(3):
            u = (abt[:, :, 0] * V[:, 0, k, None] + abt[:, :, 1] * V[:, 1, k, None]) + abt[:, :, 2] * V[:, 2, k, None]
            u = u / np.sqrt((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2])[:, None]
            R = R + u[:, :, None] * V[:, None, :, k]
        r = R.reshape(B, 9)
        det = r[:, 0] * r[:, 4] * r[:, 8] + r[:, 1] * r[:, 5] * r[:, 6]
        det = det + r[:, 2] * r[:, 3] * r[:, 7]
        det = det - r[:, 2] * r[:, 4] * r[:, 6]
        det = det - r[:, 1] * r[:, 3] * r[:, 8]
        det = det - r[:, 0] * r[:, 5] * r[:, 7]
        R[:, 2] = np.where((det < 0.0)[:, None], -R[:, 2], R[:, 2])
        t = pc0 - np.stack([dot3(R[:, i], c0) for i in range(3)], 1)
        Xc = dot3(R[:, None, 0], pw) + t[:, None, 0]
        Yc = dot3(R[:, None, 1], pw) + t[:, None, 1]
        iz = 1.0 / (dot3(R[:, None, 2], pw) + t[:, None, 2])
        du = uv[:, :, 0] - (uc + (fu * Xc) * iz)
        dv = uv[:, :, 1] - (vc + (fv * Yc) * iz)
        err = wave_sum(np.sqrt(du * du + dv * dv)) / float(n)
    return R, t, err


def epnp(pw, uv, K, eig="jacobi", canonical=True, perturb=None):
    """compute_pose over B sets of n points.  pw [B][n][3], uv [B][n][2] float64; K = (fx, fy, cx, cy).
    Returns a dict: R [B][3][3], t [B][3] float64, err (the chosen mean reprojection error), gap (least relative gap at
    the places where eigenvalues are ordered), thr (least distance, in decades, of an eigenvalue or axis length from a
    threshold), choice (distance of the chosen error from the next one / max(1, chosen)).
    perturb [B][12][12]: relative perturbation of M'M (the null-space experiment)."""
    pw, uv = np.asarray(pw, f64), np.asarray(uv, f64)
    B, n = pw.shape[:2]
    fu, fv, uc, vc = (float(f32(k)) for k in K)
    with np.errstate(all="ignore"):
        c0 = wave_sum(pw) / float(n)
        d = pw - c0[:, None]
        C3 = wave_sum(d[:, :, :, None] * d[:, :, None, :])
        w3, U3 = sorted_eig(C3, eig)
        w3c = np.where(w3 < 0.0, 0.0, w3)
        kk = np.sqrt(w3c / float(n))
        inv_k = np.where(kk <= CC_REL * kk[:, :1], 0.0, 1.0 / kk)
        cws = np.concatenate([c0[:, None], c0[:, None] + kk[:, :, None] * U3], 1)       # [B][4][3]
        ci = inv_k[:, :, None] * U3
        al = np.zeros((B, n, 4))
        for j in range(3):
            al[:, :, 1 + j] = (ci[:, None, j, 0] * d[:, :, 0] + ci[:, None, j, 1] * d[:, :, 1]) + ci[:, None, j, 2] * d[:, :, 2]
        al[:, :, 0] = ((1.0 - al[:, :, 1]) - al[:, :, 2]) - al[:, :, 3]
        M1, M2 = np.zeros((B, n, 12)), np.zeros((B, n, 12))
        for i in range(4):
            M1[:, :, 3 * i] = al[:, :, i] * fu
            M1[:, :, 3 * i + 2] = al[:, :, i] * (uc - uv[:, :, 0])
            M2[:, :, 3 * i + 1] = al[:, :, i] * fv
            M2[:, :, 3 * i + 2] = al[:, :, i] * (vc - uv[:, :, 1])
        MtM = wave_sum(M1[:, :, :, None] * M1[:, :, None, :] + M2[:, :, :, None] * M2[:, :, None, :])
        if perturb is not None:
            MtM = MtM * (1.0 + perturb)
        w12, Ut = sorted_eig(MtM, eig)
        vs = Ut[:, ::-1][:, :4].copy()                    # v[0] = the smallest eigenvalue's vector ... v[3]
        k = max(0, 12 - 2 * n)
        if canonical and k > 0:
            vs[:, :k] = canonical_basis(vs[:, :k], k)
        # well-conditioning figures: ordering of the PCA axes, of the four smallest of M'M beyond the canonical part
        gap3 = np.minimum(w3[:, 0] - w3[:, 1], w3[:, 1] - w3[:, 2]) / np.abs(w3[:, 0])
        asc = w12[:, ::-1]
        places = [j for j in range(1, 5) if not (canonical and j < k)]   # gap between the j-th and (j+1)-th smallest
        gap12 = np.min(np.stack([asc[:, j] - asc[:, j - 1] for j in places], 1), 1) / np.abs(w12[:, 0])
        gap = np.where(np.isfinite(gap3) & np.isfinite(gap12), np.minimum(gap3, gap12), 0.0)
        thr = np.abs(np.log10(kk / (CC_REL * kk[:, :1])))
        thr = np.where(np.isfinite(thr), thr, np.inf).min(1)
        L = np.zeros((B, 6, 10))
        rho = np.zeros((B, 6))
        v4 = vs.reshape(B, 4, 4, 3)
        for i, (a, b) in enumerate(PAIRS6):
            dv = v4[:, :, a] - v4[:, :, b]                # [B][4 vectors][3]
            L[:, i, 0] = dot3(dv[:, 0], dv[:, 0])
            L[:, i, 1] = 2.0 * dot3(dv[:, 0], dv[:, 1])
            L[:, i, 2] = dot3(dv[:, 1], dv[:, 1])
            L[:, i, 3] = 2.0 * dot3(dv[:, 0], dv[:, 2])
            L[:, i, 4] = 2.0 * dot3(dv[:, 1], dv[:, 2])
            L[:, i, 5] = dot3(dv[:, 2], dv[:, 2])
            L[:, i, 6] = 2.0 * dot3(dv[:, 0], dv[:, 3])
            L[:, i, 7] = 2.0 * dot3(dv[:, 1], dv[:, 3])
            L[:, i, 8] = 2.0 * dot3(dv[:, 2], dv[:, 3])
            L[:, i, 9] = dot3(dv[:, 3], dv[:, 3])
            dd = cws[:, a] - cws[:, b]
            rho[:, i] = dot3(dd, dd)
        sols = []
        for kind, cols in ((1, (0, 1, 3, 6)), (2, (0, 1, 2)), (3, (0, 1, 2, 3, 4))):
            x, near = lstsq_min_norm(L[:, :, cols], rho, eig)
            thr = np.minimum(thr, near)
            b = gauss_newton(L, rho, betas_from(x, kind))
            sols.append(pose_from_betas(b, vs, al, pw, uv, c0, (fu, fv, uc, vc), n, eig))
        R, t, err = (a.copy() for a in sols[0])
        pick = np.zeros(B, int)
        for s in (1, 2):
            better = sols[s][2] < err
            pick = np.where(better, s, pick)
            R, t, err = np.where(better[:, None, None], sols[s][0], R), np.where(better[:, None], sols[s][1], t), np.where(better, sols[s][2], err)
        errs = np.stack([s[2] for s in sols], 1)
        others = np.where(np.arange(3)[None] == pick[:, None], np.inf, np.abs(errs - err[:, None]))
        others = np.where(np.isnan(others), 0.0, others)
        choice = others.min(1) / np.maximum(1.0, np.abs(err))
        choice = np.where(np.isnan(choice), 0.0, choice)
    return {"R": R, "t": t, "err": err, "gap": gap, "thr": thr, "choice": choice, "errs": errs}


# ---- P1 / P2 / P6 / P9 -------------------------------------------------------------------------------------------------
def prepare(pr):
    n1 = len(pr["valid"])
    nl = int(pr.get("nlevels", len(pr["level_sigma2"])))
    o = np.asarray(pr["octave"], np.int64)
    valid = np.asarray(pr["valid"]) != 0
    in_range = (o >= 0) & (o < nl)
    idx = np.flatnonzero(valid & in_range)
    with np.errstate(all="ignore"):
        me = np.asarray(pr["level_sigma2"], f32) * f32(pr["th2"])
    return {"n1": n1, "N": len(idx), "indices": idx.astype(np.int32), "n_bad_index": int((valid & ~in_range).sum()),
            "p2d": np.asarray(pr["kp"], f32).reshape(n1, 2)[idx], "p3d": np.asarray(pr["Xw"], f32).reshape(n1, 3)[idx],
            "max_error": me[o[idx]] if len(idx) else np.zeros(0, f32)}


def check_inliers(prep, R, t, K):
    """CheckInliers for B poses over all N rows.  Returns (inlier [B][N], least |error2 / maxError - 1| [B])."""
    fu, fv, uc, vc = (float(f32(k)) for k in K)
    P, p2 = prep["p3d"].astype(f64)[None], prep["p2d"]
    B = R.shape[0]
    if prep["N"] == 0:
        return np.zeros((B, 0), bool), np.full(B, np.inf)
    with np.errstate(all="ignore"):
        def row(i):
            return ((R[:, i, 0, None] * P[:, :, 0] + R[:, i, 1, None] * P[:, :, 1]) + R[:, i, 2, None] * P[:, :, 2]) + t[:, i, None]
        Xc, Yc = row(0).astype(f32), row(1).astype(f32)
        invZ = (1.0 / row(2)).astype(f32)
        ue = uc + (fu * Xc.astype(f64)) * invZ.astype(f64)
        ve = vc + (fv * Yc.astype(f64)) * invZ.astype(f64)
        dx = (p2[None, :, 0].astype(f64) - ue).astype(f32)
        dy = (p2[None, :, 1].astype(f64) - ve).astype(f32)
        e2 = dx * dx + dy * dy
        inl = e2 < prep["max_error"][None]
        r = np.abs(e2.astype(f64) / prep["max_error"][None].astype(f64) - 1.0)
        r = np.where(np.isfinite(r), r, np.inf)
    return inl, r.min(1)


def mask_words(inl, indices, n1):
    bits = np.zeros(((n1 + 63) // 64) * 64, np.uint8)
    bits[indices[inl]] = 1
    return np.packbits(bits.reshape(-1, 8), axis=1, bitorder="little").reshape(-1).view(np.uint64).copy() if n1 else np.zeros(0, np.uint64)


def tcw_of(R, t):
    """P9: the float of R, t entry by entry in a 4x4 identity"""
    B = R.shape[0]
    T = np.zeros((B, 4, 4), f32)
    T[:, 3, 3] = 1.0
    with np.errstate(all="ignore"):
        T[:, :3, :3], T[:, :3, 3] = R.astype(f32), t.astype(f32)
    return T


def solve(pr, eig="jacobi", start_iteration=0, best_so_far=0, n_iterations=0):
    """The whole solver over pr["sets"] [H][min_set].  Per-hypothesis lists cover the first
    n_use = min(H, max(max_its, start_iteration + n_iterations)) sets (none if N < the adjusted min_inliers).
    n_iterations: iterate's argument (0: scan to max_its)."""
    prep = prepare(pr)
    N, n1 = prep["N"], prep["n1"]
    K = pr["K"]
    sets = np.asarray(pr["sets"], np.int64)
    min_set = int(pr["min_set"])
    sets = sets.reshape(-1, min_set)
    H = len(sets)
    mi, max_its = ransac_parameters(N, pr["probability"], pr["min_inliers"], pr["max_iterations"], min_set, pr["epsilon"])
    n_use = 0 if N < mi else min(H, max(max_its, start_iteration + n_iterations))
    words = (n1 + 63) // 64
    out = {"N": N, "min_inliers": mi, "max_its": max_its, "n_use": n_use, "n_bad_index": prep["n_bad_index"], "n_bad_set": 0,
           "indices": prep["indices"], "counts": np.zeros(H, np.int32), "masks": np.zeros((H, words), np.uint64),
           "Tcw": np.zeros((H, 4, 4), f32), "gap": np.zeros(H), "thr": np.zeros(H), "choice": np.zeros(H),
           "near": np.full(H, math.inf), "repeated": np.zeros(H, bool), "prep": prep}
    use = sets[:n_use]
    good = np.array([N > 0 and s.min() >= 0 and s.max() < N for s in use], bool) if n_use else np.zeros(0, bool)
    out["n_bad_set"] = int((~good).sum())
    out["Tcw"][:n_use][~good] = np.nan
    for k in ("gap", "thr", "choice"):                   # a refused set is NaN and 0 by definition: nothing to be sensitive
        out[k][:n_use][~good] = np.inf
    inl_all = np.zeros((H, N), bool)
    if good.any():
        g = np.flatnonzero(good)
        sel = use[g]
        hyp = epnp(prep["p3d"].astype(f64)[sel], prep["p2d"].astype(f64)[sel], K, eig)
        inl, near = check_inliers(prep, hyp["R"], hyp["t"], K)
        inl_all[g] = inl
        out["counts"][g] = inl.sum(1)
        out["Tcw"][g] = tcw_of(hyp["R"], hyp["t"])
        for k in ("gap", "thr", "choice"):
            out[k][g] = hyp[k]
        out["near"][g] = near
        out["repeated"][g] = np.array([len(set(s.tolist())) < min_set for s in sel])
        for j, h in enumerate(g):
            out["masks"][h] = mask_words(inl[j], prep["indices"], n1)
    refined = {}

    def refine(h):
        idx = np.flatnonzero(inl_all[h])
        r = epnp(prep["p3d"].astype(f64)[idx][None], prep["p2d"].astype(f64)[idx][None], K, eig)
        ri, rnear = check_inliers(prep, r["R"], r["t"], K)
        refined[h] = {"Tcw": tcw_of(r["R"], r["t"])[0], "inl": ri[0], "count": int(ri[0].sum()), "near": float(rnear[0]),
                      "gap": float(r["gap"][0]), "thr": float(r["thr"][0]), "choice": float(r["choice"][0])}
        return refined[h]["count"]

    st = RansacState(N, mi, max_its)
    st.iterations, st.best = start_iteration, best_so_far
    acc, n_inl, no_more, ran_out = st.iterate(n_iterations, out["counts"][:n_use], refine)
    out.update(accepted=acc, n_inliers=n_inl, no_more=bool(no_more), ran_out=ran_out, best_inliers=st.best,
               best_iteration=st.best_iteration, iterations=st.iterations, refined=refined,
               refined_Tcw=np.zeros((4, 4), f32), refined_mask=np.zeros(words, np.uint64))
    if acc >= 0:
        out["refined_Tcw"], out["refined_mask"] = refined[acc]["Tcw"], mask_words(refined[acc]["inl"], prep["indices"], n1)
    elif no_more and st.best_iteration >= 0 and st.best_iteration < n_use and st.best >= mi:
        b = st.best_iteration                            # the fallback: the best record's own pose and mask
        out["n_inliers"], out["refined_Tcw"], out["refined_mask"] = st.best, out["Tcw"][b], out["masks"][b]
    return out


# ---- scenes ------------------------------------------------------------------------------------------------------------
def _rot(rng, sigma):
    w = rng.normal(0, sigma, 3)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx


K_DEFAULT = (500.0, 500.0, 320.0, 240.0)


def planted(rng, n, noise_px=0.0):
    """n points seen by a 640x480 camera at depths 1-8 m with a planted pose: (Rcw, tcw, Xw [n][3], uv [n][2])"""
    fx, fy, cx, cy = K_DEFAULT
    R, t = _rot(rng, 0.4), rng.normal(0, 1.0, 3)
    z = rng.uniform(1.0, 8.0, n)
    u, v = rng.uniform(0, 640, n), rng.uniform(0, 480, n)
    Xc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    Xw = (Xc - t) @ R                                  # R' (Xc - t)
    uv = np.stack([u, v], 1) + rng.normal(0, noise_px, (n, 2)) if noise_px else np.stack([u, v], 1)
    return R, t, Xw, uv


def make_scene(n, seed, n1=None, n_hyp=300, min_set=4, outlier_frac=0.3, noise_px=0.7, min_inliers=10, max_iterations=300,
               probability=0.99, epsilon=0.5, th2=5.991):
    """A seeded frame with a planted pose: n kept correspondences scattered over n1 rows (640x480 camera, depths 1-8 m,
    noise_px per axis, a share of gross outliers 30-200 px off), sets drawn uniformly WITHOUT the reference's quirk
    (distinct indices).  The parameters are Tracking.cc:1690's."""
    rng = np.random.default_rng(seed)
    n1 = n + n // 3 + 2 if n1 is None else n1
    R, t, Xw, uv = planted(rng, n1, noise_px)
    out = rng.random(n1) < outlier_frac
    ang, mag = rng.uniform(0, 2 * math.pi, n1), rng.uniform(30, 200, n1)
    uv[out] += np.stack([np.cos(ang) * mag, np.sin(ang) * mag], 1)[out]
    valid = np.zeros(n1, np.uint8)
    valid[rng.permutation(n1)[:n]] = 1
    sets = np.zeros((n_hyp, min_set), np.int32)
    for h in range(n_hyp):
        sets[h] = rng.choice(n, min_set, replace=False) if n >= min_set else 0
    return {"valid": valid, "Xw": Xw.astype(f32), "kp": uv.astype(f32), "octave": rng.integers(0, 4, n1).astype(np.int32),
            "K": K_DEFAULT, "level_sigma2": SIGMA2.copy(), "probability": probability, "min_inliers": min_inliers,
            "max_iterations": max_iterations, "min_set": min_set, "epsilon": epsilon, "th2": th2, "sets": sets,
            "true": {"R": R, "t": t}, "outlier": out}


# size -> (seed, min_set); 3 < min_inliers = 10: no_more, nothing scanned; 9 / 10 / 11 around it; 63 / 64 / 65 around a
# mask word; "300/6" and "300/5": min_set 6 (no canonical part) and 5 (k = 2)
PARITY_SCENES = {"3": (3, 7003, 4), "9": (9, 7009, 4), "10": (10, 7010, 4), "11": (11, 7011, 4), "63": (63, 7063, 4),
                 "64": (64, 7064, 4), "65": (65, 7065, 4), "300": (300, 7300, 4), "1200": (1200, 8208, 4),
                 "300/6": (300, 7306, 6), "300/5": (300, 7305, 5)}


def parity_scene(key):
    n, seed, min_set = PARITY_SCENES[key]
    return make_scene(n, seed, min_set=min_set)


# ---- what is compared (shared by the CPU test that holds the seeds inside the cap and the device tests) ----------------
# A hypothesis is not well-conditioned when an eigenvalue gap at an ordering place is below GAP (relative to the largest
# eigenvalue: an eigenvector moves by about 2^-53 / gap under a change of algorithm, 1e-8 at 1e-8, below the 6e-8
# resolution of the float32 Tcw it is rounded to), when an eigenvalue or axis length lies within THR_DECADES decades of
# a threshold, or when its index repeats.
GAP = 1e-8
THR_DECADES = 1.0
BOUND_FACTOR = 16.0      # tools/fuzz_sim3.py's
LEFT_OUT_CAP = 0.10
# From the bound B (on |a - b| / max(1, |a|) of Tcw's entries) to error2 / maxError: a camera-frame coordinate moves by
# at most B (|X| + |Y| + |Z| + max(1, |t|)) <= 40 B in planted()'s geometry (world coordinates within about 12 of the
# origin, |t| < 4); a pixel by at most fx / z (1 + |x / z|) times that <= 500 / 1 x 2 x 40 B (depth >= 1, |x / z| <= 0.64
# inside the image, 2 with room for outliers); error2 = d'd by 2 |d| times the pixel shift, so error2 / maxError at the
# threshold (|d| = sqrt(maxError) >= sqrt(5.991)) by 2 x 40000 B / 2.44 < 3.3e4 B.  A (hypothesis, point) pair with
# |error2 / maxError - 1| below MARGIN_FACTOR x B is not compared, nor is a hypothesis that holds one.
MARGIN_FACTOR = 3.3e4


def dev(a, b):
    """largest |a - b| / max(1, |a|); NaN against NaN is no deviation, NaN against a number is infinite"""
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    if a.size == 0:
        return 0.0
    na, nb = np.isnan(a), np.isnan(b)
    if (na != nb).any():
        return float("inf")
    ok = ~na
    with np.errstate(all="ignore"):
        d = np.abs(a[ok] - b[ok]) / np.maximum(1.0, np.abs(a[ok]))
    d = np.where(np.isnan(d), 0.0 if np.array_equal(a[ok], b[ok]) else np.inf, d)
    return float(d.max()) if d.size else 0.0


def well_conditioned(m):
    u = m["n_use"]
    return ~m["repeated"][:u] & (m["gap"][:u] >= GAP) & (m["thr"][:u] >= THR_DECADES)


def model_pass(scene):
    """(model, spread): the model with its Jacobi, and its distance from itself with eigh over the well-conditioned
    hypotheses of both and over the refined poses both computed."""
    m, e = solve(scene), solve(scene, eig="eigh")
    u = m["n_use"]
    ok = well_conditioned(m) & well_conditioned(e)
    m["well"] = well_conditioned(m)
    spread = dev(m["Tcw"][:u][ok], e["Tcw"][:u][ok])
    for h, r in m["refined"].items():
        if h in e["refined"] and ok[h]:
            spread = max(spread, dev(r["Tcw"], e["refined"][h]["Tcw"]))
    return m, spread


def left_out(m, bound):
    """mask over the used hypotheses: not well-conditioned, a choice among the three solutions within the bound, or a
    near-threshold pair"""
    u = m["n_use"]
    return ~m["well"] | (m["choice"][:u] <= bound) | (m["near"][:u] < MARGIN_FACTOR * bound)
