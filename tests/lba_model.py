"""NumPy float64 restatement of Optimizer::LocalBundleAdjustment (Optimizer.cc:453-778): the oracle of the device local
bundle adjustment (orbgpu_local_ba*).

g2o is not part of the reference tree, so its behaviour is restated here from its published algorithm
(OptimizationAlgorithmLevenberg over BlockSolver_6_3 with the points marginalised, EdgeSE3ProjectXYZ /
EdgeStereoSE3ProjectXYZ, RobustKernelHuber, SE3Quat): every comparison against this file is "vs CPU restatement; g2o
boundary unpinned".  The definition, step by step (L1-L12), is in include/orbgpu.h above orbgpu_local_ba_device.

All arithmetic is IEEE double unless a float32 is named.  Every sum over edges, edge pairs or vertices runs sequentially;
`order` (default: edge order) is a permutation of the valid edges that every such sum follows, so that a permutation shows
what the summation order alone does to the result.
"""
import numpy as np

from pose_model import (CAMERA, DBL_MAX, DELTA_MONO, DELTA_STEREO, INV_LEVEL_SIGMA2, NLEVELS, chi2_of, huber, jacobian,  # noqa: F401
                        pose_from_Tcw, pose_matrix, pose_update, quat_to_matrix, se3_exp)

CHI2_MONO = np.float64(5.991)  # Optimizer.cc:680, :696: compared in double, unlike PoseOptimization's float
CHI2_STEREO = np.float64(7.815)
TRI6 = [(a, b) for a in range(6) for b in range(a, 6)]
TRI3 = [(a, b) for a in range(3) for b in range(a, 3)]


# ---- the pieces csrc/opt_math.h shares with the kernel (tests/test_opt_math_lba.py: bit for bit) ----------------------
def inv3_sym(h, lam):
    """Inverse of the symmetric 3x3 with upper triangle h = (00, 01, 02, 11, 12, 22) and lam added to the diagonal, by
    cofactors as Eigen's 3x3 inverse computes it: det from the first column's cofactors, one reciprocal.  Returns 3x3."""
    m = np.array([[h[0] + lam, h[1], h[2]], [h[1], h[3] + lam, h[4]], [h[2], h[4], h[5] + lam]])
    with np.errstate(all="ignore"):
        c = np.zeros((3, 3))
        for i in range(3):
            i1, i2 = (i + 1) % 3, (i + 2) % 3
            for j in range(3):
                j1, j2 = (j + 1) % 3, (j + 2) % 3
                c[i, j] = m[i1, j1] * m[i2, j2] - m[i1, j2] * m[i2, j1]
        det = (c[0, 0] * m[0, 0] + c[1, 0] * m[1, 0]) + c[2, 0] * m[2, 0]
        invdet = 1.0 / det
        return np.array([[c[j, i] * invdet for j in range(3)] for i in range(3)])


def llt_solve(A, b):
    """A x = b by LL^T for a symmetric A of any size, read through its lower triangle; (ok, x).  Left-looking columns,
    forward substitution column by column (per row: k ascending), back substitution column by column (per row: k
    DESCENDING, unlike pose_model.cholesky_solve).  A pivot that is not > 0 (NaN included): ok = False and x = 0."""
    n = len(b)
    L = np.zeros((n, n))
    dg = np.zeros(n)
    with np.errstate(all="ignore"):
        for j in range(n):
            d = A[j, j]
            for k in range(j):
                d = d - L[j, k] * L[j, k]
            if not d > 0.0:
                return False, np.zeros(n)
            sd = np.sqrt(d)
            dg[j] = sd
            for i in range(j + 1, n):
                s = A[i, j]
                for k in range(j):
                    s = s - L[i, k] * L[j, k]
                L[i, j] = s / sd
        y = np.array(b, np.float64)
        for k in range(n):
            y[k] = y[k] / dg[k]
            y[k + 1:] = y[k + 1:] - L[k + 1:, k] * y[k]
        x = y
        for k in range(n - 1, -1, -1):
            x[k] = x[k] / dg[k]
            x[:k] = x[:k] - L[k, :k] * x[k]
    return True, x


def _inv3_all(H, lam):
    """inv3_sym over rows of H [n][6] at once (the same operations per row)."""
    n = len(H)
    m = np.zeros((n, 3, 3))
    m[:, 0, 0], m[:, 0, 1], m[:, 0, 2] = H[:, 0] + lam, H[:, 1], H[:, 2]
    m[:, 1, 0], m[:, 1, 1], m[:, 1, 2] = H[:, 1], H[:, 3] + lam, H[:, 4]
    m[:, 2, 0], m[:, 2, 1], m[:, 2, 2] = H[:, 2], H[:, 4], H[:, 5] + lam
    c = np.zeros((n, 3, 3))
    for i in range(3):
        i1, i2 = (i + 1) % 3, (i + 2) % 3
        for j in range(3):
            j1, j2 = (j + 1) % 3, (j + 2) % 3
            c[:, i, j] = m[:, i1, j1] * m[:, i2, j2] - m[:, i1, j2] * m[:, i2, j1]
    det = (c[:, 0, 0] * m[:, 0, 0] + c[:, 1, 0] * m[:, 1, 0]) + c[:, 2, 0] * m[:, 2, 0]
    invdet = 1.0 / det
    return np.transpose(c, (0, 2, 1)) * invdet[:, None, None]


def point_update(X, xl):
    """VertexSBAPointXYZ::oplusImpl."""
    return X + xl


def _llt_solve_fast(A, b):
    """llt_solve with the inner k loops as one sequential pass per column (the same operations in the same order)."""
    n = len(b)
    L = np.zeros((n, n))
    dg = np.zeros(n)
    with np.errstate(all="ignore"):
        for j in range(n):
            s = A[j:, j].copy()
            for k in range(j):
                s = s - L[j:, k] * L[j, k]
            if not s[0] > 0.0:
                return False, np.zeros(n)
            sd = np.sqrt(s[0])
            dg[j] = sd
            L[j + 1:, j] = s[1:] / sd
        y = np.array(b, np.float64)
        for k in range(n):
            y[k] = y[k] / dg[k]
            y[k + 1:] = y[k + 1:] - L[k + 1:, k] * y[k]
        x = y
        for k in range(n - 1, -1, -1):
            x[k] = x[k] / dg[k]
            x[:k] = x[:k] - L[k, :k] * x[k]
    return True, x


# ---- edges -----------------------------------------------------------------------------------------------------------
def edge_errors(Rp, tp, X, ed):
    """e [n][3] (third component 0 for mono edges) and camera points P [n][3] of the valid edges `ed`."""
    R, t, Xe = Rp[ed["pose"]], tp[ed["pose"]], X[ed["point"]]
    fx, fy, cx, cy, bf = ed["K"]
    with np.errstate(all="ignore"):
        P = np.stack([((R[:, r, 0] * Xe[:, 0] + R[:, r, 1] * Xe[:, 1]) + R[:, r, 2] * Xe[:, 2]) + t[:, r] for r in range(3)], 1)
        iz = 1.0 / P[:, 2]
        u = (fx * P[:, 0]) * iz + cx
        e = np.zeros((len(Xe), 3))
        e[:, 0] = ed["obs"][:, 0] - u
        e[:, 1] = ed["obs"][:, 1] - ((fy * P[:, 1]) * iz + cy)
        e[:, 2] = np.where(ed["stereo"], ed["obs"][:, 2] - (u - bf * iz), 0.0)
    return e, P


def point_jacobian(P, R, stereo, K):
    """d e / d Xw = -(d proj / d Pc) R: [n][3][3] (EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ::linearizeOplus, Xi)."""
    fx, fy, cx, cy, bf = K
    with np.errstate(all="ignore"):
        x, y, z = P[:, 0], P[:, 1], P[:, 2]
        iz = 1.0 / z
        iz2 = iz * iz
        J = np.zeros((len(P), 3, 3))
        for c in range(3):
            J[:, 0, c] = -(fx * R[:, 0, c]) * iz + ((fx * x) * R[:, 2, c]) * iz2
            J[:, 1, c] = -(fy * R[:, 1, c]) * iz + ((fy * y) * R[:, 2, c]) * iz2
            J[:, 2, c] = np.where(stereo, J[:, 0, c] - (bf * R[:, 2, c]) * iz2, 0.0)
    return J


def seg_sum(values, seg, nseg, order):
    """out[s] = sequential (left to right from 0) sum of values[i] over the i of `order` with seg[i] == s."""
    out = np.zeros((nseg,) + values.shape[1:])
    if len(order) == 0:
        return out
    o = order[np.argsort(seg[order], kind="stable")]
    s = seg[o]
    start = np.searchsorted(s, np.arange(nseg), "left")
    count = np.searchsorted(s, np.arange(nseg), "right") - start
    with np.errstate(all="ignore"):
        for r in range(int(count.max())):
            live = np.flatnonzero(count > r)
            out[live] = out[live] + values[o[start[live] + r]]
    return out


def seq_total(values):
    with np.errstate(all="ignore"):
        return float(np.cumsum(values)[-1]) if len(values) else 0.0


# ---- the optimisation ------------------------------------------------------------------------------------------------
def local_ba(pr, order=None, stop_before=False, stop_between=False):
    """The definition.  pr: dict with Tcw [P][4][4] float32 (the first n_local rows are lLocalKeyFrames, the rest
    lFixedCameras), n_local, fixed [n_local] (mnId == 0), cam [P][5] float32 (fx, fy, cx, cy, mbf), inv_sigma2 [P][nlevels]
    float32, world_pos [M][3] float32, e_point / e_pose / e_oct [E] ints, e_xy [E][2] float32, e_ur [E] float32.

    Returns a dict: Tcw_d [n_local][4][4], Tcw (float32), pos_d [M][3], pos (float32), erase (uint8 [E], 255 = not an edge:
    untouched), n_edges, n_erased, iterations [2], trials [2], chi2_start [2], chi2_end [2], rounds, stopped, n_bad_index,
    trace (the accept / reject decisions), margin (least |chi2 / threshold - 1| over all classifications)."""
    Tcw = np.asarray(pr["Tcw"], np.float32).reshape(-1, 4, 4)
    Pn, nl = len(Tcw), int(pr["n_local"])
    fixed = np.asarray(pr["fixed"], np.uint8).astype(bool)
    cam = np.asarray(pr["cam"], np.float32).reshape(Pn, 5).astype(np.float64)
    inv_sigma2 = np.asarray(pr["inv_sigma2"], np.float32).reshape(Pn, -1)
    nlevels = inv_sigma2.shape[1]
    X = np.asarray(pr["world_pos"], np.float32).reshape(-1, 3).astype(np.float64)
    Mn = len(X)
    e_point, e_pose, e_oct = (np.asarray(pr[k], np.int64) for k in ("e_point", "e_pose", "e_oct"))
    e_xy, e_ur = np.asarray(pr["e_xy"], np.float32).reshape(-1, 2), np.asarray(pr["e_ur"], np.float32)
    En = len(e_point)
    bad_index = (e_point < 0) | (e_point >= Mn) | (e_pose < 0) | (e_pose >= Pn) | (e_oct < 0) | (e_oct >= nlevels)
    valid = np.flatnonzero(~bad_index)
    ne = len(valid)
    free_of = np.full(Pn, -1, np.int64)  # pose row -> slot in the reduced system
    free_rows = np.flatnonzero(~fixed[:nl]) if nl else np.zeros(0, np.int64)
    free_of[free_rows] = np.arange(len(free_rows))
    nf = len(free_rows)

    ed = {"point": e_point[valid], "pose": e_pose[valid]}
    ed["stereo"] = ~(e_ur[valid] < 0)
    ed["obs"] = np.concatenate([e_xy[valid].astype(np.float64), e_ur[valid].astype(np.float64)[:, None]], 1)
    ed["w"] = inv_sigma2[ed["pose"], e_oct[valid]].astype(np.float64)
    ed["K"] = tuple(cam[ed["pose"], k] for k in range(5))
    ed["free"] = free_of[ed["pose"]]
    delta = np.where(ed["stereo"], DELTA_STEREO, DELTA_MONO)
    thr = np.where(ed["stereo"], CHI2_STEREO, CHI2_MONO)
    order = np.arange(ne) if order is None else np.asarray(order)

    out = dict(n_edges=ne, n_bad_index=int(bad_index.sum()), n_erased=0, iterations=[0, 0], trials=[0, 0],
               chi2_start=[0.0, 0.0], chi2_end=[0.0, 0.0], rounds=0, stopped=0, margin=np.inf, trace=[])
    erase = np.full(En, 255, np.uint8)
    out["erase"] = erase
    if stop_before:
        out["stopped"] = 1
        return out

    qs, ts = [], []
    for i in range(Pn):
        q, t = pose_from_Tcw(Tcw[i])
        qs.append(q)
        ts.append(t)
    qs, ts = np.array(qs).reshape(Pn, 4), np.array(ts).reshape(Pn, 3)

    def rotations(q_):
        return np.array([quat_to_matrix(q) for q in q_]).reshape(Pn, 3, 3)

    # the pairs of edges that share a point and both end at free poses, the first's pose slot not below the second's:
    # the terms of the Schur complement's lower block triangle, in `order`
    rank = np.empty(ne, np.int64)
    rank[order] = np.arange(ne)
    fe = order[ed["free"][order] >= 0]
    by_point = fe[np.argsort(ed["point"][fe], kind="stable")]
    p1, p2 = [], []
    pts = ed["point"][by_point]
    bounds = np.flatnonzero(np.r_[True, pts[1:] != pts[:-1], True]) if len(pts) else np.zeros(1, np.int64)
    for a, b in zip(bounds[:-1], bounds[1:]):
        g = by_point[a:b]
        i1, i2 = np.meshgrid(g, g, indexing="ij")
        p1.append(i1.ravel())
        p2.append(i2.ravel())
    p1 = np.concatenate(p1) if p1 else np.zeros(0, np.int64)
    p2 = np.concatenate(p2) if p2 else np.zeros(0, np.int64)
    keep = ed["free"][p1] >= ed["free"][p2]
    p1, p2 = p1[keep], p2[keep]
    f1, f2 = ed["free"][p1], ed["free"][p2]
    pair_blk = f1 * (f1 + 1) // 2 + f2
    nblk = nf * (nf + 1) // 2

    level1 = np.zeros(ne, bool)
    use_kernel = np.ones(ne, bool)

    def classify(q_, t_, X_):
        e_, P_ = edge_errors(rotations(q_), t_, X_, ed)
        c_ = chi2_of(e_, ed["w"])
        with np.errstate(all="ignore"):
            bad = (c_ > thr) | ~(P_[:, 2] > 0.0)
            mg = np.abs(c_ / thr - 1.0)
        if np.isfinite(mg).any():
            out["margin"] = min(out["margin"], float(np.nanmin(mg)))
        return bad

    for rnd, n_it in enumerate((5, 10)):
        if rnd == 1 and stop_between:
            out["stopped"] = 1
            break
        act = order[~level1[order]]
        on = ~level1
        pt_on = np.zeros(Mn, bool)
        pt_on[ed["point"][act]] = True
        fr_on = np.zeros(nf, bool)
        fr_on[ed["free"][act][ed["free"][act] >= 0]] = True
        act_free = act[ed["free"][act] >= 0]
        pair_on = on[p1] & on[p2]
        pair_order = np.flatnonzero(pair_on)

        def robust_chi(q_, t_, X_):
            e_, _ = edge_errors(rotations(q_), t_, X_, ed)
            r0, _ = huber(chi2_of(e_, ed["w"]), delta, use_kernel)
            return seq_total(r0[act])

        lam, nu = 0.0, 2.0
        cur = robust_chi(qs, ts, X)
        out["chi2_start"][rnd] = cur
        for it in range(n_it):
            Rp = rotations(qs)
            e, Pc = edge_errors(Rp, ts, X, ed)
            r0, r1 = huber(chi2_of(e, ed["w"]), delta, use_kernel)
            cur = seq_total(r0[act])
            Jc = jacobian(Pc, ed["stereo"], ed["K"])
            Jp = point_jacobian(Pc, Rp[ed["pose"]], ed["stereo"], ed["K"])
            with np.errstate(all="ignore"):
                s = ed["w"] * r1
                Jcw, Jpw = Jc * s[:, None, None], Jp * s[:, None, None]
                cc = np.zeros((ne, 27))
                for k, (a, b_) in enumerate(TRI6):
                    cc[:, k] = (Jcw[:, 0, a] * Jc[:, 0, b_] + Jcw[:, 1, a] * Jc[:, 1, b_]) + Jcw[:, 2, a] * Jc[:, 2, b_]
                for a in range(6):
                    cc[:, 21 + a] = -((Jcw[:, 0, a] * e[:, 0] + Jcw[:, 1, a] * e[:, 1]) + Jcw[:, 2, a] * e[:, 2])
                cp = np.zeros((ne, 9))
                for k, (a, b_) in enumerate(TRI3):
                    cp[:, k] = (Jpw[:, 0, a] * Jp[:, 0, b_] + Jpw[:, 1, a] * Jp[:, 1, b_]) + Jpw[:, 2, a] * Jp[:, 2, b_]
                for a in range(3):
                    cp[:, 6 + a] = -((Jpw[:, 0, a] * e[:, 0] + Jpw[:, 1, a] * e[:, 1]) + Jpw[:, 2, a] * e[:, 2])
                Hpl = np.zeros((ne, 6, 3))  # J_pose' (rho1 W) J_point
                for a in range(6):
                    for c in range(3):
                        Hpl[:, a, c] = (Jcw[:, 0, a] * Jp[:, 0, c] + Jcw[:, 1, a] * Jp[:, 1, c]) + Jcw[:, 2, a] * Jp[:, 2, c]
            tot_p = seg_sum(cc, ed["free"], nf, act_free)
            tot_l = seg_sum(cp, ed["point"], Mn, act)
            Hpp, bp = tot_p[:, :21], tot_p[:, 21:]
            Hll, bl = tot_l[:, :6], tot_l[:, 6:]
            if it == 0:
                m = 0.0
                for f in np.flatnonzero(fr_on):
                    for k in (0, 6, 11, 15, 18, 20):
                        m = abs(Hpp[f, k]) if abs(Hpp[f, k]) > m else m
                for p in np.flatnonzero(pt_on):
                    for k in (0, 3, 5):
                        m = abs(Hll[p, k]) if abs(Hll[p, k]) > m else m
                lam, nu = 1e-5 * m, 2.0
            rho, trial, stop = 0.0, 0, False
            out["iterations"][rnd] += 1
            while True:
                with np.errstate(all="ignore"):
                    inv = np.zeros((Mn, 3, 3))
                    inv[pt_on] = _inv3_all(Hll[pt_on], lam)
                    ie = inv[ed["point"]]
                    Y = np.zeros((ne, 6, 3))  # Hpl Hll^-1
                    for a in range(6):
                        for c in range(3):
                            Y[:, a, c] = (Hpl[:, a, 0] * ie[:, 0, c] + Hpl[:, a, 1] * ie[:, 1, c]) + Hpl[:, a, 2] * ie[:, 2, c]
                    # reduced system
                    T = np.zeros((len(p1), 36))
                    for a in range(6):
                        for c in range(6):
                            T[:, 6 * a + c] = (Y[p1, a, 0] * Hpl[p2, c, 0] + Y[p1, a, 1] * Hpl[p2, c, 1]) + Y[p1, a, 2] * Hpl[p2, c, 2]
                    Tb = seg_sum(T, pair_blk, nblk, pair_order)
                    S = np.zeros((6 * nf, 6 * nf))
                    for fa in range(nf):
                        for fb in range(fa + 1):
                            blk = 0.0 - Tb[fa * (fa + 1) // 2 + fb].reshape(6, 6)
                            if fa == fb:
                                if fr_on[fa]:
                                    A = np.zeros((6, 6))
                                    for k, (a, b_) in enumerate(TRI6):
                                        A[a, b_] = A[b_, a] = Hpp[fa, k]
                                    for a in range(6):
                                        A[a, a] = A[a, a] + lam
                                    blk = A - Tb[fa * (fa + 1) // 2 + fb].reshape(6, 6)
                                else:
                                    blk = np.eye(6)  # a free pose without an active edge: x = 0, coupled to nothing
                            S[6 * fa:6 * fa + 6, 6 * fb:6 * fb + 6] = blk
                    gy = np.zeros((ne, 6))
                    ble = bl[ed["point"]]
                    for a in range(6):
                        gy[:, a] = (Y[:, a, 0] * ble[:, 0] + Y[:, a, 1] * ble[:, 1]) + Y[:, a, 2] * ble[:, 2]
                    g = bp - seg_sum(gy, ed["free"], nf, act_free)
                    g[~fr_on] = 0.0
                    ok, xp = _llt_solve_fast(S, g.ravel())
                    xp = xp.reshape(nf, 6)
                    # back substitution to the points
                    xe = xp[ed["free"].clip(0)] if nf else np.zeros((ne, 6))
                    ht = np.zeros((ne, 3))
                    for c in range(3):
                        v = Hpl[:, 0, c] * xe[:, 0]
                        for a in range(1, 6):
                            v = v + Hpl[:, a, c] * xe[:, a]
                        ht[:, c] = v
                    r = bl - seg_sum(ht, ed["point"], Mn, act_free)
                    xl = np.zeros((Mn, 3))
                    for c in range(3):
                        xl[:, c] = (inv[:, c, 0] * r[:, 0] + inv[:, c, 1] * r[:, 1]) + inv[:, c, 2] * r[:, 2]
                    xl[~pt_on] = 0.0
                    if not ok:
                        xl[:] = 0.0
                qn, tn = qs.copy(), ts.copy()
                for f in np.flatnonzero(fr_on):
                    qn[free_rows[f]], tn[free_rows[f]] = pose_update(qs[free_rows[f]], ts[free_rows[f]], xp[f])
                Xn = X.copy()
                Xn[pt_on] = point_update(X[pt_on], xl[pt_on])
                tmp = robust_chi(qn, tn, Xn)
                if not ok:
                    tmp = DBL_MAX
                with np.errstate(all="ignore"):
                    terms = np.r_[(xp * (lam * xp + bp))[fr_on].ravel(), (xl * (lam * xl + bl))[pt_on].ravel()]
                    scale = seq_total(terms) + 1e-3
                    rho = (cur - tmp) / scale
                out["trials"][rnd] += 1
                if rho > 0 and np.isfinite(tmp):
                    with np.errstate(all="ignore"):
                        c3 = 2.0 * rho - 1.0
                        alpha = min(1.0 - (c3 * c3) * c3, 2.0 / 3.0)
                        lam = lam * max(1.0 / 3.0, alpha)
                    nu = 2.0
                    qs, ts, X, cur = qn, tn, Xn, tmp
                    out["trace"].append(1)
                else:
                    with np.errstate(all="ignore"):
                        lam = lam * nu
                        nu = nu * 2.0
                    if not np.isfinite(lam):
                        stop = True
                    out["trace"].append(0)
                trial += 1
                if stop or not (rho < 0 and trial < 10):
                    break
            if trial == 10 or rho == 0 or stop:
                break
        out["chi2_end"][rnd] = cur
        out["rounds"] = rnd + 1
        if rnd == 0 and not stop_between:
            level1 = classify(qs, ts, X)
            use_kernel[:] = False
    bad = classify(qs, ts, X)
    erase[valid] = bad.astype(np.uint8)
    out["n_erased"] = int(bad.sum())
    out["Tcw_d"] = np.array([pose_matrix(qs[i], ts[i]) for i in range(nl)]).reshape(nl, 4, 4)
    out["Tcw"] = out["Tcw_d"].astype(np.float32)
    out["pos_d"] = X
    with np.errstate(all="ignore"):
        out["pos"] = X.astype(np.float32)
    return out


# ---- the graph gathering (Optimizer.cc:455-504, :522-652) -------------------------------------------------------------
def gather(mp):
    """The problem of a map as OptimizerT::LocalBundleAdjustment builds it.  mp: dict with cur (index of the key frame that
    was just inserted), kfs: list of dicts (id, bad, cov: indices of GetVectorCovisibleKeyFrames() in order, K (5), Tcw,
    inv_sigma2, kps [n][4] = x, y, u_right, octave, mps [n]: index of the key point's map point or -1), mps: list of dicts
    (id, bad, pos, obs {key-frame index: key-point index}).  The reference walks std::map<KeyFrame *, size_t>, that is, the
    observations in pointer order: here the index order.  Returns the problem dict of local_ba plus local, fixed, points
    (indices in list order) and edge_kf / edge_mp."""
    kfs, mps, cur = mp["kfs"], mp["mps"], mp["cur"]
    local, mark_local = [cur], {cur}
    for k in kfs[cur]["cov"]:
        mark_local.add(k)
        if not kfs[k]["bad"]:
            local.append(k)
    points, seen = [], set()
    for k in local:
        for m in kfs[k]["mps"]:
            if m >= 0 and not mps[m]["bad"] and m not in seen:
                points.append(int(m))
                seen.add(m)
    fixed, mark_fixed = [], set()
    for m in points:
        for k in sorted(mps[m]["obs"]):
            if k not in mark_local and k not in mark_fixed:
                mark_fixed.add(k)
                if not kfs[k]["bad"]:
                    fixed.append(k)
    rows = {k: i for i, k in enumerate(local + fixed)}
    nlevels = max(1, min(len(kfs[cur]["inv_sigma2"]), 8))
    sig = np.zeros((len(rows), nlevels), np.float32)
    for k, i in rows.items():
        s = np.asarray(kfs[k]["inv_sigma2"], np.float32)[:nlevels]
        sig[i, :len(s)] = s
    e = {k: [] for k in ("point", "pose", "oct", "xy", "ur", "kf", "mp")}
    for j, m in enumerate(points):
        for k in sorted(mps[m]["obs"]):
            if kfs[k]["bad"]:
                continue
            x, y, ur, octave = kfs[k]["kps"][mps[m]["obs"][k]]
            e["point"].append(j), e["pose"].append(rows.get(k, -1)), e["kf"].append(k), e["mp"].append(m)
            e["oct"].append(int(octave) if 0 <= int(octave) < len(kfs[k]["inv_sigma2"]) else -1)
            e["xy"].append((x, y)), e["ur"].append(ur)
    order = local + fixed
    return dict(Tcw=np.array([kfs[k]["Tcw"] for k in order], np.float32).reshape(-1, 4, 4), n_local=len(local),
                fixed=np.array([kfs[k]["id"] == 0 for k in local], np.uint8),
                cam=np.array([kfs[k]["K"] for k in order], np.float32).reshape(-1, 5), inv_sigma2=sig,
                world_pos=np.array([mps[m]["pos"] for m in points], np.float32).reshape(-1, 3),
                e_point=np.array(e["point"], np.int32), e_pose=np.array(e["pose"], np.int32), e_oct=np.array(e["oct"], np.int32),
                e_xy=np.array(e["xy"], np.float32).reshape(-1, 2), e_ur=np.array(e["ur"], np.float32),
                local=local, fixed_list=fixed, points=points, edge_kf=e["kf"], edge_mp=e["mp"])


# ---- scenes ----------------------------------------------------------------------------------------------------------
def make_scene(n_free, n_fixed, n_points, seed, mode="mixed", kf0_fixed=False, noise=0.5, outlier_frac=0.05, obs_frac=0.7,
               rot_sigma=0.004, trans_sigma=0.01, point_sigma=0.02, outlier_px=(30.0, 60.0)):
    """A seeded local map in the form the entry points take it: n_free local key frames (plus one more, fixed, when
    kf0_fixed: the mnId == 0 case) and n_fixed fixed cameras looking at n_points points 2-7 m ahead; every camera sees about
    obs_frac of the points, every point is seen at least twice; pixel noise scaled by the level's sigma; planted gross
    outliers displaced by outlier_px[0] .. outlier_px[1] sigma; mode "mono" / "stereo" / "mixed" (70 % stereo).  Local
    poses and points start perturbed; fixed ones at truth.  Returns the problem dict plus `bad` [E] and the truth."""
    rng = np.random.default_rng(seed)
    nl = n_free + (1 if kf0_fixed else 0)
    Pn = nl + n_fixed
    fx, fy, cx, cy, bf = [float(k) for k in CAMERA]
    Xw = np.stack([rng.uniform(-2.5, 2.5, n_points), rng.uniform(-1.8, 1.8, n_points), rng.uniform(3.0, 7.0, n_points)], 1)
    Xw = Xw.astype(np.float32).astype(np.float64)
    Tt = np.zeros((Pn, 4, 4))
    for i in range(Pn):
        R, _ = se3_exp(np.r_[rng.normal(0, 0.04, 3), 0, 0, 0])
        Tt[i] = np.eye(4)
        Tt[i, :3, :3] = R
        Tt[i, :3, 3] = rng.normal(0, 0.25, 3) * np.array([1.0, 0.5, 0.6])
    Tt = Tt.astype(np.float32).astype(np.float64)
    cam = np.tile(np.asarray(CAMERA, np.float32), (Pn, 1))
    cam[:, 0] *= (1.0 + 0.01 * np.arange(Pn)).astype(np.float32)  # per key frame: every row has its own intrinsics
    inv_sigma2 = np.tile(INV_LEVEL_SIGMA2, (Pn, 1))
    sees = rng.random((n_points, Pn)) < obs_frac
    for p in range(n_points):
        while sees[p].sum() < min(2, Pn):
            sees[p, rng.integers(Pn)] = True
    e_point, e_pose = np.nonzero(sees)
    E = len(e_point)
    Pc = np.einsum("eij,ej->ei", Tt[e_pose, :3, :3], Xw[e_point]) + Tt[e_pose, :3, 3]
    c = cam.astype(np.float64)[e_pose]
    octave = rng.integers(0, NLEVELS, E).astype(np.int32)
    sig = np.float64(1.2) ** octave
    u = c[:, 0] * Pc[:, 0] / Pc[:, 2] + c[:, 2]
    v = c[:, 1] * Pc[:, 1] / Pc[:, 2] + c[:, 3]
    xy = np.stack([u, v], 1) + rng.normal(0, noise, (E, 2)) * sig[:, None]
    ur = u - c[:, 4] / Pc[:, 2] + rng.normal(0, noise, E) * sig
    stereo = {"mono": np.zeros(E, bool), "stereo": np.ones(E, bool)}.get(mode, rng.random(E) < 0.7)
    bad = rng.random(E) < outlier_frac
    nb = int(bad.sum())
    ang, mag = rng.uniform(0, 2 * np.pi, nb), rng.uniform(outlier_px[0], outlier_px[1], nb)
    xy[bad] += np.stack([mag * np.cos(ang), mag * np.sin(ang)], 1) * sig[bad, None]
    stereo = stereo & (ur >= 0)
    ur = np.where(stereo, ur, -1.0).astype(np.float32)
    T0 = Tt.copy()
    fixed = np.zeros(nl, np.uint8)
    if kf0_fixed:
        fixed[int(rng.integers(nl))] = 1
    for i in range(nl):
        if not fixed[i]:
            dR, dt = se3_exp(np.r_[rng.normal(0, rot_sigma, 3), rng.normal(0, trans_sigma, 3)])
            T0[i, :3, :3] = dR @ Tt[i, :3, :3]
            T0[i, :3, 3] = dR @ Tt[i, :3, 3] + dt
    X0 = Xw + rng.normal(0, point_sigma, Xw.shape)
    perm = rng.permutation(E)  # edges arrive grouped by neither point nor pose
    return dict(Tcw=T0.astype(np.float32), n_local=nl, fixed=fixed, cam=cam, inv_sigma2=inv_sigma2,
                world_pos=X0.astype(np.float32), e_point=e_point[perm].astype(np.int32), e_pose=e_pose[perm].astype(np.int32),
                e_oct=octave[perm], e_xy=xy[perm].astype(np.float32), e_ur=ur[perm], bad=bad[perm], Tcw_true=Tt, pos_true=Xw)


def permutation_spread(pr, base, n_perm=4, seed=0):
    """Over n_perm seeded permutations of the summation order: the largest deviation of the poses and of the points from
    `base`, whether the accept / reject trace or a discrete output changed, and the least classification margin."""
    rng = np.random.default_rng(10_000 + seed)
    dev_T, dev_X, same, margin = 0.0, 0.0, True, base["margin"]
    for _ in range(n_perm):
        r = local_ba(pr, order=rng.permutation(base["n_edges"]))
        margin = min(margin, r["margin"])
        same = same and r["trace"] == base["trace"] and np.array_equal(r["erase"], base["erase"])
        with np.errstate(all="ignore"):
            dT, dX = np.abs(r["Tcw_d"] - base["Tcw_d"]), np.abs(r["pos_d"] - base["pos_d"])
        dev_T = max(dev_T, float(np.nanmax(dT)) if dT.size else 0.0)
        dev_X = max(dev_X, float(np.nanmax(dX)) if dX.size else 0.0)
    return dev_T, dev_X, same, margin
