"""NumPy float64 restatement of Optimizer::PoseOptimization (Optimizer.cc:239-451): the oracle of the device
motion-only bundle adjustment (orbgpu_pose_optimization*).

g2o is not part of the reference tree, so its behaviour is restated here from its published algorithm
(OptimizationAlgorithmLevenberg over a dense 6x6 solver, EdgeSE3ProjectXYZOnlyPose / EdgeStereoSE3ProjectXYZOnlyPose,
RobustKernelHuber, SE3Quat): every comparison against this file is "vs CPU restatement; g2o boundary unpinned".
The definition, step by step, is in include/orbgpu.h above orbgpu_pose_optimization_device and DESIGN.md section 2.

All arithmetic is IEEE double unless a float32 is named.  Sums over edges run sequentially in `order` (default: key-point
order), so that a permutation of `order` shows what the summation order alone does to the result.
"""
import numpy as np

DELTA_MONO = np.float64(np.float32(np.sqrt(5.991)))
DELTA_STEREO = np.float64(np.float32(np.sqrt(7.815)))
CHI2_MONO = np.float32(5.991)
CHI2_STEREO = np.float32(7.815)
DBL_MAX = np.finfo(np.float64).max


# ---- SE3Quat ---------------------------------------------------------------------------------------------------------
def quat_from_matrix(m):
    """Eigen's Quaterniond(Matrix3d); returns (x, y, z, w)."""
    q = np.zeros(4)
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[2, 1] - m[1, 2]) * t
        q[1] = (m[0, 2] - m[2, 0]) * t
        q[2] = (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[k, j] - m[j, k]) * t
        q[j] = (m[j, i] + m[i, j]) * t
        q[k] = (m[k, i] + m[i, k]) * t
    return q


def quat_normalize(q):
    """SE3Quat::normalizeRotation: w >= 0, unit norm."""
    if q[3] < 0:
        q = -q
    n = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return q / n


def quat_to_matrix(q):
    x, y, z, w = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([((aw * bx + ax * bw) + ay * bz) - az * by,
                     ((aw * by + ay * bw) + az * bx) - ax * bz,
                     ((aw * bz + az * bw) + ax * by) - ay * bx,
                     ((aw * bw - ax * bx) - ay * by) - az * bz])


def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def se3_exp(u):
    """SE3Quat::exp of (omega, upsilon): rotation matrix and translation."""
    w, v = np.asarray(u[:3], np.float64), np.asarray(u[3:], np.float64)
    th = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    O = skew(w)
    O2 = np.array([[(O[r, 0] * O[0, c] + O[r, 1] * O[1, c]) + O[r, 2] * O[2, c] for c in range(3)] for r in range(3)])
    if th < 1e-5:
        R = (np.eye(3) + O) + O2
        V = R
    else:
        a = np.sin(th) / th
        b = (1.0 - np.cos(th)) / (th * th)
        c = (th - np.sin(th)) / ((th * th) * th)
        R = (np.eye(3) + a * O) + b * O2
        V = (np.eye(3) + b * O) + c * O2
    return R, mat_vec(V, v)


def mat_vec(M, v):
    return np.array([(M[r, 0] * v[0] + M[r, 1] * v[1]) + M[r, 2] * v[2] for r in range(3)])


def pose_from_Tcw(Tcw):
    """Converter::toSE3Quat: float 3x3 -> double -> unit quaternion, float t -> double."""
    T = np.asarray(Tcw, np.float32).reshape(4, 4).astype(np.float64)
    return quat_normalize(quat_from_matrix(T[:3, :3])), T[:3, 3].copy()


def pose_update(q, t, x):
    """T <- exp(x) * T (SE3Quat::operator*, normalised)."""
    dR, dt = se3_exp(x)
    dq = quat_normalize(quat_from_matrix(dR))
    return quat_normalize(quat_mul(dq, q)), mat_vec(quat_to_matrix(dq), t) + dt


def pose_matrix(q, t):
    T = np.eye(4)
    T[:3, :3] = quat_to_matrix(q)
    T[:3, 3] = t
    return T


# ---- edges -----------------------------------------------------------------------------------------------------------
def errors(q, t, Xw, obs, stereo, K):
    """e [n][3] (third component 0 for mono edges) and camera points P [n][3]."""
    fx, fy, cx, cy, bf = K
    R = quat_to_matrix(q)
    with np.errstate(all="ignore"):
        P = np.stack([((R[r, 0] * Xw[:, 0] + R[r, 1] * Xw[:, 1]) + R[r, 2] * Xw[:, 2]) + t[r] for r in range(3)], 1)
        iz = 1.0 / P[:, 2]
        u = (fx * P[:, 0]) * iz + cx
        e = np.zeros((len(Xw), 3))
        e[:, 0] = obs[:, 0] - u
        e[:, 1] = obs[:, 1] - ((fy * P[:, 1]) * iz + cy)
        e[:, 2] = np.where(stereo, obs[:, 2] - (u - bf * iz), 0.0)
    return e, P


def chi2_of(e, w):
    with np.errstate(all="ignore"):
        return w * ((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])


def jacobian(P, stereo, K):
    """d e / d (omega, upsilon) of the left update exp(omega, upsilon) * T at zero: [n][3][6]."""
    fx, fy, cx, cy, bf = K
    with np.errstate(all="ignore"):
        x, y, z = P[:, 0], P[:, 1], P[:, 2]
        iz = 1.0 / z
        iz2 = iz * iz
        J = np.zeros((len(P), 3, 6))
        J[:, 0, 0] = ((x * y) * iz2) * fx
        J[:, 0, 1] = -(1.0 + (x * x) * iz2) * fx
        J[:, 0, 2] = (y * iz) * fx
        J[:, 0, 3] = -iz * fx
        J[:, 0, 5] = (x * iz2) * fx
        J[:, 1, 0] = (1.0 + (y * y) * iz2) * fy
        J[:, 1, 1] = -((x * y) * iz2) * fy
        J[:, 1, 2] = -(x * iz) * fy
        J[:, 1, 4] = -iz * fy
        J[:, 1, 5] = (y * iz2) * fy
        J[:, 2, 0] = J[:, 0, 0] - (bf * y) * iz2
        J[:, 2, 1] = J[:, 0, 1] + (bf * x) * iz2
        J[:, 2, 2] = J[:, 0, 2]
        J[:, 2, 3] = J[:, 0, 3]
        J[:, 2, 5] = J[:, 0, 5] - bf * iz2
        J[~stereo, 2, :] = 0.0
    return J


def huber(chi2, delta, use_kernel):
    """rho0, rho1 of RobustKernelHuber (no second-order term); plain chi2 where the edge has no kernel."""
    d2 = delta * delta
    with np.errstate(all="ignore"):
        s = np.sqrt(chi2)
        small = (chi2 <= d2) | ~use_kernel
        rho0 = np.where(small, chi2, (2.0 * s) * delta - d2)
        rho1 = np.where(small, 1.0, delta / s)
    return rho0, rho1


def seq_sum(a, order):
    """Sequential (left to right) float64 sum of a[order] along axis 0."""
    if len(order) == 0:
        return np.zeros(a.shape[1:])
    return np.cumsum(a[order], axis=0)[-1]


TRI = [(a, b) for a in range(6) for b in range(a, 6)]


def cholesky_solve(H, lam, b):
    """(H + lam I) x = b by LL^T on the upper triangle of H, of any size (6 here, 7 in sim3opt_model); (ok, x).  Not
    positive definite (a pivot that is not > 0, NaN included): ok = False and x = 0."""
    n = len(H)
    A = H.copy()
    for i in range(n):
        A[i, i] = A[i, i] + lam
    L = np.zeros((n, n))
    with np.errstate(all="ignore"):
        for j in range(n):
            d = A[j, j]
            for k in range(j):
                d = d - L[j, k] * L[j, k]
            if not d > 0.0:
                return False, np.zeros(n)
            d = np.sqrt(d)
            L[j, j] = d
            for i in range(j + 1, n):
                s = A[j, i]
                for k in range(j):
                    s = s - L[i, k] * L[j, k]
                L[i, j] = s / d
        y = np.zeros(n)
        for i in range(n):
            s = b[i]
            for k in range(i):
                s = s - L[i, k] * y[k]
            y[i] = s / L[i, i]
        x = np.zeros(n)
        for i in range(n - 1, -1, -1):
            s = y[i]
            for k in range(i + 1, n):
                s = s - L[k, i] * x[k]
            x[i] = s / L[i, i]
    return True, x


# ---- the optimisation ------------------------------------------------------------------------------------------------
def pose_optimization(kps_xy, octave, u_right, kp_to_mp, world_pos, Tcw, inv_level_sigma2, K, order=None):
    """The definition.  kps_xy [n][2] float32 (mvKeysUn), octave [n], u_right [n] float32, kp_to_mp [n] (>= 0 row of
    world_pos, < 0 no edge), world_pos [rows][3] float32, Tcw 4x4 float32, inv_level_sigma2 [nlevels] float32,
    K = (fx, fy, cx, cy, mbf) float32.  order: a permutation of the EDGES (positions in key-point order) for the sums.

    Returns a dict: Tcw_d, Tcw, n_initial, n_inliers, rounds, iterations, trials, n_bad_index, outlier (uint8 [n], 255 =
    not an edge: untouched), margin (least |chi2 / threshold - 1| over all classifications)."""
    kps_xy = np.asarray(kps_xy, np.float32)
    n = len(kps_xy)
    octave = np.asarray(octave, np.int64)
    kp_to_mp = np.asarray(kp_to_mp, np.int64)
    world_pos = np.asarray(world_pos, np.float32).reshape(-1, 3)
    inv_level_sigma2 = np.asarray(inv_level_sigma2, np.float32)
    K = tuple(np.float64(np.float32(k)) for k in K)
    rows, nlevels = len(world_pos), len(inv_level_sigma2)
    has = kp_to_mp >= 0
    bad_index = has & ((kp_to_mp >= rows) | (octave < 0) | (octave >= nlevels))
    edge = np.flatnonzero(has & ~bad_index)
    ne = len(edge)
    Xw = world_pos[kp_to_mp[edge]].astype(np.float64)
    stereo = ~(np.asarray(u_right, np.float32)[edge] < 0)
    obs = np.zeros((ne, 3))
    obs[:, :2] = kps_xy[edge].astype(np.float64)
    obs[:, 2] = np.asarray(u_right, np.float32)[edge].astype(np.float64)
    w = inv_level_sigma2[octave[edge]].astype(np.float64)
    delta = np.where(stereo, DELTA_STEREO, DELTA_MONO)
    thr = np.where(stereo, CHI2_STEREO, CHI2_MONO)
    order = np.arange(ne) if order is None else np.asarray(order)

    q0, t0 = pose_from_Tcw(Tcw)
    out = dict(n_initial=ne, n_bad_index=int(bad_index.sum()), rounds=0, iterations=0, trials=0, margin=np.inf)
    outlier = np.full(n, 255, np.uint8)
    outlier[edge] = 0
    out["outlier"] = outlier
    if ne < 3:
        out["Tcw_d"] = np.asarray(Tcw, np.float32).reshape(4, 4).astype(np.float64)
        out["Tcw"] = np.asarray(Tcw, np.float32).reshape(4, 4).copy()
        out["n_inliers"] = 0
        return out

    level1 = np.zeros(ne, bool)
    use_kernel = np.ones(ne, bool)
    n_bad = 0
    q, t = q0, t0
    for rnd in range(4):
        q, t = q0.copy(), t0.copy()
        act = order[~level1[order]]

        def robust_chi(q_, t_):
            e_, _ = errors(q_, t_, Xw, obs, stereo, K)
            r0, _ = huber(chi2_of(e_, w), delta, use_kernel)
            return float(seq_sum(r0, act))

        lam, nu = 0.0, 2.0
        for it in range(10):
            e, P = errors(q, t, Xw, obs, stereo, K)
            c = chi2_of(e, w)
            r0, r1 = huber(c, delta, use_kernel)
            cur = float(seq_sum(r0, act))
            J = jacobian(P, stereo, K)
            with np.errstate(all="ignore"):
                s = w * r1
                Jw = J * s[:, None, None]
                contrib = np.zeros((ne, 27))
                for k, (a, b_) in enumerate(TRI):
                    contrib[:, k] = (Jw[:, 0, a] * J[:, 0, b_] + Jw[:, 1, a] * J[:, 1, b_]) + Jw[:, 2, a] * J[:, 2, b_]
                for a in range(6):
                    contrib[:, 21 + a] = -((Jw[:, 0, a] * e[:, 0] + Jw[:, 1, a] * e[:, 1]) + Jw[:, 2, a] * e[:, 2])
                tot = seq_sum(contrib, act)
            H = np.zeros((6, 6))
            for k, (a, b_) in enumerate(TRI):
                H[a, b_] = H[b_, a] = tot[k]
            b = tot[21:27].copy()
            if it == 0:
                m = 0.0
                for a in range(6):
                    if abs(H[a, a]) > m:
                        m = abs(H[a, a])
                lam, nu = 1e-5 * m, 2.0
            rho, trial, stop = 0.0, 0, False
            out["iterations"] += 1
            while True:
                ok, x = cholesky_solve(H, lam, b)
                qn, tn = pose_update(q, t, x)
                tmp = robust_chi(qn, tn)
                if not ok:
                    tmp = DBL_MAX
                with np.errstate(all="ignore"):
                    scale = 0.0
                    for a in range(6):
                        scale = scale + x[a] * (lam * x[a] + b[a])
                    scale = scale + 1e-3
                    rho = (cur - tmp) / scale
                out["trials"] += 1
                if rho > 0 and np.isfinite(tmp):
                    with np.errstate(all="ignore"):
                        c3 = 2.0 * rho - 1.0
                        alpha = min(1.0 - (c3 * c3) * c3, 2.0 / 3.0)
                        lam = lam * max(1.0 / 3.0, alpha)
                    nu = 2.0
                    q, t, cur = qn, tn, tmp
                else:
                    with np.errstate(all="ignore"):
                        lam = lam * nu
                        nu = nu * 2.0
                    if not np.isfinite(lam):
                        stop = True
                trial += 1
                if stop or not (rho < 0 and trial < 10):
                    break
            if trial == 10 or rho == 0 or stop:
                break
        # classification at the round's final pose (Optimizer.cc:384-437)
        e, _ = errors(q, t, Xw, obs, stereo, K)
        c = chi2_of(e, w)
        with np.errstate(all="ignore"):
            is_out = c.astype(np.float32) > thr
            mg = np.abs(c / thr.astype(np.float64) - 1.0)
        if np.isfinite(mg).any():
            out["margin"] = min(out["margin"], float(np.nanmin(mg)))
        level1 = is_out.copy()
        n_bad = int(is_out.sum())
        out["rounds"] = rnd + 1
        if rnd == 2:
            use_kernel[:] = False
        if ne < 10:
            break
    outlier[edge] = is_out.astype(np.uint8)
    out["Tcw_d"] = pose_matrix(q, t)
    out["Tcw"] = out["Tcw_d"].astype(np.float32)
    out["n_inliers"] = ne - n_bad
    return out


# ---- scenes ----------------------------------------------------------------------------------------------------------
CAMERA = (np.float32(535.4), np.float32(539.2), np.float32(320.1), np.float32(247.6), np.float32(40.0))
NLEVELS = 8
INV_LEVEL_SIGMA2 = (1.0 / (np.float32(1.2) ** np.arange(NLEVELS, dtype=np.float32)) ** 2).astype(np.float32)


def make_scene(n, seed, mode="mixed", assoc_frac=0.8, outlier_frac=0.2, noise=0.7, rot_sigma=0.01, trans_sigma=0.03,
               outlier_px=None):
    """A seeded tracking situation in the form the entry points take it.  n key points, of which about assoc_frac hold a
    map point (exactly n when assoc_frac == 1); ground-truth pose; points at 0.5-6 m; pixel noise scaled by the level's
    sigma; a share of gross outliers; mode "mono" / "stereo" / "mixed" (70 % stereo); start pose = truth perturbed by about
    rot_sigma rad / trans_sigma m.  Returns a dict (arrays as the ABI takes them, plus planted `bad` and `Tcw_true`)."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy, bf = [float(k) for k in CAMERA]
    Rg, _ = se3_exp(np.r_[rng.normal(0, 0.3, 3), 0, 0, 0])
    tg = rng.normal(0, 0.5, 3)
    uv = np.stack([rng.uniform(20, 620, n), rng.uniform(20, 460, n)], 1)
    z = rng.uniform(0.5, 6.0, n)
    Pc = np.stack([(uv[:, 0] - cx) * z / fx, (uv[:, 1] - cy) * z / fy, z], 1)
    Xw = ((Pc - tg) @ Rg).astype(np.float32)
    octave = rng.integers(0, NLEVELS, n).astype(np.int32)
    sig = np.float64(1.2) ** octave
    if mode == "mono":
        stereo = np.zeros(n, bool)
    elif mode == "stereo":
        stereo = np.ones(n, bool)
    else:
        stereo = rng.random(n) < 0.7
    xy = uv + rng.normal(0, noise, (n, 2)) * sig[:, None]
    ur = xy[:, 0] - bf / z + rng.normal(0, noise, n) * sig
    bad = rng.random(n) < outlier_frac
    nb = int(bad.sum())
    if outlier_px is None:
        xy[bad] += rng.normal(0, 25, (nb, 2))
        ur[bad] += rng.normal(0, 25, nb)
    else:  # unmistakable: every planted outlier is displaced by outlier_px[0] .. outlier_px[1] pixels
        ang, mag = rng.uniform(0, 2 * np.pi, nb), rng.uniform(outlier_px[0], outlier_px[1], nb)
        xy[bad] += np.stack([mag * np.cos(ang), mag * np.sin(ang)], 1) * sig[bad, None]
    stereo = stereo & (ur >= 0)  # a negative right coordinate reads as "mono" (Optimizer.cc:276)
    ur = np.where(stereo, ur, -1.0).astype(np.float32)
    has = np.ones(n, bool) if assoc_frac >= 1 else rng.random(n) < assoc_frac
    # map-point rows in a shuffled table with some rows nobody points at
    rows = n + 7
    perm = rng.permutation(rows)[:n]
    world_pos = rng.normal(0, 1, (rows, 3)).astype(np.float32)
    world_pos[perm] = Xw
    kp_to_mp = np.where(has, perm, -1).astype(np.int32)
    dR, dt = se3_exp(np.r_[rng.normal(0, rot_sigma, 3), rng.normal(0, trans_sigma, 3)])
    T0 = np.eye(4)
    T0[:3, :3] = dR @ Rg
    T0[:3, 3] = dR @ tg + dt
    Tt = np.eye(4)
    Tt[:3, :3] = Rg
    Tt[:3, 3] = tg
    return dict(n=n, kps_xy=xy.astype(np.float32), octave=octave, u_right=ur, kp_to_mp=kp_to_mp, world_pos=world_pos,
                Tcw=T0.astype(np.float32), Tcw_true=Tt, inv_level_sigma2=INV_LEVEL_SIGMA2.copy(), K=CAMERA,
                bad=bad & has, has=has)


def run_model(sc, order=None):
    return pose_optimization(sc["kps_xy"], sc["octave"], sc["u_right"], sc["kp_to_mp"], sc["world_pos"], sc["Tcw"],
                             sc["inv_level_sigma2"], sc["K"], order=order)


def permutation_spread(sc, base, n_perm=8, seed=0):
    """Largest entry-wise deviation of Tcw_d over n_perm seeded permutations of the edge order, and whether any discrete
    output changed."""
    rng = np.random.default_rng(10_000 + seed)
    dev, flips = 0.0, 0
    for _ in range(n_perm):
        r = run_model(sc, order=rng.permutation(base["n_initial"]))
        dev = max(dev, float(np.abs(r["Tcw_d"] - base["Tcw_d"]).max()))
        flips += int((r["outlier"] != base["outlier"]).sum())
    return dev, flips
