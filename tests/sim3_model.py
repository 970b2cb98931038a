"""Sim3Solver (Sim3Solver.cc, DUtils/Random.cpp) restated in numpy: the definition the device entry points
(orbgpu_sim3_*, include/orbgpu.h H1-H8) are compared with -- vs CPU restatement; OpenCV boundary unpinned.

float32 steps round after every operation (numpy scalars / arrays of float32), the steps from the eigen-decomposition to
the rotation matrix run in float64 on the float32 inputs and are rounded once.  Nothing here is fast."""
import math

import numpy as np

from jacobi_model import JACOBI_STOP, jacobi_sym  # noqa: F401  (the one Jacobi of the models)

f32, f64 = np.float32, np.float64
CHI2 = 9.210
JACOBI_SWEEPS = 16
NLEVELS = 8
SIGMA2 = (f32(1.2) ** np.arange(NLEVELS, dtype=f32)) ** 2
INT_MAX = 2 ** 31 - 1


# ---- H2 / H3 -----------------------------------------------------------------------------------------------------------
def rt_apply(T, X):
    """cv::Mat 3x3 * 3x1 + 3x1, small-matrix path: float products summed left to right, then one add.  X [n][3]."""
    T = np.asarray(T, f32)
    X = np.asarray(X, f32).reshape(-1, 3)
    out = np.empty_like(X)
    with np.errstate(all="ignore"):
        for i in range(3):
            s = T[i, 0] * X[:, 0]
            s = s + T[i, 1] * X[:, 1]
            s = s + T[i, 2] * X[:, 2]
            out[:, i] = s + T[i, 3]
    return out


def to_image(K, Xc):
    """FromCameraToImage / Project: invz = 1/z; fx*(x*invz)+cx.  K = (fx, fy, cx, cy)."""
    fx, fy, cx, cy = (f32(k) for k in K)
    with np.errstate(all="ignore"):
        invz = f32(1.0) / Xc[:, 2]
        x, y = Xc[:, 0] * invz, Xc[:, 1] * invz
        return np.stack([fx * x + cx, fy * y + cy], 1).astype(f32)


def max_errors(level_sigma2):
    """mvnMaxError is a vector<size_t>: 9.210 * sigma2 in double, truncated; not >= 0 gives 0."""
    with np.errstate(all="ignore"):
        e = CHI2 * np.asarray(level_sigma2, f32).astype(f64)
        return np.where(e >= 0, np.trunc(e), 0.0).astype(f32)


def prepare(pr):
    """H1-H3.  pr: the problem dict of make_scene.  Returns the compacted lists."""
    n1 = len(pr["valid"])
    nl = len(pr["level_sigma2"])
    o1, o2 = np.asarray(pr["octave1"], np.int64), np.asarray(pr["octave2"], np.int64)
    valid = np.asarray(pr["valid"]) != 0
    in_range = (o1 >= 0) & (o1 < nl) & (o2 >= 0) & (o2 < nl)
    keep = valid & in_range
    idx = np.flatnonzero(keep)
    me = max_errors(pr["level_sigma2"])
    X1 = rt_apply(pr["T1w"], np.asarray(pr["Xw1"], f32).reshape(n1, 3)[idx])
    X2 = rt_apply(pr["T2w"], np.asarray(pr["Xw2"], f32).reshape(n1, 3)[idx])
    return {"n1": n1, "N": len(idx), "indices1": idx.astype(np.int32), "n_bad_index": int((valid & ~in_range).sum()),
            "X1": X1, "X2": X2, "p1": to_image(pr["K1"], X1), "p2": to_image(pr["K2"], X2),
            "max1": me[o1[idx]], "max2": me[o2[idx]]}


# ---- H4 / H5 / H8 ------------------------------------------------------------------------------------------------------
def _log(x):
    return math.nan if (x != x or x < 0) else (-math.inf if x == 0 else math.log(x))


def iteration_cap(probability, eps):
    """ceil(log(1 - p) / log(1 - eps^3)) as an int, for both solvers (pnp_model.py); eps: a float32's value."""
    with np.errstate(all="ignore"):  # libm's log and pow as the C++ side calls them; the division and ceil in IEEE
        try:
            pw = math.pow(float(eps), 3.0)
        except OverflowError:  # C's pow returns inf
            pw = math.inf
        v = np.ceil(f64(_log(1.0 - probability)) / f64(_log(1.0 - pw)))
    return int(v) if np.isfinite(v) and -2 ** 31 <= v <= INT_MAX else INT_MAX  # NaN, +-inf: larger than max_iterations


def ransac_iterations(n, probability, min_inliers, max_iterations):
    if n == 0:
        return 1
    nit = 1 if min_inliers == n else iteration_cap(probability, f32(min_inliers) / f32(n))
    return max(1, min(nit, max_iterations))


def reference_random_int(rand, rand_max=2147483647):
    """DUtils::Random::RandomInt over a caller's rand(): int(((double)rand()/((double)RAND_MAX+1.0))*d)+min."""
    def f(lo, hi):
        d = hi - lo + 1
        return int((float(rand()) / (float(rand_max) + 1.0)) * d) + lo
    return f


def sample_triples(n, iterations, random_int):
    """The draw of Sim3Solver::iterate (:163-177) replayed: it overwrites vAvailableIndices[idx], not [randi], so a point
    can be drawn twice, and after the pop it may write at position size() or size()+1 -- into a vector that keeps
    capacity n.  random_int(lo, hi) is called three times per iteration.  n < 3 and a random_int outside [lo, hi] are
    refused, as orbgpu_shim::Sim3SampleTriples refuses them."""
    if n < 3:  # the reference would call RandomInt(0, -1) and read an empty vector
        raise ValueError("fewer than 3 correspondences to draw from")
    out = np.zeros((iterations, 3), np.int32)
    for it in range(iterations):
        avail = list(range(n))
        size = n
        for i in range(3):
            randi = random_int(0, size - 1)
            if not 0 <= randi < size:
                raise ValueError("RandomInt outside [min, max]")
            idx = avail[randi]
            out[it, i] = idx
            avail[idx] = avail[size - 1]
            size -= 1
    return out


class RansacState:
    """mnIterations / mnBestInliers between calls of iterate, over per-hypothesis counts."""

    def __init__(self, n, min_inliers, max_its):
        self.n, self.min_inliers, self.max_its = n, min_inliers, max_its
        self.iterations, self.best, self.best_iteration = 0, 0, -1

    def iterate(self, n_iterations, counts):
        """Returns (accepted iteration or -1, n_inliers, no_more)."""
        if self.n < self.min_inliers:
            return -1, 0, True
        cur = 0
        while self.iterations < self.max_its and cur < n_iterations:
            if self.iterations >= len(counts):
                return -1, 0, False  # out of hypotheses before max_its: not the reference's business
            cur += 1
            it = self.iterations
            self.iterations += 1
            if counts[it] >= self.best:
                self.best, self.best_iteration = int(counts[it]), it
                if counts[it] > self.min_inliers:
                    return it, int(counts[it]), False
        return -1, 0, self.iterations >= self.max_its


# ---- H6 ----------------------------------------------------------------------------------------------------------------
def jacobi4(N):
    """Cyclic Jacobi on the symmetric 4x4 (float64).  Returns (eigenvalues = diagonal, V with eigenvectors in columns)."""
    A = [[float(x) for x in row] for row in np.array(N, f64)]
    V = jacobi_sym(A, JACOBI_SWEEPS)
    return np.array([A[i][i] for i in range(4)], f64), np.array(V, f64)


def top_eigenvector(N, eig="jacobi"):
    """(q, relative gap of the two largest eigenvalues).  eig = "eigh": numpy.linalg.eigh in place of the Jacobi."""
    if eig == "eigh":
        if not np.all(np.isfinite(N)):
            return np.full(4, np.nan), 0.0
        w, V = np.linalg.eigh(np.array(N, f64))
        k = 3
    else:
        w, V = jacobi4(N)
        k = 0
        for j in range(1, 4):
            if w[j] > w[k]:
                k = j
    ws = np.sort(w)
    with np.errstate(all="ignore"):
        gap = (ws[3] - ws[2]) / max(abs(ws[3]), abs(ws[0]), 1e-300) if np.all(np.isfinite(ws)) else 0.0
    return V[:, k].copy(), float(gap)


def rotation_from_quaternion(q):
    """ang = atan2(|v|, q0); vec = 2 ang v / |v|; Rodrigues -- float64, NaN when |v| = 0."""
    with np.errstate(all="ignore"):
        q = np.asarray(q, f64)
        nv = np.sqrt((q[1] * q[1] + q[2] * q[2]) + q[3] * q[3])
        ang = np.arctan2(nv, q[0])
        vec = ((2.0 * ang) * q[1:4]) / nv
        theta = np.sqrt((vec[0] * vec[0] + vec[1] * vec[1]) + vec[2] * vec[2])
        cs, sn = np.cos(theta), np.sin(theta)
        c1 = 1.0 - cs
        r = vec / theta
        K = np.array([[0.0, -r[2], r[1]], [r[2], 0.0, -r[0]], [-r[1], r[0], 0.0]])
        R = np.empty((3, 3))
        for i in range(3):
            for j in range(3):
                R[i, j] = (cs * (1.0 if i == j else 0.0) + c1 * (r[i] * r[j])) + sn * K[i, j]
    return R


def horn(P1, P2, fix_scale, eig="jacobi", flip=False):
    """ComputeSim3.  P1, P2 [3 points][3] float32 in camera 1 / camera 2.  flip: use -q (for the sign test)."""
    P1, P2 = np.asarray(P1, f32), np.asarray(P2, f32)
    with np.errstate(all="ignore"):
        O1 = ((P1[0] + P1[1]) + P1[2]) / f32(3.0)
        O2 = ((P2[0] + P2[1]) + P2[2]) / f32(3.0)
        Pr1, Pr2 = P1 - O1, P2 - O2                      # [k][a]
        d1, d2 = Pr1.astype(f64), Pr2.astype(f64)
        M = np.empty((3, 3), f32)
        for i in range(3):
            for j in range(3):
                M[i, j] = f32((d2[0, i] * d1[0, j] + d2[1, i] * d1[1, j]) + d2[2, i] * d1[2, j])
        m = M.astype(f64)
        N11, N12, N13, N14 = (m[0, 0] + m[1, 1]) + m[2, 2], m[1, 2] - m[2, 1], m[2, 0] - m[0, 2], m[0, 1] - m[1, 0]
        N22, N23, N24 = (m[0, 0] - m[1, 1]) - m[2, 2], m[0, 1] + m[1, 0], m[2, 0] + m[0, 2]
        N33, N34, N44 = (-m[0, 0] + m[1, 1]) - m[2, 2], m[1, 2] + m[2, 1], (-m[0, 0] - m[1, 1]) + m[2, 2]
        N = np.array([[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]], f64).astype(f32)
        q, gap = top_eigenvector(N.astype(f64), eig)
        if flip:
            q = -q
        Rd = rotation_from_quaternion(q)
        R = Rd.astype(f32)
        s = f32(1.0)
        if not fix_scale:
            P3 = np.empty((3, 3), f32)                   # [k][i]
            for k in range(3):
                for i in range(3):
                    P3[k, i] = (R[i, 0] * Pr2[k, 0] + R[i, 1] * Pr2[k, 1]) + R[i, 2] * Pr2[k, 2]
            nom = den = f64(0.0)
            for i in range(3):
                for k in range(3):
                    nom = nom + f64(Pr1[k, i]) * f64(P3[k, i])
                    den = den + f64(P3[k, i] * P3[k, i])
            s = f32(nom / den)
        inv_s = f32(1.0) / s
        t = np.empty(3, f32)
        for i in range(3):
            u = (R[i, 0] * O2[0] + R[i, 1] * O2[1]) + R[i, 2] * O2[2]
            t[i] = O1[i] - s * u
        T12, T21 = np.eye(4, dtype=f32), np.eye(4, dtype=f32)
        T12[:3, :3] = s * R
        T12[:3, 3] = t
        T21[:3, :3] = inv_s * R.T
        for i in range(3):
            T21[i, 3] = -((T21[i, 0] * t[0] + T21[i, 1] * t[1]) + T21[i, 2] * t[2])
    return {"R": R, "R_d": Rd, "t": t, "s": s, "T12": T12, "T21": T21, "gap": gap, "q": q}


# ---- H7 ----------------------------------------------------------------------------------------------------------------
def check_inliers(prep, hyp, K1, K2):
    """Returns (inlier [N] bool, least |err / maxError - 1| over both images)."""
    with np.errstate(all="ignore"):
        d1 = (prep["p1"] - to_image(K1, rt_apply(hyp["T12"], prep["X2"]))).astype(f64)
        d2 = (to_image(K2, rt_apply(hyp["T21"], prep["X1"])) - prep["p2"]).astype(f64)
        e1 = (d1[:, 0] * d1[:, 0] + d1[:, 1] * d1[:, 1]).astype(f32)
        e2 = (d2[:, 0] * d2[:, 0] + d2[:, 1] * d2[:, 1]).astype(f32)
        inl = (e1 < prep["max1"]) & (e2 < prep["max2"])
        r = np.concatenate([np.abs(e1.astype(f64) / prep["max1"] - 1.0), np.abs(e2.astype(f64) / prep["max2"] - 1.0)])
        r = r[np.isfinite(r)]
    return inl, (float(r.min()) if len(r) else math.inf)


def mask_words(inl, indices1, n1):
    bits = np.zeros(((n1 + 63) // 64) * 64, np.uint8)
    bits[indices1[inl]] = 1
    return np.packbits(bits.reshape(-1, 8), axis=1, bitorder="little").reshape(-1).view(np.uint64).copy() if n1 else np.zeros(0, np.uint64)


def solve(pr, eig="jacobi", start_iteration=0, best_so_far=0):
    """The whole solver over pr["triples"].  Per-hypothesis lists cover the first n_use = min(H, max_its) triples."""
    prep = prepare(pr)
    N, n1 = prep["N"], prep["n1"]
    tri = np.asarray(pr["triples"], np.int64).reshape(-1, 3)
    H = len(tri)
    max_its = ransac_iterations(N, pr["probability"], pr["min_inliers"], pr["max_iterations"])
    n_use = 0 if N < pr["min_inliers"] else min(H, max_its)
    words = (n1 + 63) // 64
    out = {"N": N, "max_its": max_its, "n_use": n_use, "n_bad_index": prep["n_bad_index"], "indices1": prep["indices1"],
           "counts": np.zeros(H, np.int32), "masks": np.zeros((H, words), np.uint64), "R": np.zeros((H, 3, 3), f32),
           "t": np.zeros((H, 3), f32), "s": np.zeros(H, f32), "T12": np.zeros((H, 4, 4), f32), "gap": np.zeros(H),
           "near": np.full(H, math.inf), "n_bad_triple": 0, "prep": prep}
    for h in range(n_use):
        if N == 0 or tri[h].min() < 0 or tri[h].max() >= N:
            out["n_bad_triple"] += 1
            for k in ("R", "t", "s", "T12"):
                out[k][h] = np.nan
            continue
        hyp = horn(prep["X1"][tri[h]], prep["X2"][tri[h]], pr["fix_scale"], eig)
        inl, near = check_inliers(prep, hyp, pr["K1"], pr["K2"])
        out["counts"][h], out["masks"][h] = int(inl.sum()), mask_words(inl, prep["indices1"], n1)
        out["R"][h], out["t"][h], out["s"][h], out["T12"][h] = hyp["R"], hyp["t"], hyp["s"], hyp["T12"]
        out["gap"][h], out["near"][h] = hyp["gap"], near
    st = RansacState(N, pr["min_inliers"], max_its)
    st.iterations, st.best = start_iteration, best_so_far
    acc, n_inl, no_more = st.iterate(max(n_use - start_iteration, 0), out["counts"]) if n_use or N < pr["min_inliers"] else (-1, 0, False)
    out.update(accepted=acc, n_inliers=n_inl, no_more=bool(no_more), best_inliers=st.best, best_iteration=st.best_iteration,
               iterations=st.iterations)
    return out


# ---- scenes ------------------------------------------------------------------------------------------------------------
def _rot(rng, sigma):
    w = rng.normal(0, sigma, 3)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K


def _pose(rng):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = _rot(rng, 0.3), rng.normal(0, 1.0, 3)
    return T


def make_scene(n, seed, n1=None, n_hyp=300, fix_scale=False, outlier_frac=0.3, noise_px=0.7, min_inliers=20,
               max_iterations=300, probability=0.99):
    """A seeded key-frame pair with a planted Sim3: n kept correspondences scattered over n1 rows, inliers with about
    1 px of reprojection noise (noise_px per axis), a share of gross outliers >= 50 px off, triples drawn uniformly
    WITHOUT the reference's quirk (three distinct indices).  K = (500, 500, 320, 240) for both key frames."""
    rng = np.random.default_rng(seed)
    n1 = n + n // 3 + 2 if n1 is None else n1
    K = (500.0, 500.0, 320.0, 240.0)
    s12 = 1.0 if fix_scale else float(rng.uniform(0.7, 1.4))
    R12, t12 = _rot(rng, 0.1), rng.normal(0, 0.2, 3)
    T1w, T2w = _pose(rng), _pose(rng)
    X2 = np.stack([rng.uniform(-2, 2, n1), rng.uniform(-1.5, 1.5, n1), rng.uniform(4, 8, n1)], 1)
    X1 = s12 * X2 @ R12.T + t12
    # pixel noise as a lateral shift at the point's depth
    X1n, X2n = X1.copy(), X2.copy()
    for X in (X1n, X2n):
        X[:, :2] += rng.normal(0, noise_px, (n1, 2)) * X[:, 2:3] / K[0]
    out = rng.random(n1) < outlier_frac
    ang = rng.uniform(0, 2 * math.pi, n1)
    mag = rng.uniform(50, 200, n1)
    X1n[out, 0] += (np.cos(ang) * mag * X1n[:, 2] / K[0])[out]
    X1n[out, 1] += (np.sin(ang) * mag * X1n[:, 2] / K[0])[out]
    inv = np.linalg.inv
    Xw1 = (X1n - T1w[:3, 3]) @ inv(T1w[:3, :3]).T
    Xw2 = (X2n - T2w[:3, 3]) @ inv(T2w[:3, :3]).T
    valid = np.zeros(n1, np.uint8)
    valid[rng.permutation(n1)[:n]] = 1
    tri = np.zeros((n_hyp, 3), np.int32)
    for h in range(n_hyp):
        tri[h] = rng.choice(n, 3, replace=False) if n >= 3 else 0
    return {"valid": valid, "Xw1": Xw1.astype(f32), "Xw2": Xw2.astype(f32), "octave1": rng.integers(0, 4, n1).astype(np.int32),
            "octave2": rng.integers(0, 4, n1).astype(np.int32), "T1w": T1w.astype(f32), "T2w": T2w.astype(f32), "K1": K, "K2": K,
            "level_sigma2": SIGMA2.copy(), "fix_scale": bool(fix_scale), "probability": probability, "min_inliers": min_inliers,
            "max_iterations": max_iterations, "triples": tri, "true": {"s": s12, "R": R12, "t": t12}, "outlier": out}


PARITY_SIZES = (3, 19, 20, 21, 63, 64, 65, 300, 2816)  # 19 < min_inliers = 20 (one iteration) < 21; 63..65 around a ballot word


def parity_scenes(n):
    """The committed scenes of the device parity test at size n: fixed and free scale; n1 > N with the invalid rows
    scattered; H = 300, so H > max_its wherever max_its is smaller (N = 20: 1, N = 21: 3, N = 63..65: 142..156); H = 1 and 5
    at the ballot-word sizes."""
    sc = [make_scene(n, 7000 + n, fix_scale=False), make_scene(n, 8000 + n, fix_scale=True)]
    if n in (63, 64, 65):
        sc += [make_scene(n, 9000 + n, n_hyp=1), make_scene(n, 9500 + n, n_hyp=5, fix_scale=True)]
    return sc
