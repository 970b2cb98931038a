"""NumPy float64 restatement of Optimizer::OptimizeEssentialGraph (Optimizer.cc:780-1045): the oracle of the device Sim3
pose graph (orbgpu_essential_graph*).

g2o is not part of the reference tree, so its behaviour is restated here from its published algorithm
(OptimizationAlgorithmLevenberg with setUserLambdaInit(1e-16) over BlockSolver_7_3, VertexSim3Expmap, EdgeSim3 with numeric
Jacobians, Sim3::log): every comparison against this file is "vs CPU restatement; g2o boundary unpinned".  The definition,
conventions G1-G12, is in include/orbgpu.h above orbgpu_essential_graph_device and DESIGN.md 9.28.

All arithmetic is IEEE double, unfused, three-term sums left to right.  A state is 8 doubles (qx, qy, qz, qw, tx, ty, tz, s)
and nothing is ever normalised.  The per-edge functions work on arrays of states ([N][8]), element by element the
operations of the device's per-lane code.  Sums over edges run sequentially in `order` (default: edge order), so that a
permutation of `order` shows what the summation order alone does; `libm_nudge` moves every result of exp, sin, cos, acos
and log by that many ulps, which shows what another libm's rounding does through the 1e-9 difference quotient."""
import numpy as np

from pose_model import DBL_MAX, quat_from_matrix, quat_normalize
import sim3opt_model as S3

DELTA = 1e-9      # G5
EPS = 1e-5        # G3
LAMBDA0 = 1e-16   # G8
MAX_VERTICES, MAX_EDGES, MAX_POINTS, MAX_ENVELOPE, MAX_ITERATIONS = 8192, 1 << 18, 1 << 22, 1 << 26, 100
THREADS = 512     # EG_THREADS in csrc/essential_graph.hip
LOG_CASES = ("small_theta_small_sigma", "theta_small_sigma", "small_theta_sigma", "theta_sigma")


def _nudge(v, n):
    v = np.asarray(v, np.float64)
    for _ in range(abs(n)):
        v = np.nextafter(v, np.inf if n > 0 else -np.inf)
    return v


# ---- G2: the algebra, on arrays of states -------------------------------------------------------------------------------
def qmat(q):
    """R [..., 3, 3] of quaternions [..., 4] (x, y, z, w), not normalised (opt_math.h quat_to_matrix)."""
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0], R[..., 0, 1], R[..., 0, 2] = 1.0 - (tyy + tzz), txy - twz, txz + twy
    R[..., 1, 0], R[..., 1, 1], R[..., 1, 2] = txy + twz, 1.0 - (txx + tzz), tyz - twx
    R[..., 2, 0], R[..., 2, 1], R[..., 2, 2] = txz - twy, tyz + twx, 1.0 - (txx + tyy)
    return R


def qmul(a, b):
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([((aw * bx + ax * bw) + ay * bz) - az * by, ((aw * by + ay * bw) + az * bx) - ax * bz,
                     ((aw * bz + az * bw) + ax * by) - ay * bx, ((aw * bw - ax * bx) - ay * by) - az * bz], -1)


def mv(R, v):
    return np.stack([(R[..., r, 0] * v[..., 0] + R[..., r, 1] * v[..., 1]) + R[..., r, 2] * v[..., 2] for r in range(3)], -1)


def mtv(R, v):
    return np.stack([(R[..., 0, r] * v[..., 0] + R[..., 1, r] * v[..., 1]) + R[..., 2, r] * v[..., 2] for r in range(3)], -1)


def s_mul(A, B):
    """A * B = (qa qb, sa (Ra tb) + ta, sa sb)."""
    with np.errstate(all="ignore"):
        q = qmul(A[..., :4], B[..., :4])
        t = A[..., 7:8] * mv(qmat(A[..., :4]), B[..., 4:7]) + A[..., 4:7]
        return np.concatenate([q, t, A[..., 7:8] * B[..., 7:8]], -1)


def s_inv(S):
    """S^-1 = (q conjugate, R'((-1 / s) t), 1 / s)."""
    with np.errstate(all="ignore"):
        q = S[..., :4] * np.array([-1.0, -1.0, -1.0, 1.0])
        i_s = 1.0 / S[..., 7:8]
        return np.concatenate([q, mtv(qmat(S[..., :4]), -i_s * S[..., 4:7]), i_s], -1)


def s_map(S, X):
    """S X = s (R X) + t."""
    with np.errstate(all="ignore"):
        return S[..., 7:8] * mv(qmat(S[..., :4]), X) + S[..., 4:7]


def lu_solve3(W, t):
    """W x = t, 3x3, by LU with partial pivoting: column by column the later row is swapped in when its entry is
    strictly larger in magnitude (row 1 against 0, then 2 against 0; then 2 against 1)."""
    a = [[W[..., r, c].copy() for c in range(3)] for r in range(3)]
    b = [t[..., r].copy() for r in range(3)]

    def swap(p, q, col):
        m = np.abs(a[q][col]) > np.abs(a[p][col])
        for c in range(3):
            a[p][c], a[q][c] = np.where(m, a[q][c], a[p][c]), np.where(m, a[p][c], a[q][c])
        b[p], b[q] = np.where(m, b[q], b[p]), np.where(m, b[p], b[q])

    with np.errstate(all="ignore"):
        swap(0, 1, 0)
        swap(0, 2, 0)
        for r in (1, 2):
            m = a[r][0] / a[0][0]
            a[r][1] = a[r][1] - m * a[0][1]
            a[r][2] = a[r][2] - m * a[0][2]
            b[r] = b[r] - m * b[0]
        swap(1, 2, 1)
        m = a[2][1] / a[1][1]
        a[2][2] = a[2][2] - m * a[1][2]
        b[2] = b[2] - m * b[1]
        x2 = b[2] / a[2][2]
        x1 = (b[1] - a[1][2] * x2) / a[1][1]
        x0 = ((b[0] - a[0][1] * x1) - a[0][2] * x2) / a[0][0]
    return np.stack([x0, x1, x2], -1)


def s_log(S, libm_nudge=0, cases=None):
    """G3: log of states [..., 8] -> (omega, upsilon, sigma) [..., 7].  cases: an int array [4] that counts LOG_CASES."""
    S = np.asarray(S, np.float64)
    q, t, s = S[..., :4], S[..., 4:7], S[..., 7]
    with np.errstate(all="ignore"):
        sigma = _nudge(np.log(s), libm_nudge)
        R = qmat(q)
        d = 0.5 * (((R[..., 0, 0] + R[..., 1, 1]) + R[..., 2, 2]) - 1.0)
        dR = np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1)
        small_th = d > 1.0 - EPS
        small_sigma = np.abs(sigma) < EPS
        th = _nudge(np.arccos(d), libm_nudge)
        omega = np.where(small_th[..., None], 0.5 * dR, (th / (2.0 * np.sqrt(1.0 - d * d)))[..., None] * dR)
        sn, cs = _nudge(np.sin(th), libm_nudge), _nudge(np.cos(th), libm_nudge)
        th2 = th * th
        sigma2 = sigma * sigma
        # O5's four cases with s in the place of s_x
        C = np.where(small_sigma, 1.0, (s - 1.0) / sigma)
        A_ss, B_ss = 0.5, 1.0 / 6.0
        A_ts, B_ts = (1.0 - cs) / th2, (th - sn) / (th2 * th)
        A_sl = ((sigma - 1.0) * s + 1.0) / sigma2
        B_sl = (((0.5 * sigma2 - sigma) + 1.0) * s) / (sigma2 * sigma)   # as published (G3)
        a, b = s * sn, s * cs
        c = th2 + sigma2
        A_tl = (a * sigma + (1.0 - b) * th) / (th * c)
        B_tl = (C - ((b - 1.0) * sigma + a * th) / c) / th2
        A = np.where(small_sigma, np.where(small_th, A_ss, A_ts), np.where(small_th, A_sl, A_tl))
        B = np.where(small_sigma, np.where(small_th, B_ss, B_ts), np.where(small_th, B_sl, B_tl))
        z = np.zeros_like(d)
        O = np.stack([np.stack([z, -omega[..., 2], omega[..., 1]], -1), np.stack([omega[..., 2], z, -omega[..., 0]], -1),
                      np.stack([-omega[..., 1], omega[..., 0], z], -1)], -2)
        O2 = np.stack([np.stack([(O[..., r, 0] * O[..., 0, c_] + O[..., r, 1] * O[..., 1, c_]) + O[..., r, 2] * O[..., 2, c_]
                                 for c_ in range(3)], -1) for r in range(3)], -2)
        W = (A[..., None, None] * O + B[..., None, None] * O2) + C[..., None, None] * np.eye(3)
        ups = lu_solve3(W, t)
    if cases is not None:
        idx = 2 * (~small_sigma).astype(int) + (~small_th).astype(int)
        cases += np.bincount(np.ravel(idx), minlength=4)
    return np.concatenate([omega, ups, sigma[..., None]], -1)


def exp_state(x, fix_scale, libm_nudge=0, cases=None):
    """exp(x) of O5 as a state; with fix_scale x[6] is set to 0 first (G5).  cases: [4] counts of O5's branches, indexed
    as LOG_CASES."""
    x = np.array(x, np.float64)
    if fix_scale:
        x[6] = 0.0
    qx, tx, sx = S3.sim3_exp(x, libm_nudge)
    if cases is not None:
        with np.errstate(all="ignore"):
            th = np.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])
        cases[2 * int(not abs(x[6]) < EPS) + int(not th < EPS)] += 1
    return np.concatenate([qx, tx, [sx]])


def s_update(S, x, fix_scale, libm_nudge=0, cases=None):
    """Vertex <- exp(x) vertex (O4): (q_x q, s_x (R_x t) + t_x, s_x s) -- the product of G2."""
    return s_mul(exp_state(x, fix_scale, libm_nudge, cases), S)


def state_from_pose(Tcw):
    """orbgpu_sim3_from_pose: quat_normalize(quat_from_matrix((double)R)), (double)t, 1."""
    T = np.asarray(Tcw, np.float32).reshape(4, 4).astype(np.float64)
    return np.concatenate([quat_normalize(quat_from_matrix(T[:3, :3])), T[:3, 3], [1.0]])


def tiw_of(S):
    """G10: (float) of R and of t * (1 / s), last row 0 0 0 1, for states [V][8] -> float32 [V][16]."""
    S = np.asarray(S, np.float64).reshape(-1, 8)
    T = np.zeros((len(S), 4, 4), np.float32)
    with np.errstate(all="ignore"):
        T[:, :3, :3] = qmat(S[:, :4]).astype(np.float32)
        T[:, :3, 3] = (S[:, 4:7] * (1.0 / S[:, 7:8])).astype(np.float32)
    T[:, 3, 3] = 1.0
    return T.reshape(len(S), 16)


def correct_points(Siw, Scw, pos, ref):
    """G11: (out float32 [M][3], n_bad_ref)."""
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    ref = np.asarray(ref, np.int64)
    ok = (ref >= 0) & (ref < len(Scw))
    out = pos.copy()
    r = ref[ok]
    if len(r):
        Pc = s_map(np.asarray(Scw, np.float64)[r], pos[ok].astype(np.float64))
        with np.errstate(all="ignore"):
            out[ok] = s_map(s_inv(np.asarray(Siw, np.float64)[r]), Pc).astype(np.float32)
    return out, int((~ok).sum())


# ---- G1, G6: the graph ------------------------------------------------------------------------------------------------
def index_of(pr):
    """Taken edges (caller order), n_bad_index, the active mask and the free active rows."""
    V = len(pr["Scw"])
    ei, ej = np.asarray(pr["edge_i"], np.int64), np.asarray(pr["edge_j"], np.int64)
    ok = (ei >= 0) & (ei < V) & (ej >= 0) & (ej < V) & (ei != ej)
    taken = np.flatnonzero(ok)
    active = np.zeros(V, bool)
    active[ei[taken]] = True
    active[ej[taken]] = True
    free = np.flatnonzero(active & (np.asarray(pr["fixed"]) == 0))
    return taken, int((~ok).sum()), active, free


def measurements(pr, taken):
    Scw, Snc = np.asarray(pr["Scw"], np.float64), np.asarray(pr["Snc"], np.float64)
    i, j = np.asarray(pr["edge_i"])[taken], np.asarray(pr["edge_j"])[taken]
    kind = np.asarray(pr["edge_kind"])[taken]
    src = np.where((kind == 0)[:, None, None], Scw[None], Snc[None]) if len(taken) else np.zeros((0, len(Scw), 8))
    a = np.arange(len(taken))
    return s_mul(src[a, j], s_inv(src[a, i]))


def edge_errors(Mm, Si, Sj, libm_nudge=0, cases=None):
    """G4: e = log(M * S_i * S_j^-1) [E][7]."""
    return s_log(s_mul(s_mul(Mm, Si), s_inv(Sj)), libm_nudge, cases)


def chi2_terms(e):
    with np.errstate(all="ignore"):
        c = e[:, 0] * e[:, 0]
        for r in range(1, 7):
            c = c + e[:, r] * e[:, r]
    return c


def _seq(a, order):
    return float(np.cumsum(a[order])[-1]) if len(order) else 0.0


def jacobians(Mm, St, i, j, fix_scale, libm_nudge=0):
    """G5: Ji, Jj [E][7 error rows][7 parameters] by central differences through the update."""
    E = len(i)
    Ji, Jj = np.zeros((E, 7, 7)), np.zeros((E, 7, 7))
    scale = 1.0 / (2.0 * DELTA)
    for k in range(7):
        x = np.zeros(7)
        x[k] = DELTA
        Pp, Pm = exp_state(x, fix_scale, libm_nudge), exp_state(-x, fix_scale, libm_nudge)
        Sp, Sm = s_mul(Pp, St), s_mul(Pm, St)
        with np.errstate(all="ignore"):
            Ji[:, :, k] = (edge_errors(Mm, Sp[i], St[j], libm_nudge) - edge_errors(Mm, Sm[i], St[j], libm_nudge)) * scale
            Jj[:, :, k] = (edge_errors(Mm, St[i], Sp[j], libm_nudge) - edge_errors(Mm, St[i], Sm[j], libm_nudge)) * scale
    return Ji, Jj


def assemble(e, Ji, Jj, i, j, slot, nf, order):
    """G6: dense H [7 nf][7 nf] and b over the free active vertices (slot[v] >= 0), every sum in `order`, an edge's seven
    error rows one by one."""
    H, b = np.zeros((7 * nf, 7 * nf)), np.zeros(7 * nf)
    with np.errstate(all="ignore"):
        for k in order:
            a, c = slot[i[k]], slot[j[k]]
            for f, J in ((a, Ji[k]), (c, Jj[k])):
                if f < 0:
                    continue
                blk = H[7 * f:7 * f + 7, 7 * f:7 * f + 7]
                for r in range(7):
                    blk += np.outer(J[r], J[r])
                g = J[0] * e[k, 0]
                for r in range(1, 7):
                    g = g + J[r] * e[k, r]
                b[7 * f:7 * f + 7] -= g
            if a >= 0 and c >= 0:
                blk = H[7 * a:7 * a + 7, 7 * c:7 * c + 7]
                for r in range(7):
                    blk += np.outer(Ji[k][r], Jj[k][r])
                H[7 * c:7 * c + 7, 7 * a:7 * a + 7] = blk.T
    return H, b


def solve(H, lam, b):
    """G7: (H + lam I) x = b by LL' (column by column; the dot products vectorised, so the order inside them is numpy's --
    the device's is k ascending in its own permutation: a difference of rounding, inside the measured spread).  A pivot
    that is not > 0, NaN included: (False, 0)."""
    n = len(b)
    L = np.tril(H)
    L[np.diag_indices(n)] += lam
    with np.errstate(all="ignore"):
        for j in range(n):
            if j:
                L[j:, j] -= L[j:, :j] @ L[j, :j]
            d = L[j, j]
            if not d > 0.0:
                return False, np.zeros(n)
            d = np.sqrt(d)
            L[j, j] = d
            L[j + 1:, j] /= d
        y = b.copy()
        for k in range(n):
            y[k] /= L[k, k]
            y[k + 1:] -= L[k + 1:, k] * y[k]
        for k in range(n - 1, -1, -1):
            y[k] /= L[k, k]
            y[:k] -= L[k, :k] * y[k]
    return True, y


def essential_graph(pr, order=None, libm_nudge=0):
    """The definition.  pr: Scw, Snc [V][8], fixed [V], edge_i, edge_j, edge_kind [E], fix_scale, n_iterations and,
    optionally, world_pos [M][3] float32 with point_ref [M].  order: a permutation of the taken edges for the sums.
    Returns a dict: Siw_d [V][8], Tiw [V][16] float32, pos, chi2_start, chi2_end, iterations, trials, trace (one 'a' /
    'r' / 'p' per trial: accepted, rejected, rejected with a failed pivot), n_edges, n_bad_index, n_free_active,
    n_bad_ref, log_cases, exp_cases (counts in the order of LOG_CASES)."""
    Scw = np.array(pr["Scw"], np.float64).reshape(-1, 8)
    taken, n_bad_index, active, free = index_of(pr)
    V, E, nf = len(Scw), len(taken), len(free)
    fix_scale = bool(pr["fix_scale"])
    i, j = np.asarray(pr["edge_i"], np.int64)[taken], np.asarray(pr["edge_j"], np.int64)[taken]
    Mm = measurements(pr, taken)
    slot = np.full(V, -1)
    slot[free] = np.arange(nf)
    order = np.arange(E) if order is None else np.asarray(order)
    log_cases, exp_cases = np.zeros(4, np.int64), np.zeros(4, np.int64)
    St = Scw.copy()

    def chi2_at(S, cases=None):
        return _seq(chi2_terms(edge_errors(Mm, S[i], S[j], libm_nudge, cases)), order)

    cur = chi2_at(St)
    out = dict(chi2_start=cur, iterations=0, trials=0, trace="")
    lam, nu = 0.0, 2.0
    for it in range(int(pr["n_iterations"])):
        e = edge_errors(Mm, St[i], St[j], libm_nudge, log_cases)
        cur = _seq(chi2_terms(e), order)
        Ji, Jj = jacobians(Mm, St, i, j, fix_scale, libm_nudge)
        H, b = assemble(e, Ji, Jj, i, j, slot, nf, order)
        if it == 0:
            lam, nu = LAMBDA0, 2.0
        rho, trial, stop = 0.0, 0, False
        out["iterations"] += 1
        while True:
            ok, x = solve(H, lam, b)
            cand = St.copy()
            for f, v in enumerate(free):
                cand[v] = s_update(St[v], x[7 * f:7 * f + 7], fix_scale, libm_nudge, exp_cases)
            tmp = chi2_at(cand)
            if not ok:
                tmp = DBL_MAX
            with np.errstate(all="ignore"):
                scale = 0.0
                for a in range(7 * nf):
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
                St, cur = cand, tmp
                out["trace"] += "a"
            else:
                with np.errstate(all="ignore"):
                    lam = lam * nu
                    nu = nu * 2.0
                if not np.isfinite(lam):
                    stop = True
                out["trace"] += "r" if ok else "p"
            trial += 1
            if stop or not (rho < 0 and trial < 10):
                break
        if trial == 10 or rho == 0 or stop:
            break
    out.update(chi2_end=cur, Siw_d=St, Tiw=tiw_of(St), n_edges=E, n_bad_index=n_bad_index, n_free_active=nf,
               log_cases=log_cases, exp_cases=exp_cases, n_bad_ref=0, pos=None)
    if pr.get("world_pos") is not None:
        out["pos"], out["n_bad_ref"] = correct_points(St, Scw, pr["world_pos"], pr["point_ref"])
    return out


DISCRETE = ("iterations", "trials", "trace", "n_edges", "n_bad_index", "n_free_active", "n_bad_ref")


def state_deviation(a, b):
    """Largest entry-wise deviation of the states of two results (NaN against NaN counts as equal)."""
    with np.errstate(all="ignore"):
        d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    d = d[~(np.isnan(np.asarray(a, np.float64)) & np.isnan(np.asarray(b, np.float64)))]
    return float(d.max()) if d.size else 0.0


def model_spread(pr, base, n_perm=8, seed=0):
    """The model's own spread on a problem: the largest state deviation over n_perm seeded permutations of the edge order
    plus the two runs libm_nudge = +-1, and how many of those runs changed a discrete output."""
    rng = np.random.default_rng(20_000 + seed)
    runs = [essential_graph(pr, order=rng.permutation(base["n_edges"])) for _ in range(n_perm)]
    runs += [essential_graph(pr, libm_nudge=-1), essential_graph(pr, libm_nudge=1)]
    dev, flips = 0.0, 0
    for r in runs:
        dev = max(dev, state_deviation(r["Siw_d"], base["Siw_d"]))
        flips += int(any(r[k] != base[k] for k in DISCRETE))
    return dev, flips


# ---- scenes ------------------------------------------------------------------------------------------------------------
def _rand_rot(rng, angle):
    ax = rng.normal(0, 1, 3)
    ax /= np.linalg.norm(ax)
    return angle * ax


def true_states(V, seed, radius=4.0):
    """Key frames on a circle, one Sim3 (world -> camera, scale 1) each."""
    rng = np.random.default_rng(30_000 + seed)
    out = np.zeros((V, 8))
    for v in range(V):
        a = 2.0 * np.pi * v / max(V, 3)
        x = np.concatenate([np.array([0.0, a, 0.0]) + rng.normal(0, 0.05, 3),
                            np.array([radius * np.cos(a), 0.2 * rng.normal(), radius * np.sin(a)]), [0.0]])
        out[v] = exp_state(x, True)
        out[v, :4] = quat_normalize(out[v, :4])
    return out


def make_scene(V, seed, reach=1, fix_scale=False, rot_drift=0.05, scale_drift=0.1, trans_drift=0.3, n_corrected=2,
               n_iterations=20, closed=True, n_points=0, noise=0.0, perturb=0.0, perturb_scale=True, compose=False):
    """A loop closure on a ring of V key frames (G1): row 0 is pLoopKF (fixed), the chain drifts away from the truth on its
    way round (rot_drift rad, trans_drift m and, without fix_scale, a relative scale_drift at the last row); the last
    n_corrected rows carry CorrectedSim3 (their true state) with their drifted state as NonCorrectedSim3.  The chain and
    neighbour edges (kind 1) measure the drifted map, the edges that cross the seam between row V - 1 and row 0 are the loop
    connections (kind 0).  compose: the drift accumulates step by step, as odometry's does, so that the map stays
    consistent from one key frame to the next and is off by the whole drift across the seam."""
    rng = np.random.default_rng(40_000 + seed)
    G = true_states(V, seed)
    x = np.concatenate([_rand_rot(rng, rot_drift), rng.normal(0, 1, 3) * trans_drift / np.sqrt(3.0),
                        [0.0 if fix_scale else np.log1p(scale_drift)]])
    if compose:  # odometry: every step of the chain is off by its share of the drift, and the steps add up
        Snc = [G[0]]
        for v in range(1, V):
            step = s_mul(G[v], s_inv(G[v - 1]))
            Snc.append(s_mul(exp_state(x / (V - 1) + rng.normal(0, noise, 7), fix_scale), s_mul(step, Snc[-1])))
        Snc = np.stack(Snc)
    else:
        Snc = np.stack([s_mul(exp_state(x * (v / max(V - 1, 1)) + rng.normal(0, noise, 7) * (v > 0), fix_scale), G[v])
                        for v in range(V)])
    Scw = Snc.copy()
    for v in range(1, V):  # entry estimates off the map the edges measure
        if perturb:
            Scw[v] = s_mul(exp_state(rng.normal(0, perturb, 7) * ([1.0] * 6 + [float(perturb_scale)]), fix_scale), Snc[v])
    if closed:
        Scw[V - n_corrected:] = G[V - n_corrected:]
    pairs = [(v, v + d) for v in range(V) for d in range(1, reach + 1) if v + d < V]
    kinds = [1] * len(pairs)
    if closed:
        seam = [(v, (v + d) % V) for v in range(V) for d in range(1, reach + 1) if v + d >= V]
        pairs += seam
        kinds += [0] * len(seam)
    fixed = np.zeros(V, np.uint8)
    fixed[0] = 1
    sc = {"Scw": Scw, "Snc": Snc, "fixed": fixed, "edge_i": np.array([p[0] for p in pairs], np.int32),
          "edge_j": np.array([p[1] for p in pairs], np.int32), "edge_kind": np.array(kinds, np.int32),
          "fix_scale": bool(fix_scale), "n_iterations": int(n_iterations), "true": G}
    if n_points:
        add_points(sc, n_points, seed)
    return sc


def add_points(sc, n_points, seed, bad_refs=()):
    rng = np.random.default_rng(50_000 + seed)
    V = len(sc["Scw"])
    sc["world_pos"] = rng.normal(0, 3, (n_points, 3)).astype(np.float32)
    sc["point_ref"] = rng.integers(0, V, n_points).astype(np.int32)
    for k, r in enumerate(bad_refs):
        sc["point_ref"][(7 * k + 3) % n_points] = r
    return sc


def with_edges(sc, n_edges, seed):
    """The scene with exactly n_edges edges: its own first, then seeded pairs of kind 1 (parallel ones among them)."""
    rng = np.random.default_rng(60_000 + seed)
    V = len(sc["Scw"])
    i, j, k = list(sc["edge_i"][:n_edges]), list(sc["edge_j"][:n_edges]), list(sc["edge_kind"][:n_edges])
    while len(i) < n_edges:
        a, b = rng.integers(0, V, 2)
        if a != b:
            i.append(a), j.append(b), k.append(1)
    sc = dict(sc)
    sc["edge_i"], sc["edge_j"], sc["edge_kind"] = np.array(i, np.int32), np.array(j, np.int32), np.array(k, np.int32)
    return sc


def _parity_scenes():
    """The committed scenes of the device parity test, the smallest that can go wrong (W = THREADS); (name, scene) pairs.
    tests/test_eg_model.py asserts that none of them flips a discrete output under model_spread."""
    sc = []
    s = make_scene(2, 1, closed=False, perturb=0.05, n_iterations=2, n_points=5)
    sc.append(("v2_one_edge", s))
    sc.append(("chain3", make_scene(3, 2, closed=False, perturb=0.05, n_iterations=2, n_points=9)))
    for V in (8, 40):
        for fs in (False, True):
            sc.append(("ring%d_fix%d" % (V, fs), make_scene(V, 10 + V + fs, reach=2 if V == 40 else 1, fix_scale=fs,
                                                            n_iterations=3 if V == 8 else 4, n_points=64)))
    for n in (63, 64, 65, THREADS - 1, THREADS, THREADS + 1):
        sc.append(("edges%d" % n, with_edges(make_scene(24, 100 + n, reach=2, n_iterations=3, noise=0.002), n, n)))
    for nf in (9, 10, 73, 74):  # 7 nf crosses 64 and THREADS
        sc.append(("free%d" % nf, make_scene(nf + 1, 200 + nf, reach=2, fix_scale=bool(nf & 1), n_iterations=3)))
    # two components, each with its own fixed vertex, beside an isolated vertex
    a, b = make_scene(6, 301), make_scene(5, 302)
    two = {"Scw": np.concatenate([a["Scw"], b["Scw"], true_states(1, 303)]),
           "Snc": np.concatenate([a["Snc"], b["Snc"], true_states(1, 304)]),
           "fixed": np.concatenate([a["fixed"], b["fixed"], [0]]).astype(np.uint8),
           "edge_i": np.concatenate([a["edge_i"], b["edge_i"] + 6]).astype(np.int32),
           "edge_j": np.concatenate([a["edge_j"], b["edge_j"] + 6]).astype(np.int32),
           "edge_kind": np.concatenate([a["edge_kind"], b["edge_kind"]]).astype(np.int32),
           "fix_scale": False, "n_iterations": 3}
    sc.append(("two_components_isolated", add_points(two, 40, 305)))
    # parallel edges (both directions), an edge between two fixed vertices and three bad edges
    p = make_scene(7, 310, n_iterations=3)
    p["fixed"][3] = 1
    p["edge_i"] = np.concatenate([p["edge_i"], [1, 2, 0, 3, 4, -1, 2]]).astype(np.int32)
    p["edge_j"] = np.concatenate([p["edge_j"], [2, 1, 3, 0, 4, 2, 7]]).astype(np.int32)
    p["edge_kind"] = np.concatenate([p["edge_kind"], [1, 0, 1, 0, 1, 1, 0]]).astype(np.int32)
    sc.append(("parallel_fixed_pair_bad_edges", add_points(p, 30, 311, bad_refs=(-1, 7))))
    sc.append(("iterations0", make_scene(6, 320, n_iterations=0, n_points=10)))
    sc.append(("iterations1", make_scene(6, 321, n_iterations=1, n_points=10)))
    # a pure scale drift: the rotations stay where they are, G3's small-angle case with |sigma| >= eps and O5's
    sc.append(("scale_only", make_scene(6, 330, rot_drift=0.0, trans_drift=0.0, scale_drift=0.05, n_iterations=6)))
    # two rows that differ from the map by their scale alone: O5's small-angle case with |sigma| >= eps in the update
    v3 = make_scene(3, 360, closed=False, rot_drift=0.0, trans_drift=0.0, scale_drift=0.0, n_iterations=2)
    for v in (1, 2):
        v3["Scw"][v] = s_mul(exp_state([0, 0, 0, 0, 0, 0, 0.05 * v], False), v3["Snc"][v])
    sc.append(("scale_steps", v3))
    # a small drift with the scale fixed: G3's small-angle, small-sigma case at every edge
    sc.append(("small_fix", make_scene(6, 331, fix_scale=True, rot_drift=1e-3, trans_drift=0.01, n_iterations=2)))
    # a drift Gauss-Newton oversteps: rejected trials
    sc.append(("large_drift", make_scene(12, 340, rot_drift=1.2, trans_drift=2.0, scale_drift=0.8, n_iterations=8)))
    # a state without scale: log(0), every sum NaN, every pivot fails and nothing is ever accepted
    z = make_scene(4, 350, n_iterations=3)
    z["Scw"][2, 7] = 0.0
    sc.append(("failed_pivot", z))
    return sc


PARITY_SCENES = _parity_scenes()
