"""NumPy float64 restatement of Optimizer::OptimizeSim3 (Optimizer.cc:1079-1236): the oracle of the device 7-DoF
refinement of a loop candidate's Sim3 (orbgpu_sim3_optimize*).

g2o is not part of the reference tree, so its behaviour is restated here from its published algorithm
(OptimizationAlgorithmLevenberg over a dense 7x7 solver, EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ with numeric
Jacobians, RobustKernelHuber, Sim3): every comparison against this file is "vs CPU restatement; g2o boundary unpinned".
The definition, conventions O1-O9, is in include/orbgpu.h above orbgpu_sim3_optimize_device and DESIGN.md section 2.

All arithmetic is IEEE double unless a float32 is named.  Sums over edges run sequentially in `order` (default: edge
order, e12 of a correspondence before its e21), so that a permutation of `order` shows what the summation order alone
does to the result; `libm_nudge` moves every result of exp, sin and cos by that many ulps, which shows what another
libm's rounding does through the 1e-9 difference quotient."""
import numpy as np

from pose_model import (cholesky_solve, huber, quat_from_matrix, quat_mul, quat_normalize, quat_to_matrix, seq_sum, mat_vec,
                        skew)
import sim3_model
from sim3_model import rt_apply

DELTA = 1e-9          # O6
EPS = 1e-5            # O5
TH2 = 10.0            # LoopClosing.cc:327
DBL_MAX = np.finfo(np.float64).max
TRI = [(a, b) for a in range(7) for b in range(a, 7)]
NLEVELS = sim3_model.NLEVELS
INV_LEVEL_SIGMA2 = (np.float32(1.0) / sim3_model.SIGMA2).astype(np.float32)


# ---- Sim3 (O4, O5) -----------------------------------------------------------------------------------------------------
def _nudge(v, n):
    v = np.float64(v)
    for _ in range(abs(n)):
        v = np.nextafter(v, np.inf if n > 0 else -np.inf)
    return v


def sim3_exp(x, libm_nudge=0):
    """exp of x = (omega, upsilon, sigma): (q_x not normalised, t_x, s_x)."""
    w, v, sigma = np.asarray(x[:3], np.float64), np.asarray(x[3:6], np.float64), np.float64(x[6])
    with np.errstate(all="ignore"):
        th = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
        sx = _nudge(np.exp(sigma), libm_nudge)
        O = skew(w)
        O2 = np.array([[(O[r, 0] * O[0, c] + O[r, 1] * O[1, c]) + O[r, 2] * O[2, c] for c in range(3)] for r in range(3)])
        I = np.eye(3)
        small_th, small_sigma = bool(th < EPS), bool(abs(sigma) < EPS)
        if not small_th:
            sn, cs = _nudge(np.sin(th), libm_nudge), _nudge(np.cos(th), libm_nudge)
        if small_sigma:
            C = 1.0
            if small_th:
                A, B = 0.5, 1.0 / 6.0
            else:
                A = (1.0 - cs) / (th * th)
                B = (th - sn) / ((th * th) * th)
        else:
            C = (sx - 1.0) / sigma
            if small_th:
                sigma2 = sigma * sigma
                A = ((sigma - 1.0) * sx + 1.0) / sigma2
                B = (((0.5 * sigma2 - sigma) + 1.0) * sx) / (sigma2 * sigma)
            else:
                a, b, th2 = sx * sn, sx * cs, th * th
                c = th2 + sigma * sigma
                A = (a * sigma + (1.0 - b) * th) / (th * c)
                B = (C - ((b - 1.0) * sigma + a * th) / c) / th2
        if small_th:
            R = (I + O) + O2
        else:
            R = (I + (sn / th) * O) + ((1.0 - cs) / (th * th)) * O2
        W = (A * O + B * O2) + C * I
        return quat_from_matrix(R), mat_vec(W, v), sx


def sim3_update(state, x, fix_scale, libm_nudge=0):
    """S <- exp(x) S; no renormalisation."""
    q, t, s = state
    x = np.array(x, np.float64)
    if fix_scale:
        x[6] = 0.0
    qx, tx, sx = sim3_exp(x, libm_nudge)
    with np.errstate(all="ignore"):
        return quat_mul(qx, q), sx * mat_vec(quat_to_matrix(qx), t) + tx, sx * s


def state_from_floats(R12, t12, s12):
    R = np.asarray(R12, np.float32).reshape(3, 3).astype(np.float64)
    return (quat_normalize(quat_from_matrix(R)), np.asarray(t12, np.float32).astype(np.float64).reshape(3),
            np.float64(np.float32(s12)))


def to_cvmat(state):
    """Converter::toCvMat(g2o::Sim3): (float)(s R), (float)t."""
    q, t, s = state
    T = np.eye(4, dtype=np.float32)
    with np.errstate(all="ignore"):
        T[:3, :3] = (s * quat_to_matrix(q)).astype(np.float32)
        T[:3, 3] = np.asarray(t).astype(np.float32)
    return T


def scw_of(state, T2w):
    """LoopClosing.cc:334-336: toCvMat(S12 * Smw), Smw = (R2w, t2w, 1) of the float pose."""
    T = np.asarray(T2w, np.float32).reshape(4, 4).astype(np.float64)
    qm, tm = quat_normalize(quat_from_matrix(T[:3, :3])), T[:3, 3]
    q, t, s = state
    with np.errstate(all="ignore"):
        return to_cvmat((quat_mul(q, qm), s * mat_vec(quat_to_matrix(q), tm) + t, s * 1.0))


# ---- edges (O3) --------------------------------------------------------------------------------------------------------
def _xf(states):
    """R [S][3][3], t [S][3], s [S], 1 / s and the inverse's translation for a list of states."""
    R = np.stack([quat_to_matrix(q) for q, _, _ in states])
    t = np.stack([np.asarray(t_, np.float64) for _, t_, _ in states])
    s = np.array([s_ for _, _, s_ in states], np.float64)
    with np.errstate(all="ignore"):
        i_s = 1.0 / s
        u = -i_s[:, None] * t
        ti = np.stack([(R[:, 0, r] * u[:, 0] + R[:, 1, r] * u[:, 1]) + R[:, 2, r] * u[:, 2] for r in range(3)], 1)
    return R, t, s, i_s, ti


def pair_errors_multi(states, X1, X2, obs1, obs2, K1, K2):
    """e12 [S][N][2], e21 [S][N][2] for a list of S states; every state's arithmetic is pair_errors' (O3)."""
    R, t, s, i_s, ti = _xf(states)
    c = lambda a: a[:, None]  # noqa: E731  per-state scalar against the N correspondences
    with np.errstate(all="ignore"):
        P = [c(s) * ((c(R[:, r, 0]) * X2[:, 0] + c(R[:, r, 1]) * X2[:, 1]) + c(R[:, r, 2]) * X2[:, 2]) + c(t[:, r])
             for r in range(3)]
        Q = [c(i_s) * ((c(R[:, 0, r]) * X1[:, 0] + c(R[:, 1, r]) * X1[:, 1]) + c(R[:, 2, r]) * X1[:, 2]) + c(ti[:, r])
             for r in range(3)]
        e12 = np.stack([obs1[:, 0] - ((P[0] / P[2]) * K1[0] + K1[2]), obs1[:, 1] - ((P[1] / P[2]) * K1[1] + K1[3])], 2)
        e21 = np.stack([obs2[:, 0] - ((Q[0] / Q[2]) * K2[0] + K2[2]), obs2[:, 1] - ((Q[1] / Q[2]) * K2[1] + K2[3])], 2)
    return e12, e21


def pair_errors(state, X1, X2, obs1, obs2, K1, K2):
    """e12 [N][2], e21 [N][2]."""
    e12, e21 = pair_errors_multi([state], X1, X2, obs1, obs2, K1, K2)
    return e12[0], e21[0]


def edge_errors_multi(states, pb):
    """e [S][2N][2] in edge order (edge 2c = e12 of correspondence c, 2c + 1 = its e21)."""
    e12, e21 = pair_errors_multi(states, pb["X1"], pb["X2"], pb["obs1"], pb["obs2"], pb["K1"], pb["K2"])
    e = np.empty((len(states), 2 * e12.shape[1], 2))
    e[:, 0::2], e[:, 1::2] = e12, e21
    return e


def edge_errors(state, pb):
    """All 2N edge errors of one state: e [2N][2]."""
    return edge_errors_multi([state], pb)[0]


def chi2_of(e, w):
    with np.errstate(all="ignore"):
        return w * (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1])


def numeric_jacobian(state, pb, fix_scale, delta=DELTA, libm_nudge=0):
    """O6: J [2N][2][7] by central differences through the update."""
    states = []
    for k in range(7):
        for d in (delta, -delta):
            x = np.zeros(7)
            x[k] = d
            states.append(sim3_update(state, x, fix_scale, libm_nudge))
    e = edge_errors_multi(states, pb)
    with np.errstate(all="ignore"):
        scale = 1.0 / (2.0 * delta)
        return np.stack([(e[2 * k] - e[2 * k + 1]) * scale for k in range(7)], 2)


# ---- the optimisation (O7, O8) -----------------------------------------------------------------------------------------
def optimize(state, pb, active, budget, fix_scale, delta_huber, order, libm_nudge, out):
    """optimize(budget) over the edges of the active correspondences; returns the kept state."""
    n_edges = 2 * len(pb["X1"])
    w = pb["w"]
    edge_active = np.repeat(active, 2)
    act = order[edge_active[order]]
    use_kernel = np.ones(n_edges, bool)

    def robust_chi(st):
        r0, _ = huber(chi2_of(edge_errors(st, pb), w), delta_huber, use_kernel)
        return float(seq_sum(r0, act))

    lam, nu = 0.0, 2.0
    for it in range(budget):
        e = edge_errors(state, pb)
        r0, r1 = huber(chi2_of(e, w), delta_huber, use_kernel)
        cur = float(seq_sum(r0, act))
        J = numeric_jacobian(state, pb, fix_scale, DELTA, libm_nudge)
        with np.errstate(all="ignore"):
            s = w * r1
            Jw = J * s[:, None, None]
            contrib = np.zeros((n_edges, 35))
            for k, (a, b_) in enumerate(TRI):
                contrib[:, k] = Jw[:, 0, a] * J[:, 0, b_] + Jw[:, 1, a] * J[:, 1, b_]
            for a in range(7):
                contrib[:, 28 + a] = -(Jw[:, 0, a] * e[:, 0] + Jw[:, 1, a] * e[:, 1])
            tot = seq_sum(contrib, act)
        H = np.zeros((7, 7))
        for k, (a, b_) in enumerate(TRI):
            H[a, b_] = H[b_, a] = tot[k]
        b = tot[28:35].copy()
        if it == 0:
            m = 0.0
            for a in range(7):
                if abs(H[a, a]) > m:
                    m = abs(H[a, a])
            lam, nu = 1e-5 * m, 2.0
        rho, trial, stop = 0.0, 0, False
        out["iterations"] += 1
        while True:
            ok, x = cholesky_solve(H, lam, b)
            cand = sim3_update(state, x, fix_scale, libm_nudge)
            tmp = robust_chi(cand)
            if not ok:
                tmp = DBL_MAX
            with np.errstate(all="ignore"):
                scale = 0.0
                for a in range(7):
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
                state, cur = cand, tmp
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
    return state


def optimize_core(pb, state0, th2, fix_scale, order=None, libm_nudge=0):
    """O7-O8 over widened inputs.  pb: X1, X2 [N][3], obs1, obs2 [N][2], w [2N] (edge order), K1, K2 as float64.
    Returns a dict: state, n_bad, n_inliers, stages, iterations, trials, margin, cleared [N] bool."""
    N = len(pb["X1"])
    th2f = np.float32(th2)
    th2d = np.float64(th2f)
    delta_huber = np.float64(np.sqrt(th2f))
    order = np.arange(2 * N) if order is None else np.asarray(order)
    out = dict(state=state0, n_bad=0, n_inliers=0, stages=0, iterations=0, trials=0, margin=np.inf,
               cleared=np.zeros(N, bool))
    if N == 0:
        return out
    active = np.ones(N, bool)

    def classify(st):
        c = chi2_of(edge_errors(st, pb), pb["w"])
        with np.errstate(all="ignore"):
            bad = ((c[0::2] > th2d) | (c[1::2] > th2d)) & active
            mg = np.abs(c / th2d - 1.0)[np.repeat(active, 2)]
        mg = mg[np.isfinite(mg)]
        if len(mg):
            out["margin"] = min(out["margin"], float(mg.min()))
        return bad

    state = optimize(state0, pb, active, 5, fix_scale, delta_huber, order, libm_nudge, out)
    bad = classify(state)
    out["n_bad"], out["stages"] = int(bad.sum()), 1
    active &= ~bad
    out["cleared"] |= bad
    if N - out["n_bad"] < 10:
        return out
    state = optimize(state, pb, active, 10 if out["n_bad"] > 0 else 5, fix_scale, delta_huber, order, libm_nudge, out)
    bad = classify(state)
    out["cleared"] |= bad
    out["n_inliers"] = int((active & ~bad).sum())
    out["state"], out["stages"] = state, 2
    return out


def prepare(pr):
    """O1-O3: the correspondences and their widened records from a problem dict (the arrays as the ABI takes them)."""
    n1 = len(pr["valid"])
    nl = int(pr.get("nlevels", len(pr["inv_level_sigma2"])))
    o1, o2 = np.asarray(pr["octave1"], np.int64), np.asarray(pr["octave2"], np.int64)
    valid = np.asarray(pr["valid"]) != 0
    in_range = (o1 >= 0) & (o1 < nl) & (o2 >= 0) & (o2 < nl)
    idx = np.flatnonzero(valid & in_range)
    sg = np.asarray(pr["inv_level_sigma2"], np.float32)
    w = np.empty(2 * len(idx))
    w[0::2], w[1::2] = sg[o1[idx]].astype(np.float64), sg[o2[idx]].astype(np.float64)
    f64 = np.float64
    return {"n1": n1, "idx": idx, "n_bad_index": int((valid & ~in_range).sum()),
            "X1": rt_apply(pr["T1w"], np.asarray(pr["Xw1"], np.float32).reshape(n1, 3)[idx]).astype(f64),
            "X2": rt_apply(pr["T2w"], np.asarray(pr["Xw2"], np.float32).reshape(n1, 3)[idx]).astype(f64),
            "obs1": np.asarray(pr["kp1_xy"], np.float32).reshape(n1, 2)[idx].astype(f64),
            "obs2": np.asarray(pr["kp2_xy"], np.float32).reshape(n1, 2)[idx].astype(f64), "w": w,
            "K1": tuple(f64(np.float32(k)) for k in pr["K1"]), "K2": tuple(f64(np.float32(k)) for k in pr["K2"])}


def outputs_of(state, T2w):
    """O9 from a state."""
    q, t, s = state
    Rd = quat_to_matrix(q)
    with np.errstate(all="ignore"):
        return {"R12_d": Rd, "t12_d": np.array(t, np.float64), "s12_d": np.float64(s), "R12": Rd.astype(np.float32),
                "t12": np.asarray(t).astype(np.float32), "s12": np.float32(s), "T12": to_cvmat(state),
                "Scw": scw_of(state, T2w)}


def optimize_sim3(pr, order=None, libm_nudge=0):
    """The definition.  pr: valid, Xw1, Xw2, octave1, octave2, kp1_xy, kp2_xy, T1w, T2w, K1, K2, inv_level_sigma2, R12, t12,
    s12, th2, fix_scale.  order: a permutation of the 2N edges for the sums.  Returns a dict: the O9 outputs,
    n_correspondences, n_bad, n_inliers, stages, iterations, trials, n_bad_index, inlier (uint8 [n1], 255 = not a
    correspondence: untouched), margin (least |chi2 / th2 - 1| over all classifications)."""
    pb = prepare(pr)
    state0 = state_from_floats(pr["R12"], pr["t12"], pr["s12"])
    r = optimize_core(pb, state0, pr["th2"], bool(pr["fix_scale"]), order, libm_nudge)
    out = outputs_of(r["state"], pr["T2w"])
    inlier = np.full(pb["n1"], 255, np.uint8)
    inlier[pb["idx"]] = (~r["cleared"]).astype(np.uint8)
    out.update(n_correspondences=len(pb["idx"]), n_bad=r["n_bad"], n_inliers=r["n_inliers"], stages=r["stages"],
               iterations=r["iterations"], trials=r["trials"], n_bad_index=pb["n_bad_index"], inlier=inlier,
               margin=r["margin"])
    return out


# ---- scenes ------------------------------------------------------------------------------------------------------------
def make_scene(n, seed, fix_scale=False, outlier_frac=0.3, n1=None, noise_px=0.7, rot_sigma=0.01, trans_sigma=0.02,
               scale_sigma=0.02):
    """A seeded loop candidate on sim3_model.make_scene's key-frame pair: n correspondences scattered over n1 rows, the
    observations the (noisy) own-image projections of the two map points, a share of gross outliers >= 50 px off in image 1,
    th2 = 10 (LoopClosing.cc:327); the start is the planted Sim3 perturbed by about rot_sigma rad, trans_sigma m and
    scale_sigma (relative; the scale stays 1 with fix_scale)."""
    b = sim3_model.make_scene(n, seed, n1=n1, n_hyp=1, fix_scale=fix_scale, outlier_frac=outlier_frac, noise_px=noise_px)
    rng = np.random.default_rng(77_000 + seed)
    n1 = len(b["valid"])
    kp1 = sim3_model.to_image(b["K1"], rt_apply(b["T1w"], b["Xw1"]))
    kp2 = sim3_model.to_image(b["K2"], rt_apply(b["T2w"], b["Xw2"]))
    tr = b["true"]
    R0 = sim3_model._rot(rng, rot_sigma) @ tr["R"]
    t0 = tr["t"] + rng.normal(0, trans_sigma, 3)
    s0 = 1.0 if fix_scale else tr["s"] * (1.0 + rng.normal(0, scale_sigma))
    return {"valid": b["valid"], "Xw1": b["Xw1"], "Xw2": b["Xw2"], "octave1": b["octave1"], "octave2": b["octave2"],
            "kp1_xy": kp1, "kp2_xy": kp2, "T1w": b["T1w"], "T2w": b["T2w"], "K1": b["K1"], "K2": b["K2"],
            "inv_level_sigma2": INV_LEVEL_SIGMA2.copy(), "R12": R0.astype(np.float32), "t12": t0.astype(np.float32),
            "s12": np.float32(s0), "th2": np.float32(TH2), "fix_scale": bool(fix_scale), "true": tr,
            "outlier": b["outlier"] & (b["valid"] != 0), "n": n, "n1": n1}


LDS_PAIRS = 768  # correspondences a workgroup keeps in LDS (SO_LDS_PAIRS in csrc/sim3_opt.hip)
PARITY_SIZES = (1, 9, 10, 11, 63, 64, 65, 255, 256, 257, 300, LDS_PAIRS + 1)


def _parity_scenes():
    """The committed scenes of the device parity test: every size x fix_scale with n1 > N and scattered invalid rows, two
    scenes without outliers (the 5-iteration second stage), one whose first stage leaves fewer than 10, one with octaves
    out of range.  (name, scene) pairs; tests/test_sim3opt_model.py asserts that each has margin >= 1e-6."""
    sc = []
    for n in PARITY_SIZES:
        for fs in (False, True):
            clean = n in (10, 11) and not fs  # exactly 10 and 11 left after stage 1: the second stage runs
            sc.append(("n%d_fix%d" % (n, fs), make_scene(n, 3000 + 2 * n + fs, fix_scale=fs, outlier_frac=0.0 if clean else 0.3,
                                                         noise_px=0.2 if clean else 0.7)))
    sc.append(("clean_40", make_scene(40, 4001, outlier_frac=0.0, noise_px=0.1)))
    sc.append(("clean_130_fix", make_scene(130, 4002, fix_scale=True, outlier_frac=0.0, noise_px=0.1)))
    sc.append(("few_left", make_scene(16, 4003, outlier_frac=0.6)))
    s = make_scene(90, 4004)
    v = np.flatnonzero(s["valid"])
    s["octave1"] = s["octave1"].copy()
    s["octave2"] = s["octave2"].copy()
    s["octave1"][v[3]], s["octave2"][v[10]], s["octave1"][v[20]], s["octave2"][v[20]] = NLEVELS, -1, 1 << 20, -7
    sc.append(("bad_octaves", s))
    return sc


PARITY_SCENES = _parity_scenes()


def state_deviation(a, b):
    """Largest entry-wise deviation of (R12_d, t12_d, s12_d) between two results."""
    with np.errstate(all="ignore"):
        return max(float(np.abs(a["R12_d"] - b["R12_d"]).max()), float(np.abs(a["t12_d"] - b["t12_d"]).max()),
                   float(abs(a["s12_d"] - b["s12_d"])))


DISCRETE = ("n_correspondences", "n_bad", "n_inliers", "stages", "n_bad_index")


def model_spread(sc, base, n_perm=8, seed=0):
    """The model's own spread on a scene: the largest state deviation over n_perm seeded permutations of the edge order plus
    the two runs libm_nudge = +-1, and how many of those runs changed a discrete output."""
    rng = np.random.default_rng(10_000 + seed)
    runs = [optimize_sim3(sc, order=rng.permutation(2 * base["n_correspondences"])) for _ in range(n_perm)]
    runs += [optimize_sim3(sc, libm_nudge=-1), optimize_sim3(sc, libm_nudge=1)]
    dev, flips = 0.0, 0
    for r in runs:
        dev = max(dev, state_deviation(r, base))
        flips += int(any(r[k] != base[k] for k in DISCRETE) or not np.array_equal(r["inlier"], base["inlier"]))
    return dev, flips
