"""NumPy float64 restatement of Optimizer::BundleAdjustment / GlobalBundleAdjustemnt (Optimizer.cc:41-237): the oracle of
the device bundle adjustment (orbgpu_bundle_adjustment*).

One optimize(n_iterations) of lba_model.py's Levenberg-Marquardt loop over every key frame and every point of a map: no
classification, no second round, no erase.  The pieces (edge errors, Jacobians, the sequential sums, the 3x3 inverse, the
LL' solve, the vertex updates) are lba_model's and pose_model's; the loop is restated here because lba_model.local_ba
is not edited and runs two rounds.  tests/test_ba_model.py pins this loop to lba_model.local_ba(stop_between=True) bit for
bit.  The definition (B1-B7) is in include/orbgpu.h above orbgpu_bundle_adjustment_device; g2o boundary unpinned.
"""
import numpy as np

from lba_model import TRI3, TRI6, _inv3_all, _llt_solve_fast, edge_errors, point_jacobian, point_update, seg_sum, seq_total
from pose_model import (DBL_MAX, chi2_of, huber, jacobian, pose_from_Tcw, pose_matrix, pose_update, quat_to_matrix)

HUBER_CHI2 = (5.99, 7.815)  # Optimizer.cc:85, :131: thHuber2D = sqrt(5.99), not LocalBundleAdjustment's 5.991
MAX_ITERATIONS = 100


def deltas(huber_chi2=HUBER_CHI2):
    """(mono, stereo) Huber deltas: g2o takes the float of Optimizer.cc's `const float thHuber2D = sqrt(5.99)`."""
    return tuple(np.float64(np.float32(np.sqrt(c))) for c in huber_chi2)


def bundle_adjustment(pr, n_iterations, robust=True, order=None, stop_before=False, huber_chi2=HUBER_CHI2):
    """The definition.  pr: dict as lba_model.local_ba takes it, except that `fixed` has one entry per pose row (n_local is
    not read): Tcw [P][4][4] float32, fixed [P], cam [P][5], inv_sigma2 [P][nlevels], world_pos [M][3], e_point / e_pose /
    e_oct [E], e_xy [E][2], e_ur [E].

    Returns a dict: Tcw_d [P][4][4], Tcw (float32), pos_d [M][3], pos (float32), not_included (uint8 [M]), n_edges,
    n_not_included, iterations, trials, chi2_start, chi2_end, stopped, n_bad_index, trace (the accept / reject decisions)
    and rel_change (per trial, |chi2 - the trial's chi2| / chi2: how far each decision was from a tie).  With stop_before
    only the counters are returned."""
    Tcw = np.asarray(pr["Tcw"], np.float32).reshape(-1, 4, 4)
    Pn = len(Tcw)
    fixed = np.asarray(pr["fixed"], np.uint8).astype(bool).reshape(-1)[:Pn]
    cam = np.asarray(pr["cam"], np.float32).reshape(Pn, 5).astype(np.float64)
    inv_sigma2 = np.asarray(pr["inv_sigma2"], np.float32).reshape(Pn, -1)
    nlevels = inv_sigma2.shape[1]
    X = np.asarray(pr["world_pos"], np.float32).reshape(-1, 3).astype(np.float64)
    Mn = len(X)
    e_point, e_pose, e_oct = (np.asarray(pr[k], np.int64) for k in ("e_point", "e_pose", "e_oct"))
    e_xy, e_ur = np.asarray(pr["e_xy"], np.float32).reshape(-1, 2), np.asarray(pr["e_ur"], np.float32)
    bad_index = (e_point < 0) | (e_point >= Mn) | (e_pose < 0) | (e_pose >= Pn) | (e_oct < 0) | (e_oct >= nlevels)
    valid = np.flatnonzero(~bad_index)
    ne = len(valid)
    free_of = np.full(Pn, -1, np.int64)  # pose row -> slot in the reduced system
    free_rows = np.flatnonzero(~fixed) if Pn else np.zeros(0, np.int64)
    free_of[free_rows] = np.arange(len(free_rows))
    nf = len(free_rows)

    ed = {"point": e_point[valid], "pose": e_pose[valid]}
    ed["stereo"] = ~(e_ur[valid] < 0)
    ed["obs"] = np.concatenate([e_xy[valid].astype(np.float64), e_ur[valid].astype(np.float64)[:, None]], 1)
    ed["w"] = inv_sigma2[ed["pose"], e_oct[valid]].astype(np.float64)
    ed["K"] = tuple(cam[ed["pose"], k] for k in range(5))
    ed["free"] = free_of[ed["pose"]]
    d_mono, d_stereo = deltas(huber_chi2)
    delta = np.where(ed["stereo"], d_stereo, d_mono)
    use_kernel = np.full(ne, bool(robust))
    order = np.arange(ne) if order is None else np.asarray(order)

    pt_on = np.zeros(Mn, bool)
    pt_on[ed["point"]] = True
    out = dict(n_edges=ne, n_bad_index=int(bad_index.sum()), n_not_included=int((~pt_on).sum()), iterations=0, trials=0,
               chi2_start=0.0, chi2_end=0.0, stopped=0, trace=[], rel_change=[])
    if stop_before:
        out["stopped"] = 1
        return out
    out["not_included"] = (~pt_on).astype(np.uint8)

    qs, ts = [], []
    for i in range(Pn):
        q, t = pose_from_Tcw(Tcw[i])
        qs.append(q)
        ts.append(t)
    qs, ts = np.array(qs).reshape(Pn, 4), np.array(ts).reshape(Pn, 3)

    def rotations(q_):
        return np.array([quat_to_matrix(q) for q in q_]).reshape(Pn, 3, 3)

    # the terms of the Schur complement's lower block triangle, in `order` (lba_model.local_ba)
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

    act = order
    fr_on = np.zeros(nf, bool)
    fr_on[ed["free"][act][ed["free"][act] >= 0]] = True
    act_free = act[ed["free"][act] >= 0]
    pair_order = np.arange(len(p1))

    def robust_chi(q_, t_, X_):
        e_, _ = edge_errors(rotations(q_), t_, X_, ed)
        r0, _ = huber(chi2_of(e_, ed["w"]), delta, use_kernel)
        return seq_total(r0[act])

    lam, nu = 0.0, 2.0
    cur = robust_chi(qs, ts, X)
    out["chi2_start"] = cur
    for it in range(int(n_iterations)):
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
        out["iterations"] += 1
        while True:
            with np.errstate(all="ignore"):
                inv = np.zeros((Mn, 3, 3))
                inv[pt_on] = _inv3_all(Hll[pt_on], lam)
                ie = inv[ed["point"]]
                Y = np.zeros((ne, 6, 3))  # Hpl Hll^-1
                for a in range(6):
                    for c in range(3):
                        Y[:, a, c] = (Hpl[:, a, 0] * ie[:, 0, c] + Hpl[:, a, 1] * ie[:, 1, c]) + Hpl[:, a, 2] * ie[:, 2, c]
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
                                blk = np.eye(6)  # a free pose without an edge: x = 0, coupled to nothing
                        S[6 * fa:6 * fa + 6, 6 * fb:6 * fb + 6] = blk
                gy = np.zeros((ne, 6))
                ble = bl[ed["point"]]
                for a in range(6):
                    gy[:, a] = (Y[:, a, 0] * ble[:, 0] + Y[:, a, 1] * ble[:, 1]) + Y[:, a, 2] * ble[:, 2]
                g = bp - seg_sum(gy, ed["free"], nf, act_free)
                g[~fr_on] = 0.0
                ok, xp = _llt_solve_fast(S, g.ravel())
                xp = xp.reshape(nf, 6)
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
            out["trials"] += 1
            with np.errstate(all="ignore"):
                out["rel_change"].append(float(abs(cur - tmp) / cur))
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
    out["chi2_end"] = cur
    out["Tcw_d"] = np.array([pose_matrix(qs[i], ts[i]) for i in range(Pn)]).reshape(Pn, 4, 4)
    out["Tcw"] = out["Tcw_d"].astype(np.float32)
    out["pos_d"] = X
    with np.errstate(all="ignore"):
        out["pos"] = X.astype(np.float32)
    return out


def permutation_spread(pr, base, n_iterations, robust=True, n_perm=4, seed=0, huber_chi2=HUBER_CHI2):
    """Over n_perm seeded permutations of the summation order: the largest deviation of the poses and of the points from
    `base`, and whether the accept / reject trace stayed the same."""
    rng = np.random.default_rng(10_000 + seed)
    dev_T, dev_X, same = 0.0, 0.0, True
    for _ in range(n_perm):
        r = bundle_adjustment(pr, n_iterations, robust=robust, order=rng.permutation(base["n_edges"]), huber_chi2=huber_chi2)
        same = same and r["trace"] == base["trace"]
        with np.errstate(all="ignore"):
            dT, dX = np.abs(r["Tcw_d"] - base["Tcw_d"]), np.abs(r["pos_d"] - base["pos_d"])
        dev_T = max(dev_T, float(np.nanmax(dT)) if dT.size and not np.isnan(dT).all() else 0.0)
        dev_X = max(dev_X, float(np.nanmax(dX)) if dX.size and not np.isnan(dX).all() else 0.0)
    return dev_T, dev_X, same


def from_lba_scene(sc, all_free=False):
    """A scene of lba_model.make_scene as a bundle-adjustment problem: `fixed` per pose row, the local flags followed by
    ones for the fixed cameras (all_free: no fixed row at all)."""
    pr = dict(sc)
    Pn, nl = len(sc["Tcw"]), int(sc["n_local"])
    fixed = np.ones(Pn, np.uint8)
    fixed[:nl] = np.asarray(sc["fixed"], np.uint8)
    pr["fixed"] = np.zeros(Pn, np.uint8) if all_free else fixed
    return pr


# ---- the graph gathering (Optimizer.cc:68-184) ------------------------------------------------------------------------
def gather_all(mp, vp_kfs=None, vp_mps=None):
    """The problem of a map as OptimizerT::BundleAdjustment builds it, over the map format of lba_model.gather (kfs: id,
    bad, K, Tcw, inv_sigma2, kps, mps; mps: id, bad, pos, obs).  vp_kfs / vp_mps: indices of the key frames and points
    handed in, by default all in list order.  Pose rows are the key frames that are not bad, point rows the points that
    are not bad; maxKFid is the largest id among the rows; per point the observations in index order (the reference's
    pointer order) without bad key frames and without ids above maxKFid; an observer that is in no row keeps its edge with
    pose -1.  Returns the problem dict of bundle_adjustment plus kf_rows, points (indices), edge_kf / edge_mp."""
    kfs, mps = mp["kfs"], mp["mps"]
    vp_kfs = list(range(len(kfs))) if vp_kfs is None else list(vp_kfs)
    vp_mps = list(range(len(mps))) if vp_mps is None else list(vp_mps)
    kf_rows = [k for k in vp_kfs if not kfs[k]["bad"]]
    points = [m for m in vp_mps if not mps[m]["bad"]]
    max_id = max([kfs[k]["id"] for k in kf_rows], default=0)
    rows = {k: i for i, k in enumerate(kf_rows)}
    nlevels = max(1, min(len(kfs[kf_rows[0]]["inv_sigma2"]), 8)) if kf_rows else 1
    sig = np.zeros((len(rows), nlevels), np.float32)
    for k, i in rows.items():
        s = np.asarray(kfs[k]["inv_sigma2"], np.float32)[:nlevels]
        sig[i, :len(s)] = s
    e = {k: [] for k in ("point", "pose", "oct", "xy", "ur", "kf", "mp")}
    for j, m in enumerate(points):
        for k in sorted(mps[m]["obs"]):
            if kfs[k]["bad"] or kfs[k]["id"] > max_id:
                continue
            x, y, ur, octave = kfs[k]["kps"][mps[m]["obs"][k]]
            e["point"].append(j), e["pose"].append(rows.get(k, -1)), e["kf"].append(k), e["mp"].append(m)
            e["oct"].append(int(octave) if 0 <= int(octave) < len(kfs[k]["inv_sigma2"]) else -1)
            e["xy"].append((x, y)), e["ur"].append(ur)
    return dict(Tcw=np.array([kfs[k]["Tcw"] for k in kf_rows], np.float32).reshape(-1, 4, 4),
                fixed=np.array([kfs[k]["id"] == 0 for k in kf_rows], np.uint8),
                cam=np.array([kfs[k]["K"] for k in kf_rows], np.float32).reshape(-1, 5), inv_sigma2=sig,
                world_pos=np.array([mps[m]["pos"] for m in points], np.float32).reshape(-1, 3),
                e_point=np.array(e["point"], np.int32), e_pose=np.array(e["pose"], np.int32), e_oct=np.array(e["oct"], np.int32),
                e_xy=np.array(e["xy"], np.float32).reshape(-1, 2), e_ur=np.array(e["ur"], np.float32),
                kf_rows=kf_rows, points=points, edge_kf=e["kf"], edge_mp=e["mp"], max_kf_id=max_id)
